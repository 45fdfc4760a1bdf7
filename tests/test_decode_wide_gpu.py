"""The wide decode GEMMs (vp_decode_gemm_wide / _w8_wide / _w4_wide, 17 <= M <= 64) and generate() at more than 16 sequences.

The contract is equality, not a bound: output row m of a wide call is the parent entry point's result for that row inside a 16-row slice of
A (ops.decode_gemm(..., wide=False) makes exactly those parent calls), bit for bit, on Gaussian operands (where any change of the summation
order shows) and on the exact integer draws of tests/decode_cases.py (where the value itself is known).  A session of 20 or 33 sequences
then returns the same tokens and logits on either route, in every weight and cache format, eager and captured; the only bounded comparison
is the teacher-forced one against the training forward (2e-2, test_generate_gpu's bound)."""
import pytest
import torch

import decode_cases as DC
import parity

pytestmark = pytest.mark.gpu
WIDE_MS = (17, 32, 33, 48, 49, 64)
# one K per kind that ends in a partial chunk (DC.K_TABLE), at N = DC.GEMM_N (a tail tile of 8 rows)
PARTIAL_K = dict(bf16=2064, w8=4656, w4=4640)
GAUSS = dict(bf16="gaussbf", w8="gauss8", w4="gauss4")
EXACT = dict(bf16="w8", w8="w8", w4="w4")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops as o
    return o


def run_gemm(ops, c, ko, wide, epi=DC.EPI_NONE, norm=False):
    out = DC.out_box(c, "bf16" if epi else ko, c.N // 2 if epi else None)
    kw = {}
    if c.kind == "w8":
        kw["w_scale"] = c.s8
    elif c.kind == "w4":
        kw["w_block_scale"] = c.e.view
    ops.decode_gemm(c.a.view, c.w.view, residual=c.res.view if ko == "res" else None, norm_w=c.gamma.view[0] if norm else None, eps=c.inp.eps,
                    epi=epi, out=out.view, wide=wide, **kw)
    return out


def wide_equals_parent(ops, c, ko, epi=DC.EPI_NONE, norm=False, want=None):
    tag = (c.kind, c.M, c.N, c.K, ko, epi, norm)
    got = run_gemm(ops, c, ko, None, epi, norm)
    ref = run_gemm(ops, c, ko, False, epi, norm)                  # the parent entry point on every 16-row slice
    assert ref.outside_intact() and got.outside_intact(), tag
    for m0 in range(0, c.M, 16):
        assert DC.bits_equal(got.view[m0:m0 + 16], ref.view[m0:m0 + 16]), (tag, m0, (got.view != ref.view).nonzero()[:4].tolist())
    again = run_gemm(ops, c, ko, None, epi, norm)
    assert DC.bits_equal(again.view, got.view), tag
    if want is not None:
        assert torch.equal(got.view, want), (tag, (got.view != want).nonzero()[:4].tolist())
    assert DC.inputs_unchanged(c), tag


# ================================================================================================ 1. kernel against parent
@pytest.mark.parametrize("M", WIDE_MS)
@pytest.mark.parametrize("kind", DC.KERNELS)
def test_wide_gemm_equals_parent_on_every_slice(ops, kind, M):
    """N = 136 at a K that ends in a partial chunk, the single clamped tile, and the split-K shapes; strided operands in sentinel boxes;
    plain bf16, fp32 out, residual, each with and without the norm prologue"""
    shapes = [(DC.GEMM_N, PARTIAL_K[kind]), DC.ONE_TILE] + DC.SWIGLU_SHAPES
    for N, K in shapes:
        assert (ops.decode_gemm_ws_bytes(M, N, K, w8=kind == "w8", w4=kind == "w4") > 0) == ((N, K) in DC.SWIGLU_SHAPES)
        inp = DC.gemm_inputs(GAUSS[kind], M, N, K)
        c = DC.gemm_call(kind, inp, strided=True, device="cuda")
        for ko in ("bf16", "f32", "res"):
            wide_equals_parent(ops, c, ko)
        for ko in ("bf16", "res") if N == DC.GEMM_N else ("f32",):
            wide_equals_parent(ops, c, ko, norm=True)
        # the exact draw: the value itself, whatever the order
        inp = DC.gemm_inputs(EXACT[kind], M, N, K)
        want = {k: v.cuda() for k, v in DC.exact_outputs(inp).items()}
        c = DC.gemm_call(kind, inp, strided=True, device="cuda")
        for ko in ("bf16", "f32", "res"):
            wide_equals_parent(ops, c, ko, want=want[ko])


@pytest.mark.parametrize("M", WIDE_MS)
@pytest.mark.parametrize("kind", DC.KERNELS)
def test_wide_gemm_swiglu_equals_parent_under_split_k(ops, kind, M):
    """SwiGLU on the interleaved and the halves layout at ks > 1 (the combine kernel applies it), with and without the norm prologue"""
    for N, K in DC.SWIGLU_SHAPES:
        for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
            assert ops.decode_gemm_ws_bytes(M, N, K, epi, w8=kind == "w8", w4=kind == "w4") == DC.SWIGLU_KS[kind][K] * M * N * 4
            inp = DC.gemm_inputs(GAUSS[kind], M, N, K, seed=epi)
            c = DC.gemm_call(kind, inp, strided=True, device="cuda", ncols=N // 2)
            for norm in (False, True):
                wide_equals_parent(ops, c, "bf16", epi=epi, norm=norm)


@pytest.mark.parametrize("kind", DC.KERNELS)
def test_wide_gemm_swiglu_in_the_kernel_epilogue(ops, kind):
    """ks = 1 (K = 2592 admits no split): SwiGLU stored by the wide kernel's own epilogue, per A tile"""
    N, K = 256, 2592
    for M in (17, 40, 64):
        for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
            assert ops.decode_gemm_ws_bytes(M, N, K, epi, w8=kind == "w8", w4=kind == "w4") == 0
            c = DC.gemm_call(kind, DC.gemm_inputs(GAUSS[kind], M, N, K, seed=epi), strided=True, device="cuda", ncols=N // 2)
            wide_equals_parent(ops, c, "bf16", epi=epi, norm=True)
            wide_equals_parent(ops, c, "bf16", epi=epi)


# ================================================================================================ 2. routing
def test_routing_by_m(ops, monkeypatch):
    from visper_lm_amd import _lib
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    g = torch.Generator(device="cuda").manual_seed(3)
    N, K = 256, 1024                                             # splits K: the combine belongs to the entry point, not to the host
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    q8, s8 = ops.quant_rows_e4m3(w)
    q4, e4 = ops.quant_blocks_mxfp4(w)
    for parent, wt, kw in (("vp_decode_gemm", w, {}), ("vp_decode_gemm_w8", q8, dict(w_scale=s8)), ("vp_decode_gemm_w4", q4, dict(w_block_scale=e4))):
        a = torch.randn(40, K, device="cuda", generator=g).to(torch.bfloat16)
        del names[:]
        o16 = ops.decode_gemm(a[:16], wt, **kw)
        assert names == [parent]
        del names[:]
        o16f = ops.decode_gemm(a[:16], wt, wide=False, **kw)
        assert names == [parent] and DC.bits_equal(o16, o16f)
        del names[:]
        o40 = ops.decode_gemm(a, wt, **kw)
        assert names == [parent + "_wide"]
        del names[:]
        o40f = ops.decode_gemm(a, wt, wide=False, **kw)
        assert names == [parent] * 3
        assert DC.bits_equal(o40, o40f) and DC.bits_equal(o40[:16], o16)
    with pytest.raises(ValueError, match="at most 64"):
        ops.decode_gemm(torch.zeros(65, K, device="cuda", dtype=torch.bfloat16), w)


# ================================================================================================ 3. sessions of 20 sequences, tiny models
B20 = 20


def _tiny_engine(arch, quantize=None):
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.engine import Engine
    ocfg, W, batch, g = cases.tiny_llama_case(arch)
    eng = Engine(VisperConfig(**vars(ocfg)))
    eng.load_weights(W)
    if quantize:
        eng.quantize_decoder(fmt=quantize)
    return eng, batch


def _ragged_with_image(batch, B=B20):
    """B prompts from the case's two rows, each with its own number of leading text tokens dropped (the <image> token stays), left-padded as
    the eval scripts' tokenizers pad -> (ids [B, T], mask [B, T], images [B, 3, h, w])"""
    src, T = batch["input_ids"], batch["input_ids"].shape[1]
    first_image = int((src[0] < 0).nonzero()[0])
    ids = torch.zeros(B, T, dtype=torch.long)
    am = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        drop = (5 * b) % min(first_image, 12)
        ids[b, drop:] = src[b % 2, drop:]
        am[b, drop:] = 1
    assert len({int(x) for x in am.sum(1)}) > 4
    return ids, am, batch["images"][torch.arange(B) % 2].cuda()


def _session(eng, ids, am, images, N, wide, kv=None, graph=False):
    """N greedy tokens [B, N] and the fp32 logits each was chosen from, on one route of the step's GEMMs"""
    from visper_lm_amd import decode
    sess = decode.DecodeSession(eng, kv)
    sess.wide_gemm = wide
    sess.use_graph = graph
    toks, kept = [], []
    with torch.no_grad():
        logits = sess.prefill(ids, am, images, None, N)
        for i in range(N):
            if i:
                logits = sess.step(tok)
            kept.append(logits.clone())
            tok = torch.argmax(logits, -1)
            toks.append(tok)
    assert sess.replays == (N - 1 if graph else 0)
    sess.graph = None
    return torch.stack(toks, 1).cpu(), kept


def _same(x, y):
    return torch.equal(x[0], y[0]) and len(x[1]) == len(y[1]) and all(DC.bits_equal(a, b) for a, b in zip(x[1], y[1]))


def _calls(monkeypatch):
    from visper_lm_amd import _lib
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("fmt,kv", [(None, None), ("e4m3", None), ("mxfp4", None), ("mxfp4", "fp8_e4m3")])
@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_session_of_20_wide_equals_chunked(ops, monkeypatch, arch, fmt, kv):
    eng, batch = _tiny_engine(arch, fmt)
    ids, am, images = _ragged_with_image(batch)
    names = _calls(monkeypatch)
    wide = _session(eng, ids, am, images, 8, None, kv)
    gemm = {"e4m3": "vp_decode_gemm_w8", "mxfp4": "vp_decode_gemm_w4"}.get(fmt, "vp_decode_gemm")
    layers = eng.cfg.num_hidden_layers
    assert names.count(gemm + "_wide") >= 7 * 4 * layers and not [n for n in names if n in ("vp_decode_gemm", "vp_decode_gemm_w8", "vp_decode_gemm_w4")]
    del names[:]
    chunked = _session(eng, ids, am, images, 8, False, kv)
    assert names.count(gemm) >= 7 * 4 * layers * 2 and not [n for n in names if n.endswith("_wide")]
    assert wide[0].shape == (B20, 8) and _same(wide, chunked)


def test_session_of_20_captured_equals_eager(ops):
    eng, batch = _tiny_engine("llama", "mxfp4")
    ids, am, images = _ragged_with_image(batch)
    eager = _session(eng, ids, am, images, 8, None)
    assert _same(_session(eng, ids, am, images, 8, None, graph=True), eager)
    assert _same(_session(eng, ids, am, images, 8, False, graph=True), eager)


def test_generate_of_20_takes_the_wide_route_and_64_is_the_limit(ops, monkeypatch):
    from visper_lm_amd import decode
    eng, batch = _tiny_engine("llama")
    ids, am, images = _ragged_with_image(batch)
    names = _calls(monkeypatch)
    toks, kept, sess = decode.generate(eng, ids, am, images, None, max_new_tokens=3, return_logits=True)
    assert sess.wide_gemm is None and "vp_decode_gemm_wide" in names and "vp_decode_gemm" not in names
    want = _session(eng, ids, am, images, 3, False)
    assert torch.equal(toks.cpu(), want[0]) and all(DC.bits_equal(a, b) for a, b in zip(kept, want[1]))
    del names[:]
    with pytest.raises(ValueError, match="at most 64"):
        decode.generate(eng, ids[:1].repeat(65, 1), None, images[:1].repeat(65, 1, 1, 1), None, max_new_tokens=2)
    assert not names                                              # refused before the prefill


# ================================================================================================ 4. against the training forward
def test_session_of_20_teacher_forced_against_training_forward(ops):
    """First, a middle and the last sequence of the B = 20 session: the logits of every step against logits_of over that sequence's own
    prompt + generated tokens (test_generate_gpu._teacher_forced, its bound)"""
    eng, batch = _tiny_engine("llama")
    ids, am, images = _ragged_with_image(batch)
    N = 8
    toks, kept = _session(eng, ids, am, images, N, None)
    for b in (0, B20 // 2, B20 - 1):
        full = torch.cat([ids[b][am[b].bool()], toks[b]])[None]
        plan = eng.build_plan(full, None, None)
        x, *_ = eng._embed(images[b:b + 1], plan)
        dec = eng._decoder_fwd(x, plan, compute_grads=False)
        lg = eng.logits_of(dec["hidden"], plan)
        L = int(plan["lens_host"][0])
        worst = max(parity.max_rel(kept[i][b], lg[0, L - N - 1 + i]) for i in range(N))
        parity.check(f"teacher-forced decode logits tiny llama B = 20, sequence {b} (wide GEMMs)", worst, 2e-2)


# ================================================================================================ 5. full width
def test_full_width_llama_33_sequences_mxfp4_wide_equals_chunked(ops):
    from visper_lm_amd.config import llama3_8b
    from visper_lm_amd.engine import Engine
    eng = Engine(llama3_8b(num_hidden_layers=2, aux_mode="", num_task_tokens=0, vit_layers=1))
    eng.init_random(seed=1)
    eng.quantize_decoder(fmt="mxfp4")
    ids = torch.randint(0, 120000, (33, 300), generator=torch.Generator().manual_seed(3))
    wide = _session(eng, ids, None, None, 4, None)
    assert wide[0].shape == (33, 4) and _same(wide, _session(eng, ids, None, None, 4, False))
