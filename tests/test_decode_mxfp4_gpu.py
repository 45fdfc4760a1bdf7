"""MXFP4 weight-only decoding on the GPU: the block quantiser kernel against the CPU contract (quant.py), one-hot products that pin nibble
order, k permutation and scale indexing of the W4A16 skinny GEMM exactly, the GEMM against the fp32 product on the written-back weights
under the bf16 kernel's own bounds, the engine's 4-bit decode steps teacher-forced against the label-less forward on the same quantised
engine, mxfp4 vs bf16 greedy tokens, graph capture, staleness after an optimizer step, switching formats, and a record of what the format
itself costs against the un-quantised model."""
import functools
import warnings

import pytest
import torch

from parity import check, log, max_rel
from test_decode_fp8_gpu import _bf16_decode, _recompute_logits, _sd

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

QUANT_SHAPES = [(128, 32), (136, 96), (384, 128), (1000, 256), (64, 8192), (4096, 14336)]
# one block per row | N % 16 != 0, K no multiple of 64 | the tiny models' own (4 shapes) | (256, 1056): whole chunks plus one block, where a
# chunk is what ONE WAVE consumes per iteration, 512 k in this kernel (DG4_KCHUNK): waves 0 and 1 get a whole chunk each, wave 2 the single
# block | split-K over blocks | Phi-3 qkv, 96 blocks per row | Llama qkv | Llama down
GEMM_SHAPES = [(128, 32), (136, 96), (128, 128), (384, 128), (128, 256), (1000, 256), (256, 1056), (64, 8192), (9216, 3072), (6144, 4096),
               (4096, 14336)]


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops
    return ops


def _weight(N, K, g):
    """randn * 0.02 as the decode tests draw it, every BLOCK of 32 k times its own 2^-3 .. 2^3: the scales differ within a row (a kernel that
    indexes the scale bytes wrongly, or applies one scale to a whole row, fails)"""
    w = torch.randn(N, K // 32, 32, device="cuda", generator=g) * 0.02
    w = w * torch.exp2(torch.randint(-3, 4, (N, K // 32, 1), device="cuda", generator=g).float())
    return w.view(N, K).to(BF16)


def _ref_gemm(a, w):
    return a.float() @ w.float().t()


@functools.lru_cache(maxsize=None)
def _qweight(N, K, seed=0):
    """(written-back bf16 weight, codes, scale bytes) of one shape: quantised once, shared by the tests, never modified"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + N + K)
    w = _weight(N, K, g)
    q, e = ops.quant_blocks_mxfp4(w, writeback=True)
    if K > 32:
        assert (e.max(dim=1).values != e.min(dim=1).values).any(), "the scales must differ within a row"
    else:
        assert e.unique().numel() > 1
    return w, q, e


@pytest.fixture(scope="module", autouse=True)
def _release_shared_device_memory():
    """the shared weights and the shared engine hold several GB of device memory: give it back when this module is done"""
    yield
    _qweight.cache_clear()
    _shared_full_width_quantised_engine.cache_clear()
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ quantiser
def _special_rows(w, g):
    """the special rows of the host test's matrices: zeros, one huge outlier, bf16 subnormals with signs, the smallest subnormal alone"""
    K = w.shape[1]
    w[3] = 0
    w[5, 7] = 3.0e4
    sub = torch.randint(0, 128, (K,), device="cuda", generator=g) | (torch.randint(0, 2, (K,), device="cuda", generator=g) << 15)
    w[6] = sub.to(torch.int32).to(torch.int16).view(BF16)
    w[7] = 0
    w[7, 1] = torch.tensor([1], dtype=torch.int16).view(BF16)[0]
    return w


@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quant_blocks_kernel_matches_the_cpu_contract_exactly(N, K):
    ops = _ops()
    from visper_lm_amd import quant
    g = torch.Generator(device="cuda").manual_seed(N + K)
    w = _weight(N, K, g)
    if N in (384, 136):                                               # the special rows, through the kernel as well
        w = _special_rows(w, g)
    w0 = w.clone()
    q, e = ops.quant_blocks_mxfp4(w)
    assert q.shape == (N, K // 2) and e.shape == (N, K // 32) and q.dtype == e.dtype == torch.uint8
    assert torch.equal(w, w0), "without write-back the weight is read only"
    if K > 32:
        assert (e.max(dim=1).values != e.min(dim=1).values).any(), "the scales must differ within a row"
    q2, e2 = ops.quant_blocks_mxfp4(w, writeback=True)
    assert torch.equal(q, q2) and torch.equal(e, e2)
    q3, e3 = ops.quant_blocks_mxfp4(w0.clone())
    assert torch.equal(q, q3) and torch.equal(e, e3), "a second call gives identical output"
    wb, qh, eh, w0h = w.cpu(), q.cpu(), e.cpu(), w0.cpu()
    for r0 in range(0, N, 1024):                                      # the CPU reference in row blocks (float64 temporaries)
        r1 = min(N, r0 + 1024)
        qc, ec = quant.quantize_blocks_mxfp4(w0h[r0:r1])
        assert torch.equal(qh[r0:r1], qc), (N, K, r0)
        assert torch.equal(eh[r0:r1], ec), (N, K, r0)
        deq = quant.dequantize_mxfp4(qc, ec)
        assert torch.equal(wb[r0:r1].float(), deq), (N, K, r0)        # write-back == dequantize(...) exactly
        assert torch.equal(torch.signbit(wb[r0:r1]), torch.signbit(w0h[r0:r1])), "the sign survives, also on a zero"
    # quantising the written-back weights again changes nothing the GEMM sees
    if N * K <= 2 ** 24:
        q4, e4 = ops.quant_blocks_mxfp4(w.clone())
        assert torch.equal(quant.dequantize_mxfp4(q4.cpu(), e4.cpu()), wb.float())


# ------------------------------------------------------------------------------------------------ one-hot products: the layout, exactly
# (N, K): one partial chunk, scale rows unaligned | 4 whole chunks + a partial one (a wave's second, partial chunk), scale rows unaligned |
# 9 whole chunks (a wave's second and third chunk), 16-byte scale runs | split-K over 8 blocks
ONE_HOT_SHAPES = [(40, 160), (24, 2144), (32, 4608), (64, 8192)]


@pytest.mark.parametrize("N,K", ONE_HOT_SHAPES)
def test_decode_gemm_w4_one_hot_products_are_exact(N, K):
    """A row that is 1.0 at column k and 0 elsewhere must return W[n, k] itself, bit for bit: this pins the nibble order, the k permutation
    of both MFMA operands, the scale byte's index and the conversion's exactness for every code at scale bytes 97 .. 137."""
    ops = _ops()
    from visper_lm_amd import quant
    g = torch.Generator().manual_seed(K)
    codes = torch.randint(0, 16, (N, K), generator=g)
    codes[0, :16] = torch.arange(16)
    assert set(codes.unique().tolist()) == set(range(16))
    e = torch.randint(97, 138, (N, K // 32), generator=g).to(torch.uint8)
    e[0, 0], e[-1, -1] = 97, 137
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8).contiguous()
    want = quant.dequantize_mxfp4(q, e)                                            # [N, K] fp32
    ks = ops.decode_gemm_ws_bytes(1, N, K, w4=True) // (4 * N)
    cols = set(range(32)) | {0, 1, 15, 16, 31, 32, 33, 63, 64, 127, 128, K - 1}    # both nibbles, every position of a 16-byte load, block edges
    cols |= {K - 2, K - 32, K - 33}                                                # the last block's first code and its neighbours
    cols |= {512 + 5, 1024 + 38, 1536 + 71, 2048 + 4, 2048 + 101, 4096 + 9}        # the other waves' chunks, a wave's second and third chunk
    if ks > 1:
        Kc = K // ks
        cols |= {Kc - 1, Kc, Kc + 1, Kc + 33, 2 * Kc + 2, K - Kc, K - Kc - 1}      # the second split and the last one
    cols = sorted(c for c in cols if 0 <= c < K)
    qd, ed = q.cuda(), e.cuda()
    for i in range(0, len(cols), 16):
        km = cols[i:i + 16]                                                        # the last batch has fewer than 16 rows
        a = torch.zeros(len(km), K, dtype=BF16)
        a[torch.arange(len(km)), torch.tensor(km)] = 1.0
        out = ops.decode_gemm(a.cuda(), qd, w_block_scale=ed, out_f32=True).cpu()
        assert out.shape == (len(km), N)
        exp = want[:, km].t().contiguous()
        assert torch.equal(out, exp), (N, K, km, (out != exp).nonzero()[:8].tolist())


# ------------------------------------------------------------------------------------------------ skinny GEMM
@pytest.mark.parametrize("M", [1, 3, 8, 16])
def test_decode_gemm_w4_plain_and_fp32_out(M):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(M)
    for N, K in GEMM_SHAPES:
        a = torch.randn(M, K, device="cuda", generator=g).to(BF16)
        w, q, e = _qweight(N, K)                                        # w is dequantize(q, e) exactly (the quantiser test)
        ref = _ref_gemm(a, w)
        out32 = ops.decode_gemm(a, q, w_block_scale=e, out_f32=True)
        check(f"decode_gemm_w4 fp32 out M={M} N={N} K={K}", max_rel(out32, ref), 5e-6)
        log(f"decode_gemm (bf16 kernel, written-back weights) fp32 out M={M} N={N} K={K}", max_rel(ops.decode_gemm(a, w, out_f32=True), ref))
        out = ops.decode_gemm(a, q, w_block_scale=e)
        check(f"decode_gemm_w4 bf16 out M={M} N={N} K={K}", max_rel(out, ref), 5e-3)
        log(f"decode_gemm (bf16 kernel, written-back weights) bf16 out M={M} N={N} K={K}", max_rel(ops.decode_gemm(a, w), ref))
        assert torch.equal(ops.decode_gemm(a, q, w_block_scale=e, out_f32=True), out32), (N, K)      # run to run bit-identical
        assert torch.equal(ops.decode_gemm(a, q, w_block_scale=e), out), (N, K)


def test_decode_gemm_w4_lm_head_shape():
    ops = _ops()
    N, K = 128256, 4096
    g = torch.Generator(device="cuda").manual_seed(7)
    a = torch.randn(1, K, device="cuda", generator=g).to(BF16)
    w = _weight(N, K, g)
    q, e = ops.quant_blocks_mxfp4(w, writeback=True)
    ref = _ref_gemm(a, w)
    out32 = ops.decode_gemm(a, q, w_block_scale=e, out_f32=True)
    check(f"decode_gemm_w4 fp32 out M=1 N={N} K={K}", max_rel(out32, ref), 5e-6)
    log(f"decode_gemm (bf16 kernel, written-back weights) fp32 out M=1 N={N} K={K}", max_rel(ops.decode_gemm(a, w, out_f32=True), ref))
    out = ops.decode_gemm(a, q, w_block_scale=e)
    check(f"decode_gemm_w4 bf16 out M=1 N={N} K={K}", max_rel(out, ref), 5e-3)
    assert torch.equal(ops.decode_gemm(a, q, w_block_scale=e, out_f32=True), out32)


@pytest.mark.parametrize("M", [1, 5, 16])
def test_decode_gemm_w4_epilogues_and_norm_prologue(M):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(100 + M)
    for H, I in ((128, 256), (4096, 14336)):
        x = torch.randn(M, H, device="cuda", generator=g).to(BF16)
        gamma = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).to(BF16)
        wgu_rows, q_rows, e_rows = _qweight(2 * I, H)                   # quantisation is per row block: any row order of it is quantised too
        wgu, q, e = (ops.interleave_gate_up(t) for t in (wgu_rows, q_rows, e_rows))
        # RMSNorm prologue + SwiGLU epilogue against vp_rmsnorm_fwd -> fp32 product (bf16-rounded gate_up) -> vp_swiglu_fwd
        xn, _ = ops.rmsnorm_fwd(x, gamma, 1e-5)
        want = ops.swiglu_fwd(_ref_gemm(xn, wgu).to(BF16))
        got = ops.decode_gemm(x, q, w_block_scale=e, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL)
        check(f"decode_gemm_w4 norm+swiglu M={M} H={H} I={I}", max_rel(got, want), 2e-3)
        log(f"decode_gemm (bf16 kernel) norm+swiglu M={M} H={H} I={I}",
            max_rel(ops.decode_gemm(x, wgu, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL), want))
        assert torch.equal(got, ops.decode_gemm(x, q, w_block_scale=e, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL))
        # [gate | up] halves (IFT layout): the same rows in another order, each with its own scale bytes
        got_h = ops.decode_gemm(x, q_rows, w_block_scale=e_rows, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_HALVES)
        check(f"decode_gemm_w4 swiglu halves == interleaved M={M} H={H}", max_rel(got_h, got), 0.0)
        # residual epilogue (down_proj): bf16(bf16(acc) + residual)
        act = torch.randn(M, I, device="cuda", generator=g).to(BF16)
        wd, qd, ed = _qweight(H, I)
        res = torch.randn(M, H, device="cuda", generator=g).to(BF16)
        want = (_ref_gemm(act, wd).to(BF16).float() + res.float())
        got = ops.decode_gemm(act, qd, w_block_scale=ed, residual=res)
        check(f"decode_gemm_w4 residual M={M} H={H} K={I}", max_rel(got, want), 5e-3)
        log(f"decode_gemm (bf16 kernel) residual M={M} H={H} K={I}", max_rel(ops.decode_gemm(act, wd, residual=res), want))
        assert torch.equal(got, ops.decode_gemm(act, qd, w_block_scale=ed, residual=res))
        # norm prologue alone: the rounding points of rmsnorm_fwd, then the product
        w2, q2, e2 = _qweight(136, H)
        got = ops.decode_gemm(x, q2, w_block_scale=e2, norm_w=gamma, eps=1e-5, out_f32=True)
        check(f"decode_gemm_w4 norm prologue M={M} H={H}", max_rel(got, _ref_gemm(xn, w2)), 1e-6)
        log(f"decode_gemm (bf16 kernel) norm prologue M={M} H={H}",
            max_rel(ops.decode_gemm(x, w2, norm_w=gamma, eps=1e-5, out_f32=True), _ref_gemm(xn, w2)))
        assert torch.equal(got, ops.decode_gemm(x, q2, w_block_scale=e2, norm_w=gamma, eps=1e-5, out_f32=True))


# ------------------------------------------------------------------------------------------------ engines
def _engine_case(arch, quantize=True, lm_head=True, fmt="mxfp4"):
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.engine import Engine
    ocfg, W, batch, g = cases.tiny_llama_case(arch)
    eng = Engine(VisperConfig(**vars(ocfg)))
    eng.load_weights(W)
    if quantize:
        eng.quantize_decoder(lm_head=lm_head, fmt=fmt)
        assert eng.dequantized() and eng.fq_format == fmt
    return eng, batch


def _full_width_llama_engine(layers=2, quantize=True):
    from visper_lm_amd.config import llama3_8b
    from visper_lm_amd.engine import Engine
    cfg = llama3_8b(num_hidden_layers=layers, aux_mode="", num_task_tokens=0, vit_layers=1)
    eng = Engine(cfg)
    eng.init_random(seed=1)
    if quantize:
        eng.quantize_decoder(lm_head=True, fmt="mxfp4")
    return eng


@functools.lru_cache(maxsize=None)
def _shared_full_width_quantised_engine():
    """one quantised full-width engine for the tests that only decode from it"""
    return _full_width_llama_engine()


def _teacher_forced(eng, ids, images, N, name, bound):
    """test_decode_fp8_gpu._teacher_forced on an engine quantised to mxfp4: the 4-bit path's step logits against logits_of over prompt +
    generated tokens (asserted), the bf16 path's own deviation on the same engine beside it (logged)."""
    from visper_lm_amd import decode
    assert eng.dequantized() and eng.fq_format == "mxfp4"
    toks, kept, sess = decode.generate(eng, ids, None, images, None, max_new_tokens=N, return_logits=True)
    assert sess.fq is not None and sess.fq_format == "mxfp4", "the session must have decoded from the mxfp4 copies"
    want = _recompute_logits(eng, ids, toks, images)
    worst = max(max_rel(kept[i][0], want[i]) for i in range(N))
    with _bf16_decode(eng):
        toks_b, kept_b, sess_b = decode.generate(eng, ids, None, images, None, max_new_tokens=N, return_logits=True)
        assert sess_b.fq is None and sess_b.fq_format is None
    want_b = _recompute_logits(eng, ids, toks_b, images)
    log(f"teacher-forced decode logits {name}: bf16 path on the same mxfp4-quantised engine", max(max_rel(kept_b[i][0], want_b[i]) for i in range(N)))
    check(f"teacher-forced mxfp4 decode logits {name}", worst, bound)
    return (toks, kept, want), (toks_b, kept_b, want_b)


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_engine_mxfp4_decode_teacher_forced_tiny(arch):
    _ops()
    eng, batch = _engine_case(arch)
    ids = batch["input_ids"][:1]
    _teacher_forced(eng, ids, batch["images"][:1].cuda(), 12, f"tiny {arch} with image", 2e-2)
    text = ids[:, :24][ids[:, :24] >= 0][None]                            # text-only prompt: the <image> token dropped
    _teacher_forced(eng, text, None, 12, f"tiny {arch} text-only", 2e-2)


def test_engine_mxfp4_decode_teacher_forced_full_width_llama():
    _ops()
    eng = _shared_full_width_quantised_engine()
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _teacher_forced(eng, ids, None, 12, "full-width Llama-3 2 layers", 3e-2)


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_mxfp4_and_bf16_decode_agree_on_greedy_tokens(arch):
    """On a quantised engine both paths compute the same model: their greedy tokens agree wherever the bf16 path's top-1 / top-2 gap exceeds
    twice the larger of the two measured logit errors against the full recompute (the near-tie rule of _oracle_argmax_check).  The first
    disagreement ends the comparison (the sequences differ from there) and must itself be a near-tie."""
    _ops()
    eng, batch = _engine_case(arch)
    ids = batch["input_ids"][:1]
    N = 16
    (t4, k4, w4), (tb, kb, wb) = _teacher_forced(eng, ids, batch["images"][:1].cuda(), N, f"tiny {arch} with image, {N} tokens", 2e-2)
    err4 = max(float((k4[i][0] - w4[i]).abs().max()) for i in range(N))
    errb = max(float((kb[i][0] - wb[i]).abs().max()) for i in range(N))
    err = max(err4, errb)
    near, bad, seen = 0, [], 0
    for i in range(N):
        if i > 0 and not torch.equal(t4[0, :i], tb[0, :i]):
            break
        seen += 1
        top2 = kb[i][0].topk(2)
        if float(top2.values[0] - top2.values[1]) <= 2 * err:
            near += 1
        elif int(t4[0, i]) != int(tb[0, i]):
            bad.append(i)
    log(f"mxfp4 vs bf16 decode tiny {arch}: logit error mxfp4 path (max abs)", err4)
    log(f"mxfp4 vs bf16 decode tiny {arch}: logit error bf16 path (max abs)", errb)
    log(f"mxfp4 vs bf16 decode tiny {arch}: positions compared of {N}", seen)
    log(f"mxfp4 vs bf16 decode tiny {arch}: near-ties (top-2 gap <= {2 * err:.3g})", near)
    assert not bad, (arch, bad)
    assert near < seen, "every position was a near-tie: the comparison showed nothing"


def test_mxfp4_ragged_batch_eos_pad_eager_equals_graph(monkeypatch):
    _ops()
    from visper_lm_amd import decode
    eng, batch = _engine_case("llama")
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, 1000, (n,), generator=g) for n in (7, 19, 12)]
    T = max(len(p) for p in prompts)
    ids = torch.zeros(3, T, dtype=torch.long)
    am = torch.zeros(3, T, dtype=torch.long)
    for b, p in enumerate(prompts):                                        # left padding, as the eval scripts' tokenizers pad
        ids[b, T - len(p):] = p
        am[b, T - len(p):] = 1
    N = 10
    monkeypatch.setenv("VP_DECODE_GRAPH", "0")
    eager, _, s_e = decode.generate(eng, ids, am, None, None, max_new_tokens=N, return_logits=True)
    monkeypatch.setenv("VP_DECODE_GRAPH", "1")                            # the environment switch itself, not the use_graph argument
    captured, _, s_g = decode.generate(eng, ids, am, None, None, max_new_tokens=N, return_logits=True)
    assert s_e.fq_format == s_g.fq_format == "mxfp4" and not s_e.use_graph and s_g.use_graph and s_g.replays == N - 1
    assert torch.equal(eager, captured)
    for b, p in enumerate(prompts):                                        # each row decodes as it does alone
        single = decode.generate(eng, p[None], None, None, None, max_new_tokens=N)
        assert torch.equal(captured[b], single[0]), b
    # EOS: the token sequence 0 emits at step 3 ends it; later positions are pad, the others run on; eager == captured there too
    eos = int(eager[0, 3])
    out_g = decode.generate(eng, ids, am, None, None, max_new_tokens=N, eos_token_id=[eos], pad_token_id=-7)
    monkeypatch.setenv("VP_DECODE_GRAPH", "0")
    out_e = decode.generate(eng, ids, am, None, None, max_new_tokens=N, eos_token_id=[eos], pad_token_id=-7)
    assert torch.equal(out_g, out_e)
    for b in range(3):
        row = eager[b].tolist()
        stop = row.index(eos) if eos in row else None
        if stop is None:
            assert out_e[b].tolist() == row[:out_e.shape[1]]
        else:
            assert out_e[b, :stop + 1].tolist() == row[:stop + 1] and (out_e[b, stop + 1:] == -7).all()


def test_switching_an_engine_from_8_bit_to_4_bit_requantises():
    _ops()
    from visper_lm_amd import quant
    eng, batch = _engine_case("llama", fmt="e4m3")
    assert eng.fq_format == "e4m3"
    key = "dec.0.wqkv"
    N, K = eng.fz[key].shape
    assert eng.fq[key][0].shape == (N, K) and eng.fq[key][1].dtype == torch.float32
    eng.quantize_decoder(lm_head=True, fmt="mxfp4")
    assert eng.fq_format == "mxfp4" and eng.dequantized()
    for k, (q, e) in eng.fq.items():
        n, kk = eng.fz[k].shape
        assert q.shape == (n, kk // 2) and e.shape == (n, kk // 32) and e.dtype == torch.uint8, k
        assert torch.equal(eng.fz[k].float().cpu(), quant.dequantize_mxfp4(q, e)), k        # the bf16 weights are the 4-bit model now
    ids = batch["input_ids"][:1]
    _teacher_forced(eng, ids, batch["images"][:1].cuda(), 4, "tiny llama with image after e4m3 -> mxfp4", 2e-2)
    eng.quantize_decoder(lm_head=False)                                    # and back: the default format is e4m3
    assert eng.fq_format == "e4m3" and "lm_head" not in eng.fq
    with pytest.raises(ValueError, match="fmt"):
        eng.quantize_decoder(fmt="int4")


# ------------------------------------------------------------------------------------------------ staleness
def test_stale_mxfp4_copies_are_dropped_with_one_warning_after_an_optimizer_step():
    _ops()
    from oracle import cases
    from visper_lm_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    ocfg, W, batch, _ = cases.tiny_ift_case()
    model = LlavaLlamaForCausalLM(LlavaConfig(**vars(ocfg)), init="empty")
    model.load_state_dict(_sd(W), strict=True)
    ids = batch["input_ids"][:1, :24]
    ids = torch.where(ids < 0, torch.ones_like(ids), ids)                  # text-only prompt: no <image> token
    assert model.quantize_for_generation_4bit() is model
    eng = model._get_engine()
    assert eng.dequantized() and eng.fq_format == "mxfp4"
    with warnings.catch_warnings(record=True) as rec0:                     # current copies: no warning
        warnings.simplefilter("always")
        toks_q = model.generate(ids, max_new_tokens=8)
    assert not [r for r in rec0 if "stale" in str(r.message)]
    assert toks_q.shape == (1, 8)
    kw = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"], images=batch["images"].cuda())
    model(**kw).loss.backward()
    model.optimizer_step(lr=1e-2)
    with pytest.warns(RuntimeWarning, match="stale") as rec:
        toks = model.generate(ids, max_new_tokens=8)
    assert len([r for r in rec if "stale" in str(r.message)]) == 1
    assert not eng.dequantized() and eng.fq is None and eng.fq_format is None
    with warnings.catch_warnings(record=True) as rec2:                     # warned once: the next call is silent and still bf16
        warnings.simplefilter("always")
        toks2 = model.generate(ids, max_new_tokens=8)
    assert not [r for r in rec2 if "stale" in str(r.message)]
    assert torch.equal(toks, toks2)
    fresh = LlavaLlamaForCausalLM(LlavaConfig(**vars(ocfg)), init="empty")  # a never-quantised copy of the updated model
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=True)
    assert not fresh._get_engine().dequantized()
    assert torch.equal(fresh.generate(ids, max_new_tokens=8), toks)
    # re-quantising picks the updated weights up
    model.quantize_for_generation_4bit()
    assert eng.dequantized() and eng.fq_format == "mxfp4"


# ------------------------------------------------------------------------------------------------ what the format costs (a record, no gate)
def _cost(name, eng_ref, eng_q, ids, images, N=16):
    from visper_lm_amd import decode
    t_ref = decode.generate(eng_ref, ids, None, images, None, max_new_tokens=N)
    t_q = decode.generate(eng_q, ids, None, images, None, max_new_tokens=N)
    a = _recompute_logits(eng_ref, ids, t_ref, images)
    b = _recompute_logits(eng_q, ids, t_ref, images)                       # the same token sequence through both models
    log(f"quantisation cost {name}: logit deviation, quantised vs bf16 model (max abs / max |logit|)", float((a - b).abs().max() / a.abs().max()))
    agree = 0
    while agree < N and int(t_ref[0, agree]) == int(t_q[0, agree]):
        agree += 1
    log(f"quantisation cost {name}: greedy tokens equal before the first difference, of {N}", agree)
    log(f"quantisation cost {name}: greedy tokens equal position by position, of {N}", int((t_ref == t_q).sum()))


def test_record_quantisation_cost():
    _ops()
    for lm_head in (False, True):
        ref, batch = _engine_case("llama", quantize=False)
        qe, _ = _engine_case("llama", lm_head=lm_head)
        ids = batch["input_ids"][:1]
        _cost(f"tiny llama with image (mxfp4, lm_head {'mxfp4' if lm_head else 'bf16'})", ref, qe, ids, batch["images"][:1].cuda())
    ref, qe = _full_width_llama_engine(quantize=False), _shared_full_width_quantised_engine()
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _cost("full-width Llama-3 2 layers (mxfp4, lm_head mxfp4)", ref, qe, ids, None)
