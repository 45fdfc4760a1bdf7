"""The FP8 (e4m3) KV cache on the GPU: the prefill quantiser and the RoPE + append kernel against the CPU contract (quant.py) bit for bit,
the byte-cache decode attention with its conversion pinned code by code and against fp64 softmax attention on the dequantised cache (gated
by what the bf16 kernel itself needs on the same cache), the engine's fp8-cache steps against the emulated cache (the same model on the
bf16 kernels), ragged batches, the public API, and a record of what the format itself costs against the bf16 cache."""
import functools
import math

import pytest
import torch

from parity import check, log, max_rel

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
U8 = torch.uint8
F32 = torch.float32


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops
    return ops


def _deq(q, s, D):
    """fp32 = e4m3fn(q [..., H*D]) * s [..., H] per head, in plain torch on the CPU (exact)"""
    qc, sc = q.detach().cpu().contiguous(), s.detach().cpu().contiguous()
    v = qc.view(torch.float8_e4m3fn).to(F32).unflatten(-1, (sc.shape[-1], D))
    return (v * sc[..., None]).flatten(-2)


# ------------------------------------------------------------------------------------------------ quantiser (the prefill's cache writer)
@pytest.mark.parametrize("Hkv,D", [(2, 32), (32, 96), (8, 128)])
def test_quant_kv_kernel_matches_the_cpu_contract_exactly(Hkv, D):
    ops = _ops()
    from visper_lm_amd import quant
    n, Hq, C = 37, 2 * Hkv, 2 * Hkv * D
    g = torch.Generator(device="cuda").manual_seed(Hkv + D)
    qkv = torch.randn(n, (Hq + 2 * Hkv) * D, device="cuda", generator=g)
    fac = torch.exp2(torch.randint(-6, 7, (n, Hq + 2 * Hkv, 1), device="cuda", generator=g).float())   # scales differ per (token, head)
    qkv = (qkv.view(n, -1, D) * fac).view(n, -1).to(BF16)
    qkv[4, Hq * D:Hq * D + D] = 0                                         # a zero head
    qkv[5, Hq * D + D + 3] = 3.0e4                                        # an outlier
    qkv0 = qkv.clone()
    src = qkv[:, Hq * D:]                                                  # the k|v columns: a strided view
    B, Smax, b, r0 = 2, 50, 1, 3
    qc = torch.full((B, Smax, C), 0xAB, device="cuda", dtype=U8)
    sc = torch.full((B, Smax, 2 * Hkv), 123.0, device="cuda", dtype=F32)
    dc = torch.full((B, Smax, C), 7.0, device="cuda", dtype=BF16)
    ops.quant_kv_e4m3(src, D, q_out=qc[b, r0:r0 + n], scale_out=sc[b, r0:r0 + n], deq_out=dc[b, r0:r0 + n])
    assert torch.equal(qkv, qkv0), "the source is read only"
    want_q, want_s = quant.quantize_kv_heads(qkv0[:, Hq * D:].cpu().contiguous(), 2 * Hkv, D)
    assert torch.equal(qc[b, r0:r0 + n].cpu(), want_q)
    assert torch.equal(sc[b, r0:r0 + n].cpu(), want_s)
    assert len(torch.unique(want_s)) >= 8                                  # the scales did differ
    assert torch.equal(dc[b, r0:r0 + n].cpu().float(), quant.dequantize_kv_heads(want_q, want_s, 2 * Hkv, D))
    rows = torch.ones(B, Smax, dtype=torch.bool, device="cuda")
    rows[b, r0:r0 + n] = False
    assert (qc[rows] == 0xAB).all() and (sc[rows] == 123.0).all() and (dc[rows] == 7.0).all()       # every other cache row untouched
    # a second call gives identical output; either destination alone gives the same values
    q1, s1, d1 = qc.clone(), sc.clone(), dc.clone()
    ops.quant_kv_e4m3(src, D, q_out=qc[b, r0:r0 + n], scale_out=sc[b, r0:r0 + n], deq_out=dc[b, r0:r0 + n])
    assert torch.equal(qc, q1) and torch.equal(sc, s1) and torch.equal(dc, d1)
    q2 = torch.zeros(n, C, device="cuda", dtype=U8)
    s2 = torch.zeros(n, 2 * Hkv, device="cuda", dtype=F32)
    d2 = torch.zeros(n, C, device="cuda", dtype=BF16)
    ops.quant_kv_e4m3(src, D, q_out=q2, scale_out=s2)
    ops.quant_kv_e4m3(src, D, deq_out=d2)
    assert torch.equal(q2, q1[b, r0:r0 + n]) and torch.equal(s2, s1[b, r0:r0 + n]) and torch.equal(d2, d1[b, r0:r0 + n])
    assert torch.equal(qkv, qkv0)


# ------------------------------------------------------------------------------------------------ RoPE + append
@pytest.mark.parametrize("B,Hq,Hkv,D,Smax,positions", [(3, 8, 2, 32, 40, (0, 17, 39)), (3, 4, 2, 128, 24, (5, 23, 24)),
                                                       (2, 4, 4, 96, 16, (15, -1))])
def test_decode_rope_append_kv8_writes_the_contract_into_row_pos_only(B, Hq, Hkv, D, Smax, positions):
    """the first case is test_decode_rope_append_writes_only_row_pos's; the others add D = 128 / 96 and positions outside [0, Smax), which
    write nothing"""
    ops = _ops()
    from visper_lm_amd import quant
    g = torch.Generator(device="cuda").manual_seed(7)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", generator=g)
    fac = torch.exp2(torch.randint(-6, 7, (B, Hq + 2 * Hkv, 1), device="cuda", generator=g).float())
    qkv = (qkv.view(B, -1, D) * fac).view(B, -1).to(BF16)
    pos = torch.tensor(positions, device="cuda", dtype=torch.int32)
    cos, sin = ops.rope_tables(64, D, 10000.0, "cuda")
    # what the bf16 kernel stores
    cache = torch.full((B, Smax, 2, Hkv * D), 7.0, device="cuda", dtype=BF16)
    q_ref = torch.empty(B, Hq * D, device="cuda", dtype=BF16)
    ops.decode_rope_append(qkv, q_ref, cache[:, :, 0].unflatten(-1, (Hkv, D)), cache[:, :, 1].unflatten(-1, (Hkv, D)), cos, sin, pos, Hq, Hkv, D)
    # the kv8 kernel: bytes + scales + the bf16 destination
    qc = torch.full((B, Smax, 2, Hkv * D), 0xAB, device="cuda", dtype=U8)
    sc = torch.full((B, Smax, 2, Hkv), 123.0, device="cuda", dtype=F32)
    dc = torch.full((B, Smax, 2, Hkv * D), 7.0, device="cuda", dtype=BF16)
    k4 = lambda t: t[:, :, 0].unflatten(-1, (Hkv, D))
    v4 = lambda t: t[:, :, 1].unflatten(-1, (Hkv, D))
    q = torch.empty(B, Hq * D, device="cuda", dtype=BF16)
    qkv0 = qkv.clone()
    ops.decode_rope_append_kv8(qkv, q, cos, sin, pos, Hq, Hkv, D, k_bytes=k4(qc), v_bytes=v4(qc), k_scale=sc[:, :, 0], v_scale=sc[:, :, 1],
                               k_deq=k4(dc), v_deq=v4(dc))
    assert torch.equal(qkv, qkv0)
    assert torch.equal(q, q_ref), "q must be bit-identical to the bf16 kernel's"
    mask = torch.zeros(B, Smax, dtype=torch.bool, device="cuda")
    for b, p in enumerate(positions):
        if 0 <= p < Smax:
            mask[b, p] = True
            for kv in (0, 1):
                want_q, want_s = quant.quantize_kv_heads(cache[b, p, kv][None].cpu(), Hkv, D)
                assert torch.equal(qc[b, p, kv].cpu(), want_q[0]), (b, kv)
                assert torch.equal(sc[b, p, kv].cpu(), want_s[0]), (b, kv)
                assert torch.equal(dc[b, p, kv].cpu().float(), quant.dequantize_kv_heads(want_q, want_s, Hkv, D)[0]), (b, kv)
    assert int(mask.sum()) == sum(0 <= p < Smax for p in positions)
    assert (qc[~mask] == 0xAB).all() and (sc[~mask] == 123.0).all() and (dc[~mask] == 7.0).all()     # every other row and scale untouched
    # either destination alone: the same q, the same row
    qc2, sc2, dc2 = torch.full_like(qc, 0xAB), torch.full_like(sc, 123.0), torch.full_like(dc, 7.0)
    qa, qb = torch.empty_like(q), torch.empty_like(q)
    ops.decode_rope_append_kv8(qkv, qa, cos, sin, pos, Hq, Hkv, D, k_bytes=k4(qc2), v_bytes=v4(qc2), k_scale=sc2[:, :, 0], v_scale=sc2[:, :, 1])
    ops.decode_rope_append_kv8(qkv, qb, cos, sin, pos, Hq, Hkv, D, k_deq=k4(dc2), v_deq=v4(dc2))
    assert torch.equal(qa, q_ref) and torch.equal(qb, q_ref)
    assert torch.equal(qc2, qc) and torch.equal(sc2, sc) and torch.equal(dc2, dc)


# ------------------------------------------------------------------------------------------------ the conversion, code by code
CODES = [c for c in range(256) if c & 0x7f != 0x7f]                        # the 254 e4m3fn bytes that are not NaN


@pytest.mark.parametrize("D", [32, 96, 128])
def test_decode_attn_kv8_conversion_is_exact_for_every_code(D):
    """one visible key: the softmax weight is 1 and the output is the dequantised v row.  Pins the byte order within the 16-byte load, the
    head and token indexing of the scale, and the conversion of every code"""
    ops = _ops()
    B, Hq, Hkv, Smax = 4, 4, 2, 4
    g = torch.Generator().manual_seed(D)
    codes = torch.tensor(CODES, dtype=U8)
    vscales = torch.tensor([2.0 ** -20, 1.0, 2.0 ** 9])
    kv = torch.empty(B, Smax, 2, Hkv * D, dtype=U8)
    sc = torch.empty(B, Smax, 2, Hkv, dtype=F32)
    kv[:, :, 0] = codes[torch.randint(0, 254, (B, Smax, Hkv * D), generator=g)]
    sc[:, :, 0] = torch.exp2(torch.randint(-3, 4, (B, Smax, Hkv), generator=g).float())
    for t in range(Smax):                                                  # every token its own lay-out of the codes and of the scales
        idx = (torch.arange(B * Hkv * D) + 37 * t) % 254
        kv[:, t, 1] = codes[idx].view(B, Hkv * D)
        sc[:, t, 1] = vscales[(torch.arange(B * Hkv) + t) % 3].view(B, Hkv)
    assert len(set(kv[:, 0, 1].flatten().tolist())) == 254                 # token 0 alone carries every code
    kvd, scd = kv.cuda(), sc.cuda()
    k4, v4 = kvd[:, :, 0].unflatten(-1, (Hkv, D)), kvd[:, :, 1].unflatten(-1, (Hkv, D))
    q = torch.randn(B, Hq * D, generator=g).to(BF16).cuda()
    want_all = _deq(kv[:, :, 1], sc[:, :, 1], D).view(B, Smax, Hkv, D)
    # (kv_len, window) -> the one visible token
    for kv_len, window, tok in ((1, 0, 0), (3, 1, 2), (4, 1, 3)):
        kl = torch.full((B,), kv_len, device="cuda", dtype=torch.int32)
        got = ops.decode_attn_kv8(q, k4, v4, scd[:, :, 0], scd[:, :, 1], kl, Hq, window=window).cpu().float().view(B, Hq, D)
        want = want_all[:, tok].repeat_interleave(Hq // Hkv, 1)            # code x scale; -0 == 0 as numbers
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (D, kv_len, window, bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ attention against fp64
def _ref_attn64(q, k, v, lens, window, scale):
    """fp64 softmax attention, one query row per sequence: q [B, Hq, D], k / v [B, Smax, Hkv, D] (fp32 values) -> [B, Hq, D] float64"""
    B, Hq, D = q.shape
    Hkv = k.shape[2]
    out = torch.zeros(B, Hq, D, device=q.device, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        lo = max(0, L - window) if window else 0
        kk = k[b, lo:L].double().repeat_interleave(Hq // Hkv, 1)           # [n, Hq, D]
        vv = v[b, lo:L].double().repeat_interleave(Hq // Hkv, 1)
        s = torch.einsum("hd,nhd->hn", q[b].double(), kk) * scale
        out[b] = torch.einsum("hn,nhd->hd", s.softmax(-1), vv)
    return out


def _tol_needed(got, want):
    """the smallest tol with |got - want| <= 2^-8 |want| + tol max|want| elementwise, the max taken over each (b, head)"""
    got, want = got.double(), want.double()
    excess = ((got - want).abs() - 2.0 ** -8 * want.abs()).clamp_min(0)
    return float((excess / want.abs().amax(-1, keepdim=True).clamp_min(1e-300)).max())


@pytest.mark.parametrize("D,Hq,Hkv", [(32, 4, 2), (96, 32, 32), (128, 32, 8), (128, 8, 8)])
def test_decode_attn_kv8_against_fp64_on_the_dequantised_cache(D, Hq, Hkv):
    """|got - want| <= 2^-8 |want| + tol max|want|: 2^-8 is the output's bf16 rounding (half an ulp), tol covers the fp32 arithmetic.  The
    bf16 kernel's own tol on the dequantised cache is measured in the same run; the byte kernel is gated at max(1e-4, 4 x) of it (x 4: a
    different summation order over twice the elements per lane).  An fp32 evaluation needs tol < 1e-7; a kernel that takes the k or v scale
    of the neighbouring token needs >= 0.26, one that reads the un-quantised cache 0.09 .. 0.22."""
    ops = _ops()
    lens = [1, 2, 33, 777, 2100]                                           # one key, less than one pass, splits crossing 512, ragged
    B, Smax, C = len(lens), max(lens), 2 * Hkv * D
    g = torch.Generator(device="cuda").manual_seed(D + Hq)
    x = torch.randn(B, Smax, 2 * Hkv, D, device="cuda", generator=g)
    ek = torch.randint(-2, 3, (B, Smax, Hkv, 1), device="cuda", generator=g)
    ev = torch.randint(-6, 7, (B, Smax, Hkv, 1), device="cuda", generator=g)
    x = (x * torch.exp2(torch.cat([ek, ev], 2).float())).to(BF16).view(B * Smax, C)
    kvq = torch.empty(B, Smax, C, device="cuda", dtype=U8)
    kvs = torch.empty(B, Smax, 2 * Hkv, device="cuda", dtype=F32)
    kvd = torch.empty(B, Smax, C, device="cuda", dtype=BF16)
    ops.quant_kv_e4m3(x, D, q_out=kvq.view(B * Smax, C), scale_out=kvs.view(B * Smax, 2 * Hkv), deq_out=kvd.view(B * Smax, C))
    deq = _deq(kvq, kvs, D).cuda()                                         # the cache's values, from the bytes and scales in plain torch
    assert torch.equal(deq, kvd.float())
    halves = lambda t, w: (t[:, :, :Hkv * w], t[:, :, Hkv * w:])
    kq, vq = (t.unflatten(-1, (Hkv, D)) for t in halves(kvq, D))
    kd, vd = (t.unflatten(-1, (Hkv, D)) for t in halves(kvd, D))
    kf, vf = (t.unflatten(-1, (Hkv, D)) for t in halves(deq, D))
    ks, vs = halves(kvs, 1)
    q = torch.randn(B, Hq * D, device="cuda", generator=g).to(BF16)
    kl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    for window in (0, 500):
        want = _ref_attn64(q.view(B, Hq, D), kf, vf, lens, window, 1.0 / math.sqrt(D))
        parent = ops.decode_attn(q, kd, vd, kl, Hq, window=window)
        got = ops.decode_attn_kv8(q, kq, vq, ks, vs, kl, Hq, window=window)
        t_parent, t_got = _tol_needed(parent.view(B, Hq, D), want), _tol_needed(got.view(B, Hq, D), want)
        name = f"D={D} {Hq}:{Hkv} window={window}"
        log(f"decode_attn (bf16 kernel, dequantised cache) vs fp64 {name}: tol needed", t_parent)
        check(f"decode_attn_kv8 vs fp64 on the dequantised cache {name}: tol needed", t_got, max(1e-4, 4 * t_parent))
        assert torch.equal(got, ops.decode_attn_kv8(q, kq, vq, ks, vs, kl, Hq, window=window))        # bit-identical run to run


# ------------------------------------------------------------------------------------------------ engine: the same model on two kernels
@functools.lru_cache(maxsize=None)
def _case(arch):
    from oracle import cases
    return cases.tiny_llama_case(arch)


def _tiny_engine(arch):
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.engine import Engine
    ocfg, W, batch, g = _case(arch)
    eng = Engine(VisperConfig(**vars(ocfg)))
    eng.load_weights(W)
    return eng, batch


@functools.lru_cache(maxsize=None)
def _full_width_llama_engine(layers=2):
    from visper_lm_amd.config import llama3_8b
    from visper_lm_amd.engine import Engine
    eng = Engine(llama3_8b(num_hidden_layers=layers, aux_mode="", num_task_tokens=0, vit_layers=1))
    eng.init_random(seed=1)
    return eng


def _forced(eng, dtype, ids, am, images, toks, N):
    """a session of its own with cache `dtype`, fed `toks` [B, >= N - 1] through step() -> ([N] logits [B, V], session)"""
    from visper_lm_amd import decode
    sess = decode.DecodeSession(eng, kv_cache_dtype=dtype)
    sess.use_graph = False
    out = []
    with torch.no_grad():
        out.append(sess.prefill(ids, am, images, None, N).clone())
        for i in range(1, N):
            out.append(sess.step(toks[:, i - 1].to(eng.dev)).clone())
    return out, sess


def _same_model_two_kernels(eng, ids, images, N, name, bound, use_graph=False):
    """session A ("fp8_e4m3") generates greedily; session B ("fp8_e4m3_emulated": the dequantised rows in a bf16 cache, read by
    vp_decode_attn) is fed A's tokens; their step logits agree within the decode path's own bound"""
    from visper_lm_amd import decode
    toks, kept, sa = decode.generate(eng, ids, None, images, None, max_new_tokens=N, return_logits=True, kv_cache_dtype="fp8_e4m3",
                                     use_graph=use_graph)
    assert sa.kv_cache_dtype == "fp8_e4m3" and sa.cache.kv[0].dtype == U8 and sa.use_graph == use_graph and len(kept) == N
    emu, sb = _forced(eng, "fp8_e4m3_emulated", ids, None, images, toks, N)
    assert sb.cache.kv[0].dtype == BF16 and sb.cache.nbytes * (eng.cfg.head_dim + 4) == sa.cache.nbytes * 2 * eng.cfg.head_dim
    check(f"fp8 KV cache vs emulated cache, step logits {name}", max(max_rel(kept[i], emu[i]) for i in range(N)), bound)
    # the prompt's rows were written by one quantiser from the same prefill: the bytes times the scales ARE the emulated cache's rows
    L0 = int(sa.cache.lens_host[0]) - (N - 1)
    hd = eng.cfg.head_dim
    for l in (0, eng.cfg.num_hidden_layers - 1):
        assert torch.equal(_deq(sa.cache.kv[l][0, :L0], sa.cache.scales[l][0, :L0], hd), sb.cache.kv[l][0, :L0].cpu().float()), l
    return toks, kept


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_engine_fp8_cache_equals_emulated_cache_tiny(arch):
    _ops()
    eng, batch = _tiny_engine(arch)
    ids, img = batch["input_ids"][:1], batch["images"][:1].cuda()
    toks, kept = _same_model_two_kernels(eng, ids, img, 12, f"tiny {arch} with image", 2e-2)
    if arch == "llama":                                                    # the captured step: the eager run's logits
        toks_g, kept_g = _same_model_two_kernels(eng, ids, img, 12, "tiny llama with image, captured step", 2e-2, use_graph=True)
        assert torch.equal(toks_g, toks) and all(torch.equal(a, b) for a, b in zip(kept_g, kept))


def test_engine_fp8_cache_with_mxfp4_weights():
    """the cache format is independent of the weight format"""
    _ops()
    eng, batch = _tiny_engine("llama")
    eng.quantize_decoder(fmt="mxfp4")
    assert eng.dequantized() and eng.fq_format == "mxfp4"
    _same_model_two_kernels(eng, batch["input_ids"][:1], batch["images"][:1].cuda(), 12, "tiny llama with image, mxfp4 weights", 2e-2)


def test_engine_fp8_cache_equals_emulated_cache_full_width_llama():
    _ops()
    eng = _full_width_llama_engine()
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _same_model_two_kernels(eng, ids, None, 12, "full-width Llama-3 2 layers", 3e-2)


# ------------------------------------------------------------------------------------------------ ragged batch, EOS, pad, graph
def test_fp8_cache_ragged_batch_eos_pad_and_graph():
    _ops()
    from visper_lm_amd import decode
    eng, batch = _tiny_engine("llama")
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, 1000, (n,), generator=g) for n in (7, 19, 12)]
    T = max(len(p) for p in prompts)
    ids = torch.zeros(3, T, dtype=torch.long)
    am = torch.zeros(3, T, dtype=torch.long)
    for b, p in enumerate(prompts):                                        # left padding, as the eval scripts' tokenizers pad
        ids[b, T - len(p):] = p
        am[b, T - len(p):] = 1
    N = 10
    kw = dict(max_new_tokens=N, kv_cache_dtype="fp8_e4m3")
    batched, kept, sess = decode.generate(eng, ids, am, None, None, use_graph=False, return_logits=True, **kw)
    assert sess.cache.dtype == "fp8_e4m3"
    captured = decode.generate(eng, ids, am, None, None, use_graph=True, **kw)
    assert torch.equal(batched, captured)                                  # graph replay == eager launches
    worst = 0.0
    for b, p in enumerate(prompts):                                        # each row alone, fed the batch's tokens
        alone, _ = _forced(eng, "fp8_e4m3", p[None], None, None, batched[b:b + 1], N)
        worst = max(worst, max(max_rel(kept[i][b], alone[i][0]) for i in range(N)))
    check("fp8 KV cache: a row's step logits in the ragged batch vs alone", worst, 2e-2)
    # EOS: the token sequence 0 emits at step 3 ends it; later positions are pad, the others run on
    eos = int(batched[0, 3])
    out = decode.generate(eng, ids, am, None, None, eos_token_id=[eos], pad_token_id=-7, **kw)
    for b in range(3):
        row = batched[b].tolist()
        stop = row.index(eos) if eos in row else None
        if stop is None:
            assert out[b].tolist() == row[:out.shape[1]]
        else:
            assert out[b, :stop + 1].tolist() == row[:stop + 1] and (out[b, stop + 1:] == -7).all()
    assert out.shape[1] <= N
    first = [int(batched[b, 0]) for b in range(3)]                         # every row finished -> the loop stops early
    assert decode.generate(eng, ids, am, None, None, eos_token_id=first, **kw).shape[1] == 1


# ------------------------------------------------------------------------------------------------ public API
def _sd(W):
    return {k.replace("model.vision_tower.vision_tower.", "model.vision_tower.vision_tower.vision_model.")
            if k.startswith("model.vision_tower.vision_tower.") else k: v for k, v in W.items()}


def test_model_generate_kv_cache_dtype_and_default():
    _ops()
    from visper_lm_amd import decode
    from visper_lm_amd.model import OlaLlavaLlamaConfig, OlaLlavaLlamaForCausalLM
    ocfg, W, batch, g = _case("llama")
    model = OlaLlavaLlamaForCausalLM(OlaLlavaLlamaConfig(**vars(ocfg)), init="empty")
    model.load_state_dict(_sd(W), strict=True)
    model.reload_frozen()
    ids = torch.cat([batch["input_ids"][:1]] * 2)
    img = torch.cat([batch["images"][:1]] * 2).cuda()
    eng = model._get_engine()
    assert eng.kv_cache_dtype == "bf16"
    t_bf16 = model.generate(ids, images=img, max_new_tokens=6)
    t_fp8 = model.generate(ids, images=img, max_new_tokens=6, kv_cache_dtype="fp8_e4m3")
    assert t_fp8.shape == (2, 6) and t_fp8.dtype == torch.long and t_bf16.shape == (2, 6)
    with pytest.raises(ValueError, match="fp8_e4m3"):
        model.generate(ids, images=img, max_new_tokens=6, kv_cache_dtype="int3")
    with pytest.raises(ValueError, match="fp8_e4m3"):
        decode.DecodeSession(eng, kv_cache_dtype="fp4")
    assert model.quantize_kv_cache_for_generation() is model and eng.kv_cache_dtype == "fp8_e4m3"
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=6), t_fp8)                     # now the default
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=6, kv_cache_dtype="bf16"), t_bf16)          # the argument overrides it
    _, _, sess = decode.generate(eng, ids, None, img, None, max_new_tokens=6, return_logits=True)
    cfg = eng.cfg
    L, Hkv, D = cfg.num_hidden_layers, cfg.num_key_value_heads, cfg.head_dim
    assert sess.cache.dtype == "fp8_e4m3" and sess.cache.nbytes == L * 2 * sess.cache.Smax * 2 * Hkv * (D + 4)
    _, _, sess_b = decode.generate(eng, ids, None, img, None, max_new_tokens=6, return_logits=True, kv_cache_dtype="bf16")
    assert sess.cache.nbytes * 2 * D == sess_b.cache.nbytes * (D + 4)                                # the halved cache
    model.quantize_kv_cache_for_generation(enable=False)
    assert eng.kv_cache_dtype == "bf16" and torch.equal(model.generate(ids, images=img, max_new_tokens=6), t_bf16)


# ------------------------------------------------------------------------------------------------ what the format costs (a record, no gate)
def _kv_cost(name, eng, ids, images, N=16):
    from visper_lm_amd import decode
    t_ref, k_ref, _ = decode.generate(eng, ids, None, images, None, max_new_tokens=N, return_logits=True)
    t_q = decode.generate(eng, ids, None, images, None, max_new_tokens=N, kv_cache_dtype="fp8_e4m3")
    k_q, _ = _forced(eng, "fp8_e4m3", ids, None, images, t_ref, N)          # the same token sequence over both caches
    dev = max(float((a - b).abs().max()) for a, b in zip(k_ref, k_q)) / max(float(a.abs().max()) for a in k_ref)
    log(f"KV quantisation cost {name}: logit deviation, fp8 vs bf16 cache (max abs / max |logit|)", dev)
    agree = 0
    while agree < N and int(t_ref[0, agree]) == int(t_q[0, agree]):
        agree += 1
    log(f"KV quantisation cost {name}: greedy tokens equal before the first difference, of {N}", agree)
    log(f"KV quantisation cost {name}: greedy tokens equal position by position, of {N}", int((t_ref == t_q).sum()))


def test_record_kv_quantisation_cost():
    _ops()
    for arch in ("llama", "phi3"):
        eng, batch = _tiny_engine(arch)
        _kv_cost(f"tiny {arch} with image", eng, batch["input_ids"][:1], batch["images"][:1].cuda())
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _kv_cost("full-width Llama-3 2 layers", _full_width_llama_engine(), ids, None)
