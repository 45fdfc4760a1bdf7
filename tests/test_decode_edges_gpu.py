"""The quantised decode kernels of csrc/decode.hip (vp_decode_gemm_w8 / _w4 beside vp_decode_gemm, vp_decode_attn_kv8, vp_quant_kv_e4m3, the two
RoPE + append kernels, the two weight quantisers) at the chunk, split and stride edges of tests/decode_cases.py.  tests/DECODE_PATHS.md maps
every path to its case; tests/test_decode_edges_host.py proves on the CPU that the tables enter what they claim and that the comparisons made
here reject every mutant.

Every operand and every output of the GEMMs is a view inside a sentinel-filled allocation (decode_cases.Box).  Per case:
  outside   every element of the output allocation outside the view keeps the sentinel; the input allocations are bit-unchanged
  exact     the exact draws: torch.equal with the fp64 product (fp32 out), with bf16(fp32(exact)), with dg_store's two rounding points
            (residual); strided == contiguous and kernel == kernel, bit for bit
  bounded   regimes.group_err against fp64 with regimes.bound(...), y = the fp32 reference's own error, through parity.check"""
import math

import pytest
import torch

import decode_cases as DC
import parity
import regimes as R
from decode_cases import BF, F32, F64, U8

pytestmark = pytest.mark.gpu
OUTS = ("f32", "bf16", "res")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops as o
    return o


def run_gemm(ops, c, ko, epi=DC.EPI_NONE, norm=False, ncols=None):
    out = DC.out_box(c, "bf16" if epi else ko, ncols)
    kw = {}
    if c.kind == "w8":
        kw["w_scale"] = c.s8
    elif c.kind == "w4":
        kw["w_block_scale"] = c.e.view
    ops.decode_gemm(c.a.view, c.w.view, residual=c.res.view if ko == "res" else None, norm_w=c.gamma.view[0] if norm else None, eps=c.inp.eps,
                    epi=epi, out=out.view, **kw)
    return out


def check_bounded(label, rb):
    """every comparison through parity.check, all of them before the first failure is raised"""
    fails = []
    for g, (e, b) in rb.items():
        try:
            parity.check(f"decode edges {label} [{g}]", e if math.isfinite(e) else 1e30, b)
        except AssertionError as ex:
            fails.append(str(ex))
    assert not fails, "\n".join(fails)


# ================================================================================================ 1. skinny GEMMs: chunk paths, exactly
def test_split_factors_are_the_models(ops):
    """ks == workspace bytes / (4 M N), or 1 when the query returns 0: the library agrees with decode_cases.ksplit on every case"""
    q = lambda kind, M, N, K, epi: (ops.decode_gemm_ws_bytes(M, N, K, epi, w8=kind == "w8", w4=kind == "w4") // (4 * M * N)) or 1
    for kind in DC.KERNELS:
        for K, ks in DC.K_TABLE[kind]:
            for M in DC.GEMM_MS:
                assert q(kind, M, DC.GEMM_N, K, DC.EPI_NONE) == ks == DC.ksplit(kind, DC.GEMM_N, K), (kind, K, M)
        for N, K in DC.SWIGLU_SHAPES:
            for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
                assert q(kind, 5, N, K, epi) == DC.SWIGLU_KS[kind][K] == DC.ksplit(kind, N, K, epi), (kind, N, K, epi)
        assert q(kind, 5, *DC.ONE_TILE, DC.EPI_NONE) == DC.ksplit(kind, *DC.ONE_TILE)


def exact_case(ops, kind, draw, M, N, K, layouts):
    """every kernel that admits K, the table's own first, on one exact draw: each layout bit-equal to the expected values, the sentinel intact,
    the inputs unchanged, every layout and every kernel bit-equal to the first"""
    inp = DC.gemm_inputs(draw, M, N, K)
    want = {k: v.cuda() for k, v in DC.exact_outputs(inp).items()}
    first = {}
    for k2 in [kind] + [k for k in DC.kernels_at(K) if k != kind]:
        for lay in (layouts if k2 == "w4" else [l for l in layouts if "lde" not in l and "e_off" not in l]):
            c = DC.gemm_call(k2, inp, device="cuda", **lay)
            for ko in OUTS:
                out = run_gemm(ops, c, ko)
                tag = (kind, K, M, k2, lay, ko)
                assert out.outside_intact(), tag
                assert torch.equal(out.view, want[ko]), (tag, (out.view != want[ko]).nonzero()[:4].tolist())
                assert DC.bits_equal(out.view, first.setdefault(ko, out.view.clone())), tag
            assert DC.inputs_unchanged(c), (kind, K, M, k2, lay)


@pytest.mark.parametrize("kind,K", [(kind, K) for kind in DC.KERNELS for K, _ in DC.K_TABLE[kind]])
def test_gemm_chunk_paths_are_exact(ops, kind, K):
    """N = 136 (a tail tile of 8 rows), M in {1, 5, 16}; lda = K + 16, ldw = K + 32 (K / 2 + 16 bytes for W4), ldc = N + 8, ldr = N + 24 against
    the contiguous call; for W4 the scale rows tight (lde = K / 32) and padded to a multiple of 16 plus 16 (the 16-byte scale loads)"""
    layouts = [{}, dict(strided=False)] + ([dict(lde=DC.lde_padded(K))] if K % 32 == 0 else [])
    for M in DC.GEMM_MS:
        exact_case(ops, kind, "w4" if kind == "w4" else "w8", M, DC.GEMM_N, K, layouts)


@pytest.mark.parametrize("kind", DC.KERNELS)
def test_gemm_single_tile_clamped_to_the_last_row(ops, kind):
    N, K = DC.ONE_TILE
    for M in DC.GEMM_MS:
        exact_case(ops, kind, "w4" if kind == "w4" else "w8", M, N, K, [{}, dict(strided=False), dict(lde=DC.lde_padded(K))])


@pytest.mark.parametrize("K", DC.W4_MISALIGNED_E)
def test_w4_misaligned_scale_base_takes_the_byte_path(ops, K):
    """E one byte into its allocation with lde % 16 == 0 on whole chunks: evec is false by the base alone.  Bit-equal to the expected values
    and hence to the aligned call's 16-byte scale loads"""
    for M in DC.GEMM_MS:
        inp = DC.gemm_inputs("w4", M, DC.GEMM_N, K)
        want = {k: v.cuda() for k, v in DC.exact_outputs(inp).items()}
        c = DC.gemm_call("w4", inp, device="cuda", lde=DC.lde_padded(K), e_off=1)
        assert c.e.view.data_ptr() % 16 == 1 and c.e.ld % 16 == 0 and K % 512 == 0
        ca = DC.gemm_call("w4", inp, device="cuda", lde=DC.lde_padded(K))
        assert ca.e.view.data_ptr() % 16 == 0
        for ko in OUTS:
            out = run_gemm(ops, c, ko)
            assert out.outside_intact() and torch.equal(out.view, want[ko]), (K, M, ko)
            assert DC.bits_equal(out.view, run_gemm(ops, ca, ko).view)
        assert DC.inputs_unchanged(c)


CODES = [c for c in range(256) if c & 0x7f != 0x7f]                        # the 254 e4m3fn bytes that are not NaN


@pytest.mark.parametrize("N,K", DC.W8_ONE_HOT)
def test_decode_gemm_w8_one_hot_products_are_exact(ops, N, K):
    """The counterpart of test_decode_gemm_w4_one_hot_products_are_exact: a row that is 1.0 at column k must return code x scale of W[n, k]
    exactly in fp32 (torch.equal: every bit of every non-zero value; the codes 0x00 and 0x80 must both return a zero, whose sign a sum that
    starts at +0 does not keep).  Every non-NaN code in row 0 (K >= 254; K = 80 cannot hold them) and, at every K, among the entries the
    one-hot columns look at; row scales 2^-20 .. 2^9.  Under split-K (K = 8192, ks = 8) the columns hold both sides of each of the seven Kc
    boundaries.  Pins the byte order within a 16-byte load, the k permutation of both MFMA operands and the row of the scale."""
    g = torch.Generator().manual_seed(K)
    codes = torch.tensor(CODES, dtype=U8)
    ks = (ops.decode_gemm_ws_bytes(1, N, K, w8=True) // (4 * N)) or 1
    cols = set(range(16)) | {63, 64, 65, 127, 128, 191, 192, 255, 256, K - 1, K - 16, K - 17}      # every byte of a load, the 64-byte lane groups
    cols |= {512 + 5, 1024 + 38, 1536 + 71, 2048 + 4, 2048 + 101, 2560 + 3, 4096 + 9, 4608 + 1}   # the other waves' chunks, a second and a third chunk
    assert ks == (8 if K == 8192 else 1), (N, K, ks)
    if ks > 1:
        Kc = K // ks
        for sp in range(1, ks):
            cols |= {sp * Kc - 1, sp * Kc}                                                         # both sides of every Kc boundary
        cols |= {Kc + 1, Kc + 17}
        assert all(sp * Kc - 1 in cols and sp * Kc in cols for sp in range(1, ks))
    cols = sorted(c for c in cols if 0 <= c < K)
    q = codes[torch.randint(0, 254, (N, K), generator=g)]
    q[1:, cols] = codes[torch.arange((N - 1) * len(cols)) % 254].view(N - 1, len(cols))            # every code at a column that is looked at
    q[0] = codes[(torch.arange(K) * 7) % 254]                                                      # and (K >= 254) every code in row 0
    assert set(q[:, cols].flatten().tolist()) == set(CODES) and (K < 254 or set(q[0].tolist()) == set(CODES))
    s = torch.exp2(torch.randint(-20, 10, (N,), generator=g).float())
    s[0], s[-1] = 2.0 ** -20, 2.0 ** 9
    assert len(torch.unique(s)) >= 8
    want = DC.quant().dequantize(q, s)                                             # [N, K] fp32: code x scale
    qd, sd = q.cuda(), s.cuda()
    for i in range(0, len(cols), 16):
        km = cols[i:i + 16]
        a = torch.zeros(len(km), K, dtype=BF)
        a[torch.arange(len(km)), torch.tensor(km)] = 1.0
        out = ops.decode_gemm(a.cuda(), qd, w_scale=sd, out_f32=True).cpu()
        exp = want[:, km].t().contiguous()
        assert torch.equal(out, exp), (N, K, km, (out != exp).nonzero()[:8].tolist())


@pytest.mark.parametrize("kind,K", [(kind, K) for kind in DC.KERNELS for K, _ in DC.K_TABLE[kind]])
def test_gemm_norm_prologue_on_the_chunk_paths(ops, kind, K):
    """fp32 out, N(0, 1) rows (integers do not survive the normalisation), lda > K, gamma 128 bytes into a larger buffer.  Per row against the
    fp64 product of vp_rmsnorm_fwd's rounding points restated in torch (decode_cases.norm_rows): fp32 output that sums K terms."""
    draw = dict(bf16="gaussbf", w8="gauss8", w4="gauss4")[kind]
    for M in DC.GEMM_MS:
        inp = DC.gemm_inputs(draw, M, DC.GEMM_N, K, seed=M)
        c = DC.gemm_call(kind, inp, device="cuda")
        out = run_gemm(ops, c, "f32", norm=True)
        assert out.outside_intact() and DC.inputs_unchanged(c)
        ref64, ref32 = DC.gemm_expected(inp, "f32", F64, norm=True), DC.gemm_expected(inp, "f32", F32, norm=True)
        check_bounded(f"{kind} norm prologue K={K} M={M}", DC.row_bounds(out.view, ref64, ref32, R.out_spec(n=K), M))
        assert DC.bits_equal(out.view, run_gemm(ops, DC.gemm_call(kind, inp, strided=False, device="cuda"), "f32", norm=True).view)


# ================================================================================================ 2. SwiGLU under split-K
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("N,K", DC.SWIGLU_SHAPES)
def test_swiglu_under_split_k(ops, N, K, norm):
    """The combine kernels' SwiGLU branch (ks = 4 / 8 for bf16, 2 / 4 for W8 and W4; test_split_factors_are_the_models).  Integer operands: the gate
    and up sums are exact under any split, the device silu is the only inexact step: r = 2 against fp64 (with the norm prologue the sums are
    not exact any more; the bound is the same).  IL and HALVES bit-equal on the same rows; without the prologue W8 and W4 bit-equal to the
    bf16 kernel although their splits differ (the sums are exact); ldc = N / 2 + 8 with the sentinel intact."""
    for M in DC.GEMM_MS:
        outs = {}
        for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
            inp = DC.swiglu_inputs(M, N, K, epi)
            ref64, ref32 = DC.swiglu_expected(inp, epi, F64, norm), DC.swiglu_expected(inp, epi, F32, norm)
            for kind in DC.KERNELS:
                c = DC.gemm_call(kind, inp, device="cuda", ncols=N // 2)
                out = run_gemm(ops, c, "bf16", epi=epi, norm=norm, ncols=N // 2)
                assert out.outside_intact() and DC.inputs_unchanged(c), (kind, epi, M)
                check_bounded(f"swiglu split-K {kind} epi={epi} norm={int(norm)} N={N} K={K} M={M}",
                              DC.row_bounds(out.view, ref64, ref32, R.out_spec(r=2), M))
                outs[kind, epi] = out.view.clone()
        for kind in DC.KERNELS:
            assert DC.bits_equal(outs[kind, DC.EPI_SWIGLU_IL], outs[kind, DC.EPI_SWIGLU_HALVES]), (kind, M)
            if not norm:
                assert DC.bits_equal(outs[kind, DC.EPI_SWIGLU_IL], outs["bf16", DC.EPI_SWIGLU_IL]), (kind, M)


# ================================================================================================ 3. FP8-cache attention at split boundaries
@pytest.mark.parametrize("D,Hq,Hkv", DC.ATTN_CONFIGS)
def test_decode_attn_kv8_split_boundaries_windows_strides(ops, D, Hq, Hkv):
    """test_decode_attn_split_boundaries_windows_strides on vp_decode_attn_kv8: lengths 0 / 1 / 511 / 512 / 513 / 1024 / 1536 in one batch,
    windows 0 / 1 / 512 / 4096, nsplit = 3 (a split of exactly 512 keys), 8 and 64, q / o rows 64 elements wider than Hq D, the byte caches
    and scales k|v-interleaved views as DecodeSession lays them out.  The cache comes from ops.quant_kv_e4m3; its values are taken from the
    bytes and scales in plain torch.  Per tensor 1e-3 of the tensor maximum; per sequence regimes.bound(out_spec(r = 1)) against fp64; length
    0: exact zeros; window 1: the dequantised v row at len - 1 exactly, from the byte kernel and from the bf16 kernel on the dequantised
    cache; each nsplit bit-identical run to run."""
    lens = DC.ATTN_LENS
    B, Smax, C = len(lens), max(lens), 2 * Hkv * D
    x, q = DC.attn_source(D, Hq, Hkv, lens)
    kvq = torch.full((B, Smax, 2, Hkv * D), 0xAB, device="cuda", dtype=U8)
    kvs = torch.full((B, Smax, 2, Hkv), 123.0, device="cuda", dtype=F32)
    kvd = torch.full((B, Smax, 2, Hkv * D), 7.0, device="cuda", dtype=BF)
    ops.quant_kv_e4m3(x.cuda().view(B * Smax, C), D, q_out=kvq.view(B * Smax, C), scale_out=kvs.view(B * Smax, 2 * Hkv), deq_out=kvd.view(B * Smax, C))
    kb, vb, ksc, vsc = kvq[:, :, 0].cpu(), kvq[:, :, 1].cpu(), kvs[:, :, 0].cpu(), kvs[:, :, 1].cpu()
    vdeq = DC.kv_dequant(vb, vsc, D)                                                     # [B, Smax, Hkv, D]
    assert torch.equal(vdeq.flatten(-2), kvd[:, :, 1].cpu().float())
    vlast = torch.stack([vdeq[b, max(L, 1) - 1] for b, L in enumerate(lens)]).repeat_interleave(Hq // Hkv, 1)
    q_buf = torch.zeros(B, Hq * D + 64, dtype=BF)
    q_buf[:, :Hq * D] = q
    qd = q_buf.cuda()[:, :Hq * D]
    k4, v4 = kvq[:, :, 0].unflatten(-1, (Hkv, D)), kvq[:, :, 1].unflatten(-1, (Hkv, D))
    kl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    q3 = q.view(B, Hq, D)
    fails = []
    for window in DC.ATTN_WINDOWS:
        want = DC.attn_sim(q3, kb, ksc, vb, vsc, lens, window, 1)
        y32 = DC.attn_sim(q3, kb, ksc, vb, vsc, lens, window, 1, F32)
        for ns in DC.attn_nsplits(Smax):
            o_buf = torch.full((B, Hq * D + 64), 7.0, device="cuda", dtype=BF)
            ops.decode_attn_kv8(qd, k4, v4, kvs[:, :, 0], kvs[:, :, 1], kl, Hq, window=window, nsplit=ns, out=o_buf[:, :Hq * D])
            assert bool((o_buf[:, Hq * D:] == 7.0).all()), (window, ns)
            got = o_buf[:, :Hq * D]
            assert torch.equal(got, ops.decode_attn_kv8(qd, k4, v4, kvs[:, :, 0], kvs[:, :, 1], kl, Hq, window=window, nsplit=ns)), (window, ns)
            v = DC.attn_verify(got.cpu().reshape(B, Hq, D), want, y32, lens, window, vlast)
            for name, (e, b) in v.bounded.items():
                try:
                    parity.check(f"decode edges attn_kv8 D={D} {Hq}:{Hkv} window={window} nsplit={ns} [{name}]", e, b)
                except AssertionError as ex:
                    fails.append(str(ex))
            for name, e in v.info.items():
                parity.log(f"decode edges attn_kv8 D={D} {Hq}:{Hkv} window={window} nsplit={ns} [{name}]", e)
            fails += [f"window={window} nsplit={ns} {name}: not exact" for name, ok in v.exact.items() if not ok]
            if window == 1:                                                              # the bf16 kernel on the dequantised cache: the same rows
                par = ops.decode_attn(qd, kvd[:, :, 0].unflatten(-1, (Hkv, D)), kvd[:, :, 1].unflatten(-1, (Hkv, D)), kl, Hq, window=1, nsplit=ns)
                for b, L in enumerate(lens):
                    assert torch.equal(par[b].cpu().float().view(Hq, D), vlast[b] if L else torch.zeros(Hq, D)), ("bf16 kernel", ns, L)
    assert not fails, "\n".join(fails)


# ================================================================================================ 4. cache writers and weight quantisers
@pytest.mark.parametrize("D", DC.QUANT_KV_DS)
def test_quant_kv_head_dims_and_padded_rows(ops, D):
    """lph = 2 (D = 8, 16), idle lanes (D = 24, 40, 72, 120), D = 64; heads 1 / 3 / 6; n = 37 into padded row views of sentinel caches: bit-equal
    to quant.quantize_kv_heads / dequantize_kv_heads, every other byte, scale and bf16 element unchanged, the source bit-unchanged"""
    Q = DC.quant()
    for heads in DC.QUANT_KV_HEADS:
        n, C = 37, heads * D
        x = DC.quant_kv_source(n, heads, D)
        src = DC.Box(n, C, C + 16, fill=x, device="cuda")
        qb = DC.Box(n, C, C + 8, dtype=U8, device="cuda")
        sb = DC.Box(n, heads, heads + 3, dtype=F32, device="cuda")
        db = DC.Box(n, C, C + 8, device="cuda")
        ops.quant_kv_e4m3(src.view, D, q_out=qb.view, scale_out=sb.view, deq_out=db.view)
        want_q, want_s = Q.quantize_kv_heads(x, heads, D)
        assert src.unchanged() and qb.outside_intact() and sb.outside_intact() and db.outside_intact(), (D, heads)
        assert torch.equal(qb.view.cpu(), want_q) and torch.equal(sb.view.cpu(), want_s), (D, heads)
        assert torch.equal(db.view.cpu().float(), Q.dequantize_kv_heads(want_q, want_s, heads, D)), (D, heads)
        assert float(want_s[4, 0]) == 1.0 and len(torch.unique(want_s)) >= 6              # the zero head; the scales did differ


def test_quant_kv_second_sweep(ops):
    """n = 1100, heads = 64, D = 96: 1 126 400 lane slots against the grid cap of 4096 x 256, so rows >= 1024 are written by a block's second
    pass (Phi-3 prompts longer than 1024 tokens).  Those rows are compared as their own group: a kernel that stops after one sweep fails by name."""
    sw = DC.QUANT_KV_SWEEP
    C = sw.heads * sw.D
    x = DC.quant_kv_source(sw.n, sw.heads, sw.D)
    qb = torch.full((sw.n, C), 0xAB, device="cuda", dtype=U8)
    sb = torch.full((sw.n, sw.heads), 123.0, device="cuda", dtype=F32)
    db = torch.full((sw.n, C), 7.0, device="cuda", dtype=BF)
    ops.quant_kv_e4m3(x.cuda(), sw.D, q_out=qb, scale_out=sb, deq_out=db)
    want_q, want_s = DC.quant().quantize_kv_heads(x, sw.heads, sw.D)
    want_d = DC.quant().dequantize_kv_heads(want_q, want_s, sw.heads, sw.D)
    for name, rows in (("first sweep", slice(0, 1024)), ("second sweep (rows >= 1024)", slice(1024, None))):
        assert DC.quant_kv_verify(qb.cpu(), sb.cpu(), x, sw.heads, sw.D, rows=rows), name
        assert torch.equal(db[rows].cpu().float(), want_d[rows]), name


def _sweep_inputs(ops, B, Hq, Hkv, D, Smax):
    g = torch.Generator().manual_seed(B)
    qkv = torch.randn(B, Hq + 2 * Hkv, D, generator=g) * torch.exp2(torch.randint(-6, 7, (B, Hq + 2 * Hkv, 1), generator=g).float())
    qkv = qkv.view(B, -1).to(BF).cuda()
    pos = torch.tensor([0, 1, 2, 3, -1, Smax], dtype=torch.int32)[torch.arange(B) % 6].cuda()
    cos, sin = ops.rope_tables(64, D, 10000.0, "cuda")
    want = qkv.clone()                                                                   # the training vp_rope with position ids
    ops.rope_(want, B, 64, Hq + Hkv, D, cos, sin, pos=pos.clamp(0, Smax - 1))
    valid = (pos >= 0) & (pos < Smax)
    return qkv, pos, cos, sin, want, valid


SWEEP = dict(Hq=32, Hkv=8, D=128, Smax=4)


def test_decode_rope_append_second_sweep(ops):
    """B = 1200: 537 600 work items against the grid cap of 2048 x 256; sequences >= 1171 are reached only by a block's second pass.  Positions
    cycle through 0 .. 3, -1 and Smax: row pos[b] holds vp_rope's k and the projected v, rows of out-of-range positions and all other rows are
    bit-unchanged, q is written for every b."""
    B, (Hq, Hkv, D, Smax) = 1200, SWEEP.values()
    assert B * ((Hq + Hkv) * (D // 16) + Hkv * (D // 8)) > 2048 * 256
    qkv, pos, cos, sin, want, valid = _sweep_inputs(ops, B, Hq, Hkv, D, Smax)
    qkv0 = qkv.clone()
    cache = torch.full((B, Smax, 2, Hkv * D), 7.0, device="cuda", dtype=BF)
    q = torch.full((B, Hq * D), float("nan"), device="cuda", dtype=BF)
    ops.decode_rope_append(qkv, q, cache[:, :, 0].unflatten(-1, (Hkv, D)), cache[:, :, 1].unflatten(-1, (Hkv, D)), cos, sin, pos, Hq, Hkv, D)
    exp = torch.full_like(cache, 7.0)
    bi = valid.nonzero()[:, 0]
    exp[bi, pos[bi].long(), 0] = want[bi, Hq * D:(Hq + Hkv) * D]
    exp[bi, pos[bi].long(), 1] = qkv0[bi, (Hq + Hkv) * D:]
    first = 2048 * 256 // ((Hq + Hkv) * (D // 16) + Hkv * (D // 8))                      # 1170: the last sequence the first pass reaches
    for name, rows in (("first sweep", slice(0, first)), ("second sweep", slice(first + 1, None)), ("all", slice(None))):
        assert torch.equal(cache[rows], exp[rows]), name
        assert torch.equal(q[rows][valid[rows]], want[rows][valid[rows]][:, :Hq * D]), name
    assert bool(torch.isfinite(q.float()).all()) and torch.equal(qkv, qkv0)


def test_decode_rope_append_kv8_second_sweep(ops):
    """B = 1400: 537 600 lane slots against 2048 x 256; sequences >= 1366 belong to the second pass.  Row pos[b] holds quant.quantize_kv_heads of
    vp_rope's k row and of the v row (bytes, scales, dequantised bf16), everything else is bit-unchanged, q is vp_rope's for every valid b."""
    Q = DC.quant()
    B, (Hq, Hkv, D, Smax) = 1400, SWEEP.values()
    assert B * (Hq + 2 * Hkv) * 8 > 2048 * 256
    qkv, pos, cos, sin, want, valid = _sweep_inputs(ops, B, Hq, Hkv, D, Smax)
    qkv0 = qkv.clone()
    qc = torch.full((B, Smax, 2, Hkv * D), 0xAB, device="cuda", dtype=U8)
    sc = torch.full((B, Smax, 2, Hkv), 123.0, device="cuda", dtype=F32)
    dc = torch.full((B, Smax, 2, Hkv * D), 7.0, device="cuda", dtype=BF)
    k4 = lambda t: t[:, :, 0].unflatten(-1, (Hkv, D))
    v4 = lambda t: t[:, :, 1].unflatten(-1, (Hkv, D))
    q = torch.full((B, Hq * D), float("nan"), device="cuda", dtype=BF)
    ops.decode_rope_append_kv8(qkv, q, cos, sin, pos, Hq, Hkv, D, k_bytes=k4(qc), v_bytes=v4(qc), k_scale=sc[:, :, 0], v_scale=sc[:, :, 1],
                               k_deq=k4(dc), v_deq=v4(dc))
    eq, es, ed = torch.full_like(qc, 0xAB).cpu(), torch.full_like(sc, 123.0).cpu(), torch.full_like(dc, 7.0).cpu()
    bi = valid.nonzero()[:, 0].cpu()
    pi = pos.cpu()[bi].long()
    for kv, rows in ((0, want[:, Hq * D:(Hq + Hkv) * D]), (1, qkv0[:, (Hq + Hkv) * D:])):
        wq, ws = Q.quantize_kv_heads(rows.cpu().contiguous(), Hkv, D)
        eq[bi, pi, kv], es[bi, pi, kv] = wq[bi], ws[bi]
        ed[bi, pi, kv] = Q.dequantize_kv_heads(wq, ws, Hkv, D)[bi].to(BF)
    first = 2048 * 256 // ((Hq + 2 * Hkv) * 8)                                            # 1365
    qcc, scc, dcc = qc.cpu(), sc.cpu(), dc.cpu()
    for name, rows in (("first sweep", slice(0, first)), ("second sweep", slice(first + 1, None)), ("all", slice(None))):
        assert torch.equal(qcc[rows], eq[rows]) and torch.equal(scc[rows], es[rows]) and torch.equal(dcc[rows].float(), ed[rows].float()), name
        assert torch.equal(q[rows][valid[rows]], want[rows][valid[rows]][:, :Hq * D]), name
    assert bool(torch.isfinite(q.float()).all()) and torch.equal(qkv, qkv0)


@pytest.mark.parametrize("N,K", [(136, 80), (40, 2064)])
@pytest.mark.parametrize("writeback", [0, 1])
def test_quant_rows_e4m3_strided_source_and_padded_destination(ops, N, K, writeback):
    """vp_quant_rows_e4m3 through the library entry (ops.quant_rows_e4m3 always passes ldq = K): ldw = K + 8, ldq = K + 8"""
    Q = DC.quant()
    w = (torch.randn(N, K, generator=R.gen(K)) * torch.exp2(torch.randint(-8, 9, (N, 1), generator=R.gen(K + 1)).float())).to(BF)
    w[3] = 0
    wbx = DC.Box(N, K, K + 8, fill=w, device="cuda")
    qb = DC.Box(N, K, K + 8, dtype=U8, device="cuda")
    sc = torch.full((N + 2,), 123.0, device="cuda")
    ops._lib.call("vp_quant_rows_e4m3", N, K, ops._p(wbx.view), wbx.ld, ops._p(qb.view), qb.ld, ops._p(sc), writeback, ops._stream())
    want_q, want_s = Q.quantize_rows_pow2(w)
    assert torch.equal(qb.view.cpu(), want_q) and torch.equal(sc[:N].cpu(), want_s) and bool((sc[N:] == 123.0).all())
    assert qb.outside_intact() and wbx.outside_intact()
    assert torch.equal(wbx.view.cpu().float(), Q.dequantize(want_q, want_s)) if writeback else wbx.unchanged()


@pytest.mark.parametrize("N,K", [(136, 96), (40, 2080)])
@pytest.mark.parametrize("writeback", [0, 1])
def test_quant_blocks_mxfp4_strided_source_and_padded_destinations(ops, N, K, writeback):
    """vp_quant_blocks_mxfp4 through the library entry: ldw = K + 8, ldq = K / 2 + 16 bytes, lde = K / 32 + 3"""
    Q = DC.quant()
    w = (torch.randn(N, K // 32, 32, generator=R.gen(K)) * torch.exp2(torch.randint(-8, 9, (N, K // 32, 1), generator=R.gen(K + 1)).float()))
    w = w.view(N, K).to(BF)
    w[3, :32] = 0
    wbx = DC.Box(N, K, K + 8, fill=w, device="cuda")
    qb = DC.Box(N, K // 2, K // 2 + 16, dtype=U8, device="cuda")
    eb = DC.Box(N, K // 32, K // 32 + 3, dtype=U8, device="cuda")
    ops._lib.call("vp_quant_blocks_mxfp4", N, K, ops._p(wbx.view), wbx.ld, ops._p(qb.view), qb.ld, ops._p(eb.view), eb.ld, writeback, ops._stream())
    want_q, want_e = Q.quantize_blocks_mxfp4(w)
    assert torch.equal(qb.view.cpu(), want_q) and torch.equal(eb.view.cpu(), want_e)
    assert qb.outside_intact() and eb.outside_intact() and wbx.outside_intact()
    assert torch.equal(wbx.view.cpu().float(), Q.dequantize_mxfp4(want_q, want_e)) if writeback else wbx.unchanged()
