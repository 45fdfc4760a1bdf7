"""CPU proof behind tests/test_decode_edges_gpu.py (no GPU, no built library).

1. The case tables enter what they claim: the chunk-path model of decode_cases.py over each skinny GEMM's K list covers every kind of step,
   and the split factors are the ones tests/DECODE_PATHS.md states.
2. The references are torch's own operators / quant.py plus the stated rounding points, and the exact draws keep their promise.
3. The comparison made on the GPU accepts the reference in the role of an honest kernel and rejects every mutant on the case aimed at it.
4. OLD_CATCHES: whether the parent's comparison on the parent's inputs (dense contiguous operands, the models' own K, max_rel 5e-3; the
   cache tests' lengths and head dims) sees each mutant."""
import pytest
import torch
import torch.nn.functional as F

import decode_cases as DC
import regimes as R
from decode_cases import BF, F32, F64, I64
from parity import max_rel


# ------------------------------------------------------------------------------------------------ 1. the tables enter what they claim
@pytest.mark.parametrize("kind", DC.KERNELS)
def test_k_table_covers_every_chunk_kind(kind):
    got, other = DC.coverage(kind, DC.K_TABLE[kind])
    assert got == DC.required_kinds(), (kind, got)
    assert other, "no partial chunk in a wave other than wave 0"
    for K, ks in DC.K_TABLE[kind]:
        assert DC.ksplit(kind, DC.GEMM_N, K) == ks, (kind, K)
    # drop any one of the unsplit K values that carries a kind alone and the table no longer covers
    alone = [i for i in range(len(DC.K_TABLE[kind]))
             if DC.coverage(kind, DC.K_TABLE[kind][:i] + DC.K_TABLE[kind][i + 1:]) != (DC.required_kinds(), True)]
    assert alone, "no K value is needed: the coverage assertion cannot fail"


def test_the_chunk_kinds_the_issue_names():
    for kind, k_other, k_next2, k_third in (("w8", 528, 2064, 4656), ("w4", 544, 2080, 4640)):
        p = DC.chunk_paths(kind, k_other, 1)
        assert p.partial_other == [(512, k_other)] and "idle" in p.kinds and ("step", True, 0, 1) in p.kinds      # wave 1 partial, waves 2, 3 idle
        p = DC.chunk_paths(kind, k_next2, 1)
        assert ("step", True, 2, 1) in p.kinds and ("step", False, 0, 2) in p.kinds and p.next2
        p = DC.chunk_paths(kind, k_third, 1)
        assert ("step", True, 0, 3) in p.kinds and ("step", False, 0, 3) in p.kinds
    p = DC.chunk_paths("w8", 8192, 8)
    assert p.Kc == 1024 and p.kinds == {"idle", ("first", True), ("step", True, 0, 1)}


def test_swiglu_shapes_split():
    for N, K in DC.SWIGLU_SHAPES:
        for kind in DC.KERNELS:
            for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
                assert DC.ksplit(kind, N, K, epi) == DC.SWIGLU_KS[kind][K] > 1


# ------------------------------------------------------------------------------------------------ 2. the references
@pytest.mark.parametrize("draw,K", [("w8", 2592), ("w4", 2592), ("w8", 80), ("w4", 160)])
def test_exact_draws_are_what_every_format_holds(draw, K):
    Q = DC.quant()
    inp = DC.gemm_inputs(draw, 5, 40, K)
    assert torch.equal(Q.dequantize(inp.q8, inp.s8).double(), inp.w)
    if K % 32 == 0:
        assert torch.equal(Q.dequantize_mxfp4(inp.q4, inp.e4).double(), inp.w)
    # the int64 product, the fp64 and the fp32 restatement agree bit for bit, also when the fp32 sum is taken in pieces in another order
    want = (inp.a.to(I64) @ (inp.w * 16).to(I64).t()).double() / 16
    ex = DC.exact_outputs(inp)
    assert torch.equal(ex["f32"].double(), want)
    assert torch.equal(DC.gemm_expected(inp, "f32", F32).double(), want) and torch.equal(DC.gemm_expected(inp, "f32", F64), want)
    a, w = inp.a.float(), inp.w.float()
    pieces = sum((a[:, k:k + 16] @ w[:, k:k + 16].t() for k in reversed(range(0, K, 16))), torch.zeros(5, 40))
    assert torch.equal(pieces.double(), want)
    assert torch.equal(ex["bf16"], want.to(BF)) and torch.equal(ex["res"], (want.to(BF).double() + inp.res.double()).to(BF))
    assert torch.equal(DC.gemm_expected(inp, "res", F64).to(BF), ex["res"])


def test_the_exactness_condition_is_asserted():
    """row scales of 2^14 .. 2^20 would push partial sums past 2^20, scales of 2^-8 .. 2^-2 leave the multiples of 2^-4: the generator refuses
    both, and takes the scales of the tables"""
    for off in (17, -5):
        with pytest.raises(AssertionError, match="exactness condition"):
            DC.gemm_inputs("w8", 5, 40, 2592, exp_offset=off)
    DC.gemm_inputs("w8", 5, 40, 2592, exp_offset=0)


def test_norm_silu_and_swiglu_references():
    inp = R.rmsnorm_inputs(64)
    for dt in (F32, F64):
        assert torch.equal(DC.norm_rows(inp.x, inp.w, inp.eps, dt), R.bfr(R.rmsnorm_ref(inp, dt)["y"]))
    # against torch's own operator in fp64 only: in fp32 torch may sum in another order, and the line above covers both
    y = F.rms_norm(inp.x.double(), (64,), None, inp.eps)
    assert torch.equal(DC.norm_rows(inp.x, inp.w, inp.eps, F64), R.bfr(inp.w.double() * R.bfr(y)))
    x = torch.linspace(-20, 20, 401, dtype=F64)
    assert bool(((DC.silu(x) - F.silu(x)).abs() <= 2 * torch.finfo(F64).eps * F.silu(x).abs()).all())      # two fp64 ulps
    si = R.swiglu_inputs()
    assert torch.equal(DC.swiglu_store(si.gate.double(), si.up.double(), last_round=False), R.swiglu_ref(si, F64)["act"])
    # the two layouts read the same rows
    for N in (32, 256):
        rows = torch.arange(N)
        for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
            rg, ru = DC.swiglu_rows(N, epi)
            lay = DC.to_layout(rows, epi)
            assert torch.equal(lay[rg], torch.arange(N // 2)) and torch.equal(lay[ru], torch.arange(N // 2) + N // 2)


def _host_attn(D=32, Hq=4, Hkv=2, lens=DC.ATTN_LENS, spikes=True):
    Q = DC.quant()
    x, q = DC.attn_source(D, Hq, Hkv, lens, spikes=spikes)
    B, Smax = x.shape[:2]
    qb, sc = Q.quantize_kv_heads(x.view(B * Smax, 2 * Hkv * D), 2 * Hkv, D)
    qb, sc = qb.view(B, Smax, 2, Hkv * D), sc.view(B, Smax, 2, Hkv)
    return R.NS(q=q.view(B, Hq, D), kb=qb[:, :, 0], vb=qb[:, :, 1], ks=sc[:, :, 0], vs=sc[:, :, 1], lens=lens, D=D, Hq=Hq, Hkv=Hkv, x=x)


ATT = _host_attn()


def test_attention_reference_is_torchs_softmax_attention():
    c = ATT
    k, v = DC.kv_dequant(c.kb, c.ks, c.D).double(), DC.kv_dequant(c.vb, c.vs, c.D).double()
    assert torch.equal(k.flatten(-2).float(), DC.quant().dequantize_kv_heads(c.kb.reshape(-1, c.Hkv * c.D), c.ks.reshape(-1, c.Hkv), c.Hkv, c.D).view(k.shape[0], -1, c.Hkv * c.D))
    want = DC.attn_sim(c.q, c.kb, c.ks, c.vb, c.vs, c.lens, 0, 3)
    for b, L in enumerate(c.lens):
        if L == 0:
            assert not want[b].any()
            continue
        kk = k[b, :L].repeat_interleave(c.Hq // c.Hkv, 1).transpose(0, 1)[None]
        vv = v[b, :L].repeat_interleave(c.Hq // c.Hkv, 1).transpose(0, 1)[None]
        o = F.scaled_dot_product_attention(c.q[b].double()[None, :, None], kk, vv)[0, :, 0]
        assert float((o - want[b]).abs().max()) <= 1e-12 * float(o.abs().max())
    # the window keeps the last `window` keys; the split count does not enter the honest reference
    w512 = DC.attn_sim(c.q, c.kb, c.ks, c.vb, c.vs, c.lens, 512, 64)
    b = c.lens.index(1536)
    kk = k[b, 1024:1536].repeat_interleave(c.Hq // c.Hkv, 1).transpose(0, 1)[None]
    vv = v[b, 1024:1536].repeat_interleave(c.Hq // c.Hkv, 1).transpose(0, 1)[None]
    o = F.scaled_dot_product_attention(c.q[b].double()[None, :, None], kk, vv)[0, :, 0]
    assert float((o - w512[b]).abs().max()) <= 1e-12 * float(o.abs().max())
    assert float(ATT.x[c.lens.index(1), 0, c.Hkv:].float().abs().max()) >= 512.0           # the one-key v row carries exponent 9


# ------------------------------------------------------------------------------------------------ 3. honest accepted, mutants rejected
def _gemm_verdicts(kind, draw, M, N, K, mut, outs=("f32", "bf16", "res"), **lay):
    inp = DC.gemm_inputs(draw, M, N, K)
    c = DC.gemm_call(kind, inp, **lay)
    want = DC.exact_outputs(inp)
    return {ko: DC.verify_exact(DC.gemm_sim(c, ko, mut=mut), want[ko]) for ko in outs}, c


# mutant -> the (kind, draw, K, layout) aimed at it
GEMM_TARGETS = {
    "next2_reread_not_zeroed": [("w8", "w8", 2064, {}), ("w4", "w4", 2080, {})],
    "partial_chunk_of_other_wave_dropped": [("w8", "w8", 528, {}), ("w4", "w4", 544, {}), ("bf16", "w8", 264, {})],
    "w8_scale_after_rounding": [("w8", "w8", 528, {})],
    "ldw_ignored": [("bf16", "w8", 264, {}), ("w8", "w8", 528, {}), ("w4", "w4", 544, {})],
    "lde_ignored": [("w4", "w4", 544, dict(lde=DC.lde_padded(544))), ("w4", "w4", 2592, dict(lde=DC.lde_padded(2592)))],
    "ldr_ignored": [("w8", "w8", 528, {}), ("w4", "w4", 544, {}), ("bf16", "w8", 264, {})],
    "w4_byte_path_neighbour_scale": [("w4", "w4", 1024, dict(lde=DC.lde_padded(1024), e_off=1))],
    "n_tail_stored_past_n": [("w8", "w8", 528, {}), ("w4", "w4", 544, {}), ("bf16", "w8", 264, {})],
}


@pytest.mark.parametrize("kind", DC.KERNELS)
def test_honest_gemm_is_accepted_on_every_case(kind):
    draw = "w4" if kind == "w4" else "w8"
    for K, _ in DC.K_TABLE[kind]:
        for M in DC.GEMM_MS:
            for lay in ({}, dict(strided=False)) + ((dict(lde=DC.lde_padded(K)),) if kind == "w4" else ()):
                v, c = _gemm_verdicts(kind, draw, M, DC.GEMM_N, K, None, **lay)
                assert not any(DC.rejected(x) for x in v.values()), (kind, K, M, lay)
                assert DC.inputs_unchanged(c)
    v, _ = _gemm_verdicts(kind, draw, 5, *DC.ONE_TILE, None)
    assert not any(DC.rejected(x) for x in v.values())
    if kind == "w4":
        for K in DC.W4_MISALIGNED_E:
            v, c = _gemm_verdicts(kind, draw, 5, DC.GEMM_N, K, None, lde=DC.lde_padded(K), e_off=1)
            assert not DC.evec_of(c) and c.e.ld % 16 == 0 and c.e.view.data_ptr() % 16 == 1
            assert not any(DC.rejected(x) for x in v.values())


@pytest.mark.parametrize("mut", DC.GEMM_MUTANTS)
def test_gemm_mutant_is_rejected_on_its_case(mut):
    for kind, draw, K, lay in GEMM_TARGETS[mut]:
        for M in DC.GEMM_MS[1 if mut == "ldr_ignored" else 0:]:          # one row has no row stride
            v, _ = _gemm_verdicts(kind, draw, M, DC.GEMM_N, K, mut, **lay)
            if mut == "n_tail_stored_past_n":                      # caught by the sentinel only
                assert all(not x.outside and x.exact for x in v.values()), (mut, kind, K, M)
            elif mut in ("w8_scale_after_rounding", "ldr_ignored"):
                assert DC.rejected(v["res"]) and not DC.rejected(v["f32"]), (mut, kind, K, M)
            else:
                assert all(DC.rejected(x) for x in v.values()), (mut, kind, K, M, v)


def _swiglu_verdict(kind, M, N, K, epi, norm, mut):
    inp = DC.swiglu_inputs(M, N, K, epi)
    c = DC.gemm_call(kind, inp, ncols=N // 2)
    out = DC.swiglu_sim(c, epi, norm, mut)
    ref64, ref32 = DC.swiglu_expected(inp, epi, F64, norm), DC.swiglu_expected(inp, epi, F32, norm)
    rb = DC.row_bounds(out.view, ref64, ref32, R.out_spec(r=2), M)
    return out, all(e <= b for e, b in rb.values()) and out.outside_intact()


@pytest.mark.parametrize("norm", [False, True])
def test_swiglu_split_k_honest_accepted_mutants_rejected(norm):
    N, K = DC.SWIGLU_SHAPES[0]
    for kind in DC.KERNELS:
        outs = {}
        for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
            for M in DC.GEMM_MS:
                outs[epi, M], ok = _swiglu_verdict(kind, M, N, K, epi, norm, None)
                assert ok, (kind, epi, M)
        assert all(torch.equal(outs[DC.EPI_SWIGLU_IL, M].view, outs[DC.EPI_SWIGLU_HALVES, M].view) for M in DC.GEMM_MS)
        assert not _swiglu_verdict(kind, 5, N, K, DC.EPI_SWIGLU_HALVES, norm, "halves_up_row_interleaved")[1], kind
        # the wrong up row is also a difference between the two layouts
        assert not torch.equal(_swiglu_verdict(kind, 5, N, K, DC.EPI_SWIGLU_HALVES, norm, "halves_up_row_interleaved")[0].view, outs[DC.EPI_SWIGLU_IL, 5].view)
    for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
        assert not _swiglu_verdict("w8", 5, N, K, epi, norm, "w8_gate_scale_on_up")[1], epi


def _attn_verdict(c, window, nsplit, mut, lens=None):
    lens = c.lens if lens is None else lens
    got = DC.attn_sim(c.q, c.kb, c.ks, c.vb, c.vs, lens, window, nsplit, F32, mut).to(BF)
    want = DC.attn_sim(c.q, c.kb, c.ks, c.vb, c.vs, lens, window, nsplit)
    y32 = DC.attn_sim(c.q, c.kb, c.ks, c.vb, c.vs, lens, window, nsplit, F32)
    v = DC.kv_dequant(c.vb, c.vs, c.D)
    vlast = torch.stack([v[b, max(L, 1) - 1] for b, L in enumerate(lens)]).repeat_interleave(c.Hq // c.Hkv, 1)
    return DC.attn_verify(got, want, y32, lens, window, vlast)


def test_attention_honest_accepted_mutants_rejected():
    seen = {m: set() for m in DC.ATTN_MUTANTS}
    for window in DC.ATTN_WINDOWS:
        for ns in DC.attn_nsplits(max(ATT.lens)):
            assert not DC.attn_rejected(_attn_verdict(ATT, window, ns, None)), (window, ns)
            for m in DC.ATTN_MUTANTS:
                if DC.attn_rejected(_attn_verdict(ATT, window, ns, m)):
                    seen[m].add((window, ns))
    assert len(seen["v_scale_of_next_token"]) == 12                                       # everywhere
    # the window-1 row equality sees this mutant under every nsplit (one ordinary key more among 512 is below the output's bf16 rounding;
    # at window 512 it is the spike key at 1023 entering the longest sequence's window that the bound sees)
    assert {(1, ns) for ns in DC.attn_nsplits(max(ATT.lens))} <= seen["window_lower_bound_off_by_one"]
    assert seen["last_key_of_full_split_dropped"] and {ns for _, ns in seen["last_key_of_full_split_dropped"]} == {3}      # only 512-key splits
    assert len(seen["length_zero_gives_nan"]) == 12


@pytest.mark.parametrize("D", DC.QUANT_KV_DS)
def test_quant_kv_small_cases_accept_the_contract_and_see_the_lane_mutants(D):
    for heads in DC.QUANT_KV_HEADS:
        x = DC.quant_kv_source(37, heads, D)
        src = DC.Box(37, heads * D, heads * D + 16, fill=x)
        q, s, w = DC.quant_kv_sim(src, heads, D)
        assert w.all() and DC.quant_kv_verify(q, s, x, heads, D)
        lph = DC.quant_kv_lph(D)
        if D > 8:
            q, s, _ = DC.quant_kv_sim(src, heads, D, "absmax_over_half_the_lanes")
            assert not DC.quant_kv_verify(q, s, x, heads, D), (D, heads)
        if lph * 8 > D:
            q, s, _ = DC.quant_kv_sim(src, heads, D, "idle_lanes_stale")
            assert not DC.quant_kv_verify(q, s, x, heads, D), (D, heads)
    assert {D: DC.quant_kv_lph(D) for D in DC.QUANT_KV_DS} == {8: 2, 16: 2, 24: 4, 40: 8, 64: 8, 72: 16, 120: 16}


def test_quant_kv_second_sweep_is_its_own_group():
    sw = DC.QUANT_KV_SWEEP
    lph = DC.quant_kv_lph(sw.D)
    assert sw.n * sw.heads * lph > sw.blocks * 256 and sw.blocks * 256 // (sw.heads * lph) == 1024
    x = DC.quant_kv_source(sw.n, sw.heads, sw.D)
    src = DC.Box(sw.n, sw.heads * sw.D, fill=x)
    q, s, w = DC.quant_kv_sim(src, sw.heads, sw.D, "first_sweep_only")
    q = torch.where(w.repeat_interleave(sw.D, 1), q, torch.full_like(q, 0xAB))
    assert torch.equal(w.all(1), torch.arange(sw.n) < 1024)
    assert DC.quant_kv_verify(q, s, x, sw.heads, sw.D, rows=slice(0, 1024))
    assert not DC.quant_kv_verify(q, s, x, sw.heads, sw.D, rows=slice(1024, None))


# ------------------------------------------------------------------------------------------------ 4. the parent's tests
# mutant -> does the parent's suite notice it?  Its calls of these kernels, by what matters here: dense contiguous operands (ld = the row length,
# every base at the start of its allocation), N(0, 1) data, K in {128, 256, 3072, 4096, 8192, 14336} (whole chunks, or one partial chunk in
# wave 0), max_rel 5e-6 (fp32) / 5e-3 (bf16) per tensor; SwiGLU only where K is not split; the W4 one-hot test at (40, 160) and (24, 2144) with
# tight scale rows (the byte path); the byte attention at lengths 1 / 2 / 33 / 777 / 2100 under the default nsplit with windows 0 and 500, and one
# code per token at Smax = 4; quant_kv at n = 37 and D in {32, 96, 128}.
OLD_CATCHES = {
    # the GEMM mutants: the set of kernels on which the parent sees them
    "next2_reread_not_zeroed": {"w4"},               # the W4 one-hot test's K = 2144 has a whole chunk followed by a partial one; no W8 K has
    "partial_chunk_of_other_wave_dropped": set(),    # K = 128 / 256 / 160 / 2144: the partial chunk is wave 0's
    "w8_scale_after_rounding": {"w8"},               # random residuals at 5e-3
    "halves_up_row_interleaved": False,              # the combine kernels' SwiGLU branch never runs
    "w8_gate_scale_on_up": False,
    "ldw_ignored": set(),                            # ld == row length everywhere
    "lde_ignored": set(),
    "ldr_ignored": set(),
    "w4_byte_path_neighbour_scale": {"w4"},          # the one-hot test's tight scale rows take the byte path
    "n_tail_stored_past_n": set(),                   # nothing looks beside the output
    "v_scale_of_next_token": True,
    "window_lower_bound_off_by_one": True,           # one code per token: window 1 at kv_len 3 and 4
    "last_key_of_full_split_dropped": False,         # no split holds 512 keys
    "length_zero_gives_nan": False,                  # no length 0
    "first_sweep_only": False,                       # n = 37
    "absmax_over_half_the_lanes": True,              # D = 96 / 128 with random data
    "idle_lanes_stale": True,                        # D = 96 leaves 4 of 16 lanes idle
}
OLD_TOL = dict(f32=5e-6, bf16=5e-3, res=5e-3)


def _old_gemm_rejects(mut):
    hit = set()
    for kind, draw in (("bf16", "gaussbf"), ("w8", "gauss8"), ("w4", "gauss4")):
        for K in (128, 256, 3072):
            inp = DC.gemm_inputs(draw, 5, DC.GEMM_N, K, seed=K)
            c = DC.gemm_call(kind, inp, strided=False)
            for ko, tol in OLD_TOL.items():
                want = DC.gemm_expected(inp, ko, F32)
                assert max_rel(DC.gemm_sim(c, ko).view, want) <= tol
                if not max_rel(DC.gemm_sim(c, ko, mut=mut).view, want) <= tol:
                    hit.add(kind)
    # test_decode_gemm_w4_one_hot_products_are_exact: tight scale rows
    for N, K in ((40, 160), (24, 2144)):
        inp = DC.gemm_inputs("w4", 16, N, K, seed=K)
        inp.a = torch.zeros(16, K, dtype=BF)
        cols = [0, 31, 32, 33, 63, 64, 127, 128, K - 1, K - 2, K - 32, K - 33, 5, 17, 100, 150][:16]
        inp.a[torch.arange(16), torch.tensor(cols)] = 1.0
        c = DC.gemm_call("w4", inp, strided=False)
        want = inp.w[:, cols].t().float()
        assert torch.equal(DC.gemm_sim(c, "f32").view, want)
        if not torch.equal(DC.gemm_sim(c, "f32", mut=mut).view, want):
            hit.add("w4")
    return hit


def _old_swiglu_rejects(mut):
    """N / 16 >= 512 tiles or an unsplittable K: ks == 1 (here K = 1280, which no ksplit halves)"""
    hit = False
    for kind in DC.KERNELS:
        for epi in (DC.EPI_SWIGLU_IL, DC.EPI_SWIGLU_HALVES):
            inp = DC.swiglu_inputs(5, 256, 1280, epi)
            assert DC.ksplit(kind, 256, 1280, epi) == 1
            c = DC.gemm_call(kind, inp, strided=False, ncols=128)
            want = DC.swiglu_expected(inp, epi, F32, last_round=True)
            assert max_rel(DC.swiglu_sim(c, epi).view, want) <= 5e-3
            hit |= not max_rel(DC.swiglu_sim(c, epi, mut=mut).view, want) <= 5e-3
    return hit


def _tol_needed(got, want):
    """tests/test_decode_kvfp8_gpu.py: the smallest tol with |got - want| <= 2^-8 |want| + tol max|want| per (b, head)"""
    got, want = got.double(), want.double()
    excess = ((got - want).abs() - 2.0 ** -8 * want.abs()).clamp_min(0)
    return float((excess / want.abs().amax(-1, keepdim=True).clamp_min(1e-300)).nan_to_num(nan=1e30).max())


def _old_attn_rejects(mut):
    hit = False
    lens = [1, 2, 33, 777, 2100]
    c = _host_attn(lens=lens, spikes=False)
    ns = min(1024, max(-(-512 // (len(lens) * c.Hkv)), -(-max(lens) // 512)))             # ops.decode_attn_splits
    for window in (0, 500):
        want = DC.attn_sim(c.q, c.kb, c.ks, c.vb, c.vs, lens, window, ns)
        sim = lambda m: DC.attn_sim(c.q, c.kb, c.ks, c.vb, c.vs, lens, window, ns, F32, m).to(BF)
        bound = max(1e-4, 4 * _tol_needed(sim(None), want))
        hit |= not _tol_needed(sim(mut), want) <= bound
    c4 = _host_attn(lens=[4, 4, 4, 4], spikes=False)                                                       # one code per token: Smax = 4
    v = DC.kv_dequant(c4.vb, c4.vs, c4.D)
    for kv_len, window, tok in ((1, 0, 0), (3, 1, 2), (4, 1, 3)):
        got = DC.attn_sim(c4.q, c4.kb, c4.ks, c4.vb, c4.vs, [kv_len] * 4, window, 64, F32, mut).to(BF)
        hit |= not torch.equal(got.float(), v[:, tok].repeat_interleave(c4.Hq // c4.Hkv, 1))
    return hit


def _old_quant_kv_rejects(mut):
    hit = False
    for heads, D in ((4, 32), (64, 96), (16, 128)):
        x = DC.quant_kv_source(37, heads, D)
        src = DC.Box(37, heads * D, heads * D + 2 * heads * D, fill=x)                     # the k|v columns of fused qkv rows
        q, s, w = DC.quant_kv_sim(src, heads, D, mut)
        hit |= not (w.all() and DC.quant_kv_verify(q, s, x, heads, D))
    return hit


def test_old_catches():
    seen = {}
    for m in DC.GEMM_MUTANTS:
        seen[m] = _old_gemm_rejects(m)
    for m in DC.SWIGLU_MUTANTS:
        seen[m] = _old_swiglu_rejects(m)
    for m in DC.ATTN_MUTANTS:
        seen[m] = _old_attn_rejects(m)
    for m in DC.QUANT_KV_MUTANTS:
        seen[m] = _old_quant_kv_rejects(m)
    assert seen == OLD_CATCHES
