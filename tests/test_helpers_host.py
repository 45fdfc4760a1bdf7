"""CPU proof behind tests/test_helpers_gpu.py, tests/test_attention_generic_gpu.py and tests/test_attention_d128_gpu.py.

1. Every reference of tests/helpers_ref.py agrees with torch's own operator where one exists (F.unfold, F.conv_transpose2d with an identity-like
   weight, F.interpolate in both align_corners modes, the oracle's RoPE, index_add_ / plain loops, autograd through attn_ref).
2. The comparisons used on the GPU (exact / by value / regimes.group_err with its computed bound / close() for attention) accept the honest
   reference evaluated in fp32 with its bf16 output rounding, and reject every mutant of tests/PATHS.md.
3. Whether TODAY's comparison (close() with the arguments and inputs of tests/test_kernels_gpu.py) sees each mutant: OLD_CATCHES.
4. D = 128 / 96 attention at block edges (tests/ATTENTION_D128.md): the reference with lse and defined empty rows against torch's softmax and
   autograd, the ten mutants against the comparisons of helpers_ref.d128_compare, and the fp32 no-rounding-boundary property of the exact pass."""
import math

import pytest
import torch
import torch.nn.functional as F

import helpers_ref as HR
import regimes as R
from regimes import BF, gen, randn
from test_attention_generic_gpu import EDGES
from test_kernels_gpu import attn_ref, close, rnd

F32, F64 = torch.float32, torch.float64
I32 = torch.int32


def passes(fn):
    try:
        fn()
        return True
    except AssertionError:
        return False


# ------------------------------------------------------------------------------------------------ 1. the references against torch
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 13), (12, 10)])
@pytest.mark.parametrize("stride", [1, 2])
def test_im2col_is_unfold(H, W, stride):
    B, C = 2, 8
    x = randn(B, H, W, C, seed=1)
    for relu in (0, 1):
        xn = x.float().permute(0, 3, 1, 2)
        u = F.unfold(F.relu(xn) if relu else xn, 3, padding=1, stride=stride)          # [B, C * 9, L], channel-major
        want = u.reshape(B, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)
        assert torch.equal(HR.im2col3x3(x, stride, relu), want)
        if H * W > 1:
            assert not torch.equal(HR.im2col3x3(x, stride, relu, mut="taps_kx_ky"), want)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_pixel_shuffle_is_conv_transpose_with_identity_weight(k):
    B, H, W, C = 2, 5, 3, 8
    t = randn(B * H * W, k * k * C, seed=2)
    w = torch.zeros(k * k * C, C, k, k)
    for ky in range(k):
        for kx in range(k):
            for c in range(C):
                w[(ky * k + kx) * C + c, c, ky, kx] = 1.0
    want = F.conv_transpose2d(t.float().reshape(B, H, W, -1).permute(0, 3, 1, 2), w, stride=k).permute(0, 2, 3, 1)
    assert torch.equal(HR.pixel_shuffle(t, B, H, W, k, C).float(), want)
    if k > 1:
        assert not torch.equal(HR.pixel_shuffle(t, B, H, W, k, C, mut="ky_kx_swapped").float(), want)
    idx = torch.arange(B * H * W * k * k * C).reshape(B * H * W, k * k * C)            # and the kernel's index formula
    y = HR.pixel_shuffle(idx, B, H, W, k, C)
    b, yy, xx, kk, c = 1, 3, 2, k * k - 1, 5
    assert int(y[b, yy * k + kk // k, xx * k + kk % k, c]) == int(idx[(b * H + yy) * W + xx, kk * C + c])


BILINEAR = [(12, 10, 17, 31), (12, 10, 24, 20), (12, 10, 12, 10), (24, 20, 7, 9), (12, 10, 1, 15), (12, 10, 9, 1), (1, 1, 5, 7), (37, 37, 145, 145)]


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("H,W,Ho,Wo", BILINEAR)
def test_bilinear_is_interpolate(H, W, Ho, Wo, align):
    x = randn(2, H, W, 8, seed=3)
    for dt, tol in ((F64, 1e-12), (F32, 2e-6)):
        want = F.interpolate(x.to(dt).permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
        got = HR.bilinear(x, Ho, Wo, align, dt)
        assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), (dt, float((got - want).abs().max()))


def test_minmax_is_torch_bf16_arithmetic():
    x = randn(3, 1000, seed=4, scale=3.0)
    mn, mx = x.amin(1, keepdim=True), x.amax(1, keepdim=True)
    assert HR.exact(HR.minmax(x).to(BF), (x - mn) / (mx - mn))                       # bf16 tensors: torch rounds after each operation


@pytest.mark.parametrize("hd", [32, 64, 96, 128])
def test_rope_is_the_oracles(hd):
    """forward: bit-equal to the oracle's q cos + rotate_half(q) sin in bf16 arithmetic (HF's rounding points), with position ids; the tables are the
    oracle's; inverse: the autograd transpose of the fp64 rotation, up to the two restated roundings"""
    from oracle import visper_oracle as O
    T, S, nh = 50, 16, 3
    x = randn(T, nh * hd + 24, seed=5)
    pos = torch.randint(0, S, (T,), generator=gen(6))
    pos[0] = S - 1
    cs, sn = HR.rope_tables(S, hd, 10000.0)
    oc, os_ = O.rope_tables(torch.arange(S)[None], hd, 10000.0, BF)
    assert torch.equal(oc[0, :, :hd // 2].float(), cs) and torch.equal(os_[0, :, :hd // 2].float(), sn)
    c, s = O.rope_tables(pos[None], hd, 10000.0, BF)                                   # [1, T, hd] bf16
    q = x[:, :nh * hd].reshape(T, nh, hd)
    want = q * c[0][:, None] + O._rot_half(q) * s[0][:, None]                         # bf16 arithmetic
    got = HR.rope(x, cs, sn, pos.to(I32), nh, hd, False).to(BF)
    assert HR.exact(got[:, :nh * hd].reshape(T, nh, hd), want)
    assert HR.exact(got[:, nh * hd:], x[:, nh * hd:])
    qq = q.double().clone().requires_grad_(True)
    g = randn(T, nh, hd, seed=7)
    (qq * c[0][:, None].double() + O._rot_half(qq) * s[0][:, None].double()).backward(g.double())
    gx = torch.zeros(T, nh * hd + 24, dtype=BF)
    gx[:, :nh * hd] = g.reshape(T, -1)
    inv = HR.rope(gx, cs, sn, pos.to(I32), nh, hd, True, F64)[:, :nh * hd].reshape(T, nh, hd)
    assert float((inv - qq.grad).abs().max()) <= 2 * 2.0 ** -9 * float(qq.grad.abs().max())
    bad = HR.rope(gx, cs, sn, pos.to(I32), nh, hd, True, F64, mut="inverse_sign_wrong_half")[:, :nh * hd].reshape(T, nh, hd)
    assert float((bad - qq.grad).abs().max()) > 0.1 * float(qq.grad.abs().max())


def test_gathers_and_scatters_are_loops():
    H, n = 16, 23
    srcs = [randn(r, H + 8, seed=8 + i) for i, r in enumerate((10, 7, 5))]
    kind = torch.randint(-1, 3, (n,), generator=gen(11)).to(I32)
    row = torch.randint(0, 5, (n,), generator=gen(12)).to(I32)
    before = randn(n, H + 8, seed=13)
    want = before.clone()
    for i in range(n):
        want[i, :H] = srcs[kind[i]][row[i], :H] if kind[i] >= 0 else 0
    assert HR.exact(HR.gather_rows(srcs, kind, row, H, before), want)
    src, cnt = randn(11, H + 8, seed=14), 3
    idx = torch.randint(-1, 11, (n * cnt,), generator=gen(15)).to(I32)
    b32 = before.float()
    for acc in (False, True):
        want = b32.double().clone()
        for i in range(n):
            a = sum((src[j, :H].double() for j in idx[i * cnt:(i + 1) * cnt].tolist() if j >= 0), torch.zeros(H, dtype=F64)) * 0.5
            want[i, :H] = want[i, :H] + a if acc else a
        assert torch.equal(HR.gather_sum_rows(src, idx, cnt, 0.5, b32, H, acc, F64), want)
    d0 = randn(30, H, seed=16).float()
    ix = torch.randint(-1, 30, (n,), generator=gen(17)).to(I32)
    src2 = randn(n, H, seed=18)
    want = d0.double().clone()
    for r in range(n):
        if ix[r] >= 0:
            want[ix[r]] += src2[r].double()
    assert torch.equal(HR.scatter_add_rows(src2, ix, d0, F64), want)                  # index_add_ with duplicates and skips
    perm = torch.randperm(30, generator=gen(19))[:n].to(I32)
    perm[4] = -1
    want = d0.clone()
    for r in range(n):
        if perm[r] >= 0:
            want[perm[r]] = src2[r].float()
    assert torch.equal(HR.scatter_rows(src2, perm, d0, H), want)
    x = randn(257, 70, seed=20)
    part = HR.colsum_partial(x, 70, HR.colsum_rpb(257), F64)
    assert part.shape == (129, 70) and torch.equal(part.sum(0), x.double().sum(0))
    assert torch.equal(part[128], x[256].double())                                    # the short last slab holds one row


@pytest.mark.parametrize("causal,window,kvl,Sq,Skv,Hq,Hkv", [(True, 0, None, 77, 77, 4, 2), (False, 0, [60, 33], 40, 90, 4, 4), (True, 50, None, 161, 161, 2, 2),
                                                       (True, 0, [96, 41], 96, 96, 4, 1), (True, 0, None, 30, 50, 4, 1)])
def test_attention_is_autograd_through_attn_ref(causal, window, kvl, Sq, Skv, Hq, Hkv):
    B, D = 2, 32
    q, k, v, do = randn(B, Sq, Hq, D, seed=21), randn(B, Skv, Hkv, D, seed=22), randn(B, Skv, Hkv, D, seed=23), randn(B, Sq, Hq, D, seed=24)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o = attn_ref(qr, kr, vr, causal, kv_len=kvl, window=window)
    o.backward(do.double())
    got = HR.attention(q, k, v, do, causal, kvl, window, F64)
    for name, want in (("o", o.detach()), ("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad)):
        assert float((got[name] - want).abs().max()) < 1e-12, name


# ------------------------------------------------------------------------------------------------ 2. + 3. mutants: new comparisons, old comparisons
def sim(t):
    """what a kernel with fp32 math and a bf16 output returns"""
    return t.to(BF)


# mutant -> does today's comparison (tests/test_kernels_gpu.py: close() with that test's arguments, on that test's inputs) notice it?
OLD_CATCHES = {
    "bilinear align_corners flag ignored": False,            # only align_corners=True is ever called
    "bilinear h0 / h1 swapped": True,
    "im2col taps in (kx, ky) order": True,                   # through the GEMM against F.conv2d
    "pixel shuffle kk / k and kk % k swapped": True,         # through the GEMM against F.conv_transpose2d
    "minmax without the intermediate roundings": False,      # the old expected value IS this mutant
    "rope pos = t % S when ids are given": False,            # pos = NULL only
    "rope inverse, sign on the wrong half": True,
    "gather kind < 0 rows left unwritten": None,             # `out` is torch.empty: seen only when the allocator hands back non-zero memory
    "gather_sum scale ignored when accumulate is set": False,
    "colsum last short slab dropped": False,                 # M = 70: one row per slab, no short slab
    "first sweep only": False,                               # no unit test is large enough for a second sweep
    "attention kv_len ignored in dK / dV": False,            # no backward runs with kv_len at D = 32 / 64
    "attention window lower bound off by one": True,
    # D = 128: attention_failures with close() on the seven edge shapes of test_attention_d128_dma_kernels_edges (it never looks at lse, no
    # shape has a causal or windowed row >= 256, an offset past the first block or a row without a key)
    "d128 block_first_key_dropped": False,
    "d128 offset_dropped_after_first_block": False,
    "d128 window_off_by_one": True,
    "d128 kvlen_ignored_dkdv": True,
    "d128 empty_row_nan": False,
    "d128 empty_row_uniform": False,
    "d128 lse_natural_log": False,
    "d128 lse_without_last_tile": False,
    "d128 kv_head_modulo": True,
    "d128 gqa_last_head_dropped_in_dkdv": True,
}


def test_bilinear_mutants():
    x = randn(2, 12, 10, 16, seed=30)
    new = {"align_ignored": False, "h_swapped": False}
    for (H, W, Ho, Wo) in BILINEAR[:7]:
        xx = randn(2, H, W, 8, seed=31)
        for align in (1, 0):
            assert not HR.failures(HR.bilinear_check(sim(HR.bilinear(xx, Ho, Wo, align)), xx, Ho, Wo, align)), (H, W, Ho, Wo, align)
            for m in new:
                new[m] |= bool(HR.failures(HR.bilinear_check(sim(HR.bilinear(xx, Ho, Wo, align, mut=m)), xx, Ho, Wo, align)))
    assert all(new.values()), new
    assert not HR.failures(HR.bilinear_check(sim(HR.bilinear(x, 17, 31, 1, mut="align_ignored")), x, 17, 31, 1))       # invisible where align = 1 is asked
    # today: test_dpt_conv_helpers, x = rnd(2, 12, 10, 16, seed=40), align_corners=True, close(rtol=1e-2)
    xo = rnd(2, 12, 10, 16, seed=40)
    old = {m: False for m in new}
    for (Ho, Wo) in ((24, 20), (17, 31), (12, 10)):
        ref = F.interpolate(xo.float().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        assert passes(lambda: close(sim(HR.bilinear(xo, Ho, Wo, True)), ref, rtol=1e-2))
        for m in old:
            old[m] |= not passes(lambda: close(sim(HR.bilinear(xo, Ho, Wo, True, mut=m)), ref, rtol=1e-2))
    assert old == {"align_ignored": OLD_CATCHES["bilinear align_corners flag ignored"], "h_swapped": OLD_CATCHES["bilinear h0 / h1 swapped"]}


def test_im2col_and_pixel_shuffle_mutants():
    x = randn(2, 5, 13, 8, seed=32)
    for stride in (1, 2):
        want = HR.im2col3x3(x, stride, 1).to(BF)
        assert HR.same_values(sim(HR.im2col3x3(x, stride, 1)), want)
        assert not HR.same_values(sim(HR.im2col3x3(x, stride, 1, mut="taps_kx_ky")), want)
    t = randn(2 * 5 * 3, 16 * 8, seed=33)
    assert HR.exact(HR.pixel_shuffle(t, 2, 5, 3, 4, 8), HR.pixel_shuffle(t, 2, 5, 3, 4, 8))
    assert not HR.exact(HR.pixel_shuffle(t, 2, 5, 3, 4, 8, mut="ky_kx_swapped"), HR.pixel_shuffle(t, 2, 5, 3, 4, 8))
    # today: test_dpt_conv_helpers runs both through the GEMM against F.conv2d / F.conv_transpose2d
    B, H, W, Cc, Co = 2, 12, 10, 16, 24
    xo = rnd(B, H, W, Cc, seed=40)
    xn = xo.float().permute(0, 3, 1, 2)
    w, b = rnd(Co, Cc, 3, 3, seed=41) * 0.2, rnd(Co, seed=42)
    ref = F.conv2d(xn, w.float(), b.float(), stride=1, padding=1).permute(0, 2, 3, 1)
    wm = w.permute(0, 2, 3, 1).reshape(Co, -1).float()
    conv = lambda mut: sim(HR.im2col3x3(xo, 1, 0, mut=mut) @ wm.t() + b.float()).reshape(B, H, W, Co)
    assert passes(lambda: close(conv(None), ref))
    assert (not passes(lambda: close(conv("taps_kx_ky"), ref))) == OLD_CATCHES["im2col taps in (kx, ky) order"]
    k = 2
    wt, bt = rnd(Cc, Co, k, k, seed=43) * 0.2, rnd(Co, seed=44)
    ref = F.conv_transpose2d(xn, wt.float(), bt.float(), stride=k).permute(0, 2, 3, 1)
    wm = wt.permute(2, 3, 1, 0).reshape(k * k * Co, Cc).float()
    tt = sim(xo.float().reshape(-1, Cc) @ wm.t() + bt.float().repeat(k * k))
    assert passes(lambda: close(HR.pixel_shuffle(tt, B, H, W, k, Co), ref))
    assert (not passes(lambda: close(HR.pixel_shuffle(tt, B, H, W, k, Co, mut="ky_kx_swapped"), ref))) == OLD_CATCHES["pixel shuffle kk / k and kk % k swapped"]


@pytest.mark.parametrize("n", [63, 1000, 1024, 1025, 3000])
def test_minmax_mutant(n):
    x = randn(3, n, seed=34, scale=3.0)
    assert not HR.failures(HR.minmax_check(sim(HR.minmax(x)), x))
    bad = HR.failures(HR.minmax_check(sim(HR.minmax(x, mut="no_intermediate_rounding")), x))
    assert "flips" in bad
    assert not [g for g in bad if g.startswith("image")]       # the r = 3 bound alone does not see it (tests/PATHS.md)
    # today: d = rnd(3, 1000, seed=45).abs(); close() against the unrounded fp32 expression
    d = rnd(3, 1000, seed=45).abs()
    mn, mx = d.float().amin(1, keepdim=True), d.float().amax(1, keepdim=True)
    old_ref = (d.float() - mn) / (mx - mn)
    assert passes(lambda: close(sim(HR.minmax(d)), old_ref))
    assert (not passes(lambda: close(sim(HR.minmax(d, mut="no_intermediate_rounding")), old_ref))) == OLD_CATCHES["minmax without the intermediate roundings"]


def test_rope_mutants():
    T, S, nh, hd = 50, 16, 3, 64
    x = randn(T, nh * hd + 24, seed=35)
    cs, sn = HR.rope_tables(S, hd, 10000.0)
    pos = torch.randint(0, S, (T,), generator=gen(36)).to(I32)
    for inverse in (False, True):
        want = HR.rope(x, cs, sn, pos, nh, hd, inverse).to(BF)
        assert not HR.exact(HR.rope(x, cs, sn, pos, nh, hd, inverse, mut="pos_ignored").to(BF), want)
        assert HR.exact(HR.rope(x, cs, sn, None, nh, hd, inverse, mut="pos_ignored").to(BF), HR.rope(x, cs, sn, None, nh, hd, inverse).to(BF))
    want = HR.rope(x, cs, sn, pos, nh, hd, True).to(BF)
    assert not HR.exact(HR.rope(x, cs, sn, pos, nh, hd, True, mut="inverse_sign_wrong_half").to(BF), want)
    # today: test_rope_fwd_and_inverse, pos = NULL, ascending table, close() on the inverse against the autograd transpose
    from oracle import visper_oracle as O
    B, S2 = 2, 50
    g = rnd(B, S2, nh * hd, seed=19)
    cs2, sn2 = HR.rope_tables(S2, hd, 10000.0)
    cos, sin = O.rope_tables(torch.arange(S2)[None].expand(B, S2), hd, 10000.0, BF)
    qq = torch.randn(B, nh, S2, hd, requires_grad=True)
    (qq * cos[:, None].float() + O._rot_half(qq) * sin[:, None].float()).backward(g.reshape(B, S2, nh, hd).transpose(1, 2).float())
    ref = qq.grad.transpose(1, 2)
    inv = lambda mut: sim(HR.rope(g.reshape(B * S2, -1), cs2, sn2, None, nh, hd, True, mut=mut)).reshape(B, S2, nh, hd)
    assert passes(lambda: close(inv(None), ref))
    assert (not passes(lambda: close(inv("inverse_sign_wrong_half"), ref))) == OLD_CATCHES["rope inverse, sign on the wrong half"]
    assert HR.exact(inv("pos_ignored"), inv(None)) and not OLD_CATCHES["rope pos = t % S when ids are given"]


def test_gather_and_reduction_mutants():
    H, n = 8, 9
    srcs = [randn(r, H, seed=37 + i) for i, r in enumerate((10, 7, 5))]
    kind = torch.tensor([0, 1, -1, 2, 0, 1, 2, -1, 0], dtype=I32)
    row = torch.tensor([3, 6, 0, 4, 9, 0, 1, 0, 0], dtype=I32)
    sent = torch.full((n, H + 16), 0x7A5A, dtype=torch.int16).view(BF)
    want = HR.gather_rows(srcs, kind, row, H, sent)
    assert not HR.exact(HR.gather_rows(srcs, kind, row, H, sent, mut="skip_rows_unwritten"), want)
    # today: `out = torch.empty(...)`: the mutant is invisible whenever that memory happens to hold zeros
    zeros = torch.zeros(n, H, dtype=BF)
    assert HR.exact(HR.gather_rows(srcs, kind, row, H, zeros, mut="skip_rows_unwritten"), HR.gather_rows(srcs, kind, row, H, zeros))
    assert OLD_CATCHES["gather kind < 0 rows left unwritten"] is None
    # gather_sum: exact on integers
    src = HR.ints(11, H, seed=40)
    idx = torch.randint(-1, 11, (n * 3,), generator=gen(41)).to(I32)
    o0 = HR.ints(n, H, seed=42).float()
    want = HR.gather_sum_rows(src, idx, 3, 0.5, o0, H, True)
    assert not HR.exact(HR.gather_sum_rows(src, idx, 3, 0.5, o0, H, True, mut="scale_ignored_on_accumulate"), want)
    assert HR.exact(HR.gather_sum_rows(src, idx, 3, 0.5, o0, H, False, mut="scale_ignored_on_accumulate"), HR.gather_sum_rows(src, idx, 3, 0.5, o0, H, False))
    assert not OLD_CATCHES["gather_sum scale ignored when accumulate is set"]           # today's call: accumulate off
    # ... and bounded on random values
    srcr = torch.randn(11, H, generator=gen(43))
    ref = lambda dt: HR.gather_sum_rows(srcr, idx, 3, 0.375, o0, H, True, dt)
    assert not HR.failures(HR.bounded(ref(F32), ref, n=4))
    assert HR.failures(HR.bounded(HR.gather_sum_rows(srcr, idx, 3, 0.375, o0, H, True, mut="scale_ignored_on_accumulate"), ref, n=4))
    # colsum: M = 257 has a short last slab
    x = HR.ints(257, 70, seed=44)
    fin = lambda mut, xx, M: HR.colsum_finish(HR.colsum_partial(xx, 70, HR.colsum_rpb(M), mut=mut), 1.0, False, torch.zeros(70))
    assert not HR.exact(fin("last_short_slab_dropped", x, 257), fin(None, x, 257))
    xr = randn(257, 70, seed=45)
    assert HR.failures(HR.bounded(fin("last_short_slab_dropped", xr, 257), lambda dt: HR.colsum_finish(HR.colsum_partial(xr, 70, 2, dt), 1.0, False, torch.zeros(70), dt), n=258))
    xo = rnd(70, 64, seed=24)                                                              # today: M = 70
    assert HR.exact(HR.colsum_partial(xo, 64, HR.colsum_rpb(70), mut="last_short_slab_dropped"), HR.colsum_partial(xo, 64, HR.colsum_rpb(70)))
    assert not OLD_CATCHES["colsum last short slab dropped"]


def test_first_sweep_only_mutants():
    """a kernel that never takes its grid-stride loop a second time, at the wrap shapes of tests/test_helpers_gpu.py; today's shapes stay inside one
    sweep, where this mutant IS the honest kernel"""
    sent = lambda *shape: torch.full(shape, 0x7A5A, dtype=torch.int16).view(BF)
    n = HR.EW_CAP * 256 * 8 + 2400
    a, b = randn(n, seed=50), randn(n, seed=51)
    assert not HR.exact(HR.first_sweep(a + b, sent(n), HR.EW_CAP * 256 * 8), a + b)                     # add: items of 8 elements
    assert HR.exact(HR.first_sweep(a[:4480] + b[:4480], sent(4480), HR.EW_CAP * 256 * 8), a[:4480] + b[:4480])      # today: 70 x 64
    nc = HR.EW_CAP * 256 + 300
    x = torch.randn(nc, generator=gen(52))
    assert not HR.exact(HR.first_sweep(x.to(BF), sent(nc), HR.EW_CAP * 256), x.to(BF))                   # casts: items of 1 element
    s0 = randn(2050, 2048, seed=53)
    assert not HR.exact(HR.first_sweep(s0, sent(2050, 2048), HR.EW_CAP * 256 * 8), s0)                   # copy2d / add2d / swiglu rows
    assert HR.first_sweep(s0, sent(2050, 2048), HR.EW_CAP * 256 * 8)[2047].equal(s0[2047])
    for cap_rows, rows in ((HR.GATHER_ROWS_CAP * 4, HR.GATHER_ROWS_CAP * 4 + 5), (HR.SCATTER_ROWS_CAP * 4, HR.SCATTER_ROWS_CAP * 4 + 5), (HR.GATHER_SUM_CAP, HR.GATHER_SUM_CAP + 5)):
        g = randn(rows, 8, seed=54)
        assert not HR.exact(HR.first_sweep(g, sent(rows, 8), cap_rows * 8), g)
    xi = HR.ints(5000, seed=55).float()
    xi[-1] = 7.0
    assert not HR.exact(HR.sum_f32(xi, 0.5, mut="first_sweep"), HR.sum_f32(xi, 0.5))
    assert HR.exact(HR.sum_f32(xi[:1000], 0.5, mut="first_sweep"), HR.sum_f32(xi[:1000], 0.5))            # today: n = 1000
    xr = torch.randn(5000, generator=gen(56))
    assert HR.failures(HR.bounded(HR.sum_f32(xr, 0.5, mut="first_sweep"), lambda dt: HR.sum_f32(xr, 0.5, dt), n=5000))
    nq = HR.SUMSQ_CAP * 4096 + 1000
    xs = torch.randint(-1, 2, (nq,), generator=gen(57)).float()
    xs[-1000:] = 2.0
    assert float(HR.sumsq(xs)) < 2 ** 24
    # (sumsq's blocks stride by gridDim * 256: "first sweep" = the first 1024 * 256 elements)
    assert not HR.exact(HR.sumsq(xs, mut="first_sweep"), HR.sumsq(xs))
    assert HR.exact(HR.sumsq(xs[:100003], mut="first_sweep"), HR.sumsq(xs[:100003]))                       # today: n = 100 003
    img = randn(1, 37, 37, 8, seed=58)
    y = HR.bilinear(img, 1450, 1450, 0)
    res = HR.bilinear_check(HR.first_sweep(sim(y), torch.zeros(1, 1450, 1450, 8, dtype=BF), HR.CONV_CAP * 256 * 8), img, 1450, 1450, 0)
    assert HR.failures(res)
    assert not HR.failures(HR.bilinear_check(sim(y), img, 1450, 1450, 0))
    assert not OLD_CATCHES["first sweep only"]


ATTN_NEW = [  # (B, Hq, Hkv, Sq, Skv, causal, window, kvl): cases of test_attn_generic_masks_gqa_views that carry a kv_len / a window
    (2, 4, 2, 96, 96, True, 0, [96, 41]), (1, 2, 1, 257, 257, False, 0, [200]), (2, 2, 2, 161, 161, True, 50, None)]


@pytest.mark.parametrize("D", [64, 32])
def test_attention_mutants(D):
    caught = {"kvlen_ignored_dkdv": [], "window_off_by_one": []}
    for (B, Hq, Hkv, Sq, Skv, causal, window, kvl) in ATTN_NEW:
        q, k, v, do = rnd(B, Sq, Hq, D, seed=81), rnd(B, Skv, Hkv, D, seed=82), rnd(B, Skv, Hkv, D, seed=83), rnd(B, Sq, Hq, D, seed=84)
        ref = HR.attention(q, k, v, do, causal, kvl, window)
        honest = {n_: sim(t) for n_, t in ref.items()}
        assert not HR.attention_failures(honest, ref, kvl, close)
        for m in caught:
            got = {n_: sim(t) for n_, t in HR.attention(q, k, v, do, causal, kvl, window, mut=m).items()}
            caught[m] += HR.attention_failures(got, ref, kvl, close)
    assert "dk beyond kv_len" in caught["kvlen_ignored_dkdv"] and "dv beyond kv_len" in caught["kvlen_ignored_dkdv"]
    assert "o" in caught["window_off_by_one"]
    assert not OLD_CATCHES["attention kv_len ignored in dK / dV"]       # today's D = 32 / 64 backward cases carry no kv_len: the mutant is the honest kernel
    if D == 32:        # today: test_attention_sliding_window, forward only, B, S, H, D = 1, 200, 2, 32, window 70
        q, k, v = rnd(1, 200, 2, 32, seed=36), rnd(1, 200, 2, 32, seed=37), rnd(1, 200, 2, 32, seed=38)
        ref = attn_ref(q.float(), k.float(), v.float(), True, window=70)
        assert passes(lambda: close(sim(HR.attention(q, k, v, q, True, None, 70)["o"]), ref))
        assert (not passes(lambda: close(sim(HR.attention(q, k, v, q, True, None, 70, mut="window_off_by_one")["o"]), ref))) == OLD_CATCHES["attention window lower bound off by one"]


# ------------------------------------------------------------------------------------------------ D = 128 / 96 at block edges (tests/ATTENTION_D128.md)
D128 = [(n, D) for n in HR.D128_CASES for D in HR.D128_DIMS]


@pytest.mark.parametrize("name,D", D128)
def test_d128_reference_is_torch_softmax_and_autograd(name, D):
    """o, lse, dq, dk, dv of helpers_ref.attention in fp64 against torch.softmax / torch.logsumexp and autograd.  torch yields NaN for a row without
    a visible key, so such rows are given every key here and their output rows multiplied by zero before the backward: what is compared is the
    non-empty rows, and that an empty row adds nothing."""
    B, Hq, Hkv, Sq, Skv, causal, window, kvl = HR.D128_CASES[name]
    inp, ref, _ = HR.d128_refs(name, D, "random")
    allow = HR.attention_mask(B, Sq, Skv, causal, kvl, window)
    live = allow.any(-1, keepdim=True)
    qr, kr, vr = (inp[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    rep = Hq // Hkv
    s = qr.transpose(1, 2) @ kr.transpose(1, 2).repeat_interleave(rep, dim=1).transpose(-1, -2) / math.sqrt(D)
    s = s.masked_fill(~(allow | ~live), float("-inf"))
    o = ((torch.softmax(s, -1) @ vr.transpose(1, 2).repeat_interleave(rep, dim=1)) * live).transpose(1, 2)
    o.backward(inp["do"].double())
    lse = torch.logsumexp(s.detach(), -1) * HR.LOG2E
    rows = live[:, 0, :, 0]
    assert int((~rows).sum()) == (407 if name == "window-kvlen-empty" else 0)
    for nm, want in (("o", o.detach()), ("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad)):
        assert float((ref[nm] - want).abs().max()) < 1e-12, nm
    keep = rows[:, None, :].expand(B, Hq, Sq)
    assert float((ref["lse"] - lse)[keep].abs().max()) < 1e-12
    assert bool((ref["lse"][~keep] == HR.EMPTY_LSE).all()) and bool((ref["o"][~rows] == 0).all()) and bool((ref["dq"][~rows] == 0).all())


def _rejected(name, D, kind, mut):
    res, bad = HR.d128_compare(name, D, kind, HR.d128_simulate(name, D, kind, mut))
    return [k for k, (e, b) in res.items() if not e <= b], bad


@pytest.mark.parametrize("name,D", D128)
def test_d128_comparisons_accept_the_honest_reference(name, D):
    for kind in ("random", "exact"):
        assert _rejected(name, D, kind, None) == ([], []), kind


@pytest.mark.parametrize("D", HR.D128_DIMS)
@pytest.mark.parametrize("mut", HR.ATTENTION_MUTANTS)
def test_d128_mutants(mut, D):
    """the comparisons of tests/test_attention_d128_gpu.py reject each mutant on the case it is aimed at, in the random AND in the exact pass"""
    name = HR.D128_MUTANT_CASE[mut]
    (bounded, exact), (bounded_x, exact_x) = _rejected(name, D, "random", mut), _rejected(name, D, "exact", mut)
    assert bounded or exact, "random pass"
    assert bounded_x or exact_x, "exact pass"
    if mut in ("block_first_key_dropped", "offset_dropped_after_first_block", "window_off_by_one", "lse_natural_log", "lse_without_last_tile"):
        assert any(g.startswith("lse") for g in bounded) and "round(2^lse) is not the number of visible keys" in exact_x
    if mut in ("block_first_key_dropped", "offset_dropped_after_first_block", "window_off_by_one"):
        assert "o is not bf16(cnt / n)" in exact_x
    if mut.startswith("empty_row"):
        assert {"lse of an empty row is not -1e30", "o of an empty row is not zero", "dq of an empty row is not zero"} <= set(exact)
    if mut == "kvlen_ignored_dkdv":
        assert {"dk beyond kv_len", "dv beyond kv_len"} <= set(exact)
    if mut == "block_first_key_dropped":
        # with equal scores (the exact pass) every row that loses key 256 moves its lse by log2(n / (n - 1)) >= 1 / (513 ln 2) = 2.8e-3, eighty times
        # the lse bound; with N(0, 1) scores the lost key's weight varies from row to row, and it is the block's largest move that is compared
        got, ref = HR.d128_simulate(name, D, "exact", mut)["lse"], HR.d128_refs(name, D, "exact")[1]["lse"]
        assert float((got.double() - ref)[:, :, 256:].abs().min()) >= 2.8e-3
        assert {"lse[block1]", "lse[block2]"} <= set(bounded)


def test_d128_old_catches():
    """the parent's comparison (attention_failures with close() on the seven edge shapes, D = 128) on the ten mutants: OLD_CATCHES"""
    D = 128
    old = {m: False for m in HR.ATTENTION_MUTANTS}
    for (B, Hq, Hkv, Sq, Skv, causal, window, kvl) in EDGES:
        q, k, v, do = rnd(B, Sq, Hq, D, seed=81), rnd(B, Skv, Hkv, D, seed=82), rnd(B, Skv, Hkv, D, seed=83), rnd(B, Sq, Hq, D, seed=84)
        ref = HR.attention(q, k, v, do, causal, kvl, window)
        assert not HR.attention_failures({n_: sim(t) for n_, t in ref.items()}, ref, kvl, close)
        for m in old:
            got = {n_: sim(t) for n_, t in HR.attention(q, k, v, do, causal, kvl, window, mut=m).items()}
            old[m] |= bool(HR.attention_failures(got, ref, kvl, close))
    assert old == {m: OLD_CATCHES[f"d128 {m}"] for m in HR.ATTENTION_MUTANTS}
    assert sum(old.values()) == 4


@pytest.mark.parametrize("name,D", D128)
def test_d128_exact_pass_is_out_of_reach_of_a_rounding_boundary(name, D):
    """The exact pass demands o == bf16(cnt / n) bit for bit.  A kernel forms it in fp32 as cnt * (1 / n), its reciprocal possibly a hardware
    approximation: for every row of every case cnt * fp32(1 / n) rounds to the same bf16 as the fp64 quotient, also with 1 / n off by +-2^-22
    relative (four fp32 ulps)."""
    n, cnt = HR.d128_counts(name, D)
    live = n > 0
    n, cnt = n[live], cnt[live]
    assert int(cnt.max()) <= 8 and bool((cnt.sum(-1) == n).all())
    want = (cnt.double() / n.double()[:, None]).to(BF)
    for pert in (0.0, 2.0 ** -22, -2.0 ** -22):
        inv = ((1.0 / n.double()).float().double() * (1.0 + pert)).float()
        assert HR.exact((cnt.float() * inv[:, None]).to(BF), want), pert
