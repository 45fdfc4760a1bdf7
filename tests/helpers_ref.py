"""Plain torch references of the bandwidth-bound helper kernels (csrc/elementwise.hip, csrc/conv.hip, the transposes of csrc/gemm.hip) and of
masked attention with its gradients, shared by tests/test_helpers_host.py (CPU), tests/test_helpers_gpu.py and
tests/test_attention_generic_gpu.py.

Every reference runs in the float dtype `dt` it is given (fp32: what a kernel with fp32 math computes; fp64: the truth), restates the
kernel's documented bf16 rounding points with `bfr`, and leaves the LAST rounding of a bf16 output out (the caller applies `.to(BF)` where
the comparison is exact).  `mut` selects a MUTANT: the same reference with one plausible mistake.  tests/PATHS.md lists them.

Two kinds of comparison, see tests/test_helpers_gpu.py: `exact` (integer views, torch.equal) and `bounded` (regimes.group_err against the
fp64 reference, bound from regimes.bound with y = the fp32 reference's own error)."""
import math

import torch
import torch.nn.functional as F

import regimes as R
from regimes import BF, bfr, gen

# The grid caps of the launchers (csrc/elementwise.hip, csrc/conv.hip): blocks of 256 threads; a kernel with more work items than
# cap * 256 runs its grid-stride loop a second time.
EW_CAP = 2048            # elementwise.hip GRID_FOR
CONV_CAP = 8192          # conv.hip GRID_FOR
GATHER_ROWS_CAP = 4096   # vp_gather_rows: blocks of 4 rows (one wave each)
SCATTER_ROWS_CAP = 8192  # vp_scatter_rows_bf16_to_f32: blocks of 4 rows
GATHER_SUM_CAP = 8192    # vp_gather_sum_rows: grid.y rows
SUMSQ_CAP = 1024         # vp_sumsq_nblk: blocks of 256 elements
SUM_BLOCK = 1024         # sum_f32_kernel: one block of 1024 threads


def ints(*shape, seed, lo=-8, hi=8):
    """small integers as bf16: every partial sum of a few thousand of them is an integer below 2^24, exact in fp32 in any order"""
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(BF)


def first_sweep(out, before, done):
    """MUTANT of any kernel whose work items run in the row-major order of `out`: only the first `done` ELEMENTS are processed (a grid-stride
    loop that never loops), the rest keep `before`"""
    o, b = out.clone().reshape(-1), before.reshape(-1)
    o[done:] = b[done:].to(o.dtype)
    return o.reshape(out.shape)


# ------------------------------------------------------------------------------------------------ conv.hip
def im2col3x3(x, stride, relu_in, dt=torch.float32, mut=None):
    """x [B, H, W, C] -> col [B * Ho * Wo, 9 C], column (ky * 3 + kx) * C + c = relu?(x[b, oy s + ky - 1, ox s + kx - 1, c]), zero padding"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=dt)
    xp[:, 1:-1, 1:-1] = x.to(dt)
    if relu_in:
        xp = xp.clamp_min(0)
    taps = []
    for a in range(3):
        for b in range(3):
            ky, kx = (b, a) if mut == "taps_kx_ky" else (a, b)
            taps.append(xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride])
    return torch.stack(taps, 3).reshape(B * Ho * Wo, 9 * C)


def pixel_shuffle(t, B, H, W, k, C, mut=None):
    """t [B * H * W, k * k * C], column (ky * k + kx) * C + c  ->  [B, H k, W k, C]"""
    v = t.reshape(B, H, W, k, k, C)
    v = v.permute(0, 1, 4, 2, 3, 5) if mut == "ky_kx_swapped" else v.permute(0, 1, 3, 2, 4, 5)
    return v.reshape(B, H * k, W * k, C)


def _src_index(n_in, n_out, align, dt):
    """aten area_pixel_compute_source_index in `dt` -> (i0, i1, lambda0, lambda1)"""
    o = torch.arange(n_out, dtype=dt)
    if align:
        src = torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=dt) * o
    else:
        src = (torch.tensor(n_in / n_out, dtype=dt) * (o + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = src - i0.to(dt)
    return i0, i1, 1 - l1, l1


def bilinear(x, Ho, Wo, align, dt=torch.float32, mut=None):
    """torch upsample_bilinear2d on NHWC: h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11), no intermediate rounding (one, the output's)"""
    if mut == "align_ignored":
        align = True
    xx = x.to(dt)
    y0, y1, h0, h1 = _src_index(x.shape[1], Ho, align, dt)
    x0, x1, w0, w1 = _src_index(x.shape[2], Wo, align, dt)
    if mut == "h_swapped":
        h0, h1 = h1, h0
    h0, h1 = h0[None, :, None, None], h1[None, :, None, None]
    w0, w1 = w0[None, None, :, None], w1[None, None, :, None]
    top, bot = xx[:, y0], xx[:, y1]
    return h0 * (w0 * top[:, :, x0] + w1 * top[:, :, x1]) + h1 * (w0 * bot[:, :, x0] + w1 * bot[:, :, x1])


def minmax(x, dt=torch.float32, mut=None):
    """x [B, n]: bf16(x - min) / bf16(max - min) per row: torch's bf16 arithmetic rounds after each operation (conv.hip minmax_norm_kernel)"""
    xx = x.to(dt)
    mn, mx = xx.amin(1, keepdim=True), xx.amax(1, keepdim=True)
    if mut == "no_intermediate_rounding":
        return (xx - mn) / (mx - mn)
    return bfr(xx - mn) / bfr(mx - mn)


def dwconv7x7(x, w_tap, bias, dt=torch.float32):
    """x [B, H, W, C], w_tap [49, C] tap-major, bias [C]: depthwise 7 x 7, zero padding 3, one rounding (the output's)"""
    C = x.shape[-1]
    w = w_tap.to(dt).t().reshape(C, 1, 7, 7)
    return F.conv2d(x.to(dt).permute(0, 3, 1, 2), w, bias.to(dt), padding=3, groups=C).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ RoPE
def rope_tables(S, hd, theta):
    """cos / sin [S, hd / 2] fp32 holding bf16 values (HF casts the tables to the activation dtype); the formula of ops.rope_tables"""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    fr = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().to(BF).float(), fr.sin().to(BF).float()


def rope(x, cos_t, sin_t, pos, nheads, hd, inverse, dt=torch.float32, mut=None):
    """x [T, ld] with ld >= nheads * hd; position of row t = pos[t] (None: t % S).  HF: q cos + rotate_half(q) sin with each product rounded to
    bf16 before the add; inverse = the transpose rotation (sin negated).  Columns >= nheads * hd are returned unchanged."""
    T, S, half = x.shape[0], cos_t.shape[0], hd // 2
    p = torch.arange(T) % S if (pos is None or mut == "pos_ignored") else pos.long()
    c, s = cos_t.to(dt)[p][:, None], sin_t.to(dt)[p][:, None]
    out = x.to(dt).clone()
    v = out[:, :nheads * hd].reshape(T, nheads, hd)
    x1, x2 = v[..., :half], v[..., half:]
    sa = sb = -s if inverse else s
    if mut == "inverse_sign_wrong_half" and inverse:
        sa, sb = s, -s                                       # the first half keeps the forward's minus while the second half also takes one
    oa = bfr(x1 * c) + bfr(-x2 * sa)
    ob = bfr(x2 * c) + bfr(x1 * sb)
    out[:, :nheads * hd] = torch.cat([oa, ob], -1).reshape(T, nheads * hd)
    return out


# ------------------------------------------------------------------------------------------------ gathers / scatters
def gather_rows(srcs, kind, row, H, before, mut=None):
    """out[i, :H] = srcs[kind[i]][row[i], :H], zeros where kind[i] < 0; `before` [n, ldo] is what the output buffer held"""
    out = before.clone()
    if mut != "skip_rows_unwritten":
        out[kind < 0, :H] = 0
    for k, s in enumerate(srcs):
        m = kind == k
        out[m, :H] = s[row[m].long(), :H].to(out.dtype)
    return out


def gather_sum_rows(src, idx, cnt, scale, before, H, accumulate, dt=torch.float32, mut=None):
    """out[i, :H] (+)= scale * sum_{k < cnt} src[idx[i cnt + k], :H] over the idx >= 0; -> `dt`, columns >= H as in `before`"""
    n = before.shape[0]
    ix = idx.reshape(n, cnt).long()
    rows = src.to(dt)[ix.clamp_min(0), :H] * (ix >= 0)[..., None].to(dt)
    a = rows.sum(1)
    if not (mut == "scale_ignored_on_accumulate" and accumulate):
        a = a * scale
    out = before.to(dt).clone()
    out[:, :H] = out[:, :H] + a if accumulate else a
    return out


def scatter_rows(src, idx, before, H):
    """dst[idx[r], :H] = float(src[r, :H]) (idx None: row r; idx < 0 skips)"""
    out = before.clone()
    t = torch.arange(src.shape[0]) if idx is None else idx.long()
    keep = t >= 0
    out[t[keep], :H] = src[keep, :H].float()
    return out


def scatter_add_rows(src, idx, before, dt=torch.float32):
    """dst[idx[r], :] += src[r, :] (idx < 0 skips); duplicates add up"""
    keep = idx >= 0
    return before.to(dt).clone().index_add_(0, idx[keep].long(), src[keep].to(dt))


# ------------------------------------------------------------------------------------------------ reductions
def colsum_partial(x, N, rpb, dt=torch.float32, mut=None):
    """x [M, ld >= N] -> part [ceil(M / rpb), N]: sums of slabs of rpb rows (the last one may be short)"""
    M = x.shape[0]
    nslab = (M + rpb - 1) // rpb
    xx = torch.zeros(nslab * rpb, N, dtype=dt)
    xx[:M] = x[:, :N].to(dt)
    if mut == "last_short_slab_dropped" and M % rpb:
        xx[(nslab - 1) * rpb:] = 0
    return xx.reshape(nslab, rpb, N).sum(1)


def colsum_finish(part, scale, accumulate, before, dt=torch.float32):
    a = part.to(dt).sum(0) * scale
    return before.to(dt) + a if accumulate else a


def colsum_rpb(M):
    """rows per slab as ops.colsum chooses them (at most 256 slabs)"""
    return max(1, (M + 255) // 256)


def sum_f32(x, scale, dt=torch.float32, mut=None):
    xx = x.to(dt)
    if mut == "first_sweep":
        xx = xx[:SUM_BLOCK]
    return (xx.sum() * scale).reshape(1)


def sumsq(x, dt=torch.float32, mut=None):
    xx = x.to(dt)
    if mut == "first_sweep":
        xx = xx[:SUMSQ_CAP * 256]
    return (xx * xx).sum().reshape(1)


# ------------------------------------------------------------------------------------------------ attention
def attention(q, k, v, do, causal, kv_len=None, window=0, dt=torch.float32, mut=None):
    """q / do [B, Sq, Hq, D], k / v [B, Skv, Hkv, D]: HF-eager masked softmax attention (the mask of test_kernels_gpu.attn_ref: causal with
    offset Skv - Sq, keys > i - window, keys < kv_len[b]) and its gradients written out: P = softmax(S), dV = P^T dO, dS = P (dO V^T - rowsum(dO O)),
    dQ = dS K / sqrt(D), dK = dS^T Q / sqrt(D).  Mutants: `kvlen_ignored_dkdv` (the dK / dV pass recomputes P from the row statistics without the
    kv_len term of its mask), `window_off_by_one` (keys >= i - window)."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    qq, dd = q.to(dt).transpose(1, 2), do.to(dt).transpose(1, 2)
    kk = k.to(dt).transpose(1, 2).repeat_interleave(rep, dim=1)
    vv = v.to(dt).transpose(1, 2).repeat_interleave(rep, dim=1)
    sc = 1.0 / math.sqrt(D)
    s = qq @ kk.transpose(-1, -2) * sc
    i = torch.arange(Sq)[:, None] + (Skv - Sq)
    j = torch.arange(Skv)[None, :]
    allow = torch.ones(Sq, Skv, dtype=torch.bool)
    if causal:
        allow &= j <= i
    if window > 0:
        allow &= (j >= i - window) if mut == "window_off_by_one" else (j > i - window)
    allow = allow[None, None].expand(B, 1, Sq, Skv).clone()
    no_len = allow.clone()
    if kv_len is not None:
        for b in range(B):
            allow[b, :, :, kv_len[b]:] = False
    sm = s.masked_fill(~allow, float("-inf"))
    lse = torch.logsumexp(sm, -1, keepdim=True)
    P = torch.exp(sm - lse)
    o = P @ vv
    Pk = torch.exp(s.masked_fill(~no_len, float("-inf")) - lse) if mut == "kvlen_ignored_dkdv" else P
    delta = (dd * o).sum(-1, keepdim=True)
    dP = dd @ vv.transpose(-1, -2)
    dS, dSk = P * (dP - delta), Pk * (dP - delta)
    dq = dS @ kk * sc
    dk = (dSk.transpose(-1, -2) @ qq * sc).reshape(B, Hkv, rep, Skv, D).sum(2)
    dv = (Pk.transpose(-1, -2) @ dd).reshape(B, Hkv, rep, Skv, D).sum(2)
    return dict(o=o.transpose(1, 2), dq=dq.transpose(1, 2), dk=dk.transpose(1, 2), dv=dv.transpose(1, 2))


# ------------------------------------------------------------------------------------------------ comparisons
def exact(got, want):
    """bit equality through integer views (NaN payloads and the sign of zero count)"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    return torch.equal(got.view(iv), want.view(iv))


def same_values(got, want):
    """equality by value: -0 == +0 (im2col's ReLU keeps no sign)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    return got.shape == want.shape and bool((got.float() == want.float()).all())


def bounded(got, ref, r=0, n=None, groups=None):
    """(error, bound) per group for `got` against ref(fp64), with y from ref(fp32): `ref` is a callable dt -> tensor"""
    r64, r32 = ref(torch.float64), ref(torch.float32)
    spec = R.out_spec(r=r, n=n, groups=groups)
    y = R.group_err(r32, r64, groups)
    e = R.group_err(got, r64, groups)
    return {g: (e[g], R.bound(spec, y[g])) for g in e}


def failures(res):
    return [g for g, (e, b) in res.items() if not e <= b]


def bilinear_check(got, x, Ho, Wo, align):
    return bounded(got, lambda dt: bilinear(x, Ho, Wo, align, dt), r=1)


# minmax_norm.  The issue's bound, r = 3, is 5 * 2^-8: wide enough for a kernel that skips both intermediate roundings (they move a value by at
# most 2 * 2^-9 of the row maximum), so a second criterion stands beside it.  The reference restates those roundings, so an honest kernel
# differs from it only through its division: a few fp32 ulps, <= 2^-21 relative, where one bf16 rounding interval is >= 2^-8 relative.  Were the
# quotients spread evenly, a fraction 2 * 2^-21 / 2^-8 = 2^-12 of them would lie within reach of a rounding boundary; each of those may land
# one bf16 ulp away.  Allowed: 1 % of the elements (a factor 40 above that), by one ulp.  Skipping the roundings moves tens of percent.
MINMAX_FLIP_FRACTION = 0.01
MINMAX_FLIP_ULPS = 1


def minmax_check(got, x):
    """group_err per image (rows whose reference is NaN, 0 / 0, are the caller's to compare) + the flip criterion on the finite rows"""
    B = x.shape[0]
    res = bounded(got, lambda dt: minmax(x, dt), r=3, groups={f"image{b}": [b] for b in range(B)})
    want = minmax(x, torch.float32).to(BF)
    fin = torch.isfinite(want.float()).all(1)
    if bool(fin.any()):
        g = got.detach().cpu()[fin]
        if not bool(torch.isfinite(g.float()).all()):
            res["flips"] = (R.INF, MINMAX_FLIP_FRACTION)
        else:
            frac, ulps = flips(g, want[fin])
            res["flips"] = (frac, MINMAX_FLIP_FRACTION)
            res["flip_ulps"] = (float(ulps), float(MINMAX_FLIP_ULPS))
    return res


def attention_failures(got, ref, kv_len, close):
    """The comparisons of test_attention_d128_dma_kernels_edges on the same operation: `close` (tests/test_kernels_gpu.py) on o, rtol 3e-2 on the
    gradients, exact zeros in dK / dV at keys >= kv_len.  -> the names that fail"""
    bad = []
    for name, kw in (("o", {}), ("dq", dict(rtol=3e-2)), ("dk", dict(rtol=3e-2)), ("dv", dict(rtol=3e-2))):
        try:
            close(got[name], ref[name], what=name, **kw)
        except AssertionError:
            bad.append(name)
    if kv_len is not None:
        for b, n in enumerate(kv_len):
            for name in ("dk", "dv"):
                if n < got[name].shape[1] and float(got[name][b, n:].float().abs().max()) != 0.0:
                    bad.append(f"{name} beyond kv_len")
    return bad


def flips(got, want):
    """(fraction of elements whose bf16 bits differ, largest difference in bf16 ulps) between two finite same-sign bf16 tensors"""
    a, b = got.detach().cpu().contiguous().view(torch.int16).int(), want.detach().cpu().contiguous().view(torch.int16).int()
    d = (a - b).abs()
    return float((d > 0).float().mean()), int(d.max())
