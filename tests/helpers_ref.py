"""Plain torch references of the bandwidth-bound helper kernels (csrc/elementwise.hip, csrc/conv.hip, the transposes of csrc/gemm.hip) and of
masked attention with its gradients and lse, shared by tests/test_helpers_host.py (CPU), tests/test_helpers_gpu.py,
tests/test_attention_generic_gpu.py and tests/test_attention_d128_gpu.py (whose cases, inputs and comparisons are the last section here).

Every reference runs in the float dtype `dt` it is given (fp32: what a kernel with fp32 math computes; fp64: the truth), restates the
kernel's documented bf16 rounding points with `bfr`, and leaves the LAST rounding of a bf16 output out (the caller applies `.to(BF)` where
the comparison is exact).  `mut` selects a MUTANT: the same reference with one plausible mistake.  tests/PATHS.md lists them.

Two kinds of comparison, see tests/test_helpers_gpu.py: `exact` (integer views, torch.equal) and `bounded` (regimes.group_err against the
fp64 reference, bound from regimes.bound with y = the fp32 reference's own error)."""
import math

import torch
import torch.nn.functional as F

import regimes as R
from regimes import BF, bfr, gen, randn

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
LOG2E = 1.4426950408889634
EMPTY_LSE = -1e30        # lse of a query row that sees no key (include/visper_hip.h)
ATTENTION_MUTANTS = ["block_first_key_dropped", "offset_dropped_after_first_block", "window_off_by_one", "kvlen_ignored_dkdv", "empty_row_nan",
                     "empty_row_uniform", "lse_natural_log", "lse_without_last_tile", "kv_head_modulo", "gqa_last_head_dropped_in_dkdv"]


def attention_mask(B, Sq, Skv, causal, kv_len=None, window=0, mut=None):
    """allow [B, 1, Sq, Skv]: the mask of test_kernels_gpu.attn_ref (causal with offset Skv - Sq, keys > i - window, keys < kv_len[b]).  Mutants:
    `window_off_by_one` (keys >= i - window), `block_first_key_dropped` (key 256 is invisible to rows >= 256: a second 256-row block that starts
    its key loop one key late), `offset_dropped_after_first_block` (Skv - Sq taken as 0 for rows >= 256)."""
    off = torch.full((Sq, 1), Skv - Sq)
    if mut == "offset_dropped_after_first_block":
        off[256:] = 0
    i = torch.arange(Sq)[:, None] + off
    j = torch.arange(Skv)[None, :]
    allow = torch.ones(Sq, Skv, dtype=torch.bool)
    if causal:
        allow &= j <= i
    if window > 0:
        allow &= (j >= i - window) if mut == "window_off_by_one" else (j > i - window)
    if mut == "block_first_key_dropped" and Skv > 256:
        allow[256:, 256] = False
    allow = allow[None, None].expand(B, 1, Sq, Skv).clone()
    if kv_len is not None:
        for b in range(B):
            allow[b, :, :, kv_len[b]:] = False
    return allow


def attention(q, k, v, do, causal, kv_len=None, window=0, dt=torch.float32, mut=None):
    """q / do [B, Sq, Hq, D], k / v [B, Skv, Hkv, D]: HF-eager masked softmax attention (attention_mask) and its gradients written out:
    P = softmax(S), dV = P^T dO, dS = P (dO V^T - rowsum(dO O)), dQ = dS K / sqrt(D), dK = dS^T Q / sqrt(D); lse [B, Hq, Sq] = log2 sum_j exp(S_ij)
    (the log2 domain of include/visper_hip.h).  A query row that sees no key (a window together with kv_len) has P = 0: o = 0, lse = EMPTY_LSE,
    dq = 0, nothing added to dk / dv (HF-eager's softmax yields NaN there; the header defines the kernels' value).
    Mutants (value-only): those of attention_mask; `kvlen_ignored_dkdv` (the dK / dV pass recomputes P from the row statistics without the kv_len
    term of its mask); `empty_row_nan` (an empty row's P is softmax of an all-masked row: NaN); `empty_row_uniform` (its P is 1 / Skv: o = the mean
    of all V); `lse_natural_log` (only lse changes); `lse_without_last_tile` (lse from the keys below the last started 64-key tile, everything else
    honest); `kv_head_modulo` (q head h reads kv head h % Hkv, not h // rep); `gqa_last_head_dropped_in_dkdv` (the last q head of each group is
    missing from dk / dv)."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    if mut == "kv_head_modulo":
        spread = lambda t: t.repeat(1, rep, 1, 1)                                                      # head h <- kv head h % Hkv
        gather = lambda t: t.reshape(B, rep, Hkv, Skv, D).sum(1)
    else:
        spread = lambda t: t.repeat_interleave(rep, dim=1)                                             # head h <- kv head h // rep
        gather = lambda t: t.reshape(B, Hkv, rep, Skv, D)[:, :, :rep - (mut == "gqa_last_head_dropped_in_dkdv")].sum(2)
    qq, dd = q.to(dt).transpose(1, 2), do.to(dt).transpose(1, 2)
    kk, vv = spread(k.to(dt).transpose(1, 2)), spread(v.to(dt).transpose(1, 2))
    sc = 1.0 / math.sqrt(D)
    s = qq @ kk.transpose(-1, -2) * sc
    allow = attention_mask(B, Sq, Skv, causal, kv_len, window, mut)
    empty = ~allow.any(-1, keepdim=True)                                                               # [B, 1, Sq, 1]
    sm = s.masked_fill(~allow, float("-inf"))
    lse = torch.logsumexp(sm.masked_fill(empty, 0.0), -1, keepdim=True)                                # (a finite placeholder on empty rows)
    P = torch.exp(sm - lse)                                                                            # exp(-inf) = 0 on empty rows
    lse2 = (lse * LOG2E).masked_fill(empty, EMPTY_LSE)
    if mut == "empty_row_nan":
        P, lse2 = P.masked_fill(empty, float("nan")), lse2.masked_fill(empty, float("nan"))
    elif mut == "empty_row_uniform":
        P, lse2 = P.masked_fill(empty, 1.0 / Skv), lse2.masked_fill(empty, math.log2(Skv))
    elif mut == "lse_natural_log":
        lse2 = lse.masked_fill(empty, EMPTY_LSE)
    elif mut == "lse_without_last_tile":
        j = torch.arange(Skv)
        last = (allow * j).amax(-1, keepdim=True)                                                      # the row's last visible key
        below = allow & (j < last // 64 * 64)
        none = ~below.any(-1, keepdim=True)
        lse2 = (torch.logsumexp(s.masked_fill(~below, float("-inf")).masked_fill(none, 0.0), -1, keepdim=True) * LOG2E).masked_fill(none, EMPTY_LSE)
    o = P @ vv
    Pk = P
    if mut == "kvlen_ignored_dkdv":
        Pk = torch.exp(s.masked_fill(~attention_mask(B, Sq, Skv, causal, None, window), float("-inf")) - lse)
    delta = (dd * o).sum(-1, keepdim=True)
    dP = dd @ vv.transpose(-1, -2)
    dS, dSk = P * (dP - delta), Pk * (dP - delta)
    dq = dS @ kk * sc
    dk = gather(dSk.transpose(-1, -2) @ qq * sc)
    dv = gather(Pk.transpose(-1, -2) @ dd)
    return dict(o=o.transpose(1, 2), dq=dq.transpose(1, 2), dk=dk.transpose(1, 2), dv=dv.transpose(1, 2), lse=lse2[..., 0].expand(B, Hq, Sq))


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


# ------------------------------------------------------------------------------------------------ D = 128 / 96 attention at block edges
# tests/ATTENTION_D128.md maps each case to the path it enters.  (B, Hq, Hkv, Sq, Skv, causal, window, kv_len); each runs at D = 128 and D = 96.
D128_CASES = {
    "three-blocks-one-row": (1, 2, 1, 513, 513, True, 0, None),
    "offset-across-blocks": (1, 4, 2, 300, 600, True, 0, None),
    "window-kstart": (2, 2, 2, 600, 600, True, 70, None),
    "window-kvlen-empty": (2, 2, 1, 600, 600, True, 64, [600, 130]),
    "noncausal-kvlen": (1, 2, 2, 260, 700, False, 0, [650]),
    "gqa-permuted": (1, 8, 2, 520, 520, True, 0, None),
}
D128_DIMS = (128, 96)
D128_BLOCK = 256         # query rows / keys per block of the forward and of the default backward
# the case each mutant is aimed at
D128_MUTANT_CASE = {
    "block_first_key_dropped": "three-blocks-one-row", "offset_dropped_after_first_block": "offset-across-blocks", "window_off_by_one": "window-kstart",
    "kvlen_ignored_dkdv": "noncausal-kvlen", "empty_row_nan": "window-kvlen-empty", "empty_row_uniform": "window-kvlen-empty",
    "lse_natural_log": "three-blocks-one-row", "lse_without_last_tile": "noncausal-kvlen", "kv_head_modulo": "gqa-permuted",
    "gqa_last_head_dropped_in_dkdv": "gqa-permuted"}
# bf16 roundings on the path to each output (the fp64 reference restates none): o: P as a bf16 MFMA operand, the output; dv: P, the output;
# dq, dk: the two of o (through delta = rowsum(dO o O) from the bf16 o), dS as a bf16 MFMA operand, the output.  The same points in all five
# kernels (attention_bwd64.h:29; attention_d128.h: pk / dsk packs of the DMA-ring pair, pf of the forward; attention.hip pack8 of the 16-row forward).
D128_ROUNDINGS = dict(o=2, dv=2, dq=4, dk=4)


def d128_inputs(name, D, kind):
    """kind "random": N(0, 1) bf16 q, k, v, do.  kind "exact": q = 0, k random, v[j, d] = (d == j % D): every visible score is exactly 0, so
    m = 0, p = 1, l = n (the number of visible keys) and the accumulators hold integer counts."""
    B, Hq, Hkv, Sq, Skv, causal, window, kvl = D128_CASES[name]
    seed = 500 + 10 * sorted(D128_CASES).index(name) + (D == 96) * 100
    q, k, v, do = randn(B, Sq, Hq, D, seed=seed), randn(B, Skv, Hkv, D, seed=seed + 1), randn(B, Skv, Hkv, D, seed=seed + 2), randn(B, Sq, Hq, D, seed=seed + 3)
    if kind == "exact":
        q = torch.zeros_like(q)
        v = (torch.arange(D)[None, :] == (torch.arange(Skv) % D)[:, None]).to(BF)[None, :, None, :].expand(B, Skv, Hkv, D).contiguous()
    return dict(q=q, k=k, v=v, do=do)


def d128_counts(name, D):
    """-> n [B, Sq] visible keys per row, cnt [B, Sq, D] visible keys j with j % D == d (int64)"""
    B, Hq, Hkv, Sq, Skv, causal, window, kvl = D128_CASES[name]
    allow = attention_mask(B, Sq, Skv, causal, kvl, window)[:, 0]
    onehot = (torch.arange(D)[None, :] == (torch.arange(Skv) % D)[:, None]).long()
    return allow.sum(-1), allow.long() @ onehot


_D128_REFS = {}


def d128_refs(name, D, kind):
    """(inputs, fp64 reference, fp32 reference), computed once per process and left unchanged"""
    key = (name, D, kind)
    if key not in _D128_REFS:
        B, Hq, Hkv, Sq, Skv, causal, window, kvl = D128_CASES[name]
        inp = d128_inputs(name, D, kind)
        _D128_REFS[key] = (inp,) + tuple(attention(inp["q"], inp["k"], inp["v"], inp["do"], causal, kvl, window, dt) for dt in (torch.float64, torch.float32))
    return _D128_REFS[key]


def d128_simulate(name, D, kind, mut=None):
    """what a kernel with fp32 math returns: the fp32 reference (or a mutant of it), o / dq / dk / dv rounded to bf16, lse fp32"""
    B, Hq, Hkv, Sq, Skv, causal, window, kvl = D128_CASES[name]
    inp = d128_refs(name, D, kind)[0]
    out = d128_refs(name, D, kind)[2] if mut is None else attention(inp["q"], inp["k"], inp["v"], inp["do"], causal, kvl, window, torch.float32, mut)
    return {n: (t.float() if n == "lse" else t.to(BF)) for n, t in out.items()}


def _blocks(n, dim):
    return {f"block{i}": (slice(None),) * dim + (slice(i * D128_BLOCK, min(n, (i + 1) * D128_BLOCK)),) for i in range((n + D128_BLOCK - 1) // D128_BLOCK)}


def d128_compare(name, D, kind, got):
    """The comparisons of tests/test_attention_d128_gpu.py on `got` (o, lse and, if present, dq, dk, dv; CPU tensors).
    -> (bounded {label: (error, bound)}, exact [what failed]).
    bounded: lse by absolute error over the non-empty rows per q block, bound the fp32 sum form with n = Skv; o / dq per q block and dk / dv per key
    block against fp64 with D128_ROUNDINGS, the gradients normalised by the tensor maximum.  exact: everything finite; o, dq zero and
    lse = EMPTY_LSE on empty rows; dk / dv zero at keys >= kv_len; kind "exact" also round(2^lse) = n, o bit-equal to bf16(cnt / n), dk zero."""
    B, Hq, Hkv, Sq, Skv, causal, window, kvl = D128_CASES[name]
    inp, r64, r32 = d128_refs(name, D, kind)
    n, cnt = d128_counts(name, D)
    empty = n == 0                                                                     # [B, Sq]
    res, bad = {}, []
    for nm, t in got.items():
        if not bool(torch.isfinite(t.float()).all()):
            bad.append(f"{nm} is not finite")
    hide = empty[:, None, :].expand(B, Hq, Sq)
    lse = got["lse"].float()
    if not bool((lse[hide] == EMPTY_LSE).all()):
        bad.append("lse of an empty row is not -1e30")
    qg3 = _blocks(Sq, 2)
    want, have = r64["lse"].masked_fill(hide, float("inf")), lse.masked_fill(hide, 0.0)          # group_err leaves non-finite references out
    y, e = R.group_err(r32["lse"].masked_fill(hide, 0.0), want, qg3, 1.0), R.group_err(have, want, qg3, 1.0)
    if kind == "random":
        for g in e:
            res[f"lse[{g}]"] = (e[g], R.bound(R.out_spec(n=Skv), y[g]))
    for nm, blocks in (("o", _blocks(Sq, 1)), ("dq", _blocks(Sq, 1)), ("dk", _blocks(Skv, 1)), ("dv", _blocks(Skv, 1))):
        if nm not in got or (kind == "exact" and nm in ("o", "dk")):
            continue
        norm = None if nm == "o" else float(r64[nm].abs().max())
        y, e = R.group_err(r32[nm], r64[nm], blocks, norm), R.group_err(got[nm], r64[nm], blocks, norm)
        for g in e:
            res[f"{nm}[{g}]"] = (e[g], R.bound(R.out_spec(r=D128_ROUNDINGS[nm]), y[g]))
    for nm in ("o", "dq"):
        if nm in got and not bool((got[nm].float()[empty] == 0).all()):
            bad.append(f"{nm} of an empty row is not zero")
    if kvl is not None:
        for b, kl in enumerate(kvl):
            for nm in ("dk", "dv"):
                if nm in got and kl < Skv and not bool((got[nm][b, kl:].float() == 0).all()):
                    bad.append(f"{nm} beyond kv_len")
    if kind == "exact":
        full = n[:, None, :].expand(B, Hq, Sq)
        if not bool((torch.round(torch.exp2(lse.double()))[~hide] == full[~hide].double()).all()):
            bad.append("round(2^lse) is not the number of visible keys")
        o_want = (cnt.double() / n.clamp_min(1)[..., None].double()).to(BF)[:, :, None, :].expand(B, Sq, Hq, D)
        if not exact(got["o"], o_want):
            bad.append("o is not bf16(cnt / n)")
        if "dk" in got and not bool((got["dk"].float() == 0).all()):
            bad.append("dk is not zero with q = 0")
    return res, bad
