"""The bandwidth-bound helper kernels (csrc/elementwise.hip, csrc/conv.hip, the transposes of csrc/gemm.hip) against the references of
tests/helpers_ref.py, at the shapes that enter every flag value, template instantiation, lane / column tail, stride form and the SECOND SWEEP
of every grid-stride loop (tests/PATHS.md maps each path to its case here).

Two kinds of comparison:
  exact    torch.equal on integer views.  Data movement (im2col by value: its ReLU keeps no sign of zero; pixel shuffle, transposes,
           gather_rows, copy2d, scatter_rows, both casts), add / add2d (one fp32 add of two bf16 values, rounded once), RoPE (fp32 products of
           bf16 values are exact, each is rounded to bf16, their sum is rounded once: replayed on the CPU), and the reductions on small-integer
           inputs (every partial sum an integer below 2^24: any order gives the same bits, a dropped or doubled term cannot hide).
  bounded  regimes.group_err against the fp64 reference, bound (2 r - 1) 2^-8 + 4 y for a bf16 output with r roundings, the two fp32 forms of
           tests/regimes.py for fp32 outputs; y = the fp32 reference's own error.  Bilinear (r = 1), minmax_norm (r = 3), dwconv7x7 (r = 1),
           the random-valued runs of the reductions, SwiGLU and the activations at the wrap size.  The library is built with -ffast-math:
           divisions are not correctly rounded and multiply-adds may be contracted, so these are not compared for equality.

Every output is a view inside a larger allocation filled with a sentinel bit pattern (padded columns where the ABI takes a stride, 64
elements before and after otherwise); after the call every byte outside the view is unchanged.  Every index handed to a kernel is in range or
a documented negative skip."""
import ctypes as C

import pytest
import torch

import helpers_ref as HR
import parity
import regimes as R
from regimes import BF, NS, gen, randn

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
I32 = torch.int32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops as o
    return o


def dev(t):
    return t.cuda()


class Guarded:
    """A strided view (sizes, strides in elements) inside a 1-D allocation with `pad` elements before and after it.  `fill` = the view's initial
    content (default: the sentinel everywhere); everything else holds the sentinel.  `untouched()` after the call: every element outside the view
    has its bits unchanged."""
    SENT = {BF: (torch.int16, 0x7A5A), F32: (torch.int32, 0x7A5A5A5A)}

    def __init__(self, sizes, strides=None, dtype=BF, pad=64, offset=0, fill=None):
        sizes = tuple(sizes)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(sizes):
                strides.insert(0, acc)
                acc *= s
        extent = sum((s - 1) * st for s, st in zip(sizes, strides)) + 1
        n = pad + offset + extent + pad
        it, bits = self.SENT[dtype]
        self.buf = torch.full((n,), bits, dtype=it).view(dtype).cuda()
        self.view = torch.as_strided(self.buf, sizes, tuple(strides), pad + offset)
        self.mask = torch.zeros(n, dtype=torch.bool)
        torch.as_strided(self.mask, sizes, tuple(strides), pad + offset).fill_(True)
        if fill is not None:
            self.view.copy_(fill)
        self.before = self.buf.cpu()

    def untouched(self):
        after = self.buf.cpu()
        return HR.exact(after[~self.mask], self.before[~self.mask])

    def cpu(self):
        return self.view.cpu()


def rows_view(rows, cols, ld, dtype=BF, fill=None, offset=0):
    return Guarded((rows, cols), (ld, 1), dtype, fill=fill, offset=offset)


def check(label, res):
    """every (error, bound) pair of a bounded comparison through parity.check, all of them before the first failure is raised"""
    R.check_all(label, {("", g): v for g, v in res.items()})


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ================================================================================================ elementwise.hip: exact
# GRID_FOR caps the grid at 2048 blocks of 256 threads: 524 288 work items per sweep.  add / act: one item = 8 elements.
@pytest.mark.parametrize("n", [8, 8 * 1000, HR.EW_CAP * 256 * 8 + 8 * 300])
def test_add(ops, n):
    """exact; n = 4 194 304 + 2400: second sweep with a partial last block"""
    a, b = randn(n, seed=1), randn(n, seed=2, scale=3.0)
    out = Guarded((n,))
    ops.add(dev(a), dev(b), out=out.view)
    assert HR.exact(out.cpu(), a + b)                       # torch's bf16 add on the CPU: the fp32 sum rounded once
    assert out.untouched()


# add2d / copy2d / swiglu: one item = 8 columns of a row; R = 2050 rows of 2048 columns = 2050 * 256 items > 2048 * 256
@pytest.mark.parametrize("Rr,Cc", [(3, 8), (37, 264), (2050, 2048)])
def test_add2d_copy2d(ops, Rr, Cc):
    """exact, strided on both sides; add2d is in place: the padded columns of dst are compared with what they held"""
    d0, s0 = randn(Rr, Cc, seed=3), randn(Rr, Cc, seed=4, scale=0.5)
    src = rows_view(Rr, Cc, Cc + 16, fill=s0)
    dst = rows_view(Rr, Cc, Cc + 8, fill=d0)
    ops.add2d_(dst.view, src.view)
    assert HR.exact(dst.cpu(), d0 + s0) and dst.untouched() and src.untouched()
    cp = rows_view(Rr, Cc, Cc + 24)
    ops.copy2d_(cp.view, src.view)
    assert HR.exact(cp.cpu(), s0) and cp.untouched()


@pytest.mark.parametrize("n", [1, 255, 257, HR.EW_CAP * 256 + 300])          # casts: one item = one element
def test_casts(ops, n):
    """exact.  f32 -> bf16 is round-to-nearest-even: exact ties above an even and above an odd bf16, a carry into the next binade, both signs.
    bf16 -> f32 with accumulate = 1 is one fp32 add."""
    x = torch.randn(n, generator=gen(5)) * 4.0
    edge = torch.tensor([0x3F808000, 0x3F818000, 0x3FFFC000, 0x3FFF8000, 0x3F807FFF, 0x3F808001, 0x7F7F7FFF], dtype=torch.int32)
    edge = torch.cat([edge, edge | torch.tensor(-0x80000000, dtype=torch.int32)]).view(F32)
    k = min(n, edge.numel())
    x[n - k:] = edge[:k]                                    # in the last (second-sweep) elements too
    out = Guarded((n,))
    ops.cast_to_bf16(dev(x), out=out.view)
    assert HR.exact(out.cpu(), x.to(BF)) and out.untouched()
    if n > 14:
        got = out.cpu()[n - 14:].view(torch.int16).int() & 0xFFFF
        assert got.tolist()[:7] == [0x3F80, 0x3F82, 0x4000, 0x4000, 0x3F80, 0x3F81, 0x7F7F]      # ties to even, carry, just below / above a tie
    b = randn(n, seed=6, scale=2.0)
    y0 = torch.randn(n, generator=gen(7))
    for acc in (0, 1):
        y = Guarded((n,), dtype=F32, fill=y0)
        ops.cast_to_f32(dev(b), out=y.view, accumulate=bool(acc))
        assert HR.exact(y.cpu(), y0 + b.float() if acc else b.float()), acc
        assert y.untouched()


ROPE_CASES = [(hd, T, S, nh, mode) for hd in (32, 64, 96, 128) for (T, S, nh, mode) in ((50, 16, 3, "mod"), (50, 16, 3, "ids"))]
# second sweep: T * nheads * head_dim / 16 = 4100 * 16 * 8 = 524 800 items > 2048 * 256
ROPE_CASES.append((128, 4100, 1000, 16, "ids"))


@pytest.mark.parametrize("hd,T,S,nh,mode", ROPE_CASES)
def test_rope(ops, hd, T, S, nh, mode):
    """exact, forward and inverse: pos = NULL with T no multiple of S (row t takes t % S), explicit ids that are not monotone, repeat and include
    S - 1; ld > nheads * head_dim, the other columns untouched.  inverse(forward(x)) == x is NOT asserted: the roundings do not invert."""
    ld = nh * hd + 24
    x = randn(T, ld, seed=8 + hd)
    cs, sn = HR.rope_tables(S, hd, 10000.0 if hd != 128 else 500000.0)
    pos = None
    if mode == "ids":
        pos = torch.randint(0, S, (T,), generator=gen(9)).to(I32)
        pos[0], pos[1], pos[2], pos[T - 1] = S - 1, 0, S - 1, 5 % S
    for inverse in (False, True):
        g = rows_view(T, ld, ld, fill=x)                    # the whole padded row is the view's content; rope gets the first nh * hd columns
        ops.rope_(g.view, T, S, nh, hd, dev(cs), dev(sn), pos=None if pos is None else dev(pos), inverse=inverse)
        want = HR.rope(x, cs, sn, pos, nh, hd, inverse).to(BF)
        assert HR.exact(g.cpu(), want), (hd, mode, inverse)
        assert g.untouched()
        assert HR.exact(g.cpu()[:, nh * hd:], x[:, nh * hd:])


@pytest.mark.parametrize("n,H,V,dup", [(400, 64, 50, True), (37, 8, 40, False), (8200, 512, 8300, False)])
def test_scatter_add_rows(ops, n, H, V, dup):
    """exact on small integers (atomics in any order give the same bits): duplicate indices and negative skips; n = 8200 rows of 512 = 524 800
    items of 8 columns: second sweep, unique indices; lds > H"""
    src = HR.ints(n, H, seed=10)
    idx = (torch.randint(-1, V, (n,), generator=gen(11)) if dup else torch.randperm(V, generator=gen(11))[:n]).to(I32)
    if not dup:
        idx[3] = -1
    d0 = HR.ints(V, H, seed=12).float()
    dst = Guarded((V, H), dtype=F32, fill=d0)
    s = rows_view(n, H, H + 8, fill=src)
    ops.scatter_add_rows_(dst.view, s.view, dev(idx))
    assert HR.exact(dst.cpu(), HR.scatter_add_rows(src, idx, d0)) and dst.untouched()


LANE_H = [8, 504, 512, 520, 1032]      # `for (e = lane * 8; e < H; e += 512)`: idle lanes, one lane idle, exactly one pass, a second pass with one / two live lanes


@pytest.mark.parametrize("n,H", [(9, h) for h in LANE_H] + [(HR.SCATTER_ROWS_CAP * 4 + 5, 8)])        # 8192 blocks of 4 rows: 32 768 + 5 rows wrap
def test_scatter_rows(ops, n, H):
    """exact (a widening): permuted rows with a negative skip into a wider fp32 matrix (ldd > H, lds > H), and idx = NULL row for row"""
    src = randn(n, H, seed=13)
    s = rows_view(n, H, H + 8, fill=src)
    nd = n + 3
    idx = torch.randperm(nd, generator=gen(14))[:n].to(I32)
    idx[n // 2] = -1
    for ix in (idx, None):
        d = rows_view(nd, H, H + 4, dtype=F32)
        ops.scatter_rows_to_f32(s.view, None if ix is None else dev(ix), d.view if ix is not None else d.view[:n])
        assert HR.exact(d.cpu(), HR.scatter_rows(src, ix, d.before[d.mask].view(nd, H), H)) and d.untouched()


@pytest.mark.parametrize("n,H", [(9, h) for h in LANE_H] + [(HR.GATHER_ROWS_CAP * 4 + 5, 8)])          # 4096 blocks of 4 rows: 16 384 + 5 rows wrap
def test_gather_rows(ops, n, H):
    """exact: three sources with ld > H (two) and ld == H, ldo > H (through the C ABI: ops.gather_rows passes ldo = H), zero rows for kind < 0"""
    lds = (H + 8, H + 24, H)
    nsrc_rows = (10, 7, 5)
    srcs = [randn(r, H, seed=15 + i) for i, r in enumerate(nsrc_rows)]
    gs = [rows_view(r, H, ld, fill=s) for r, ld, s in zip(nsrc_rows, lds, srcs)]
    kind = torch.randint(-1, 3, (n,), generator=gen(18)).to(I32)
    kind[0], kind[n - 1] = -1, 2
    row = (torch.rand(n, generator=gen(19)) * torch.tensor(nsrc_rows)[kind.clamp_min(0).long()]).long().to(I32)       # < rows of its source
    assert all(0 <= int(r) < nsrc_rows[int(k)] for k, r in zip(kind, row) if k >= 0)
    out = rows_view(n, H, H + 16)
    arr_p = (C.c_void_p * 3)(*[g.view.data_ptr() for g in gs])
    arr_l = (C.c_long * 3)(*lds)
    d_kind, d_row = dev(kind), dev(row)
    ops._lib.call("vp_gather_rows", n, H, arr_p, arr_l, 3, p(d_kind), p(d_row), p(out.view), H + 16, ops._stream())
    torch.cuda.synchronize()
    want = HR.gather_rows(srcs, kind, row, H, out.before[out.mask].view(n, H))
    assert HR.exact(out.cpu(), want) and out.untouched()


GS_H = [8, 250, 256, 264, 520]         # one thread per column, 256-column blocks: a partial block, exactly one, a second block with 8 / 8 live threads


@pytest.mark.parametrize("src_f32", [False, True])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("n,H,cnt", [(7, h, c) for h in GS_H for c in (1, 3)] + [(HR.GATHER_SUM_CAP + 5, 8, 3)])      # grid.y caps at 8192 rows
def test_gather_sum_rows(ops, n, H, cnt, src_f32, out_f32):
    """all four instantiations, accumulate off and (fp32 output) on, cnt 1 and 3, skipped (< 0) indices, lds > H, ldo > H, scale a power of two.
    exact on small integers; then random values, bounded (fp32 output: a sum of cnt terms; bf16 output: one rounding)."""
    nsrc = 11
    idx = torch.randint(-1, nsrc, (n * cnt,), generator=gen(20)).to(I32)
    idx[0] = -1
    for kind in ("ints", "random"):
        src = HR.ints(nsrc, H, seed=21).float() if kind == "ints" else torch.randn(nsrc, H, generator=gen(22))
        src = src if src_f32 else src.to(BF)
        s = rows_view(nsrc, H, H + 8, dtype=F32 if src_f32 else BF, fill=src)
        for acc in ((False, True) if out_f32 else (False,)):
            o0 = (HR.ints(n, H, seed=23).float() if kind == "ints" else torch.randn(n, H, generator=gen(24)))
            o0 = o0 if out_f32 else o0.to(BF)
            out = rows_view(n, H, H + 8, dtype=F32 if out_f32 else BF, fill=o0)
            scale = 0.5 if kind == "ints" else 0.375
            ops.gather_sum_rows(s.view, dev(idx), cnt, scale, out.view, accumulate=acc)
            ref = lambda dt: HR.gather_sum_rows(src, idx, cnt, scale, o0, H, acc, dt)
            if kind == "ints":
                assert HR.exact(out.cpu(), ref(F32).to(out.view.dtype)), (kind, acc)
            else:
                check(f"gather_sum_rows n{n} H{H} cnt{cnt} src32={src_f32} out32={out_f32} acc={acc}",
                      HR.bounded(out.cpu(), ref, r=0 if out_f32 else 1, n=cnt + 1 if out_f32 else None))
            assert out.untouched() and s.untouched()


@pytest.mark.parametrize("M", [1, 70, 257, 1000])              # ops.colsum: rows per slab = ceil(M / 256); M = 257: two rows per slab, a short last slab
@pytest.mark.parametrize("N", [1, 63, 64, 70, 300])           # 256-column blocks of the partial kernel, 64-column blocks of the finish
def test_colsum(ops, M, N):
    """vp_colsum_partial + vp_colsum_finish with ld > N, accumulate and scale.  exact on small integers (|x| <= 8, M <= 1000 terms), bounded on
    random values (fp32 output summing M terms)."""
    o0 = HR.ints(N, seed=30).float()
    for kind in ("ints", "random"):
        x = HR.ints(M, N, seed=31) if kind == "ints" else randn(M, N, seed=32)
        g = rows_view(M, N, N + 5, fill=x)                   # bf16 scalar loads: any ld
        for acc, scale in ((False, 1.0), (True, 0.25), (False, 2.0)):
            out = Guarded((N,), dtype=F32, fill=o0)
            ops.colsum(g.view, out=out.view, accumulate=acc, scale=scale)
            ref = lambda dt: HR.colsum_finish(HR.colsum_partial(x, N, HR.colsum_rpb(M), dt), scale, acc, o0, dt)
            if kind == "ints":
                assert HR.exact(out.cpu(), ref(F32)), (M, N, acc, scale)
            else:
                check(f"colsum M{M} N{N} acc={acc} scale={scale}", HR.bounded(out.cpu(), ref, n=M + 1))
            assert out.untouched()


@pytest.mark.parametrize("nslab", [1, 3, 4, 13, 16, 17, 29])   # 4 waves stride the slabs by 4, unrolled by 16: every remainder of both loops
def test_colsum_finish_direct(ops, nslab):
    """vp_colsum_finish on host-made partials; exact on small integers, with accumulate and a power-of-two scale"""
    N = 70
    part = HR.ints(nslab, N, seed=33).float() * torch.arange(1, nslab + 1)[:, None].float()       # a slab's weight tells which slab was dropped
    o0 = HR.ints(N, seed=34).float()
    for acc, scale in ((False, 1.0), (True, 0.5), (False, 4.0)):
        out = Guarded((N,), dtype=F32, fill=o0)
        d_part = dev(part)
        ops._lib.call("vp_colsum_finish", nslab, N, p(d_part), p(out.view), scale, int(acc), ops._stream())
        torch.cuda.synchronize()
        assert HR.exact(out.cpu(), HR.colsum_finish(part, scale, acc, o0)), (nslab, acc, scale)
        assert out.untouched()


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000])     # sum_f32_kernel: ONE block of 1024 threads, `i += 1024`
def test_sum_f32(ops, n):
    """exact on small integers with a power-of-two scale; bounded on random values (n terms)"""
    x = HR.ints(n, seed=35).float()
    x[n - 1] = 7.0                                           # the last element is never a zero
    out = Guarded((1,), dtype=F32)
    ops.sum_f32(dev(x), 0.5, out=out.view)
    assert HR.exact(out.cpu(), HR.sum_f32(x, 0.5)) and out.untouched()
    xr = torch.randn(n, generator=gen(36))
    got = ops.sum_f32(dev(xr), 0.5)
    check(f"sum_f32 n{n}", HR.bounded(got.cpu(), lambda dt: HR.sum_f32(xr, 0.5, dt), n=n))


@pytest.mark.parametrize("n", [1, 4095, 4097, 100003, HR.SUMSQ_CAP * 4096 + 1000])      # vp_sumsq_nblk: ceil(n / 4096) blocks, at most 1024: 4 194 304 + 1000 wraps
def test_sumsq(ops, n):
    """exact on {-1, 0, 1} with 2s in the last elements (the sum stays below 2^24); bounded on random values"""
    x = torch.randint(-1, 2, (n,), generator=gen(37)).float()
    x[max(0, n - 1000):] = 2.0
    assert HR.exact(ops.sumsq(dev(x)).cpu(), HR.sumsq(x))
    xr = torch.randn(n, generator=gen(38))
    check(f"sumsq n{n}", HR.bounded(ops.sumsq(dev(xr)).cpu(), lambda dt: HR.sumsq(xr, dt), n=n))


# ================================================================================================ elementwise.hip: bounded, at the wrap size
def _sweeps(rows_first):
    return {"sweep1": slice(0, rows_first), "sweep2": slice(rows_first, None)}


@pytest.mark.parametrize("il", [True, False])
def test_swiglu_second_sweep(ops, il):
    """R = 2050 rows of F = 2048: 2050 * 256 items; the rows of the second sweep are a group of their own.  References of tests/regimes.py."""
    from test_kernels_gpu import _ileave
    Rr, Fd = 2050, 2048
    inp = NS(gate=randn(Rr, Fd, seed=40, scale=2.0), up=randn(Rr, Fd, seed=41), dact=randn(Rr, Fd, seed=42))
    gu = torch.cat([inp.gate, inp.up], 1)
    lay = (lambda t: _ileave(t, Fd)) if il else (lambda t: t)
    gud = rows_view(Rr, 2 * Fd, 2 * Fd + 8, fill=lay(gu))
    act = Guarded((Rr, Fd))
    ops._lib.call("vp_swiglu_fwd", Rr, Fd, p(gud.view), 2 * Fd + 8, p(act.view), Fd, int(il), ops._stream())
    dgu = rows_view(Rr, 2 * Fd, 2 * Fd + 8)
    d_inp_dact = dev(inp.dact)
    ops._lib.call("vp_swiglu_bwd", Rr, Fd, p(d_inp_dact), Fd, p(gud.view), p(dgu.view), 2 * Fd + 8, int(il), ops._stream())
    torch.cuda.synchronize()
    gr = _sweeps(HR.EW_CAP * 256 // (Fd // 8))
    refs = {dt: R.swiglu_ref(inp, dt) for dt in (F64, F32)}          # computed once, shared by the comparisons below
    check(f"swiglu wrap il={il} act", HR.bounded(act.cpu(), lambda dt: refs[dt]["act"], r=2, groups=gr))
    check(f"swiglu wrap il={il} dgate|dup", HR.bounded(dgu.cpu(), lambda dt: lay(torch.cat([refs[dt]["dgate"], refs[dt]["dup"]], 1)), r=1, groups=gr))
    assert act.untouched() and dgu.untouched() and gud.untouched()


@pytest.mark.parametrize("kind", [R.ACT_GELU, R.ACT_RELU])
def test_act_second_sweep(ops, kind):
    """n = 4 194 304 + 2400 (items of 8): the elements of the second sweep are a group of their own"""
    n = HR.EW_CAP * 256 * 8 + 8 * 300
    inp = NS(x=randn(1, n, seed=43, scale=2.0), dy=randn(1, n, seed=44), kind=kind)
    y, dx = Guarded((1, n)), Guarded((1, n))
    d_inp_x = dev(inp.x)
    ops._lib.call("vp_act_fwd", kind, n, p(d_inp_x), p(y.view), ops._stream())
    d_inp_dy, d_inp_x = dev(inp.dy), dev(inp.x)
    ops._lib.call("vp_act_bwd", kind, n, p(d_inp_dy), p(d_inp_x), p(dx.view), ops._stream())
    torch.cuda.synchronize()
    gr = {"sweep1": (Ellipsis, slice(0, HR.EW_CAP * 256 * 8)), "sweep2": (Ellipsis, slice(HR.EW_CAP * 256 * 8, None))}
    refs = {dt: R.act_ref(inp, dt) for dt in (F64, F32)}
    check(f"act {kind} wrap y", HR.bounded(y.cpu(), lambda dt: refs[dt]["y"], r=1, groups=gr))
    check(f"act {kind} wrap dx", HR.bounded(dx.cpu(), lambda dt: refs[dt]["dx"], r=1, groups=gr))
    assert y.untouched() and dx.untouched()


# ================================================================================================ conv.hip
# conv.hip's GRID_FOR caps at 8192 blocks of 256: 2 097 152 items of 8 channels per sweep
IM2COL = [(2, h, w, c, s, r) for (h, w) in ((1, 1), (2, 3), (5, 13), (12, 10)) for c in (8, 24) for s in (1, 2) for r in (0, 1)]
IM2COL.append((1, 484, 484, 8, 1, 1))                          # 484 * 484 * 9 = 2 108 304 items: second sweep


@pytest.mark.parametrize("B,H,W,Cc,stride,relu", IM2COL)
def test_im2col(ops, B, H, W, Cc, stride, relu):
    """exact BY VALUE (the ReLU turns -x into +0 where the reference may hold -0)"""
    x = randn(B, H, W, Cc, seed=50)
    want = HR.im2col3x3(x, stride, relu).to(BF)
    col = Guarded(tuple(want.shape))
    d_x = dev(x)
    ops._lib.call("vp_im2col3x3_nhwc", B, H, W, Cc, stride, relu, p(d_x), p(col.view), ops._stream())
    torch.cuda.synchronize()
    assert HR.same_values(col.cpu(), want) and col.untouched()


@pytest.mark.parametrize("B,H,W,k,Cc", [(2, 5, 3, k, c) for k in (1, 2, 4) for c in (8, 24)] + [(1, 363, 363, 4, 8)])      # 363 * 363 * 16 items: second sweep
def test_pixel_shuffle(ops, B, H, W, k, Cc):
    """exact; H != W"""
    t = randn(B * H * W, k * k * Cc, seed=51)
    y = Guarded((B, H * k, W * k, Cc))
    d_t = dev(t)
    ops._lib.call("vp_pixel_shuffle_nhwc", B, H, W, k, Cc, p(d_t), p(y.view), ops._stream())
    torch.cuda.synchronize()
    assert HR.exact(y.cpu(), HR.pixel_shuffle(t, B, H, W, k, Cc)) and y.untouched()


BILINEAR = [(2, 12, 10, 16, 17, 31), (2, 12, 10, 16, 24, 20), (2, 12, 10, 16, 12, 10), (2, 24, 20, 8, 7, 9), (2, 12, 10, 8, 1, 15), (2, 12, 10, 8, 9, 1),
            (2, 1, 1, 8, 5, 7), (1, 37, 37, 8, 1450, 1450)]    # 1450 * 1450 = 2 102 500 items: second sweep


@pytest.mark.parametrize("align", [1, 0])
@pytest.mark.parametrize("B,H,W,Cc,Ho,Wo", BILINEAR)
def test_bilinear(ops, B, H, W, Cc, Ho, Wo, align):
    """bounded, r = 1: both align_corners modes on a non-integer upscale, 2x, identity, a downscale, Ho = 1, Wo = 1, a 1 x 1 input"""
    x = randn(B, H, W, Cc, seed=52)
    y = Guarded((B, Ho, Wo, Cc))
    d_x = dev(x)
    ops._lib.call("vp_bilinear_nhwc", B, H, W, Cc, Ho, Wo, align, p(d_x), p(y.view), ops._stream())
    torch.cuda.synchronize()
    check(f"bilinear {H}x{W}->{Ho}x{Wo} align={align}", HR.bilinear_check(y.cpu(), x, Ho, Wo, align))
    assert y.untouched()


@pytest.mark.parametrize("n", [1, 63, 1000, 1024, 1025, 3000])      # one block of 1024 threads per image: fewer elements than threads, one pass, a tail, three passes
def test_minmax_norm(ops, n):
    """bounded, r = 3 (the two restated intermediate roundings and the output's), B = 3 mixed-sign images, the second one constant when n == 1000;
    where torch's bf16 (x - min) / (max - min) is NaN on the CPU (0 / 0: n = 1 and the constant image) the kernel's is NaN."""
    x = randn(3, n, seed=53, scale=3.0)
    if n == 1000:
        x[1] = 1.5
    y = Guarded((3, n))
    d_x = dev(x)
    ops._lib.call("vp_minmax_norm", 3, n, p(d_x), p(y.view), ops._stream())
    torch.cuda.synchronize()
    got = y.cpu()
    torch_bf16 = (x - x.amin(1, keepdim=True)) / (x.amax(1, keepdim=True) - x.amin(1, keepdim=True))      # bf16 arithmetic, a rounding per operation
    assert torch.equal(torch.isnan(got), torch.isnan(torch_bf16))
    assert bool(torch.isnan(torch_bf16[1]).all()) == (n in (1, 1000))
    check(f"minmax n{n}", HR.minmax_check(got, x))
    assert y.untouched()


@pytest.mark.parametrize("B,H,W,Cc", [(2, 12, 16, 16), (1, 5, 13, 24), (2, 3, 7, 8), (1, 9, 10, 8)])
def test_dwconv7x7(ops, B, H, W, Cc):
    """bounded, r = 1: widths that are / are not multiples of the 4-pixel strip, maps smaller than the window.  (The second sweep of this kernel
    needs 65 536 * 256 items, a 1 GB input: not entered, see tests/PATHS.md.)"""
    x, w, b = randn(B, H, W, Cc, seed=54), randn(49, Cc, seed=55, scale=0.2), randn(Cc, seed=56)
    y = Guarded((B, H, W, Cc))
    d_x, d_w, d_b = dev(x), dev(w), dev(b)
    ops._lib.call("vp_dwconv7x7_nhwc", B, H, W, Cc, p(d_x), p(d_w), p(d_b), p(y.view), ops._stream())
    torch.cuda.synchronize()
    check(f"dwconv7x7 {B}x{H}x{W}x{Cc}", HR.bounded(y.cpu(), lambda dt: HR.dwconv7x7(x, w, b, dt), r=1))
    assert y.untouched()


# ================================================================================================ gemm.hip: transposes
TR = [1, 63, 64, 65, 130]       # 64 x 64 tiles: one element, one short of a tile, a whole (vector-path) tile, one over, two tiles and an edge


@pytest.mark.parametrize("form", ["dense", "ld_multiple_of_8", "ld_odd", "base_offset_1"])
def test_transpose_strides(ops, form):
    """exact, all 25 shapes: dense, ld_in > cols and ld_out > rows by a multiple of 8 (interior tiles stay on the vector path) and by an odd
    amount, and a base one element off 16-byte alignment (both force interior tiles onto the element path)"""
    for rows in TR:
        for cols in TR:
            x = randn(rows, cols, seed=60)
            ai, ao = {"dense": (0, 0), "ld_multiple_of_8": (8, 16), "ld_odd": (3, 5), "base_offset_1": (8, 8)}[form]
            off = 1 if form == "base_offset_1" else 0
            src = rows_view(rows, cols, cols + ai, fill=x, offset=off)
            out = rows_view(cols, rows, rows + ao, offset=off)
            ops._lib.call("vp_transpose_bf16", rows, cols, p(src.view), cols + ai, p(out.view), rows + ao, ops._stream())
            torch.cuda.synchronize()
            assert HR.exact(out.cpu(), x.t().contiguous()) and out.untouched(), (form, rows, cols)


@pytest.mark.parametrize("rows,cols", [(130, 75), (64, 128), (1, 9)])
def test_transpose_batched_strides(ops, rows, cols):
    """exact: batch strides larger than one matrix and ld > cols / rows, through the C ABI (ops.transpose_batched passes dense strides)"""
    Bn = 3
    x = randn(Bn, rows, cols, seed=61)
    ldi, ldo = cols + 8, rows + 16
    bsi, bso = (rows * ldi + 15) // 8 * 8 + 8, (cols * ldo + 15) // 8 * 8 + 24
    src = Guarded((Bn, rows, cols), (bsi, ldi, 1), fill=x)
    out = Guarded((Bn, cols, rows), (bso, ldo, 1))
    ops._lib.call("vp_transpose_batched_bf16", Bn, rows, cols, p(src.view), bsi, ldi, p(out.view), bso, ldo, ops._stream())
    torch.cuda.synchronize()
    assert HR.exact(out.cpu(), x.transpose(1, 2).contiguous()) and out.untouched()
