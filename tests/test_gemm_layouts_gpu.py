"""vp_gemm_bf16 and its sibling entry points (csrc/gemm.hip) on the operand layouts, tails and routing edges of tests/gemm_cases.py
(tests/GEMM_PATHS.md maps each path to its case; tests/test_gemm_route_host.py proves on the CPU which kernel each case reaches and
tests/test_gemm_layouts_host.py that the comparison made here rejects every mutant).

Every operand and every output is a view inside an allocation filled with a sentinel bit pattern.  Per case:
  outside   every element of the output allocation outside the view keeps the sentinel; the input allocations are bit-unchanged
  exact     integer inputs (epilogues NONE and ReLU): torch.equal with the int64 reference, bf16 and fp32 output
  bounded   N(0, 1) inputs: regimes.group_err against fp64 over interior rows / the last row tile / the last column tile, bound
            regimes.bound(out_spec(r = 1 | 2 | 3)) (out_spec(n = K) for fp32), y = the fp32 reference's own error, through parity.check
  twin      where an aligned contiguous call reaches the same kernel, its result is bit-equal

The large-leading-dimension cases come last, one allocation at a time (peak device memory of that group: 4.3 GB + 2.1 GB of compare mask)."""
import ctypes as C

import pytest
import torch

import gemm_cases as G
import parity
from gemm_cases import BF, F32, F64, I64, PAD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops as o
    return o


def bits_equal(x, y):
    it = {2: torch.int16, 4: torch.int32}[x.element_size()]
    return x.shape == y.shape and bool(torch.equal(x.contiguous().view(it), y.contiguous().view(it)))


def on_device(view, dbuf):
    return torch.as_strided(dbuf, view.shape, view.stride(), view.storage_offset())


class DevView:
    """rows x cols at leading dimension ld, `off` elements into a sentinel-filled device allocation (PAD elements before and after, `tall` rows
    of sentinel below).  outside_untouched() overwrites the view with the sentinel and compares the whole allocation in slabs: no second copy."""

    def __init__(self, rows, cols, ld=None, off=0, dtype=BF, tall=0, fill=None):
        ld = cols if ld is None else ld
        self.it, self.bits = G.SENT[dtype]
        n = PAD + off + (rows + tall - 1) * ld + cols + PAD
        self.buf = torch.full((n,), self.bits, dtype=self.it, device="cuda").view(dtype)
        self.view = torch.as_strided(self.buf, (rows, cols), (ld, 1), PAD + off)
        self.ld = ld
        if fill is not None:
            self.view.copy_(fill)

    def outside_untouched(self):
        self.view.view(self.it).fill_(self.bits)
        flat = self.buf.view(self.it)
        step = 1 << 28
        return all(bool((flat[i:i + step] == self.bits).all()) for i in range(0, flat.numel(), step))

    def all_sentinel(self):
        flat = self.buf.view(self.it)
        return bool((flat == self.bits).all())


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ================================================================================================ vp_gemm_bf16: the case table
def run_case(ops, c, kind):
    inp = G.make_inputs(c, kind)
    dbufs = {k: v.cuda() for k, v in inp.bufs.items()}
    dv = {k: (None if getattr(inp, k) is None else on_device(getattr(inp, k), dbufs[k])) for k in ("a", "w", "bias", "res")}
    cbuf, mask = G.out_buffer(c)
    dc = cbuf.cuda()
    ops.gemm(dv["a"], dv["w"], bias=dv["bias"], residual=dv["res"], epi=c.epi, out=G.out_view(c, dc), force_generic=c.sel)
    torch.cuda.synchronize()
    for k, d in dbufs.items():
        assert bits_equal(d.cpu(), inp.bufs[k]), f"{c.name}: the allocation of {k} changed"
    return inp, dv, dc.cpu(), mask


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_gemm_layout(ops, c):
    if c.ints:
        inp, _, after, mask = run_case(ops, c, "int")
        v = G.verify(c, inp, after, mask)
        assert v.outside, f"{c.name}: a sentinel element outside the output view changed (integer pass)"
        assert v.exact, f"{c.name}: not equal to the int64 reference"
    inp, dv, after, mask = run_case(ops, c, "gauss")
    v = G.verify(c, inp, after, mask)
    assert v.outside, f"{c.name}: a sentinel element outside the output view changed"
    fails = []
    for g, (e, b) in v.bounded.items():
        try:
            parity.check(f"gemm_layout {c.kernel} {c.name} [{g}]", e if e == e and e != float("inf") else 1e30, b)
        except AssertionError as ex:
            fails.append(str(ex))
    assert not fails, "\n".join(fails)
    if c.twin is not None:
        fresh = lambda t: None if t is None else t.clone(memory_format=torch.contiguous_format)      # its own allocation: aligned, dense
        twin = ops.gemm(fresh(dv["a"]), fresh(dv["w"]), bias=fresh(dv["bias"]), residual=fresh(dv["res"]), epi=c.epi, out_f32=c.f32, force_generic=c.twin)
        assert bits_equal(twin.cpu(), G.out_view(c, after)), f"{c.name}: differs from the aligned contiguous call under selector {c.twin}"


# ================================================================================================ sibling entry points
def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (4096, 3072, 256)])          # the 8-phase kernel; the one-wave-per-SIMD kernel (192 tiles)
def test_swiglu_entry_point_strided_outputs(ops, M, N, K):
    """mode 1 and 2 with ldc, ldc2, ldaux above the row length (multiples of 8) and bases 8 elements in: bit-equal to the contiguous call,
    nothing outside the views written"""
    from visper_lm_amd import _lib
    a, w = rnd(M, K, seed=1).cuda(), rnd(N, K, seed=2, scale=0.1).cuda()
    gu, act = ops.gemm_swiglu_fwd(a, w)
    dgu_buf, dact = DevView(M, N, N + 16, 8), DevView(M, N // 2, N // 2 + 24, 8)
    _lib.call("vp_gemm_bf16_swiglu", 1, M, N, K, p(a), K, p(w), K, p(dgu_buf.view), dgu_buf.ld, p(dact.view), dact.ld, None, 0, None, stream())
    torch.cuda.synchronize()
    assert bits_equal(dgu_buf.view, gu) and bits_equal(dact.view, act)
    assert dgu_buf.outside_untouched() and dact.outside_untouched()
    # mode 2: d_gate_up[M, 2N] from dy[M, K] . w^T[N, K] and the saved gate_up[M, 2N]
    saved = rnd(M, 2 * N, seed=3).cuda()
    want = ops.gemm_swiglu_bwd(a, w, saved)
    aux, out = DevView(M, 2 * N, 2 * N + 8, 8, fill=saved), DevView(M, 2 * N, 2 * N + 32, 8)
    _lib.call("vp_gemm_bf16_swiglu", 2, M, N, K, p(a), K, p(w), K, p(out.view), out.ld, None, 0, p(aux.view), aux.ld, None, stream())
    torch.cuda.synchronize()
    assert bits_equal(out.view, want) and bits_equal(aux.view, saved)
    assert out.outside_untouched() and aux.outside_untouched()


def test_sumsq_entry_point_strided_output_and_residual(ops):
    from visper_lm_amd import _lib
    M, N, K = 256, 256, 128
    a, w, r = rnd(M, K, seed=4).cuda(), rnd(N, K, seed=5, scale=0.1).cuda(), rnd(M, N, seed=6).cuda()
    want, part = ops.gemm_sumsq(a, w, r)
    out, res, pt = DevView(M, N, N + 8, 8), DevView(M, N, N + 40, 16, fill=r), DevView(M, N // 16, dtype=F32)
    _lib.call("vp_gemm_bf16_sumsq", M, N, K, p(a), K, p(w), K, p(out.view), out.ld, p(res.view), res.ld, p(pt.view), stream())
    torch.cuda.synchronize()
    assert bits_equal(out.view, want) and bits_equal(pt.view, part) and bits_equal(res.view, r)
    assert out.outside_untouched() and pt.outside_untouched() and res.outside_untouched()


def test_rope_entry_point_strided_output_row_tail(ops):
    """(300, 256, 128), rope_cols = 128, ldc > N, the output above 256 rows of sentinel: the last row tile's rows 300 .. 383 are dropped"""
    from visper_lm_amd import _lib
    M, N, K, S = 300, 256, 128, 64
    a, w = rnd(M, K, seed=7).cuda(), rnd(N, K, seed=8, scale=0.1).cuda()
    cos_t, sin_t = ops.rope_tables(S, 128, 10000.0, "cuda")
    want = ops.gemm_rope(a, w, S, 128, cos_t, sin_t)
    out = DevView(M, N, N + 8, 8, tall=256)
    _lib.call("vp_gemm_bf16_rope", M, N, K, p(a), K, p(w), K, p(out.view), out.ld, None, 128, p(cos_t), p(sin_t), None, S, stream())
    torch.cuda.synchronize()
    assert bits_equal(out.view, want)
    assert out.outside_untouched()


@pytest.mark.parametrize("f32", [True, False])
def test_tn_entry_point_strided_output(ops, f32):
    from visper_lm_amd import _lib
    M, N, K = 256, 256, 64
    a, b = rnd(K, M, seed=9).cuda(), rnd(K, N, seed=10).cuda()
    want = ops.gemm_tn(a, b, out_f32=f32)
    out = DevView(M, N, N + 8, 8, dtype=F32 if f32 else BF)
    _lib.call("vp_gemm_tn_bf16", M, N, K, p(a), M, p(b), N, p(out.view), out.ld, int(f32), 0, None, stream())
    torch.cuda.synchronize()
    assert bits_equal(out.view, want)
    assert out.outside_untouched()


REFUSALS = ["gemm-ldc-below-n", "swiglu-ldc-odd", "swiglu-m255", "sumsq-c-misaligned", "sumsq-m255", "rope-cols64", "rope-m255", "rope-ldc-odd", "tn-ldc-odd",
            "tn-c-misaligned"]


@pytest.mark.parametrize("what", REFUSALS)
def test_entry_points_refuse_and_write_nothing(ops, what):
    """a layout or shape the entry point does not take: RuntimeError, and the sentinel-filled output keeps every bit"""
    from visper_lm_amd import _lib
    M, N, K, S = 256, 256, 128, 64
    if what.endswith("m255"):
        M = 255
    a, w = rnd(M, K, seed=11).cuda(), rnd(N, K, seed=12, scale=0.1).cuda()
    odd, mis = "ldc-odd" in what, "misaligned" in what
    out = DevView(M, 2 * N, 2 * N + (9 if odd else 8), 1 if mis else 0, dtype=F32 if what.startswith("tn") else BF)
    o2 = DevView(M, N)
    cos_t, sin_t = ops.rope_tables(S, 128, 10000.0, "cuda")
    st = stream()
    with pytest.raises(RuntimeError):
        if what == "gemm-ldc-below-n":
            _lib.call("vp_gemm_bf16", M, N, K, p(a), K, p(w), K, p(out.view), N - 8, None, None, 0, 0, 0, 0, None, st)
        elif what.startswith("swiglu"):
            _lib.call("vp_gemm_bf16_swiglu", 1, M, N, K, p(a), K, p(w), K, p(out.view), out.ld, p(o2.view), o2.ld, None, 0, None, st)
        elif what.startswith("sumsq"):
            r = rnd(M, N, seed=13).cuda()
            pt = torch.zeros(M, N // 16, device="cuda")
            _lib.call("vp_gemm_bf16_sumsq", M, N, K, p(a), K, p(w), K, p(out.view), out.ld, p(r), N, p(pt), st)
        elif what.startswith("rope"):
            _lib.call("vp_gemm_bf16_rope", M, N, K, p(a), K, p(w), K, p(out.view), out.ld, None, 64 if what == "rope-cols64" else 128, p(cos_t), p(sin_t), None, S, st)
        else:
            at, bt = rnd(K, 256, seed=14).cuda(), rnd(K, N, seed=15).cuda()
            _lib.call("vp_gemm_tn_bf16", 256, N, K, p(at), 256, p(bt), N, p(out.view), out.ld, 1, 0, None, st)
    torch.cuda.synchronize()
    assert out.all_sentinel() and o2.all_sentinel()


# ================================================================================================ large leading dimensions (last: 2 - 4 GB each)
@pytest.mark.parametrize("c", G.LARGE_LD, ids=lambda c: c.name)
def test_gemm_large_leading_dimension(ops, c):
    """ldc / ldr at (1 << 22) - 8, the last value the one-wave-per-SIMD kernels and the 8-phase kernel's non-temporal stores admit, and at
    1 << 22, where the route must send the call elsewhere (tests/GEMM_PATHS.md holds the 32-bit arithmetic of each).  Integer pass; one
    allocation at a time; the outside of the view is checked in place."""
    small = G.case(c.name, c.sel, c.M, c.N, c.K, c.kernel, bias=c.bias, res=c.res)          # the same values, compact: for the reference
    inp = G.make_inputs(small, "int")
    want = G.ref_of(small, inp, I64)
    a, w = inp.a.contiguous().cuda(), inp.w.contiguous().cuda()
    bias = inp.bias.contiguous().cuda() if c.bias else None
    out = DevView(c.M, c.N, c.lay.c[0])
    res = DevView(c.M, c.N, c.lay.r[0], fill=inp.res.cuda()) if c.res else None
    ops.gemm(a, w, bias=bias, residual=None if res is None else res.view, out=out.view, force_generic=c.sel)
    torch.cuda.synchronize()
    got = out.view.cpu()
    assert torch.equal(got.to(F64), want.to(F64)), f"{c.name}: not equal to the int64 reference"
    assert out.outside_untouched(), f"{c.name}: a sentinel element outside the output view changed"
    if res is not None:
        assert bits_equal(res.view.cpu(), inp.res.contiguous()) and res.outside_untouched()
    del out, res
    torch.cuda.empty_cache()
