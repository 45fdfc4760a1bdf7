"""CPU proof behind tests/test_gemm_layouts_gpu.py.

1. gemm_ref in fp64 is torch's matmul plus the stated roundings, on strided operands; the integer generator keeps its promise.
2. The comparison the GPU test uses (gemm_cases.verify: sentinel outside the view, torch.equal in the integer pass, regimes.group_err with its
   computed bound in the gaussian pass) accepts a simulated honest kernel on every small case and rejects every mutant on the case aimed at it.
3. Whether the PARENT's GEMM tests see each mutant: OLD_CATCHES.  Their comparison (close() of tests/test_kernels_gpu.py, plus the two places
   where they look beside the output) runs here on their own layouts."""
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G
from gemm_cases import BF, F32, F64, I64
from test_kernels_gpu import close

SMALL = [c for c in G.CASES if c.M * c.N <= 512 * 512]


def passes(fn):
    try:
        fn()
        return True
    except AssertionError:
        return False


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("name", ["coltail-300x203x64-s7", "res-ld261-off1-bias-relu-512x256x128-s3", "f32-n50-512x50x128-s2", "lda129-512x256x128-s0"])
def test_gemm_ref_is_matmul_plus_the_stated_roundings(name):
    c = G.BY_NAME[name]
    inp = G.make_inputs(c, "gauss")
    a, w = inp.a.contiguous().double(), inp.w.contiguous().double()
    x = a @ w.t()
    if c.bias:
        x = x + inp.bias.double()
    if not c.f32:
        x = x.to(BF).double()
    if c.epi == G.EPI_RELU:
        x = F.relu(x)
        if not c.f32:
            x = x.to(BF).double()
    if c.res:
        x = x + inp.res.contiguous().double()
        if not c.f32:
            x = x.to(BF).double()
    assert torch.equal(G.ref_of(c, inp, F64), x)
    # without the last rounding: within half a bf16 ulp of it
    if not c.f32:
        raw = G.ref_of(c, inp, F64, last_round=False)
        assert torch.equal(raw.to(BF).double(), x)


@pytest.mark.parametrize("epi", [G.EPI_GELU, G.EPI_QUICK_GELU])
def test_gemm_ref_activations_are_torchs(epi):
    c = G.case("t", 0, 64, 48, 64, "NT128", epi=epi, bias=True)
    inp = G.make_inputs(c, "gauss")
    lin = (inp.a.double() @ inp.w.double().t() + inp.bias.double()).to(BF).double()
    want = F.gelu(lin) if epi == G.EPI_GELU else lin * torch.sigmoid(1.702 * lin)
    assert float((G.ref_of(c, inp, F64, last_round=False) - want).abs().max()) <= 1e-14


def test_integer_inputs_are_exact_in_every_float_type():
    """the int64 reference, the fp64 and the fp32 restatement agree bit for bit on the integer inputs (so a kernel's fp32 accumulation order
    cannot matter), and the sentinel is no integer below 2^24"""
    for name in ("coltail-300x263x64-s3", "res-ld261-off1-bias-relu-512x256x128-s7", "w4g-tail-300x256x128-s14"):
        c = G.BY_NAME[name]
        inp = G.make_inputs(c, "int")
        want = G.ref_of(c, inp, I64)
        assert int(want.abs().max()) <= 256 and int(want.abs().max()) >= 8
        for dt in (F64, F32):
            assert torch.equal(G.ref_of(c, inp, dt).to(I64), want)
        assert torch.equal(want.to(BF).to(I64), want)
    c = G.case("k192", 0, 64, 64, 192, "NT128", bias=True, res=True)
    G.make_inputs(c, "int")                                   # asserts its own bound
    assert G.sent_value(BF) > 1e30 and G.sent_value(F32) > 1e30


# ------------------------------------------------------------------------------------------------ 2. the new comparison
@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_honest_kernel_is_accepted(c):
    for kind in (("int", "gauss") if c.ints else ("gauss",)):
        inp = G.make_inputs(c, kind)
        _, mask = G.out_buffer(c)
        v = G.verify(c, inp, G.simulate(c, inp), mask)
        assert not G.rejected(v), (kind, v)


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_mutant_is_rejected_on_its_case(mut):
    c = G.BY_NAME[G.TARGET[mut]]
    for kind in ("int", "gauss"):
        inp = G.make_inputs(c, kind)
        _, mask = G.out_buffer(c)
        assert not G.rejected(G.verify(c, inp, G.simulate(c, inp), mask))
        v = G.verify(c, inp, G.simulate(c, inp, mut), mask)
        assert G.rejected(v), (mut, kind, v)


def test_store_mutants_are_seen_by_the_sentinel_or_the_values():
    """which of the three assertions sees which store mutant (the reason all three are made)"""
    see = {}
    for mut in ("column_tail_unwritten", "c_rows_written_with_ld_rounded_to_8", "row_tail_written_past_m"):
        c = G.BY_NAME[G.TARGET[mut]]
        inp = G.make_inputs(c, "int")
        _, mask = G.out_buffer(c)
        v = G.verify(c, inp, G.simulate(c, inp, mut), mask)
        see[mut] = (v.outside, v.exact)
    assert see["column_tail_unwritten"] == (True, False)                      # the sentinel is still in the view
    assert see["c_rows_written_with_ld_rounded_to_8"] == (False, False)
    assert see["row_tail_written_past_m"] == (False, True)                    # only the rows below the view change


# ------------------------------------------------------------------------------------------------ 3. the parent's tests
# mutant -> does the parent suite notice it?  Its GEMM calls, by layout: contiguous operands at their allocation's base (test_gemm_plain,
# _epilogues, _256_tile_kernel, _4wave_*), among them ONE fast-kernel shape with N % 8 != 0: (700, 300, 192) under selectors 3, 2 and 7, which
# also has ldc = 300; (77, 50, 40) on the generic kernel; A a column slice at + K elements, C a column slice of a zeroed buffer at + N, both
# 16-byte aligned (test_gemm_strided_views); A at + 8 elements with lda = K + 16 and the bias at + 3 elements (test_gemm_random_shape_sweep); C
# the first M rows of a taller buffer under selector 14 (test_gemm_4wave_general_variant).  Where the answer is True the new cases add the
# kernels and positions the old shape does not reach (tests/GEMM_PATHS.md).
OLD_CATCHES = {
    "column_tail_unwritten": True,                   # (700, 300, 192): the 128-tile, 256-tile and 8-phase kernels, by close(); not selector 13
    "column_tail_shifted_by_one": True,              # the same shape
    "residual_read_with_ld_n": False,                # ldr == N in every call
    "residual_base_aligned_down": False,             # every residual starts its allocation
    "bias_base_aligned_down": True,                  # the sweep's bias at + 3 elements
    "c_rows_written_with_ld_rounded_to_8": True,     # (700, 300, 192) again: ldc = 300
    "row_tail_written_past_m": True,                 # test_gemm_4wave_general_variant looks at the rows below M
    "a_base_aligned_down": False,                    # the sweep's A offset is 8 elements: aligned down it is itself
}
OLD_LAYOUTS = [
    G.case("old-plain-300x200x128", 0, 300, 200, 128, "NT128"),
    G.case("old-plain-77x50x40", 1, 77, 50, 40, "GENERIC"),
    G.case("old-epilogues-200x328x192", 0, 200, 328, 192, "NT128", epi=G.EPI_RELU, bias=True, res=True),
    G.case("old-256tile-700x300x192-s7", 7, 700, 300, 192, "P8", bias=True, res=True),
    G.case("old-strided-views-192x64x128", 0, 192, 64, 128, "NT128", a=(384, 128), c=(192, 64)),
    G.case("old-sweep-300x264x192", 0, 300, 264, 192, "NT128", a=(208, 8), bias=True, bias_off=3, res=True),
    G.case("old-w4g-300x256x128-s14", 14, 300, 256, 128, "W4G", bias=True, res=True, tall=300),
]
OLD_LOOKS_BESIDE = {"old-strided-views-192x64x128", "old-w4g-300x256x128-s14"}


def old_check(c, inp, buf, mask):
    """the parent's comparison: close() against the fp32 matmul with the roundings its tests restate; beside the output it looks only in
    test_gemm_strided_views (the other column slices stay zero) and test_gemm_4wave_general_variant (the rows below M keep their fill)"""
    close(G.out_view(c, buf), G.ref_of(c, inp, F32))
    if c.name in OLD_LOOKS_BESIDE:
        region = torch.zeros_like(mask)
        torch.as_strided(region, (c.M + c.tall, c.lay.c[0]), (c.lay.c[0], 1), G.PAD).fill_(True)      # the buffer the old test allocates
        region &= ~mask
        it, bits = G.SENT[F32 if c.f32 else BF]
        assert bool((buf.view(it)[region] == bits).all())


def test_old_catches():
    seen = {m: False for m in G.MUTANTS}
    for c in OLD_LAYOUTS:
        inp = G.make_inputs(c, "gauss")
        _, mask = G.out_buffer(c)
        assert passes(lambda: old_check(c, inp, G.simulate(c, inp), mask)), c.name
        for m in G.MUTANTS:
            seen[m] |= not passes(lambda: old_check(c, inp, G.simulate(c, inp, m), mask))
    assert seen == OLD_CATCHES
