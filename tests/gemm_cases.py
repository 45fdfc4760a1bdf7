"""Operand layouts, tails and routing edges of vp_gemm_bf16 (csrc/gemm.hip behind csrc/gemm_route.h), shared by tests/test_gemm_route_host.py,
tests/test_gemm_layouts_host.py (both CPU) and tests/test_gemm_layouts_gpu.py.  Importable without a device.  tests/GEMM_PATHS.md maps every
path to its case.

A CASE names a selector, a shape, an epilogue and, for each of A, B, C, bias and residual, a LAYOUT: a leading dimension and a base offset in
elements from a 256-byte-aligned allocation.  It also states the GemmKernel it must reach (tests/test_gemm_route_host.py computes that from the
header; a route change that moves a case off its kernel fails there, without a GPU).

`gemm_ref` restates the operation in fp64 / fp32 / int64 with store4's rounding points.  Two input generators: small integers (every value
of the reference is an integer of magnitude <= 256, exact in bf16 and in fp32 whatever the summation order: torch.equal) and N(0, 1) as rnd()
of tests/test_kernels_gpu.py (bounded with tests/regimes.py).  MUTANTS are value errors of the kind the branches entered here could make;
`simulate` plays a kernel (fp32 math) with one of them, `verify` is the comparison the GPU test uses."""
from types import SimpleNamespace as NS

import torch

import regimes as R
from regimes import BF

F32, F64, I64 = torch.float32, torch.float64, torch.int64
EPI_NONE, EPI_GELU, EPI_QUICK_GELU, EPI_RELU = 0, 1, 2, 3
KERNELS = ["NONE", "W4", "W4G", "W4F", "P8", "PH4", "NT256", "NT128", "GENERIC", "TN"]      # enum GemmKernel of gemm_route.h, from GK_NONE = -1
TILE = {"W4": 256, "W4G": 256, "W4F": 256, "P8": 256, "PH4": 256, "NT256": 256, "NT128": 128, "GENERIC": 64}
PAD = 128                       # elements before and after every view: 256 bytes of bf16, 512 of fp32 (the view's base keeps its stated alignment)
SENT = {BF: (torch.int16, 0x7A5A), F32: (torch.int32, 0x7A5A5A5A)}      # finite (2.8e35 / 2.8e35): no result below can equal it


def sent_value(dtype):
    it, bits = SENT[dtype]
    return float(torch.tensor([bits], dtype=it).view(dtype)[0])


# ------------------------------------------------------------------------------------------------ the case table
def case(name, sel, M, N, K, kernel, epi=EPI_NONE, bias=False, res=False, f32=False, a=None, b=None, c=None, bias_off=0, r=None, tall=0,
         grid=None, sched=False, c_nt=0, twin=None, ints=None):
    """a / b / c / r: (leading dimension, base offset in elements), default (row length, 0).  tall: rows of sentinel below C (and below the
    residual).  twin: the selector under which the aligned contiguous call reaches the same kernel (None: no twin, or the case is its own).
    grid / sched / c_nt: what gemm_route must return beside the kernel (grid None: not pinned)."""
    lay = NS(a=a or (K, 0), b=b or (K, 0), c=c or (N, 0), bias=bias_off, r=(r or (N, 0)) if res else None)
    if ints is None:
        ints = epi in (EPI_NONE, EPI_RELU)
    return NS(name=name, sel=sel, M=M, N=N, K=K, kernel=kernel, epi=epi, bias=bias, res=res, f32=f32, lay=lay, tall=tall, grid=grid, sched=sched,
              c_nt=c_nt, twin=twin, ints=ints)


def _cases():
    cs = []
    by_sel = {0: "NT128", 2: "NT128", 3: "NT256", 7: "P8", 13: "PH4", 8: "NT128", 14: "NT128"}      # a small aligned problem under each selector
    # column tail N % 8 != 0 on the fast kernels (epilogue_swz's scalar tail loops); 203 / 263: the tail in the second 128- / 256-column tile.
    # The 8-phase kernel gets c_nt = 1 here: its tail tiles must not take the non-temporal descriptor stores.
    for N in (50, 203, 263):
        for sel in (0, 2, 3, 7, 13, 8, 14):
            cs.append(case(f"coltail-300x{N}x64-s{sel}", sel, 300, N, 64, by_sel[sel], bias=True, res=True, c_nt=1 if sel == 7 else 0,
                           grid=((300 + 255) // 256) * ((N + 255) // 256) if sel in (7, 13) else None))
    # ldc % 8 != 0 on interior tiles: the not-`fast` branch of epilogue_swz with whole tiles
    for sel in (0, 3, 7, 13, 8, 14):
        cs.append(case(f"ldc259-512x256x128-s{sel}", sel, 512, 256, 128, by_sel[sel], c=(259, 0), c_nt=1 if sel == 7 else 0, twin=2 if sel in (0, 8, 14) else sel))
    for sel in (3, 7, 13, 8, 14):
        cs.append(case(f"cbase1-512x256x128-s{sel}", sel, 512, 256, 128, by_sel[sel], c=(264, 1), c_nt=1 if sel == 7 else 0, twin=2 if sel in (8, 14) else sel))
    # residual: odd ldr and a base one element off; plain, and behind bias + ReLU
    for sel in (2, 3, 7, 13):
        cs.append(case(f"res-ld261-off1-512x256x128-s{sel}", sel, 512, 256, 128, by_sel[sel], res=True, r=(261, 1), c_nt=1 if sel == 7 else 0, twin=sel))
        cs.append(case(f"res-ld261-off1-bias-relu-512x256x128-s{sel}", sel, 512, 256, 128, by_sel[sel], epi=EPI_RELU, bias=True, res=True, r=(261, 1),
                       c_nt=1 if sel == 7 else 0, twin=sel))
    # bias one element off (2-byte aligned): the general variant's 16-byte bias loads must be refused, the others take the element path
    cs.append(case("bias-off1-2048x2048x128-s0", 0, 2048, 2048, 128, "NT128", bias=True, bias_off=1, twin=2))
    cs.append(case("bias-off1-2048x2048x128-s14", 14, 2048, 2048, 128, "NT128", bias=True, bias_off=1, twin=2))
    cs.append(case("bias-off1-512x256x128-s13", 13, 512, 256, 128, "PH4", bias=True, bias_off=1, twin=13))
    # fp32 output: store4's element path (ldc % 4 != 0, C base + 1 float) and its nv < 4 tail (N = 50)
    for sel, k in ((2, "NT128"), (3, "NT256"), (7, "P8")):
        cs.append(case(f"f32-ldc258-512x256x128-s{sel}", sel, 512, 256, 128, k, f32=True, c=(258, 0), twin=sel))
        cs.append(case(f"f32-cbase1-512x256x128-s{sel}", sel, 512, 256, 128, k, f32=True, c=(260, 1), bias=True, twin=sel))
        cs.append(case(f"f32-n50-512x50x128-s{sel}", sel, 512, 50, 128, k, f32=True, epi=EPI_RELU, bias=True, res=True))
    cs.append(case("f32-ldc4098-3072x4096x128-s0", 0, 3072, 4096, 128, "P8", f32=True, c=(4098, 0), grid=192, twin=7))
    # a misaligned A or B must fall to the generic kernel under every selector
    for sel in (0, 2, 3, 7, 8, 14):
        cs.append(case(f"a-off1-512x256x128-s{sel}", sel, 512, 256, 128, "GENERIC", a=(128, 1), twin=1))
        cs.append(case(f"b-off1-512x256x128-s{sel}", sel, 512, 256, 128, "GENERIC", b=(128, 1), bias=True, twin=1))
        cs.append(case(f"lda129-512x256x128-s{sel}", sel, 512, 256, 128, "GENERIC", a=(129, 0), res=True, twin=1))
    # the general one-wave-per-SIMD variant drops rows >= M through its descriptor's num_records: C and the residual are the first M rows of a
    # taller buffer
    for M in (257, 300, 400):
        cs.append(case(f"w4g-tail-{M}x256x128-s14", 14, M, 256, 128, "W4G", bias=True, res=True, tall=256, grid=2, twin=14))
    cs.append(case("w4g-tail-255x256x128-s14", 14, 255, 256, 128, "NT128", bias=True, res=True, tall=256, twin=2))
    # where the automatic route changes kernel
    cs.append(case("auto-3072x4096x128", 0, 3072, 4096, 128, "W4", grid=192, c_nt=1))
    cs.append(case("auto-3072x4096x128-f32", 0, 3072, 4096, 128, "W4", f32=True, grid=192))
    cs.append(case("auto-3072x3840x128", 0, 3072, 3840, 128, "W4G", grid=180))
    cs.append(case("auto-3072x3840x128-f32", 0, 3072, 3840, 128, "NT128", f32=True))
    cs.append(case("auto-2048x2048x128-bias", 0, 2048, 2048, 128, "W4G", bias=True, grid=64))
    cs.append(case("auto-2048x1792x128-bias", 0, 2048, 1792, 128, "NT128", bias=True))
    cs.append(case("auto-2048x2048x128-bias-gelu", 0, 2048, 2048, 128, "NT128", bias=True, epi=EPI_GELU))
    cs.append(case("auto-2048x2048x128-res", 0, 2048, 2048, 128, "W4G", res=True, grid=64))
    cs.append(case("auto-2048x2048x128-res-relu", 0, 2048, 2048, 128, "NT128", res=True, epi=EPI_RELU))
    cs.append(case("auto-2048x2048x128-res-off1", 0, 2048, 2048, 128, "NT128", res=True, r=(2056, 1), twin=2))
    cs.append(case("auto-1800x2048x128-bias", 0, 1800, 2048, 128, "W4G", bias=True, grid=64))
    cs.append(case("auto-3072x4096x192", 0, 3072, 4096, 192, "PH4", grid=192, c_nt=1))
    # the 8-phase grid rule: an odd K-tile count runs one block a tile, an even one the persistent grid with the caller's claim counters
    cs.append(case("p8grid-4352x4096x192-s7", 7, 4352, 4096, 192, "P8", grid=272, c_nt=1))
    cs.append(case("p8grid-4352x4096x128-s7", 7, 4352, 4096, 128, "P8", grid=256, sched=True, c_nt=1))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Large leading dimensions (tests/GEMM_PATHS.md derives every 32-bit quantity): N = 256, K = 128, integer pass, C (and the residual) views of
# a sentinel-filled buffer.  LD_EDGE is the last admitted leading dimension of the one-wave-per-SIMD kernels, LD_EDGE + 8 the first refused.
LD_EDGE = (1 << 22) - 8
LARGE_LD = [
    case("bigld-c-256-s8", 8, 256, 256, 128, "W4", c=(LD_EDGE, 0), grid=1, c_nt=1),
    case("bigld-c-256-s14", 14, 256, 256, 128, "W4G", bias=True, c=(LD_EDGE, 0), grid=1),
    case("bigld-r-256-s8", 8, 256, 256, 128, "W4", res=True, r=(LD_EDGE, 0), grid=1, c_nt=1),
    case("bigld-r-256-s14", 14, 256, 256, 128, "W4G", bias=True, res=True, r=(LD_EDGE, 0), grid=1),
    case("bigld-c-256-s7", 7, 256, 256, 128, "P8", c=(LD_EDGE, 0), grid=1, c_nt=1),              # M ldc 2 = 2 147 479 552 < 0x7fffffff
    case("bigld-c-256-s8-refused", 8, 256, 256, 128, "NT128", c=(1 << 22, 0)),
    case("bigld-c-512-s7", 7, 512, 256, 128, "P8", c=(1 << 22, 0), grid=2, c_nt=0),              # the output spans 2^31 and 2^32 bytes
]


def alignment(c):
    """the (a_al, b_al, c_al, bias_al, res_al) gemm_route sees: pointer & 15 for a 256-byte-aligned allocation"""
    cw = 4 if c.f32 else 2
    return ((c.lay.a[1] * 2) & 15, (c.lay.b[1] * 2) & 15, (c.lay.c[1] * cw) & 15, (c.lay.bias * 2) & 15 if c.bias else 0,
            (c.lay.r[1] * 2) & 15 if c.res else 0)


def twin_of(c):
    """the aligned contiguous call on the same kernel"""
    return case(c.name + "-twin", c.twin, c.M, c.N, c.K, c.kernel, epi=c.epi, bias=c.bias, res=c.res, f32=c.f32)


# ------------------------------------------------------------------------------------------------ the reference and its mutants
MUTANTS = ["column_tail_unwritten", "column_tail_shifted_by_one", "residual_read_with_ld_n", "residual_base_aligned_down",
           "bias_base_aligned_down", "c_rows_written_with_ld_rounded_to_8", "row_tail_written_past_m", "a_base_aligned_down"]
# the case each mutant is aimed at (the GPU test's comparison must reject it there: tests/test_gemm_layouts_host.py)
TARGET = {
    "column_tail_unwritten": "coltail-300x50x64-s0",
    "column_tail_shifted_by_one": "coltail-300x203x64-s7",
    "residual_read_with_ld_n": "res-ld261-off1-512x256x128-s2",
    "residual_base_aligned_down": "res-ld261-off1-bias-relu-512x256x128-s3",
    "bias_base_aligned_down": "bias-off1-512x256x128-s13",
    "c_rows_written_with_ld_rounded_to_8": "ldc259-512x256x128-s0",
    "row_tail_written_past_m": "w4g-tail-300x256x128-s14",
    "a_base_aligned_down": "a-off1-512x256x128-s0",
}


def _restride(t, size, stride, offset):
    """the same storage read with another (stride, base): what a kernel that mis-forms an address reads"""
    base = t._base if t._base is not None else t
    return torch.as_strided(base, size, stride, offset)


def _rnd(t, dt):
    """a restated bf16 rounding point (the integer pass: every value is an integer of magnitude <= 256, which bf16 holds)"""
    return t if dt == I64 else R.bfr(t)


def _act(x, epi, dt):
    if epi == EPI_NONE:
        return x
    if epi == EPI_RELU:
        return x.clamp_min(0)
    assert dt != I64, "the integer pass serves EPI_NONE and EPI_RELU"
    if epi == EPI_GELU:
        return x * 0.5 * (1 + torch.erf(x * 0.70710678118654752))
    return x * torch.sigmoid(1.702 * x)


def gemm_ref(a, w, bias, res, epi, out_f32, dt, mut=None, last_round=True):
    """epi(a @ w^T + bias) + res with store4's rounding points (csrc/gemm.hip): linear (+ bias) -> bf16 -> activation -> bf16 -> + residual -> bf16;
    no rounding at all for fp32 output.  dt: torch.float64 / float32, or int64 for the integer inputs (the products are summed in fp64, where
    integers below 2^53 are exact, and converted).  last_round=False leaves the final bf16 rounding out (tests/regimes.py's convention for a
    bounded comparison: the bound (2 r - 1) 2^-8 counts it as half an ulp).
    mut: an operand read through a wrong address (the mutants that act on the written output are simulate()'s)."""
    M, K = a.shape
    N = w.shape[0]
    if mut == "a_base_aligned_down":
        a = _restride(a, (M, K), a.stride(), a.storage_offset() & ~7)
    if mut == "bias_base_aligned_down" and bias is not None:
        bias = _restride(bias, (N,), (1,), bias.storage_offset() & ~7)
    if res is not None:
        if mut == "residual_read_with_ld_n":
            res = _restride(res, (M, N), (N, 1), res.storage_offset())
        if mut == "residual_base_aligned_down":
            res = _restride(res, (M, N), res.stride(), res.storage_offset() & ~7)
    cdt = F64 if dt == I64 else dt
    x = a.to(cdt) @ w.to(cdt).t()
    if dt == I64:
        x = x.to(I64)
    if bias is not None:
        x = x + bias.to(dt)
    if out_f32:
        x = _act(x, epi, dt)
        return x + res.to(dt) if res is not None else x
    nround = 1 + (epi != EPI_NONE) + (res is not None)
    rounds = [True] * (nround - 1) + [last_round]
    x = _rnd(x, dt) if rounds.pop(0) else x
    if epi != EPI_NONE:
        x = _act(x, epi, dt)
        x = _rnd(x, dt) if rounds.pop(0) else x
    if res is not None:
        x = x + res.to(dt)
        x = _rnd(x, dt) if rounds.pop(0) else x
    return x


def roundings(c):
    """r of regimes.out_spec for a bf16 output: 1 (plain, bias), 2 (activation or residual), 3 (activation, then residual)"""
    return 1 + (c.epi != EPI_NONE) + (1 if c.res else 0)


# ------------------------------------------------------------------------------------------------ inputs
def _view(buf, rows, cols, ld, off):
    return torch.as_strided(buf, (rows, cols), (ld, 1), PAD + off)


def _alloc(n, dtype):
    it, bits = SENT[dtype]
    return torch.full((n,), bits, dtype=it).view(dtype)


def _extent(rows, cols, ld, off, tall=0):
    return PAD + off + (rows + tall - 1) * ld + cols + PAD


def out_buffer(c):
    """the sentinel-filled output allocation and the bool mask of the view inside it"""
    dt = F32 if c.f32 else BF
    ld, off = c.lay.c
    n = _extent(c.M, c.N, ld, off, c.tall)
    buf = _alloc(n, dt)
    mask = torch.zeros(n, dtype=torch.bool)
    _view(mask, c.M, c.N, ld, off).fill_(True)
    return buf, mask


def out_view(c, buf):
    return _view(buf, c.M, c.N, *c.lay.c)


def make_inputs(c, kind, seed=0):
    """kind "int": operands from {-1, 0, 1} (zeros thinned in so that K > 128 adds no magnitude), bias in [-4, 4], residual in [-8, 8];
    kind "gauss": rnd() of tests/test_kernels_gpu.py (weights scaled by 0.1).  Every operand is a view at its case's (ld, offset) inside a
    sentinel-filled allocation.  -> NS(a, w, bias, res: the views; bufs: {name: allocation})"""
    g = R.gen(9000 + seed + 7919 * (c.M + c.N + c.K))
    M, N, K = c.M, c.N, c.K

    def fill(shape, scale, lo_hi):
        if kind == "int":
            t = torch.randint(lo_hi[0], lo_hi[1] + 1, shape, generator=g).float()
            if lo_hi == (-1, 1) and K > 128:
                t = t * (torch.rand(shape, generator=g) < 128.0 / K)
            return t.to(BF)
        return (torch.randn(shape, generator=g) * scale).to(BF)

    bufs, views = {}, {}
    for name, rows, cols, (ld, off), scale, rng in (("a", M, K, c.lay.a, 1.0, (-1, 1)), ("w", N, K, c.lay.b, 0.1, (-1, 1))):
        bufs[name] = _alloc(_extent(rows, cols, ld, off), BF)
        views[name] = _view(bufs[name], rows, cols, ld, off)
        views[name].copy_(fill((rows, cols), scale, rng))
    views["bias"] = views["res"] = None
    if c.bias:
        bufs["bias"] = _alloc(PAD + c.lay.bias + N + PAD, BF)
        views["bias"] = torch.as_strided(bufs["bias"], (N,), (1,), PAD + c.lay.bias)
        views["bias"].copy_(fill((N,), 1.0, (-4, 4)))
    if c.res:
        ld, off = c.lay.r
        bufs["res"] = _alloc(_extent(M, N, ld, off, c.tall), BF)
        views["res"] = _view(bufs["res"], M, N, ld, off)
        views["res"].copy_(fill((M, N), 1.0, (-8, 8)))
    inp = NS(a=views["a"], w=views["w"], bias=views["bias"], res=views["res"], bufs=bufs, kind=kind)
    if kind == "int":
        # every rounding point of the int64 reference holds an integer of magnitude <= 256: exact in bf16, so the kernel's result is the
        # reference's whatever its summation order (fp32 partial sums of integers below 2^24 are exact)
        lin = (inp.a.double() @ inp.w.double().t()).to(I64) + (inp.bias.to(I64) if c.bias else 0)
        assert int(lin.abs().max()) <= 256
        post = _act(lin, c.epi, I64)
        assert int((post + (inp.res.to(I64) if c.res else 0)).abs().max()) <= 256
    return inp


def ref_of(c, inp, dt, mut=None, last_round=True):
    return gemm_ref(inp.a, inp.w, inp.bias, inp.res, c.epi, c.f32, dt, mut, last_round)


# ------------------------------------------------------------------------------------------------ a simulated kernel, and the comparison
def simulate(c, inp, mut=None):
    """The output allocation a kernel with fp32 math (exact integers in the integer pass) would leave, with one mutant.  Mutants of the store:
    the column tail (columns from N // 8 * 8 on, fast kernels only) left unwritten / taken from one accumulator further; rows written with
    ldc rounded down to 8; the general one-wave-per-SIMD variant writing its whole last 128-row sub-tile."""
    dt = F32 if c.f32 else BF
    y = ref_of(c, inp, I64 if inp.kind == "int" else F32, mut)
    y = y.to(dt)
    buf, _ = out_buffer(c)
    ld, off = c.lay.c
    t = c.N // 8 * 8
    fastk = c.kernel != "GENERIC"
    if mut == "column_tail_shifted_by_one" and fastk and t < c.N:
        y = y.clone()
        y[:, t:] = torch.roll(y[:, t:], -1, 1)
    if mut == "c_rows_written_with_ld_rounded_to_8":
        ld = ld & ~7
    rows = c.M
    if mut == "row_tail_written_past_m" and c.kernel == "W4G":
        rows = min((c.M + 127) // 128 * 128, c.M + c.tall)
        y = torch.cat([y, torch.zeros(rows - c.M, c.N, dtype=dt)])
    cols = t if (mut == "column_tail_unwritten" and fastk) else c.N
    _view(buf, rows, c.N, ld, off)[:, :cols] = y[:, :cols]
    return buf


def groups_of(c):
    """interior rows and columns, the last row tile, the last column tile (of the kernel the case reaches)"""
    T = TILE[c.kernel]
    mi, ni = (c.M - 1) // T * T, (c.N - 1) // T * T
    return {"interior": (slice(0, mi), slice(0, ni)), "last_row_tile": (slice(mi, c.M), slice(None)), "last_col_tile": (slice(None), slice(ni, c.N))}


def verify(c, inp, buf, mask, refs=None):
    """What the GPU test asserts of the output allocation `buf` (a CPU tensor) after the call:
       outside   every element outside the view still holds the sentinel bits
       exact     integer pass: the view equals the int64 reference
       bounded   gaussian pass: {group: (regimes.group_err against fp64, regimes.bound)} with y the fp32 reference's own error
    -> NS(outside, exact (None in the gaussian pass), bounded ({} in the integer pass))"""
    dt = F32 if c.f32 else BF
    it, bits = SENT[dt]
    outside = bool((buf.view(it)[~mask] == bits).all())
    got = out_view(c, buf)
    if inp.kind == "int":
        want = ref_of(c, inp, I64)
        return NS(outside=outside, exact=bool(torch.equal(got.to(F64), want.to(F64))), bounded={})
    ref64, ref32 = refs if refs is not None else (ref_of(c, inp, F64, last_round=False), ref_of(c, inp, F32, last_round=False))
    gr = groups_of(c)
    spec = R.out_spec(n=c.K) if c.f32 else R.out_spec(r=roundings(c))
    y = R.group_err(ref32, ref64, gr)
    e = R.group_err(got, ref64, gr)
    return NS(outside=outside, exact=None, bounded={g: (e[g], R.bound(spec, y[g])) for g in e})


def rejected(v):
    return (not v.outside) or v.exact is False or any(not e <= b for e, b in v.bounded.values())
