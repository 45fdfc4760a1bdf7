"""csrc/gemm_route.h compiled with the host compiler (tests/route_shim.cpp, loaded with ctypes; nothing is committed as a binary):

1. every case of tests/gemm_cases.py reaches the kernel, grid class and c_nt its row states;
2. over a grid of problems, whatever kernel the route returns, the preconditions that kernel's comments and the header state hold;
3. the Python mirrors of the routing in visper_lm_amd/ops.py admit nothing the library refuses."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest
import torch

import gemm_cases as G

HERE = os.path.dirname(os.path.abspath(__file__))
NQ = 24


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and shutil.which(cand.split()[0]):
            return cand.split()
    return None


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine ($CXX, c++, g++, clang++)")
    so = str(tmp_path_factory.mktemp("route_shim") / "route_shim.so")
    subprocess.check_call(cxx + ["-std=c++17", "-O1", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "route_shim.cpp")])
    lib = C.CDLL(so)
    L = C.c_long
    lib.route.argtypes = [C.POINTER(L), C.POINTER(L)]
    lib.route_many.argtypes = [L, C.c_void_p, C.c_void_p]
    lib.route_swiglu.argtypes = [L] * 10 + [C.POINTER(L)]
    for name, n in (("grid_p8", 3), ("c_nt", 3), ("sel_known", 1), ("kernel_id", 1)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [L] * n, L
    lib.names = {int(lib.kernel_id(i)): k for i, k in enumerate(G.KERNELS)}
    assert lib.names[-1] == "NONE" and len(lib.names) == len(G.KERNELS)
    return lib


def problem(M, N, K, lda, ldb, ldc, ldr, al, bias, res, epi, f32, sel, sched_ws=0, w4=1, w4g=1, ph4=1, c_nt=1, dbg=0):
    return [M, N, K, lda, ldb, ldc, ldr, *al, int(bias), int(res), epi, int(f32), sel, sched_ws, w4, w4g, ph4, c_nt, dbg, 0]


def problem_of(c, **switches):
    return problem(c.M, c.N, c.K, c.lay.a[0], c.lay.b[0], c.lay.c[0], c.lay.r[0] if c.res else 0, G.alignment(c), c.bias, c.res, c.epi, c.f32, c.sel,
                   **switches)


def route(shim, q):
    assert len(q) == NQ
    out = (C.c_long * 4)()
    shim.route((C.c_long * NQ)(*q), out)
    return G.NS(kernel=shim.names[out[0]], grid=int(out[1]), sched=bool(out[2]), c_nt=int(out[3]))


# ------------------------------------------------------------------------------------------------ 1. the case table
@pytest.mark.parametrize("c", G.CASES + G.LARGE_LD, ids=lambda c: c.name)
def test_case_reaches_its_kernel(shim, c):
    r = route(shim, problem_of(c))
    assert r.kernel == c.kernel, (c.name, r)
    assert r.c_nt == c.c_nt and r.sched == c.sched, (c.name, r)
    if c.grid is not None:
        assert r.grid == c.grid, (c.name, r)
    if r.kernel in ("W4", "W4G", "NT256"):
        assert r.grid == min(256, ((c.M + 255) // 256) * ((c.N + 255) // 256))
    if c.twin is not None:
        t = route(shim, problem_of(G.twin_of(c)))
        assert t.kernel == c.kernel, ("twin", c.name, t)


def test_routes_worth_pinning(shim):
    """the routes worth pinning, stated once more by shape (a renamed case cannot take them along)"""
    al0 = (0, 0, 0, 0, 0)
    k = lambda *a, **kw: route(shim, problem(*a, **kw)).kernel
    assert k(3072, 3840, 128, 128, 128, 3840, 0, al0, 0, 0, 0, 1, 0) == "NT128"            # an out_f32 problem of 180 tiles: the 128-tile kernel
    assert k(3072, 3840, 128, 128, 128, 3840, 0, al0, 0, 0, 0, 0, 0) == "W4G"              # a plain bf16 problem of 180 tiles: the general variant
    assert k(300, 50, 64, 64, 64, 50, 0, al0, 0, 0, 0, 0, 8) == "NT128"                    # a refused 8 / 14 lands on the 128-tile kernel
    assert k(300, 50, 64, 64, 64, 50, 0, al0, 0, 0, 0, 0, 14) == "NT128"
    assert k(255, 256, 128, 128, 128, 256, 256, al0, 1, 1, 0, 0, 14) == "NT128" and k(300, 256, 128, 128, 128, 256, 256, al0, 1, 1, 0, 0, 14) == "W4G"
    r = route(shim, problem(4352, 4096, 192, 192, 192, 4096, 0, al0, 0, 0, 0, 0, 7))
    assert (r.kernel, r.grid, r.sched) == ("P8", 272, False)
    r = route(shim, problem(4352, 4096, 128, 128, 128, 4096, 0, al0, 0, 0, 0, 0, 7))
    assert (r.kernel, r.grid, r.sched) == ("P8", 256, True)
    r = route(shim, problem(512, 256, 128, 128, 128, 1 << 22, 0, al0, 0, 0, 0, 0, 7))
    assert (r.kernel, r.c_nt) == ("P8", 0)
    r = route(shim, problem(256, 256, 128, 128, 128, G.LD_EDGE, 0, al0, 0, 0, 0, 0, 7))
    assert (r.kernel, r.c_nt) == ("P8", 1) and 256 * G.LD_EDGE * 2 == 2147479552 < 0x7fffffff


# ------------------------------------------------------------------------------------------------ 2. properties over a grid
SELS = [0, 1, 2, 3, 7, 8, 13, 14]
# the grid the route was once compared on against a transcription of its predecessor (EXPERIMENTS.md, "One host-side launch layer") ...
PRODUCT = list(itertools.product([1, 64, 128, 255, 256, 300, 512, 4096, 8192, 16384], [1, 64, 128, 255, 256, 300, 512, 4096, 8192, 16384],
                                 [32, 64, 96, 128, 192, 4096]))
# ... and the shapes at the route's thresholds
SHAPES = [(1, 1024, 64), (255, 256, 128), (256, 256, 64), (256, 256, 128), (257, 256, 128), (300, 50, 64), (300, 200, 128), (512, 256, 128),
          (512, 256, 192), (77, 50, 40), (2048, 2048, 128), (2048, 1792, 128), (1800, 2048, 128), (3072, 3840, 128), (3072, 4096, 128),
          (3072, 4096, 192), (4352, 4096, 128), (4352, 4096, 192), (4096, 16384, 256), (256, 256, 1 << 20)]


def _grid():
    """problems x switches, thinned: every (shape, selector, epilogue set) meets each state of ONE operand at a time (padded by 8, an odd leading
    dimension, a base one element off, and for C and the residual both sides of 1 << 22; the route's conditions are conjunctions: two operands
    misaligned at once take no other branch than one of them), the all-aligned problem meets every switch setting, and a seeded sample of the
    full product comes on top"""
    qs = []
    epis = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 3, 0), (0, 1, 3, 0), (1, 1, 2, 0), (0, 0, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1)]
    sw = [dict(), dict(w4=0), dict(w4=2), dict(w4=2, sched_ws=1), dict(w4g=0), dict(ph4=0), dict(c_nt=0), dict(sched_ws=1)]
    for (M, N, K), sel, (bias, res, epi, f32) in itertools.product(SHAPES, SELS, epis):
        variants = [dict()]                                   # {field: value}; "al": (operand index, pointer & 15)
        for key, i in (("lda", 0), ("ldb", 1)):
            variants += [{key: K + 8}, {key: K + 1}, {"al": (i, 2)}]
        variants += [{"ldc": N + 8}, {"ldc": N + 1}, {"al": (2, 4 if f32 else 2)}, {"ldc": G.LD_EDGE}, {"ldc": 1 << 22}]
        if bias:
            variants += [{"al": (3, 2)}]
        if res:
            variants += [{"ldr": N + 8}, {"ldr": N + 1}, {"al": (4, 2)}, {"ldr": G.LD_EDGE}, {"ldr": 1 << 22}]
        for v in variants:
            d = dict(lda=K, ldb=K, ldc=N, ldr=N if res else 0)
            al = [0] * 5
            if "al" in v:
                al[v["al"][0]] = v["al"][1]
            d.update({k: x for k, x in v.items() if k != "al"})
            for s in (sw if not v else sw[:1]):
                qs.append(problem(M, N, K, d["lda"], d["ldb"], d["ldc"], d["ldr"], al, bias, res, epi, f32, sel, **s))
    for (M, N, K), sel, (bias, res, epi, f32) in itertools.product(PRODUCT, SELS, epis):      # the product of sizes: all aligned, default switches
        qs.append(problem(M, N, K, K, K, N, N if res else 0, [0] * 5, bias, res, epi, f32, sel))
    sw += [dict(dbg=0x20000), dict(w4=0, ph4=0), dict(w4g=0, c_nt=0, sched_ws=1)]
    g = torch.Generator().manual_seed(5)
    pick = lambda xs: xs[int(torch.randint(0, len(xs), (1,), generator=g))]
    for _ in range(60000):
        M, N, K = pick(SHAPES + PRODUCT)
        bias, res, epi, f32 = pick(epis)
        lds = [pick([0, 8, 1, (1 << 22) - 8, 1 << 22]) for _ in range(4)]
        ld = [K + min(lds[0], 8), K + min(lds[1], 8), lds[2] if lds[2] >= 1 << 21 else N + lds[2], lds[3] if lds[3] >= 1 << 21 else N + lds[3]]
        al = [pick([0, 0, 2]), pick([0, 0, 2]), pick([0, 0, 4 if f32 else 2]), pick([0, 2]) if bias else 0, pick([0, 2]) if res else 0]
        qs.append(problem(M, N, K, ld[0], ld[1], ld[2], ld[3] if res else 0, al, bias, res, epi, f32, pick(SELS), **pick(sw)))
    return qs


def test_route_properties(shim):
    qs = _grid()
    n = len(qs)
    flat = torch.tensor(qs, dtype=torch.int64).contiguous()
    out = torch.zeros(n, 4, dtype=torch.int64)
    shim.route_many(n, flat.data_ptr(), out.data_ptr())
    seen = set()
    for q, (kid, grid, sched, c_nt) in zip(qs, out.tolist()):
        M, N, K, lda, ldb, ldc, ldr, a_al, b_al, c_al, bias_al, res_al, bias, res, epi, f32, sel, sched_ws, w4, w4g, ph4, c_nt_sw, dbg, _ = q
        k = shim.names[kid]
        seen.add(k)
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        why = (k, q)
        assert k not in ("NONE", "W4F", "TN"), why                      # vp_gemm_bf16 always finds a kernel, and never a sibling's
        if sel == 1:
            assert k == "GENERIC", why
        if k != "GENERIC":                                              # every fast kernel
            assert K % 64 == 0 and lda % 8 == 0 and ldb % 8 == 0 and a_al == 0 and b_al == 0, why
        if k == "W4":
            assert M % 256 == 0 and N % 256 == 0 and K % 128 == 0 and not bias and epi == 0 and c_al == 0 and sel in (0, 8), why
            assert ldc % (4 if f32 else 8) == 0 and not (res and f32), why
            if not f32:
                assert ldc < 1 << 22 and (not res or (ldr % 8 == 0 and ldr < 1 << 22 and res_al == 0)), why
            if sel == 0:
                assert tiles >= 192 and (w4 == 1 or (w4 == 2 and not sched_ws)), why
        if k == "W4G":
            assert N % 256 == 0 and K % 128 == 0 and M >= 256 and not f32 and c_al == 0 and bias_al == 0 and sel in (0, 14), why
            assert ldc % 8 == 0 and ldc < 1 << 22 and not (res and epi != 0), why
            assert not res or (ldr % 8 == 0 and ldr < 1 << 22 and res_al == 0), why
            if sel == 0:
                assert tiles >= 64 and epi != G.EPI_GELU and w4g == 1, why
        if k == "PH4":
            assert not f32 and sel in (0, 13) and (sel == 13 or ph4 != 0), why
        if k in ("W4", "W4G", "NT256"):
            assert grid == min(tiles, 256), why                         # a persistent grid is <= 256
        if k in ("P8", "PH4"):
            assert grid == (256 if (K // 64) % 2 == 0 and tiles > 256 and not dbg & 0x20000 else tiles), why
        if k == "NT128":
            assert grid == ((M + 127) // 128) * ((N + 127) // 128), why
        if sched:
            assert k in ("P8", "PH4") and grid == 256, why
        if c_nt:
            assert k in ("W4", "P8", "PH4") and not f32 and N <= 8192 and c_nt_sw != 0, why
            assert not (k in ("P8", "PH4") and M * ldc * 2 >= 0x7fffffff), why
        if k in ("W4", "W4G", "P8", "PH4", "NT256") and sel == 0 and k != "W4G":
            assert tiles >= 192, why
    assert seen == {"W4", "W4G", "P8", "PH4", "NT256", "NT128", "GENERIC"}, seen
    assert not shim.sel_known(4) and not shim.sel_known(-1) and all(shim.sel_known(s) for s in SELS)


def test_grid_and_c_nt_rules(shim):
    for K, tiles in itertools.product((64, 128, 192, 256, 4096), (1, 2, 192, 256, 257, 272, 1024)):
        want = 256 if (K // 64) % 2 == 0 and tiles > 256 else tiles
        assert shim.grid_p8(K, tiles, 0) == want
        assert shim.grid_p8(K, tiles, 0x20000) == tiles                # the debug flag: always one block a tile
    for f32, N, sw in itertools.product((0, 1), (8, 8192, 8200, 16384), (0, 1)):
        assert shim.c_nt(f32, N, sw) == int(not f32 and N <= 8192 and sw != 0)


# ------------------------------------------------------------------------------------------------ 3. the Python mirrors
DIMS = [255, 256, 257, 300, 512, 2048, 4096, 14336]
KS = [64, 128, 192]
# shapes right at the tile thresholds of the mirrors (64 and 192 big tiles), each with its neighbours
THRESHOLD = [(2048, 2048), (2048, 1792), (1792, 2304), (3072, 4096), (3072, 3840), (4096, 3072), (256, 49152), (256, 48896), (256, 16384), (256, 16128)]


def rope_require(M, N, K, rope_cols=0, ld_ok=True):
    """the VP_REQUIRE of vp_gemm_bf16_rope (csrc/gemm.hip), restated once: what the entry point admits for contiguous aligned operands"""
    return N % 256 == 0 and K % 128 == 0 and M >= 256 and rope_cols % 128 == 0 and ld_ok and N < 1 << 22


@pytest.mark.parametrize("env", [{}, {"VP_GEMM_W4": "0"}, {"VP_GEMM_W4": "2"}, {"VP_GEMM_ROPE": "0"}, {"VP_FOLD_NORM": "0"}, {"VP_GEMM_PH4": "0"}])
def test_python_mirrors_admit_nothing_the_library_refuses(shim, env, monkeypatch):
    for k in ("VP_GEMM_W4", "VP_GEMM_ROPE", "VP_FOLD_NORM", "VP_GEMM_PH4", "VP_GEMM_W4G"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from visper_lm_amd import ops
    w4, ph4 = int(env.get("VP_GEMM_W4", "1")), int(env.get("VP_GEMM_PH4", "1"))
    out = (C.c_long * 4)()
    shapes = [(M, N) for M in DIMS for N in DIMS] + THRESHOLD
    admitted = dict(swiglu=0, fold=0, rowscale=0, tn=0)
    for (M, N), K in itertools.product(shapes, KS):
        if ops.swiglu_fusable(M, N, K):
            admitted["swiglu"] += 1
            assert M % 256 == 0 and N % 256 == 0 and K % 64 == 0           # vp_gemm_bf16_swiglu's own VP_REQUIRE
            for sched_ws in (0, 1):
                shim.route_swiglu(M, N, K, N, N // 2, 0, 0, sched_ws, w4, ph4, out)                     # mode 1, contiguous
                assert shim.names[out[0]] in ("W4", "P8", "PH4"), (M, N, K, env)
                shim.route_swiglu(M, N, K, 2 * N, 0, 2 * N, 0, sched_ws, w4, ph4, out)                   # mode 2
                assert shim.names[out[0]] in ("W4", "P8", "PH4"), (M, N, K, env)
        if ops.gemm_tn_ok(M, N, K):
            admitted["tn"] += 1
            assert M % 256 == 0 and N % 256 == 0 and K % 64 == 0           # vp_gemm_tn_bf16's VP_REQUIRE
        if ops.gemm_rowscale_ok(M, N, K):
            admitted["rowscale"] += 1
            assert rope_require(M, N, K), (M, N, K)
            assert ops.gemm_rope_ok(M, N, K, 128) and not ops.gemm_rope_ok(M, N, K, 96)
            assert rope_require(M, N, K, rope_cols=128)
        # fold_norm_ok(M, H, I, head_dim, nqkv): its SwiGLU clause is the gate_up GEMM [M, 2 I] x [2 I, H] with a row scale.  The engine has no
        # sched_ws on one GPU; with one (world > 1) VP_GEMM_W4 = 2 sends the route elsewhere, which the mirror excludes by asking for W4 == 1.
        H, I = N, K * 32
        for nqkv in (N, 3 * N):
            if ops.fold_norm_ok(M, H, I, 128, nqkv):
                admitted["fold"] += 1
                for sched_ws in (0, 1):
                    shim.route_swiglu(M, 2 * I, H, 2 * I, I, 0, 1, sched_ws, w4, ph4, out)
                    assert shim.names[out[0]] == "W4F", (M, H, I, env)
                assert rope_require(M, nqkv, H) and M % 256 == 0 and H % 256 == 0
    if not env:
        assert all(v > 0 for v in admitted.values()), admitted
    if env.get("VP_GEMM_ROPE") == "0":
        assert admitted["rowscale"] == 0 and admitted["fold"] == 0
    if env.get("VP_FOLD_NORM") == "0" or env.get("VP_GEMM_W4") in ("0", "2"):
        assert admitted["fold"] == 0
