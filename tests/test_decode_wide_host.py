"""The wide decode GEMMs (vp_decode_gemm_wide / _w8_wide / _w4_wide: 17 <= M <= 64 rows on one streamed weight) without a GPU: the C ABI
in header and binding, the argument checks (the library loads without a device), the workspace query, the host-side routing and refusals,
and the registers of the new kernels as the built library records them."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("", "_w8", "_w4")
F = ctypes.c_float(1e-5)


def _lib():
    from visper_lm_amd import _lib as L
    return L


def _gemm(lib, kind, suffix, M, N, K, ptr, epi=0, a=True, ws=None, ld=None):
    """one call with a dummy pointer for every operand (never dereferenced: the checks fail first)"""
    ld = ld or max(N, K)
    head = (M, N, K, ptr if a else None, ld, ptr, ld)
    mid = {"": (), "_w8": (ptr,), "_w4": (ptr, ld)}[kind]
    return getattr(lib, "vp_decode_gemm" + kind + suffix)(*head, *mid, ptr, ld, None, 0, None, F, epi, 0, ws, None)


def test_wide_entry_points_in_header_and_binding():
    L = _lib()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "visper_hip.h")).read()
    for kind in KINDS:
        for name in (f"vp_decode_gemm{kind}_wide", f"vp_decode_gemm{kind}_wide_workspace_bytes"):
            assert name in L.EXPORTS and hasattr(lib, name), name
            assert re.search(r"\b(int|long) " + name + r"\(", header), name
        # the argument list is the parent's
        assert L._SIGS[f"vp_decode_gemm{kind}_wide"] == L._SIGS[f"vp_decode_gemm{kind}"]
        assert getattr(lib, f"vp_decode_gemm{kind}_wide_workspace_bytes").restype is ctypes.c_long


@pytest.mark.parametrize("kind", KINDS)
def test_wide_entry_points_reject_bad_arguments(kind):
    lib = _lib().load()
    err = lambda: lib.vp_last_error_string()
    p = ctypes.c_void_p(16)
    name = f"vp_decode_gemm{kind}_wide".encode()
    for M in (0, 65):
        assert _gemm(lib, kind, "_wide", M, 64, 64, p) == -2
        assert name in err() and f"M = {M}".encode() in err() and b"<= 64" in err(), err()
    # the parents' codes: null operand, bad K, SwiGLU with N % 16 != 0, a split-K shape without workspace
    for M in (1, 16, 17, 64):
        assert _gemm(lib, kind, "", 1, 64, 64, p, a=False) == _gemm(lib, kind, "_wide", M, 64, 64, p, a=False) == -1
        assert name + b": null" in err()
        assert _gemm(lib, kind, "", 1, 64, 60, p) == _gemm(lib, kind, "_wide", M, 64, 60, p) == -2
        assert name + b": N = 64, K = 60" in err()
        assert _gemm(lib, kind, "", 1, 40, 64, p, epi=4) == _gemm(lib, kind, "_wide", M, 40, 64, p, epi=4) == -2
        assert name + b": SwiGLU" in err()
        assert _gemm(lib, kind, "", 1, 4096, 4096, p) == _gemm(lib, kind, "_wide", M, 4096, 4096, p) == -1
        assert b"workspace" in err() and name + b"_workspace_bytes" in err()
        assert _gemm(lib, kind, "_wide", M, 64, 64, p, epi=9) == -1


@pytest.mark.parametrize("kind", KINDS)
def test_parent_entry_points_still_refuse_m_17_and_point_at_the_wide_ones(kind):
    lib = _lib().load()
    p = ctypes.c_void_p(16)
    assert _gemm(lib, kind, "", 17, 64, 64, p) == -2
    e = lib.vp_last_error_string()
    assert f"vp_decode_gemm{kind}: M = 17 (1 <= M <= 16".encode() in e and f"vp_decode_gemm{kind}_wide".encode() in e, e
    assert _gemm(lib, kind, "", 64, 64, 64, p) == -2


@pytest.mark.parametrize("kind", KINDS)
def test_wide_workspace_query_covers_the_slabs(kind):
    import decode_cases as DC
    lib = _lib().load()
    q = getattr(lib, f"vp_decode_gemm{kind}_wide_workspace_bytes")
    parent = getattr(lib, f"vp_decode_gemm{kind}_workspace_bytes")
    k = {"": "bf16", "_w8": "w8", "_w4": "w4"}[kind]
    for N, K, epi in ((4096, 4096, 0), (6144, 4096, 0), (128256, 4096, 0), (136, 1024, 0), (256, 2048, 4), (256, 1024, 5), (28672, 4096, 4)):
        ks = DC.ksplit(k, N, K, epi)
        prev = 0
        for M in range(1, 65):
            b = q(M, N, K, epi)
            assert b >= (ks * M * N * 4 if ks > 1 else 0) and b >= prev, (kind, M, N, K, epi)
            if M <= 16:
                assert b == parent(M, N, K, epi)
            prev = b
    assert q(0, 64, 64, 0) == 0


def test_ops_routing_is_decided_on_the_host():
    from visper_lm_amd import ops
    assert ops._decode_gemm_route(1, None) == ops._decode_gemm_route(16, None) == ops._decode_gemm_route(16, False) == ("", 16)
    assert ops._decode_gemm_route(17, None) == ops._decode_gemm_route(64, None) == ("_wide", 64)
    assert ops._decode_gemm_route(17, False) == ops._decode_gemm_route(64, False) == ("", 16)
    for wide in (None, False):
        with pytest.raises(ValueError, match="at most 64"):
            ops._decode_gemm_route(65, wide)
        with pytest.raises(ValueError, match="at most 64"):
            ops.decode_gemm_ws_bytes(65, 4096, 4096, wide=wide)
        with pytest.raises(ValueError, match="at most 64"):                        # before any pointer is taken: CPU tensors never reach the library
            ops.decode_gemm(torch.zeros(65, 64, dtype=torch.bfloat16), torch.zeros(64, 64, dtype=torch.bfloat16), wide=wide)
    for w8, w4 in ((False, False), (True, False), (False, True)):
        kw = dict(w8=w8, w4=w4)
        ks_bytes = ops.decode_gemm_ws_bytes(1, 4096, 4096, **kw)
        assert ks_bytes > 0
        assert ops.decode_gemm_ws_bytes(40, 4096, 4096, **kw) == 40 * ks_bytes                   # one wide call: slabs of 40 rows
        assert ops.decode_gemm_ws_bytes(40, 4096, 4096, wide=False, **kw) == 16 * ks_bytes       # chunked: the largest slice's
        assert ops.decode_gemm_ws_bytes(12, 4096, 4096, wide=False, **kw) == 12 * ks_bytes


def test_generate_refuses_more_than_64_sequences_before_any_gpu_work(monkeypatch):
    from test_generate_host import _cpu_model
    from visper_lm_amd import decode
    model, batch = _cpu_model()
    built = []
    monkeypatch.setattr(type(model), "_get_engine", lambda self: built.append(1) or (_ for _ in ()).throw(AssertionError("engine built")))
    ids = batch["input_ids"][:1].repeat(65, 1)
    with pytest.raises(ValueError, match=r"65 sequences.*at most 64"):
        model.generate(ids, max_new_tokens=2)
    with pytest.raises(ValueError, match=r"65 sequences.*at most 64"):
        decode.generate(None, ids, max_new_tokens=2)                               # no engine is touched
    # the older refusals still come first
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(ids, num_beams=4)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        model.generate(ids, kv_cache_dtype="int3")
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens = 2 at batch 65"):
        model.generate(ids, prompt_lookup_num_tokens=2)
    assert not built
    decode.check_batch(64)
    assert decode.MAX_BATCH == 64 and decode.MAX_VERIFY_ROWS == 16 and decode.DecodeSession.wide_gemm is None


def test_wide_kernels_exist_for_every_format_and_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    L = _lib()
    ks = KR.matching(L.LIB_PATH, ["decode_gemm_wide_kernel", "decode_gemm_w8_wide_kernel", "decode_gemm_w4_wide_kernel"])
    for fmt in ("decode_gemm_wide_kernel", "decode_gemm_w8_wide_kernel", "decode_gemm_w4_wide_kernel"):
        for norm in ("false", "true"):
            for tiles in (2, 3, 4):
                hit = [d for n, d in ks.items() if re.search(rf"\b{fmt}<{norm}, {tiles}>", n)]
                assert len(hit) == 1, (fmt, norm, tiles, sorted(ks))
                d = hit[0]
                assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0, (fmt, norm, tiles, d)
                assert d["vgpr_count"] + d.get("agpr_count", 0) <= 256, (fmt, norm, tiles, d)      # at least 2 waves per SIMD
    assert len(ks) == 18, sorted(ks)
