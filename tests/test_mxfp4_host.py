"""MXFP4 weight-only decoding without a GPU: the properties of the format contract (quant.py), the new entry points' argument checks (the
library loads without a device), the built W4 kernels' code-object metadata, and the mirrors' quantize_for_generation_4bit()."""
import ctypes
import os
import sys

import pytest
import torch

from test_quant_host import _cpu_model, _matrices

BF16 = torch.bfloat16


def _mx_matrices():
    """test_quant_host._matrices() (rows of zeros, an outlier, bf16 subnormals, absmax walking through whole binades) plus binades 5 - 8
    (blocks around the scale clamp at 2^-120: bytes 7 and just above), and a matrix whose blocks differ in scale within a row."""
    g = torch.Generator().manual_seed(1)
    out = _matrices()
    bits = torch.cat([torch.arange(e << 7, (e + 1) << 7) for e in (5, 6, 7, 8)]).to(torch.int16)
    w = torch.zeros(bits.numel(), 64, dtype=BF16)
    w[:, 0] = bits.view(BF16)
    w[:, 1:] = (w[:, :1].double() * torch.rand(bits.numel(), 63, generator=g).double()).to(BF16)
    out.append(w)
    w = (torch.randn(64, 256, generator=g) * 0.02).view(64, 8, 32) * torch.exp2(torch.randint(-3, 4, (64, 8, 1), generator=g).float())
    out.append(w.view(64, 256).to(BF16))
    return out


def test_quantize_blocks_mxfp4_properties():
    """float64 restatement of the contract, every property asserted exactly"""
    from visper_lm_amd import quant
    grid = torch.tensor(quant.E2M1_VALUES, dtype=torch.float64)
    seen_codes = set()
    for w in _mx_matrices():
        N, K = w.shape
        q, e = quant.quantize_blocks_mxfp4(w)
        assert q.dtype == torch.uint8 and q.shape == (N, K // 2) and e.dtype == torch.uint8 and e.shape == (N, K // 32)
        assert int(e.min()) >= 7 and int(e.max()) <= 252, (int(e.min()), int(e.max()))
        deq = quant.dequantize_mxfp4(q, e)
        assert deq.dtype == torch.float32 and deq.shape == w.shape
        assert torch.equal(deq.to(BF16).float(), deq), "q * s is exactly representable in bf16"
        nz = deq[deq != 0].abs()
        assert nz.numel() == 0 or float(nz.min()) >= 2.0 ** -126, "every nonzero dequantised value is a normal bf16 number"
        wd, dd = w.double().view(N, K // 32, 32), deq.double().view(N, K // 32, 32)
        s = torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e.to(torch.int64) - 127)
        amax = wd.abs().amax(2)
        zero = amax == 0
        assert (e[zero] == 127).all() and (dd[zero] == 0).all(), "a block of zeros gets byte 127"
        clamped = (e == 7) & ~zero                                   # exponent -120: the clamp may hold (absmax / s can then be below 3)
        free = ~zero & ~clamped
        scaled = amax / s
        assert (scaled[free] > 3).all() and (scaled[free] <= 6).all(), (float(scaled[free].min()), float(scaled[free].max()))
        assert (scaled <= 6).all(), "nothing saturates, clamped blocks included"
        # every dequantised value is a grid value times its block's scale
        t = (dd / s[:, :, None]).abs()
        assert torch.isin(t, grid).all()
        # block-wise error: half a step of the e2m1 grid at the scaled magnitude
        a = wd.abs() / s[:, :, None]
        step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0)).double()
        err = (wd - dd).abs()
        assert (err <= s[:, :, None] * step / 2).all(), float((err / (s[:, :, None] * step / 2)).max())
        # ties go to the even code: where the error is exactly half a step the chosen code is even
        code = torch.stack([q & 0xf, q >> 4], dim=2).view(N, K // 32, 32)
        tie = (err == s[:, :, None] * step / 2) & (err > 0)
        assert ((code[tie] & 1) == 0).all()
        # the sign bit is the weight's, also on values that rounded to zero
        assert torch.equal((code & 8) != 0, torch.signbit(w).view(N, K // 32, 32))
        seen_codes |= set(code.unique().tolist())
    assert seen_codes == set(range(16)), sorted(seen_codes)


def test_mxfp4_packing_and_dequantize_by_hand():
    """element k in byte k // 2, even k in the low nibble; codes 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 is the sign; scale 2^(byte - 127)"""
    from visper_lm_amd import quant
    vals = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    row = torch.tensor(vals + [-v for v in vals] + [0.0] * 16) * 2.0 ** -5                 # absmax 6 * 2^-5: scale 2^-5, byte 122
    q, e = quant.quantize_blocks_mxfp4(row.to(BF16)[None])
    assert e.tolist() == [[122]]
    want = [(2 * i) | ((2 * i + 1) << 4) for i in range(8)] + [0] * 8
    want[4] = 0x08 | (9 << 4)                                                               # -0.0 keeps its sign bit: code 8
    assert q[0].tolist() == want, q[0].tolist()
    assert torch.equal(quant.dequantize_mxfp4(q, e)[0], row.float())
    # ties to the even code on every midpoint of the grid, scale 1 (absmax 6 pins byte 127)
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0] + [6.0] + [0.0] * 24)
    q, e = quant.quantize_blocks_mxfp4(mids.to(BF16)[None])
    assert e.tolist() == [[127]]
    assert quant.dequantize_mxfp4(q, e)[0, :8].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0]


def test_quantize_mxfp4_is_idempotent_on_dequantised_weights():
    """write-back makes the bf16 weights the dequantised model; quantising those again must give the same VALUES (a block whose largest code
    rounded down to 3 gets half the scale the second time, a block that rounded to all zeros gets byte 127)"""
    from visper_lm_amd import quant
    halved = 0
    for w in _mx_matrices():
        q, e = quant.quantize_blocks_mxfp4(w)
        deq = quant.dequantize_mxfp4(q, e)
        q2, e2 = quant.quantize_blocks_mxfp4(deq.to(BF16))
        assert torch.equal(quant.dequantize_mxfp4(q2, e2), deq)
        allzero = deq.view(e.shape[0], e.shape[1], 32).abs().amax(2) == 0
        assert (e2[allzero] == 127).all()
        same, half = e2 == e, e2.to(torch.int64) == e.to(torch.int64) - 1
        assert (same | half | allzero).all()
        top = (deq.double().view(e.shape[0], e.shape[1], 32).abs().amax(2) /
               torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e.to(torch.int64) - 127))
        assert (top[half & ~allzero] == 3).all()
        halved += int((half & ~allzero).sum())
    assert halved > 0, "no block exercised the halved scale"


def test_w4_entry_points_reject_bad_arguments():
    from visper_lm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vp_last_error_string()
    p = ctypes.c_void_p(16)                                           # never dereferenced: every call below fails its checks first
    eps = ctypes.c_float(1e-5)
    w4 = lambda M, N, K, A=p, W=p, E=p, epi=0, ws=None: lib.vp_decode_gemm_w4(M, N, K, A, K, W, K // 2, E, K // 32, p, N, None, 0, None, eps, epi, 0,
                                                                              ws, None)
    bf = lambda M, N, K, A=p, W=p, epi=0, ws=None: lib.vp_decode_gemm(M, N, K, A, K, W, K, p, N, None, 0, None, eps, epi, 0, ws, None)
    assert bf(17, 64, 64) == w4(17, 64, 64) == -2 and b"vp_decode_gemm_w4" in err() and b"M = 17" in err()
    assert w4(0, 64, 64) == bf(0, 64, 64) == -2
    assert w4(1, 64, 64, A=None) == bf(1, 64, 64, A=None) == -1
    assert w4(1, 64, 64, W=None) == -1
    assert w4(1, 64, 64, E=None) == -1 and b"block scales" in err()   # a null scale pointer is a null operand
    assert w4(1, 64, 80) == -2 and b"multiple of 32" in err()         # K % 32 (K = 80 passes the bf16 sibling's K % 8)
    assert w4(1, 64, 60) == bf(1, 64, 60) == -2
    assert w4(1, 40, 64, epi=4) == bf(1, 40, 64, epi=4) == -2         # SwiGLU with N % 16 != 0
    assert w4(1, 64, 64, epi=9) == bf(1, 64, 64, epi=9) == -1
    assert lib.vp_decode_gemm_w4(1, 64, 64, ctypes.c_void_p(24), 64, p, 32, p, 2, p, 64, None, 0, None, eps, 0, 0, None, None) == -2     # A not 16-byte aligned
    assert lib.vp_decode_gemm_w4(1, 64, 64, p, 64, p, 24, p, 2, p, 64, None, 0, None, eps, 0, 0, None, None) == -2                       # ldw < K / 2
    assert lib.vp_decode_gemm_w4(1, 64, 64, p, 64, p, 32, p, 1, p, 64, None, 0, None, eps, 0, 0, None, None) == -2                       # lde < K / 32
    assert lib.vp_decode_gemm_w4(1, 64, 64, p, 64, p, 32, p, 2, p, 64, p, 64, None, eps, 0, 1, None, None) == -1                         # fp32 out + residual
    assert bf(1, 4096, 4096) == w4(1, 4096, 4096) == -1 and b"workspace" in err()          # split-K shape without workspace
    # the workspace query is a pure function of the shape
    q = lib.vp_decode_gemm_w4_workspace_bytes
    assert q(1, 4096, 4096, 0) > 0 and q(1, 6144, 4096, 0) > 0 and q(1, 128256, 4096, 0) == 0 and q(0, 64, 64, 0) == 0
    for args in ((1, 4096, 4096, 0), (8, 6144, 4096, 0), (16, 28672, 4096, 4), (3, 4096, 14336, 0), (1, 128, 256, 5), (2, 64, 8192, 0)):
        assert q(*args) == q(*args)
        assert q(*args) % (args[0] * args[1] * 4) == 0                # whole fp32 slabs [ks][M][N]
    # quantiser: null pointers, leading dimensions, K % 32
    qb = lib.vp_quant_blocks_mxfp4
    assert qb(4, 64, None, 64, p, 32, p, 2, 0, None) == -1 and b"vp_quant_blocks_mxfp4" in err()
    assert qb(4, 64, p, 64, None, 32, p, 2, 0, None) == -1
    assert qb(4, 64, p, 64, p, 32, None, 2, 0, None) == -1
    assert qb(4, 64, p, 48, p, 32, p, 2, 0, None) == -1 and b"ldw >= K" in err()
    assert qb(4, 64, p, 64, p, 16, p, 2, 1, None) == -1
    assert qb(4, 64, p, 64, p, 32, p, 1, 1, None) == -1
    assert qb(0, 64, p, 64, p, 32, p, 2, 0, None) == -1
    assert qb(4, 48, p, 48, p, 32, p, 2, 0, None) == -2 and b"multiple of 32" in err()


def test_w4_kernels_use_no_scratch_and_do_not_spill():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    import kernel_resources as kr
    so = os.path.join(os.path.dirname(__file__), "..", "visper-lm_amd", "libvisper_hip.so")
    assert os.path.exists(so), "library not built"
    res = kr.matching(so, ("decode_gemm_w4_kernel", "decode_gemm_combine_kernel", "quant_blocks_mxfp4_kernel"))
    assert len(res) == 4, sorted(res)                                 # <true> / <false> norm prologue, the combine, the quantiser
    for n, d in res.items():
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (n, d)
    for n, d in res.items():
        if "decode_gemm_w4_kernel" in n:
            assert d["vgpr_count"] + d.get("agpr_count", 0) <= 256, (n, d)      # at least 2 blocks of 4 waves per CU


@pytest.mark.parametrize("cls_name", ["OlaLlavaLlamaForCausalLM", "LlavaLlamaForCausalLM", "OlaLlavaPhi3ForCausalLM", "LlavaPhi3ForCausalLM"])
def test_mirrors_have_quantize_for_generation_4bit_and_keep_their_refusals(cls_name):
    import inspect
    model, batch = _cpu_model(cls_name)
    for name in ("quantize_for_generation", "quantize_for_generation_4bit"):
        assert callable(getattr(model, name))
        sig = inspect.signature(getattr(model, name))
        assert list(sig.parameters) == ["lm_head"] and sig.parameters["lm_head"].default is False
    gen = inspect.signature(model.generate)
    assert "weights" not in gen.parameters and "quantize" not in gen.parameters             # generate() keeps its signature
    ids = batch["input_ids"][:1]
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(ids, num_beams=4)
    with pytest.raises(NotImplementedError, match="output_scores"):
        model.generate(ids, output_scores=True)
    with pytest.raises(NotImplementedError, match="return_dict_in_generate"):
        model.generate(ids, return_dict_in_generate=True)
    with pytest.raises(NotImplementedError, match="inputs_embeds"):
        model.generate(ids, inputs_embeds=torch.zeros(1, 3, 128))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):         # there is no CPU path to quantise on: an error, not a silent no-op
            model.quantize_for_generation_4bit()


def test_ops_route_and_engine_signature_import_without_a_device():
    import inspect
    from visper_lm_amd import ops, quant
    from visper_lm_amd.engine import Engine
    sig = inspect.signature(ops.decode_gemm).parameters
    assert sig["w_block_scale"].default is None and sig["w_scale"].default is None
    assert inspect.signature(ops.decode_gemm_ws_bytes).parameters["w4"].default is False
    assert list(inspect.signature(ops.quant_blocks_mxfp4).parameters) == ["w", "writeback"]
    qd = inspect.signature(Engine.quantize_decoder).parameters
    assert list(qd) == ["self", "lm_head", "fmt"] and qd["fmt"].default == "e4m3" and qd["lm_head"].default is False
    assert quant.E2M1_VALUES == (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0) and quant.MXFP4_BLOCK == 32
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.quant_blocks_mxfp4(torch.zeros(8, 32, dtype=BF16))
    with pytest.raises(AssertionError):
        quant.quantize_blocks_mxfp4(torch.zeros(8, 48, dtype=BF16))   # K % 32
