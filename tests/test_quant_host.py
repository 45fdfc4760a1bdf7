"""FP8 weight-only decoding without a GPU: the properties of the format contract (quant.py), the new entry points' argument checks (the
library loads without a device), the built W8 kernels' code-object metadata, and the mirrors' quantize_for_generation()."""
import ctypes
import os
import sys

import pytest
import torch

BF16 = torch.bfloat16


def _matrices():
    """Matrices drawn as the decode tests draw them (randn * 0.02, bf16), with rows of zeros, a row with one huge outlier and a row of bf16
    subnormals spliced in; plus rows whose absmax walks through every bf16 mantissa of a few binades (the scale's decision boundary; the top binade is left out: rounding
    up to 2^128 leaves bf16, quant.py)."""
    g = torch.Generator().manual_seed(0)
    out = []
    for N, K in ((384, 128), (136, 128), (64, 4096), (48, 1024)):
        w = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
        w[3] = 0
        w[5, 7] = 3.0e4                                                        # one huge outlier: the rest of the row falls into the subnormal range / to zero
        sub = torch.randint(0, 128, (K,), generator=g) | (torch.randint(0, 2, (K,), generator=g) << 15)
        w[6] = sub.to(torch.int32).to(torch.int16).view(BF16)                 # sign + mantissa, exponent field 0: a row of bf16 subnormals
        w[7] = 0
        w[7, 1] = torch.tensor([1], dtype=torch.int16).view(BF16)[0]           # the smallest bf16 subnormal alone in its row
        out.append(w)
    bits = torch.cat([torch.arange(e << 7, (e + 1) << 7) for e in (0, 1, 2, 100, 126, 127, 140, 253)]).to(torch.int16)
    w = torch.zeros(bits.numel(), 32, dtype=BF16)
    w[:, 0] = bits.view(BF16)
    w[:, 1:] = (w[:, :1].double() * torch.rand(bits.numel(), 31, generator=g).double()).to(BF16)
    out.append(w)
    return out


def test_quantize_rows_pow2_properties():
    """The issue states the quantised row's absmax range as (224, 448].  That holds for the scaled row w / s before rounding (asserted here
    exactly); after round-to-nearest-even onto e4m3's grid (spacing 32 in [256, 448], 16 in [128, 256)) a scaled absmax in (224, 232] becomes
    224 itself, so the rounded bytes' absmax lies in [224, 448] (also asserted).  No byte saturates either way.
    The two error bounds are split by where the SCALED value lies (|w / s| >= 2^-6: e4m3's normal range), not by the byte it rounds to: a
    value just below 2^-6 that rounds up to the first normal carries the subnormal range's error (half of 2^-9), up to 1/15 of itself."""
    from visper_lm_amd import quant
    for w in _matrices():
        q, s = quant.quantize_rows_pow2(w)
        assert q.dtype == torch.uint8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (w.shape[0],)
        m, _ = torch.frexp(s.double())
        assert (m == 0.5).all(), "every scale is a power of two"
        amax = w.double().abs().amax(1)
        zero = amax == 0
        assert (s[zero] == 1).all() and (q[zero] == 0).all()
        scaled = amax[~zero] / s[~zero].double()
        assert (scaled > 224).all() and (scaled <= 448).all(), (float(scaled.min()), float(scaled.max()))
        qa = q.view(torch.float8_e4m3fn).float().abs().amax(1)[~zero]
        assert (qa >= 224).all() and (qa <= 448).all(), (float(qa.min()), float(qa.max()))
        assert ((q & 0x7f) != 0x7f).all(), "no NaN byte"
        deq = quant.dequantize(q, s)
        assert torch.equal(deq.to(BF16).float(), deq), "q * s is exactly representable in bf16"
        # error: half an ulp of a 3-bit mantissa where the scaled value lies in e4m3's normal range, half the subnormal spacing (x scale) below it
        wd, dd, sd = w.double(), deq.double(), s.double()[:, None]
        normal = (wd.abs() / sd) >= quant.E4M3_MIN_NORMAL
        err = (wd - dd).abs()
        assert (err[normal] <= 2.0 ** -4 * wd.abs()[normal]).all(), float((err[normal] / wd.abs()[normal]).max())
        assert float((err[normal] / wd.abs()[normal]).max()) <= 1.0 / 17 + 1e-12             # 0.0588: a tie just above a power of two
        sub_bound = (0.5 * quant.E4M3_SUBNORMAL_STEP * sd).expand_as(err)
        assert (err[~normal] <= sub_bound[~normal]).all()
        assert torch.equal(torch.signbit(dd)[dd != 0], torch.signbit(wd)[dd != 0])


def test_quantize_is_idempotent_on_dequantised_weights():
    """write-back makes the bf16 weights the dequantised model; quantising those again must give the same model (a row whose largest byte
    rounded down to 224 gets half the scale and 448 the second time: other bytes, the same values)"""
    from visper_lm_amd import quant
    for w in _matrices()[:2]:
        q, s = quant.quantize_rows_pow2(w)
        q2, s2 = quant.quantize_rows_pow2(quant.dequantize(q, s).to(BF16))
        assert ((s2 == s) | (s2 == s / 2)).all()
        assert torch.equal(quant.dequantize(q2, s2), quant.dequantize(q, s))


def test_w8_entry_points_reject_bad_arguments():
    from visper_lm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vp_last_error_string()
    p = ctypes.c_void_p(16)                                           # never dereferenced: every call below fails its checks first
    eps = ctypes.c_float(1e-5)
    w8 = lambda M, N, K, A=p, W=p, S=p, epi=0, ws=None: lib.vp_decode_gemm_w8(M, N, K, A, K, W, K, S, p, N, None, 0, None, eps, epi, 0, ws, None)
    bf = lambda M, N, K, A=p, W=p, epi=0, ws=None: lib.vp_decode_gemm(M, N, K, A, K, W, K, p, N, None, 0, None, eps, epi, 0, ws, None)
    assert bf(17, 64, 64) == w8(17, 64, 64) == -2 and b"vp_decode_gemm_w8" in err() and b"M = 17" in err()
    assert w8(0, 64, 64) == bf(0, 64, 64) == -2
    assert w8(1, 64, 64, A=None) == bf(1, 64, 64, A=None) == -1
    assert w8(1, 64, 64, S=None) == -1 and b"w_scale" in err()       # a null scale is a null operand
    assert w8(1, 64, 72) == -2 and b"multiples of 16" in err()        # K % 16 (the bf16 sibling: K % 8 -> the same code)
    assert w8(1, 64, 60) == bf(1, 64, 60) == -2
    assert w8(1, 40, 64, epi=4) == bf(1, 40, 64, epi=4) == -2         # SwiGLU with N % 16 != 0
    assert w8(1, 64, 64, epi=9) == bf(1, 64, 64, epi=9) == -1
    assert bf(1, 4096, 4096) == w8(1, 4096, 4096) == -1 and b"workspace" in err()          # split-K shape without workspace
    # the workspace query is a pure function of the shape
    q = lib.vp_decode_gemm_w8_workspace_bytes
    assert q(1, 4096, 4096, 0) > 0 and q(1, 128256, 4096, 0) == 0 and q(0, 64, 64, 0) == 0
    for args in ((1, 4096, 4096, 0), (8, 6144, 4096, 0), (16, 28672, 4096, 4), (3, 4096, 14336, 0), (1, 128, 256, 5)):
        assert q(*args) == q(*args)
        assert q(*args) % (args[0] * args[1] * 4) == 0                # whole fp32 slabs [ks][M][N]
    # quantiser: null pointers, ld < K
    qr = lib.vp_quant_rows_e4m3
    assert qr(4, 64, None, 64, p, 64, p, 0, None) == -1 and b"vp_quant_rows_e4m3" in err()
    assert qr(4, 64, p, 64, None, 64, p, 0, None) == -1
    assert qr(4, 64, p, 64, p, 64, None, 0, None) == -1
    assert qr(4, 64, p, 48, p, 64, p, 0, None) == -1 and b"ld >= K" in err()
    assert qr(4, 64, p, 64, p, 48, p, 1, None) == -1
    assert qr(0, 64, p, 64, p, 64, p, 0, None) == -1


def test_w8_kernels_use_no_scratch_and_do_not_spill():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    import kernel_resources as kr
    so = os.path.join(os.path.dirname(__file__), "..", "visper-lm_amd", "libvisper_hip.so")
    assert os.path.exists(so), "library not built"
    res = kr.matching(so, ("decode_gemm_w8_kernel", "decode_gemm_combine_kernel", "quant_rows_e4m3_kernel"))
    assert len(res) == 4, sorted(res)                                 # <true> / <false> norm prologue, the combine, the quantiser
    for n, d in res.items():
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (n, d)
    for n, d in res.items():
        if "decode_gemm_w8_kernel" in n:
            assert d["vgpr_count"] + d.get("agpr_count", 0) <= 256, (n, d)      # at least 2 blocks of 4 waves per CU


def _cpu_model(cls_name):
    from oracle import cases
    from visper_lm_amd import model as M
    arch = "phi3" if "Phi3" in cls_name else "llama"
    ocfg, W, batch, g = cases.tiny_llama_case(arch)
    cfg_cls = {"OlaLlavaLlamaForCausalLM": M.OlaLlavaLlamaConfig, "LlavaLlamaForCausalLM": M.LlavaConfig,
               "OlaLlavaPhi3ForCausalLM": M.OlaLlavaPhi3Config, "LlavaPhi3ForCausalLM": M.LlavaPhi3Config}[cls_name]
    return getattr(M, cls_name)(cfg_cls(**vars(ocfg)), device="cpu", init="empty"), batch


@pytest.mark.parametrize("cls_name", ["OlaLlavaLlamaForCausalLM", "LlavaLlamaForCausalLM", "OlaLlavaPhi3ForCausalLM", "LlavaPhi3ForCausalLM"])
def test_mirrors_have_quantize_for_generation_and_keep_their_refusals(cls_name):
    import inspect
    model, batch = _cpu_model(cls_name)
    assert callable(getattr(model, "quantize_for_generation"))
    sig = inspect.signature(model.quantize_for_generation)
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
            model.quantize_for_generation()


def test_ops_route_and_quant_module_import_without_a_device():
    import inspect
    from visper_lm_amd import ops, quant
    assert "w_scale" in inspect.signature(ops.decode_gemm).parameters
    assert inspect.signature(ops.decode_gemm).parameters["w_scale"].default is None
    assert list(inspect.signature(ops.quant_rows_e4m3).parameters) == ["w", "writeback"]
    assert quant.E4M3_MAX == 448.0
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.quant_rows_e4m3(torch.zeros(8, 16, dtype=BF16))
