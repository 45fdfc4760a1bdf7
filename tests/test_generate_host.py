"""generate() without a GPU: HF's sampling semantics, the decode entry points' argument checks (the library loads without a device) and
the options generate() refuses."""
import ctypes

import pytest
import torch


def test_temperature_top_p_match_hf_warpers():
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopPLogitsWarper
    from visper_lm_amd.decode import warp_logits
    g = torch.Generator().manual_seed(0)
    for B, V in ((1, 17), (4, 1000), (3, 32064)):
        logits = torch.randn(B, V, generator=g) * 4
        ids = torch.zeros(B, 1, dtype=torch.long)
        for temp, top_p in ((1.0, 1.0), (0.7, 1.0), (1.0, 0.9), (0.2, 0.5), (1.3, 0.05), (0.9, 1e-6)):
            want = logits
            if temp != 1.0:
                want = TemperatureLogitsWarper(temp)(ids, want)
            if top_p < 1.0:
                want = TopPLogitsWarper(top_p, min_tokens_to_keep=1)(ids, want)
            got = warp_logits(logits, temp, top_p)
            assert torch.equal(torch.isinf(got), torch.isinf(want)), (B, V, temp, top_p)
            fin = ~torch.isinf(want)
            assert torch.equal(got[fin], want[fin]), (B, V, temp, top_p)
            assert (fin.sum(-1) >= 1).all()


def test_greedy_is_argmax_with_torch_tie_breaking():
    from visper_lm_amd.decode import next_tokens
    x = torch.tensor([[0.0, 3.0, 3.0, 1.0], [5.0, 5.0, 5.0, 5.0]])
    assert next_tokens(x).tolist() == torch.argmax(x, -1).tolist()


def test_decode_entry_points_reject_bad_arguments():
    from visper_lm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vp_last_error_string()
    p = ctypes.c_void_p(16)                                           # never dereferenced: every call below fails its checks first
    # skinny GEMM: M > 16, M = 0, null operands, K not a multiple of 8, SwiGLU with N % 16 != 0, split-K shape without workspace
    assert lib.vp_decode_gemm(17, 64, 64, p, 64, p, 64, p, 64, None, 0, None, ctypes.c_float(1e-5), 0, 0, None, None) == -2
    assert b"vp_decode_gemm" in err() and b"M = 17" in err()
    assert lib.vp_decode_gemm(0, 64, 64, p, 64, p, 64, p, 64, None, 0, None, ctypes.c_float(1e-5), 0, 0, None, None) == -2
    assert lib.vp_decode_gemm(1, 64, 64, None, 64, p, 64, p, 64, None, 0, None, ctypes.c_float(1e-5), 0, 0, None, None) == -1
    assert lib.vp_decode_gemm(1, 64, 60, p, 64, p, 64, p, 64, None, 0, None, ctypes.c_float(1e-5), 0, 0, None, None) == -2
    assert lib.vp_decode_gemm(1, 40, 64, p, 64, p, 64, p, 64, None, 0, None, ctypes.c_float(1e-5), 4, 0, None, None) == -2
    assert lib.vp_decode_gemm(1, 64, 64, p, 64, p, 64, p, 64, None, 0, None, ctypes.c_float(1e-5), 9, 0, None, None) == -1
    assert lib.vp_decode_gemm_workspace_bytes(1, 4096, 4096, 0) > 0                 # 256 tiles: K split over blocks
    assert lib.vp_decode_gemm_workspace_bytes(1, 128256, 4096, 0) == 0              # lm_head fills the chip by N alone
    assert lib.vp_decode_gemm(1, 4096, 4096, p, 4096, p, 4096, p, 4096, None, 0, None, ctypes.c_float(1e-5), 0, 0, None, None) == -1
    assert b"workspace" in err()
    # attention: unsupported head_dim, group size, too few splits for Smax, null workspace
    args = lambda B, Hq, Hkv, D, Smax, ns, ws: (B, Hq, Hkv, D, Smax, p, Hq * D, p, Smax * Hkv * D, Hkv * D, p, Smax * Hkv * D, Hkv * D,
                                                 p, Hq * D, p, 0, ctypes.c_float(0.1), ns, ws, None)
    assert lib.vp_decode_attn(*args(1, 32, 8, 80, 64, 1, p)) == -2 and b"head_dim 80" in err()
    assert lib.vp_decode_attn(*args(1, 24, 8, 128, 64, 1, p)) == -2
    assert lib.vp_decode_attn(*args(1, 32, 8, 128, 8192, 4, p)) == -2 and b"nsplit" in err()
    assert lib.vp_decode_attn(*args(1, 32, 8, 128, 64, 1, None)) == -1 and b"workspace" in err()
    assert lib.vp_decode_attn_workspace_bytes(2, 32, 8, 128, 16) == 2 * 32 * 16 * 130 * 4
    # rope + append: head_dim not a multiple of 16, null position array
    assert lib.vp_decode_rope_append(1, 4, 2, 40, p, 256, p, 160, p, 0, 80, p, 0, 80, p, p, p, 8, None) == -2
    assert lib.vp_decode_rope_append(1, 4, 2, 32, p, 256, p, 128, p, 0, 64, p, 0, 64, p, p, None, 8, None) == -1
    assert lib.vp_add_i32(0, p, 1, None) == -1


def _cpu_model(cls_name="OlaLlavaLlamaForCausalLM"):
    from oracle import cases
    from visper_lm_amd import model as M
    ocfg, W, batch, g = cases.tiny_llama_case()
    cfg_cls = {"OlaLlavaLlamaForCausalLM": M.OlaLlavaLlamaConfig, "LlavaLlamaForCausalLM": M.LlavaConfig}[cls_name]
    return getattr(M, cls_name)(cfg_cls(**vars(ocfg)), device="cpu", init="empty"), batch


@pytest.mark.parametrize("cls_name", ["OlaLlavaLlamaForCausalLM", "LlavaLlamaForCausalLM"])
def test_generate_refuses_unbuilt_options(cls_name):
    model, batch = _cpu_model(cls_name)
    ids = batch["input_ids"][:1]
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(ids, num_beams=4)
    with pytest.raises(NotImplementedError, match="output_scores"):
        model.generate(ids, output_scores=True)
    with pytest.raises(NotImplementedError, match="return_dict_in_generate"):
        model.generate(ids, return_dict_in_generate=True)
    with pytest.raises(NotImplementedError, match="inputs_embeds"):
        model.generate(ids, inputs_embeds=torch.zeros(1, 3, 128))
    with pytest.raises(NotImplementedError, match="out of scope"):                # forward keeps refusing incremental decoding
        model(input_ids=ids, use_cache=True)
