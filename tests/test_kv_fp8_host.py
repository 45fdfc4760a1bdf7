"""The FP8 KV cache without a GPU: the per-(token, head) wrappers against the e4m3 rows contract (quant.py), the cache's size, the names
generate() accepts for `kv_cache_dtype`, and the argument checks of the three entry points (the library loads without a device)."""
import ctypes

import pytest
import torch

BF16 = torch.bfloat16


def _heads(n, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, Hkv, D, generator=g) * torch.exp2(torch.randint(-6, 7, (n, Hkv, 1), generator=g).float())
    x = x.to(BF16)
    x[1, 0] = 0                                                        # a zero head: scale 1
    x[2, Hkv - 1, D // 3] = 3.0e4                                       # one outlier decides the head's scale
    x[3, 0] = torch.randint(0, 128, (D,), generator=g).to(torch.int16).view(BF16)      # a head of bf16 subnormals
    x[3, 0, 1] = -x[3, 0, 1]
    return x.reshape(n, Hkv * D)


@pytest.mark.parametrize("D", [32, 96, 128])
def test_kv_head_wrappers_equal_the_rows_contract(D):
    from visper_lm_amd import quant
    n, Hkv = 9, 3
    x = _heads(n, Hkv, D, D)
    q, s = quant.quantize_kv_heads(x, Hkv, D)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (n, Hkv * D) and s.dtype == torch.float32 and tuple(s.shape) == (n, Hkv)
    qr, sr = quant.quantize_rows_pow2(x.reshape(n * Hkv, D))
    assert torch.equal(q.reshape(n * Hkv, D), qr) and torch.equal(s.reshape(-1), sr)
    assert float(s[1, 0]) == 1.0 and not q[1, :D].any()                # the zero head
    assert float(s[2, Hkv - 1]) == 2.0 ** 7                            # 3e4 / 448 = 66.96 -> 2^7
    assert float(s[3, 0]) < 2.0 ** -126                                # subnormal head: a subnormal fp32 scale
    assert not ((q & 0x7f) == 0x7f).any()                              # no NaN byte
    d = quant.dequantize_kv_heads(q, s, Hkv, D)
    assert tuple(d.shape) == (n, Hkv * D)
    assert torch.equal(d, quant.dequantize(qr, sr).view(n, Hkv * D))
    assert torch.equal(d.to(BF16).float(), d)                          # every dequantised value is a bf16 number
    # the scaled absmax of every nonzero head lies in (224, 448]: nothing saturates
    am = x.float().view(n, Hkv, D).abs().amax(-1).double() / s.double()
    nz = am > 0
    assert (am[nz] > 224).all() and (am[nz] <= 448).all()
    # quantising the dequantised rows again reproduces the values (the emulated cache is a fixed point)
    q2, s2 = quant.quantize_kv_heads(d.to(BF16), Hkv, D)
    assert torch.equal(quant.dequantize_kv_heads(q2, s2, Hkv, D), d)


def test_kv_cache_size():
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.decode import KVCache
    for arch in ("llama", "phi3"):
        ocfg, *_ = cases.tiny_llama_case(arch)
        cfg = VisperConfig(**vars(ocfg))
        L, Hkv, D = cfg.num_hidden_layers, cfg.num_key_value_heads, cfg.head_dim
        B, Smax = 3, 41
        c8 = KVCache(cfg, B, Smax, "cpu", dtype="fp8_e4m3")
        cb = KVCache(cfg, B, Smax, "cpu")
        ce = KVCache(cfg, B, Smax, "cpu", dtype="fp8_e4m3_emulated")
        assert c8.nbytes == L * B * Smax * 2 * Hkv * (D + 4)
        assert cb.nbytes == ce.nbytes == L * B * Smax * 2 * Hkv * D * 2
        assert c8.nbytes * 2 * D == cb.nbytes * (D + 4)                # the ratio is (D + 4) / 2D exactly
        assert c8.dtype == "fp8_e4m3" and cb.dtype == "bf16" and cb.scales is None
        assert c8.k(0).dtype == torch.uint8 and tuple(c8.k(0).shape) == (B, Smax, Hkv, D) == tuple(c8.v(L - 1).shape)
        assert tuple(c8.k_scale(0).shape) == (B, Smax, Hkv) == tuple(c8.v_scale(0).shape) and c8.k_scale(0).dtype == torch.float32
        # views of the one buffer per layer: k heads | v heads, k scales | v scales
        c8.kv[0].zero_()
        c8.scales[0].zero_()
        c8.v(0)[1, 2, 0, 0] = 7
        c8.v_scale(0)[1, 2, 0] = 3.0
        assert int(c8.kv[0][1, 2, Hkv * D]) == 7 and float(c8.scales[0][1, 2, Hkv]) == 3.0
        assert cb.k(0).dtype == BF16 and ce.v(0).dtype == BF16


def test_kv_cache_dtype_names():
    from visper_lm_amd.decode import KV_CACHE_DTYPES, resolve_kv_cache_dtype
    assert resolve_kv_cache_dtype(None) == "bf16"
    for name in ("bf16", "fp8_e4m3", "fp8_e4m3_emulated"):
        assert resolve_kv_cache_dtype(name) == name and name in KV_CACHE_DTYPES
    for bad in ("int3", "fp8", "", 8):
        with pytest.raises(ValueError) as ei:
            resolve_kv_cache_dtype(bad)
        assert all(n in str(ei.value) for n in KV_CACHE_DTYPES)       # the message names the choices


def test_generate_refuses_an_unknown_kv_cache_dtype_on_the_host():
    from oracle import cases
    from visper_lm_amd import model as M
    ocfg, W, batch, g = cases.tiny_llama_case()
    for cls, cfg_cls in ((M.OlaLlavaLlamaForCausalLM, M.OlaLlavaLlamaConfig), (M.LlavaLlamaForCausalLM, M.LlavaConfig)):
        model = cls(cfg_cls(**vars(ocfg)), device="cpu", init="empty")
        with pytest.raises(ValueError, match="fp8_e4m3_emulated"):     # before the engine (which needs a GPU) is touched
            model.generate(batch["input_ids"][:1], kv_cache_dtype="int3")


def test_kv8_entry_points_reject_bad_arguments():
    from visper_lm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vp_last_error_string()
    p = ctypes.c_void_p(16)                                           # never dereferenced: every call below fails its checks first
    f = ctypes.c_float(0.1)
    # quantiser: no destination, bytes without scales, head_dim not a multiple of 8, a row stride below heads * D, no rows
    assert lib.vp_quant_kv_e4m3(4, 4, 32, p, 128, None, 0, None, 0, None, 0, None) == -1 and b"vp_quant_kv_e4m3" in err()
    assert lib.vp_quant_kv_e4m3(4, 4, 32, p, 128, p, 128, None, 4, None, 0, None) == -1
    assert lib.vp_quant_kv_e4m3(4, 4, 36, p, 144, p, 144, p, 4, None, 0, None) == -2 and b"head_dim 36" in err()
    assert lib.vp_quant_kv_e4m3(4, 4, 32, p, 120, p, 128, p, 4, None, 0, None) == -2
    assert lib.vp_quant_kv_e4m3(4, 4, 32, p, 128, None, 0, None, 0, p, 120, None) == -2
    assert lib.vp_quant_kv_e4m3(0, 4, 32, p, 128, p, 128, p, 4, None, 0, None) == -1
    # rope + append: k bytes without v bytes, no destination at all, head_dim not a multiple of 16, null position array
    ra = lambda D, kq, vq, ks, vs, kd, vd, pos: (1, 4, 2, D, p, 8 * D, p, 4 * D, kq, 0, 4 * D, vq, 0, 4 * D, ks, 0, 4, vs, 0, 4,
                                                  kd, 0, 4 * D, vd, 0, 4 * D, p, p, pos, 8, None)
    assert lib.vp_decode_rope_append_kv8(*ra(32, p, None, p, p, None, None, p)) == -1 and b"go together" in err()
    assert lib.vp_decode_rope_append_kv8(*ra(32, None, None, None, None, None, None, p)) == -1
    assert lib.vp_decode_rope_append_kv8(*ra(40, p, p, p, p, None, None, p)) == -2 and b"head_dim 40" in err()
    assert lib.vp_decode_rope_append_kv8(*ra(32, p, p, p, p, None, None, None)) == -1
    # attention: unsupported head_dim, group size, too few splits for Smax, null workspace, null scales, a byte stride that is no multiple of 16
    aa = lambda B, Hq, Hkv, D, Smax, ns, ws, ks=p, kts=None: (B, Hq, Hkv, D, Smax, p, Hq * D, p, Smax * 2 * Hkv * D,
                                                              2 * Hkv * D if kts is None else kts, ks, Smax * 2 * Hkv, 2 * Hkv, p,
                                                              Smax * 2 * Hkv * D, 2 * Hkv * D, p, Smax * 2 * Hkv, 2 * Hkv, p, Hq * D, p, 0, f,
                                                              ns, ws, None)
    assert lib.vp_decode_attn_kv8(*aa(1, 32, 8, 80, 64, 1, p)) == -2 and b"head_dim 80" in err()
    assert lib.vp_decode_attn_kv8(*aa(1, 24, 8, 128, 64, 1, p)) == -2
    assert lib.vp_decode_attn_kv8(*aa(1, 32, 8, 128, 8192, 4, p)) == -2 and b"nsplit" in err()
    assert lib.vp_decode_attn_kv8(*aa(1, 32, 8, 128, 64, 1, None)) == -1 and b"workspace" in err()
    assert lib.vp_decode_attn_kv8(*aa(1, 32, 8, 128, 64, 1, p, ks=None)) == -1
    assert lib.vp_decode_attn_kv8(*aa(1, 32, 8, 128, 64, 1, p, kts=2056)) == -2 and b"16 bytes" in err()
