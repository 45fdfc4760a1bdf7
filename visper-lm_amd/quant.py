"""FP8 and MXFP4 weight-only decoding and the FP8 KV cache: the format contracts, and their plain-torch CPU references (host-only: importable
without a GPU, no kernels).  The FP8 contract comes first; the MXFP4 contract and the KV cache's are documented above their functions, further down.

The reference loads a checkpoint for evaluation with `load_pretrained_model(..., load_8bit=..., load_4bit=...)` (ola_vlm/model/builder.py:26-34),
which goes through bitsandbytes.  That route does not exist on this part; what gfx950 has natively is OCP FP8, so `generate()` can stream its
decoder weights as e4m3fn bytes instead of bf16 (Engine.quantize_decoder, model.quantize_for_generation).

The contract (vp_quant_rows_e4m3 computes exactly this on the device, vp_decode_gemm_w8 consumes it):

  * format   OCP `e4m3fn` (torch.float8_e4m3fn; NOT the MI300 `fnuz` encoding), one byte per weight, stored as uint8 [N, K].
  * scale    one fp32 per weight ROW, a power of two: s = 2^ceil(log2(absmax / 448)), i.e. the smallest power of two that brings the row's
             largest magnitude into (224, 448].  Rows of zeros get s = 1.  The scale travels with the row, so row permutations (interleaved
             gate|up, [gate | up] halves) and column scalings done before quantisation (fold_norm) need no special handling.
  * rounding q = e4m3fn(w / s), to nearest, ties to even; w / s is exact (division by a power of two), nothing saturates, no NaN byte.
  * exact    q * s is a 4-bit significand times a power of two: exactly representable in bf16.  Written back over the bf16 weight, it makes the
             bf16 kernels and the FP8 decode path compute the SAME mathematical model: every bound the project holds for decoding applies to
             the FP8 path unchanged, and prefill / training forward / logits_of see the weights generate() decodes with.
  * product  the GEMM keeps the activation in bf16, converts the bytes to bf16 in registers (exact), accumulates in fp32 and multiplies row n's
             accumulator by s[n] in fp32 before any rounding point of its epilogue (for SwiGLU: gate and up sums each by their own scale).
  * range    weights are finite; a row whose absmax lies in bf16's topmost binade (>= 2^127) can round up to 2^128, which bf16 does not hold:
             such rows are outside the contract (no weight is within 30 orders of magnitude of them).
  * error    |w - q s| <= 2^-4 |w| where the SCALED value lies in e4m3's normal range, |w / s| >= 2^-6 (half an ulp of a 3-bit mantissa; the
             worst case is 1/17, a tie just above a power of two); below it (|w / s| < 2^-6) the absolute error is at most half the subnormal
             spacing, 2^-10 s — also for a value just below 2^-6 that rounds UP to the first normal byte (up to 1/15 of itself).
  * absmax   the scaled row's absmax lies in (224, 448]; after rounding the largest byte lies in [224, 448] (a scaled absmax in (224, 232]
             rounds down to 224 on e4m3's grid, whose spacing is 16 there).
"""
from __future__ import annotations

import torch

E4M3_MAX = 448.0
E4M3_MIN_NORMAL = 2.0 ** -6
E4M3_SUBNORMAL_STEP = 2.0 ** -9


def row_scales_pow2(w):
    """fp32 [N]: per-row power-of-two scale of a [N, K] matrix (see the module docstring)."""
    a = w.detach().abs().amax(dim=1).double()
    m, e = torch.frexp(a)                                       # a = m 2^e, m in [0.5, 1): exact in float64 for bf16 subnormals as well
    se = e.to(torch.int64) - 9 + (m > 0.875).to(torch.int64)   # 448 = 0.875 * 2^9
    s = torch.ldexp(torch.ones_like(a), se)
    return torch.where(a == 0, torch.ones_like(s), s).float()   # 2^-141 .. 2^120: fp32 holds every one (subnormal below 2^-126)


def quantize_rows_pow2(w_bf16):
    """bf16 [N, K] -> (q uint8 [N, K] of e4m3fn bytes, scale fp32 [N]) on the CPU."""
    assert w_bf16.dim() == 2 and w_bf16.dtype == torch.bfloat16, (w_bf16.shape, w_bf16.dtype)
    w = w_bf16.detach().cpu()
    s = row_scales_pow2(w)
    t = (w.double() / s.double()[:, None]).float()              # exact: |t| <= 448, a bf16 significand
    q = t.to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s


def dequantize(q, scale):
    """fp32 [N, K] = e4m3fn(q) * scale[:, None] (exact; every value is representable in bf16)."""
    v = q.detach().cpu().view(torch.float8_e4m3fn).to(torch.float32).double()
    return (v * scale.detach().cpu().double()[:, None]).float()


# ------------------------------------------------------------------------------------------------ MXFP4 (4-bit weight-only decoding)
# The 4-bit half of the reference's load_8bit / load_4bit: OCP MXFP4, which gfx950 converts to bf16 natively with the block scale applied by
# the conversion itself.  The contract (vp_quant_blocks_mxfp4 computes exactly this on the device through the integer arithmetic of
# csrc/mxfp4.h, vp_decode_gemm_w4 consumes it):
#
#   * elements OCP e2m1: codes 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 is the sign.  Two codes per byte: element k of a row lives in byte
#              k // 2, even k in the low nibble.  Stored as uint8 [N, K/2], row-major.
#   * blocks   32 consecutive k of one row (K % 32 == 0); one e8m0 byte per block, uint8 [N, K/32], scale 2^(byte - 127).
#   * scale    the smallest power of two with absmax / s <= 6: the block's largest magnitude lands in (3, 6], nothing saturates.  The exponent
#              is clamped below at -120, so every nonzero dequantised value is a normal bf16 number (>= 2^-121) and neither the conversion
#              nor the MFMA depends on a denormal mode; a clamped block's values may all round to zero.  A block of zeros gets byte 127.
#   * range    weights are finite.  Below bf16's topmost binade (|w| < 2^127) the byte is at most 252 and q * s is exact; a block whose absmax
#              lies in [2^127, 2^128) gets byte 252 or 253 and can round up to 6 * 2^126, which bf16 does not hold: outside the contract,
#              as for e4m3.
#   * rounding w / s is exact; round to nearest on the e2m1 grid, ties to the even code.  The sign bit is the weight's sign bit, also where the
#              value rounds to zero.
#   * exact    q * s is a 2-bit significand times a power of two: exactly representable in bf16, so write-back makes the bf16 weights the
#              dequantised model, as for e4m3.
#   * error    block-wise |w - q s| <= s * step / 2 with step 0.5 for |w / s| < 2, 1 for < 4, 2 above.
#   * again    quantising the dequantised weights again gives the same VALUES: a scale halves when the block's largest code rounded down to
#              3, and a block that rounded to all zeros gets byte 127.
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MXFP4_BLOCK = 32
MXFP4_MIN_SCALE_EXP = -120
_E2M1_CODE_OF_HALVES = (0, 1, 2, 3, 4, -1, 5, -1, 6, -1, -1, -1, 7)     # code of a grid value given in units of 0.5


def block_scale_exps_mxfp4(w):
    """int64 [N, K/32]: exponent se of every block's power-of-two scale (the e8m0 byte is se + 127)."""
    N, K = w.shape
    assert K % MXFP4_BLOCK == 0, K
    a = w.detach().abs().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK).amax(dim=2).double()
    m, e = torch.frexp(a)                                       # a = m 2^e, m in [0.5, 1): exact in float64 for bf16 subnormals as well
    se = e.to(torch.int64) - 3 + (m > 0.75).to(torch.int64)    # 6 = 0.75 * 2^3
    se = se.clamp(min=MXFP4_MIN_SCALE_EXP)
    return torch.where(a == 0, torch.zeros_like(se), se)


def quantize_blocks_mxfp4(w_bf16):
    """bf16 [N, K] -> (q uint8 [N, K/2] of packed e2m1 codes, e uint8 [N, K/32] of e8m0 scale bytes) on the CPU."""
    assert w_bf16.dim() == 2 and w_bf16.dtype == torch.bfloat16, (w_bf16.shape, w_bf16.dtype)
    w = w_bf16.detach().cpu()
    N, K = w.shape
    se = block_scale_exps_mxfp4(w)
    s = torch.ldexp(torch.ones_like(se, dtype=torch.float64), se)
    t = (w.double().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK) / s[:, :, None]).view(N, K)      # exact: |t| <= 6
    at = t.abs()
    step = torch.where(at < 2, 0.5, torch.where(at < 4, 1.0, 2.0)).double()
    r = torch.round(at / step) * step                           # half to even: the even multiple of the step is the even code
    code = torch.tensor(_E2M1_CODE_OF_HALVES, dtype=torch.int64)[(r * 2).to(torch.int64)]
    assert (code >= 0).all()
    code = code | (torch.signbit(w).to(torch.int64) << 3)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    return q.contiguous(), (se + 127).to(torch.uint8)


def dequantize_mxfp4(q, e):
    """fp32 [N, K] = e2m1(q) * 2^(e - 127) per block (exact; every value is representable in bf16)."""
    q, e = q.detach().cpu(), e.detach().cpu()
    N, K = q.shape[0], q.shape[1] * 2
    code = torch.stack([q & 0xf, q >> 4], dim=2).view(N, K).to(torch.int64)
    v = torch.tensor(E2M1_VALUES, dtype=torch.float64)[code & 7]
    v = torch.where((code & 8) != 0, -v, v)
    s = torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e.to(torch.int64) - 127)
    return (v.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * s[:, :, None]).view(N, K).float()


# ------------------------------------------------------------------------------------------------ FP8 KV cache (e4m3 per (token, KV head))
# The third member of the family: after the weights, the KV cache is what a decode step reads (at B = 8 far more than the 4-bit weights), and
# it caps batch and context length.  `generate(..., kv_cache_dtype="fp8_e4m3")` keeps it in 8 bits.  The contract (vp_quant_kv_e4m3 and
# vp_decode_rope_append_kv8 compute exactly this on the device through the integer arithmetic of csrc/fp8_e4m3.h, vp_decode_attn_kv8
# consumes it):
#
#   * unit     the D elements of one (token, KV head) of K form one row; the same holds for V.
#   * format   the e4m3 ROW contract above with row length D: OCP `e4m3fn` bytes, one fp32 power-of-two scale per (token, head),
#              s = 2^ceil(log2(absmax / 448)); a zero head gets s = 1; round to nearest even; nothing saturates; no NaN byte.
#   * K        is quantised AFTER RoPE: the rotated bf16 row the bf16 cache would have stored is what gets quantised.  V as projected.
#   * storage  per layer bytes uint8 [B, Smax, 2*Hkv*D] (token row = k heads | v heads, the bf16 cache's layout) and scales fp32
#              [B, Smax, 2*Hkv] (k scales | v scales): (D + 4) / 2D of the bf16 cache, 0.516 at D = 128 and 0.521 at D = 96.
#   * exact    q * s is a bf16 number, so a bf16 cache holding the dequantised rows ("fp8_e4m3_emulated") read by the bf16 attention kernel
#              is the SAME mathematical model as the byte cache read by vp_decode_attn_kv8: the decode path's own bounds compare the two.
#   * product  the attention keeps q in bf16, converts the bytes in registers (exact), multiplies a key's finished fp32 dot product by its
#              scale and a value row's softmax weight by its scale (exact power-of-two products in fp32).
#   * error    per element as for the rows contract: |x - q s| <= 2^-4 |x| in the scaled normal range, 2^-10 s below it.
def quantize_kv_heads(x_bf16, Hkv, D):
    """bf16 [n, Hkv*D] (the k heads, or the v heads, of n tokens) -> (q uint8 [n, Hkv*D], scale fp32 [n, Hkv]) on the CPU: quantize_rows_pow2
    on the [n*Hkv, D] view."""
    assert x_bf16.dim() == 2 and x_bf16.shape[1] == Hkv * D, (x_bf16.shape, Hkv, D)
    n = x_bf16.shape[0]
    q, s = quantize_rows_pow2(x_bf16.detach().cpu().reshape(n * Hkv, D))
    return q.view(n, Hkv * D), s.view(n, Hkv)


def dequantize_kv_heads(q, s, Hkv, D):
    """fp32 [n, Hkv*D] = e4m3fn(q) * s per (token, head) (exact; every value is representable in bf16): dequantize on the [n*Hkv, D] view."""
    n = q.shape[0]
    assert q.shape[1] == Hkv * D and tuple(s.shape) == (n, Hkv), (q.shape, s.shape, Hkv, D)
    return dequantize(q.detach().cpu().reshape(n * Hkv, D), s.detach().cpu().reshape(n * Hkv)).view(n, Hkv * D)
