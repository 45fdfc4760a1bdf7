"""FP8 weight-only decoding: the format contract, and its plain-torch CPU reference (host-only: importable without a GPU, no kernels).

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
