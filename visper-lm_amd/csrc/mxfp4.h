// OCP MXFP4: e2m1 elements (1 sign, 2 exponent (bias 1), 1 mantissa bit: codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 = sign) in blocks of
// 32 consecutive k of one row, one e8m0 scale byte per block (scale 2^(byte - 127)): the weight format of the 4-bit weight-only decode path
// (vp_quant_blocks_mxfp4 / vp_decode_gemm_w4).  Two codes per byte, element k in byte k / 2, even k in the low nibble.
// Everything here is integer arithmetic on the bit patterns, so quantisation and write-back are exact, independent of the float mode of the
// unit that runs them (denormal flushing, fast-math), and the same on the host and on the device.
//   scale    s = 2^se, the smallest power of two with absmax / s <= 6: the block's largest magnitude lands in (3, 6]; se is clamped below at
//            -120 (every nonzero dequantised value is then a normal bf16 number: 0.5 * 2^-120 = 2^-121); a block of zeros has se = 0
//   quantise code = e2m1(w / s), round to nearest, ties to the even code; never saturates; the sign bit is the weight's, also on a zero
//   dequant  bf16(code * s): exact (a 2-bit significand times a power of two)
#pragma once
#include <stdint.h>

#include "fp8_e4m3.h"  // VP_HD, vp_top_bit

#define VP_MXFP4_BLOCK 32
#define VP_MXFP4_MIN_SCALE_EXP (-120)

// exponent se of the block scale from the block's absmax (bf16 bits, sign cleared, finite); the scale byte is se + 127
VP_HD int vp_mxfp4_scale_exp(uint32_t amax_bits) {
  const int E = (int)(amax_bits >> 7) & 0xff, M = (int)amax_bits & 0x7f;
  if (E == 0 && M == 0) return 0;
  int sig, ea;                                                   // absmax = sig / 128 * 2^ea, sig in [128, 256)
  if (E) { sig = 128 | M; ea = E - 127; }
  else { const int p = vp_top_bit((uint64_t)M); sig = M << (7 - p); ea = p - 133; }
  const int se = ea - 2 + (sig > 192 ? 1 : 0);                   // 6 = 1.5 * 2^2 = 192 / 128 * 2^2
  return se < VP_MXFP4_MIN_SCALE_EXP ? VP_MXFP4_MIN_SCALE_EXP : se;
}

// e2m1 code (4 bits) of w / 2^se (w: bf16 bits, finite, |w| / 2^se <= 6)
VP_HD uint32_t vp_mxfp4_quant(uint32_t w_bits, int se) {
  const uint32_t sign = (w_bits >> 12) & 0x8;
  const int E = (int)(w_bits >> 7) & 0xff, M = (int)w_bits & 0x7f;
  const int sig = E ? (128 | M) : M;                             // |w| = sig * 2^(max(E, 1) - 134)
  if (sig == 0) return sign;
  const int d = (E ? E : 1) - 134 - se + 1 + 40;                 // |w| / s in units of 0.5 (the e2m1 subnormal spacing), 40 fraction bits kept
  if (d < 0) return sign;                                        // below 2^-32 units: rounds to zero
  const uint64_t z = (uint64_t)sig << d;                         // < 2^44 (|w| / s <= 6 = 12 units)
  const int p = vp_top_bit(z);
  const int drop = p - 40 >= 1 ? p - 1 : 40;                     // normals keep 2 significant bits, the subnormal range the integer part
  uint64_t n = z >> drop;
  const uint64_t rem = z & (((uint64_t)1 << drop) - 1), half = (uint64_t)1 << (drop - 1);
  n += (rem > half || (rem == half && (n & 1))) ? 1 : 0;
  // drop == 40: n in 0..4 is the code itself (units of 0.5 up to 2.0); above: n in 2..4, exponent field drop - 39, a carry to 4 moves up one
  const uint32_t mag = drop == 40 ? (uint32_t)n : (uint32_t)(((drop - 39) << 1) + (int)n - 2);
  return sign | mag;
}

// bf16 bits of code * 2^se (exact; se >= -120: a normal number whenever it is nonzero)
VP_HD uint16_t vp_mxfp4_dequant_bf16(uint32_t code, int se) {
  const uint32_t sign = (code & 0x8) << 12;
  const int e = (int)(code >> 1) & 3, m = (int)code & 1;
  if (e == 0 && m == 0) return (uint16_t)sign;
  const int Eb = (e ? e - 1 : -1) + se + 127;                    // 0.5 = 2^-1; (1 + m / 2) * 2^(e - 1)
  return (uint16_t)(sign | (uint32_t)(Eb << 7) | (uint32_t)(e ? m << 6 : 0));
}
