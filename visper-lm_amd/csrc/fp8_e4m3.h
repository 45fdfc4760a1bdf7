// OCP FP8 e4m3fn (1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, S.1111.111 = NaN, largest finite 448) with per-row
// power-of-two scales: the weight format of the FP8 weight-only decode path (vp_quant_rows_e4m3 / vp_decode_gemm_w8).
// Everything here is integer arithmetic on the bit patterns, so quantisation and write-back are exact, independent of the float
// mode of the unit that runs them (denormal flushing, fast-math), and the same on the host and on the device.
//   scale   s = 2^se, the smallest power of two with absmax / s <= 448: the row's largest magnitude lands in (224, 448]
//   quantise q = e4m3fn(w / s), round to nearest, ties to even (what torch's .to(torch.float8_e4m3fn) does); never NaN, never saturates
//   dequant  bf16(q * s): exact (a 4-bit significand times a power of two; rows of bf16 subnormals stay on the bf16 subnormal grid)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VP_HD __host__ __device__ __forceinline__
#else
#define VP_HD inline
#endif

VP_HD int vp_top_bit(uint64_t x) { return 63 - __builtin_clzll(x); }                 // x != 0

// exponent se of the row scale from the row's absmax (bf16 bits, sign cleared, finite); absmax == 0 -> 0 (scale 1)
VP_HD int vp_e4m3_scale_exp(uint32_t amax_bits) {
  const int E = (int)(amax_bits >> 7) & 0xff, M = (int)amax_bits & 0x7f;
  if (E == 0 && M == 0) return 0;
  int sig, ea;                                                   // absmax = sig / 128 * 2^ea, sig in [128, 256)
  if (E) { sig = 128 | M; ea = E - 127; }
  else { const int p = vp_top_bit((uint64_t)M); sig = M << (7 - p); ea = p - 133; }
  return ea - 8 + (sig > 224 ? 1 : 0);                           // 448 = 1.75 * 2^8 = 224 / 128 * 2^8
}

// 2^se as fp32 bits (se in [-141, 120]: subnormal fp32 below -126)
VP_HD uint32_t vp_pow2_f32_bits(int se) { return se >= -126 ? (uint32_t)(se + 127) << 23 : 1u << (se + 149); }

// e4m3fn byte of w / 2^se (w: bf16 bits, finite, |w| / 2^se <= 448)
VP_HD uint8_t vp_e4m3_quant(uint32_t w_bits, int se) {
  const uint32_t sign = (w_bits >> 8) & 0x80;
  const int E = (int)(w_bits >> 7) & 0xff, M = (int)w_bits & 0x7f;
  const int sig = E ? (128 | M) : M;                             // |w| = sig * 2^(max(E, 1) - 134)
  if (sig == 0) return (uint8_t)sign;
  const int d = (E ? E : 1) - 134 - se + 9 + 40;                 // |w| / s in units of 2^-9 (the e4m3 subnormal spacing), 40 fraction bits kept
  if (d < 0) return (uint8_t)sign;                               // below 2^-32 units: rounds to zero
  const uint64_t z = (uint64_t)sig << d;                         // < 2^58 (|w| / s <= 448 = 229376 units)
  const int p = vp_top_bit(z);
  const int drop = p - 40 >= 3 ? p - 3 : 40;                     // normals keep 4 significant bits, subnormals the integer part
  uint64_t n = z >> drop;
  const uint64_t rem = z & (((uint64_t)1 << drop) - 1), half = (uint64_t)1 << (drop - 1);
  n += (rem > half || (rem == half && (n & 1))) ? 1 : 0;
  // subnormal range: n in 0..8 is the byte itself (8 = the first normal); normal: n in 8..16, exponent field drop - 39, a carry to 16 moves up one
  const uint32_t mag = drop == 40 ? (uint32_t)n : (uint32_t)(((drop - 39) << 3) + (int)n - 8);
  return (uint8_t)(sign | mag);
}

// bf16 bits of q * 2^se (exact)
VP_HD uint16_t vp_e4m3_dequant_bf16(uint32_t q, int se) {
  const uint32_t sign = (q & 0x80) << 8;
  const int e = (int)(q >> 3) & 0xf, m = (int)q & 7;
  const int sig = e ? (8 | m) : m;                               // |q| = sig * 2^(max(e, 1) - 10)
  if (sig == 0) return (uint16_t)sign;
  const int ex = (e ? e : 1) - 10 + se;
  const int p = vp_top_bit((uint64_t)sig);
  const int Eb = p + ex + 127;
  if (Eb >= 1) return (uint16_t)(sign | (uint32_t)(Eb << 7) | (uint32_t)((sig << (7 - p)) & 0x7f));
  const int sh = ex + 133;                                       // bf16 subnormal: units of 2^-133
  return (uint16_t)(sign | (uint32_t)(sh >= 0 ? sig << sh : sig >> -sh));
}
