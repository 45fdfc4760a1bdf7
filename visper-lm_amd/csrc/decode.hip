// Single-token decode kernels (KV-cached generation): the reference generates with HF's generation loop over `inputs_embeds`
// (base_ola_vlm.py:579-616, llava_llama.py:122; called by eval/model_cvbench_loader.py:127, model_mmstar_loader.py:125, demo.py:328).
// At one token per sequence every decoder GEMM has M = B <= 16 rows and is bound by the bytes of its weight, not by MFMA work:
//  - decode_gemm_kernel / decode_gemm_w8_kernel / decode_gemm_w4_kernel (bf16 | e4m3 rows | MXFP4 blocks of W): C[M,N] = epi(A[M,K] W[N,K]^T),
//    W streamed once straight into VGPRs (no LDS round trip), one 16-row W tile per block, the K range split over the block's 4 waves (and,
//    where N has too few tiles to fill the chip, over KS blocks: fp32 slabs in a caller-owned workspace, summed in a fixed order by
//    decode_gemm_combine_kernel).  Optional RMSNorm prologue (rstd of the <= 16 A rows computed by every block, gamma applied while A is
//    loaded: vp_rmsnorm_fwd's rounding points), epilogues: none (bf16 / fp32 out), + residual, SwiGLU (act written directly).  Each format
//    owns its chunk loop (hand-shaped loads, waits and registers); argument block, split rule, prologue, reduction, epilogue, combine and
//    the host side (dg_run) are one piece of code for the three.
//  - decode_gemm_wide_kernel / decode_gemm_w8_wide_kernel / decode_gemm_w4_wide_kernel: the same blocks for 17 <= M <= 64 rows: up to four
//    16-row A tiles per streamed W tile, every output row bit-equal to the kernels above on that row.
//  - decode_rope_append_kernel / decode_rope_append_kv8_kernel: rotate-half RoPE of q / k at per-sequence positions pos[b] (vp_rope's
//    rounding points), k / v appended to row pos[b] of the bf16 | e4m3 cache.
//  - the *_rows entry points of the append and attention kernels: the same kernels with a row map (cache_row[r] = the cache row that batch
//    row r writes and reads; the plain entry points pass none), so that the n + 1 rows of a prompt-lookup verify step each run the
//    one-token computation on their sequence's cache.  decode_accept_kernel: the acceptance rule and the next step's counters.
//  - decode_attn_split_kernel / decode_attn_split_kv8_kernel + decode_attn_combine_kernel: one query row per sequence, the Hq/Hkv heads of
//    a KV head share every K / V read, the key range split over `nsplit` blocks (fp32 softmax, log2 domain), combined in a fixed order.
//  - the quantisers that make the byte operands: quant_rows_e4m3_kernel, quant_blocks_mxfp4_kernel, quant_kv_e4m3_kernel.
#include "common.h"
#include "fp8_e4m3.h"
#include "mxfp4.h"

#define VP_EPI_NONE 0
#define VP_EPI_SWIGLU_IL 4      // SwiGLU on the interleaved gate|up rows (8 gate rows, 8 up rows, ...)
#define VP_EPI_SWIGLU_HALVES 5  // SwiGLU on [gate | up] row halves

static constexpr int DG_THREADS = 256;       // 4 waves
static constexpr int DG_KCHUNK = 256;        // K elements one wave consumes per iteration: 4 lane groups x 64
static constexpr int DG_TARGET_BLOCKS = 512; // grid the K split aims for (2 blocks per CU on 256 CUs)

// one argument block for the three weight formats: W = bf16 rows | e4m3fn bytes | packed e2m1 codes (ldw in elements | bytes | bytes)
struct DecGemmArgs {
  const bf16_t* A; const bf16_t* W; void* C; const bf16_t* res; const bf16_t* gamma;
  float* ws;
  int M, N, K, Kc, epi, out_f32, KS;
  long lda, ldw, ldc, ldr;
  float eps;
  const float* wscale;                       // W8: one fp32 scale per W row; null otherwise
  const uint8_t* E;                          // W4: e8m0 scale bytes [N, K / 32], row stride lde; null / 0 otherwise
  long lde;
};

// split-K factor: a pure function of the shape and of the format's chunk (K elements one wave consumes per iteration), so the workspace
// size query and the launch agree and results do not depend on the device
static int dg_ksplit(int N, int K, int epi, int kchunk) {
  const int tiles = (epi == VP_EPI_SWIGLU_IL || epi == VP_EPI_SWIGLU_HALVES) ? N / 16 : (N + 15) / 16;
  int ks = 1;
  while (tiles * ks < DG_TARGET_BLOCKS && ks < 8 && K % (2 * ks * kchunk) == 0) ks *= 2;
  return ks;
}

// W row that row r (0..15) of tile t reads
__device__ __forceinline__ int dg_row(const DecGemmArgs& p, int t, int r) {
  if (p.epi == VP_EPI_SWIGLU_HALVES) return r < 8 ? 8 * t + r : (p.N >> 1) + 8 * t + r - 8;
  return 16 * t + r;
}

__device__ __forceinline__ bf16x8 dg_norm(bf16x8 a, const bf16_t* g, float rs) {
  const bf16x8 gv = *(const bf16x8*)g;
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(bf2f((bf16_t)gv[j]) * bfround(bf2f((bf16_t)a[j]) * rs));
  return o;
}

// epilogue of one output element: v = fp32 sum (gate sum for SwiGLU), u = up sum (SwiGLU only); n = output column
__device__ __forceinline__ void dg_store(const DecGemmArgs& p, int m, int n, float v, float u) {
  if (p.epi == VP_EPI_SWIGLU_IL || p.epi == VP_EPI_SWIGLU_HALVES) {
    const float g = bfround(v), up = bfround(u);
    ((bf16_t*)p.C)[(long)m * p.ldc + n] = f2bf(bfround(silu(g)) * up);
    return;
  }
  if (p.out_f32) { ((float*)p.C)[(long)m * p.ldc + n] = v; return; }
  if (p.res) v = bfround(v) + bf2f(p.res[(long)m * p.ldr + n]);
  ((bf16_t*)p.C)[(long)m * p.ldc + n] = f2bf(v);
}

// rstd of every A row over the WHOLE K (same lane -> element assignment and summation order as vp_rmsnorm_fwd: bit-identical); wave w takes
// rows w, w + 4, ...; ends with the block's barrier
__device__ __forceinline__ void dg_rstd_rows(const DecGemmArgs& p, int w, int lane, float* rstd_s) {
  for (int mm = w; mm < p.M; mm += 4) {
    const bf16_t* a2 = p.A + (long)mm * p.lda;
    float ss = 0.f;
    for (int e = lane * 8; e < p.K; e += 512) {
      const bf16x8 v = *(const bf16x8*)(a2 + e);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float f = bf2f((bf16_t)v[j]); ss += f * f; }
    }
    ss = wave_sum(ss);
    if (lane == 0) rstd_s[mm] = rsqrtf(ss / (float)p.K + p.eps);
  }
  __syncthreads();
}

// the 4 waves' accumulators -> one 16 x 16 tile in a fixed order, then the fp32 slab of split ks (KS > 1: unscaled) or the epilogue.
// M0: the A row of the tile's column 0 (the wide kernels' 16-row A tiles; 0 in the M <= 16 kernels).
// ROWSCALE (W8): W row n's sum is multiplied by wscale[n] before dg_store's first rounding point
template <bool ROWSCALE, int M0 = 0>
__device__ __forceinline__ void dg_reduce_store(const DecGemmArgs& p, f32x4 acc, int t, int ks, int w, int lane, float (*red)[256],
                                                float (*tile_s)[17]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][lane * 4 + i] = acc[i];
  __syncthreads();
  {
    const int idx = threadIdx.x, l2 = idx >> 2, i = idx & 3;
    const float s = ((red[0][idx] + red[1][idx]) + red[2][idx]) + red[3][idx];
    tile_s[(l2 >> 4) * 4 + i][l2 & 15] = s;                      // C fragment: row (n) = (lane >> 4) * 4 + reg, col (m) = lane & 15
  }
  __syncthreads();
  const int nl = threadIdx.x >> 4, ml = threadIdx.x & 15, mm = M0 + ml;
  if (p.KS > 1) {                                                // fp32 slab [ks][M][N] (W-row order), summed by the combine kernel
    const int nn = dg_row(p, t, nl);
    if (mm < p.M && nn < p.N) p.ws[((long)ks * p.M + mm) * p.N + nn] = tile_s[nl][ml];
    return;
  }
  if (p.epi == VP_EPI_SWIGLU_IL || p.epi == VP_EPI_SWIGLU_HALVES) {
    if (threadIdx.x < 128 && mm < p.M) {
      float v = tile_s[nl][ml], u = tile_s[nl + 8][ml];
      if (ROWSCALE) { v *= p.wscale[dg_row(p, t, nl)]; u *= p.wscale[dg_row(p, t, nl + 8)]; }
      dg_store(p, mm, 8 * t + nl, v, u);
    }
    return;
  }
  if (mm < p.M && 16 * t + nl < p.N) {
    float v = tile_s[nl][ml];
    if (ROWSCALE) v *= p.wscale[16 * t + nl];
    dg_store(p, mm, 16 * t + nl, v, 0.f);
  }
}

template <bool NORM>
__global__ __launch_bounds__(DG_THREADS) void decode_gemm_kernel(DecGemmArgs p) {
  __shared__ float red[4][256];
  __shared__ float tile_s[16][17];
  __shared__ float rstd_s[16];
  const int t = blockIdx.x, ks = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  if (NORM) dg_rstd_rows(p, w, lane, rstd_s);
  // rows past N / M are clamped to the last valid row: their results are never stored, so the hot loop needs no masks
  const int n = min(dg_row(p, t, r), p.N - 1);
  const int m = min(r, p.M - 1);
  const bf16_t* wr = p.W + (long)n * p.ldw;
  const bf16_t* ar = p.A + (long)m * p.lda;
  const float rs = NORM ? rstd_s[m] : 1.f;
  const int kbeg = ks * p.Kc, kend = kbeg + p.Kc;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c = kbeg + w * DG_KCHUNK; c < kend; c += 4 * DG_KCHUNK) {
    const int k0 = c + g * 64;
    bf16x8 wv[8], av[8];
    if (c + DG_KCHUNK <= kend) {
#pragma unroll
      for (int u = 0; u < 8; ++u) wv[u] = __builtin_nontemporal_load((const bf16x8*)(wr + k0 + u * 8));
#pragma unroll
      for (int u = 0; u < 8; ++u) av[u] = *(const bf16x8*)(ar + k0 + u * 8);
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool ok = k0 + u * 8 < kend;
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        wv[u] = ok ? *(const bf16x8*)(wr + k0 + u * 8) : z;
        av[u] = ok ? *(const bf16x8*)(ar + k0 + u * 8) : z;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (NORM) {
        if (c + DG_KCHUNK <= kend || k0 + u * 8 < kend) av[u] = dg_norm(av[u], p.gamma + k0 + u * 8, rs);
      }
      // D[n][m] += sum_k W[n][k] A[m][k]: both operands carry the same k permutation (lane group g owns k0 .. k0 + 63)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[u], av[u], acc, 0, 0, 0);
    }
  }
  dg_reduce_store<false>(p, acc, t, ks, w, lane, red, tile_s);
}

// all three formats: sums the KS slabs in order, scales by the row's weight scale where there is one (W8) and applies the epilogue; one
// thread per output element
__global__ __launch_bounds__(256) void decode_gemm_combine_kernel(DecGemmArgs p) {
  const bool swiglu = p.epi == VP_EPI_SWIGLU_IL || p.epi == VP_EPI_SWIGLU_HALVES;
  const int nout = swiglu ? p.N / 2 : p.N;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)p.M * nout) return;
  const int m = (int)(i / nout), n = (int)(i % nout);
  const long slab = (long)p.M * p.N;
  if (swiglu) {
    const int t = n >> 3, j = n & 7;
    const int rg = dg_row(p, t, j), ru = dg_row(p, t, j + 8);
    float v = 0.f, u = 0.f;
    for (int k = 0; k < p.KS; ++k) { v += p.ws[k * slab + (long)m * p.N + rg]; u += p.ws[k * slab + (long)m * p.N + ru]; }
    if (p.wscale) { v *= p.wscale[rg]; u *= p.wscale[ru]; }
    dg_store(p, m, n, v, u);
    return;
  }
  float v = 0.f;
  for (int k = 0; k < p.KS; ++k) v += p.ws[k * slab + (long)m * p.N + n];
  dg_store(p, m, n, p.wscale ? v * p.wscale[n] : v, 0.f);
}

// ---------------------------------------------------------------- FP8 weight-only decode ---------------
// The reference loads a checkpoint for evaluation in 8 / 4 bits through bitsandbytes (ola_vlm/model/builder.py:26-34, load_8bit / load_4bit);
// gfx950's native answer is OCP e4m3fn weights with one power-of-two fp32 scale per row (fp8_e4m3.h, quant.py: the contract), converted
// exactly to bf16 in registers: a 16-byte load then carries 16 weights instead of 8 and the skinny GEMM streams half the bytes.
//  - quant_rows_e4m3_kernel: one block per row: absmax -> scale -> bytes (+ the dequantised value written back over the bf16 row).
//  - decode_gemm_w8_kernel: one 16-row W tile per block, K over the 4 waves and KS blocks, the bf16 kernel's MFMA with the same k
//    permutation on both operands, the shared prologue / epilogue (dg_rstd_rows, dg_norm, dg_reduce_store); a wave consumes 512 k per chunk =
//    8 loads of 16 fp8 per lane, each feeding two MFMAs.  The next chunk's 8 loads are issued before the current chunk is converted, and
//    the first chunk's before the rstd pass of the norm prologue, so the conversion (one v_cvt_scalef32_pk_bf16_fp8 per pair) never waits
//    with no load in flight.  Row n's fp32 sum is multiplied by w_scale[n] before the epilogue's first rounding point.

// the two halves of the e4m3 row contract on one 8-wide vector (weight rows here, KV heads below): the running absmax of the bf16 magnitudes ...
__device__ __forceinline__ uint32_t e4m3_absmax8(const bf16x8 v, uint32_t am) {
#pragma unroll
  for (int j = 0; j < 8; ++j) am = max(am, (uint32_t)(uint16_t)v[j] & 0x7fffu);
  return am;
}

// ... and 8 bf16 -> 8 e4m3fn bytes of v / 2^se and their dequantised values
__device__ __forceinline__ void e4m3_quant8(const bf16x8 v, int se, u32x2& q, bf16x8& d) {
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t b = vp_e4m3_quant((uint16_t)v[j], se);
    if (j < 4) lo |= b << (8 * j); else hi |= b << (8 * (j - 4));
    d[j] = (short)vp_e4m3_dequant_bf16(b, se);
  }
  q[0] = lo;
  q[1] = hi;
}

__global__ __launch_bounds__(256) void quant_rows_e4m3_kernel(bf16_t* __restrict__ W, long ldw, uint8_t* __restrict__ Q, long ldq,
                                                              float* __restrict__ scale, int K, int writeback) {
  __shared__ uint32_t red[4];
  const long n = blockIdx.x;
  bf16_t* wr = W + n * ldw;
  uint8_t* qr = Q + n * ldq;
  uint32_t am = 0;
  for (int k = threadIdx.x * 8; k < K; k += 256 * 8) am = e4m3_absmax8(*(const bf16x8*)(wr + k), am);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = am;
  __syncthreads();
  am = max(max(red[0], red[1]), max(red[2], red[3]));
  const int se = vp_e4m3_scale_exp(am);
  if (threadIdx.x == 0) scale[n] = __builtin_bit_cast(float, vp_pow2_f32_bits(se));
  for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
    u32x2 qv;
    bf16x8 d;
    e4m3_quant8(*(const bf16x8*)(wr + k), se, qv, d);
    *(u32x2*)(qr + k) = qv;
    if (writeback) *(bf16x8*)(wr + k) = d;
  }
}

static constexpr int DG8_KCHUNK = 512;       // K elements one wave consumes per iteration: 8 loads x 4 lane groups x 16 fp8

// 16 e4m3fn bytes -> two MFMA fragments (bytes 0..7 | bytes 8..15), exact.  gfx950 converts a pair of fp8 straight to a bf16 pair
// (v_cvt_scalef32_pk_bf16_fp8 with scale 1: one instruction per two weights)
__device__ __forceinline__ void dg8_cvt(const u32x4 q, bf16x8& lo, bf16x8& hi) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  u32x4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16x2_t x = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[i], 1.0f, false), y = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[i], 1.0f, true);
    if (i < 2) { a[2 * i] = __builtin_bit_cast(uint32_t, x); a[2 * i + 1] = __builtin_bit_cast(uint32_t, y); }
    else { b[2 * (i - 2)] = __builtin_bit_cast(uint32_t, x); b[2 * (i - 2) + 1] = __builtin_bit_cast(uint32_t, y); }
  }
  lo = __builtin_bit_cast(bf16x8, a);
  hi = __builtin_bit_cast(bf16x8, b);
}

// L of the 8 loads of one lane (16 k each, 64 apart: the 4 lane groups of a row read 64 consecutive bytes per load instruction, so one
// instruction touches 16 half cache lines instead of 64 sixteen-byte pieces).  Past kend (a K range that is no multiple of the chunk; K and
// Kc are multiples of 16) a load re-reads the range's last 16 bytes and its value becomes zero: no load is conditional, every address lies
// inside the row
template <int L>
__device__ __forceinline__ void dg8_load(u32x4* wq, const uint8_t* wr, int k0, int kend, bool full) {
  if (full) {
#pragma unroll
    for (int u = 0; u < L; ++u) wq[u] = __builtin_nontemporal_load((const u32x4*)(wr + k0 + u * 64));
  } else {
#pragma unroll
    for (int u = 0; u < L; ++u) {
      const bool ok = k0 + u * 64 < kend;
      const u32x4 v = __builtin_nontemporal_load((const u32x4*)(wr + (ok ? k0 + u * 64 : kend - 16)));
      wq[u] = v & (ok ? ~0u : 0u);
    }
  }
}

// One lane's share of a chunk: 16 MFMAs on the 8 converted loads of wq, in parts of L loads (4; 2 with the norm prologue, whose gamma
// vectors need the registers).  Each part issues its 2 L A fragments (bf16, L2-resident; + gamma) FIRST and then L loads of the next chunk
// (wn, when there is one): the memory counter retires in order, so waiting for A leaves those W loads in flight under the conversion.  Past
// kend A re-reads valid elements (clamped address) against zero weights.
// NEXT: 0 = no next chunk, 1 = a whole one, 2 = a partial one (a template parameter: each case is its own straight-line code, so the
// memory-counter waits are exact for it instead of the minimum over the cases)
template <bool NORM, int NEXT>
__device__ __forceinline__ f32x4 dg8_chunk(f32x4 acc, const u32x4* wq, u32x4* wn, const DecGemmArgs& p, const uint8_t* wr, const bf16_t* ar,
                                           float rs, int k0, int kend, bool full) {
  constexpr int L = NORM ? 2 : 4;
#pragma unroll
  for (int h = 0; h < 8 / L; ++h) {
    bf16x8 av[2 * L], gv[2 * L];
#pragma unroll
    for (int u = 0; u < 2 * L; ++u) {
      int k = k0 + (h * L + (u >> 1)) * 64 + (u & 1) * 8;          // the two halves of load h * L + u / 2
      if (!full) k = min(k, kend - 8);
      av[u] = *(const bf16x8*)(ar + k);
      if (NORM) gv[u] = *(const bf16x8*)(p.gamma + k);
    }
    if (NEXT) dg8_load<L>(wn + L * h, wr, k0 + 4 * DG8_KCHUNK + h * L * 64, kend, NEXT == 1);
    __builtin_amdgcn_sched_barrier(0);                           // the loads above stay above: no conversion is hoisted over them (registers)
#pragma unroll
    for (int u = 0; u < L; ++u) {
      if (NORM) {
#pragma unroll
        for (int v = 2 * u; v < 2 * u + 2; ++v) av[v] = dg_norm(av[v], (const bf16_t*)&gv[v], rs);
      }
      u32x4 wv = wq[h * L + u];
      asm volatile("" : "+v"(wv));                                 // pins the conversion below the loads of its own part: hoisted to the loop top it
      bf16x8 lo, hi;                                              // would hold all 16 fragments of the chunk at once
      dg8_cvt(wv, lo, hi);
      // D[n][m] += sum_k W[n][k] A[m][k]: both operands carry the same k permutation (lane group g owns 16 k of every 64 of the chunk)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, av[2 * u], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, av[2 * u + 1], acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

template <bool NORM>
__global__ __launch_bounds__(DG_THREADS, 3) void decode_gemm_w8_kernel(DecGemmArgs p) {
  __shared__ float red[4][256];
  __shared__ float tile_s[16][17];
  __shared__ float rstd_s[16];
  const int t = blockIdx.x, ks = blockIdx.y;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  // rows past N / M are clamped to the last valid row: their results are never stored, so the hot loop needs no masks
  const int n = min(dg_row(p, t, r), p.N - 1);
  const int m = min(r, p.M - 1);
  const uint8_t* wr = (const uint8_t*)p.W + (long)n * p.ldw;
  const bf16_t* ar = p.A + (long)m * p.lda;
  const int kbeg = ks * p.Kc, kend = kbeg + p.Kc;
  int c = kbeg + w * DG8_KCHUNK;
  u32x4 w0[8], w1[8];                                            // ping-pong: one chunk converts while the next one streams
  if (c < kend) dg8_load<8>(w0, wr, c + g * 16, kend, c + DG8_KCHUNK <= kend);       // the first chunk is in flight under the rstd pass
  if (NORM) dg_rstd_rows(p, w, lane, rstd_s);
  const float rs = NORM ? rstd_s[m] : 1.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#define DG8_STEP(WQ, WN)                                                                                          \
  {                                                                                                               \
    const int cn = c + 4 * DG8_KCHUNK, k0 = c + g * 16;                                                           \
    const bool full = c + DG8_KCHUNK <= kend;                                                                     \
    if (cn >= kend) acc = dg8_chunk<NORM, 0>(acc, WQ, WN, p, wr, ar, rs, k0, kend, full);                         \
    else if (cn + DG8_KCHUNK <= kend) acc = dg8_chunk<NORM, 1>(acc, WQ, WN, p, wr, ar, rs, k0, kend, full);       \
    else acc = dg8_chunk<NORM, 2>(acc, WQ, WN, p, wr, ar, rs, k0, kend, full);                                    \
    c = cn;                                                                                                       \
  }
  while (c < kend) {                                             // c is wave-uniform: scalar branches
    DG8_STEP(w0, w1)
    if (c >= kend) break;
    DG8_STEP(w1, w0)
  }
#undef DG8_STEP
  dg_reduce_store<true>(p, acc, t, ks, w, lane, red, tile_s);
}

// ---------------------------------------------------------------- MXFP4 weight-only decode ---------------
// The 4-bit half of the same loading options (load_4bit): OCP MXFP4 (mxfp4.h, quant.py: the contract), e2m1 codes in blocks of 32 k with one
// e8m0 scale byte per block.  gfx950 converts a pair of codes to a bf16 pair with the block scale applied by the conversion
// (v_cvt_scalef32_pk_bf16_fp4, exact: a 2-bit significand times a power of two), so a 16-byte load carries 32 weights = one scale block.
//  - quant_blocks_mxfp4_kernel: one thread per block of 32 k: absmax -> scale byte -> 16 bytes of codes (+ the dequantised value written back
//    over the bf16 block), integer arithmetic only.
//  - decode_gemm_w4_kernel: the same tile, K split, MFMA, k permutation and shared prologue / epilogue as the two kernels above (no row
//    scale in dg_reduce_store); a wave consumes 512 k per chunk = 4 loads of 32 codes per lane, each feeding four MFMAs.  The chunk's 16
//    scale bytes of a row come in one 16-byte load per lane, issued with the weight loads (lane group g uses byte g of word u for load u),
//    so no weight load waits for a scale.  The next chunk's loads are issued before the current chunk is converted, the first chunk's
//    before the rstd pass.  The scale is part of the converted value: the epilogue has no per-row multiply.
__global__ __launch_bounds__(256) void quant_blocks_mxfp4_kernel(bf16_t* __restrict__ W, long ldw, uint8_t* __restrict__ Q, long ldq,
                                                                 uint8_t* __restrict__ E, long lde, int N, int K, int writeback) {
  const int nb = K / VP_MXFP4_BLOCK;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)N * nb) return;
  const long n = i / nb;
  const int b = (int)(i % nb);
  bf16_t* wb = W + n * ldw + b * VP_MXFP4_BLOCK;
  bf16x8 v[4];
  uint32_t am = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    v[u] = *(const bf16x8*)(wb + u * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) am = max(am, (uint32_t)(uint16_t)v[u][j] & 0x7fffu);
  }
  const int se = vp_mxfp4_scale_exp(am);
  E[n * lde + b] = (uint8_t)(se + 127);
  u32x4 qv;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    uint32_t word = 0;
    bf16x8 d;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t c = vp_mxfp4_quant((uint16_t)v[u][j], se);
      word |= c << (4 * j);                                       // element k in byte k / 2, even k in the low nibble
      d[j] = (short)vp_mxfp4_dequant_bf16(c, se);
    }
    qv[u] = word;
    if (writeback) *(bf16x8*)(wb + u * 8) = d;
  }
  *(u32x4*)(Q + n * ldq + b * 16) = qv;
}

// K elements one wave consumes per iteration: 4 loads x 4 lane groups x 32 codes (16 scale blocks).  A 512-k chunk per wave (not 1024)
// leaves K = 4096 two chunk rounds of the 4 waves, so split-K can still halve it
static constexpr int DG4_KCHUNK = 512;
static constexpr int DG4_LOADS = 4;

// 8 e2m1 codes (one 32-bit word: k .. k + 7) times the block scale -> one MFMA fragment, exact.  One instruction per two weights; its last
// operand selects the byte of the word
__device__ __forceinline__ bf16x8 dg4_cvt(uint32_t word, float scale) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  u32x4 a;
  a[0] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 0));
  a[1] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 1));
  a[2] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 2));
  a[3] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 3));
  return __builtin_bit_cast(bf16x8, a);
}

// loads u0 .. u0 + L - 1 of one lane's 4 loads of a chunk (32 k = 16 bytes each, 128 k apart: the 4 lane groups of a row read 64 consecutive
// bytes per load instruction, as in the W8 kernel).  Past kend (K and Kc are multiples of 32) a load re-reads the range's last block and its
// value becomes zero (code 0 times any scale is 0): no load is conditional, every address lies inside the row.
template <int L>
__device__ __forceinline__ void dg4_load(u32x4* wq, const uint8_t* wr, int k0, int kend, bool full) {
  if (full) {
#pragma unroll
    for (int u = 0; u < L; ++u) wq[u] = __builtin_nontemporal_load((const u32x4*)(wr + ((k0 + u * 128) >> 1)));
  } else {
#pragma unroll
    for (int u = 0; u < L; ++u) {
      const bool ok = k0 + u * 128 < kend;
      const u32x4 v = __builtin_nontemporal_load((const u32x4*)(wr + ((ok ? k0 + u * 128 : kend - 32) >> 1)));
      wq[u] = v & (ok ? ~0u : 0u);
    }
  }
}

// the scale bytes of one lane's 4 loads of the chunk at c.  vec (a whole chunk, the row's scale bytes 16-byte aligned): the chunk's run of 16
// bytes in one load, load u's byte is byte g of word u; otherwise 4 byte loads (index clamped into the K range), the byte is word u itself
__device__ __forceinline__ u32x4 dg4_load_scales(const uint8_t* er, int c, int g, int kend, bool vec) {
  if (vec) return *(const u32x4*)(er + (c >> 5));
  u32x4 s;
#pragma unroll
  for (int u = 0; u < DG4_LOADS; ++u) s[u] = er[min(c + g * 32 + u * 128, kend - 32) >> 5];
  return s;
}

// One lane's share of a chunk: 16 MFMAs on the 4 converted loads of wq, in parts of L loads (2; 1 with the norm prologue, whose gamma
// vectors need the registers).  Each part issues its 4 L A fragments (bf16, L2-resident; + gamma) FIRST and then L loads of the next chunk
// (wn; part 0 also its scale bytes, sn), so waiting for A leaves those W loads in flight under the conversion.  Past kend A re-reads valid
// elements (clamped address) against zero weights.  NEXT: 0 = no next chunk, 1 = a whole one, 2 = a partial one.
template <bool NORM, int NEXT>
__device__ __forceinline__ f32x4 dg4_chunk(f32x4 acc, const u32x4* wq, const u32x4 sq, int ssh, u32x4* wn, u32x4& sn, const DecGemmArgs& p,
                                           const uint8_t* wr, const uint8_t* er, const bf16_t* ar, float rs, int c, int g, int kend,
                                           bool full, bool evec) {
  constexpr int L = NORM ? 1 : 2;
  const int k0 = c + g * 32;
#pragma unroll
  for (int h = 0; h < DG4_LOADS / L; ++h) {
    bf16x8 av[4 * L], gv[4 * L];
#pragma unroll
    for (int u = 0; u < 4 * L; ++u) {
      int k = k0 + (h * L + (u >> 2)) * 128 + (u & 3) * 8;         // the four quarters of load h * L + u / 4
      if (!full) k = min(k, kend - 8);
      av[u] = *(const bf16x8*)(ar + k);
      if (NORM) gv[u] = *(const bf16x8*)(p.gamma + k);
    }
    if (NEXT) {
      if (h == 0) sn = dg4_load_scales(er, c + 4 * DG4_KCHUNK, g, kend, NEXT == 1 && evec);
      dg4_load<L>(wn + L * h, wr, k0 + 4 * DG4_KCHUNK + h * L * 128, kend, NEXT == 1);
    }
    __builtin_amdgcn_sched_barrier(0);                           // the loads above stay above: no conversion is hoisted over them (registers)
#pragma unroll
    for (int u = 0; u < L; ++u) {
      if (NORM) {
#pragma unroll
        for (int v = 4 * u; v < 4 * u + 4; ++v) av[v] = dg_norm(av[v], (const bf16_t*)&gv[v], rs);
      }
      u32x4 wv = wq[h * L + u];
      asm volatile("" : "+v"(wv));                                 // pins the conversion below the loads of its own part
      // 2^(byte - 127) as fp32 bits: byte << 23 (byte >= 7: a normal number)
      const float sc = __builtin_bit_cast(float, ((sq[h * L + u] >> ssh) & 0xffu) << 23);
      // D[n][m] += sum_k W[n][k] A[m][k]: both operands carry the same k permutation (lane group g owns 32 k of every 128 of the chunk)
#pragma unroll
      for (int f = 0; f < 4; ++f) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dg4_cvt(wv[f], sc), av[4 * u + f], acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

template <bool NORM>
__global__ __launch_bounds__(DG_THREADS, 4) void decode_gemm_w4_kernel(DecGemmArgs p) {
  __shared__ float red[4][256];
  __shared__ float tile_s[16][17];
  __shared__ float rstd_s[16];
  const int t = blockIdx.x, ks = blockIdx.y;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  // rows past N / M are clamped to the last valid row: their results are never stored, so the hot loop needs no masks
  const int n = min(dg_row(p, t, r), p.N - 1);
  const int m = min(r, p.M - 1);
  const uint8_t* wr = (const uint8_t*)p.W + (long)n * p.ldw;
  const uint8_t* er = p.E + (long)n * p.lde;
  const bf16_t* ar = p.A + (long)m * p.lda;
  const int kbeg = ks * p.Kc, kend = kbeg + p.Kc;
  // every row's scale bytes 16-byte aligned (block-uniform): whole chunks fetch their 16 scale bytes in one load
  const bool evec = ((((uintptr_t)p.E) | (uintptr_t)p.lde) & 15) == 0;
  int c = kbeg + w * DG4_KCHUNK;
  u32x4 w0[DG4_LOADS], w1[DG4_LOADS], s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};  // ping-pong: one chunk converts while the next one streams
  if (c < kend) {                                                // the first chunk is in flight under the rstd pass
    s0 = dg4_load_scales(er, c, g, kend, evec && c + DG4_KCHUNK <= kend);
    dg4_load<DG4_LOADS>(w0, wr, c + g * 32, kend, c + DG4_KCHUNK <= kend);
  }
  if (NORM) dg_rstd_rows(p, w, lane, rstd_s);
  const float rs = NORM ? rstd_s[m] : 1.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // ssh: which byte of a scale word belongs to this lane: byte g of the 16-byte run, the whole word after byte loads
#define DG4_STEP(WQ, SQ, WN, SN)                                                                                           \
  {                                                                                                                        \
    const int cn = c + 4 * DG4_KCHUNK;                                                                                     \
    const bool full = c + DG4_KCHUNK <= kend;                                                                              \
    const int ssh = (full && evec) ? 8 * g : 0;                                                                            \
    if (cn >= kend) acc = dg4_chunk<NORM, 0>(acc, WQ, SQ, ssh, WN, SN, p, wr, er, ar, rs, c, g, kend, full, evec);         \
    else if (cn + DG4_KCHUNK <= kend) acc = dg4_chunk<NORM, 1>(acc, WQ, SQ, ssh, WN, SN, p, wr, er, ar, rs, c, g, kend, full, evec); \
    else acc = dg4_chunk<NORM, 2>(acc, WQ, SQ, ssh, WN, SN, p, wr, er, ar, rs, c, g, kend, full, evec);                    \
    c = cn;                                                                                                                \
  }
  while (c < kend) {                                             // c is wave-uniform: scalar branches
    DG4_STEP(w0, s0, w1, s1)
    if (c >= kend) break;
    DG4_STEP(w1, s1, w0, s0)
  }
#undef DG4_STEP
  dg_reduce_store<false>(p, acc, t, ks, w, lane, red, tile_s);
}

// ---------------------------------------------------------------- wide decode GEMMs: 17 <= M <= 64 ---------------
// Decode is weight-bound, so more sequences per step are nearly free as long as every weight byte is still streamed once: the wide kernels
// keep the block of the kernels above (one 16-row W tile, K over the 4 waves and KS blocks, the same chunk, loads and conversion per
// format) and serve MT = ceil(M / 16) 16-row A tiles from each converted W fragment, one f32x4 accumulator per tile.  Output column m is the
// MFMA column of A row m alone: tile j, lane row r reads A row min(16 j + r, M - 1), the chunk order, the order inside a chunk, the 4-wave
// reduction (dg_reduce_store per tile, in tile order) and the combine are those of the M <= 16 kernels, so every row equals, bit for bit,
// what the M <= 16 entry point returns for it inside any 16-row slice of A.  The norm prologue stays in the block (dg_rstd_rows over all M
// rows); gamma is loaded once per part and shared by the tiles.
template <int MT>
struct DgRows {
  const bf16_t* ar[MT];                      // this lane's A row of every tile
  float rs[MT];                              // its rstd (1 without the norm prologue)
};

template <bool NORM, int MT>
__device__ __forceinline__ DgRows<MT> dg_wide_rows(const DecGemmArgs& p, int r, const float* rstd_s) {
  DgRows<MT> a;
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = min(16 * j + r, p.M - 1);  // rows past M are clamped to the last valid row: never stored
    a.ar[j] = p.A + (long)m * p.lda;
    a.rs[j] = NORM ? rstd_s[m] : 1.f;
  }
  return a;
}

// the tiles' reductions in tile order; between two of them a barrier: tile j - 1's tile_s reads are done before red / tile_s are rewritten
template <bool ROWSCALE, int MT, int J = 0>
__device__ __forceinline__ void dg_wide_reduce_store(const DecGemmArgs& p, const f32x4* acc, int t, int ks, int w, int lane,
                                                     float (*red)[256], float (*tile_s)[17]) {
  if constexpr (J < MT) {
    if (J) __syncthreads();
    dg_reduce_store<ROWSCALE, 16 * J>(p, acc[J], t, ks, w, lane, red, tile_s);
    dg_wide_reduce_store<ROWSCALE, MT, J + 1>(p, acc, t, ks, w, lane, red, tile_s);
  }
}

template <bool NORM, int MT>
__global__ __launch_bounds__(DG_THREADS) void decode_gemm_wide_kernel(DecGemmArgs p) {
  __shared__ float red[4][256];
  __shared__ float tile_s[16][17];
  __shared__ float rstd_s[16 * MT];
  const int t = blockIdx.x, ks = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  if (NORM) dg_rstd_rows(p, w, lane, rstd_s);
  const int n = min(dg_row(p, t, r), p.N - 1);
  const bf16_t* wr = p.W + (long)n * p.ldw;
  const DgRows<MT> a = dg_wide_rows<NORM, MT>(p, r, rstd_s);
  const int kbeg = ks * p.Kc, kend = kbeg + p.Kc;
  f32x4 acc[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = kbeg + w * DG_KCHUNK; c < kend; c += 4 * DG_KCHUNK) {
    const int k0 = c + g * 64;
    const bool full = c + DG_KCHUNK <= kend;
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (full) wv[u] = __builtin_nontemporal_load((const bf16x8*)(wr + k0 + u * 8));
      else wv[u] = k0 + u * 8 < kend ? *(const bf16x8*)(wr + k0 + u * 8) : z;
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      bf16x8 av[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) av[u] = (full || k0 + u * 8 < kend) ? *(const bf16x8*)(a.ar[j] + k0 + u * 8) : z;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (NORM) {
          if (full || k0 + u * 8 < kend) av[u] = dg_norm(av[u], p.gamma + k0 + u * 8, a.rs[j]);
        }
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[u], av[u], acc[j], 0, 0, 0);
      }
    }
  }
  dg_wide_reduce_store<false, MT>(p, acc, t, ks, w, lane, red, tile_s);
}

// the A side of one part of a quantised chunk, shared by W8 and W4 (F fragments at the k offsets kk, already clamped).  Every tile's
// A fragments (bf16, L2-resident; + gamma) are issued FIRST and the part's loads of the next chunk after them, as in dg8_chunk: the
// memory counter retires in order, so waiting for A leaves those W loads in flight under the conversion
template <bool NORM, int MT, int F>
__device__ __forceinline__ void dg_wide_load_a(bf16x8 (*av)[F], bf16x8* gv, const int* kk, const DecGemmArgs& p, const DgRows<MT>& a) {
#pragma unroll
  for (int j = 0; j < MT; ++j) {
#pragma unroll
    for (int u = 0; u < F; ++u) av[j][u] = *(const bf16x8*)(a.ar[j] + kk[u]);
  }
  if (NORM) {
#pragma unroll
    for (int u = 0; u < F; ++u) gv[u] = *(const bf16x8*)(p.gamma + kk[u]);
  }
}

// ... and its MFMAs: the part's converted W fragments wf against every tile
template <bool NORM, int MT, int F>
__device__ __forceinline__ void dg_wide_mfma(f32x4* acc, const bf16x8* wf, bf16x8 (*av)[F], const bf16x8* gv, const DgRows<MT>& a) {
#pragma unroll
  for (int j = 0; j < MT; ++j) {
#pragma unroll
    for (int u = 0; u < F; ++u) {
      if (NORM) av[j][u] = dg_norm(av[j][u], (const bf16_t*)&gv[u], a.rs[j]);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], av[j][u], acc[j], 0, 0, 0);
    }
  }
}

// dg8_chunk for MT tiles, in parts of 2 loads (4 fragments): the MFMA order of a row is that of dg8_chunk (loads 0 .. 7, low half then high)
template <bool NORM, int NEXT, int MT>
__device__ __forceinline__ void dg8_wide_chunk(f32x4* acc, const u32x4* wq, u32x4* wn, const DecGemmArgs& p, const uint8_t* wr,
                                               const DgRows<MT>& a, int k0, int kend, bool full) {
  constexpr int L = 2;
#pragma unroll
  for (int h = 0; h < 8 / L; ++h) {
    int kk[2 * L];
#pragma unroll
    for (int u = 0; u < 2 * L; ++u) {
      const int k = k0 + (h * L + (u >> 1)) * 64 + (u & 1) * 8;    // the two halves of load h * L + u / 2
      kk[u] = full ? k : min(k, kend - 8);
    }
    bf16x8 av[MT][2 * L], gv[2 * L], wf[2 * L];
    dg_wide_load_a<NORM, MT, 2 * L>(av, gv, kk, p, a);
    if (NEXT) dg8_load<L>(wn + L * h, wr, k0 + 4 * DG8_KCHUNK + h * L * 64, kend, NEXT == 1);
    __builtin_amdgcn_sched_barrier(0);                           // the loads above stay above: no conversion is hoisted over them (registers)
#pragma unroll
    for (int u = 0; u < L; ++u) {
      u32x4 wv = wq[h * L + u];
      asm volatile("" : "+v"(wv));                                 // pins the conversion below the loads of its own part
      dg8_cvt(wv, wf[2 * u], wf[2 * u + 1]);
    }
    dg_wide_mfma<NORM, MT, 2 * L>(acc, wf, av, gv, a);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool NORM, int MT>
__global__ __launch_bounds__(DG_THREADS, 2) void decode_gemm_w8_wide_kernel(DecGemmArgs p) {
  __shared__ float red[4][256];
  __shared__ float tile_s[16][17];
  __shared__ float rstd_s[16 * MT];
  const int t = blockIdx.x, ks = blockIdx.y;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n = min(dg_row(p, t, r), p.N - 1);
  const uint8_t* wr = (const uint8_t*)p.W + (long)n * p.ldw;
  const int kbeg = ks * p.Kc, kend = kbeg + p.Kc;
  int c = kbeg + w * DG8_KCHUNK;
  u32x4 w0[8], w1[8];                                            // ping-pong: one chunk converts while the next one streams
  if (c < kend) dg8_load<8>(w0, wr, c + g * 16, kend, c + DG8_KCHUNK <= kend);       // the first chunk is in flight under the rstd pass
  if (NORM) dg_rstd_rows(p, w, lane, rstd_s);
  const DgRows<MT> a = dg_wide_rows<NORM, MT>(p, r, rstd_s);
  f32x4 acc[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#define DG8_STEP(WQ, WN)                                                                                          \
  {                                                                                                               \
    const int cn = c + 4 * DG8_KCHUNK, k0 = c + g * 16;                                                           \
    const bool full = c + DG8_KCHUNK <= kend;                                                                     \
    if (cn >= kend) dg8_wide_chunk<NORM, 0, MT>(acc, WQ, WN, p, wr, a, k0, kend, full);                           \
    else if (cn + DG8_KCHUNK <= kend) dg8_wide_chunk<NORM, 1, MT>(acc, WQ, WN, p, wr, a, k0, kend, full);         \
    else dg8_wide_chunk<NORM, 2, MT>(acc, WQ, WN, p, wr, a, k0, kend, full);                                      \
    c = cn;                                                                                                       \
  }
  while (c < kend) {                                             // c is wave-uniform: scalar branches
    DG8_STEP(w0, w1)
    if (c >= kend) break;
    DG8_STEP(w1, w0)
  }
#undef DG8_STEP
  dg_wide_reduce_store<true, MT>(p, acc, t, ks, w, lane, red, tile_s);
}

// dg4_chunk for MT tiles, in parts of 1 load (4 fragments)
template <bool NORM, int NEXT, int MT>
__device__ __forceinline__ void dg4_wide_chunk(f32x4* acc, const u32x4* wq, const u32x4 sq, int ssh, u32x4* wn, u32x4& sn,
                                               const DecGemmArgs& p, const uint8_t* wr, const uint8_t* er, const DgRows<MT>& a, int c, int g,
                                               int kend, bool full, bool evec) {
  const int k0 = c + g * 32;
#pragma unroll
  for (int h = 0; h < DG4_LOADS; ++h) {
    int kk[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int k = k0 + h * 128 + f * 8;                          // the four quarters of load h
      kk[f] = full ? k : min(k, kend - 8);
    }
    bf16x8 av[MT][4], gv[4], wf[4];
    dg_wide_load_a<NORM, MT, 4>(av, gv, kk, p, a);
    if (NEXT) {
      if (h == 0) sn = dg4_load_scales(er, c + 4 * DG4_KCHUNK, g, kend, NEXT == 1 && evec);
      dg4_load<1>(wn + h, wr, k0 + 4 * DG4_KCHUNK + h * 128, kend, NEXT == 1);
    }
    __builtin_amdgcn_sched_barrier(0);                           // the loads above stay above: no conversion is hoisted over them (registers)
    u32x4 wv = wq[h];
    asm volatile("" : "+v"(wv));                                   // pins the conversion below the loads of its own part
    // 2^(byte - 127) as fp32 bits: byte << 23 (byte >= 7: a normal number)
    const float sc = __builtin_bit_cast(float, ((sq[h] >> ssh) & 0xffu) << 23);
#pragma unroll
    for (int f = 0; f < 4; ++f) wf[f] = dg4_cvt(wv[f], sc);
    dg_wide_mfma<NORM, MT, 4>(acc, wf, av, gv, a);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool NORM, int MT>
__global__ __launch_bounds__(DG_THREADS, 2) void decode_gemm_w4_wide_kernel(DecGemmArgs p) {
  __shared__ float red[4][256];
  __shared__ float tile_s[16][17];
  __shared__ float rstd_s[16 * MT];
  const int t = blockIdx.x, ks = blockIdx.y;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n = min(dg_row(p, t, r), p.N - 1);
  const uint8_t* wr = (const uint8_t*)p.W + (long)n * p.ldw;
  const uint8_t* er = p.E + (long)n * p.lde;
  const int kbeg = ks * p.Kc, kend = kbeg + p.Kc;
  const bool evec = ((((uintptr_t)p.E) | (uintptr_t)p.lde) & 15) == 0;
  int c = kbeg + w * DG4_KCHUNK;
  u32x4 w0[DG4_LOADS], w1[DG4_LOADS], s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};  // ping-pong: one chunk converts while the next one streams
  if (c < kend) {                                                // the first chunk is in flight under the rstd pass
    s0 = dg4_load_scales(er, c, g, kend, evec && c + DG4_KCHUNK <= kend);
    dg4_load<DG4_LOADS>(w0, wr, c + g * 32, kend, c + DG4_KCHUNK <= kend);
  }
  if (NORM) dg_rstd_rows(p, w, lane, rstd_s);
  const DgRows<MT> a = dg_wide_rows<NORM, MT>(p, r, rstd_s);
  f32x4 acc[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#define DG4_STEP(WQ, SQ, WN, SN)                                                                                           \
  {                                                                                                                        \
    const int cn = c + 4 * DG4_KCHUNK;                                                                                     \
    const bool full = c + DG4_KCHUNK <= kend;                                                                              \
    const int ssh = (full && evec) ? 8 * g : 0;                                                                            \
    if (cn >= kend) dg4_wide_chunk<NORM, 0, MT>(acc, WQ, SQ, ssh, WN, SN, p, wr, er, a, c, g, kend, full, evec);           \
    else if (cn + DG4_KCHUNK <= kend) dg4_wide_chunk<NORM, 1, MT>(acc, WQ, SQ, ssh, WN, SN, p, wr, er, a, c, g, kend, full, evec); \
    else dg4_wide_chunk<NORM, 2, MT>(acc, WQ, SQ, ssh, WN, SN, p, wr, er, a, c, g, kend, full, evec);                      \
    c = cn;                                                                                                                \
  }
  while (c < kend) {                                             // c is wave-uniform: scalar branches
    DG4_STEP(w0, s0, w1, s1)
    if (c >= kend) break;
    DG4_STEP(w1, s1, w0, s0)
  }
#undef DG4_STEP
  dg_wide_reduce_store<false, MT>(p, acc, t, ks, w, lane, red, tile_s);
}

// ---------------------------------------------------------------- RoPE + KV append ---------------
// rotate-half RoPE of 8 element pairs (a: the head's first half, b: its partner in the second half) by 8 table entries: vp_rope's rounding points
__device__ __forceinline__ void rope_rot8(const bf16x8 a, const bf16x8 b, const float* c, const float* s, bf16x8& oa, bf16x8& ob) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x1 = bf2f((bf16_t)a[j]), x2 = bf2f((bf16_t)b[j]);
    oa[j] = (short)f2bf(bfround(x1 * c[j]) + bfround(-x2 * s[j]));
    ob[j] = (short)f2bf(bfround(x2 * c[j]) + bfround(x1 * s[j]));
  }
}

// qkv [B, ldq] rows (q heads | k heads | v heads); thread = one 8-wide vector of one head's first half (q / k) or 16 elements of v.
// cache_row (null: identity): row b appends to cache row cache_row[b]; q_out stays indexed by b
__global__ void decode_rope_append_kernel(const bf16_t* __restrict__ qkv, long ldqkv, bf16_t* __restrict__ qo, long ldq,
                                          bf16_t* __restrict__ kc, long k_bs, long k_ts, bf16_t* __restrict__ vc, long v_bs, long v_ts,
                                          const float* __restrict__ cs, const float* __restrict__ sn, const int* __restrict__ pos,
                                          const int* __restrict__ cache_row, int B, int Hq, int Hkv, int D, int Smax) {
  const int half = D >> 1, vph = half >> 3;
  const int per_b = (Hq + Hkv) * vph + Hkv * (D >> 3);
  const long total = (long)B * per_b;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / per_b), r = (int)(i % per_b);
    const int p = pos[b];
    const int cb = cache_row ? cache_row[b] : b;
    const bf16_t* row = qkv + (long)b * ldqkv;
    if (r < (Hq + Hkv) * vph) {
      const int h = r / vph, v = r % vph;
      const bool isq = h < Hq;
      if (!isq && (p < 0 || p >= Smax)) continue;               // never write outside the cache
      const bf16_t* src = row + (long)h * D + v * 8;
      const bf16x8 a = *(const bf16x8*)src, bb = *(const bf16x8*)(src + half);
      const int pc = min(max(p, 0), Smax - 1);
      bf16x8 oa, ob;
      rope_rot8(a, bb, cs + (long)pc * half + v * 8, sn + (long)pc * half + v * 8, oa, ob);
      bf16_t* dst = isq ? qo + (long)b * ldq + (long)h * D + v * 8 : kc + (long)cb * k_bs + (long)p * k_ts + (long)(h - Hq) * D + v * 8;
      *(bf16x8*)dst = oa;
      *(bf16x8*)(dst + half) = ob;
    } else {
      if (p < 0 || p >= Smax) continue;
      const int e = (r - (Hq + Hkv) * vph) * 8;                  // element within the Hkv * D v block
      *(bf16x8*)(vc + (long)cb * v_bs + (long)p * v_ts + e) = *(const bf16x8*)(row + (long)(Hq + Hkv) * D + e);
    }
  }
}

// ---------------------------------------------------------------- decode attention ---------------
static constexpr int DA_CHMAX = 512;       // keys one split block handles at most (scores stay in LDS)
static constexpr float DA_LOG2E = 1.4426950408889634f;

// The two split kernels (bf16 and e4m3 caches) differ in their score and P V loops only; the three phases around them are shared.
// Keys [s0, s0 + cnt) of block (split blockIdx.x of gridDim.x, blockIdx.y = hkv, blockIdx.z = b), and where its partial goes: an even
// share of the window's / sequence's keys per split.  cnt <= DA_CHMAX: the launcher checks Smax <= nsplit * DA_CHMAX.  cb: the cache row
// the block reads (cache_row[b]; b itself without a row map); q, kv_len and the partials stay indexed by b
template <int D, int G>
__device__ __forceinline__ float* da_split_range(const int* kv_len, const int* cache_row, int Smax, int window, float* ws, int Hkv, int& s0,
                                                 int& cnt, int& cb) {
  const int s = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z, ns = gridDim.x;
  cb = cache_row ? cache_row[b] : b;
  const int len = min(kv_len[b], Smax);
  const int lo = window > 0 ? max(0, len - window) : 0;
  const int nk = max(0, len - lo);
  const int ch = (nk + ns - 1) / ns;
  s0 = lo + min(nk, s * ch);
  cnt = lo + min(nk, (s + 1) * ch) - s0;
  return ws + (((long)b * Hkv + hkv) * ns + s) * G * (D + 2);
}

// scores sc[g][0 .. cnt) (log2 domain) -> p_j = 2^(score - max) in place, ml[g] = (max, sum); wave w handles heads w, w + 4, ...  A barrier
// on either side: the scores come from, and the p_j go to, other threads
template <int G>
__device__ __forceinline__ void da_softmax(float (*sc)[DA_CHMAX], float (*ml)[2], int cnt, int w, int lane) {
  __syncthreads();
  for (int g = w; g < G; g += 4) {
    float mx = -INFINITY;
    for (int j = lane; j < cnt; j += 64) mx = fmaxf(mx, sc[g][j]);
    mx = wave_max(mx);
    float l = 0.f;
    for (int j = lane; j < cnt; j += 64) {
      const float pj = exp2f(sc[g][j] - mx);
      sc[g][j] = pj;
      l += pj;
    }
    l = wave_sum(l);
    if (lane == 0) { ml[g][0] = mx; ml[g][1] = l; }
  }
  __syncthreads();
}

// acc[g][x]: a lane's P V sums for elements e + x (EPL per lane, LPK lanes per key row).  Key groups of a wave (lanes sl, sl + LPK, ...)
// -> one, then the 4 waves in a fixed order -> the partial: D unnormalised outputs per head, then m, l
template <int D, int G, int EPL, int LPK>
__device__ __forceinline__ void da_reduce_store(float (&acc)[G][EPL], float (*red)[G][D], const float (*ml)[2], float* out, int cnt, int e,
                                                bool act, int w, int lane) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int x = 0; x < EPL; ++x)
#pragma unroll
      for (int o = LPK; o < 64; o <<= 1) acc[g][x] += __shfl_xor(acc[g][x], o, 64);
  if (lane < LPK && act)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int x = 0; x < EPL; ++x) red[w][g][e + x] = acc[g][x];
  __syncthreads();
  for (int i = tid; i < G * D; i += 256) {
    const int g = i / D, dd = i % D;
    out[g * (D + 2) + dd] = ((red[0][g][dd] + red[1][g][dd]) + red[2][g][dd]) + red[3][g][dd];
  }
  if (tid < G) {
    out[tid * (D + 2) + D] = cnt > 0 ? ml[tid][0] : -INFINITY;
    out[tid * (D + 2) + D + 1] = cnt > 0 ? ml[tid][1] : 0.f;
  }
}

// grid (nsplit, Hkv, B), 256 threads.  Partial per (b, hkv, split, g): D unnormalised fp32 outputs, then m (log2 domain), l.
template <int D, int G>
__global__ __launch_bounds__(256) void decode_attn_split_kernel(const bf16_t* __restrict__ q, long q_bs, const bf16_t* __restrict__ k,
                                                                long k_bs, long k_ts, const bf16_t* __restrict__ v, long v_bs, long v_ts,
                                                                const int* __restrict__ kv_len, const int* __restrict__ cache_row,
                                                                int Smax, int window, float scale, float* __restrict__ ws, int Hkv) {
  constexpr int LPK = D <= 32 ? 4 : (D <= 64 ? 8 : 16);         // lanes per key row (16-byte vectors; D = 96 leaves 4 of 16 idle)
  constexpr int KPB = 256 / LPK;                                 // key rows per block pass
  __shared__ float sc[G][DA_CHMAX];
  __shared__ float red[4][G][D];
  __shared__ float ml[G][2];
  const int hkv = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sl = tid % LPK, ko = tid / LPK, e = sl * 8;
  const bool act = e < D;
  int s0, cnt, cb;
  float* out = da_split_range<D, G>(kv_len, cache_row, Smax, window, ws, Hkv, s0, cnt, cb);
  float qf[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bf16x8 qv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) qv = *(const bf16x8*)(q + (long)b * q_bs + (long)(hkv * G + g) * D + e);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[g][j] = bf2f((bf16_t)qv[j]) * (scale * DA_LOG2E);
  }
  const bf16_t* kb = k + (long)cb * k_bs + (long)hkv * D + e;
  const bf16_t* vb = v + (long)cb * v_bs + (long)hkv * D + e;
  // scores (log2 domain) -> LDS
  for (int j0 = 0; j0 < cnt; j0 += KPB) {
    const int j = j0 + ko;
    bf16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act && j < cnt) kv = *(const bf16x8*)(kb + (long)(s0 + j) * k_ts);
    float d[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float a = 0.f;
#pragma unroll
      for (int x = 0; x < 8; ++x) a += qf[g][x] * bf2f((bf16_t)kv[x]);
#pragma unroll
      for (int o = LPK / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      d[g] = a;
    }
    if (sl == 0 && j < cnt)
#pragma unroll
      for (int g = 0; g < G; ++g) sc[g][j] = d[g];
  }
  da_softmax<G>(sc, ml, cnt, w, lane);
  // P V
  float acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int x = 0; x < 8; ++x) acc[g][x] = 0.f;
  for (int j0 = 0; j0 < cnt; j0 += KPB) {
    const int j = j0 + ko;
    if (act && j < cnt) {
      const bf16x8 vv = *(const bf16x8*)(vb + (long)(s0 + j) * v_ts);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pj = sc[g][j];
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[g][x] += pj * bf2f((bf16_t)vv[x]);
      }
    }
  }
  da_reduce_store<D, G, 8, LPK>(acc, red, ml, out, cnt, e, act, w, lane);
}

// grid (Hq, B), D threads: o[b, h, :] = sum_s 2^(m_s - M) o_s / sum_s 2^(m_s - M) l_s, splits in order
__global__ void decode_attn_combine_kernel(const float* __restrict__ ws, bf16_t* __restrict__ o, long o_bs, int Hkv, int G, int D,
                                           int ns) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const int hkv = h / G, g = h % G;
  const float* base = ws + ((long)b * Hkv + hkv) * ns * G * (D + 2) + (long)g * (D + 2);
  const long sstride = (long)G * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < ns; ++s) M = fmaxf(M, base[s * sstride + D]);
  float L = 0.f, acc = 0.f;
  if (M != -INFINITY)
    for (int s = 0; s < ns; ++s) {
      const float ms = base[s * sstride + D];
      if (ms == -INFINITY) continue;
      const float f = exp2f(ms - M);
      L += f * base[s * sstride + D + 1];
      acc += f * base[s * sstride + d];
    }
  if (d < D) o[(long)b * o_bs + (long)h * D + d] = f2bf(L > 0.f ? acc / L : 0.f);
}

__global__ void add_i32_kernel(int* __restrict__ x, long n, int delta) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i < n) x[i] += delta;
}

// ---------------------------------------------------------------- prompt-lookup acceptance ---------------
// One thread per sequence of a verify step of n + 1 rows: row (b, i) was fed tok[b, i] (row 0: the last emitted token, rows 1 .. n: the
// drafts) and chose next[b, i].  Draft i stands if every draft before it stands and it is the token row i - 1 chose; n_acc[b] of them do.
// The sequence moves n_acc[b] + 1 positions; the next step's rows sit at base_pos[b] + i and attend to their own key as the one-token step
// does (kv_len = pos + 1); its row 0 is fed the token chosen after the last accepted draft.  n = 0: the one-token step's + 1.
__global__ void decode_accept_kernel(const int* __restrict__ next, int* __restrict__ tok, int* __restrict__ base_pos, int* __restrict__ pos,
                                     int* __restrict__ kv_len, int* __restrict__ n_acc, int B, int n) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const long r0 = (long)b * (n + 1);
  int j = 0;
  while (j < n && tok[r0 + j + 1] == next[r0 + j]) ++j;
  const int bp = base_pos[b] + j + 1;
  n_acc[b] = j;
  base_pos[b] = bp;
  for (int i = 0; i <= n; ++i) {
    pos[r0 + i] = bp + i;
    kv_len[r0 + i] = bp + i + 1;
  }
  tok[r0] = next[r0 + j];
}

// ---------------------------------------------------------------- FP8 (e4m3) KV cache ---------------
// The third member of the e4m3 / MXFP4 family: the cache itself in OCP e4m3fn bytes with one power-of-two fp32 scale per (token, KV head) —
// the row contract of fp8_e4m3.h with row length D (quant.py: quantize_kv_heads).  K is quantised after RoPE, V as projected.
//  - quant_kv_e4m3_kernel: the prefill sink.  One (token, head) row per lane group: absmax -> scale -> bytes (and / or the dequantised
//    values as bf16 rows of a bf16 cache: the emulated mode, which the bf16 decode attention then reads), with the weight quantiser's
//    e4m3_absmax8 / e4m3_quant8.
//  - decode_rope_append_kv8_kernel: decode_rope_append_kernel's rotation (rope_rot8: q is bit-identical) with one lane group per head, so
//    that the D rotated elements of a k head (the D elements of a v head) meet for their absmax; row pos[b] receives bytes + scale.
//  - decode_attn_split_kv8_kernel: the split, softmax and reduction phases of decode_attn_split_kernel (da_split_range, da_softmax,
//    da_reduce_store) around score and P V loops on byte operands: a 16-byte load carries 16 elements, a key row takes half the lanes and a
//    block pass covers twice the keys.  The bytes are converted exactly in registers (v_cvt_scalef32_pk_bf16_fp8, scale 1); the k scale
//    multiplies the finished dot product, the v scale multiplies p_j before the P V accumulation (both exact power-of-two products in
//    fp32).  The partials have one layout: decode_attn_combine_kernel and the workspace are shared.
struct KvDst {                               // one of k / v: bytes + scales (q, s: both or neither) and / or dequantised bf16 rows (d)
  uint8_t* q; long q_bs, q_ts;               // strides in bytes
  float* s; long s_bs, s_ts;                 // [B, Smax, Hkv] fp32, strides in elements
  bf16_t* d; long d_bs, d_ts;                // strides in elements
};

// n token rows of `heads` heads (2 Hkv for a k|v row); lph lanes per head (a power of two >= D / 8 that divides 64: a head never straddles a
// wave), lane sl owns elements sl * 8 .. sl * 8 + 7.  Every lane of the block runs every shuffle (the trip count is block-uniform).
__global__ __launch_bounds__(256) void quant_kv_e4m3_kernel(const bf16_t* __restrict__ src, long ld_src, uint8_t* __restrict__ Q, long ldq,
                                                            float* __restrict__ scale, long ld_scale, bf16_t* __restrict__ deq, long ldd,
                                                            long n, int heads, int D, int lph) {
  const long total = n * heads * lph;
  for (long base = blockIdx.x * 256L; base < total; base += gridDim.x * 256L) {
    const long i = base + threadIdx.x;
    const long grp = i / lph;
    const int sl = (int)(i % lph);
    const bool act = i < total && sl * 8 < D;
    const long t = grp / heads;
    const long off = (grp % heads) * D + sl * 8;
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) v = *(const bf16x8*)(src + t * ld_src + off);
    uint32_t am = e4m3_absmax8(v, 0);
    for (int o = lph >> 1; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
    if (act) {
      const int se = vp_e4m3_scale_exp(am);
      u32x2 qv;
      bf16x8 d;
      e4m3_quant8(v, se, qv, d);
      if (Q) {
        *(u32x2*)(Q + t * ldq + off) = qv;
        if (sl == 0) scale[t * ld_scale + grp % heads] = __builtin_bit_cast(float, vp_pow2_f32_bits(se));
      }
      if (deq) *(bf16x8*)(deq + t * ldd + off) = d;
    }
  }
}

// qkv [B, ldq] rows (q heads | k heads | v heads); lph lanes per head (a power of two >= D / 16), lane sl owns the 8-wide vector sl of the
// head's first half and its partner in the second half (the rotation pair for q / k).  cache_row: as decode_rope_append_kernel
__global__ __launch_bounds__(256) void decode_rope_append_kv8_kernel(const bf16_t* __restrict__ qkv, long ldqkv, bf16_t* __restrict__ qo,
                                                                     long ldq, KvDst kd, KvDst vd, const float* __restrict__ cs,
                                                                     const float* __restrict__ sn, const int* __restrict__ pos,
                                                                     const int* __restrict__ cache_row, int B, int Hq, int Hkv, int D,
                                                                     int Smax, int lph) {
  const int half = D >> 1, vph = half >> 3;
  const int per_b = (Hq + 2 * Hkv) * lph;
  const long total = (long)B * per_b;
  for (long base = blockIdx.x * 256L; base < total; base += gridDim.x * 256L) {
    const long i = base + threadIdx.x;
    const bool in = i < total;
    const int b = in ? (int)(i / per_b) : 0, r = in ? (int)(i % per_b) : 0;
    const int h = r / lph, sl = r % lph;
    const bool act = in && sl < vph;
    const bool rot = h < Hq + Hkv;
    const int p = pos[b];
    const int cb = cache_row ? cache_row[b] : b;
    bf16x8 oa = {0, 0, 0, 0, 0, 0, 0, 0}, ob = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
      const bf16_t* src = qkv + (long)b * ldqkv + (long)h * D + sl * 8;
      const bf16x8 a = *(const bf16x8*)src, bb = *(const bf16x8*)(src + half);
      if (rot) {
        const int pc = min(max(p, 0), Smax - 1);
        rope_rot8(a, bb, cs + (long)pc * half + sl * 8, sn + (long)pc * half + sl * 8, oa, ob);
      } else {
        oa = a;
        ob = bb;
      }
    }
    uint32_t am = e4m3_absmax8(ob, e4m3_absmax8(oa, 0));
    for (int o = lph >> 1; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
    if (act && h < Hq) {
      bf16_t* dst = qo + (long)b * ldq + (long)h * D + sl * 8;
      *(bf16x8*)dst = oa;
      *(bf16x8*)(dst + half) = ob;
    } else if (act && p >= 0 && p < Smax) {                         // never write outside the cache
      const int hk = rot ? h - Hq : h - Hq - Hkv;
      const int se = vp_e4m3_scale_exp(am);
      u32x2 qa, qb;
      bf16x8 da, db;
      e4m3_quant8(oa, se, qa, da);
      e4m3_quant8(ob, se, qb, db);
      uint8_t* qp = rot ? kd.q : vd.q;
      if (qp) {
        qp += (rot ? (long)cb * kd.q_bs + (long)p * kd.q_ts : (long)cb * vd.q_bs + (long)p * vd.q_ts) + (long)hk * D + sl * 8;
        *(u32x2*)qp = qa;
        *(u32x2*)(qp + half) = qb;
        if (sl == 0) {
          float* sp = rot ? kd.s + (long)cb * kd.s_bs + (long)p * kd.s_ts : vd.s + (long)cb * vd.s_bs + (long)p * vd.s_ts;
          sp[hk] = __builtin_bit_cast(float, vp_pow2_f32_bits(se));
        }
      }
      bf16_t* dp = rot ? kd.d : vd.d;
      if (dp) {
        dp += (rot ? (long)cb * kd.d_bs + (long)p * kd.d_ts : (long)cb * vd.d_bs + (long)p * vd.d_ts) + (long)hk * D + sl * 8;
        *(bf16x8*)dp = da;
        *(bf16x8*)(dp + half) = db;
      }
    }
  }
}

// 16 e4m3fn bytes -> 16 fp32, exact: gfx950 converts a pair of fp8 to a bf16 pair in one instruction (as dg8_cvt), a bf16 is the upper half
// of its fp32
__device__ __forceinline__ void da8_cvt(const u32x4 q, float* f) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t x = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[i], 1.0f, false));
    const uint32_t y = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[i], 1.0f, true));
    f[4 * i] = __builtin_bit_cast(float, x << 16);
    f[4 * i + 1] = __builtin_bit_cast(float, x & 0xffff0000u);
    f[4 * i + 2] = __builtin_bit_cast(float, y << 16);
    f[4 * i + 3] = __builtin_bit_cast(float, y & 0xffff0000u);
  }
}

// grid (nsplit, Hkv, B), 256 threads; the partials of decode_attn_split_kernel.  k / v: e4m3fn bytes (strides in bytes), ksc / vsc: the
// fp32 scale of (b, token, hkv) (strides in elements)
template <int D, int G>
__global__ __launch_bounds__(256) void decode_attn_split_kv8_kernel(const bf16_t* __restrict__ q, long q_bs, const uint8_t* __restrict__ k,
                                                                    long k_bs, long k_ts, const float* __restrict__ ksc, long ks_bs, long ks_ts,
                                                                    const uint8_t* __restrict__ v, long v_bs, long v_ts,
                                                                    const float* __restrict__ vsc, long vs_bs, long vs_ts,
                                                                    const int* __restrict__ kv_len, const int* __restrict__ cache_row,
                                                                    int Smax, int window, float scale, float* __restrict__ ws, int Hkv) {
  constexpr int LPK = D <= 32 ? 2 : (D <= 64 ? 4 : 8);          // lanes per key row (16-byte vectors of 16 elements; D = 96 leaves 2 of 8 idle)
  constexpr int KPB = 256 / LPK;                                 // key rows per block pass
  __shared__ float sc[G][DA_CHMAX];
  __shared__ float red[4][G][D];
  __shared__ float ml[G][2];
  const int hkv = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sl = tid % LPK, ko = tid / LPK, e = sl * 16;
  const bool act = e < D;
  int s0, cnt, cb;
  float* out = da_split_range<D, G>(kv_len, cache_row, Smax, window, ws, Hkv, s0, cnt, cb);
  const uint8_t* kb = k + (long)cb * k_bs + (long)hkv * D + e;
  const uint8_t* vb = v + (long)cb * v_bs + (long)hkv * D + e;
  const float* ksb = ksc + (long)cb * ks_bs + hkv;
  const float* vsb = vsc + (long)cb * vs_bs + hkv;
  {
    float qf[G][16];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        bf16x8 qv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (act) qv = *(const bf16x8*)(q + (long)b * q_bs + (long)(hkv * G + g) * D + e + u * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[g][u * 8 + j] = bf2f((bf16_t)qv[j]) * (scale * DA_LOG2E);
      }
    // scores (log2 domain) -> LDS
    for (int j0 = 0; j0 < cnt; j0 += 2 * KPB) {                   // two key rows per lane and pass: both loads are issued before either converts
      u32x4 kq[2];
      float ksj[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = j0 + u * KPB + ko;
        kq[u] = u32x4{0, 0, 0, 0};
        ksj[u] = 0.f;
        if (act && j < cnt) kq[u] = *(const u32x4*)(kb + (long)(s0 + j) * k_ts);
        if (sl == 0 && j < cnt) ksj[u] = ksb[(long)(s0 + j) * ks_ts];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = j0 + u * KPB + ko;
        float kf[16];
        da8_cvt(kq[u], kf);
        float d[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float a = 0.f;
#pragma unroll
          for (int x = 0; x < 16; ++x) a += qf[g][x] * kf[x];
#pragma unroll
          for (int o = LPK / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
          d[g] = a * ksj[u];                                       // the key's scale on the finished dot product
        }
        if (sl == 0 && j < cnt)
#pragma unroll
          for (int g = 0; g < G; ++g) sc[g][j] = d[g];
      }
    }
  }
  da_softmax<G>(sc, ml, cnt, w, lane);
  // P V
  float acc[G][16];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[g][x] = 0.f;
  for (int j0 = 0; j0 < cnt; j0 += 2 * KPB) {
    u32x4 vq[2];
    float vsj[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = j0 + u * KPB + ko;
      vq[u] = u32x4{0, 0, 0, 0};
      vsj[u] = 0.f;
      if (act && j < cnt) {
        vq[u] = *(const u32x4*)(vb + (long)(s0 + j) * v_ts);
        vsj[u] = vsb[(long)(s0 + j) * vs_ts];
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = j0 + u * KPB + ko;
      if (act && j < cnt) {
        float vf[16];
        da8_cvt(vq[u], vf);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float pj = sc[g][j] * vsj[u];                      // the value row's scale on p_j
#pragma unroll
          for (int x = 0; x < 16; ++x) acc[g][x] += pj * vf[x];
        }
      }
    }
  }
  da_reduce_store<D, G, 16, LPK>(acc, red, ml, out, cnt, e, act, w, lane);
}

// ---------------------------------------------------------------- host side ---------------
// What differs between the three GEMM entry points: their wording, the format's divisibility rules, its chunk and its kernels
struct DgFormat {
  const char* name;                          // the entry point, for the messages
  const char* wide_name;                     // its wide (M <= 64) entry point
  const char* operands;                      // the pointers that must not be null, as the message lists them
  const char* m_hint;                        // closes the M range of the message
  const char* rule;                          // the shape rule, as the message states it
  int kchunk;                                // the split rule's chunk
  int kmul, ldwmul, kper;                    // K, ldw must be multiples of kmul, ldwmul; ldw >= K / kper
  bool rowscale, blocks;                     // needs w_scale | E and lde >= K / 32
  void (*kernel[2])(DecGemmArgs);            // without | with the norm prologue
  void (*wide[2][3])(DecGemmArgs);           // 17 <= M <= 64: the same for 2 | 3 | 4 A tiles of 16 rows
};
#define DG_WIDE(K) {{K<false, 2>, K<false, 3>, K<false, 4>}, {K<true, 2>, K<true, 3>, K<true, 4>}}
static const DgFormat DG_BF16 = {"vp_decode_gemm", "vp_decode_gemm_wide", "A / W / C", "; 17 <= M <= 64: vp_decode_gemm_wide; larger M: vp_gemm_bf16",
                                 "K, lda, ldw multiples of 8, lda / ldw >= K", DG_KCHUNK, 8, 8, 1, false, false,
                                 {decode_gemm_kernel<false>, decode_gemm_kernel<true>}, DG_WIDE(decode_gemm_wide_kernel)};
static const DgFormat DG_W8 = {"vp_decode_gemm_w8", "vp_decode_gemm_w8_wide", "A / W / w_scale / C", "; 17 <= M <= 64: vp_decode_gemm_w8_wide",
                               "K, ldw multiples of 16, lda of 8, lda / ldw >= K", DG8_KCHUNK, 16, 16, 1, true, false,
                               {decode_gemm_w8_kernel<false>, decode_gemm_w8_kernel<true>}, DG_WIDE(decode_gemm_w8_wide_kernel)};
static const DgFormat DG_W4 = {"vp_decode_gemm_w4", "vp_decode_gemm_w4_wide", "A / W / E (block scales) / C",
                               "; 17 <= M <= 64: vp_decode_gemm_w4_wide",
                               "K a multiple of 32, ldw (bytes) of 16, lda of 8, lda >= K, ldw >= K / 2, lde >= K / 32", DG4_KCHUNK, 32, 16, 2,
                               false, true, {decode_gemm_w4_kernel<false>, decode_gemm_w4_kernel<true>}, DG_WIDE(decode_gemm_w4_wide_kernel)};
#undef DG_WIDE

static long dg_workspace_bytes(int M, int N, int K, int epilogue, int kchunk) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int ks = dg_ksplit(N, K, epilogue, kchunk);
  return ks > 1 ? (long)ks * M * N * (long)sizeof(float) : 0;
}

// the three GEMM entry points and their wide forms (M <= 64; at M <= 16 they launch the same kernel as their parents): checks, the main
// kernel and, where K is split, the combine
static int dg_run(const DgFormat& f, bool wide, int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* w_scale,
                  const void* E, long lde, void* C, long ldc, const void* residual, long ldr, const void* norm_w, float eps, int epilogue,
                  int out_f32, float* workspace, hipStream_t stream) {
  const char* name = wide ? f.wide_name : f.name;
  VP_REQUIRE(A && W && C && (!f.rowscale || w_scale) && (!f.blocks || E), VP_ERR_BAD_ARG, "%s: null %s", name, f.operands);
  VP_REQUIRE(M >= 1 && M <= (wide ? 64 : 16), VP_ERR_UNSUPPORTED_SHAPE, "%s: M = %d (1 <= M <= %d%s)", name, M, wide ? 64 : 16,
             wide ? "" : f.m_hint);
  char lde_s[40] = "";
  if (f.blocks) snprintf(lde_s, sizeof(lde_s), ", lde = %ld", lde);
  VP_REQUIRE(N > 0 && K > 0 && K % f.kmul == 0 && lda % 8 == 0 && ldw % f.ldwmul == 0 && lda >= K && ldw >= K / f.kper &&
             (!f.blocks || lde >= K / 32), VP_ERR_UNSUPPORTED_SHAPE, "%s: N = %d, K = %d, lda = %ld, ldw = %ld%s (%s)", name, N, K, lda,
             ldw, lde_s, f.rule);
  VP_REQUIRE(((((uintptr_t)A) | ((uintptr_t)W) | (uintptr_t)(norm_w ? norm_w : A)) & 15) == 0, VP_ERR_UNSUPPORTED_SHAPE,
             "%s: A, W and norm_w must be 16-byte aligned", name);
  const bool swiglu = epilogue == VP_EPI_SWIGLU_IL || epilogue == VP_EPI_SWIGLU_HALVES;
  VP_REQUIRE(epilogue == VP_EPI_NONE || swiglu, VP_ERR_BAD_ARG, "%s: epilogue %d (0 none | 4 SwiGLU interleaved | 5 SwiGLU halves)", name,
             epilogue);
  VP_REQUIRE(!swiglu || (N % 16 == 0 && !out_f32 && !residual), VP_ERR_UNSUPPORTED_SHAPE,
             "%s: SwiGLU needs N %% 16 == 0, bf16 output and no residual (N = %d)", name, N);
  VP_REQUIRE(!(out_f32 && residual), VP_ERR_BAD_ARG, "%s: residual epilogue writes bf16 only", name);
  VP_REQUIRE(ldc >= (swiglu ? N / 2 : N) && (!residual || ldr >= N), VP_ERR_BAD_ARG, "%s: ldc / ldr too small", name);
  const int ks = dg_ksplit(N, K, epilogue, f.kchunk);
  VP_REQUIRE(ks == 1 || workspace, VP_ERR_BAD_ARG, "%s: this shape splits K %d ways and needs %s_workspace_bytes() of workspace (got NULL)",
             name, ks, name);
  const DecGemmArgs p{(const bf16_t*)A, (const bf16_t*)W, C, (const bf16_t*)residual, (const bf16_t*)norm_w, workspace,
                      M, N, K, K / ks, epilogue, out_f32 ? 1 : 0, ks, lda, ldw, ldc, ldr, eps, w_scale, (const uint8_t*)E, lde};
  const auto kernel = M <= 16 ? f.kernel[norm_w != nullptr] : f.wide[norm_w != nullptr][(M - 17) / 16];
  hipLaunchKernelGGL(kernel, dim3(swiglu ? N / 16 : (N + 15) / 16, ks), dim3(DG_THREADS), 0, stream, p);
  if (ks > 1) {
    const long nout = (long)M * (swiglu ? N / 2 : N);
    hipLaunchKernelGGL(decode_gemm_combine_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, stream, p);
  }
  return vp_check_launch(name);
}

// the two attention entry points: everything but the format's own stride / alignment rule
static int da_check(const char* name, bool pointers, const float* workspace, int B, int Hq, int Hkv, int D, int Smax, int window, int nsplit) {
  VP_REQUIRE(pointers, VP_ERR_BAD_ARG, "%s: null pointer", name);
  VP_REQUIRE(workspace, VP_ERR_BAD_ARG, "%s: workspace is NULL (vp_decode_attn_workspace_bytes)", name);
  VP_REQUIRE(B > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Smax > 0 && window >= 0, VP_ERR_BAD_ARG,
             "%s: bad sizes (B %d, Hq %d, Hkv %d, Smax %d)", name, B, Hq, Hkv, Smax);
  const int G = Hq / Hkv;
  VP_REQUIRE(D == 32 || D == 64 || D == 96 || D == 128, VP_ERR_UNSUPPORTED_SHAPE, "%s: head_dim %d (32 | 64 | 96 | 128)", name, D);
  VP_REQUIRE(G == 1 || G == 2 || G == 4 || G == 8, VP_ERR_UNSUPPORTED_SHAPE, "%s: Hq / Hkv = %d (1 | 2 | 4 | 8)", name, G);
  VP_REQUIRE(nsplit >= 1 && nsplit <= 1024 && (long)nsplit * DA_CHMAX >= Smax, VP_ERR_UNSUPPORTED_SHAPE,
             "%s: nsplit %d must cover Smax %d with at most %d keys per split", name, nsplit, Smax, DA_CHMAX);
  return VP_OK;
}

// launch(DA_INT<D>, DA_INT<G>) for the head_dim and group size da_check admitted: the instantiation table of both split kernels
template <int V> struct DA_INT { static constexpr int value = V; };
template <int D, class F>
static void da_dispatch_g(int G, F launch) {
  switch (G) {
    case 1: launch(DA_INT<D>{}, DA_INT<1>{}); break;
    case 2: launch(DA_INT<D>{}, DA_INT<2>{}); break;
    case 4: launch(DA_INT<D>{}, DA_INT<4>{}); break;
    default: launch(DA_INT<D>{}, DA_INT<8>{}); break;
  }
}
template <class F>
static void da_dispatch(int D, int G, F launch) {
  switch (D) {
    case 32: da_dispatch_g<32>(G, launch); break;
    case 64: da_dispatch_g<64>(G, launch); break;
    case 96: da_dispatch_g<96>(G, launch); break;
    default: da_dispatch_g<128>(G, launch); break;
  }
}

// the append and attention entry points and their *_rows siblings: checks and launches; cache_row null = the plain entry points
static int rope_append_run(const char* name, int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq,
                           void* k_cache, long k_bs, long k_ts, void* v_cache, long v_bs, long v_ts, const float* cos_t, const float* sin_t,
                           const int* pos, const int* cache_row, int Smax, hipStream_t stream) {
  VP_REQUIRE(qkv && q_out && k_cache && v_cache && cos_t && sin_t && pos, VP_ERR_BAD_ARG, "%s: null pointer", name);
  VP_REQUIRE(B > 0 && Hq > 0 && Hkv > 0 && Smax > 0, VP_ERR_BAD_ARG, "%s: bad sizes", name);
  VP_REQUIRE(D % 16 == 0 && ldqkv % 8 == 0 && ldq % 8 == 0 && k_bs % 8 == 0 && k_ts % 8 == 0 && v_bs % 8 == 0 && v_ts % 8 == 0,
             VP_ERR_UNSUPPORTED_SHAPE, "%s: head_dim %d must be a multiple of 16, strides multiples of 8", name, D);
  const long total = (long)B * ((Hq + Hkv) * (D / 16) + Hkv * (D / 8));
  hipLaunchKernelGGL(decode_rope_append_kernel, dim3((unsigned)min(2048L, (total + 255) / 256)), dim3(256), 0, stream,
                     (const bf16_t*)qkv, ldqkv, (bf16_t*)q_out, ldq, (bf16_t*)k_cache, k_bs, k_ts, (bf16_t*)v_cache, v_bs, v_ts,
                     cos_t, sin_t, pos, cache_row, B, Hq, Hkv, D, Smax);
  return vp_check_launch(name);
}

static int attn_run(const char* name, int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts,
                    const void* v, long v_bs, long v_ts, void* o, long o_bs, const int* kv_len, const int* cache_row, int window,
                    float scale, int nsplit, float* workspace, hipStream_t stream) {
  if (const int rc = da_check(name, q && k && v && o && kv_len, workspace, B, Hq, Hkv, D, Smax, window, nsplit)) return rc;
  VP_REQUIRE(q_bs % 8 == 0 && k_bs % 8 == 0 && k_ts % 8 == 0 && v_bs % 8 == 0 && v_ts % 8 == 0 &&
             ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) == 0,
             VP_ERR_UNSUPPORTED_SHAPE, "%s: strides must be multiples of 8 elements, bases 16-byte aligned", name);
  da_dispatch(D, Hq / Hkv, [&](auto d, auto g) {
    hipLaunchKernelGGL((decode_attn_split_kernel<d.value, g.value>), dim3(nsplit, Hkv, B), dim3(256), 0, stream, (const bf16_t*)q, q_bs,
                       (const bf16_t*)k, k_bs, k_ts, (const bf16_t*)v, v_bs, v_ts, kv_len, cache_row, Smax, window, scale, workspace, Hkv);
  });
  hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(Hq, B), dim3(D), 0, stream, workspace, (bf16_t*)o, o_bs, Hkv, Hq / Hkv, D, nsplit);
  return vp_check_launch(name);
}

static int rope_append_kv8_run(const char* name, int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq,
                               void* k_bytes, long k_bs, long k_ts, void* v_bytes, long v_bs, long v_ts, float* k_scale, long ks_bs,
                               long ks_ts, float* v_scale, long vs_bs, long vs_ts, void* k_deq, long kd_bs, long kd_ts, void* v_deq,
                               long vd_bs, long vd_ts, const float* cos_t, const float* sin_t, const int* pos, const int* cache_row,
                               int Smax, hipStream_t stream) {
  VP_REQUIRE(qkv && q_out && cos_t && sin_t && pos, VP_ERR_BAD_ARG, "%s: null pointer", name);
  const bool bytes = k_bytes != nullptr, deq = k_deq != nullptr;
  VP_REQUIRE(bytes == (v_bytes != nullptr) && bytes == (k_scale != nullptr) && bytes == (v_scale != nullptr) && deq == (v_deq != nullptr),
             VP_ERR_BAD_ARG, "%s: k / v bytes and scales go together, k / v bf16 destinations go together", name);
  VP_REQUIRE(bytes || deq, VP_ERR_BAD_ARG, "%s: neither a byte nor a bf16 destination", name);
  VP_REQUIRE(B > 0 && Hq > 0 && Hkv > 0 && Smax > 0, VP_ERR_BAD_ARG, "%s: bad sizes", name);
  VP_REQUIRE(D % 16 == 0 && D >= 16 && D <= 128 && ldqkv % 8 == 0 && ldq % 8 == 0 && ((((uintptr_t)qkv) | ((uintptr_t)q_out)) & 15) == 0,
             VP_ERR_UNSUPPORTED_SHAPE, "%s: head_dim %d must be a multiple of 16 (at most 128), strides multiples of 8", name, D);
  VP_REQUIRE(!bytes || (k_bs % 8 == 0 && k_ts % 8 == 0 && v_bs % 8 == 0 && v_ts % 8 == 0 &&
                        ((((uintptr_t)k_bytes) | ((uintptr_t)v_bytes)) & 7) == 0),
             VP_ERR_UNSUPPORTED_SHAPE, "%s: byte strides must be multiples of 8, byte bases 8-byte aligned", name);
  VP_REQUIRE(!deq || (kd_bs % 8 == 0 && kd_ts % 8 == 0 && vd_bs % 8 == 0 && vd_ts % 8 == 0 &&
                      ((((uintptr_t)k_deq) | ((uintptr_t)v_deq)) & 15) == 0),
             VP_ERR_UNSUPPORTED_SHAPE, "%s: bf16 strides must be multiples of 8, bf16 bases 16-byte aligned", name);
  const int lph = D <= 32 ? 2 : (D <= 64 ? 4 : 8);
  const long total = (long)B * (Hq + 2 * Hkv) * lph;
  const KvDst kd{(uint8_t*)k_bytes, k_bs, k_ts, k_scale, ks_bs, ks_ts, (bf16_t*)k_deq, kd_bs, kd_ts};
  const KvDst vd{(uint8_t*)v_bytes, v_bs, v_ts, v_scale, vs_bs, vs_ts, (bf16_t*)v_deq, vd_bs, vd_ts};
  hipLaunchKernelGGL(decode_rope_append_kv8_kernel, dim3((unsigned)min(2048L, (total + 255) / 256)), dim3(256), 0, stream,
                     (const bf16_t*)qkv, ldqkv, (bf16_t*)q_out, ldq, kd, vd, cos_t, sin_t, pos, cache_row, B, Hq, Hkv, D, Smax, lph);
  return vp_check_launch(name);
}

static int attn_kv8_run(const char* name, int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs,
                        long k_ts, const float* k_scale, long ks_bs, long ks_ts, const void* v, long v_bs, long v_ts, const float* v_scale,
                        long vs_bs, long vs_ts, void* o, long o_bs, const int* kv_len, const int* cache_row, int window, float scale,
                        int nsplit, float* workspace, hipStream_t stream) {
  if (const int rc = da_check(name, q && k && v && k_scale && v_scale && o && kv_len, workspace, B, Hq, Hkv, D, Smax, window, nsplit))
    return rc;
  VP_REQUIRE(q_bs % 8 == 0 && k_bs % 16 == 0 && k_ts % 16 == 0 && v_bs % 16 == 0 && v_ts % 16 == 0 &&
             ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) == 0,
             VP_ERR_UNSUPPORTED_SHAPE, "%s: q stride must be a multiple of 8 elements, k / v strides of 16 bytes, bases 16-byte aligned", name);
  da_dispatch(D, Hq / Hkv, [&](auto d, auto g) {
    hipLaunchKernelGGL((decode_attn_split_kv8_kernel<d.value, g.value>), dim3(nsplit, Hkv, B), dim3(256), 0, stream, (const bf16_t*)q, q_bs,
                       (const uint8_t*)k, k_bs, k_ts, k_scale, ks_bs, ks_ts, (const uint8_t*)v, v_bs, v_ts, v_scale, vs_bs, vs_ts, kv_len,
                       cache_row, Smax, window, scale, workspace, Hkv);
  });
  hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(Hq, B), dim3(D), 0, stream, workspace, (bf16_t*)o, o_bs, Hkv, Hq / Hkv, D, nsplit);
  return vp_check_launch(name);
}

extern "C" {

int vp_add_i32(long n, int* x, int delta, hipStream_t stream) {
  VP_REQUIRE(x && n > 0 && n <= (1L << 24), VP_ERR_BAD_ARG, "vp_add_i32: bad args (n = %ld)", n);
  hipLaunchKernelGGL(add_i32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, delta);
  return vp_check_launch("vp_add_i32");
}

long vp_decode_gemm_workspace_bytes(int M, int N, int K, int epilogue) { return dg_workspace_bytes(M, N, K, epilogue, DG_KCHUNK); }

int vp_decode_gemm(int M, int N, int K, const void* A, long lda, const void* W, long ldw, void* C, long ldc, const void* residual,
                   long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace, hipStream_t stream) {
  return dg_run(DG_BF16, false, M, N, K, A, lda, W, ldw, nullptr, nullptr, 0, C, ldc, residual, ldr, norm_w, eps, epilogue, out_f32, workspace, stream);
}

// the wide forms (1 <= M <= 64) need the slabs alone: the norm prologue stays in the kernel, there is no pre-pass scratch
long vp_decode_gemm_wide_workspace_bytes(int M, int N, int K, int epilogue) { return dg_workspace_bytes(M, N, K, epilogue, DG_KCHUNK); }

int vp_decode_gemm_wide(int M, int N, int K, const void* A, long lda, const void* W, long ldw, void* C, long ldc, const void* residual,
                        long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace, hipStream_t stream) {
  return dg_run(DG_BF16, true, M, N, K, A, lda, W, ldw, nullptr, nullptr, 0, C, ldc, residual, ldr, norm_w, eps, epilogue, out_f32, workspace, stream);
}

int vp_quant_rows_e4m3(int N, int K, void* W, long ldw, void* Q, long ldq, float* scale, int writeback, hipStream_t stream) {
  VP_REQUIRE(W && Q && scale, VP_ERR_BAD_ARG, "vp_quant_rows_e4m3: null W / Q / scale");
  VP_REQUIRE(N > 0 && K > 0 && ldw >= K && ldq >= K, VP_ERR_BAD_ARG, "vp_quant_rows_e4m3: N = %d, K = %d, ldw = %ld, ldq = %ld (ld >= K)", N, K,
             ldw, ldq);
  VP_REQUIRE(K % 8 == 0 && ldw % 8 == 0 && ldq % 8 == 0 && (((uintptr_t)W) & 15) == 0 && (((uintptr_t)Q) & 7) == 0, VP_ERR_UNSUPPORTED_SHAPE,
             "vp_quant_rows_e4m3: K, ldw, ldq must be multiples of 8 (K = %d), W 16-byte and Q 8-byte aligned", K);
  hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3((unsigned)N), dim3(256), 0, stream, (bf16_t*)W, ldw, (uint8_t*)Q, ldq, scale, K,
                     writeback ? 1 : 0);
  return vp_check_launch("vp_quant_rows_e4m3");
}

long vp_decode_gemm_w8_workspace_bytes(int M, int N, int K, int epilogue) { return dg_workspace_bytes(M, N, K, epilogue, DG8_KCHUNK); }

int vp_decode_gemm_w8(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* w_scale, void* C, long ldc,
                      const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace,
                      hipStream_t stream) {
  return dg_run(DG_W8, false, M, N, K, A, lda, W, ldw, w_scale, nullptr, 0, C, ldc, residual, ldr, norm_w, eps, epilogue, out_f32, workspace, stream);
}

long vp_decode_gemm_w8_wide_workspace_bytes(int M, int N, int K, int epilogue) { return dg_workspace_bytes(M, N, K, epilogue, DG8_KCHUNK); }

int vp_decode_gemm_w8_wide(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* w_scale, void* C, long ldc,
                           const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace,
                           hipStream_t stream) {
  return dg_run(DG_W8, true, M, N, K, A, lda, W, ldw, w_scale, nullptr, 0, C, ldc, residual, ldr, norm_w, eps, epilogue, out_f32, workspace, stream);
}

int vp_quant_blocks_mxfp4(int N, int K, void* W, long ldw, void* Q, long ldq, void* E, long lde, int writeback, hipStream_t stream) {
  VP_REQUIRE(W && Q && E, VP_ERR_BAD_ARG, "vp_quant_blocks_mxfp4: null W / Q / E");
  VP_REQUIRE(N > 0 && K > 0 && ldw >= K && ldq >= K / 2 && lde >= K / 32, VP_ERR_BAD_ARG,
             "vp_quant_blocks_mxfp4: N = %d, K = %d, ldw = %ld, ldq = %ld, lde = %ld (ldw >= K, ldq >= K / 2, lde >= K / 32)", N, K, ldw, ldq, lde);
  VP_REQUIRE(K % 32 == 0 && ldw % 8 == 0 && ldq % 16 == 0 && ((((uintptr_t)W) | ((uintptr_t)Q)) & 15) == 0, VP_ERR_UNSUPPORTED_SHAPE,
             "vp_quant_blocks_mxfp4: K must be a multiple of 32 (K = %d), ldw of 8, ldq of 16, W and Q 16-byte aligned", K);
  const long blocks = (long)N * (K / 32);
  hipLaunchKernelGGL(quant_blocks_mxfp4_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, stream, (bf16_t*)W, ldw, (uint8_t*)Q,
                     ldq, (uint8_t*)E, lde, N, K, writeback ? 1 : 0);
  return vp_check_launch("vp_quant_blocks_mxfp4");
}

long vp_decode_gemm_w4_workspace_bytes(int M, int N, int K, int epilogue) { return dg_workspace_bytes(M, N, K, epilogue, DG4_KCHUNK); }

int vp_decode_gemm_w4(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const void* E, long lde, void* C, long ldc,
                      const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace,
                      hipStream_t stream) {
  return dg_run(DG_W4, false, M, N, K, A, lda, W, ldw, nullptr, E, lde, C, ldc, residual, ldr, norm_w, eps, epilogue, out_f32, workspace, stream);
}

long vp_decode_gemm_w4_wide_workspace_bytes(int M, int N, int K, int epilogue) { return dg_workspace_bytes(M, N, K, epilogue, DG4_KCHUNK); }

int vp_decode_gemm_w4_wide(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const void* E, long lde, void* C,
                           long ldc, const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32,
                           float* workspace, hipStream_t stream) {
  return dg_run(DG_W4, true, M, N, K, A, lda, W, ldw, nullptr, E, lde, C, ldc, residual, ldr, norm_w, eps, epilogue, out_f32, workspace, stream);
}

int vp_decode_rope_append(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_cache, long k_bs,
                          long k_ts, void* v_cache, long v_bs, long v_ts, const float* cos_t, const float* sin_t, const int* pos, int Smax,
                          hipStream_t stream) {
  return rope_append_run("vp_decode_rope_append", B, Hq, Hkv, D, qkv, ldqkv, q_out, ldq, k_cache, k_bs, k_ts, v_cache, v_bs, v_ts, cos_t,
                         sin_t, pos, nullptr, Smax, stream);
}

int vp_decode_rope_append_rows(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_cache, long k_bs,
                               long k_ts, void* v_cache, long v_bs, long v_ts, const float* cos_t, const float* sin_t, const int* pos,
                               const int* cache_row, int Smax, hipStream_t stream) {
  return rope_append_run("vp_decode_rope_append_rows", B, Hq, Hkv, D, qkv, ldqkv, q_out, ldq, k_cache, k_bs, k_ts, v_cache, v_bs, v_ts,
                         cos_t, sin_t, pos, cache_row, Smax, stream);
}

long vp_decode_attn_workspace_bytes(int B, int Hq, int Hkv, int D, int nsplit) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || D <= 0 || nsplit <= 0) return 0;
  return (long)B * Hq * nsplit * (D + 2) * (long)sizeof(float);
}

int vp_decode_attn(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts, const void* v,
                   long v_bs, long v_ts, void* o, long o_bs, const int* kv_len, int window, float scale, int nsplit, float* workspace,
                   hipStream_t stream) {
  return attn_run("vp_decode_attn", B, Hq, Hkv, D, Smax, q, q_bs, k, k_bs, k_ts, v, v_bs, v_ts, o, o_bs, kv_len, nullptr, window, scale,
                  nsplit, workspace, stream);
}

int vp_decode_attn_rows(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts,
                        const void* v, long v_bs, long v_ts, void* o, long o_bs, const int* kv_len, const int* cache_row, int window,
                        float scale, int nsplit, float* workspace, hipStream_t stream) {
  return attn_run("vp_decode_attn_rows", B, Hq, Hkv, D, Smax, q, q_bs, k, k_bs, k_ts, v, v_bs, v_ts, o, o_bs, kv_len, cache_row, window,
                  scale, nsplit, workspace, stream);
}

int vp_quant_kv_e4m3(long n, int heads, int D, const void* src, long ld_src, void* Q, long ldq, float* scale, long ld_scale, void* deq,
                     long ldd, hipStream_t stream) {
  VP_REQUIRE(src && (Q || deq), VP_ERR_BAD_ARG, "vp_quant_kv_e4m3: null src, or neither a byte (Q) nor a bf16 (deq) destination");
  VP_REQUIRE(!Q == !scale, VP_ERR_BAD_ARG, "vp_quant_kv_e4m3: Q and scale go together (both or neither)");
  VP_REQUIRE(n > 0 && n <= (1L << 24) && heads > 0 && heads <= 1024, VP_ERR_BAD_ARG, "vp_quant_kv_e4m3: n = %ld, heads = %d", n, heads);
  VP_REQUIRE(D >= 8 && D <= 128 && D % 8 == 0, VP_ERR_UNSUPPORTED_SHAPE, "vp_quant_kv_e4m3: head_dim %d (a multiple of 8, at most 128)", D);
  const long row = (long)heads * D;
  VP_REQUIRE(ld_src >= row && ld_src % 8 == 0 && (((uintptr_t)src) & 15) == 0, VP_ERR_UNSUPPORTED_SHAPE,
             "vp_quant_kv_e4m3: ld_src = %ld (>= heads * D = %ld, a multiple of 8), src 16-byte aligned", ld_src, row);
  VP_REQUIRE(!Q || (ldq >= row && ldq % 8 == 0 && (((uintptr_t)Q) & 7) == 0 && ld_scale >= heads && (((uintptr_t)scale) & 3) == 0),
             VP_ERR_UNSUPPORTED_SHAPE, "vp_quant_kv_e4m3: ldq = %ld (>= %ld, a multiple of 8), ld_scale = %ld (>= %d), Q 8-byte aligned", ldq,
             row, ld_scale, heads);
  VP_REQUIRE(!deq || (ldd >= row && ldd % 8 == 0 && (((uintptr_t)deq) & 15) == 0), VP_ERR_UNSUPPORTED_SHAPE,
             "vp_quant_kv_e4m3: ldd = %ld (>= %ld, a multiple of 8), deq 16-byte aligned", ldd, row);
  const int lph = D <= 16 ? 2 : (D <= 32 ? 4 : (D <= 64 ? 8 : 16));
  const long total = n * heads * lph;
  hipLaunchKernelGGL(quant_kv_e4m3_kernel, dim3((unsigned)min(4096L, (total + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)src, ld_src,
                     (uint8_t*)Q, ldq, scale, ld_scale, (bf16_t*)deq, ldd, n, heads, D, lph);
  return vp_check_launch("vp_quant_kv_e4m3");
}

int vp_decode_rope_append_kv8(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_bytes, long k_bs,
                              long k_ts, void* v_bytes, long v_bs, long v_ts, float* k_scale, long ks_bs, long ks_ts, float* v_scale,
                              long vs_bs, long vs_ts, void* k_deq, long kd_bs, long kd_ts, void* v_deq, long vd_bs, long vd_ts,
                              const float* cos_t, const float* sin_t, const int* pos, int Smax, hipStream_t stream) {
  return rope_append_kv8_run("vp_decode_rope_append_kv8", B, Hq, Hkv, D, qkv, ldqkv, q_out, ldq, k_bytes, k_bs, k_ts, v_bytes, v_bs, v_ts,
                             k_scale, ks_bs, ks_ts, v_scale, vs_bs, vs_ts, k_deq, kd_bs, kd_ts, v_deq, vd_bs, vd_ts, cos_t, sin_t, pos,
                             nullptr, Smax, stream);
}

int vp_decode_rope_append_kv8_rows(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_bytes,
                                   long k_bs, long k_ts, void* v_bytes, long v_bs, long v_ts, float* k_scale, long ks_bs, long ks_ts,
                                   float* v_scale, long vs_bs, long vs_ts, void* k_deq, long kd_bs, long kd_ts, void* v_deq, long vd_bs,
                                   long vd_ts, const float* cos_t, const float* sin_t, const int* pos, const int* cache_row, int Smax,
                                   hipStream_t stream) {
  return rope_append_kv8_run("vp_decode_rope_append_kv8_rows", B, Hq, Hkv, D, qkv, ldqkv, q_out, ldq, k_bytes, k_bs, k_ts, v_bytes, v_bs,
                             v_ts, k_scale, ks_bs, ks_ts, v_scale, vs_bs, vs_ts, k_deq, kd_bs, kd_ts, v_deq, vd_bs, vd_ts, cos_t, sin_t,
                             pos, cache_row, Smax, stream);
}

int vp_decode_attn_kv8(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts,
                       const float* k_scale, long ks_bs, long ks_ts, const void* v, long v_bs, long v_ts, const float* v_scale, long vs_bs,
                       long vs_ts, void* o, long o_bs, const int* kv_len, int window, float scale, int nsplit, float* workspace,
                       hipStream_t stream) {
  return attn_kv8_run("vp_decode_attn_kv8", B, Hq, Hkv, D, Smax, q, q_bs, k, k_bs, k_ts, k_scale, ks_bs, ks_ts, v, v_bs, v_ts, v_scale,
                      vs_bs, vs_ts, o, o_bs, kv_len, nullptr, window, scale, nsplit, workspace, stream);
}

int vp_decode_attn_kv8_rows(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts,
                            const float* k_scale, long ks_bs, long ks_ts, const void* v, long v_bs, long v_ts, const float* v_scale,
                            long vs_bs, long vs_ts, void* o, long o_bs, const int* kv_len, const int* cache_row, int window, float scale,
                            int nsplit, float* workspace, hipStream_t stream) {
  return attn_kv8_run("vp_decode_attn_kv8_rows", B, Hq, Hkv, D, Smax, q, q_bs, k, k_bs, k_ts, k_scale, ks_bs, ks_ts, v, v_bs, v_ts,
                      v_scale, vs_bs, vs_ts, o, o_bs, kv_len, cache_row, window, scale, nsplit, workspace, stream);
}

int vp_decode_accept(int B, int n, const int* next, int* tok, int* base_pos, int* pos, int* kv_len, int* n_acc, hipStream_t stream) {
  VP_REQUIRE(next && tok && base_pos && pos && kv_len && n_acc, VP_ERR_BAD_ARG, "vp_decode_accept: null pointer");
  VP_REQUIRE(B > 0 && n >= 0 && (long)B * (n + 1) <= (1L << 24), VP_ERR_BAD_ARG, "vp_decode_accept: bad sizes (B %d, n %d)", B, n);
  hipLaunchKernelGGL(decode_accept_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, next, tok, base_pos, pos, kv_len, n_acc, B,
                     n);
  return vp_check_launch("vp_decode_accept");
}

}  // extern "C"
