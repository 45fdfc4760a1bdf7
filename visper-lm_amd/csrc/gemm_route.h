// Which GEMM kernel a call runs, on which grid: the decision of vp_gemm_bf16 and the grid / c_nt rules its sibling entry points share, as
// functions of plain values (no HIP type, no pointer: a host compiler builds this file, so the routing can be checked without a GPU).
// gemm.hip maps the kernel id to the launch (gemm_launch).
#pragma once

enum { EPI_NONE = 0, EPI_GELU = 1, EPI_QUICK_GELU = 2, EPI_RELU = 3 };

// vp_gemm_bf16's kernel selector (`force_generic` in include/visper_hip.h, which describes each code)
enum GemmSel { SEL_AUTO = 0, SEL_GENERIC = 1, SEL_NT128 = 2, SEL_NT256 = 3, SEL_P8 = 7, SEL_W4 = 8, SEL_PH4 = 13, SEL_W4G = 14 };
static inline bool gemm_sel_known(int s) {
  return s == SEL_AUTO || s == SEL_GENERIC || s == SEL_NT128 || s == SEL_NT256 || s == SEL_P8 || s == SEL_W4 || s == SEL_PH4 || s == SEL_W4G;
}

// rows of gemm_launch's table; out_f32 picks the fp32-output instantiation of a row that has one
enum GemmKernel {
  GK_NONE = -1, // no kernel takes the shape
  GK_W4,        // gemm_nt_256w4<f32>: one wave per SIMD, lean
  GK_W4G,       // gemm_nt_256w4<false, 1>: its general variant (bias / activation / residual / row scale / RoPE, M tail)
  GK_W4F,       // gemm_nt_256w4<false, 2>: lean + RMSNorm-fold features (row scale, sum of squares)
  GK_P8,        // gemm_nt_256p8<f32>: 8-phase ping-pong
  GK_PH4,       // gemm_nt_256p8<false, true>: 4 phases per K-tile
  GK_NT256,     // gemm_nt_256<f32>: the plain persistent 256-tile kernel
  GK_NT128,     // gemm_nt_128<f32>
  GK_GENERIC,   // gemm_nt_generic<f32>
  GK_TN,        // gemm_tn_256p8<f32>
};

struct GemmProblem {
  int M, N, K;
  long lda, ldb, ldc, ldr;
  unsigned a_al, b_al, c_al, bias_al, res_al;          // pointer & 15 (0 for a null pointer)
  bool bias, residual;
  int epilogue, out_f32, sel;
  bool sched_ws;
  int w4, w4g, ph4, c_nt;                              // VP_GEMM_W4 / VP_GEMM_W4G / VP_GEMM_PH4 / VP_GEMM_C_NT
  int dbg;                                             // VP_GEMM_DBG flags (0 in the sealed library)
};

struct GemmRoute {
  int kernel;                                          // GemmKernel
  unsigned grid;
  bool sched;                                          // the kernel gets the caller's sched_ws (else NULL: static walk)
  int c_nt;                                            // GemmArgs::c_nt
};

static inline long gemm_big_tiles(int M, int N) { return (long)((M + 255) / 256) * ((N + 255) / 256); }

// persistent 256-tile kernels: one block per CU streaming its output tiles
static inline unsigned gemm_grid_persistent(long big_tiles) { return (unsigned)(big_tiles > 256 ? 256 : big_tiles); }

// the 8-phase kernels: persistent when the K-tile count is even (buffer parity is then the same for every output tile); otherwise one block
// per output tile (debug flag 0x20000 forces that)
static inline unsigned gemm_grid_p8(int K, long big_tiles, int dbg = 0) {
  return (unsigned)(((K / 64) % 2 == 0 && big_tiles > 256 && !(dbg & 0x20000)) ? 256 : big_tiles);
}

// non-temporal bf16 C stores: N <= 8192 (see GemmArgs::c_nt); VP_GEMM_C_NT=0 switches them off (A/B)
static inline int gemm_c_nt(bool out_f32, int N, int c_nt_switch) { return (!out_f32 && N <= 8192 && c_nt_switch != 0) ? 1 : 0; }

// VP_GEMM_W4: 1 (default since round 3) = the one-wave-per-SIMD kernel, 0 = the 8-phase kernel, 2 = the one-wave-per-SIMD kernel only when no
// collective can run beside it (the caller passed no sched_ws)
static inline bool gemm_w4_wanted(int w4, bool sched_ws) { return w4 == 1 || (w4 == 2 && !sched_ws); }

static inline GemmRoute gemm_route(const GemmProblem& q) {
  const int M = q.M, N = q.N, K = q.K, sel = q.sel, epi8 = q.epilogue & 0xff;
  const bool fast = (sel != SEL_GENERIC) && (K % 64 == 0) && (q.lda % 8 == 0) && (q.ldb % 8 == 0) && (q.a_al | q.b_al) == 0;
  const long big_tiles = gemm_big_tiles(M, N);
  const bool res_ok = !q.residual || (q.ldr % 8 == 0 && q.ldr < (1L << 22) && q.res_al == 0);
  const bool w4_ok = fast && M % 256 == 0 && N % 256 == 0 && K % 128 == 0 && (big_tiles >= 192 || sel == SEL_W4) &&
                     !q.bias && epi8 == EPI_NONE && q.c_al == 0 &&
                     (q.out_f32 ? (!q.residual && q.ldc % 4 == 0)
                                : (q.ldc % 8 == 0 && q.ldc < (1L << 22) && res_ok));       // (32-bit byte offsets inside a 128-row sub-tile)
  // The 4-wave kernel walks its tiles statically.  Next to RCCL kernels (world > 1) a CU that a collective holds delays that block's share
  // (tools/gemm_interference.py: up to 1.45x for the launches that overlap a collective); in the PT step that is the handful of GEMMs under the
  // 0.2 GB gradient all-reduce, against 6-10 % on every launch with the 8-phase kernel and its per-XCD tile claims — so the multi-GPU step uses
  // it too (VP_GEMM_W4=0 / VP_GEMM_W4=2 "only when no collective can run beside it" select the 8-phase kernel).
  if (w4_ok && (sel == SEL_W4 || (sel == SEL_AUTO && gemm_w4_wanted(q.w4, q.sched_ws))))
    return {GK_W4, gemm_grid_persistent(big_tiles), false, gemm_c_nt(q.out_f32, N, q.c_nt)};
  // General variant of the 4-wave kernel (round 4; force code 14; VP_GEMM_W4G=0 turns the automatic choice off): bias / activation / residual /
  // row-scale epilogues and an M tail, for the tower, projector, head and DPT launches that used to fall to the 8-phase kernel.
  const bool w4g_ok = fast && !q.out_f32 && N % 256 == 0 && K % 128 == 0 && M >= 256 && q.c_al == 0 && q.ldc % 8 == 0 && q.ldc < (1L << 22) &&
                      q.bias_al == 0 && !(q.residual && epi8 != EPI_NONE) && res_ok;
  // erf-GELU launches stay on the 8-phase kernel: ~50 VALU instructions per element at one wave per SIMD cost more than the K loop gains
  // (ConvNeXt fc1 18432 x 6144 x 1536: 861 -> 800 TF/s; bias / residual launches: 1092 -> 1363, 1062 -> 1440, 892 -> 1101 TF/s)
  if (w4g_ok && (sel == SEL_W4G || (sel == SEL_AUTO && q.w4g == 1 && big_tiles >= 64 && epi8 != EPI_GELU)))     // (tools/vit_w4_probe.py: ahead of the 128-tile kernel from 76 tiles on)
    return {GK_W4G, gemm_grid_persistent(big_tiles), false, 0};
  const bool large = big_tiles >= 192 && M >= 256 && N >= 256;
  if (fast && (sel == SEL_P8 || (sel == SEL_AUTO && large))) {                             // default large-problem kernel
    const unsigned g8 = gemm_grid_p8(K, big_tiles, q.dbg);
    const int c_nt = (gemm_c_nt(q.out_f32, N, q.c_nt) && (long)M * q.ldc * 2 < 0x7fffffffL) ? 1 : 0;
    // VP_GEMM_PH4 (default ON since round 2: in-step A/B on one box, alternating runs: 458.1 / 459.0 ms per step against 461.7 / 462.5 with the
    // 8-phase loop (GEMM 1337 vs 1324 TFLOP/s), bit-identical results; VP_GEMM_PH4=0 selects the 8-phase loop)
    const bool ph4 = !q.out_f32 && q.ph4 != 0 && sel == SEL_AUTO;
    return {ph4 ? GK_PH4 : GK_P8, g8, g8 == 256, c_nt};
  }
  if (fast && sel == SEL_PH4 && !q.out_f32) return {GK_PH4, gemm_grid_p8(K, big_tiles, q.dbg), false, 0};      // 4-phase variant (A/B testing)
  // a forced 8 / 13 / 14 whose kernel refused the shape lands here with the automatic size rule; 3 takes this kernel at any size
  if (fast && sel != SEL_NT128 && (sel == SEL_NT256 || large)) return {GK_NT256, gemm_grid_persistent(big_tiles), false, 0};
  if (fast) return {GK_NT128, (unsigned)(((M + 127) / 128) * ((N + 127) / 128)), false, 0};
  return {GK_GENERIC, (unsigned)(((M + 63) / 64) * ((N + 63) / 64)), false, 0};
}

// vp_gemm_bf16_swiglu (M, N multiples of 256, K of 64, aligned rows: checked by the caller): the one-wave-per-SIMD kernel under the routing of
// vp_gemm_bf16 (the row scale exists there only), else the 8-phase kernel
static inline GemmRoute gemm_route_swiglu(int M, int N, int K, long ldc, long ldc2, long ldaux, bool rowscale, bool sched_ws, int w4, int ph4) {
  const long big_tiles = gemm_big_tiles(M, N);
  if (gemm_w4_wanted(w4, sched_ws) && K % 128 == 0 && big_tiles >= 192 && ldc < (1L << 21) && ldc2 < (1L << 21) && ldaux < (1L << 21))
    return {rowscale ? GK_W4F : GK_W4, gemm_grid_persistent(big_tiles), false, 0};
  if (rowscale) return {GK_NONE, 0, false, 0};
  const unsigned g8 = gemm_grid_p8(K, big_tiles);
  return {ph4 != 0 ? GK_PH4 : GK_P8, g8, g8 == 256, 0};
}
