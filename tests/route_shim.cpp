// extern "C" doors into csrc/gemm_route.h for tests/test_gemm_route_host.py: compiled with the host compiler into a temporary directory and
// loaded with ctypes; nothing here decides anything.
#include "../visper-lm_amd/csrc/gemm_route.h"

extern "C" {

// q: M N K | lda ldb ldc ldr | a_al b_al c_al bias_al res_al | bias residual | epilogue out_f32 sel | sched_ws | w4 w4g ph4 c_nt | dbg  (24 longs)
// out: kernel grid sched c_nt
void route(const long* q, long* out) {
  GemmProblem p;
  p.M = (int)q[0]; p.N = (int)q[1]; p.K = (int)q[2];
  p.lda = q[3]; p.ldb = q[4]; p.ldc = q[5]; p.ldr = q[6];
  p.a_al = (unsigned)q[7]; p.b_al = (unsigned)q[8]; p.c_al = (unsigned)q[9]; p.bias_al = (unsigned)q[10]; p.res_al = (unsigned)q[11];
  p.bias = q[12] != 0; p.residual = q[13] != 0;
  p.epilogue = (int)q[14]; p.out_f32 = (int)q[15]; p.sel = (int)q[16];
  p.sched_ws = q[17] != 0;
  p.w4 = (int)q[18]; p.w4g = (int)q[19]; p.ph4 = (int)q[20]; p.c_nt = (int)q[21];
  p.dbg = (int)q[22];
  const GemmRoute r = gemm_route(p);
  out[0] = r.kernel; out[1] = r.grid; out[2] = r.sched; out[3] = r.c_nt;
}

// many problems in one call (the property grid): q [n][24], out [n][4]
void route_many(long n, const long* q, long* out) {
  for (long i = 0; i < n; ++i) route(q + 24 * i, out + 4 * i);
}

void route_swiglu(long M, long N, long K, long ldc, long ldc2, long ldaux, long rowscale, long sched_ws, long w4, long ph4, long* out) {
  const GemmRoute r = gemm_route_swiglu((int)M, (int)N, (int)K, ldc, ldc2, ldaux, rowscale != 0, sched_ws != 0, (int)w4, (int)ph4);
  out[0] = r.kernel; out[1] = r.grid; out[2] = r.sched; out[3] = r.c_nt;
}

long grid_p8(long K, long big_tiles, long dbg) { return gemm_grid_p8((int)K, big_tiles, (int)dbg); }
long c_nt(long out_f32, long N, long c_nt_switch) { return gemm_c_nt(out_f32 != 0, (int)N, (int)c_nt_switch); }
long sel_known(long s) { return gemm_sel_known((int)s); }
long kernel_id(long i) {      // the enum's values in declaration order, so the test's names cannot drift from the header
  const int ids[] = {GK_NONE, GK_W4, GK_W4G, GK_W4F, GK_P8, GK_PH4, GK_NT256, GK_NT128, GK_GENERIC, GK_TN};
  return (i >= 0 && i < 10) ? ids[i] : -99;
}

}
