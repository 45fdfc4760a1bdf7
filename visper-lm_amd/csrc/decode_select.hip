// Device-side token selection of KV-cached generate(): HF's RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper
// -> TopPLogitsWarper, then greedy or inverse-CDF sampling, one workgroup of 1024 threads per row of fp32 logits (include/visper_hip.h:
// vp_decode_select, the contract).  This file is built WITHOUT -ffast-math (Makefile: decode_select_FLAGS): the penalty and temperature
// divisions are correctly rounded IEEE fp32 divisions, so the scores are reproducible bit for bit on the CPU.
//
// Everything the kernel decides is an integer decision, so the result does not depend on the order in which threads arrive:
//   key     an order-preserving uint32 of the score s (sign flip; -0 counts as +0).  "s >= the k-th largest" and "s_u <= s_v" become
//           comparisons of keys.
//   mass    exp(s - max) * 2^40 truncated to uint64 (the row maximum itself: exactly 2^40).  V <= 2^20, so a row's total stays below 2^60
//           and integer adds are exact in any order.
//   select  radix select over the key, four 8-bit digits from the top: a 256-bin uint64 LDS histogram (integer atomics) of the elements
//           that match the digits found so far, then the first bin at which the running weight exceeds the threshold.  With weight 1 and
//           threshold V - k it returns the k-th largest key (top-k); with the masses of the top-k survivors and threshold
//           floor((1 - top_p) * total) it returns the smallest key whose tail mass exceeds 1 - top_p (top-p).  A thread adds a run of equal
//           digits once: where the digits cluster (the exponent bits) the atomics nearly vanish, where they spread they do not collide.
//   CDF     the same search over the token INDEX instead of the key: kept masses per 4096 tokens (one wave per bin: a plain store, no
//           atomics), per 64 tokens of the bin the target falls into, then a 64-lane prefix sum.  The token is the first, in ascending
//           index order, whose inclusive cumulative mass exceeds floor(u * kept total).
// Every pass after the first reads the row from L2 (a Llama-3 row is 513 KB) and recomputes the score; there is no workspace.
// Greedy without scores_out needs the first pass only: top-k and top-p never remove the maximum.
#include "common.h"

namespace {

constexpr int NT = 1024;                                         // threads per row: 16 waves
constexpr int NW = NT / 64;
constexpr float MASS_ONE = 0x1p40f;

struct SelRow {
  const float* l;                                                // the row's raw logits
  const uint32_t* seen;                                          // the row's bitmap, or nullptr (no penalty)
  float theta, temp;
  int V;
};

__device__ __forceinline__ float sel_score(const SelRow& c, int v) {
  float x = c.l[v];
  if (c.seen && ((c.seen[v >> 5] >> (v & 31)) & 1u)) x = x < 0.f ? x * c.theta : x / c.theta;
  return x / c.temp;
}

__device__ __forceinline__ uint32_t sel_key(float s) {
  if (s == 0.f) s = 0.f;                                         // -0 and +0 compare equal: one key
  const uint32_t u = __builtin_bit_cast(uint32_t, s);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(uint32_t k) {
  return __builtin_bit_cast(float, (k >> 31) ? (k & 0x7fffffffu) : ~k);
}

// the fixed-point softmax numerator; any input bits give a value in [0, 2^40], and the row maximum gives exactly 2^40 (so a total is never 0)
__device__ __forceinline__ unsigned long long sel_mass(float s, uint32_t k, float smax, uint32_t kmax) {
  if (k == kmax) return (unsigned long long)MASS_ONE;
  float e = expf(s - smax);
  if (!(e > 0.f)) return 0ull;                                   // -inf, underflow, NaN
  if (e > 1.f) e = 1.f;
  return (unsigned long long)(e * MASS_ONE);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ unsigned long long wave_scan_u64(unsigned long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

struct SelShared {
  unsigned long long hist[256];
  unsigned long long red[NW];
  unsigned long long below, thr, total;
  int digit, token;
};

enum { THR_GIVEN = 0, THR_TOPK = 1, THR_TOPP = 2, THR_UNIFORM = 3 };

// Wave 0, after a barrier: the first of the 256 bins at which sh.below + (running sum of hist) exceeds the threshold -> sh.digit, and
// sh.below += the bins before it.  mode != THR_GIVEN first derives the threshold from the histogram's total (the first level of a search):
//   THR_TOPK     total - k               (param = k as a float-free integer in `ik`)
//   THR_TOPP     floor((1 - top_p) total)
//   THR_UNIFORM  floor(u total)
// always clamped to total - 1, so a crossing exists.  No crossing (impossible for consistent histograms): the last bin.
__device__ __forceinline__ void sel_find(SelShared& sh, int mode, double frac, int ik) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    unsigned long long h[4], loc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = sh.hist[lane * 4 + j];
      loc += h[j];
    }
    const unsigned long long incl = wave_scan_u64(loc, lane);
    const unsigned long long total = __shfl(incl, 63, 64);
    unsigned long long thr = sh.thr, below = sh.below;
    if (mode != THR_GIVEN) {
      below = 0;
      if (mode == THR_TOPK) thr = total > (unsigned long long)ik ? total - (unsigned long long)ik : 0ull;
      else thr = (unsigned long long)(frac * (double)total);
      if (total > 0 && thr > total - 1) thr = total - 1;
    }
    unsigned long long run = below + incl - loc;
    const bool cross = run <= thr && run + loc > thr;
    const unsigned long long who = __ballot(cross);
    const int first = who ? __ffsll((long long)who) - 1 : 63;
    if (lane == first) {
      int d = 3;
      if (who) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (run + h[j] > thr) { d = j; break; }
          run += h[j];
        }
      }
      sh.digit = lane * 4 + d;
      sh.below = run;
      sh.thr = thr;
      sh.total = total;
    }
  }
}

// The smallest key K among the eligible elements (key >= lo) whose weight up to and including K exceeds the threshold of `mode`
// (THR_TOPK: weight 1; THR_TOPP: the masses).  Four passes over the row.  All threads return K.
__device__ uint32_t sel_radix(SelShared& sh, const SelRow& c, int mode, double frac, int ik, uint32_t lo, float smax, uint32_t kmax) {
  uint32_t prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    if (threadIdx.x < 256) sh.hist[threadIdx.x] = 0;
    __syncthreads();
    int cur = -1;
    unsigned long long acc = 0;
    for (int v = threadIdx.x; v < c.V; v += NT) {
      const float s = sel_score(c, v);
      const uint32_t k = sel_key(s);
      if (k < lo || (k & himask) != prefix) continue;
      const int d = (k >> shift) & 255;
      const unsigned long long w = mode == THR_TOPK ? 1ull : sel_mass(s, k, smax, kmax);
      if (d != cur) {
        if (acc) atomicAdd(&sh.hist[cur], acc);
        cur = d;
        acc = 0;
      }
      acc += w;
    }
    if (acc) atomicAdd(&sh.hist[cur], acc);
    __syncthreads();
    sel_find(sh, shift == 24 ? mode : THR_GIVEN, frac, ik);
    __syncthreads();
    prefix |= (uint32_t)sh.digit << shift;
  }
  return prefix;
}

// The sampled token: the first index, ascending, whose inclusive cumulative kept mass exceeds floor(u * kept total).  All threads return it.
__device__ int sel_sample(SelShared& sh, const SelRow& c, uint32_t K, float smax, uint32_t kmax, double u, int fallback) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  auto mass_at = [&](int v) -> unsigned long long {
    if (v >= c.V) return 0ull;
    const float s = sel_score(c, v);
    const uint32_t k = sel_key(s);
    return k >= K ? sel_mass(s, k, smax, kmax) : 0ull;
  };
  // level 1: bins of 4096 tokens (V <= 2^20: at most 256), bin b summed by wave b % 16
  for (int b = w; b < 256; b += NW) {
    unsigned long long acc = 0;
    const int base = b << 12;
    if (base < c.V)
      for (int i = 0; i < 64; ++i) acc += mass_at(base + i * 64 + lane);
    acc = wave_sum_u64(acc);
    if (lane == 0) sh.hist[b] = acc;
  }
  __syncthreads();
  sel_find(sh, THR_UNIFORM, u, 0);
  __syncthreads();
  const int base1 = sh.digit << 12;
  // level 2: the 64 bins of 64 tokens of that bin
  for (int b = w; b < 256; b += NW) {
    const unsigned long long acc = b < 64 ? wave_sum_u64(mass_at(base1 + b * 64 + lane)) : 0ull;
    if (lane == 0) sh.hist[b] = acc;
  }
  __syncthreads();
  sel_find(sh, THR_GIVEN, 0., 0);
  __syncthreads();
  const int base2 = base1 + (sh.digit << 6);
  // level 3: the 64 tokens
  if (w == 0) {
    const unsigned long long m = mass_at(base2 + lane);
    const unsigned long long run = sh.below + wave_scan_u64(m, lane) - m;
    const unsigned long long who = __ballot(run <= sh.thr && run + m > sh.thr);
    if (lane == 0) {
      const int t = who ? base2 + __ffsll((long long)who) - 1 : fallback;
      sh.token = t >= 0 && t < c.V ? t : fallback;
    }
  }
  __syncthreads();
  return sh.token;
}

struct SelArgs {
  const float* logits; long ld;
  uint32_t* seen; long seen_ld;
  const float* u; int u_steps;
  const int* eos; int n_eos; int pad;
  int* finished; const int* col; int* tok;
  int* out; long out_ld; int n_out;
  float* scores; long scores_ld;
  int V, do_sample, k;
  float temp, top_p, theta;
};

__global__ __launch_bounds__(NT) void decode_select_kernel(SelArgs a) {
  __shared__ SelShared sh;
  const int r = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  SelRow c;
  c.l = a.logits + (long)r * a.ld;
  c.seen = a.seen && a.theta != 1.f ? a.seen + (long)r * a.seen_ld : nullptr;     // theta = 1: the penalty is the identity
  c.theta = a.theta;
  c.temp = a.temp;
  c.V = a.V;

  // pass 0: the maximum key and the smallest index that has it (greedy's token; argmax's tie rule)
  unsigned long long best = 0;
  for (int v = threadIdx.x; v < c.V; v += NT) {
    const unsigned long long t = ((unsigned long long)sel_key(sel_score(c, v)) << 32) | (uint32_t)(0x7fffffff - v);
    best = t > best ? t : best;
  }
  best = wave_max_u64(best);
  if (lane == 0) sh.red[w] = best;
  __syncthreads();
  best = sh.red[0];
  for (int i = 1; i < NW; ++i) best = sh.red[i] > best ? sh.red[i] : best;
  const uint32_t kmax = (uint32_t)(best >> 32);
  const float smax = sel_unkey(kmax);
  const int amax = 0x7fffffff - (int)(uint32_t)best;
  int token = amax;

  if (a.do_sample || a.scores) {
    uint32_t K = 0;                                              // kept <=> key >= K
    if (a.k < c.V) K = sel_radix(sh, c, THR_TOPK, 0., a.k, 0u, smax, kmax);
    if (a.top_p < 1.f) {
      const uint32_t Kp = sel_radix(sh, c, THR_TOPP, 1.0 - (double)a.top_p, 0, K, smax, kmax);
      K = Kp > K ? Kp : K;
    }
    if (a.scores) {
      float* so = a.scores + (long)r * a.scores_ld;
      for (int v = threadIdx.x; v < c.V; v += NT) {
        const float s = sel_score(c, v);
        so[v] = sel_key(s) >= K ? s : -__builtin_inff();
      }
    }
    if (a.do_sample) {
      const int ur = a.u_steps > 1 ? min(max(*a.col, 0), a.u_steps - 1) : 0;
      float u = a.u[(long)ur * gridDim.x + r];
      if (!(u >= 0.f)) u = 0.f;
      if (u >= 1.f) u = 0x1.fffffep-1f;
      token = sel_sample(sh, c, K, smax, kmax, (double)u, amax);
    }
  }
  __syncthreads();                                               // every read of the bitmap is done before its one bit is set
  if (threadIdx.x == 0) {
    a.tok[r] = token;
    const int was = a.finished[r];
    const int o = was ? a.pad : token;
    const int cidx = *a.col;
    if (cidx >= 0 && cidx < a.n_out) a.out[(long)r * a.out_ld + cidx] = o;
    int fin = was != 0;
    for (int i = 0; i < a.n_eos; ++i) fin |= a.eos[i] == o;
    a.finished[r] = fin;
    if (a.seen) {
      uint32_t* word = a.seen + (long)r * a.seen_ld + (token >> 5);
      *word = *word | (1u << (token & 31));
    }
  }
}

}  // namespace

extern "C" int vp_decode_select(int R, int V, const float* logits, long ld_logits, int do_sample, float temperature, int top_k, float top_p,
                                float repetition_penalty, uint32_t* seen, const float* u, int u_steps, const int* eos, int n_eos, int pad,
                                int* finished, const int* col, int* tok, int* out, long ld_out, int n_out, float* scores_out,
                                long ld_scores, hipStream_t stream) {
  VP_REQUIRE(logits && finished && col && tok && out, VP_ERR_BAD_ARG, "vp_decode_select: null pointer (logits, finished, col, tok, out)");
  VP_REQUIRE(R >= 1 && R <= (1 << 20) && V >= 1 && V <= (1 << 20), VP_ERR_BAD_ARG,
             "vp_decode_select: bad sizes (R %d, V %d: 1 <= R, V <= 2^20)", R, V);
  VP_REQUIRE(ld_logits >= V && n_out >= 1 && ld_out >= n_out && (!scores_out || ld_scores >= V), VP_ERR_BAD_ARG,
             "vp_decode_select: bad strides (ld_logits %ld, ld_out %ld, n_out %d, ld_scores %ld, V %d)", ld_logits, ld_out, n_out, ld_scores, V);
  VP_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, VP_ERR_BAD_ARG, "vp_decode_select: temperature %g must be > 0 and finite",
             (double)temperature);
  VP_REQUIRE(top_k >= 0, VP_ERR_BAD_ARG, "vp_decode_select: top_k %d must be >= 0 (0 = off)", top_k);
  VP_REQUIRE(top_p > 0.f && top_p <= 1.f, VP_ERR_BAD_ARG, "vp_decode_select: top_p %g must lie in (0, 1] (1 = off)", (double)top_p);
  VP_REQUIRE(repetition_penalty > 0.f && repetition_penalty <= 3.0e38f, VP_ERR_BAD_ARG,
             "vp_decode_select: repetition_penalty %g must be > 0 and finite (1 = off)", (double)repetition_penalty);
  VP_REQUIRE(seen || repetition_penalty == 1.f, VP_ERR_BAD_ARG, "vp_decode_select: repetition_penalty %g needs the seen bitmap",
             (double)repetition_penalty);
  VP_REQUIRE(!do_sample || (u && u_steps >= 1), VP_ERR_BAD_ARG, "vp_decode_select: do_sample needs the uniforms u (u_steps %d >= 1)", u_steps);
  VP_REQUIRE(n_eos >= 0 && n_eos <= 64 && (n_eos == 0 || eos), VP_ERR_BAD_ARG, "vp_decode_select: bad eos list (n_eos %d: 0 .. 64)", n_eos);
  SelArgs a;
  a.logits = logits; a.ld = ld_logits;
  a.seen = seen; a.seen_ld = (V + 31) / 32;
  a.u = do_sample ? u : nullptr; a.u_steps = u_steps;
  a.eos = eos; a.n_eos = n_eos; a.pad = pad;
  a.finished = finished; a.col = col; a.tok = tok;
  a.out = out; a.out_ld = ld_out; a.n_out = n_out;
  a.scores = scores_out; a.scores_ld = ld_scores;
  a.V = V; a.do_sample = do_sample != 0;
  a.k = top_k == 0 ? V : (top_k < V ? top_k : V);                // min(max(top_k, 1), V); off = keep all
  a.temp = temperature; a.top_p = top_p; a.theta = repetition_penalty;
  hipLaunchKernelGGL(decode_select_kernel, dim3((unsigned)R), dim3(NT), 0, stream, a);
  return vp_check_launch("vp_decode_select");
}
