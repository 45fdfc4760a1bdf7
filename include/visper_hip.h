/* visper_hip.h — C ABI of libvisper_hip.so: the MI355X (gfx950) kernels behind the VisPer-LM
 * pre-training step (NTP + per-layer embedding distillation).
 *
 * The reference (SHI-Labs/VisPer-LM) has NO native code and no FFI: every op below replaces a
 * PyTorch/HF call site on the hot path.  Each prototype cites the reference
 * call site it stands in for (paths relative to /root/reference; "HF:" = transformers==4.41.1, the
 * reference's pinned dependency).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - plain pointers + sizes; all tensors are device pointers owned by the caller (PyTorch caching
 *    allocator); the library never allocates, frees or retains device memory — also not for its own bookkeeping: the two kernels that need
 *    device-side counters (dynamic GEMM tile claims, the distillation loss's reduction tree) take them as caller-owned blocks
 *    (`sched_ws`, `counters`).  Only the vp_comm_* communicator object holds state.
 *  - bf16 tensors are `void*` (raw uint16 bit patterns); fp32 are `float*`; ld* = leading dimension in
 *    ELEMENTS; every call is asynchronous on `stream` (a hipStream_t passed as void*).
 *  - return 0 on success, negative VP_ERR_* otherwise; vp_last_error_string() (thread-local) explains.
 *    Nothing throws or aborts across the ABI.
 */
#ifndef VISPER_HIP_H
#define VISPER_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef void* vp_stream_t; /* hipStream_t */

#define VP_OK 0
#define VP_ERR_BAD_ARG (-1)
#define VP_ERR_UNSUPPORTED_SHAPE (-2)
#define VP_ERR_HIP (-3)

/* epilogue / activation kinds */
#define VP_EPI_NONE 0
#define VP_EPI_GELU 1       /* erf GELU: multimodal_projector/builder.py:57, resampler.py:14 */
#define VP_EPI_QUICK_GELU 2 /* HF: CLIPMLP quick_gelu */
#define VP_EPI_RELU 3       /* aux_heads/da_v2_head.py:331-335 build_mlp */

const char* vp_last_error_string(void);
int vp_version(void);
int vp_device_info(int* cu_count, int* wave_size, long* lds_bytes_per_cu);

/* ---- GEMM: C[M,N] = epi(A[M,K] . B[N,K]^T + bias[N]) + residual[M,N]   (bf16 in, fp32 MFMA accumulate)
 * replaces every nn.Linear / F.linear on the path: HF LlamaAttention/LlamaMLP q,k,v,o,gate,up,down
 * (HF modeling_llama.py), CLIP q,k,v,out,fc1,fc2 (HF modeling_clip.py), lm_head (ola_llama.py:121),
 * mm_projector (multimodal_projector/builder.py:53-60), resampler proj_in/to_q/to_kv/to_out/FF/proj_out
 * (multimodal_projector/resampler.py:9-16,40-44,186-190), depth MLPs (aux_heads/da_v2_head.py:439-442).
 * out_f32=1 writes fp32 (used for weight gradients). force_generic: 0 = auto: the one-wave-per-SIMD 256x256 kernel (code 8) for aligned
 * large problems without bias / activation (M, N multiples of 256, K of 128), its general variant (code 14: bias / activation / residual
 * epilogues, any M >= 256) for such launches from 64 tiles on (erf-GELU launches stay on the 8-phase kernel), the 128x128 kernel for small
 * problems, the bounds-checked generic kernel when K%64 != 0 or rows are not 16-B aligned.  1 = generic, 2 = 128-tile, 3 = the simple
 * persistent 256-tile kernel (kept as the A/B reference), 7 = the 256x256 8-phase ping-pong kernel (the auto choice of rounds 1-2),
 * 8 / 14 = see above, 13 = 4-phase variant of the 8-phase kernel.  Every code computes the same result (the tests compare them bit for bit);
 * any other value is VP_ERR_BAD_ARG. */
int vp_gemm_bf16(int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                 const void* bias, const void* residual, long ldr, int epilogue, int out_f32, int force_generic, int* sched_ws,
                 vp_stream_t stream);

/* sched_ws (vp_gemm_bf16, vp_gemm_bf16_swiglu, vp_gemm_tn_bf16): NULL = the persistent kernels walk their tiles statically (single GPU:
 * nothing else runs beside the GEMMs).  Non-NULL = vp_gemm_sched_workspace_bytes() bytes of CALLER-OWNED device memory, zeroed once by the
 * caller: the persistent 8-phase kernels then claim their tiles from per-XCD counters in it, so a CU held by a concurrent kernel (an RCCL
 * collective) only costs its own share instead of stalling the static grid (the reference leaves this to DeepSpeed's stream overlap,
 * scripts/zero2.json "overlap_comm").  A launch leaves the block zeroed again: one block serves every launch of one stream; launches that may
 * overlap (different streams) need different blocks.  The library keeps no pointer after the call returns. */
long vp_gemm_sched_workspace_bytes(void);

/* Fused SwiGLU GEMMs for the decoder MLP (HF LlamaMLP.forward: down_proj(act_fn(gate_proj(x)) * up_proj(x))).  The fused
 * gate/up tensor keeps gate and up interleaved in 8-column chunks (g0..7 | u0..7 | g8..15 | ...), which is also the layout
 * vp_swiglu_fwd / vp_swiglu_bwd use.  mode 1: C[M,N] = A B^T (gate_up) and C2[M,N/2] = silu(gate)*up.  mode 2: d_act = A B^T
 * stays on chip, aux = gate_up[M,2N], C[M,2N] = d_gate_up.  M, N multiples of 256, K of 64; else VP_ERR_UNSUPPORTED_SHAPE.
 * mode 1 with aux != NULL: aux is an fp32 [M] row scale applied to the accumulators (gate_up = bf16(acc * scale): RMSNorm's 1/rms when
 * gamma is folded into the frozen weight); one-wave-per-SIMD kernel only (K % 128 == 0, >= 192 tiles), else VP_ERR_UNSUPPORTED_SHAPE. */
int vp_gemm_bf16_swiglu(int mode, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                        void* C2, long ldc2, const void* aux, long ldaux, int* sched_ws, vp_stream_t stream);

/* Residual GEMM that also emits the next RMSNorm's statistics (replaces: HF LlamaDecoderLayer.forward's `residual + o_proj(...)` /
 * `residual + mlp(...)` followed by a separate pass over the stream for the norm, reached from ola_llama.py:105-115): C[M,N] = A B^T + residual
 * exactly as vp_gemm_bf16, plus sumsq_part[M, N/16] (fp32): per-row sums of squares of the result (fp32, before the last bf16 rounding) over
 * 16-column groups; vp_rstd_from_sumsq finishes them.  One-wave-per-SIMD kernel only: M, N multiples of 256, K of 128, 16-byte aligned
 * rows; otherwise VP_ERR_UNSUPPORTED_SHAPE. */
int vp_gemm_bf16_sumsq(int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc, const void* residual, long ldr,
                       float* sumsq_part, vp_stream_t stream);

/* rstd[row] = rsqrt(sum_j part[row, j] / H + eps) (HF LlamaRMSNorm.forward's variance / rsqrt), fixed summation order.  nparts % 4 == 0. */
int vp_rstd_from_sumsq(int M, int nparts, const float* part, int H, float eps, float* rstd, vp_stream_t stream);

/* QKV projection of a decoder layer with rotate-half RoPE in the GEMM epilogue (replaces: HF LlamaAttention.forward's q/k/v_proj followed by
 * apply_rotary_pos_emb, reached from ola_vlm/model/language_model/ola_llama.py:105-115): C[M,N] = (row_scale (.) A) B^T with the columns
 * < rope_cols (whole 128-wide heads: q and k of the fused qkv weight) rotated exactly as vp_gemm_bf16 + vp_rope would (same rounding points,
 * bit-identical).  cos_t / sin_t: fp32 [S, 64]; pos: int32 [M] position ids or NULL (row % S).  row_scale: fp32 [M] or NULL; it multiplies the
 * fp32 accumulator before the bf16 rounding (RMSNorm's 1/rms when gamma is folded into the frozen weight).  head_dim 128, N % 256 == 0,
 * K % 128 == 0, M >= 256 (any M: the last row tile is range-checked), 16-byte aligned rows; otherwise VP_ERR_UNSUPPORTED_SHAPE. */
int vp_gemm_bf16_rope(int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc, const float* row_scale,
                      int rope_cols, const float* cos_t, const float* sin_t, const int* pos, int S, vp_stream_t stream);

/* Weight gradient without transposes: C[M,N] (+)= A[K,M]^T B[K,N], both operands contraction-major (autograd of nn.Linear,
 * grad_weight = grad_output.t() @ input: A = dY[tokens,out], B = X[tokens,in]).  Same 8-phase kernel structure with transposing
 * LDS reads.  M, N multiples of 256, K of 64, 16-byte aligned rows; else VP_ERR_UNSUPPORTED_SHAPE (the caller transposes and
 * uses vp_gemm_bf16).  out_f32=1 writes fp32; accumulate=1 (fp32 only) adds into C (chunked lm_head gradient). */
int vp_gemm_tn_bf16(int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc, int out_f32,
                    int accumulate, int* sched_ws, vp_stream_t stream);

/* (measurement / development entry points — vp_debug_* — are NOT part of this ABI: include/visper_hip_debug.h, built with -DVP_DEBUG) */

int vp_transpose_bf16(int rows, int cols, const void* in, long ld_in, void* out, long ld_out, vp_stream_t stream);
/* `batch` independent [rows, cols] -> [cols, rows] transposes in ONE launch (matrix b at in + b * batch_stride_in / out + b * batch_stride_out,
 * strides in elements, multiples of 8): the (B, C, 24, 24) segmentation targets re-laid to the prediction's (B, 576, C) order once per step
 * (base_ola_vlm.py:289-320 compares preds [B, C, 24, 24] with targets of the same layout; the loss kernel streams both linearly). */
int vp_transpose_batched_bf16(int batch, int rows, int cols, const void* in, long batch_stride_in, long ld_in, void* out, long batch_stride_out,
                              long ld_out, vp_stream_t stream);

/* ---- norms.  HF LlamaRMSNorm (modeling_llama.py:53-68); nn.LayerNorm in CLIP and the resampler
 * (resampler.py:12,37-38,189).  rstd/mean: fp32 [M] saved for backward. */
int vp_rmsnorm_fwd(int M, int H, const void* x, long ldx, const void* w, float eps, void* y, long ldy, float* rstd,
                   vp_stream_t stream);
int vp_rmsnorm_bwd(int M, int H, const void* dy, const void* x, const void* w, const float* rstd, const void* dres,
                   void* dx, long ld, vp_stream_t stream);
int vp_layernorm_fwd(int M, int H, const void* x, long ldx, const void* w, const void* b, float eps, void* y, long ldy,
                     float* mean, float* rstd, vp_stream_t stream);
int vp_layernorm_bwd_dx(int M, int H, const void* dy, const void* x, const void* w, const float* mean,
                        const float* rstd, const void* dres, void* dx, long ld, vp_stream_t stream);
int vp_layernorm_bwd_wb_partial(int M, int H, const void* dy, const void* x, const float* mean, const float* rstd,
                                float* pw, float* pb, long ld, int rows_per_block, vp_stream_t stream);

/* ---- elementwise.  RoPE rotate-half (HF modeling_llama.py:138-160), SwiGLU (HF LlamaMLP :175-177),
 * GELU / ReLU fwd+bwd for the trainable projector/heads, residual adds. */
int vp_rope(long T, int S, int nheads, int head_dim, void* x, long ld, const float* cos_t, const float* sin_t,
            const int* pos, int inverse, vp_stream_t stream);
/* interleaved = 1: gate / up in 8-column chunks (the frozen-LLM layout of the fused GEMM epilogues); 0: [gate | up] halves
 * (trainable LLM, where gate_proj / up_proj stay contiguous views of the flat parameter buffer) */
int vp_swiglu_fwd(long M, int F, const void* gate_up, long ldg, void* out, long ldo, int interleaved, vp_stream_t stream);
int vp_swiglu_bwd(long M, int F, const void* dact, long ldd, const void* gate_up, void* dgate_up, long ldg, int interleaved,
                  vp_stream_t stream);
/* dst[idx[r], :] += src[r, :] (fp32 atomics, idx < 0 skips): embed_tokens gradient when the LLM is trainable (IFT stage) */
int vp_scatter_add_rows(long n, int H, const void* src, long lds, const int* idx, float* dst, vp_stream_t stream);
int vp_act_fwd(int kind, long n, const void* x, void* y, vp_stream_t stream);
int vp_act_bwd(int kind, long n, const void* dy, const void* x, void* dx, vp_stream_t stream);
int vp_add_bf16(long n, const void* a, const void* b, void* out, vp_stream_t stream);
int vp_add2d_bf16(long R, int C, void* dst, long ldd, const void* src, long lds, vp_stream_t stream);
int vp_copy2d_bf16(long R, int C, void* dst, long ldd, const void* src, long lds, vp_stream_t stream);
/* zero a device range on `stream` (replaces torch's `.zero_()` / `torch.zeros` of gradient buffers and scatter targets) */
int vp_memset_zero(void* ptr, long bytes, vp_stream_t stream);
/* depthwise 7x7 conv, NHWC, zero pad 3 — timm ConvNeXtBlock.conv_dw of the CLIP-ConvNeXt-XXL tower
 * (multimodal_encoder/clip_convnext_encoder.py:161-165).  w is tap-major [49, C]. */
int vp_dwconv7x7_nhwc(int B, int H, int W, int C, const void* x, const void* w, const void* bias, void* y, vp_stream_t stream);
/* bias gradients (column sums), two deterministic stages */
int vp_colsum_partial(long M, int N, const void* x, long ld, float* part, int rows_per_block, vp_stream_t stream);
int vp_colsum_finish(int nslab, int N, const float* part, float* out, float scale, int accumulate, vp_stream_t stream);

/* ---- sequence splice (ola_arch.py:224-254 append_special_tokens, :345-429 embed/concat/pad) as a row
 * gather driven by a host-built index table, and its backward as a gather-sum. */
int vp_gather_rows(long n_out, int H, const void* const* srcs, const long* lds, int nsrc, const int* kind,
                   const int* row, void* out, long ldo, vp_stream_t stream);
int vp_gather_sum_rows(long n_out, int cnt, int H, const void* src, long lds, int src_f32, const int* idx, float scale,
                       void* out, long ldo, int out_f32, int accumulate, vp_stream_t stream);

int vp_cast_f32_to_bf16(long n, const float* x, void* y, vp_stream_t stream);
int vp_cast_bf16_to_f32(long n, const void* x, float* y, int accumulate, vp_stream_t stream);
/* dst[idx[r], :] = (float)src[r, :] for n rows of H bf16 (idx NULL: row r; idx < 0: row skipped): the bf16 lm_head logits of a row chunk widened
 * into their rows of the fp32 [B*S, V] `logits` the reference's forward returns (ola_llama.py:121-122 `logits = self.lm_head(hidden_states);
 * logits = logits.float()`).  H % 8 == 0, lds % 8 == 0, ldd % 4 == 0, 16-byte aligned bases. */
int vp_scatter_rows_bf16_to_f32(long n, int H, const void* src, long lds, const int* idx, float* dst, long ldd, vp_stream_t stream);
int vp_sum_f32(long n, const float* x, float* out, float scale, vp_stream_t stream);
/* out[0] = sum x[i]^2 (global gradient norm for clip_grad_norm_ semantics); part = workspace of vp_sumsq_nblk(n) floats */
int vp_sumsq_nblk(long n);
int vp_sumsq_f32(long n, const float* x, float* part, float* out, vp_stream_t stream);

/* ---- frozen DPT depth decoder (da_v2_head.py:182-321, run under no_grad at base_ola_vlm.py:462-470; output `depth_preds`).
 * NHWC bf16.  3x3 convs = vp_im2col3x3_nhwc (pad 1, stride 1|2, optional input ReLU of ResidualConvUnit; column order
 * (ky, kx, c)) + vp_gemm_bf16; ConvTranspose2d(k = stride) = vp_gemm_bf16 to [pixels, k*k*C] + vp_pixel_shuffle_nhwc;
 * F.interpolate(mode="bilinear", align_corners=True | False) = vp_bilinear_nhwc; (x - min) / (max - min) per image = vp_minmax_norm. */
int vp_im2col3x3_nhwc(int B, int H, int W, int C, int stride, int relu_in, const void* x, void* col, vp_stream_t stream);
int vp_bilinear_nhwc(int B, int H, int W, int C, int Ho, int Wo, int align_corners, const void* x, void* y, vp_stream_t stream);
int vp_pixel_shuffle_nhwc(int B, int H, int W, int k, int C, const void* x, void* y, vp_stream_t stream);
int vp_minmax_norm(int B, long n, const void* x, void* y, vp_stream_t stream);

/* ---- attention.  HF LlamaAttention eager path (modeling_llama.py:191-214: QK^T/sqrt(d) + causal mask,
 * fp32 softmax, PV), HF CLIPAttention (non-causal), PerceiverAttention (resampler.py:46-75; scale d^-1/4
 * on q and k == d^-1/2 on the product).  Tensors are [B,S,H,D] views (strides in elements, multiples of 8; 16-byte
 * aligned bases).  lse: fp32 [B,Hq,Sq] (log2 domain).  vp_attn_bwd's `delta` is a caller-owned fp32 workspace of
 * 3*B*Hq*Sq floats (row dots dO.O, then interleaved (lse, delta) pairs for the DMA-fed dK/dV kernel).
 * Mask: key j is visible to query row i iff j < kv_len[b] (kv_len NULL: Skv), causal: j <= i + Skv - Sq, window > 0: j > i + Skv - Sq - window.
 * A query row with NO visible key (a window together with kv_len: rows past kv_len + window - 1 - (Skv - Sq) of a right-padded sample) is
 * defined: the forward writes o = 0 and lse = -1e30 for it; the backward, given that lse, writes dq = 0 for it and adds nothing of it to
 * dk / dv (keys >= kv_len get exact zeros).  HF's eager softmax yields NaN for such a row; its loss terms are masked out there.
 * Undefined for these entry points: kv_len[b] = 0, and causal with Sq > Skv. */
int vp_attn_fwd(int B, int Hq, int Hkv, int Sq, int Skv, int D, const void* q, long q_bs, long q_ts, const void* k,
                long k_bs, long k_ts, const void* v, long v_bs, long v_ts, void* o, long o_bs, long o_ts, float* lse,
                const int* kv_len, int causal, int window, float scale, vp_stream_t stream);
/* forward with additive fp32 score biases: Swin window attention of the frozen segmentation teacher (HF modeling_swin.py SwinAttention:
 * relative position bias per head [Hq,Sq,Skv] + shifted-window mask [bias_nb,Sq,Skv] indexed by batch % bias_nb); either may be NULL */
int vp_attn_fwd_bias(int B, int Hq, int Hkv, int Sq, int Skv, int D, const void* q, long q_bs, long q_ts, const void* k,
                     long k_bs, long k_ts, const void* v, long v_bs, long v_ts, void* o, long o_bs, long o_ts, float* lse,
                     const int* kv_len, int causal, int window, float scale, const float* bias_h, const float* bias_b, int bias_nb,
                     vp_stream_t stream);
int vp_attn_bwd(int B, int Hq, int Hkv, int Sq, int Skv, int D, const void* q, long q_bs, long q_ts, const void* k,
                long k_bs, long k_ts, const void* v, long v_bs, long v_ts, const void* o, long o_bs, long o_ts,
                const float* lse, const void* dout, long do_bs, long do_ts, void* dq, long dq_bs, long dq_ts, void* dk,
                long dk_bs, long dk_ts, void* dv, long dv_bs, long dv_ts, float* delta, const int* kv_len, int causal,
                int window, float scale, vp_stream_t stream);

/* vp_attn_bwd with the RoPE backward of dq / dk fused into the stores (HF LlamaAttention.forward rotates q, k with
 * apply_rotary_pos_emb before SDPA, modeling_llama.py / modeling_phi3.py; autograd rotates dq / dk back).  D = 128 or 96, causal only.
 * rope_cos / rope_sin: fp32 [positions, D / 2] as for vp_rope; rope_pos: int32 [B, S] position ids or NULL (position = row index).
 * Bit-identical to vp_attn_bwd followed by vp_rope(inverse = 1) on dq and dk. */
int vp_attn_bwd_rope(int B, int Hq, int Hkv, int Sq, int Skv, int D, const void* q, long q_bs, long q_ts, const void* k, long k_bs,
                     long k_ts, const void* v, long v_bs, long v_ts, const void* o, long o_bs, long o_ts, const float* lse,
                     const void* dout, long do_bs, long do_ts, void* dq, long dq_bs, long dq_ts, void* dk, long dk_bs, long dk_ts,
                     void* dv, long dv_bs, long dv_ts, float* delta, const int* kv_len, int causal, int window, float scale,
                     const float* rope_cos, const float* rope_sin, const int* rope_pos, vp_stream_t stream);

/* ---- single-token decode (KV-cached generation).  The reference scores every checkpoint by generating text: HF's generation loop over
 * `inputs_embeds` after the multimodal splice (base_ola_vlm.py:579-616, llava_llama.py:122), called from eval/model_cvbench_loader.py:127,
 * eval/model_mmstar_loader.py:125 and demo.py:328 with use_cache=True.  One token per sequence: every decoder GEMM has M = B <= 16 rows and
 * is bound by its weight's bytes.
 * vp_decode_gemm: C[M,N] = epi(norm(A)[M,K] . W[N,K]^T) for 1 <= M <= 16 (HF LlamaAttention q/k/v/o_proj, LlamaMLP gate/up/down_proj and
 *   lm_head at one position).  W is read once, straight into registers.  norm_w non-NULL: RMSNorm prologue (HF LlamaRMSNorm: every block
 *   computes rstd of the A rows over K itself and applies gamma = norm_w [K] while loading A; vp_rmsnorm_fwd's rounding points).
 *   epilogue VP_EPI_NONE: bf16 out, or fp32 out (out_f32 = 1: the lm_head logits, ola_llama.py:121-122 `.float()`); residual non-NULL:
 *   C = bf16(bf16(acc) + residual) (o_proj / down_proj residual adds); VP_EPI_SWIGLU_IL / VP_EPI_SWIGLU_HALVES: W is the fused gate|up
 *   weight (interleaved 8-row chunks as ops.interleave_gate_up lays it out / [gate | up] halves), C = silu(gate) * up [M, N/2].  Shapes whose
 *   N has too few 16-row tiles to fill the chip also split K over blocks: `workspace` = vp_decode_gemm_workspace_bytes(M, N, K, epilogue)
 *   bytes of caller-owned device memory (0 = none needed; NULL then allowed), summed in a fixed order (bit-identical run to run).
 *   K, lda, ldw multiples of 8, A / W / norm_w 16-byte aligned.  17 <= M <= 64: vp_decode_gemm_wide below. */
#define VP_EPI_SWIGLU_IL 4
#define VP_EPI_SWIGLU_HALVES 5
long vp_decode_gemm_workspace_bytes(int M, int N, int K, int epilogue);
int vp_decode_gemm(int M, int N, int K, const void* A, long lda, const void* W, long ldw, void* C, long ldc, const void* residual, long ldr,
                   const void* norm_w, float eps, int epilogue, int out_f32, float* workspace, vp_stream_t stream);
/* FP8 weight-only decoding.  The reference loads a checkpoint for evaluation in 8 / 4 bits with load_pretrained_model(..., load_8bit, load_4bit)
 * (ola_vlm/model/builder.py:26-34: bitsandbytes); these two entry points stand in for that on gfx950 with OCP e4m3fn weights (not the MI300
 * fnuz encoding) and one power-of-two fp32 scale per weight row.
 * vp_quant_rows_e4m3: W bf16 [N, K] (finite) -> Q uint8 [N, K] e4m3fn bytes + scale fp32 [N].  Per row: s = 2^ceil(log2(absmax / 448)) (rows of
 *   zeros: s = 1), Q = e4m3fn(W / s) rounded to nearest even as torch's .to(torch.float8_e4m3fn) does on the CPU; the row's largest magnitude
 *   lands in (224, 448] before rounding, so nothing saturates and no byte is NaN.  writeback != 0: W is overwritten in place with bf16(Q * s),
 *   which is exact (the bf16 kernels on the written-back weights and vp_decode_gemm_w8 on Q then compute the same model).  Row order only:
 *   weight layouts (interleaved gate|up, halves, folded norms) need no support, the scale travels with the row.  K, ldw, ldq multiples of 8
 *   (ldw in elements, ldq in bytes), W 16-byte and Q 8-byte aligned.
 * vp_decode_gemm_w8: vp_decode_gemm with W = uint8 [N, K] e4m3fn bytes (ldw in bytes) and w_scale fp32 [N]: the bytes are converted exactly to
 *   bf16 in registers and fed to the same MFMA against the bf16 activation (A is not quantised); row n's fp32 sum is multiplied by w_scale[n]
 *   before any rounding point of the epilogue (SwiGLU: the gate and the up sum each by their own row's scale).  Same prologue, epilogues,
 *   split-K contract (its own vp_decode_gemm_w8_workspace_bytes) and error codes as vp_decode_gemm; K and ldw multiples of 16. */
int vp_quant_rows_e4m3(int N, int K, void* W, long ldw, void* Q, long ldq, float* scale, int writeback, vp_stream_t stream);
long vp_decode_gemm_w8_workspace_bytes(int M, int N, int K, int epilogue);
int vp_decode_gemm_w8(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* w_scale, void* C, long ldc,
                      const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace,
                      vp_stream_t stream);
/* MXFP4 weight-only decoding: the 4-bit half of the same loading options (load_4bit), on gfx950 as OCP MXFP4: e2m1 codes (0, 0.5, 1, 1.5, 2, 3, 4,
 * 6; bit 3 = sign), two per byte (element k in byte k / 2, even k in the low nibble), row-major, and one e8m0 scale byte (2^(byte - 127)) per
 * block of 32 consecutive k of a row.  K % 32 == 0.
 * vp_quant_blocks_mxfp4: W bf16 [N, K] (finite) -> Q uint8 [N, K/2] codes + E uint8 [N, K/32] scale bytes.  Per block: the smallest power of two
 *   with absmax / s <= 6 (exponent clamped below at -120, so every nonzero dequantised value is a normal bf16 number; a block of zeros: byte
 *   127), Q = e2m1(W / s) rounded to nearest, ties to the even code, the weight's sign bit kept also on a zero; nothing saturates.
 *   writeback != 0: W is overwritten in place with bf16(Q * s), which is exact (the bf16 kernels on the written-back weights and
 *   vp_decode_gemm_w4 on Q, E then compute the same model).  ldw in elements (a multiple of 8), ldq and lde in bytes (ldq a multiple of 16),
 *   W and Q 16-byte aligned.
 * vp_decode_gemm_w4: vp_decode_gemm with W = uint8 [N, K/2] codes and E = uint8 [N, K/32] scale bytes (ldw and lde in bytes): a 16-byte load
 *   carries one scale block; the codes are converted to bf16 in registers with the block scale applied by the conversion itself (exact) and
 *   fed to the same MFMA against the bf16 activation (A is not quantised), so the epilogue has no scale multiply.  Same prologue, epilogues,
 *   split-K contract (its own vp_decode_gemm_w4_workspace_bytes) and error codes as vp_decode_gemm; K a multiple of 32, ldw of 16. */
int vp_quant_blocks_mxfp4(int N, int K, void* W, long ldw, void* Q, long ldq, void* E, long lde, int writeback, vp_stream_t stream);
long vp_decode_gemm_w4_workspace_bytes(int M, int N, int K, int epilogue);
int vp_decode_gemm_w4(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const void* E, long lde, void* C, long ldc,
                      const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace,
                      vp_stream_t stream);
/* 17 .. 64 sequences per step.  vp_decode_gemm_wide / _w8_wide / _w4_wide: their parents for 1 <= M <= 64, with the parents' argument lists,
 * shape and alignment rules, split-K contract (their own *_wide_workspace_bytes(M, N, K, epilogue): the slabs, nothing else) and error codes.
 * A block still streams one 16-row W tile once and serves up to four 16-row A tiles from each converted W fragment, so the weight bytes of
 * a step do not grow with M.  Output row m is a function of A row m alone: it equals, bit for bit, what the parent returns for that row
 * inside any 16-row slice of A (calling the parent once per slice is the same computation that reads W once per slice).  M <= 16 launches
 * the parent's kernel.  The RMSNorm prologue stays inside the kernel (every block computes the rstd of all M rows). */
long vp_decode_gemm_wide_workspace_bytes(int M, int N, int K, int epilogue);
int vp_decode_gemm_wide(int M, int N, int K, const void* A, long lda, const void* W, long ldw, void* C, long ldc, const void* residual,
                        long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace, vp_stream_t stream);
long vp_decode_gemm_w8_wide_workspace_bytes(int M, int N, int K, int epilogue);
int vp_decode_gemm_w8_wide(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* w_scale, void* C, long ldc,
                           const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32, float* workspace,
                           vp_stream_t stream);
long vp_decode_gemm_w4_wide_workspace_bytes(int M, int N, int K, int epilogue);
int vp_decode_gemm_w4_wide(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const void* E, long lde, void* C,
                           long ldc, const void* residual, long ldr, const void* norm_w, float eps, int epilogue, int out_f32,
                           float* workspace, vp_stream_t stream);
/* RoPE of the new token and the KV append (HF apply_rotary_pos_emb + DynamicCache.update, modeling_llama.py, at position pos[b] of each
 * sequence): qkv [B, ldqkv] rows (Hq q heads | Hkv k heads | Hkv v heads, head_dim D); q rotated into q_out [B, ldq]; k rotated and v copied
 * into row pos[b] of the caches ([B, Smax, Hkv, D] views, strides in elements).  cos_t / sin_t: fp32 [>= Smax, D/2] (ops.rope_tables); pos:
 * int32 [B] on the device (a captured step stays valid from token to token); rows with pos[b] outside [0, Smax) are not written.  Rounding
 * points of vp_rope. */
int vp_decode_rope_append(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_cache, long k_bs,
                          long k_ts, void* v_cache, long v_bs, long v_ts, const float* cos_t, const float* sin_t, const int* pos, int Smax,
                          vp_stream_t stream);
/* Decode attention (HF LlamaAttention / Phi3Attention eager path at one query row: fp32 softmax over the cached keys): q [B, Hq*D] rows
 * (stride q_bs), K / V caches [B, Smax, Hkv, D] (strides in elements), kv_len: int32 [B] on the device (keys 0 .. kv_len-1; with window > 0
 * only keys with kv_len - 1 - key < window, Engine._attn_window's convention), o [B, Hq*D] bf16 (stride o_bs).  The Hq/Hkv query heads of a
 * KV head share every K / V read; the key range is split over `nsplit` blocks (Smax <= 512 * nsplit), combined in a fixed order.  workspace:
 * vp_decode_attn_workspace_bytes(B, Hq, Hkv, D, nsplit) bytes, caller-owned.  D in {32, 64, 96, 128}, Hq/Hkv in {1, 2, 4, 8}. */
long vp_decode_attn_workspace_bytes(int B, int Hq, int Hkv, int D, int nsplit);
int vp_decode_attn(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts, const void* v,
                   long v_bs, long v_ts, void* o, long o_bs, const int* kv_len, int window, float scale, int nsplit, float* workspace,
                   vp_stream_t stream);
/* FP8 KV cache: the cache of generate() in OCP e4m3fn bytes with one power-of-two fp32 scale per (token, KV head) — the row contract of
 * vp_quant_rows_e4m3 with row length D (s = 2^ceil(log2(absmax / 448)), a zero head: s = 1, round to nearest even, nothing saturates, no NaN
 * byte; quant.py: quantize_kv_heads).  K is quantised after RoPE, V as projected.  Every dequantised value is a bf16 number, so each writer
 * can also (or instead) write the dequantised rows into a bf16 cache, which vp_decode_attn then reads: the same model on the bf16 kernel.
 * vp_quant_kv_e4m3 (the prefill's cache writer): src bf16, n token rows of `heads` heads of D elements (2 Hkv for a k|v row), row stride
 *   ld_src elements -> Q uint8 rows (stride ldq bytes) + scale fp32 [n, heads] rows (stride ld_scale elements), and / or deq bf16 rows
 *   (stride ldd elements).  Q and scale go together; Q / scale or deq may be NULL, not both.  src is read only.  D a multiple of 8, at most
 *   128; ld_src, ldq, ldd multiples of 8; src / deq 16-byte, Q 8-byte aligned.
 * vp_decode_rope_append_kv8: vp_decode_rope_append (q_out is bit-identical to it) whose row pos[b] receives the quantised rotated k and the
 *   quantised v: bytes ([B, Smax, Hkv, D] views, strides in bytes) + scales ([B, Smax, Hkv] views, strides in elements), and / or their
 *   dequantised values in bf16 caches (strides in elements).  The four byte / scale pointers go together, the two bf16 pointers go together;
 *   either set may be NULL, not both.  Rows with pos[b] outside [0, Smax) are not written.  D a multiple of 16, at most 128.
 * vp_decode_attn_kv8: vp_decode_attn on the byte cache: k / v uint8 (strides in bytes, multiples of 16, bases 16-byte aligned), k_scale /
 *   v_scale fp32 (strides in elements).  The bytes are converted exactly in registers; the key's scale multiplies its finished dot product,
 *   the value row's scale multiplies its softmax weight (exact power-of-two products in fp32).  Same window / kv_len / nsplit conventions,
 *   same workspace (vp_decode_attn_workspace_bytes), same fixed-order combine (bit-identical run to run), same shapes and error codes. */
int vp_quant_kv_e4m3(long n, int heads, int D, const void* src, long ld_src, void* Q, long ldq, float* scale, long ld_scale, void* deq,
                     long ldd, vp_stream_t stream);
int vp_decode_rope_append_kv8(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_bytes, long k_bs,
                              long k_ts, void* v_bytes, long v_bs, long v_ts, float* k_scale, long ks_bs, long ks_ts, float* v_scale,
                              long vs_bs, long vs_ts, void* k_deq, long kd_bs, long kd_ts, void* v_deq, long vd_bs, long vd_ts,
                              const float* cos_t, const float* sin_t, const int* pos, int Smax, vp_stream_t stream);
int vp_decode_attn_kv8(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts,
                       const float* k_scale, long ks_bs, long ks_ts, const void* v, long v_bs, long v_ts, const float* v_scale, long vs_bs,
                       long vs_ts, void* o, long o_bs, const int* kv_len, int window, float scale, int nsplit, float* workspace,
                       vp_stream_t stream);
/* Row-mapped siblings of the four entry points above, for the verify step of prompt-lookup decoding (HF generate(prompt_lookup_num_tokens=n):
 * transformers/generation/candidate_generator.py PromptLookupCandidateGenerator + utils.py _assisted_decoding): the n + 1 rows of a sequence
 * (its last token and n drafts) are batch rows of their own that share the sequence's cache row.  Each is its sibling plus one argument,
 * cache_row: int32 [B] on the device; batch row r writes to / reads from cache row cache_row[r] (K / V bytes, bf16 rows and scales alike),
 * while pos[r], kv_len[r], q, q_out, o and the workspace stay indexed by r.  NULL = identity: the sibling itself (same kernels, same launch
 * sequence, bit-identical results).  Same argument checks and error codes as the siblings.  The caller's contract, not checked on the
 * device: every cache_row[r] lies in [0, rows of the cache); two rows of one append launch may name the same cache row with different pos,
 * but no two rows may carry the same (cache_row, pos) pair (they would write the same cache row in an unspecified order).  A row's results
 * are a function of its own q, kv_len, window, nsplit and the keys it reads, so row r equals the sibling's row on a cache whose row r is a
 * copy of row cache_row[r], bit for bit. */
int vp_decode_rope_append_rows(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_cache, long k_bs,
                               long k_ts, void* v_cache, long v_bs, long v_ts, const float* cos_t, const float* sin_t, const int* pos,
                               const int* cache_row, int Smax, vp_stream_t stream);
int vp_decode_attn_rows(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts,
                        const void* v, long v_bs, long v_ts, void* o, long o_bs, const int* kv_len, const int* cache_row, int window,
                        float scale, int nsplit, float* workspace, vp_stream_t stream);
int vp_decode_rope_append_kv8_rows(int B, int Hq, int Hkv, int D, const void* qkv, long ldqkv, void* q_out, long ldq, void* k_bytes,
                                   long k_bs, long k_ts, void* v_bytes, long v_bs, long v_ts, float* k_scale, long ks_bs, long ks_ts,
                                   float* v_scale, long vs_bs, long vs_ts, void* k_deq, long kd_bs, long kd_ts, void* v_deq, long vd_bs,
                                   long vd_ts, const float* cos_t, const float* sin_t, const int* pos, const int* cache_row, int Smax,
                                   vp_stream_t stream);
int vp_decode_attn_kv8_rows(int B, int Hq, int Hkv, int D, int Smax, const void* q, long q_bs, const void* k, long k_bs, long k_ts,
                            const float* k_scale, long ks_bs, long ks_ts, const void* v, long v_bs, long v_ts, const float* v_scale,
                            long vs_bs, long vs_ts, void* o, long o_bs, const int* kv_len, const int* cache_row, int window, float scale,
                            int nsplit, float* workspace, vp_stream_t stream);
/* The device half of the acceptance rule of that verify step, and the next step's counters.  B sequences of n + 1 rows; all arrays int32
 * on the device.  next [B (n + 1)]: the argmax of every row's logits (read only).  tok [B (n + 1)]: what the rows were fed (row (b, 0) the
 * last emitted token, rows (b, 1 .. n) the drafts).  Per sequence: n_acc[b] = the largest j <= n with tok[b, i] == next[b, i - 1] for all
 * 1 <= i <= j; base_pos[b] += n_acc[b] + 1; pos[b, i] = base_pos[b] + i and kv_len[b, i] = pos[b, i] + 1 for the next step's rows;
 * tok[b, 0] = next[b, n_acc[b]].  n = 0 is the one-token step's + 1.  No workspace.  Null pointers, B <= 0 or n < 0: VP_ERR_BAD_ARG. */
int vp_decode_accept(int B, int n, const int* next, int* tok, int* base_pos, int* pos, int* kv_len, int* n_acc, vp_stream_t stream);
/* Token selection on the device: HF's RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, then
 * greedy or sampling, for R rows of RAW fp32 logits [R, V] (row stride ld_logits >= V; never modified), 1 <= V <= 2^20.  Per row, in fp32 IEEE
 * arithmetic (correctly rounded divisions: the scores are reproducible bit for bit on a CPU):
 *   1. penalty      x = seen[v] ? (l < 0 ? l * repetition_penalty : l / repetition_penalty) : l          (repetition_penalty 1 = off)
 *   2. temperature  s = x / temperature
 *   3. top-k        k = min(max(top_k, 1), V): every s >= the k-th largest value is kept, ties included      (top_k 0 = off)
 *   4. top-p        over the survivors, p ~ exp(s - max): v is kept iff the mass of the survivors u with s_u <= s_v exceeds 1 - top_p; the
 *                   largest is always kept                                                                 (top_p 1 = off)
 *   5. scores_out   (fp32 [R, V], stride ld_scores >= V, NULL = off) = s where kept, -inf where removed: what HF's chain returns
 *   6. greedy       (do_sample 0) the smallest index of the largest s
 *   7. sampling     the kept tokens in ascending index order; the token whose interval of the cumulative distribution of p contains u
 *                   (fp32 in [0, 1)): torch.multinomial's distribution on a different random stream.  Masses are exp(s - max) * 2^40 as
 *                   integers, so sums are exact in any order: tokens and scores_out are the same from run to run.
 * seen: uint32 [R, ceil(V / 32)], caller-owned, zeroed once by the caller: bit v of row r = the row was given token v before; the bit of the
 *   selected token is set (NULL allowed when repetition_penalty is 1).  u: fp32 [u_steps, R], row min(*col, u_steps - 1) is read (u_steps 1:
 *   a plain [R]); NULL allowed when do_sample is 0.  eos: int32 [n_eos] on the device, 0 <= n_eos <= 64.  col: ONE int32 on the device, the
 *   output column (read on the device so that a captured step replays; the caller advances it, vp_add_i32).
 * Writes tok[r] = the selected token (always the raw choice: the next step's input); out[r, *col] (int32 [R, n_out], stride ld_out; nothing
 *   when *col is outside [0, n_out)) = pad if finished[r] was set, else the token; finished[r] |= (that output is in eos).
 * For any input bits (NaN rows included) the kernel ends and tok[r] lies in [0, V).  No workspace.  Null required pointers and scalars
 * outside their ranges: VP_ERR_BAD_ARG before any launch. */
int vp_decode_select(int R, int V, const float* logits, long ld_logits, int do_sample, float temperature, int top_k, float top_p,
                     float repetition_penalty, unsigned int* seen, const float* u, int u_steps, const int* eos, int n_eos, int pad,
                     int* finished, const int* col, int* tok, int* out, long ld_out, int n_out, float* scores_out, long ld_scores,
                     vp_stream_t stream);
/* x[i] += delta for n int32 on the device (the per-sequence position / length counters of a decode step, advanced without a host round trip) */
int vp_add_i32(long n, int* x, int delta, vp_stream_t stream);

/* ---- losses.  NTP CE (ola_llama.py:121-136: logits.float(), shifted CrossEntropyLoss, ignore -100);
 * embedding distillation (base_ola_vlm.py:289-320 _emb_loss; ola_utils.py:108-125
 * calculate_contrastive_loss; :96-106 dist_collect -> tgt_all is the rank-ordered all-gather).
 * vp_ce_fwd_bwd: logits [rows, V] bf16 with row stride ld (ld % 8 == 0, ld >= V; columns V .. ld-1 are neither read nor written), overwritten
 *   in place with (softmax - onehot) * grad_scale when write_grad != 0 (left untouched when 0); row_loss[r] = logsumexp - logit[label], 0 for an
 *   ignored row (its gradient row is zeroed).  PRECONDITION: every label is negative (ignored; the reference uses -100) or in [0, V): the kernel
 *   reads logits[r, label] unchecked, so a label >= V is an out-of-bounds read. */
int vp_ce_fwd_bwd(long rows, int V, void* logits, long ld, const long* labels, float* row_loss, float grad_scale,
                  int write_grad, vp_stream_t stream);
/* vp_emb_loss_fwd: ONE launch (streaming MFMA/dot2 pass + deterministic last-block tree + the B x Bw softmax); out3 = {emb_loss, sl1,
 * contrastive} exactly as _emb_loss returns them (not yet multiplied by the task weight); coef (2B + B*Bw + 1 floats) carries the
 * backward coefficients and d loss / d logit_scale in its last slot.  workspace: vp_emb_loss_workspace(B, Bw, D) floats, uninitialised.
 * counters: vp_emb_loss_counter_bytes() bytes of CALLER-OWNED device memory holding the tree's ticket counters, zeroed once by the caller;
 * every launch leaves the block zeroed, so one block serves all launches of one stream; launches that may overlap (different streams) need
 * different blocks.  The library owns no device memory and keeps no pointer after the call returns.
 * 0 < B <= 64 local predictions, B <= Bw <= 1024 gathered targets (rank-ordered, rank r's rows at r*B), D % 8 == 0; pred [B,D] and
 * tgt_all [Bw,D] bf16 row-major, 16-byte aligned.  logit_scale NULL = no contrastive term. */
long vp_emb_loss_counter_bytes(void);
long vp_emb_loss_workspace(int B, int Bw, long D);
int vp_emb_loss_fwd(int B, int Bw, long D, int rank, const void* pred, const void* tgt_all, const float* mask,
                    const float* logit_scale, float w_contrastive, float* out3, float* coef, float* workspace, unsigned* counters,
                    vp_stream_t stream);
/* The same for `ntask` (<= 8) distillation heads in ONE launch each way (blockIdx.z = head): the heads of a step share B, Bw and rank and
 * differ in D, pointers, workspace and contrastive weight (host arrays of length ntask).  The reference calls _emb_loss once per head and
 * layer (base_ola_vlm.py:445-534). */
int vp_emb_loss_fwd_multi(int ntask, int B, int Bw, const long* D, int rank, const void* const* pred, const void* const* tgt_all,
                          const float* const* mask, const float* const* logit_scale, const float* w_contrastive, float* const* out3,
                          float* const* coef, float* const* workspace, unsigned* counters, vp_stream_t stream);
int vp_emb_loss_bwd_multi(int ntask, int B, int Bw, const long* D, int rank, const void* const* pred, const void* const* tgt_all,
                          const float* const* coef, const float* grad_out, void* const* dpred, vp_stream_t stream);
int vp_emb_loss_bwd(int B, int Bw, long D, int rank, const void* pred, const void* tgt_all, const float* coef,
                    float grad_out, void* dpred, vp_stream_t stream);

/* ---- optimizer.  HF Trainer `adamw_torch` (ola_vlm_train.py:124; torch.optim.AdamW semantics) fused over
 * the flat fp32 master buffer, bf16 shadow refreshed in the same pass. */
int vp_adamw(long n, float* p, const float* g, float* m, float* v, void* bf16_shadow, float lr, float beta1, float beta2,
             float eps, float weight_decay, int step, float grad_scale, vp_stream_t stream);

/* ---- data-parallel exchange points, RCCL over xGMI with the library's own side stream + hipEvent fences.  Replaces
 * DeepSpeed ZeRO-2's gradient reduction (scripts/zero2.json:16-22, launched by scripts/train/pretrain.sh:15) and diffdist's
 * all_gather of the contrastive targets (ola_utils.py:96-106).  One process per GPU; rank 0 creates the unique id
 * (vp_comm_unique_id_bytes() bytes) and distributes it out of band; vp_comm_init is collective.  RCCL is resolved at run time
 * (the librccl already loaded in the process, e.g. PyTorch's, else librccl.so[.1]).
 *   vp_comm_allreduce_async: in-place SUM of `count` elements (dtype 0 = fp32, 1 = bf16, 2 = int32) on the communicator's side
 *     stream, ordered after the work already queued on `compute_stream`; returns at once (overlaps the rest of the backward pass).
 *   vp_comm_wait: `compute_stream` waits on the device for every all-reduce issued since the last wait; the host never blocks.
 *   vp_comm_allgather: recv[world*count] = rank-ordered concatenation of send[count], on `stream`. */
int vp_comm_unique_id_bytes(void);
int vp_comm_unique_id(void* id_out);
int vp_comm_init(int rank, int world, const void* id, void** comm_out);
int vp_comm_allreduce_async(void* comm, void* buf, long count, int dtype, vp_stream_t compute_stream);
int vp_comm_wait(void* comm, vp_stream_t compute_stream);
int vp_comm_allgather(void* comm, const void* send, void* recv, long count, int dtype, vp_stream_t stream);
int vp_comm_info(void* comm, int* rank, int* world);
int vp_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif
