"""KV-cached generation on the engine (the reference's `generate`: base_ola_vlm.py:579-616 for the PT classes, llava_llama.py:122 for the
IFT classes — the multimodal splice, then HF's generation loop over `inputs_embeds`).

  prefill   the label-less training forward (build_plan(labels=None) -> _embed -> _decoder_fwd(compute_grads=False)) with every layer's
            post-RoPE k / v rows copied (or, for an FP8 cache, quantised: vp_quant_kv_e4m3) into the cache; lm_head on each sequence's
            last valid row only
  step      per layer: QKV (RMSNorm prologue) -> RoPE + KV append at pos[b] -> decode attention -> wo + residual -> gate_up (RMSNorm
            prologue, SwiGLU epilogue) -> down + residual; final norm folded into the fp32 lm_head launch; pos / kv_len += 1 on the device

A step takes up to 64 sequences: up to 16 its GEMMs are the skinny entry points, above that the wide ones (vp_decode_gemm*_wide: one streamed
weight for up to four 16-row tiles of rows, the same bits row for row; DecodeSession.wide_gemm = False runs the skinny ones per 16-row slice).

Every per-token scalar (token ids, positions, cache lengths) lives on the device, so one step can be captured once into a CUDA graph
(single stream, no fork) and replayed for every token (VP_DECODE_GRAPH=1; the default is eager launches: capture did not pay, see below).  Decode reads the same kernel-ready weights
_decoder_fwd reads (fused qkv, gate|up in the engine's layout, folded gamma when fold_norm is on), so IFT-trained weights are current.
After Engine.quantize_decoder() the step streams those matrices as e4m3fn bytes (vp_decode_gemm_w8) or as MXFP4 blocks (vp_decode_gemm_w4)
instead (quant.py: the contracts); the prefill stays on the bf16 weights, which by then hold exactly the dequantised values.
Independently of the weights, the cache itself can be kept as e4m3fn bytes with one scale per (token, KV head) (kv_cache_dtype="fp8_e4m3":
vp_decode_rope_append_kv8 / vp_decode_attn_kv8), or, for verification, as a bf16 cache of the dequantised values read by the bf16 kernels.

Prompt-lookup decoding (HF generate(prompt_lookup_num_tokens=n, max_matching_ngram_size=g): candidate_generator.py
PromptLookupCandidateGenerator, greedy only) raises the tokens per step without a second model:

  draft     lookup_draft: the last n-gram of a sequence's tokens is searched earlier in the sequence and what followed it there is proposed
  verify    one step on B (n + 1) rows: row (b, i) is a batch row of its own at position pos_b + i that appends to and reads sequence b's
            cache row (the *_rows entry points), so it runs exactly the computation the one-token step would have run for that token:
            the same GEMM column, the same attention splits (nsplit of B sequences, not of the rows), the same argmax
  accept    vp_decode_accept keeps the leading drafts that equal the model's own choices and sets the next step's counters; the rows of
            rejected drafts are overwritten by the next step before anything reads them
Tokens and logits are those of plain greedy decoding, bit for bit; only the number of steps changes.

Token selection.  Without top_k / repetition_penalty / device_sampling a token is chosen by plain torch between two steps (warp_logits /
next_tokens: temperature, top-p, torch.multinomial) and the loop reads the host every token.  With one of them the step itself ends in
vp_decode_select (ops.decode_select: HF's repetition penalty -> temperature -> top-k -> top-p on the raw logits, greedy or inverse-CDF
sampling from uniforms drawn once per call, EOS / pad bookkeeping) and a counter increment, so the whole token is device work that a captured
step replays; the host reads the finished flags every `sync_every` steps.  The penalised set is what THIS call emitted for the row: the
reference reaches HF through `inputs_embeds`, so HF's processor sees the new tokens only."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops

BF16 = torch.bfloat16
I32 = torch.int32


KV_CACHE_DTYPES = ("bf16", "fp8_e4m3", "fp8_e4m3_emulated")


def resolve_kv_cache_dtype(name):
    """None / "bf16" | "fp8_e4m3" | "fp8_e4m3_emulated" -> the canonical name (host-only; anything else is a ValueError)."""
    if name is None:
        return "bf16"
    if isinstance(name, str) and name in KV_CACHE_DTYPES:
        return name
    raise ValueError(f"kv_cache_dtype {name!r}: choose one of {', '.join(KV_CACHE_DTYPES)} (None = bf16)")


class KVCache:
    """Per layer one [B, Smax, 2 * Hkv * D] buffer: each token row is k (Hkv * D) | v (Hkv * D), the layout of the k|v columns of the fused
    qkv rows (the prefill writes a sequence's rows in one strided launch).  `lens`: int32 [2B] on the device = (pos [B] = tokens cached,
    kv_len [B] = pos + 1: the keys the next step attends to, its own included); `lens_host` mirrors pos.
    dtype "bf16": bf16 rows.  "fp8_e4m3": uint8 rows of e4m3fn bytes plus `scales`, per layer fp32 [B, Smax, 2 * Hkv] (k scales | v scales),
    one power-of-two scale per (token, KV head) (quant.py: quantize_kv_heads): (D + 4) / 2D of the bf16 cache's bytes.
    "fp8_e4m3_emulated": bf16 rows that hold the dequantised quantised values (the same model on the bf16 attention kernel)."""

    def __init__(self, cfg, B, Smax, device, dtype="bf16"):
        nkv, hd = cfg.num_key_value_heads, cfg.head_dim
        self.B, self.Smax, self._hd = B, Smax, hd
        self.dtype = resolve_kv_cache_dtype(dtype)
        L = cfg.num_hidden_layers
        fp8 = self.dtype == "fp8_e4m3"
        self.kv = [torch.empty(B, Smax, 2 * nkv * hd, device=device, dtype=torch.uint8 if fp8 else BF16) for _ in range(L)]
        self.scales = [torch.empty(B, Smax, 2 * nkv, device=device, dtype=torch.float32) for _ in range(L)] if fp8 else None
        self.lens = torch.zeros(2 * B, device=device, dtype=I32)
        self.lens_host = np.zeros(B, np.int64)

    @property
    def nbytes(self):
        """bytes of the k / v storage (scales included)"""
        return sum(t.numel() * t.element_size() for t in self.kv + (self.scales or []))

    def k(self, l):
        B, Smax, C = self.kv[l].shape
        return self.kv[l].view(B, Smax, 2, -1)[:, :, 0].unflatten(-1, (-1, self._hd))

    def v(self, l):
        B, Smax, C = self.kv[l].shape
        return self.kv[l].view(B, Smax, 2, -1)[:, :, 1].unflatten(-1, (-1, self._hd))

    def k_scale(self, l):
        """fp32 [B, Smax, Hkv] view ("fp8_e4m3" only)"""
        return self.scales[l][:, :, :self.scales[l].shape[2] // 2]

    def v_scale(self, l):
        return self.scales[l][:, :, self.scales[l].shape[2] // 2:]

    @property
    def pos(self):
        return self.lens[:self.B]

    @property
    def kv_len(self):
        return self.lens[self.B:]


MAX_VERIFY_ROWS = 16                                             # the skinny GEMMs' M
MAX_BATCH = ops.DECODE_GEMM_WIDE_ROWS                            # the wide GEMMs' M: sequences of one decode step


def check_batch(B):
    """Host-only, before any GPU work: a step's GEMMs have one row per sequence and take at most MAX_BATCH."""
    if int(B) > MAX_BATCH:
        raise ValueError(f"generate: batch of {int(B)} sequences, a decode step takes at most {MAX_BATCH} (its GEMMs, vp_decode_gemm*_wide, "
                         f"have 1 <= M <= {MAX_BATCH} rows); generate in groups of at most {MAX_BATCH} prompts")


def check_lookup(B, n, do_sample=False, max_ngram=2):
    """prompt_lookup_num_tokens for B sequences -> n (None / 0: 0 = the plain path).  Host-only, before any GPU work: lookup is greedy
    (speculative sampling is not built) and a verify step has B (n + 1) <= 16 rows."""
    n = 0 if n is None else int(n)
    if n < 0:
        raise ValueError(f"prompt_lookup_num_tokens = {n}: must be >= 0")
    if n == 0:
        return 0
    if do_sample:
        raise ValueError("prompt_lookup_num_tokens with do_sample=True: speculative sampling is not built; lookup decoding is greedy "
                         "(do_sample=False)")
    if int(max_ngram) < 1:
        raise ValueError(f"max_matching_ngram_size = {max_ngram}: must be >= 1")
    if B * (n + 1) > MAX_VERIFY_ROWS:
        most = MAX_VERIFY_ROWS // B - 1
        raise ValueError(f"prompt_lookup_num_tokens = {n} at batch {B}: a verify step has B (n + 1) = {B * (n + 1)} rows, the decode GEMMs "
                         f"take {MAX_VERIFY_ROWS}; the largest prompt_lookup_num_tokens for B = {B} is {max(most, 0)}"
                         + ("" if most > 0 else " (no lookup at this batch size)"))
    return n


def lookup_draft(history, n, max_ngram=2):
    """The drafter (HF PromptLookupCandidateGenerator's rule): for g = min(max_ngram, len - 1) down to 1, among the earlier windows equal to
    the last g tokens of `history` take the EARLIEST one that has a continuation, and return up to n tokens of it; the continuation stops
    before the first negative id (the <image> placeholder is no embedding row).  No match: [].  history: the sequence's valid prompt ids
    (attention mask applied) followed by the emitted tokens; plain numpy on the host."""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    L = h.size
    if int(n) <= 0:
        return []
    for g in range(min(int(max_ngram), L - 1), 0, -1):
        hit = np.flatnonzero((np.lib.stride_tricks.sliding_window_view(h, g) == h[L - g:]).all(1))
        hit = hit[hit < L - g]                                   # the suffix itself has nothing after it
        if hit.size:
            start = int(hit[0]) + g
            cont = h[start:min(start + int(n), L)]
            neg = np.flatnonzero(cont < 0)
            return cont[:int(neg[0])].tolist() if neg.size else cont.tolist()
    return []


def check_select(top_k=None, repetition_penalty=None, device_sampling=None, sync_every=1, lookup=0):
    """The token-selection arguments of generate() -> (top_k, repetition_penalty, sync_every, device): top_k 0 / repetition_penalty 1.0 =
    off; device = the selector runs on the device (vp_decode_select) — iff top_k > 0, repetition_penalty != 1 or device_sampling is true.
    Host-only, before any GPU work, after check_lookup / check_batch."""
    top_k = 0 if top_k is None else int(top_k)
    if top_k < 0:
        raise ValueError(f"top_k = {top_k}: must be >= 0 (0 / None = off)")
    theta = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if not theta > 0 or theta == float("inf"):
        raise ValueError(f"repetition_penalty = {repetition_penalty}: must be > 0 and finite (1.0 / None = off)")
    if int(sync_every) < 1:
        raise ValueError(f"sync_every = {sync_every}: must be >= 1 (the host reads the finished flags every sync_every steps)")
    if lookup and (theta != 1.0 or device_sampling):
        raise ValueError("prompt_lookup_num_tokens with repetition_penalty / device_sampling: the verify step accepts a draft iff it is the "
                         "plain argmax of its row; a penalised or device-selected verify step is not built")
    return top_k, theta, int(sync_every), bool(top_k > 0 or theta != 1.0 or device_sampling)


def text_plan(eng, input_ids, attention_mask):
    """No-splice prefill input (text-only generate of the PT classes: base_ola_vlm.py:606-607 embeds the tokens as they are): each
    sequence's valid tokens left-aligned in [B*S, H] rows gathered from the embedding table.  Returns (x, plan) with the plan fields
    _decoder_fwd reads."""
    ids = input_ids.detach().cpu().numpy().astype(np.int64)
    am = np.ones_like(ids, dtype=bool) if attention_mask is None else attention_mask.detach().cpu().numpy().astype(bool)
    B = ids.shape[0]
    toks = [ids[b][am[b]] for b in range(B)]
    V = eng.fz["embed"].shape[0]
    bad = [int(t) for tk in toks for t in tk if not 0 <= t < V]
    if bad:                                                      # (an <image> token without `images`, or an id outside the vocabulary)
        raise ValueError(f"generate without images: prompt token ids must lie in [0, {V}), got {sorted(set(bad))[:4]}")
    lens = np.array([len(t) for t in toks], np.int32)
    if (lens == 0).any():
        raise ValueError("generate: every sequence needs at least one prompt token")
    S = int(lens.max())
    kind = np.full((B, S), -1, np.int32)
    row = np.zeros((B, S), np.int32)
    for b, t in enumerate(toks):
        kind[b, :len(t)] = 0
        row[b, :len(t)] = t
    dev = eng.dev
    H = eng.cfg.hidden_size
    x = torch.empty(B * S, H, device=dev, dtype=BF16)
    ops.gather_rows([eng.fz["embed"]], torch.from_numpy(kind.reshape(-1)).to(dev), torch.from_numpy(row.reshape(-1)).to(dev), H, x)
    plan = dict(B=B, S=S, lens_host=lens, full=bool((lens == S).all()), lens=torch.from_numpy(lens).to(dev), present=None)
    return x, plan


class DecodeSession:
    """One generate() call: the cache, the preallocated step buffers and (optionally) the captured step.
    lookup = n > 0: verify mode (prompt-lookup decoding).  A step then runs R = B (n + 1) rows, row b (n + 1) + i at position pos_b + i on
    cache row b, through verify() instead of step(); `steps` and `accepted` count the verify steps and the drafts they accepted.
    wide_gemm: how the GEMMs of a step with 17 .. 64 rows run (ops.decode_gemm's `wide`): None = the wide entry points, one call each;
    False = the skinny entry points once per 16-row slice (the same tokens and logits: the verification and benchmark leg).  Set it before
    prefill(); sessions of at most 16 rows do not read it."""

    wide_gemm = None
    sel = None                                                   # device-side token selection (alloc_select): the step then ends in it

    def __init__(self, eng, kv_cache_dtype=None, lookup=None):
        self.eng = eng
        self.cfg = eng.cfg
        self.lookup = int(lookup or 0)
        self.steps = self.accepted = 0
        # the cache format (KVCache): the argument, else the engine's default (model.quantize_kv_cache_for_generation); independent of
        # the weight format below.  Resolved here, on the host, before any GPU work
        self.kv_cache_dtype = resolve_kv_cache_dtype(kv_cache_dtype if kv_cache_dtype is not None else getattr(eng, "kv_cache_dtype", None))
        self.graph = None
        # capture measured on MI355X (profiles/decode_bench_*.json): no gain — the step is GPU-bound (Llama-3-8B B = 1: 9.01 ms/token
        # replayed vs 9.06 eager, 3.3 ms of host enqueue under it), so eager launches are the default; VP_DECODE_GRAPH=1 captures
        self.use_graph = os.environ.get("VP_DECODE_GRAPH", "0") == "1"
        self.replays = 0
        # weight-only quantised decoding (Engine.quantize_decoder): {fz key: (e4m3fn bytes, per-row scales) | (e2m1 codes, block scale bytes)}
        # of the matrices the step streams in fq_format, or None (bf16).  Read once per session: a session never mixes formats, and stale
        # copies were already dropped by quantized_weights().
        self.fq = eng.quantized_weights()
        self.fq_format = eng.fq_format if self.fq is not None else None

    # ---------------------------------------------------------------------------------------------- prefill
    def prefill(self, input_ids, attention_mask=None, images=None, group_sizes=None, max_new_tokens=16):
        """-> fp32 logits [B, V] of every sequence's last prompt position; the cache holds the prompt's k / v."""
        eng, cfg = self.eng, self.cfg
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        if images is not None:
            plan = eng.build_plan(input_ids, attention_mask, None, group_sizes)
            x, *_ = eng._embed(images, plan)
        else:
            x, plan = text_plan(eng, input_ids, attention_mask)
        B, S = plan["B"], plan["S"]
        lens = np.asarray(plan["lens_host"]).astype(np.int64)
        Smax = int(lens.max()) + int(max_new_tokens) + self.lookup     # verify mode: + n rows of slack for rejected drafts
        c = self.cache = KVCache(cfg, B, Smax, eng.dev, self.kv_cache_dtype)
        cw = 2 * nkv * hd
        kvd = self.kv_cache_dtype

        def sink(l, qkv):
            src = qkv.view(B, S, -1)
            for b in range(B):                                  # rows 0 .. len_b - 1 (the kernels' layout is left-aligned for either padding side)
                n = int(lens[b])
                rows = src[b, :n, nh * hd:nh * hd + cw]
                if kvd == "bf16":
                    ops.copy2d_(c.kv[l][b, :n], rows)
                elif kvd == "fp8_e4m3":                          # bytes + one scale per (token, head)
                    ops.quant_kv_e4m3(rows, hd, q_out=c.kv[l][b, :n], scale_out=c.scales[l][b, :n])
                else:                                           # emulated: the dequantised values into the bf16 cache
                    ops.quant_kv_e4m3(rows, hd, deq_out=c.kv[l][b, :n])

        dec = eng._decoder_fwd(x, plan, compute_grads=False, kv_sink=sink)
        H = cfg.hidden_size
        last = torch.from_numpy((np.arange(B) * S + lens - 1).astype(np.int32)).to(eng.dev)
        h_last = torch.empty(B, H, device=eng.dev, dtype=BF16)
        ops.gather_rows([dec["hidden"]], torch.zeros(B, device=eng.dev, dtype=I32), last, H, h_last)
        logits = ops.decode_gemm(h_last, eng.fz["lm_head"], out_f32=True, wide=self.wide_gemm)
        c.lens.copy_(torch.from_numpy(np.concatenate([lens, lens + 1]).astype(np.int32)))
        c.lens_host[:] = lens
        self._alloc(B)
        return logits

    # ---------------------------------------------------------------------------------------------- step
    def _alloc(self, B):
        eng, cfg, dev = self.eng, self.cfg, self.eng.dev
        H, I = cfg.hidden_size, cfg.intermediate_size
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        nqkv = (nh + 2 * nkv) * hd
        V = eng.fz["lm_head"].shape[0]
        e = lambda *shape, dt=BF16: torch.empty(*shape, device=dev, dtype=dt)
        nseq, B = B, B * (self.lookup + 1)                       # verify mode: every buffer below has one row per verify row
        self.tok = torch.zeros(B, device=dev, dtype=I32)
        self.zeros_b = torch.zeros(B, device=dev, dtype=I32)
        self.x = [e(B, H), e(B, H)]
        self.qkv, self.q, self.att, self.h1, self.act = e(B, nqkv), e(B, nh * hd), e(B, nh * hd), e(B, H), e(B, I)
        self.logits = e(B, V, dt=torch.float32)
        self.epi = ops.EPI_SWIGLU_IL if eng.gu_interleaved else ops.EPI_SWIGLU_HALVES
        shapes = [(nqkv, H, 0), (H, nh * hd, 0), (2 * I, H, self.epi), (H, I, 0), (V, H, 0)]
        w4 = self.fq_format == "mxfp4"                           # the kernels the step can call: bf16 (lm_head may stay bf16) and the format's own
        nb = max(ops.decode_gemm_ws_bytes(B, N, K, ep, w8=q and not w4, w4=q and w4, wide=self.wide_gemm) for N, K, ep in shapes
                 for q in ((False, True) if self.fq else (False,)))
        self.gws = e(max(1, nb // 4), dt=torch.float32) if nb > 0 else None
        Smax = self.cache.Smax
        self.nsplit = ops.decode_attn_splits(nseq, nkv, Smax)    # of the SEQUENCES: a verify row's splits are the one-token step's
        self.aws = e(ops._lib.raw("vp_decode_attn_workspace_bytes", B, nh, nkv, hd, self.nsplit) // 4, dt=torch.float32)
        self.cos, self.sin = eng.rope(max(Smax, 1))
        if self.lookup:
            n1 = self.lookup + 1
            self.cache_row = torch.arange(nseq, device=dev, dtype=I32).repeat_interleave(n1).contiguous()
            # row (b, i): pos = pos_b + i, kv_len = pos + 1 (the row's own key included, as on the one-token step); base_pos = the cache's
            # pos (its kv_len half is not advanced in this mode)
            lens = torch.from_numpy(self.cache.lens_host.astype(np.int32))
            rp = (lens[:, None] + torch.arange(n1, dtype=I32)[None]).reshape(-1)
            self.vlens = torch.cat([rp, rp + 1]).to(dev)
            self.vpos, self.vkv = self.vlens[:B], self.vlens[B:]
            self.base_pos = self.cache.pos
            self.res = torch.zeros(B + nseq, device=dev, dtype=I32)          # next [R] | n_acc [B]: one host read per step
            self.next32, self.n_acc = self.res[:B], self.res[B:]
            self.next64 = torch.zeros(B, device=dev, dtype=torch.long)

    def _gemm(self, a, key, **kw):
        """One skinny GEMM of the step on weight `key`: its quantised copy when the session decodes from one, else the bf16 weight."""
        q = self.fq.get(key) if self.fq else None
        kw["wide"] = self.wide_gemm
        if q is None:
            return ops.decode_gemm(a, self.eng.fz[key], **kw)
        if self.fq_format == "mxfp4":
            return ops.decode_gemm(a, q[0], w_block_scale=q[1], **kw)
        return ops.decode_gemm(a, q[0], w_scale=q[1], **kw)

    def _step_launches(self):
        """The per-token launches (everything they read or write is preallocated: graph-capturable)."""
        eng, cfg, fz, c = self.eng, self.cfg, self.eng.fz, self.cache
        H, eps = cfg.hidden_size, cfg.rms_norm_eps
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        window = eng._attn_window()
        x = self.x[0]
        ops.gather_rows([fz["embed"]], self.zeros_b, self.tok, H, x)
        for l in range(cfg.num_hidden_layers):
            o = f"dec.{l}."
            self._gemm(x, o + "wqkv", norm_w=fz[o + "ln1"], eps=eps, out=self.qkv, ws=self.gws)
            if self.lookup:
                self._attend_rows(l, window)
            elif self.kv_cache_dtype == "fp8_e4m3":
                ops.decode_rope_append_kv8(self.qkv, self.q, self.cos, self.sin, c.pos, nh, nkv, hd, k_bytes=c.k(l), v_bytes=c.v(l),
                                           k_scale=c.k_scale(l), v_scale=c.v_scale(l))
                ops.decode_attn_kv8(self.q, c.k(l), c.v(l), c.k_scale(l), c.v_scale(l), c.kv_len, nh, window=window, nsplit=self.nsplit,
                                    out=self.att, ws=self.aws)
            else:
                if self.kv_cache_dtype == "bf16":
                    ops.decode_rope_append(self.qkv, self.q, c.k(l), c.v(l), self.cos, self.sin, c.pos, nh, nkv, hd)
                else:                                           # emulated: the new row's dequantised values, read by the bf16 kernel
                    ops.decode_rope_append_kv8(self.qkv, self.q, self.cos, self.sin, c.pos, nh, nkv, hd, k_deq=c.k(l), v_deq=c.v(l))
                ops.decode_attn(self.q, c.k(l), c.v(l), c.kv_len, nh, window=window, nsplit=self.nsplit, out=self.att, ws=self.aws)
            self._gemm(self.att, o + "wo", residual=x, out=self.h1, ws=self.gws)
            self._gemm(self.h1, o + "wgu", norm_w=fz[o + "ln2"], eps=eps, epi=self.epi, out=self.act, ws=self.gws)
            xn = self.x[(l + 1) % 2]
            self._gemm(self.act, o + "wd", residual=self.h1, out=xn, ws=self.gws)
            x = xn
        self._gemm(x, "lm_head", norm_w=fz["norm"], eps=eps, out_f32=True, out=self.logits, ws=self.gws)
        if self.lookup:                                          # the plain path's argmax (ties break the same way), then the acceptance rule
            torch.argmax(self.logits, dim=-1, out=self.next64)
            self.next32.copy_(self.next64)
            ops.decode_accept(self.next32, self.tok, self.base_pos, self.vpos, self.vkv, self.n_acc, self.lookup)
        else:
            ops.add_i32_(c.lens, 1)
        if self.sel is not None:                                 # the whole token is device work: the choice lands in `tok`, where the next
            self._select(self.logits)                            # step's gather reads it

    # ---------------------------------------------------------------------------------------------- device-side selection
    def alloc_select(self, B, N, eos, pad, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, generator=None):
        """Turn the session's step into step + vp_decode_select: the buffers one call owns.  finished / col / out [B, N] int32, the `seen`
        bitmap (penalty only) and, for sampling, `uniforms` [N, B]: drawn once, on the generator's device, so a seeded call reproduces."""
        assert not self.lookup and self.graph is None
        dev = self.eng.dev
        V = self.eng.fz["lm_head"].shape[0]
        self.finished = torch.zeros(B, device=dev, dtype=I32)
        self.col = torch.zeros(1, device=dev, dtype=I32)
        self.out = torch.zeros(B, max(int(N), 1), device=dev, dtype=I32)
        self.seen = torch.zeros(B, (V + 31) // 32, device=dev, dtype=I32) if repetition_penalty != 1.0 else None
        self.eos_t = torch.tensor(eos, device=dev, dtype=I32) if eos else None
        self.uniforms = None
        if do_sample:
            gdev = generator.device if generator is not None else dev
            self.uniforms = torch.rand(max(int(N), 1), B, generator=generator, device=gdev, dtype=torch.float32).to(dev)
        self.sel = dict(do_sample=bool(do_sample), temperature=float(temperature) if do_sample else 1.0, top_k=int(top_k) if do_sample else 0,
                        top_p=float(top_p) if do_sample else 1.0, repetition_penalty=float(repetition_penalty), pad=int(pad))

    def _select(self, logits):
        """Select column `col` from `logits` [B, V] into tok / out / finished, then col += 1 (two launches; inside the step they are
        captured with it)."""
        ops.decode_select(logits, self.tok, self.out, self.col, self.finished, seen=self.seen, u=self.uniforms, eos=self.eos_t, **self.sel)
        ops.add_i32_(self.col, 1)

    def select_first(self, logits):
        """The first token, from the prefill's logits: the same entry point, outside the captured step."""
        self._select(logits)

    def step_select(self):
        """One step on the token the selector left in `tok`, ending in the next selection -> the step's RAW logits (a view)."""
        self._launch()
        self.cache.lens_host += 1
        return self.logits

    def _attend_rows(self, l, window):
        """RoPE + append + attention of layer l in verify mode: the plain step's three cache formats through the *_rows entry points."""
        c, cfg, cr = self.cache, self.cfg, self.cache_row
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        if self.kv_cache_dtype == "fp8_e4m3":
            ops.decode_rope_append_kv8_rows(self.qkv, self.q, self.cos, self.sin, self.vpos, cr, nh, nkv, hd, k_bytes=c.k(l), v_bytes=c.v(l),
                                            k_scale=c.k_scale(l), v_scale=c.v_scale(l))
            ops.decode_attn_kv8_rows(self.q, c.k(l), c.v(l), c.k_scale(l), c.v_scale(l), self.vkv, cr, nh, window=window, nsplit=self.nsplit,
                                     out=self.att, ws=self.aws)
            return
        if self.kv_cache_dtype == "bf16":
            ops.decode_rope_append_rows(self.qkv, self.q, c.k(l), c.v(l), self.cos, self.sin, self.vpos, cr, nh, nkv, hd)
        else:                                                   # emulated: the new rows' dequantised values, read by the bf16 kernel
            ops.decode_rope_append_kv8_rows(self.qkv, self.q, self.cos, self.sin, self.vpos, cr, nh, nkv, hd, k_deq=c.k(l), v_deq=c.v(l))
        ops.decode_attn_rows(self.q, c.k(l), c.v(l), self.vkv, cr, nh, window=window, nsplit=self.nsplit, out=self.att, ws=self.aws)

    def step(self, tokens):
        """Feed one token per sequence (int tensor [B] on the device) -> fp32 logits [B, V] of the next position (a view of a buffer the next
        step overwrites)."""
        assert not self.lookup, "verify mode steps through verify()"
        self.tok.copy_(tokens.to(I32))
        self._launch()
        self.cache.lens_host += 1
        return self.logits

    def _launch(self):
        if self.use_graph:
            if self.graph is None:
                self._capture()
            self.graph.replay()
            self.replays += 1
        else:
            self._step_launches()

    def feed(self, tokens):
        """Verify mode: the token of row 0 of every sequence before the FIRST verify step (int [B]); later steps' are set on the device."""
        self.tok.view(-1, self.lookup + 1)[:, 0].copy_(tokens.to(I32))

    def verify(self, drafts):
        """One verify step.  drafts: int32 [B, n] on the host, the tokens of rows 1 .. n of every sequence (any valid embedding row: a draft
        counts only if it equals the model's own token).  -> (next [B, n + 1], n_acc [B]) on the host: the model's choice at every row and
        the number of drafts accepted; sequence b emitted next[b, 0 .. n_acc[b]].  `logits` [B (n + 1), V] holds the rows they were chosen
        from until the next step."""
        n1 = self.lookup + 1
        self.tok.view(-1, n1)[:, 1:].copy_(drafts.to(I32))
        self._launch()
        res = self.res.cpu()                                     # the step's one host read
        nxt, n_acc = res[:self.tok.numel()].view(-1, n1), res[self.tok.numel():]
        self.steps += 1
        self.accepted += int(n_acc.sum())
        self.cache.lens_host += n_acc.numpy().astype(np.int64) + 1
        return nxt, n_acc

    def _capture(self):
        """Capture _step_launches once (single stream, no fork).  Capture records without executing; `lens` moves only on replay."""
        g = torch.cuda.CUDAGraph()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g):
            self._step_launches()
        self.graph = g


# -------------------------------------------------------------------------------------------------- sampling (HF semantics, plain torch)
def warp_logits(scores, temperature=1.0, top_p=1.0, min_tokens_to_keep=1):
    """HF TemperatureLogitsWarper then TopPLogitsWarper (transformers/generation/logits_process.py) on fp32 [B, V] scores."""
    if temperature is not None and temperature != 1.0:
        scores = scores / temperature
    if top_p is not None and top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        sorted_indices_to_remove = cumulative_probs <= (1 - top_p)
        sorted_indices_to_remove[..., -min_tokens_to_keep:] = 0
        indices_to_remove = sorted_indices_to_remove.scatter(1, sorted_indices, sorted_indices_to_remove)
        scores = scores.masked_fill(indices_to_remove, -float("inf"))
    return scores


def next_tokens(logits, do_sample=False, temperature=1.0, top_p=1.0, generator=None):
    if not do_sample:
        return torch.argmax(logits, dim=-1)
    probs = warp_logits(logits.float(), temperature, top_p).softmax(dim=-1)
    return torch.multinomial(probs, num_samples=1, generator=generator).squeeze(1)


def generate(eng, input_ids, attention_mask=None, images=None, group_sizes=None, max_new_tokens=20, do_sample=False, temperature=1.0,
             top_p=1.0, eos_token_id=None, pad_token_id=None, streamer=None, generator=None, use_graph=None, return_logits=False,
             kv_cache_dtype=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=2, drafter=None, top_k=None,
             repetition_penalty=None, device_sampling=None, sync_every=1):
    """Greedy / sampled decoding of B prompts, each continuing at its own length -> LongTensor [B, n_new] of the new tokens only (rows that
    finished are padded with pad_token_id after their EOS); B <= 64 (check_batch).  return_logits: also the fp32 logits [B, V] each token was chosen from.
    kv_cache_dtype: None (the engine's default, initially bf16) | "bf16" | "fp8_e4m3" | "fp8_e4m3_emulated" (KVCache).
    prompt_lookup_num_tokens = n > 0 (HF's argument; greedy only, B (n + 1) <= 16): prompt-lookup decoding with n drafts per step from
    lookup_draft(history, n, max_matching_ngram_size), or from drafter(b, history) -> list of ids (no HF argument: the test and benchmark
    hook).  The result, the streamer calls and the logits are those of the plain path.
    top_k (HF; sampling only, like HF's warper) / repetition_penalty (HF; over the tokens this call emitted) / device_sampling=True: tokens
    are selected on the device (vp_decode_select; module docstring).  Greedy tokens are those of the torch path; sampled tokens follow the
    same distribution from their own random stream (`sess.uniforms`, torch.rand(max_new_tokens, B, generator=generator)), not
    torch.multinomial's.  sync_every: the host reads the finished flags every that many steps (a streamer forces 1); the result does not
    depend on it, only the number of steps run past the last EOS.  Without these arguments every launch and every token is the torch path's."""
    B = input_ids.shape[0]
    lookup = check_lookup(B, prompt_lookup_num_tokens, do_sample, max_matching_ngram_size)
    check_batch(B)
    top_k, repetition_penalty, sync_every, device = check_select(top_k, repetition_penalty, device_sampling, sync_every, lookup)
    if device and not lookup:
        return _generate_device(eng, input_ids, attention_mask, images, group_sizes, int(max_new_tokens), do_sample, temperature, top_p,
                                top_k, repetition_penalty, eos_token_id, pad_token_id, streamer, generator, use_graph, return_logits,
                                kv_cache_dtype, sync_every)
    if lookup:
        return _generate_lookup(eng, input_ids, attention_mask, images, group_sizes, int(max_new_tokens), eos_token_id, pad_token_id, streamer,
                                use_graph, return_logits, kv_cache_dtype, lookup, int(max_matching_ngram_size), drafter)
    eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(t) for t in eos_token_id])
    if pad_token_id is None:
        pad_token_id = eos[0] if eos else 0
    sess = DecodeSession(eng, kv_cache_dtype)
    if use_graph is not None:
        sess.use_graph = bool(use_graph)
    if streamer is not None:
        streamer.put(input_ids.cpu())
    with torch.no_grad():
        logits = sess.prefill(input_ids, attention_mask, images, group_sizes, max_new_tokens)
        dev = eng.dev
        eos_t = torch.tensor(eos, device=dev, dtype=torch.long) if eos else None
        finished = torch.zeros(B, device=dev, dtype=torch.bool)
        out, kept = [], []
        for i in range(int(max_new_tokens)):
            if i > 0:
                logits = sess.step(tok)
            if return_logits:
                kept.append(logits.clone())
            raw = next_tokens(logits, do_sample, temperature, top_p, generator).to(torch.long)
            nxt = torch.where(finished, torch.full_like(raw, pad_token_id), raw)
            out.append(nxt)
            if streamer is not None:
                streamer.put(nxt.cpu())
            if eos_t is not None:
                finished = finished | torch.isin(nxt, eos_t)
                if bool(finished.all()):
                    break
            tok = raw                                            # finished rows keep decoding their own (discarded) predictions: pad_token_id
                                                                 # need not be a valid embedding row
    if streamer is not None:
        streamer.end()
    res = torch.stack(out, 1) if out else torch.empty(B, 0, dtype=torch.long, device=eng.dev)
    sess.graph = None
    if return_logits:
        return res, kept, sess
    return res


def _generate_device(eng, input_ids, attention_mask, images, group_sizes, N, do_sample, temperature, top_p, top_k, repetition_penalty,
                     eos_token_id, pad_token_id, streamer, generator, use_graph, return_logits, kv_cache_dtype, sync_every):
    """generate() with the selector on the device.  Column i of `sess.out` is written by the step that computed its logits; the host only
    reads `finished` (and, for a streamer, the new column) every sync_every steps.  Rows that finished emit pad, so whatever ran past the
    column at which the plain loop would have stopped is cut off at the end: the result is the plain loop's for every sync_every."""
    B = input_ids.shape[0]
    eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(t) for t in eos_token_id])
    if pad_token_id is None:
        pad_token_id = eos[0] if eos else 0
    temperature = 1.0 if temperature is None else float(temperature)
    top_p = 1.0 if top_p is None else float(top_p)
    if do_sample and not (temperature > 0 and 0 < top_p <= 1):
        raise ValueError(f"temperature = {temperature} must be > 0 and top_p = {top_p} in (0, 1]")
    sess = DecodeSession(eng, kv_cache_dtype)
    if use_graph is not None:
        sess.use_graph = bool(use_graph)
    if streamer is not None:
        streamer.put(input_ids.cpu())
        sync_every = 1
    kept, n = [], 0
    with torch.no_grad():
        if N > 0:
            logits = sess.prefill(input_ids, attention_mask, images, group_sizes, N)
            sess.alloc_select(B, N, eos, pad_token_id, do_sample, temperature, top_k, top_p, repetition_penalty, generator)
        for i in range(N):
            if i == 0:
                sess.select_first(logits)
            else:
                logits = sess.step_select()
            if return_logits:
                kept.append(logits.clone())
            n = i + 1
            if streamer is not None:
                streamer.put(sess.out[:, i].to(torch.long).cpu())
            if eos and (n % sync_every == 0 or n == N) and bool((sess.finished != 0).all()):
                break
        res = sess.out[:, :n].to(torch.long) if n else torch.empty(B, 0, dtype=torch.long, device=eng.dev)
        if eos and n:                                            # the column after which the plain loop stops: the first at which every row is finished
            done = (torch.isin(res, torch.tensor(eos, device=res.device)).cumsum(1) > 0).all(0)
            if bool(done.any()):
                n = int(torch.nonzero(done)[0]) + 1
                res, kept = res[:, :n].contiguous(), kept[:n]
    if streamer is not None:
        streamer.end()
    sess.graph = None
    if return_logits:
        return res, kept, sess
    return res


def _generate_lookup(eng, input_ids, attention_mask, images, group_sizes, N, eos_token_id, pad_token_id, streamer, use_graph, return_logits,
                     kv_cache_dtype, n, max_ngram, drafter):
    """generate() with prompt-lookup decoding.  Every sequence keeps its own list of raw (greedy) tokens, which a verify step extends by
    1 + accepted drafts; output column i (EOS / pad handling, streamer.put, the kept logits) is produced as soon as every sequence has its
    token i, by the plain loop's rules, so the result is the plain path's whatever the drafts were."""
    B = input_ids.shape[0]
    eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(t) for t in eos_token_id])
    if pad_token_id is None:
        pad_token_id = eos[0] if eos else 0
    sess = DecodeSession(eng, kv_cache_dtype, lookup=n)
    if use_graph is not None:
        sess.use_graph = bool(use_graph)
    if streamer is not None:
        streamer.put(input_ids.cpu())
    ids = input_ids.detach().cpu().numpy().astype(np.int64)
    am = np.ones_like(ids, dtype=bool) if attention_mask is None else attention_mask.detach().cpu().numpy().astype(bool)
    prompt = [ids[b][am[b]] for b in range(B)]
    V = eng.fz["embed"].shape[0]
    if drafter is None:
        drafter = lambda b, history: lookup_draft(history, n, max_ngram)
    dev = eng.dev
    out, kept = [], []
    raw = [[] for _ in range(B)]                                 # the greedy tokens of every sequence, pad-free
    rows = [[] for _ in range(B)]                                # return_logits: the logits row each of them was chosen from
    finished = [False] * B
    done = N <= 0

    def flush():
        nonlocal done
        while not done and len(out) < min(len(r) for r in raw):
            i = len(out)
            col = [pad_token_id if finished[b] else raw[b][i] for b in range(B)]
            nxt = torch.tensor(col, dtype=torch.long, device=dev)
            out.append(nxt)
            if return_logits:
                kept.append(torch.stack([rows[b][i] for b in range(B)]))
            if streamer is not None:
                streamer.put(nxt.cpu())
            if eos:
                for b in range(B):
                    finished[b] = finished[b] or col[b] in eos
            done = len(out) >= N or (bool(eos) and all(finished))

    with torch.no_grad():
        if not done:
            logits = sess.prefill(input_ids, attention_mask, images, group_sizes, N)
            first = torch.argmax(logits, dim=-1)
            sess.feed(first)
            for b, t in enumerate(first.tolist()):
                raw[b].append(t)
                if return_logits:
                    rows[b].append(logits[b].clone())
            flush()
        drafts = torch.empty(B, n, dtype=I32)
        while not done:
            for b in range(B):
                d = [int(t) for t in drafter(b, np.concatenate([prompt[b], np.asarray(raw[b], np.int64)]))][:n]
                bad = [j for j, t in enumerate(d) if not 0 <= t < V]
                d = d[:bad[0]] if bad else d                     # a draft is an embedding row; what follows an invalid one is dropped with it
                drafts[b] = torch.tensor(d + [raw[b][-1]] * (n - len(d)), dtype=I32)     # unused slots: the row-0 token (harmless)
            nxt, n_acc = sess.verify(drafts)
            for b in range(B):
                k = int(n_acc[b]) + 1
                raw[b].extend(nxt[b, :k].tolist())
                if return_logits:
                    rows[b].extend(sess.logits[b * (n + 1):b * (n + 1) + k].clone().unbind(0))
            flush()
    if streamer is not None:
        streamer.end()
    res = torch.stack(out, 1) if out else torch.empty(B, 0, dtype=torch.long, device=dev)
    sess.graph = None
    if return_logits:
        return res, kept, sess
    return res
