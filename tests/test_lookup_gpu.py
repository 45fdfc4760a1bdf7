"""Prompt-lookup decoding on the GPU.  The design is that every row of a verify step runs exactly the computation the one-token step would
have run for it, so every comparison here is torch.equal on the raw bits: the row-mapped append / attention kernels against their
siblings on an expanded cache, vp_decode_accept against its restatement, the skinny GEMMs' rows against the one-row call (the premise), and
generate() with lookup against a plain session at the same Smax, for drafters that are right, wrong and in between.  tests/LOOKUP_PATHS.md
maps the cases."""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
I32 = torch.int32
U8 = torch.uint8


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops
    return ops


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _eq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ------------------------------------------------------------------------------------------------ 1. row-mapped kernels
CONFIGS = [(128, 8, 2), (96, 4, 4), (32, 4, 2)]
SMAX, NSPLIT = 1040, 3
CACHE_ROW = [0, 0, 0, 1, 1, 1]
KV_LEN = [511, 512, 513, 1, 2, 3]


def _i32(v):
    return torch.tensor(v, device="cuda", dtype=I32)


@pytest.mark.parametrize("D,Hq,Hkv", CONFIGS)
def test_attn_rows_equal_sibling_on_expanded_cache(D, Hq, Hkv):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(D + Hq)
    k = torch.randn(2, SMAX, Hkv, D, device="cuda", generator=g).to(BF16)
    v = torch.randn(2, SMAX, Hkv, D, device="cuda", generator=g).to(BF16)
    q = torch.randn(6, Hq * D, device="cuda", generator=g).to(BF16)
    cr, kl = _i32(CACHE_ROW), _i32(KV_LEN)
    idx = cr.long()
    k6, v6 = k[idx].contiguous(), v[idx].contiguous()                     # row r = a copy of row cache_row[r]
    # the byte cache of the same rows: bytes + one scale per (token, head)
    kb, vb = torch.empty(2, SMAX, Hkv, D, device="cuda", dtype=U8), torch.empty(2, SMAX, Hkv, D, device="cuda", dtype=U8)
    ks, vs = torch.empty(2, SMAX, Hkv, device="cuda"), torch.empty(2, SMAX, Hkv, device="cuda")
    ops.quant_kv_e4m3(k.view(2 * SMAX, Hkv * D), D, q_out=kb.view(2 * SMAX, Hkv * D), scale_out=ks.view(2 * SMAX, Hkv))
    ops.quant_kv_e4m3(v.view(2 * SMAX, Hkv * D), D, q_out=vb.view(2 * SMAX, Hkv * D), scale_out=vs.view(2 * SMAX, Hkv))
    kb6, vb6, ks6, vs6 = (t[idx].contiguous() for t in (kb, vb, ks, vs))
    for window in (0, 512):
        want = ops.decode_attn(q, k6, v6, kl, Hq, window=window, nsplit=NSPLIT)
        got = ops.decode_attn_rows(q, k, v, kl, cr, Hq, window=window, nsplit=NSPLIT)
        assert _eq(got, want), (window, "bf16")
        assert _eq(ops.decode_attn_rows(q, k6, v6, kl, None, Hq, window=window, nsplit=NSPLIT), want), (window, "bf16, no row map")
        want8 = ops.decode_attn_kv8(q, kb6, vb6, ks6, vs6, kl, Hq, window=window, nsplit=NSPLIT)
        got8 = ops.decode_attn_kv8_rows(q, kb, vb, ks, vs, kl, cr, Hq, window=window, nsplit=NSPLIT)
        assert _eq(got8, want8), (window, "e4m3")
        assert _eq(ops.decode_attn_kv8_rows(q, kb6, vb6, ks6, vs6, kl, None, Hq, window=window, nsplit=NSPLIT), want8), (window, "e4m3, no row map")


@pytest.mark.parametrize("D,Hq,Hkv", CONFIGS)
def test_append_rows_land_in_one_cache_row(D, Hq, Hkv):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(3 * D + Hq)
    qkv = torch.randn(6, (Hq + 2 * Hkv) * D, device="cuda", generator=g).to(BF16)
    cos, sin = ops.rope_tables(SMAX, D, 10000.0, "cuda")
    cr = _i32(CACHE_ROW)
    for pos_l in ([510, 511, 512, 0, 1, 2], [510, 511, SMAX, 0, 1, 2]):   # second: row 2 lies outside the cache and writes nothing
        pos = _i32(pos_l)
        written = [(c, p) for c, p in zip(CACHE_ROW, pos_l) if p < SMAX]
        mask = torch.zeros(2, SMAX, dtype=torch.bool, device="cuda")
        for c, p in written:
            mask[c, p] = True

        def bf16_caches(B):
            return [torch.full((B, SMAX, Hkv, D), 7.0, device="cuda", dtype=BF16) for _ in range(2)]

        # bf16 cache
        k6, v6 = bf16_caches(6)
        q6 = torch.empty(6, Hq * D, device="cuda", dtype=BF16)
        ops.decode_rope_append(qkv, q6, k6, v6, cos, sin, pos, Hq, Hkv, D)
        k2, v2 = bf16_caches(2)
        q2 = torch.empty_like(q6)
        ops.decode_rope_append_rows(qkv, q2, k2, v2, cos, sin, pos, cr, Hq, Hkv, D)
        assert _eq(q2, q6)
        for r, (c, p) in enumerate(zip(CACHE_ROW, pos_l)):
            if p < SMAX:
                assert _eq(k2[c, p], k6[r, p]) and _eq(v2[c, p], v6[r, p]), (r, c, p)
        assert (k2[~mask] == 7.0).all() and (v2[~mask] == 7.0).all()      # every other row untouched
        assert int(mask.sum()) == len(written) and not (k2[mask] == 7.0).all()
        kn, vn = bf16_caches(6)                                           # no row map: the sibling itself
        qn = torch.empty_like(q6)
        ops.decode_rope_append_rows(qkv, qn, kn, vn, cos, sin, pos, None, Hq, Hkv, D)
        assert _eq(qn, q6) and _eq(kn, k6) and _eq(vn, v6)

        # byte cache + scales, and the dequantised rows (the emulated cache), in one launch
        def byte_caches(B):
            return dict(k_bytes=torch.full((B, SMAX, Hkv, D), 0x55, device="cuda", dtype=U8),
                        v_bytes=torch.full((B, SMAX, Hkv, D), 0x55, device="cuda", dtype=U8),
                        k_scale=torch.full((B, SMAX, Hkv), 7.0, device="cuda"), v_scale=torch.full((B, SMAX, Hkv), 7.0, device="cuda"),
                        k_deq=torch.full((B, SMAX, Hkv, D), 7.0, device="cuda", dtype=BF16),
                        v_deq=torch.full((B, SMAX, Hkv, D), 7.0, device="cuda", dtype=BF16))

        c6, c2, cn = byte_caches(6), byte_caches(2), byte_caches(6)
        q6b, q2b, qnb = torch.empty_like(q6), torch.empty_like(q6), torch.empty_like(q6)
        ops.decode_rope_append_kv8(qkv, q6b, cos, sin, pos, Hq, Hkv, D, **c6)
        ops.decode_rope_append_kv8_rows(qkv, q2b, cos, sin, pos, cr, Hq, Hkv, D, **c2)
        ops.decode_rope_append_kv8_rows(qkv, qnb, cos, sin, pos, None, Hq, Hkv, D, **cn)
        assert _eq(q6b, q6) and _eq(q2b, q6) and _eq(qnb, q6)
        for name, t2 in c2.items():
            sentinel = 0x55 if t2.dtype == U8 else 7.0
            for r, (c, p) in enumerate(zip(CACHE_ROW, pos_l)):
                if p < SMAX:
                    assert _eq(t2[c, p], c6[name][r, p]), (name, r, c, p)
            assert (t2[~mask] == sentinel).all(), name
            assert _eq(cn[name], c6[name]), name


# ------------------------------------------------------------------------------------------------ 2. the acceptance rule
def _accept_ref(n, nxt, tok, base_pos):
    """vp_decode_accept restated: lists in, (n_acc, base_pos, pos, kv_len, tok) out"""
    B = len(base_pos)
    n_acc, bp, pos, kvl, tok = [], list(base_pos), [], [], [list(t) for t in tok]
    for b in range(B):
        j = 0
        while j < n and tok[b][j + 1] == nxt[b][j]:
            j += 1
        n_acc.append(j)
        bp[b] += j + 1
        pos.append([bp[b] + i for i in range(n + 1)])
        kvl.append([bp[b] + i + 1 for i in range(n + 1)])
        tok[b][0] = nxt[b][j]
    return n_acc, bp, pos, kvl, tok


def _accept_gpu(ops, n, nxt, tok, base_pos):
    B = len(base_pos)
    t_next, t_tok, t_bp = _i32(nxt).reshape(-1), _i32(tok).reshape(-1), _i32(base_pos)
    t_pos, t_kvl = (torch.full((B * (n + 1),), -9, device="cuda", dtype=I32) for _ in range(2))
    t_acc = torch.full((B,), -9, device="cuda", dtype=I32)
    keep = t_next.clone()
    ops.decode_accept(t_next, t_tok, t_bp, t_pos, t_kvl, t_acc, n)
    assert torch.equal(t_next, keep)                                      # read only
    return t_acc.tolist(), t_bp.tolist(), t_pos.view(B, n + 1).tolist(), t_kvl.view(B, n + 1).tolist(), t_tok.view(B, n + 1).tolist()


def test_decode_accept_every_pattern():
    ops = _ops()
    n, B = 3, 3
    patterns = list(itertools.product([True, False], repeat=n))           # draft i right / wrong
    assert (False, True, True) in patterns
    want_acc = {p: next((i for i, ok in enumerate(p) if not ok), n) for p in patterns}
    assert want_acc[(False, True, False)] == 0 and want_acc[(True, True, True)] == 3        # "draft 2 right, draft 1 wrong -> 0"
    patterns += patterns[:1]                                              # 9 = 3 launches of B = 3
    for launch in range(3):
        ps = patterns[3 * launch:3 * launch + 3]
        nxt = [[100 * (b + 1) + 10 * launch + i for i in range(n + 1)] for b in range(B)]
        tok = [[5 + b] + [nxt[b][i] if ps[b][i] else nxt[b][i] + 1 for i in range(n)] for b in range(B)]
        base_pos = [17 + 100 * b + launch for b in range(B)]
        got, want = _accept_gpu(ops, n, nxt, tok, base_pos), _accept_ref(n, nxt, tok, base_pos)
        assert got == want, (ps, got, want)
        assert got[0] == [want_acc[p] for p in ps]
        assert [t[1:] for t in got[4]] == [t[1:] for t in tok]            # the drafts are left as they were
    # n = 0: the one-token step's + 1
    got = _accept_gpu(ops, 0, [[41], [42], [43]], [[1], [2], [3]], [5, 0, 99])
    assert got == ([0, 0, 0], [6, 1, 100], [[6], [1], [100]], [[7], [2], [101]], [[41], [42], [43]])


# ------------------------------------------------------------------------------------------------ 3. the premise: GEMM rows do not depend on M
@pytest.mark.parametrize("fmt", ["bf16", "w8", "w4"])
def test_skinny_gemm_rows_are_independent_of_m(fmt):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(11)
    for N, K, split in ((256, 2048, True), (8208, 512, False)):
        assert (ops.decode_gemm_ws_bytes(6, N, K, 0, w8=fmt == "w8", w4=fmt == "w4") > 0) == split
        a = torch.randn(6, K, device="cuda", generator=g).to(BF16)
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(BF16)
        gamma = (1 + 0.1 * torch.randn(K, device="cuda", generator=g)).to(BF16)
        res = torch.randn(6, N, device="cuda", generator=g).to(BF16)
        kw = {}
        if fmt == "w8":
            w, sc = ops.quant_rows_e4m3(w)
            kw = dict(w_scale=sc)
        elif fmt == "w4":
            w, e = ops.quant_blocks_mxfp4(w)
            kw = dict(w_block_scale=e)
        for extra in (dict(norm_w=gamma, eps=1e-5, residual=res), dict(norm_w=gamma, eps=1e-5, out_f32=True), dict()):
            full = ops.decode_gemm(a, w, **{**extra, **kw})
            for m in range(6):
                ex = dict(extra)
                if "residual" in ex:
                    ex["residual"] = res[m:m + 1]
                one = ops.decode_gemm(a[m:m + 1], w, **{**ex, **kw})
                assert _eq(full[m:m + 1], one), (fmt, N, K, m, sorted(extra))


# ------------------------------------------------------------------------------------------------ 4. the engine
def _tiny_engine(arch, quantize=None):
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.engine import Engine
    ocfg, W, batch, g = cases.tiny_llama_case(arch)
    eng = Engine(VisperConfig(**vars(ocfg)))
    eng.load_weights(W)
    if quantize:
        eng.quantize_decoder(fmt=quantize)
    return eng, batch


def _ragged():
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, 1000, (n,), generator=g) for n in (7, 19, 12)]
    T = max(len(p) for p in prompts)
    ids = torch.zeros(3, T, dtype=torch.long)
    am = torch.zeros(3, T, dtype=torch.long)
    for b, p in enumerate(prompts):                                        # left padding, as the eval scripts' tokenizers pad
        ids[b, T - len(p):] = p
        am[b, T - len(p):] = 1
    return ids, am


def _plain(eng, ids, am, images, N, n, kv=None):
    """A plain DecodeSession at the lookup run's Smax (its prefill given N + n): N + n greedy tokens [B, N + n] on the host, the logits
    [B, V] each was chosen from, and the session."""
    from visper_lm_amd import decode
    sess = decode.DecodeSession(eng, kv)
    sess.use_graph = False
    toks, kept = [], []
    with torch.no_grad():
        logits = sess.prefill(ids, am, images, None, N + n)
        for i in range(N + n):
            if i:
                logits = sess.step(tok)
            kept.append(logits.clone())
            tok = torch.argmax(logits, -1)
            toks.append(tok)
    return torch.stack(toks, 1).cpu(), kept, sess


def _drafters(ref, plens, n, V):
    """b, history -> drafts, from the plain run's tokens ref [B, >= N + n]: the true continuation | always wrong | first right, rest wrong"""
    def true(b, h):
        c = len(h) - plens[b]
        return ref[b, c:c + n].tolist()

    def wrong(b, h):
        return [(t + 1) % V for t in true(b, h)]

    def first(b, h):
        t = true(b, h)
        return t[:1] + [(x + 1) % V for x in t[1:]]

    return dict(true=true, wrong=wrong, first=first)


def _lookup_equals_plain(eng, ids, am, images, N, n, kv=None, which=("real", "true", "wrong", "first"), graph=("first",)):
    from visper_lm_amd import decode
    B = ids.shape[0]
    ref, ref_kept, ps = _plain(eng, ids, am, images, N, n, kv)
    plens = [int(am[b].sum()) if am is not None else ids.shape[1] for b in range(B)]      # prompt ids (an <image> id is one of them)
    V = eng.fz["embed"].shape[0]
    dr = dict(_drafters(ref, plens, n, V), real=None)
    stats = {}
    for name in which:
        for use_graph in ((False, True) if name in graph else (False,)):
            toks, kept, s = decode.generate(eng, ids, am, images, None, max_new_tokens=N, return_logits=True, kv_cache_dtype=kv,
                                            prompt_lookup_num_tokens=n, drafter=dr[name], use_graph=use_graph)
            assert s.lookup == n and s.cache.Smax == ps.cache.Smax and s.nsplit == ps.nsplit and s.kv_cache_dtype == ps.kv_cache_dtype
            assert toks.shape == (B, N) and torch.equal(toks.cpu(), ref[:, :N]), (name, use_graph)
            assert len(kept) == N and all(_eq(kept[i], ref_kept[i]) for i in range(N)), (name, use_graph)
            assert s.use_graph == use_graph and (s.replays == s.steps if use_graph else s.replays == 0)
            stats[name] = (s.steps, s.accepted)
    if "true" in stats:                                                   # every step accepts n drafts of every sequence
        assert stats["true"] == (math.ceil((N - 1) / (n + 1)), B * n * math.ceil((N - 1) / (n + 1))), stats
    if "wrong" in stats:
        assert stats["wrong"] == (N - 1, 0), stats
    if "first" in stats:
        assert stats["first"] == (math.ceil((N - 1) / 2), B * math.ceil((N - 1) / 2)), stats
    return ref, stats


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_lookup_equals_plain_tiny_with_image(arch):
    _ops()
    eng, batch = _tiny_engine(arch)
    _lookup_equals_plain(eng, batch["input_ids"][:1], None, batch["images"][:1].cuda(), 11, 3)


def test_lookup_equals_plain_ragged_batch_eos_and_streamer():
    _ops()
    from visper_lm_amd import decode
    eng, _ = _tiny_engine("llama")
    ids, am = _ragged()
    N, n = 11, 3
    ref, _ = _lookup_equals_plain(eng, ids, am, None, N, n)
    plens = [int(x) for x in am.sum(1)]
    dr = _drafters(ref, plens, n, eng.fz["embed"].shape[0])
    # an EOS chosen inside an accepted run (token 2 of sequence 0: the first verify step accepts tokens 1 .. 3): plain generate's output
    eos = int(ref[0, 2])
    kw = dict(max_new_tokens=N, eos_token_id=[eos], pad_token_id=-7)
    want = decode.generate(eng, ids, am, None, None, **kw)
    assert (want[0, 3:] == -7).all()
    for name in ("true", "first", "wrong"):
        assert torch.equal(decode.generate(eng, ids, am, None, None, prompt_lookup_num_tokens=n, drafter=dr[name], **kw), want), name
    # every row finished at once -> the loop stops where the plain loop does
    firsts = [int(ref[b, 0]) for b in range(3)]
    assert decode.generate(eng, ids, am, None, None, max_new_tokens=N, eos_token_id=firsts, prompt_lookup_num_tokens=n).shape == (3, 1)
    # the streamer: the prompt, then one token per put, in order

    class S:
        def __init__(self):
            self.calls = []

        def put(self, v):
            self.calls.append(v.clone())

        def end(self):
            self.calls.append("end")

    s = S()
    toks = decode.generate(eng, ids, am, None, None, max_new_tokens=N, streamer=s, prompt_lookup_num_tokens=n, drafter=dr["true"])
    assert torch.equal(s.calls[0], ids) and s.calls[-1] == "end" and len(s.calls) == N + 2
    assert all(c.shape == (3,) for c in s.calls[1:-1])
    assert torch.equal(torch.stack([c.cpu() for c in s.calls[1:-1]], 1), toks.cpu()) and torch.equal(toks.cpu(), ref[:, :N])


def test_lookup_equals_plain_mxfp4_weights_fp8_cache():
    _ops()
    eng, batch = _tiny_engine("llama", quantize="mxfp4")
    assert eng.fq_format == "mxfp4"
    ids, img = batch["input_ids"][:1], batch["images"][:1].cuda()
    _lookup_equals_plain(eng, ids, None, img, 11, 3, kv="fp8_e4m3", which=("true", "wrong"), graph=())
    _lookup_equals_plain(eng, ids, None, img, 11, 3, kv="fp8_e4m3_emulated", which=("first",), graph=())


# ------------------------------------------------------------------------------------------------ 5. full width
def test_lookup_equals_plain_full_width_llama():
    _ops()
    from visper_lm_amd.config import llama3_8b
    from visper_lm_amd.engine import Engine
    eng = Engine(llama3_8b(num_hidden_layers=2, aux_mode="", num_task_tokens=0, vit_layers=1))
    eng.init_random(seed=1)
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _lookup_equals_plain(eng, ids, None, None, 12, 4, which=("true", "wrong"), graph=())


# ------------------------------------------------------------------------------------------------ 6. the model API
def _sd(W):
    return {k.replace("model.vision_tower.vision_tower.", "model.vision_tower.vision_tower.vision_model.")
            if k.startswith("model.vision_tower.vision_tower.") else k: v for k, v in W.items()}


def test_model_generate_with_lookup_equals_without():
    _ops()
    from oracle import cases
    from visper_lm_amd.model import OlaLlavaLlamaConfig, OlaLlavaLlamaForCausalLM
    ocfg, W, batch, g = cases.tiny_llama_case()
    model = OlaLlavaLlamaForCausalLM(OlaLlavaLlamaConfig(**vars(ocfg)), init="empty")
    model.load_state_dict(_sd(W), strict=True)
    model.reload_frozen()
    ids, img = batch["input_ids"][:1], batch["images"][:1].cuda()
    want = model.generate(ids, images=img, max_new_tokens=8)
    got = model.generate(ids, images=img, max_new_tokens=8, prompt_lookup_num_tokens=3)
    assert got.shape == (1, 8) and got.dtype == torch.long and torch.equal(got, want)
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=8, prompt_lookup_num_tokens=3, max_matching_ngram_size=3), want)
    with pytest.raises(ValueError, match="do_sample"):
        model.generate(ids, images=img, max_new_tokens=8, prompt_lookup_num_tokens=3, do_sample=True)
