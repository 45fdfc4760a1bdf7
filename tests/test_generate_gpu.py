"""KV-cached generate() on the GPU: the decode kernels (skinny GEMM, RoPE + KV append, decode attention) against torch / the training
kernels, the engine's decode steps teacher-forced against the label-less forward, the model API against the CPU oracle's full recompute,
ragged batches, EOS / padding, graph capture and sampling."""
import math

import numpy as np
import pytest
import torch

from parity import check, log, max_rel

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops
    return ops


def _ref_gemm(a, w):
    return a.float() @ w.float().t()


# ------------------------------------------------------------------------------------------------ skinny GEMM
SHAPES = [(6144, 4096), (4096, 4096), (4096, 14336), (128256, 4096), (9216, 3072), (3072, 3072), (3072, 8192), (32064, 3072),
          (384, 128), (128, 128), (128, 256), (1000, 256), (136, 128)]


@pytest.mark.parametrize("M", [1, 2, 5, 8, 16])
def test_decode_gemm_plain_and_fp32_out(M):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(M)
    worst = 0.0
    for N, K in SHAPES:
        if N * K > 2 ** 28 and M not in (1, 8):
            continue
        a = torch.randn(M, K, device="cuda", generator=g).to(BF16)
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF16)
        ref = _ref_gemm(a, w)
        out32 = ops.decode_gemm(a, w, out_f32=True)
        worst = max(worst, max_rel(out32, ref))
        out = ops.decode_gemm(a, w)
        check(f"decode_gemm bf16 out M={M} N={N} K={K}", max_rel(out, ref), 5e-3)
        assert torch.equal(ops.decode_gemm(a, w, out_f32=True), out32), (N, K)          # run to run bit-identical (split-K combine in order)
    check(f"decode_gemm fp32 out M={M}", worst, 5e-6)


@pytest.mark.parametrize("M", [1, 5, 16])
def test_decode_gemm_epilogues_and_norm_prologue(M):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(100 + M)
    for H, I in ((4096, 14336), (3072, 8192), (128, 256)):
        x = torch.randn(M, H, device="cuda", generator=g).to(BF16)
        gamma = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).to(BF16)
        wgu = ops.interleave_gate_up((torch.randn(2 * I, H, device="cuda", generator=g) * 0.02).to(BF16))
        # RMSNorm prologue + SwiGLU epilogue against vp_rmsnorm_fwd -> fp32 product (bf16-rounded gate_up) -> vp_swiglu_fwd
        xn, _ = ops.rmsnorm_fwd(x, gamma, 1e-5)
        want = ops.swiglu_fwd(_ref_gemm(xn, wgu).to(BF16))
        got = ops.decode_gemm(x, wgu, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL)
        check(f"decode_gemm norm+swiglu M={M} H={H} I={I}", max_rel(got, want), 2e-3)
        assert torch.equal(got, ops.decode_gemm(x, wgu, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL))
        # [gate | up] halves (IFT layout)
        halves = torch.cat([wgu.view(I // 8, 2, 8, H)[:, 0].reshape(I, H), wgu.view(I // 8, 2, 8, H)[:, 1].reshape(I, H)], 0).contiguous()
        got_h = ops.decode_gemm(x, halves, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_HALVES)
        check(f"decode_gemm swiglu halves == interleaved M={M} H={H}", max_rel(got_h, got), 0.0)
        # residual epilogue (down_proj): bf16(bf16(acc) + residual)
        act = torch.randn(M, I, device="cuda", generator=g).to(BF16)
        wd = (torch.randn(H, I, device="cuda", generator=g) * 0.02).to(BF16)
        res = torch.randn(M, H, device="cuda", generator=g).to(BF16)
        want = (_ref_gemm(act, wd).to(BF16).float() + res.float())
        got = ops.decode_gemm(act, wd, residual=res)
        check(f"decode_gemm residual M={M} H={H} K={I}", max_rel(got, want), 5e-3)
        # norm prologue alone: the rounding points of rmsnorm_fwd, then the product
        w2 = (torch.randn(136, H, device="cuda", generator=g) * 0.02).to(BF16)
        got = ops.decode_gemm(x, w2, norm_w=gamma, eps=1e-5, out_f32=True)
        check(f"decode_gemm norm prologue M={M} H={H}", max_rel(got, _ref_gemm(xn, w2)), 1e-6)


# ------------------------------------------------------------------------------------------------ RoPE + append
def test_decode_rope_append_writes_only_row_pos():
    ops = _ops()
    B, Hq, Hkv, D, Smax = 3, 8, 2, 32, 40
    g = torch.Generator(device="cuda").manual_seed(7)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", generator=g).to(BF16)
    cache = torch.full((B, Smax, 2, Hkv * D), 7.0, device="cuda", dtype=BF16)
    k4 = cache[:, :, 0].unflatten(-1, (Hkv, D))
    v4 = cache[:, :, 1].unflatten(-1, (Hkv, D))
    q = torch.empty(B, Hq * D, device="cuda", dtype=BF16)
    pos = torch.tensor([0, 17, 39], device="cuda", dtype=torch.int32)
    cos, sin = ops.rope_tables(64, D, 10000.0, "cuda")
    ops.decode_rope_append(qkv, q, k4, v4, cos, sin, pos, Hq, Hkv, D)
    want = qkv.clone()
    ops.rope_(want, B, 64, Hq + Hkv, D, cos, sin, pos=pos)                 # the training kernel with position ids
    assert torch.equal(q, want[:, :Hq * D])
    mask = torch.zeros(B, Smax, dtype=torch.bool, device="cuda")
    mask[torch.arange(B), pos.long()] = True
    assert (cache[~mask] == 7.0).all()                                     # every other row untouched
    for b in range(B):
        p = int(pos[b])
        assert torch.equal(cache[b, p, 0], want[b, Hq * D:(Hq + Hkv) * D])
        assert torch.equal(cache[b, p, 1], qkv[b, (Hq + Hkv) * D:])


# ------------------------------------------------------------------------------------------------ decode attention
def _ref_attn(q, k, v, lens, window, scale):
    B, Hq, D = q.shape
    Hkv = k.shape[2]
    out = torch.zeros(B, Hq, D, device=q.device)
    for b in range(B):
        L = int(lens[b])
        lo = max(0, L - window) if window else 0
        kk = k[b, lo:L].float().repeat_interleave(Hq // Hkv, 1)           # [n, Hq, D]
        vv = v[b, lo:L].float().repeat_interleave(Hq // Hkv, 1)
        s = torch.einsum("hd,nhd->hn", q[b].float(), kk) * scale
        out[b] = torch.einsum("hn,nhd->hd", s.softmax(-1), vv)
    return out


@pytest.mark.parametrize("D,Hq,Hkv", [(32, 4, 2), (96, 32, 32), (128, 32, 8), (128, 8, 8)])
def test_decode_attn_against_fp32_and_training_forward(D, Hq, Hkv):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(D + Hq)
    lens = [1, 777, 8192, 300] if D != 96 else [1, 777, 2100]
    B, Smax = len(lens), max(lens)
    k = torch.randn(B, Smax, Hkv, D, device="cuda", generator=g).to(BF16)
    v = torch.randn(B, Smax, Hkv, D, device="cuda", generator=g).to(BF16)
    q = torch.randn(B, Hq * D, device="cuda", generator=g).to(BF16)
    kl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    for window in (0, 500):
        got = ops.decode_attn(q, k, v, kl, Hq, window=window)
        want = _ref_attn(q.view(B, Hq, D), k, v, lens, window, scale)
        check(f"decode_attn vs fp32 D={D} {Hq}:{Hkv} window={window}", max_rel(got.view(B, Hq, D), want), 1e-3)
        assert torch.equal(got, ops.decode_attn(q, k, v, kl, Hq, window=window))
    # row p of the training forward (causal, the same q placed at row p = len - 1 of each sequence)
    Sq = max(lens)
    qf = torch.zeros(B, Sq, Hq, D, device="cuda", dtype=BF16)
    for b, L in enumerate(lens):
        qf[b, L - 1] = q.view(B, Hq, D)[b]
    for window in (0, 500):
        o, _ = ops.attn_fwd(qf, k, v, causal=True, window=window, kv_len=kl)
        rows = torch.stack([o[b, L - 1] for b, L in enumerate(lens)])
        got = ops.decode_attn(q, k, v, kl, Hq, window=window).view(B, Hq, D)
        check(f"decode_attn vs vp_attn_fwd row D={D} {Hq}:{Hkv} window={window}", max_rel(got, rows), 1.5e-3)


# ------------------------------------------------------------------------------------------------ engine, teacher-forced
def _engine_case(arch):
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.engine import Engine
    ocfg, W, batch, g = cases.tiny_llama_case(arch)
    eng = Engine(VisperConfig(**vars(ocfg)))
    eng.load_weights(W)
    return eng, batch


def _full_width_llama_engine(layers=2):
    from visper_lm_amd.config import llama3_8b
    from visper_lm_amd.engine import Engine
    cfg = llama3_8b(num_hidden_layers=layers, aux_mode="", num_task_tokens=0, vit_layers=1)
    eng = Engine(cfg)
    eng.init_random(seed=1)
    return eng


def _teacher_forced(eng, ids, images, N, name, bound):
    """Greedy N tokens; the logits of every decode step against logits_of over prompt + generated tokens (last valid row)."""
    from visper_lm_amd import decode
    toks, kept, _ = decode.generate(eng, ids, None, images, None, max_new_tokens=N, return_logits=True)
    full = torch.cat([ids, toks.cpu()], 1)
    plan = eng.build_plan(full, None, None) if images is not None else None
    if images is not None:
        x, *_ = eng._embed(images, plan)
    else:
        x, plan = decode.text_plan(eng, full, None)
    dec = eng._decoder_fwd(x, plan, compute_grads=False)
    lg = eng.logits_of(dec["hidden"], plan)                                  # [1, S, V]
    L = int(plan["lens_host"][0])
    worst = 0.0
    for i in range(N):
        want = lg[0, L - N - 1 + i]
        worst = max(worst, max_rel(kept[i][0], want))
    check(f"teacher-forced decode logits {name}", worst, bound)
    return toks


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_engine_decode_teacher_forced_tiny(arch):
    _ops()
    eng, batch = _engine_case(arch)
    ids = batch["input_ids"][:1]
    _teacher_forced(eng, ids, batch["images"][:1].cuda(), 12, f"tiny {arch} with image", 2e-2)
    text = ids[:, :24][ids[:, :24] >= 0][None]                            # text-only prompt: the <image> token dropped
    _teacher_forced(eng, text, None, 12, f"tiny {arch} text-only", 2e-2)
    with pytest.raises(ValueError, match="token ids"):                     # an <image> token without images is refused on the host
        from visper_lm_amd import decode
        decode.generate(eng, ids, None, None, None, max_new_tokens=2)


def test_engine_decode_teacher_forced_full_width_llama():
    _ops()
    eng = _full_width_llama_engine()
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _teacher_forced(eng, ids, None, 12, "full-width Llama-3 2 layers", 3e-2)


# ------------------------------------------------------------------------------------------------ model API vs the CPU oracle
def _oracle_argmax_check(model, W, ocfg, ids, images, toks, name):
    """Each HIP token must be the oracle's argmax wherever the oracle's top-1 / top-2 gap exceeds the measured logit error (the engine's
    per-step logits against the oracle's full recompute at the same positions, x 2)."""
    import oracle.visper_oracle as O
    from visper_lm_amd import decode
    Wq = {k: v.detach().cpu().to(BF16).float() for k, v in W.items()}
    full = torch.cat([ids, toks.cpu()], 1)
    with torch.no_grad():
        if images is not None:
            feats = O.encode_images(images.cpu().to(BF16).float(), Wq, ocfg)
            _, am, emb, _ = O.prepare_inputs_labels_for_multimodal(full, None, None, feats, Wq, ocfg)
        else:
            emb, am = Wq["model.embed_tokens.weight"][full], torch.ones_like(full, dtype=torch.bool)
        hidden, _ = O.decoder_forward(emb, None, am, Wq, ocfg)
        logits = torch.nn.functional.linear(hidden, Wq["lm_head.weight"]).float()[0]
    N = toks.shape[1]
    L = logits.shape[0]
    eng = model._get_engine()
    toks2, kept, _ = decode.generate(eng, ids, None, None if images is None else images.cuda(), None, max_new_tokens=N, return_logits=True)
    assert torch.equal(toks2.cpu(), toks.cpu())
    err = max(float((kept[i][0].cpu() - logits[L - N - 1 + i]).abs().max()) for i in range(N))
    scale = float(logits[L - N - 1:].abs().max())
    check(f"generate logits vs oracle {name} (max abs / max |logit|)", err / scale, 3e-2)
    near, bad = 0, []
    for i in range(N):
        top2 = logits[L - N - 1 + i].topk(2)
        if float(top2.values[0] - top2.values[1]) <= 2 * err:
            near += 1
        elif int(top2.indices[0]) != int(toks[0, i]):
            bad.append(i)
    log(f"generate vs oracle {name}: near-ties (top-2 gap <= {2 * err:.3g}) of {N}", near)
    assert not bad, (name, bad)
    assert near < N, "every position was a near-tie: the comparison showed nothing"


def _sd(W):
    return {k.replace("model.vision_tower.vision_tower.", "model.vision_tower.vision_tower.vision_model.")
            if k.startswith("model.vision_tower.vision_tower.") else k: v for k, v in W.items()}


def test_generate_pt_with_image_and_ift_text_only_match_oracle():
    _ops()
    from oracle import cases
    from visper_lm_amd.model import LlavaConfig, LlavaLlamaForCausalLM, OlaLlavaLlamaConfig, OlaLlavaLlamaForCausalLM
    ocfg, W, batch, g = cases.tiny_llama_case()
    model = OlaLlavaLlamaForCausalLM(OlaLlavaLlamaConfig(**vars(ocfg)), init="empty")
    model.load_state_dict(_sd(W), strict=True)
    model.reload_frozen()
    ids, img = batch["input_ids"][:1], batch["images"][:1]
    toks = model.generate(ids, images=img.cuda(), max_new_tokens=16)
    assert toks.shape == (1, 16) and toks.dtype == torch.long
    _oracle_argmax_check(model, W, ocfg, ids, img, toks, "tiny PT Ola-Llama + image")
    ocfg2, W2, batch2, _ = cases.tiny_ift_case()
    ift = LlavaLlamaForCausalLM(LlavaConfig(**vars(ocfg2)), init="empty")
    ift.load_state_dict(_sd(W2), strict=True)
    ids2 = batch2["input_ids"][:1, :24]
    ids2 = torch.where(ids2 < 0, torch.ones_like(ids2), ids2)              # text-only prompt: no <image> token
    toks2 = ift.generate(ids2, max_new_tokens=16)
    _oracle_argmax_check(ift, W2, ocfg2, ids2, None, toks2, "tiny IFT Llava text-only")


# ------------------------------------------------------------------------------------------------ ragged batch, EOS, graph, sampling
def test_ragged_batch_eos_pad_graph_and_sampling():
    _ops()
    from visper_lm_amd import decode
    eng, batch = _engine_case("llama")
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, 1000, (n,), generator=g) for n in (7, 19, 12)]
    T = max(len(p) for p in prompts)
    ids = torch.zeros(3, T, dtype=torch.long)
    am = torch.zeros(3, T, dtype=torch.long)
    for b, p in enumerate(prompts):                                        # left padding, as the eval scripts' tokenizers pad
        ids[b, T - len(p):] = p
        am[b, T - len(p):] = 1
    N = 10
    batched = decode.generate(eng, ids, am, None, None, max_new_tokens=N, use_graph=True)
    eager = decode.generate(eng, ids, am, None, None, max_new_tokens=N, use_graph=False)
    assert torch.equal(batched, eager)                                     # graph replay == eager launches
    for b, p in enumerate(prompts):
        single = decode.generate(eng, p[None], None, None, None, max_new_tokens=N)
        assert torch.equal(batched[b], single[0]), b
    # EOS: the token sequence 0 emits at step 3 ends it; later positions are pad, the others run on
    eos = int(batched[0, 3])
    out = decode.generate(eng, ids, am, None, None, max_new_tokens=N, eos_token_id=[eos], pad_token_id=-7)
    for b in range(3):
        row = batched[b].tolist()
        stop = row.index(eos) if eos in row else None
        if stop is None:
            assert out[b].tolist() == row[:out.shape[1]]
        else:
            assert out[b, :stop + 1].tolist() == row[:stop + 1] and (out[b, stop + 1:] == -7).all()
    assert out.shape[1] <= N
    # every row finished -> the loop stops early
    first = [int(batched[b, 0]) for b in range(3)]
    assert decode.generate(eng, ids, am, None, None, max_new_tokens=N, eos_token_id=first).shape[1] == 1
    # sampling: seeded runs reproduce; top_p -> 0 keeps only the top token = greedy
    s1 = decode.generate(eng, ids, am, None, None, max_new_tokens=N, do_sample=True, temperature=0.8, top_p=0.9,
                         generator=torch.Generator(device="cuda").manual_seed(11))
    s2 = decode.generate(eng, ids, am, None, None, max_new_tokens=N, do_sample=True, temperature=0.8, top_p=0.9,
                         generator=torch.Generator(device="cuda").manual_seed(11))
    assert torch.equal(s1, s2)
    s3 = decode.generate(eng, ids, am, None, None, max_new_tokens=N, do_sample=True, top_p=1e-9,
                         generator=torch.Generator(device="cuda").manual_seed(12))
    assert torch.equal(s3, batched)


def test_streamer_sees_prompt_then_each_token():
    _ops()
    from visper_lm_amd import decode
    eng, batch = _engine_case("llama")

    class S:
        def __init__(self):
            self.calls = []

        def put(self, v):
            self.calls.append(v.clone())

        def end(self):
            self.calls.append("end")

    s = S()
    ids = batch["input_ids"][:1, :16].clamp_min(1)
    toks = decode.generate(eng, ids, None, None, None, max_new_tokens=5, streamer=s)
    assert torch.equal(s.calls[0], ids) and s.calls[-1] == "end"
    assert torch.equal(torch.stack([c.cpu() for c in s.calls[1:-1]], 1), toks.cpu())
