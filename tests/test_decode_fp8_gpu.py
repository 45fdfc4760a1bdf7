"""FP8 weight-only decoding on the GPU: the quantiser kernel against the CPU contract (quant.py), the W8A16 skinny GEMM against the fp32
product on the dequantised weights under the bf16 kernel's own bounds, the engine's fp8 decode steps teacher-forced against the label-less
forward on the same quantised engine, fp8 vs bf16 greedy tokens, graph capture, staleness after an optimizer step, and a record of what the
format itself costs against the un-quantised model."""
import contextlib
import warnings

import pytest
import torch

from parity import check, log, max_rel

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# the weight shapes of both architectures and the tiny cases (tests/test_generate_gpu.py SHAPES; every K is a multiple of 16 already)
SHAPES = [(6144, 4096), (4096, 4096), (4096, 14336), (128256, 4096), (9216, 3072), (3072, 3072), (3072, 8192), (32064, 3072),
          (384, 128), (128, 128), (128, 256), (1000, 256), (136, 128)]


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops
    return ops


def _weight(N, K, g, spread=True):
    """randn * 0.02 as the decode tests draw it; spread: rows times 2^-3 .. 2^3, so that the row scales differ (a kernel that forgets the
    scale, or applies it after a rounding point, fails)"""
    w = torch.randn(N, K, device="cuda", generator=g) * 0.02
    if spread:
        w = w * torch.exp2(torch.randint(-3, 4, (N, 1), device="cuda", generator=g).float())
    return w.to(BF16)


def _ref_gemm(a, w):
    return a.float() @ w.float().t()


# ------------------------------------------------------------------------------------------------ quantiser
def test_quant_rows_kernel_matches_the_cpu_contract_exactly():
    ops = _ops()
    from visper_lm_amd import quant
    g = torch.Generator(device="cuda").manual_seed(0)
    for N, K in SHAPES:
        w = _weight(N, K, g)
        if N == 384:                                                   # the special rows of the host test, through the kernel as well
            w[3] = 0
            w[5, 7] = 3.0e4
            w[6] = torch.randint(0, 128, (K,), device="cuda", generator=g).to(torch.int16).view(BF16)
        w0 = w.clone()
        q, s = ops.quant_rows_e4m3(w)
        assert torch.equal(w, w0), "without write-back the weight is read only"
        q2, s2 = ops.quant_rows_e4m3(w, writeback=True)
        assert torch.equal(q, q2) and torch.equal(s, s2)
        q3, s3 = ops.quant_rows_e4m3(w0.clone())
        assert torch.equal(q, q3) and torch.equal(s, s3), "a second call gives identical output"
        wb = w.cpu()
        for r0 in range(0, N, 16384):                                  # the CPU reference in row blocks (float64 temporaries)
            r1 = min(N, r0 + 16384)
            qc, sc = quant.quantize_rows_pow2(w0[r0:r1].cpu())
            assert torch.equal(q[r0:r1].cpu(), qc), (N, K, r0)
            assert torch.equal(s[r0:r1].cpu(), sc), (N, K, r0)
            deq = quant.dequantize(qc, sc)
            assert torch.equal(wb[r0:r1].float(), deq), (N, K, r0)    # write-back == dequantize(...) exactly
        # quantising the written-back weights again changes nothing the GEMM sees
        q4, s4 = ops.quant_rows_e4m3(w.clone(), writeback=False)
        if N * K <= 2 ** 24:
            assert torch.equal(quant.dequantize(q4.cpu(), s4.cpu()), wb.float())


# ------------------------------------------------------------------------------------------------ skinny GEMM
@pytest.mark.parametrize("M", [1, 2, 5, 8, 16])
def test_decode_gemm_w8_plain_and_fp32_out(M):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(M)
    worst, worst_bf16 = 0.0, 0.0
    for N, K in SHAPES:
        if N * K > 2 ** 28 and M not in (1, 8):
            continue
        a = torch.randn(M, K, device="cuda", generator=g).to(BF16)
        w = _weight(N, K, g)
        q, s = ops.quant_rows_e4m3(w, writeback=True)                   # w is now dequantize(q, s) (exactly: the test above)
        assert s.unique().numel() > 1
        ref = _ref_gemm(a, w)
        out32 = ops.decode_gemm(a, q, w_scale=s, out_f32=True)
        worst = max(worst, max_rel(out32, ref))
        worst_bf16 = max(worst_bf16, max_rel(ops.decode_gemm(a, w, out_f32=True), ref))
        out = ops.decode_gemm(a, q, w_scale=s)
        check(f"decode_gemm_w8 bf16 out M={M} N={N} K={K}", max_rel(out, ref), 5e-3)
        log(f"decode_gemm (bf16 kernel, written-back weights) bf16 out M={M} N={N} K={K}", max_rel(ops.decode_gemm(a, w), ref))
        assert torch.equal(ops.decode_gemm(a, q, w_scale=s, out_f32=True), out32), (N, K)      # run to run bit-identical
        assert torch.equal(ops.decode_gemm(a, q, w_scale=s), out), (N, K)
    log(f"decode_gemm (bf16 kernel, written-back weights) fp32 out M={M}", worst_bf16)
    check(f"decode_gemm_w8 fp32 out M={M}", worst, 5e-6)


@pytest.mark.parametrize("M", [1, 5, 16])
def test_decode_gemm_w8_epilogues_and_norm_prologue(M):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(100 + M)
    for H, I in ((4096, 14336), (3072, 8192), (128, 256)):
        x = torch.randn(M, H, device="cuda", generator=g).to(BF16)
        gamma = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).to(BF16)
        wgu = ops.interleave_gate_up(_weight(2 * I, H, g))
        q, s = ops.quant_rows_e4m3(wgu, writeback=True)
        # RMSNorm prologue + SwiGLU epilogue against vp_rmsnorm_fwd -> fp32 product (bf16-rounded gate_up) -> vp_swiglu_fwd
        xn, _ = ops.rmsnorm_fwd(x, gamma, 1e-5)
        want = ops.swiglu_fwd(_ref_gemm(xn, wgu).to(BF16))
        got = ops.decode_gemm(x, q, w_scale=s, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL)
        check(f"decode_gemm_w8 norm+swiglu M={M} H={H} I={I}", max_rel(got, want), 2e-3)
        log(f"decode_gemm (bf16 kernel) norm+swiglu M={M} H={H} I={I}",
            max_rel(ops.decode_gemm(x, wgu, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL), want))
        assert torch.equal(got, ops.decode_gemm(x, q, w_scale=s, norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_IL))
        # [gate | up] halves (IFT layout): the same rows in another order, each with its own scale
        halves = lambda t: torch.cat([t.view(I // 8, 2, 8, -1)[:, 0].reshape(I, -1), t.view(I // 8, 2, 8, -1)[:, 1].reshape(I, -1)], 0).contiguous()
        got_h = ops.decode_gemm(x, halves(q), w_scale=halves(s).view(-1), norm_w=gamma, eps=1e-5, epi=ops.EPI_SWIGLU_HALVES)
        check(f"decode_gemm_w8 swiglu halves == interleaved M={M} H={H}", max_rel(got_h, got), 0.0)
        # residual epilogue (down_proj): bf16(bf16(acc) + residual)
        act = torch.randn(M, I, device="cuda", generator=g).to(BF16)
        wd = _weight(H, I, g)
        qd, sd = ops.quant_rows_e4m3(wd, writeback=True)
        res = torch.randn(M, H, device="cuda", generator=g).to(BF16)
        want = (_ref_gemm(act, wd).to(BF16).float() + res.float())
        got = ops.decode_gemm(act, qd, w_scale=sd, residual=res)
        check(f"decode_gemm_w8 residual M={M} H={H} K={I}", max_rel(got, want), 5e-3)
        log(f"decode_gemm (bf16 kernel) residual M={M} H={H} K={I}", max_rel(ops.decode_gemm(act, wd, residual=res), want))
        assert torch.equal(got, ops.decode_gemm(act, qd, w_scale=sd, residual=res))
        # norm prologue alone: the rounding points of rmsnorm_fwd, then the product
        w2 = _weight(136, H, g)
        q2, s2 = ops.quant_rows_e4m3(w2, writeback=True)
        got = ops.decode_gemm(x, q2, w_scale=s2, norm_w=gamma, eps=1e-5, out_f32=True)
        check(f"decode_gemm_w8 norm prologue M={M} H={H}", max_rel(got, _ref_gemm(xn, w2)), 1e-6)
        log(f"decode_gemm (bf16 kernel) norm prologue M={M} H={H}",
            max_rel(ops.decode_gemm(x, w2, norm_w=gamma, eps=1e-5, out_f32=True), _ref_gemm(xn, w2)))
        assert torch.equal(got, ops.decode_gemm(x, q2, w_scale=s2, norm_w=gamma, eps=1e-5, out_f32=True))


# ------------------------------------------------------------------------------------------------ engines
def _engine_case(arch, quantize=True, lm_head=True):
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.engine import Engine
    ocfg, W, batch, g = cases.tiny_llama_case(arch)
    eng = Engine(VisperConfig(**vars(ocfg)))
    eng.load_weights(W)
    if quantize:
        eng.quantize_decoder(lm_head=lm_head)
        assert eng.dequantized()
    return eng, batch


def _full_width_llama_engine(layers=2, quantize=True):
    from visper_lm_amd.config import llama3_8b
    from visper_lm_amd.engine import Engine
    cfg = llama3_8b(num_hidden_layers=layers, aux_mode="", num_task_tokens=0, vit_layers=1)
    eng = Engine(cfg)
    eng.init_random(seed=1)
    if quantize:
        eng.quantize_decoder(lm_head=True)
    return eng


@contextlib.contextmanager
def _bf16_decode(eng):
    """decode through the bf16 kernels on the same (written-back) weights: the fp8 copies hidden for the block"""
    fq, eng.fq = eng.fq, None
    try:
        yield
    finally:
        eng.fq = fq


def _recompute_logits(eng, ids, toks, images):
    """logits_of over prompt + generated tokens -> the N rows the decode steps predicted from"""
    from visper_lm_amd import decode
    full = torch.cat([ids, toks.cpu()], 1)
    if images is not None:
        plan = eng.build_plan(full, None, None)
        x, *_ = eng._embed(images, plan)
    else:
        x, plan = decode.text_plan(eng, full, None)
    dec = eng._decoder_fwd(x, plan, compute_grads=False)
    lg = eng.logits_of(dec["hidden"], plan)                                  # [1, S, V]
    L, N = int(plan["lens_host"][0]), toks.shape[1]
    return lg[0, L - N - 1:L - 1]


def _teacher_forced(eng, ids, images, N, name, bound):
    """test_generate_gpu._teacher_forced on a quantised engine: the fp8 path's step logits against logits_of over prompt + generated tokens
    (asserted), the bf16 path's own deviation on the same engine beside it (logged)."""
    from visper_lm_amd import decode
    assert eng.dequantized()
    toks, kept, sess = decode.generate(eng, ids, None, images, None, max_new_tokens=N, return_logits=True)
    assert sess.fq is not None, "the session must have decoded from the fp8 copies"
    want = _recompute_logits(eng, ids, toks, images)
    worst = max(max_rel(kept[i][0], want[i]) for i in range(N))
    with _bf16_decode(eng):
        toks_b, kept_b, sess_b = decode.generate(eng, ids, None, images, None, max_new_tokens=N, return_logits=True)
        assert sess_b.fq is None
    want_b = _recompute_logits(eng, ids, toks_b, images)
    log(f"teacher-forced decode logits {name}: bf16 path on the same quantised engine", max(max_rel(kept_b[i][0], want_b[i]) for i in range(N)))
    check(f"teacher-forced fp8 decode logits {name}", worst, bound)
    return (toks, kept, want), (toks_b, kept_b, want_b)


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_engine_fp8_decode_teacher_forced_tiny(arch):
    _ops()
    eng, batch = _engine_case(arch)
    ids = batch["input_ids"][:1]
    _teacher_forced(eng, ids, batch["images"][:1].cuda(), 12, f"tiny {arch} with image", 2e-2)
    text = ids[:, :24][ids[:, :24] >= 0][None]                            # text-only prompt: the <image> token dropped
    _teacher_forced(eng, text, None, 12, f"tiny {arch} text-only", 2e-2)


def test_engine_fp8_decode_teacher_forced_full_width_llama():
    _ops()
    eng = _full_width_llama_engine()
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _teacher_forced(eng, ids, None, 12, "full-width Llama-3 2 layers", 3e-2)


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_fp8_and_bf16_decode_agree_on_greedy_tokens(arch):
    """On a quantised engine both paths compute the same model: their greedy tokens agree wherever the bf16 path's top-1 / top-2 gap exceeds
    twice the larger of the two measured logit errors against the full recompute (the near-tie rule of _oracle_argmax_check).  The first
    disagreement ends the comparison (the sequences differ from there) and must itself be a near-tie."""
    _ops()
    eng, batch = _engine_case(arch)
    ids = batch["input_ids"][:1]
    N = 16
    (t8, k8, w8), (tb, kb, wb) = _teacher_forced(eng, ids, batch["images"][:1].cuda(), N, f"tiny {arch} with image, {N} tokens", 2e-2)
    err8 = max(float((k8[i][0] - w8[i]).abs().max()) for i in range(N))
    errb = max(float((kb[i][0] - wb[i]).abs().max()) for i in range(N))
    err = max(err8, errb)
    near, bad, seen = 0, [], 0
    for i in range(N):
        if i > 0 and not torch.equal(t8[0, :i], tb[0, :i]):
            break
        seen += 1
        top2 = kb[i][0].topk(2)
        if float(top2.values[0] - top2.values[1]) <= 2 * err:
            near += 1
        elif int(t8[0, i]) != int(tb[0, i]):
            bad.append(i)
    log(f"fp8 vs bf16 decode tiny {arch}: logit error fp8 path (max abs)", err8)
    log(f"fp8 vs bf16 decode tiny {arch}: logit error bf16 path (max abs)", errb)
    log(f"fp8 vs bf16 decode tiny {arch}: positions compared of {N}", seen)
    log(f"fp8 vs bf16 decode tiny {arch}: near-ties (top-2 gap <= {2 * err:.3g})", near)
    assert not bad, (arch, bad)
    assert near < seen, "every position was a near-tie: the comparison showed nothing"


def test_fp8_ragged_batch_eos_pad_eager_equals_graph(monkeypatch):
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
    monkeypatch.setenv("VP_DECODE_GRAPH", "0")
    eager, _, s_e = decode.generate(eng, ids, am, None, None, max_new_tokens=N, return_logits=True)
    monkeypatch.setenv("VP_DECODE_GRAPH", "1")                            # the environment switch itself, not the use_graph argument
    captured, _, s_g = decode.generate(eng, ids, am, None, None, max_new_tokens=N, return_logits=True)
    assert s_e.fq is not None and s_g.fq is not None and not s_e.use_graph and s_g.use_graph and s_g.replays == N - 1
    assert torch.equal(eager, captured)
    for b, p in enumerate(prompts):                                        # each row decodes as it does alone
        single = decode.generate(eng, p[None], None, None, None, max_new_tokens=N)
        assert torch.equal(captured[b], single[0]), b
    # EOS: the token sequence 0 emits at step 3 ends it; later positions are pad, the others run on; eager == captured there too
    eos = int(eager[0, 3])
    out_g = decode.generate(eng, ids, am, None, None, max_new_tokens=N, eos_token_id=[eos], pad_token_id=-7)
    monkeypatch.setenv("VP_DECODE_GRAPH", "0")
    out_e = decode.generate(eng, ids, am, None, None, max_new_tokens=N, eos_token_id=[eos], pad_token_id=-7)
    assert torch.equal(out_g, out_e)
    for b in range(3):
        row = eager[b].tolist()
        stop = row.index(eos) if eos in row else None
        if stop is None:
            assert out_e[b].tolist() == row[:out_e.shape[1]]
        else:
            assert out_e[b, :stop + 1].tolist() == row[:stop + 1] and (out_e[b, stop + 1:] == -7).all()


# ------------------------------------------------------------------------------------------------ staleness
def _sd(W):
    return {k.replace("model.vision_tower.vision_tower.", "model.vision_tower.vision_tower.vision_model.")
            if k.startswith("model.vision_tower.vision_tower.") else k: v for k, v in W.items()}


def test_stale_fp8_copies_are_dropped_with_one_warning_after_an_optimizer_step():
    _ops()
    from oracle import cases
    from visper_lm_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    ocfg, W, batch, _ = cases.tiny_ift_case()
    model = LlavaLlamaForCausalLM(LlavaConfig(**vars(ocfg)), init="empty")
    model.load_state_dict(_sd(W), strict=True)
    ids = batch["input_ids"][:1, :24]
    ids = torch.where(ids < 0, torch.ones_like(ids), ids)                  # text-only prompt: no <image> token
    assert model.quantize_for_generation() is model
    eng = model._get_engine()
    assert eng.dequantized()
    with warnings.catch_warnings(record=True) as rec0:                     # current copies: no warning
        warnings.simplefilter("always")
        toks_q = model.generate(ids, max_new_tokens=8)
    assert not [r for r in rec0 if "stale" in str(r.message)]
    assert toks_q.shape == (1, 8)
    kw = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"], images=batch["images"].cuda())
    model(**kw).loss.backward()
    model.optimizer_step(lr=1e-2)
    with pytest.warns(RuntimeWarning, match="stale") as rec:
        toks = model.generate(ids, max_new_tokens=8)
    assert len([r for r in rec if "stale" in str(r.message)]) == 1
    assert not eng.dequantized() and eng.fq is None
    with warnings.catch_warnings(record=True) as rec2:                     # warned once: the next call is silent and still bf16
        warnings.simplefilter("always")
        toks2 = model.generate(ids, max_new_tokens=8)
    assert not [r for r in rec2 if "stale" in str(r.message)]
    assert torch.equal(toks, toks2)
    fresh = LlavaLlamaForCausalLM(LlavaConfig(**vars(ocfg)), init="empty")  # a never-quantised copy of the updated model
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=True)
    assert not fresh._get_engine().dequantized()
    assert torch.equal(fresh.generate(ids, max_new_tokens=8), toks)
    # re-quantising picks the updated weights up
    model.quantize_for_generation()
    assert eng.dequantized()


# ------------------------------------------------------------------------------------------------ what the format costs (a record, no gate)
def _cost(name, eng_ref, eng_q, ids, images, N=16):
    from visper_lm_amd import decode
    t_ref = decode.generate(eng_ref, ids, None, images, None, max_new_tokens=N)
    t_q = decode.generate(eng_q, ids, None, images, None, max_new_tokens=N)
    a = _recompute_logits(eng_ref, ids, t_ref, images)
    b = _recompute_logits(eng_q, ids, t_ref, images)                       # the same token sequence through both models
    log(f"quantisation cost {name}: logit deviation, quantised vs bf16 model (max abs / max |logit|)", float((a - b).abs().max() / a.abs().max()))
    agree = 0
    while agree < N and int(t_ref[0, agree]) == int(t_q[0, agree]):
        agree += 1
    log(f"quantisation cost {name}: greedy tokens equal before the first difference, of {N}", agree)
    log(f"quantisation cost {name}: greedy tokens equal position by position, of {N}", int((t_ref == t_q).sum()))


def test_record_quantisation_cost():
    _ops()
    for lm_head in (False, True):
        ref, batch = _engine_case("llama", quantize=False)
        qe, _ = _engine_case("llama", lm_head=lm_head)
        ids = batch["input_ids"][:1]
        _cost(f"tiny llama with image (lm_head {'fp8' if lm_head else 'bf16'})", ref, qe, ids, batch["images"][:1].cuda())
    ref, qe = _full_width_llama_engine(quantize=False), _full_width_llama_engine()
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    _cost("full-width Llama-3 2 layers (lm_head fp8)", ref, qe, ids, None)
