"""vp_decode_select on the GPU against the CPU restatement of its contract (tests/select_ref.py, itself held against HF's processors in
test_decode_select_host.py), and generate() with the selector on the device against the plain path.  Kernel-level operands sit in sentinel
boxes (row stride > V, NaN in the padding, guard rows and columns around every output).  tests/SELECT_PATHS.md maps the cases."""
import functools

import numpy as np
import pytest
import torch

import select_ref as SR

pytestmark = pytest.mark.gpu
I32 = torch.int32
NEG_INF = float("-inf")


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_select(logits, seen=None, u=None, eos=None, pad=-7, finished=None, col=1, n_out=3, scores=True, **params):
    """One launch on boxed operands.  logits fp32 [R, V] (CPU), seen bool [R, V], u fp32 [R] or [steps, R], finished list -> dict of CPU
    results; asserts that the logits, the padding and everything around the outputs are as they were."""
    ops = _ops()
    R, V = logits.shape
    ld = V + 5
    box = torch.full((R + 2, ld), float("nan"))
    box[1:R + 1, :V] = logits
    box = box.cuda()
    before = _bits(box).clone()
    sbox = torch.full((R + 2, ld + 2), 777.0, device="cuda")
    tokb = torch.full((R + 2,), -99, device="cuda", dtype=I32)
    finb = torch.full((R + 2,), -99, device="cuda", dtype=I32)
    finb[1:R + 1] = 0 if finished is None else torch.tensor(finished, dtype=I32).cuda()
    outb = torch.full((R + 2, n_out + 2), -99, device="cuda", dtype=I32)
    colb = torch.tensor([-99, col, -99], device="cuda", dtype=I32)
    W = (V + 31) // 32
    seenb = None
    if seen is not None:
        seenb = torch.full((R + 2, W), 0x5A5A5A5A, dtype=I32)
        seenb[1:R + 1] = SR.pack_bits(seen)
        seenb = seenb.cuda()
    ops.decode_select(box[1:R + 1, :V], tokb[1:R + 1], outb[1:R + 1, 1:1 + n_out], colb[1:2], finb[1:R + 1],
                      seen=None if seenb is None else seenb[1:R + 1], u=None if u is None else u.cuda(),
                      eos=None if eos is None else torch.tensor(eos, dtype=I32).cuda(), pad=pad,
                      scores_out=sbox[1:R + 1, 1:1 + V] if scores else None, **params)
    torch.cuda.synchronize()
    assert torch.equal(_bits(box), before), "the logits or their padding changed"
    guard = sbox.clone()
    if scores:
        guard[1:R + 1, 1:1 + V] = 777.0
    assert (guard == 777.0).all(), "scores_out wrote outside its rows"
    assert tokb[0] == -99 and tokb[-1] == -99 and finb[0] == -99 and finb[-1] == -99 and colb.tolist() == [-99, col, -99]
    o = outb.cpu()
    inner = o[1:R + 1, 1:1 + n_out].clone()
    if 0 <= col < n_out:
        o[1:R + 1, 1 + col] = -99
    assert (o == -99).all(), "out wrote outside its column"
    res = dict(tok=tokb[1:R + 1].cpu().long(), out=inner[:, col].long() if 0 <= col < n_out else None, fin=finb[1:R + 1].cpu(), scores=sbox[1:R + 1, 1:1 + V].cpu() if scores else None)
    if seenb is not None:
        sb = seenb.cpu()
        assert (sb[0] == 0x5A5A5A5A).all() and (sb[-1] == 0x5A5A5A5A).all()
        res["seen"] = SR.unpack_bits(sb[1:R + 1], V)
        tailbits = W * 32 - V
        if tailbits:
            assert ((sb[1:R + 1, -1].numpy().view(np.uint32) >> np.uint32(V % 32)) == 0).all(), "bits past V in the bitmap's tail word"
    return res


def _same_scores(got, want, where=None):
    """bit for bit on the finite values, and the same -inf mask"""
    gm, wm = got == NEG_INF, want == NEG_INF
    if where is not None:
        gm, wm, got, want = gm[where], wm[where], got[where], want[where]
    if not torch.equal(gm, wm):
        return False
    return torch.equal(_bits(got[~wm]), _bits(want[~wm]))


def _draw(R, V, sigma, seed, special=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g) * sigma
    if special and V >= 8:
        x[0, :8] = torch.tensor([0.0, -0.0, NEG_INF, -1.5, 2.0, 2.0, -3.0, 1.0])
    seen = torch.rand(R, V, generator=g) < 0.3
    if special and V >= 8:
        seen[0, :8] = torch.tensor([True, True, True, True, True, False, True, False])      # zero, -inf, negative and positive penalised
    return x, seen


# ------------------------------------------------------------------------------------------------ kernel: scores, top-k, greedy
# V: 1 and 31 below one wave, 33 a bitmap tail word past one full word, 97 / 1000 / 4099 no multiple of 64 or 1024, 4099 past one 4096-token
# CDF bin, both production vocabularies; R = 64 where a row is cheap
GRID = [(1, 1), (1, 3), (31, 3), (33, 64), (97, 3), (1000, 64), (4099, 3), (32064, 3), (128256, 1)]


@pytest.mark.parametrize("V,R", GRID)
def test_scores_bit_exact_and_greedy_token(V, R):
    x, seen = _draw(R, V, 3.0, 100 + V + R)
    u = torch.rand(R, generator=torch.Generator().manual_seed(V + R))
    for temperature in (0.2, 0.7, 1.0, 1.3):
        for theta in (1.0, 1.3, 0.8):
            for top_k in (0, 1, 2, 50, V, V + 5):
                ref = SR.ref_scores(x, seen, temperature, top_k, 1.0, theta)
                got = run_select(x, seen=seen, u=u, do_sample=True, temperature=temperature, top_k=top_k, repetition_penalty=theta)
                assert _same_scores(got["scores"], ref["scores"]), (V, R, temperature, theta, top_k)
                for r in range(R):                               # (the accepted set is pinned to <= 2 tokens in the CDF tests below)
                    assert int(got["tok"][r]) in SR.accepted(ref["scores"][r], float(u[r])).tolist(), (V, R, temperature, theta, top_k, r)
        # greedy: HF applies the penalty only; the token is the first index of the largest penalised score
        for theta in (1.0, 1.3, 0.8):
            ref = SR.ref_scores(x, seen, 1.0, 0, 1.0, theta)
            got = run_select(x, seen=seen, repetition_penalty=theta)
            assert _same_scores(got["scores"], ref["scores"]) and torch.equal(got["tok"], SR.ref_greedy(ref["scores"])), (V, R, theta)


def test_top_k_ties_are_all_kept():
    x = torch.full((2, 97), -5.0)
    x[0, [3, 40, 41, 90]] = 2.0                                  # k = 3: the third value is shared by 4 tokens, one beyond the first k
    x[0, 17] = 7.0
    x[0, 60] = 4.0
    x[1, :] = 1.25                                               # a row of one value: everything ties with the k-th
    got = run_select(x, u=torch.tensor([0.999, 0.5]), do_sample=True, top_k=3)
    assert sorted(torch.nonzero(got["scores"][0] > NEG_INF).flatten().tolist()) == [3, 17, 40, 41, 60, 90]
    assert (got["scores"][1] == 1.25).all()
    assert _same_scores(got["scores"], SR.ref_scores(x, top_k=3)["scores"])
    assert int(got["tok"][1]) == 48                              # 97 equal masses, u = 0.5: the 49th


def test_greedy_tie_eos_pad_finished_and_seen_bit():
    V = 33
    x = torch.randn(5, V, generator=torch.Generator().manual_seed(1))
    x[:, 7] = 9.0
    x[:, 32] = 9.0                                               # an exact tie of the maximum: the first index wins, as torch.argmax
    x[3, 2] = 9.5
    x[4, 31] = 9.5
    seen = torch.zeros(5, V, dtype=torch.bool)
    seen[0, 5] = seen[1, 32] = True
    for eos in (None, [7], [2, 7]):
        got = run_select(x, seen=seen, eos=eos, pad=-7, finished=[0, 1, 0, 0, 1], col=2, scores=False)
        assert got["tok"].tolist() == [7, 7, 7, 2, 31]           # always the raw choice
        assert got["out"].tolist() == [7, -7, 7, 2, -7]          # rows finished before emit pad
        e = eos or []
        assert got["fin"].tolist() == [int(7 in e), 1, int(7 in e), int(2 in e), 1]
        want = seen.clone()
        want[torch.arange(5), got["tok"]] = True                 # the raw token's bit, nothing else
        assert torch.equal(got["seen"], want)
    # with a penalty the seen maximum of row 1 (token 32) and the tie partner change places: 9 / 1.5 < 9
    seen[1, 7] = True
    got = run_select(x, seen=seen, repetition_penalty=1.5, scores=False)
    assert got["tok"].tolist() == [7, int(torch.argmax(SR.ref_scores(x, seen, penalty=1.5)["scores"][1])), 7, 2, 31]
    # a column outside the output is not written (run_select checks that nothing else was)
    got = run_select(x, col=3, n_out=3, scores=False)
    assert got["tok"].tolist() == [7, 7, 7, 2, 31]


# ------------------------------------------------------------------------------------------------ kernel: top-p
@functools.lru_cache(maxsize=None)
def _top_p_case(V, sigma, top_k):
    x, _ = _draw(3, V, sigma, 7 * V + int(sigma) + top_k, special=False)
    return x


@pytest.mark.parametrize("V", [97, 4099, 32064, 128256])
def test_top_p_mask_within_the_band(V):
    worst_band, worst_dev = 0, 0.0
    for sigma in (1.0, 3.0):
        for top_k in (0, 50):
            x = _top_p_case(V, sigma, top_k)
            for top_p in (1e-9, 0.05, 0.5, 0.9, 1.0):
                ref = SR.ref_scores(x, None, 0.7, top_k, top_p, 1.0)
                pop = ref["band"].sum(-1)
                assert int(pop.max()) <= 2, ("the draw puts too many tokens near the threshold", V, sigma, top_k, top_p, pop.tolist())
                worst_band = max(worst_band, int(pop.max()))
                got = run_select(x, u=torch.zeros(3), do_sample=True, temperature=0.7, top_k=top_k, top_p=top_p)
                kept = got["scores"] > NEG_INF
                diff = kept != ref["keep"]
                if diff.any():
                    thr = 1.0 - float(np.float32(top_p))
                    worst_dev = max(worst_dev, float((ref["tail"][diff] - thr).abs().max()))
                print(f"top-p V {V} sigma {sigma} top_k {top_k} top_p {top_p}: kept {ref['keep'].sum(-1).tolist()}, band {pop.tolist()}, "
                      f"decided differently {int(diff.sum())}")
                assert not (diff & ~ref["band"]).any(), (V, sigma, top_k, top_p, torch.nonzero(diff & ~ref["band"]).tolist())
                assert _same_scores(got["scores"], ref["scores"], ~ref["band"]), (V, sigma, top_k, top_p)
                assert kept[torch.arange(3), ref["s"].argmax(-1)].all()                  # the top token is always kept
    print(f"top-p V {V}: largest band population {worst_band}, largest tail-mass deviation of a differently decided token {worst_dev:.3g}")


# ------------------------------------------------------------------------------------------------ kernel: the inverse CDF
def test_inverse_cdf_pinned_on_identical_rows():
    R, V = 64, 8
    row = torch.log(torch.tensor([0.07, 0.21, 0.0, 0.13, 0.29, 0.02, 0.17, 0.11]))         # token 2: -inf, no interval
    x = row.repeat(R, 1)
    u = (torch.arange(R, dtype=torch.float32) + 0.5) / R
    idx, lo, hi = SR.ref_cdf(row)
    bounds = np.concatenate([lo, hi[-1:]])
    assert np.abs(u.double().numpy()[:, None] - bounds[None]).min() > SR.DELTA             # no u near a boundary: the counts are exact
    want = np.zeros(V, np.int64)
    for i, a, b in zip(idx, lo, hi):
        want[i] = int(((u.double().numpy() >= a) & (u.double().numpy() < b)).sum())
    assert want[2] == 0 and want.sum() == R
    # u as [steps, R] read at row min(col, steps - 1): row 1 of 2 here; row 0 would give the last token everywhere
    u3 = torch.stack([torch.full((R,), 0.999), u])
    got = run_select(x, u=u3, do_sample=True, col=1)
    assert np.bincount(got["tok"].numpy(), minlength=V).tolist() == want.tolist()
    assert torch.equal(got["tok"], torch.tensor([int(idx[np.searchsorted(hi, float(v), side="right")]) for v in u.double()]))
    assert torch.equal(run_select(x, u=u3, do_sample=True, col=2)["tok"], got["tok"])      # col past the steps: the last row again
    assert (run_select(x, u=u3, do_sample=True, col=0)["tok"] == 7).all()


@pytest.mark.parametrize("V", [97, 32064, 128256])
def test_sampled_token_lies_in_the_accepted_set(V):
    R = 16 if V < 100000 else 4
    x, _ = _draw(R, V, 3.0, 900 + V, special=False)
    u = torch.rand(R, generator=torch.Generator().manual_seed(V))
    for kw in (dict(top_k=50), dict(top_p=0.9)):
        ref = SR.ref_scores(x, None, 1.0, kw.get("top_k", 0), kw.get("top_p", 1.0), 1.0)
        acc = [SR.accepted(ref["scores"][r], float(u[r])) for r in range(R)]
        assert all(1 <= len(a) <= 2 for a in acc), ("the draw puts u near too many boundaries", V, kw, [len(a) for a in acc])
        got = run_select(x, u=u, do_sample=True, **kw)
        again = run_select(x, u=u, do_sample=True, **kw)
        assert torch.equal(got["tok"], again["tok"]) and torch.equal(_bits(got["scores"]), _bits(again["scores"]))      # run to run
        for r in range(R):
            assert int(got["tok"][r]) in acc[r].tolist(), (V, kw, r, int(got["tok"][r]), acc[r].tolist(), float(u[r]))
        assert ((got["scores"] > NEG_INF).gather(1, got["tok"][:, None])).all()             # a kept token
        # top_k = 1 and top_p -> 0 leave one token: greedy for every u
        greedy = ref["s"].argmax(-1)
        assert torch.equal(run_select(x, u=u, do_sample=True, top_k=1, scores=False)["tok"], greedy)
        assert torch.equal(run_select(x, u=u, do_sample=True, top_p=1e-9, scores=False)["tok"], greedy)


def test_two_runs_are_bit_identical_at_width():
    R, V = 64, 32064
    x, seen = _draw(R, V, 3.0, 4242)
    u = torch.rand(R, generator=torch.Generator().manual_seed(9))
    kw = dict(seen=seen, u=u, do_sample=True, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.1)
    a, b = run_select(x, **kw), run_select(x, **kw)
    assert torch.equal(a["tok"], b["tok"]) and torch.equal(_bits(a["scores"]), _bits(b["scores"])) and torch.equal(a["seen"], b["seen"])
    ref = SR.ref_scores(x, seen, 0.8, 50, 0.9, 1.1)
    assert _same_scores(a["scores"], ref["scores"], ~ref["band"])


def test_nan_row_and_single_finite_row_leave_the_others_alone():
    V = 1000
    x, _ = _draw(6, V, 3.0, 77, special=False)
    clean = x.clone()
    x[1] = float("nan")
    x[3] = NEG_INF
    x[3, 613] = -2.5
    x[4, ::2] = float("nan")                                     # NaNs among finite values
    u = torch.tensor([0.3, 0.6, 0.9, 0.99, 0.5, 0.7])
    for kw in (dict(), dict(do_sample=True, u=u), dict(do_sample=True, u=u, top_k=50, top_p=0.9, temperature=0.8)):
        got = run_select(x, **kw)
        want = run_select(clean, **kw)
        assert ((got["tok"] >= 0) & (got["tok"] < V)).all(), got["tok"].tolist()
        assert int(got["tok"][3]) == 613
        for r in (0, 2, 5):
            assert int(got["tok"][r]) == int(want["tok"][r]) and torch.equal(_bits(got["scores"][r]), _bits(want["scores"][r])), (kw, r)


# ------------------------------------------------------------------------------------------------ engine
def _engine_case(arch):
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.engine import Engine
    ocfg, W, batch, g = cases.tiny_llama_case(arch)
    eng = Engine(VisperConfig(**vars(ocfg)))
    eng.load_weights(W)
    return eng, batch


def _ragged():
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, 1000, (n,), generator=g) for n in (7, 19, 12)]
    T = max(len(p) for p in prompts)
    ids, am = torch.zeros(3, T, dtype=torch.long), torch.zeros(3, T, dtype=torch.long)
    for b, p in enumerate(prompts):                              # left padding
        ids[b, T - len(p):] = p
        am[b, T - len(p):] = 1
    return ids, am


def _greedy_parity(eng, ids, am, images, N, **kw):
    """device_sampling greedy == the plain call, free-running and with EOS ids from the plain run's own output, eager / captured, any
    sync_every"""
    from visper_lm_amd import decode
    gen = lambda **k: decode.generate(eng, ids, am, images, None, max_new_tokens=N, **kw, **k)
    plain = gen()
    assert torch.equal(gen(device_sampling=True), plain)
    B = ids.shape[0]
    eos = sorted({int(plain[b, min(2 + 2 * b, N - 1)]) for b in range(B)})             # rows finish at different steps
    want = gen(eos_token_id=eos, pad_token_id=-7)
    assert want.shape[1] <= N
    for k in (dict(use_graph=False), dict(use_graph=True), dict(use_graph=False, sync_every=4), dict(use_graph=True, sync_every=4)):
        got = gen(eos_token_id=eos, pad_token_id=-7, device_sampling=True, **k)
        assert got.dtype == torch.long and torch.equal(got, want), (k, got.tolist(), want.tolist())
    assert torch.equal(gen(), plain)                             # no side effect on the plain path of the same engine
    return plain


@pytest.mark.parametrize("arch", ["llama", "phi3"])
def test_engine_greedy_parity_tiny(arch):
    _ops()
    eng, batch = _engine_case(arch)
    _greedy_parity(eng, batch["input_ids"][:1], None, batch["images"][:1].cuda(), 12)
    ids, am = _ragged()
    _greedy_parity(eng, ids, am, None, 10)


def test_engine_greedy_parity_mxfp4_weights_fp8_cache():
    _ops()
    eng, batch = _engine_case("llama")
    eng.quantize_decoder(fmt="mxfp4")
    ids, am = _ragged()
    _greedy_parity(eng, ids, am, None, 10, kv_cache_dtype="fp8_e4m3")


def test_engine_greedy_with_penalty_follows_hf_processor():
    _ops()
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from visper_lm_amd import decode
    eng, batch = _engine_case("llama")
    ids, am = _ragged()
    N = 12
    toks, kept, sess = decode.generate(eng, ids, am, None, None, max_new_tokens=N, repetition_penalty=1.3, return_logits=True)
    plain = decode.generate(eng, ids, am, None, None, max_new_tokens=N)
    toks = toks.cpu()
    proc = RepetitionPenaltyLogitsProcessor(1.3)
    for i in range(N):                                           # exact: the processor on that step's raw logits and the row's own history
        want = torch.argmax(proc(toks[:, :i], kept[i].cpu().clone()), -1)
        assert torch.equal(toks[:, i], want), (i, toks[:, i].tolist(), want.tolist())
    assert torch.equal(SR.unpack_bits(sess.seen, sess.seen.shape[1] * 32).sum(-1), torch.tensor([len(set(r.tolist())) for r in toks]))
    print("penalty changed", int((toks != plain.cpu()).sum()), "of", toks.numel(), "tokens")
    captured = decode.generate(eng, ids, am, None, None, max_new_tokens=N, repetition_penalty=1.3, use_graph=True)
    assert torch.equal(captured.cpu(), toks)


def _sampled_in_accepted_set(eng, ids, am, N, rows=None, **extra):
    from visper_lm_amd import decode
    kw = dict(max_new_tokens=N, do_sample=True, top_k=50, top_p=0.9, temperature=0.8, repetition_penalty=1.1, **extra)
    toks, kept, sess = decode.generate(eng, ids, am, None, None, return_logits=True, generator=torch.Generator().manual_seed(21), **kw)
    toks, U = toks.cpu(), sess.uniforms.cpu()
    assert tuple(U.shape) == (N, ids.shape[0]) and float(U.min()) >= 0 and float(U.max()) < 1
    V = kept[0].shape[1]
    sizes = []
    for i in range(N):
        ref = SR.ref_scores(kept[i].cpu(), SR.seen_mask(toks[:, :i], V), 0.8, 50, 0.9, 1.1)
        for b in range(ids.shape[0]):
            # a band token may be kept or not: both CDFs are legal
            cands = set(SR.accepted(ref["scores"][b], float(U[i, b])).tolist())
            for v in torch.nonzero(ref["band"][b]).flatten().tolist():
                alt = ref["scores"][b].clone()
                alt[v] = NEG_INF if bool(ref["keep"][b, v]) else ref["s"][b, v]
                cands |= set(SR.accepted(alt, float(U[i, b])).tolist())
            sizes.append(len(cands))
            assert int(toks[b, i]) in cands, (i, b, int(toks[b, i]), sorted(cands), float(U[i, b]))
    assert max(sizes) <= 3 and sum(s == 1 for s in sizes) >= len(sizes) // 2, sizes
    again = decode.generate(eng, ids, am, None, None, generator=torch.Generator().manual_seed(21), **kw)
    assert torch.equal(again.cpu(), toks)                        # a seeded call reproduces
    return toks


def test_engine_sampling_accepted_set_seeded_and_top_k_1():
    _ops()
    from visper_lm_amd import decode
    eng, batch = _engine_case("llama")
    ids, am = _ragged()
    N = 10
    plain = decode.generate(eng, ids, am, None, None, max_new_tokens=N)
    toks = _sampled_in_accepted_set(eng, ids, am, N)
    assert torch.equal(_sampled_in_accepted_set(eng, ids, am, N, use_graph=True, sync_every=4), toks)
    one = decode.generate(eng, ids, am, None, None, max_new_tokens=N, do_sample=True, top_k=1, generator=torch.Generator().manual_seed(3))
    assert torch.equal(one, plain)                               # top_k = 1 sampled is greedy
    # through the model mirror's keyword path the arguments reach the selector instead of being dropped: see test_model_generate below
    assert torch.equal(decode.generate(eng, ids, am, None, None, max_new_tokens=N), plain)


def test_model_generate_passes_the_new_arguments():
    _ops()
    from oracle import cases
    from visper_lm_amd.model import OlaLlavaLlamaConfig, OlaLlavaLlamaForCausalLM
    ocfg, W, batch, g = cases.tiny_llama_case()
    model = OlaLlavaLlamaForCausalLM(OlaLlavaLlamaConfig(**vars(ocfg)), init="empty")
    sd = {k.replace("model.vision_tower.vision_tower.", "model.vision_tower.vision_tower.vision_model.")
          if k.startswith("model.vision_tower.vision_tower.") else k: v for k, v in W.items()}
    model.load_state_dict(sd, strict=True)
    model.reload_frozen()
    ids, img = batch["input_ids"][:1], batch["images"][:1].cuda()
    plain = model.generate(ids, images=img, max_new_tokens=8)
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=8, device_sampling=True, sync_every=3), plain)
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=8, do_sample=True, top_k=1), plain)
    pen = model.generate(ids, images=img, max_new_tokens=8, repetition_penalty=50.0)
    assert len(set(pen[0].tolist())) == 8                        # a penalty this large never repeats a token (random-init logits are flat)
    assert torch.equal(model.generate(ids, images=img, max_new_tokens=8), plain)


def test_engine_full_width_llama():
    _ops()
    from visper_lm_amd import decode
    from visper_lm_amd.config import llama3_8b
    from visper_lm_amd.engine import Engine
    eng = Engine(llama3_8b(num_hidden_layers=2, aux_mode="", num_task_tokens=0, vit_layers=1))
    eng.init_random(seed=1)
    ids = torch.randint(0, 120000, (1, 300), generator=torch.Generator().manual_seed(3))
    N = 6
    plain = decode.generate(eng, ids, None, None, None, max_new_tokens=N)
    assert torch.equal(decode.generate(eng, ids, None, None, None, max_new_tokens=N, device_sampling=True, use_graph=True), plain)
    _sampled_in_accepted_set(eng, ids, None, N)
