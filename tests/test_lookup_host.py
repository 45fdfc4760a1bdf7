"""Prompt-lookup decoding without a GPU: the drafter against a brute-force restatement, hand cases and (where this transformers version has
it) HF's PromptLookupCandidateGenerator; the argument checks of the five new entry points (the library loads without a device); and what
generate() refuses before any GPU work."""
import ctypes

import numpy as np
import pytest
import torch


# ------------------------------------------------------------------------------------------------ the drafter
def _brute(history, n, max_ngram):
    """The rule restated position by position: g from min(max_ngram, len - 1) down to 1; the earliest i < len - g with history[i : i + g] equal
    to the last g tokens; up to n tokens from i + g, cut at the end of the history and before the first negative id."""
    h = [int(t) for t in history]
    L = len(h)
    for g in range(min(max_ngram, L - 1), 0, -1):
        for i in range(0, L - g):
            if h[i:i + g] == h[L - g:]:
                out = []
                for t in h[i + g:i + g + n]:
                    if t < 0:
                        break
                    out.append(t)
                return out
    return []


def test_lookup_draft_matches_brute_force_on_random_histories():
    from visper_lm_amd.decode import lookup_draft
    rng = np.random.default_rng(0)
    hits = 0
    for trial in range(400):
        L = int(rng.integers(1, 40))
        h = rng.integers(0, 5, L)                                        # 5 symbols: matches are common
        if trial % 4 == 0 and L > 3:
            h[int(rng.integers(0, L - 1))] = -200                        # an <image> placeholder somewhere in the prompt
        n, g = int(rng.integers(1, 8)), int(rng.integers(1, 5))
        got = lookup_draft(h, n, g)
        assert got == _brute(h, n, g), (h.tolist(), n, g)
        assert len(got) <= n and all(t >= 0 for t in got)
        hits += bool(got)
    assert hits > 200                                                    # the comparison was not of empty lists
    assert lookup_draft(torch.tensor([1, 2, 3, 1, 2]), 2, 2) == [3, 1]   # any integer sequence is a history
    assert lookup_draft([1, 2, 3, 1, 2], 0, 2) == []


def test_lookup_draft_hand_cases():
    from visper_lm_amd.decode import lookup_draft
    # earliest of two matches of the bigram (7, 8): what followed the first one
    assert lookup_draft([7, 8, 1, 2, 7, 8, 3, 4, 7, 8], 2, 2) == [1, 2]
    # the longer n-gram wins over a shorter, earlier one: (5, 6) occurs at 3, the unigram 6 already at 0
    assert lookup_draft([6, 9, 9, 5, 6, 4, 4, 5, 6], 2, 2) == [4, 4]
    assert lookup_draft([6, 9, 9, 5, 6, 4, 4, 5, 6], 2, 1) == [9, 9]
    # the continuation is cut at the end of the history
    assert lookup_draft([1, 2, 3, 1, 2], 5, 2) == [3, 1, 2]
    # ... and before a -200
    assert lookup_draft([1, 2, 3, -200, 9, 1, 2], 4, 2) == [3]
    assert lookup_draft([1, 2, -200, 9, 1, 2], 4, 2) == []
    # the only match is the suffix itself
    assert lookup_draft([1, 2, 3, 4], 3, 2) == []
    assert lookup_draft([4, 4], 3, 2) == [4]                              # (the unigram at 0 is an earlier window: its continuation is the last 4)
    # a history of length 1 has no earlier window
    assert lookup_draft([5], 3, 2) == []
    assert lookup_draft([], 3, 2) == []


def test_lookup_draft_matches_hf_prompt_lookup_generator():
    """HF's own drafter, where this transformers version has it and it runs stand-alone; the brute force above is the pin that always runs."""
    from visper_lm_amd.decode import lookup_draft
    try:
        from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
        gen = PromptLookupCandidateGenerator(num_output_tokens=3, max_matching_ngram_size=2, max_length=10 ** 6)
        gen.get_candidates(torch.tensor([[1, 2, 3, 1, 2]]))
    except Exception as e:                                               # absent, or another constructor / call signature
        pytest.skip(f"PromptLookupCandidateGenerator does not run on this transformers version: {type(e).__name__}")
    rng = np.random.default_rng(1)
    for trial in range(100):
        L = int(rng.integers(2, 40))
        h = rng.integers(0, 5, L)
        n, g = int(rng.integers(1, 8)), int(rng.integers(1, 5))
        gen = PromptLookupCandidateGenerator(num_output_tokens=n, max_matching_ngram_size=g, max_length=10 ** 6)
        cand, _ = gen.get_candidates(torch.from_numpy(h)[None])
        assert cand[0, L:].tolist() == lookup_draft(h, n, g), (h.tolist(), n, g)


# ------------------------------------------------------------------------------------------------ entry points
def test_lookup_entry_points_reject_bad_arguments():
    from visper_lm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vp_last_error_string()
    p = ctypes.c_void_p(16)                                               # never dereferenced: every call below fails its checks first
    f = ctypes.c_float
    # attention, bf16 and byte caches: the siblings' codes (test_generate_host / test_decode_edges_host), with and without a row map
    for cr in (p, None):
        a = lambda B, Hq, Hkv, D, Smax, ns, ws, q=p: (B, Hq, Hkv, D, Smax, q, Hq * D, p, Smax * Hkv * D, Hkv * D, p, Smax * Hkv * D, Hkv * D,
                                                       p, Hq * D, p, cr, 0, f(0.1), ns, ws, None)
        assert lib.vp_decode_attn_rows(*a(1, 32, 8, 80, 64, 1, p)) == -2 and b"vp_decode_attn_rows" in err() and b"head_dim 80" in err()
        assert lib.vp_decode_attn_rows(*a(1, 24, 8, 128, 64, 1, p)) == -2
        assert lib.vp_decode_attn_rows(*a(1, 32, 8, 128, 8192, 4, p)) == -2 and b"nsplit" in err()
        assert lib.vp_decode_attn_rows(*a(1, 32, 8, 128, 64, 0, p)) == -2 and b"nsplit" in err()
        assert lib.vp_decode_attn_rows(*a(1, 32, 8, 128, 64, 1, None)) == -1 and b"workspace" in err()
        assert lib.vp_decode_attn_rows(*a(1, 32, 8, 128, 64, 1, p, q=None)) == -1 and b"null" in err()
        a8 = lambda B, Hq, Hkv, D, Smax, ns, ws, q=p: (B, Hq, Hkv, D, Smax, q, Hq * D, p, Smax * Hkv * D, Hkv * D, p, Smax * Hkv, Hkv,
                                                        p, Smax * Hkv * D, Hkv * D, p, Smax * Hkv, Hkv, p, Hq * D, p, cr, 0, f(0.1), ns, ws, None)
        assert lib.vp_decode_attn_kv8_rows(*a8(1, 32, 8, 80, 64, 1, p)) == -2 and b"vp_decode_attn_kv8_rows" in err() and b"head_dim 80" in err()
        assert lib.vp_decode_attn_kv8_rows(*a8(1, 32, 8, 128, 8192, 4, p)) == -2 and b"nsplit" in err()
        assert lib.vp_decode_attn_kv8_rows(*a8(1, 32, 8, 128, 64, 1, None)) == -1 and b"workspace" in err()
        assert lib.vp_decode_attn_kv8_rows(*a8(1, 32, 8, 128, 64, 1, p, q=None)) == -1
        # rope + append: head_dim not a multiple of 16, null position array
        assert lib.vp_decode_rope_append_rows(1, 4, 2, 40, p, 256, p, 160, p, 0, 80, p, 0, 80, p, p, p, cr, 8, None) == -2
        assert b"vp_decode_rope_append_rows" in err() and b"head_dim 40" in err()
        assert lib.vp_decode_rope_append_rows(1, 4, 2, 32, p, 256, p, 128, p, 0, 64, p, 0, 64, p, p, None, cr, 8, None) == -1
        kv8 = lambda D, pos, kb=p: (1, 4, 2, D, p, 256, p, 128, kb, 0, 64, kb, 0, 64, kb, 0, 2, kb, 0, 2, None, 0, 0, None, 0, 0, p, p, pos, cr,
                                    8, None)
        assert lib.vp_decode_rope_append_kv8_rows(*kv8(40, p)) == -2 and b"vp_decode_rope_append_kv8_rows" in err() and b"head_dim 40" in err()
        assert lib.vp_decode_rope_append_kv8_rows(*kv8(32, None)) == -1
        assert lib.vp_decode_rope_append_kv8_rows(*kv8(32, p, kb=None)) == -1 and b"neither" in err()
    # the acceptance rule: null operands, n < 0, no sequences
    assert lib.vp_decode_accept(1, 3, None, p, p, p, p, p, None) == -1 and b"vp_decode_accept" in err() and b"null" in err()
    assert lib.vp_decode_accept(1, 3, p, p, p, p, p, None, None) == -1
    assert lib.vp_decode_accept(1, -1, p, p, p, p, p, p, None) == -1 and b"n -1" in err()
    assert lib.vp_decode_accept(0, 3, p, p, p, p, p, p, None) == -1


# ------------------------------------------------------------------------------------------------ what generate() refuses
def _cpu_model(cls_name="OlaLlavaLlamaForCausalLM"):
    from oracle import cases
    from visper_lm_amd import model as M
    ocfg, W, batch, g = cases.tiny_llama_case()
    cfg_cls = {"OlaLlavaLlamaForCausalLM": M.OlaLlavaLlamaConfig, "LlavaLlamaForCausalLM": M.LlavaConfig}[cls_name]
    return getattr(M, cls_name)(cfg_cls(**vars(ocfg)), device="cpu", init="empty"), batch


@pytest.mark.parametrize("cls_name", ["OlaLlavaLlamaForCausalLM", "LlavaLlamaForCausalLM"])
def test_generate_refuses_lookup_it_cannot_run(cls_name):
    model, batch = _cpu_model(cls_name)
    ids = batch["input_ids"][:1]
    with pytest.raises(ValueError, match="do_sample"):
        model.generate(ids, prompt_lookup_num_tokens=3, do_sample=True)
    ids4 = ids.repeat(4, 1)
    with pytest.raises(ValueError, match=r"largest prompt_lookup_num_tokens for B = 4 is 3"):
        model.generate(ids4, prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        model.generate(ids, prompt_lookup_num_tokens=3, max_matching_ngram_size=0)
    with pytest.raises(NotImplementedError, match="num_beams"):            # the older refusals come first and stay
        model.generate(ids, num_beams=4, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(ids, num_beams=4)


def test_check_lookup_limits():
    from visper_lm_amd.decode import check_lookup
    assert check_lookup(1, None) == 0 and check_lookup(4, 0) == 0 and check_lookup(3, 0, do_sample=True) == 0
    assert check_lookup(1, 15) == 15 and check_lookup(2, 7) == 7 and check_lookup(8, 1) == 1 and check_lookup(3, 4) == 4
    for B, n in ((1, 16), (2, 8), (3, 5), (8, 2), (9, 1), (17, 1)):
        with pytest.raises(ValueError, match=f"for B = {B} is {max(16 // B - 1, 0)}"):
            check_lookup(B, n)
    with pytest.raises(ValueError, match=">= 0"):
        check_lookup(1, -1)
