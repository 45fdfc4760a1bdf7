"""Device-side token selection without a GPU: the CPU restatement of vp_decode_select's contract (tests/select_ref.py) against HF's processor
chain, the entry point's argument checks (the library loads without a device), what generate() refuses and in which order, and generate()'s
host loop around a stubbed selector: untouched without the new arguments, the plain loop's result with them for every sync_every."""
import ctypes
import types

import numpy as np
import pytest
import torch

import select_ref as SR


# ------------------------------------------------------------------------------------------------ the reference against HF
def _hf_chain(logits, ids, temperature, top_k, top_p, penalty):
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    x = RepetitionPenaltyLogitsProcessor(penalty)(ids, logits.clone())
    x = TemperatureLogitsWarper(temperature)(ids, x)
    if top_k > 0:
        x = TopKLogitsWarper(top_k)(ids, x)
    if top_p < 1.0:
        x = TopPLogitsWarper(top_p, min_tokens_to_keep=1)(ids, x)
    return x


@pytest.mark.parametrize("V", [31, 97, 1000, 32064])
def test_reference_matches_hf_chain(V):
    g = torch.Generator().manual_seed(V)
    R = 3
    logits = torch.randn(R, V, generator=g) * 3
    logits[0, : min(V, 8)] = torch.tensor([0.0, -0.0, float("-inf"), -1.5, 2.0, 2.0, -3.0, 1.0])[: min(V, 8)]
    ids = torch.randint(0, V, (R, 12), generator=g)
    ids[0, : min(V, 8)] = torch.arange(min(V, 8))                # the penalised set holds zero, -inf, negative and positive logits
    seen = SR.seen_mask(ids, V)
    checked = banded = 0
    for temperature in (0.2, 0.7, 1.0, 1.3):
        for penalty in (1.0, 1.3, 0.8):
            for top_k in (0, 1, 2, 50, V, V + 5):
                for top_p in (1.0, 0.9, 0.5, 0.05, 1e-9):
                    ref = SR.ref_scores(logits, seen, temperature, top_k, top_p, penalty)
                    want = _hf_chain(logits, ids, temperature, top_k, top_p, penalty)
                    got = ref["scores"]
                    for r in range(R):                           # rows with an empty band: the whole row; others: everything outside it
                        ok = ~ref["band"][r]
                        banded += int((~ok).any())
                        assert torch.equal(torch.isinf(got[r]) & (got[r] < 0), torch.isinf(want[r]) & (want[r] < 0)) if ok.all() else \
                            torch.equal((got[r] == float("-inf"))[ok], (want[r] == float("-inf"))[ok]), (V, temperature, penalty, top_k, top_p, r)
                        fin = torch.isfinite(want[r]) & ok & torch.isfinite(got[r])
                        assert torch.equal(got[r][fin], want[r][fin]), (V, temperature, penalty, top_k, top_p, r)
                        assert bool(ref["keep"][r].any())
                        checked += 1
    assert banded <= checked // 20, (banded, checked)            # the band is the exception, not a way round the comparison


def test_reference_hand_cases():
    # top-k ties: the k-th value (2.0) is shared by a token inside and two outside the first k = 2 of a sort: all of them stay
    x = torch.tensor([[1.0, 2.0, 3.0, 2.0, 0.5, 2.0]])
    assert SR.ref_scores(x, top_k=2)["keep"].tolist() == [[False, True, True, True, False, True]]
    # top-p on p = (0.5, 0.25, 0.125, 0.125): tail masses 1, 0.5, 0.25 (the tie shares one), kept iff > 1 - top_p
    x = torch.log(torch.tensor([[0.5, 0.25, 0.125, 0.125]]))
    assert SR.ref_scores(x, top_p=0.6)["keep"].tolist() == [[True, True, False, False]]
    assert SR.ref_scores(x, top_p=0.8)["keep"].tolist() == [[True, True, True, True]]
    assert SR.ref_scores(x, top_p=1e-9)["keep"].tolist() == [[True, False, False, False]]
    # penalty: negative logits are multiplied, the others divided; then the temperature
    x = torch.tensor([[-2.0, 2.0, 0.0, 4.0]])
    s = SR.ref_scores(x, torch.tensor([[True, True, True, False]]), temperature=0.5, penalty=2.0)["s"]
    assert s.tolist() == [[-8.0, 2.0, 0.0, 8.0]]
    # the CDF: intervals in ascending index order, removed tokens have none
    idx, lo, hi = SR.ref_cdf(torch.log(torch.tensor([0.25, 0.0, 0.5, 0.25])))
    assert idx.tolist() == [0, 2, 3] and np.allclose(lo, [0, 0.25, 0.75]) and np.allclose(hi, [0.25, 0.75, 1.0])
    assert SR.accepted(torch.log(torch.tensor([0.25, 0.0, 0.5, 0.25])), 0.5).tolist() == [2]
    assert SR.accepted(torch.log(torch.tensor([0.25, 0.0, 0.5, 0.25])), 0.25 + SR.DELTA / 2).tolist() == [0, 2]
    m = torch.rand(5, 77) > 0.5
    assert torch.equal(SR.unpack_bits(SR.pack_bits(m), 77), m)


# ------------------------------------------------------------------------------------------------ the entry point's refusals
def test_decode_select_rejects_bad_arguments():
    from visper_lm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vp_last_error_string()
    p, f = ctypes.c_void_p(16), ctypes.c_float                   # never dereferenced: every call below fails its checks first

    def call(R=2, V=100, logits=p, ld=100, do_sample=0, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, seen=None, u=None, u_steps=1,
             eos=None, n_eos=0, pad=0, finished=p, col=p, tok=p, out=p, ld_out=4, n_out=4, scores=None, ld_scores=0):
        return lib.vp_decode_select(R, V, logits, ld, do_sample, f(temperature), top_k, f(top_p), f(penalty), seen, u, u_steps, eos, n_eos,
                                    pad, finished, col, tok, out, ld_out, n_out, scores, ld_scores, None)

    for name in ("logits", "finished", "col", "tok", "out"):
        assert call(**{name: None}) == -1 and b"vp_decode_select" in err() and b"null" in err(), name
    assert call(R=0) == -1 and b"R 0" in err()
    assert call(V=0) == -1 and call(V=(1 << 20) + 1) == -1 and b"2^20" in err()
    assert call(ld=99) == -1 and b"strides" in err()
    assert call(n_out=0) == -1 and call(ld_out=3) == -1 and call(scores=p, ld_scores=99) == -1
    assert call(temperature=0.0) == -1 and b"temperature" in err()
    assert call(temperature=-1.0) == -1 and call(temperature=float("nan")) == -1 and call(temperature=float("inf")) == -1
    assert call(top_k=-1) == -1 and b"top_k -1" in err()
    assert call(top_p=0.0) == -1 and b"top_p" in err()
    assert call(top_p=1.5) == -1 and call(top_p=float("nan")) == -1
    assert call(penalty=0.0) == -1 and b"repetition_penalty" in err()
    assert call(penalty=-2.0) == -1 and call(penalty=float("nan")) == -1
    assert call(penalty=1.3) == -1 and b"seen" in err()          # the penalty needs the bitmap
    assert call(do_sample=1) == -1 and b"uniforms" in err()      # sampling needs u
    assert call(do_sample=1, u=p, u_steps=0) == -1
    assert call(n_eos=-1) == -1 and call(n_eos=2) == -1 and b"eos" in err()
    assert call(n_eos=65, eos=p) == -1


# ------------------------------------------------------------------------------------------------ what generate() refuses
def _cpu_model(cls_name="OlaLlavaLlamaForCausalLM"):
    from oracle import cases
    from visper_lm_amd import model as M
    ocfg, W, batch, g = cases.tiny_llama_case()
    cfg_cls = {"OlaLlavaLlamaForCausalLM": M.OlaLlavaLlamaConfig, "LlavaLlamaForCausalLM": M.LlavaConfig}[cls_name]
    return getattr(M, cls_name)(cfg_cls(**vars(ocfg)), device="cpu", init="empty"), batch


@pytest.mark.parametrize("cls_name", ["OlaLlavaLlamaForCausalLM", "LlavaLlamaForCausalLM"])
def test_generate_refuses_selection_it_cannot_run(cls_name):
    model, batch = _cpu_model(cls_name)
    ids = batch["input_ids"][:1]
    with pytest.raises(ValueError, match="top_k = -1"):
        model.generate(ids, top_k=-1)
    with pytest.raises(ValueError, match="repetition_penalty = 0"):
        model.generate(ids, repetition_penalty=0)
    with pytest.raises(ValueError, match="repetition_penalty = -1.5"):
        model.generate(ids, repetition_penalty=-1.5)
    with pytest.raises(ValueError, match="sync_every = 0"):
        model.generate(ids, device_sampling=True, sync_every=0)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens with repetition_penalty"):
        model.generate(ids, prompt_lookup_num_tokens=3, repetition_penalty=1.1)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens with repetition_penalty / device_sampling"):
        model.generate(ids, prompt_lookup_num_tokens=3, device_sampling=True)
    # the older refusals come first and keep their messages
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(ids, num_beams=4, top_k=-1, repetition_penalty=0)
    with pytest.raises(NotImplementedError, match="output_scores"):
        model.generate(ids, output_scores=True, top_k=-1)
    with pytest.raises(ValueError, match="do_sample"):
        model.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, top_k=-1)
    with pytest.raises(ValueError, match="at most 64"):
        model.generate(ids.repeat(65, 1), top_k=-1)


def test_check_select():
    from visper_lm_amd.decode import check_select
    assert check_select() == (0, 1.0, 1, False)
    assert check_select(None, None, None, 1) == (0, 1.0, 1, False) and check_select(0, 1.0, False, 3) == (0, 1.0, 3, False)
    assert check_select(50) == (50, 1.0, 1, True) and check_select(repetition_penalty=1.1) == (0, 1.1, 1, True)
    assert check_select(device_sampling=True, sync_every=16) == (0, 1.0, 16, True)
    assert check_select(top_k=50, lookup=3) == (50, 1.0, 1, True)        # greedy lookup: top-k never removes the argmax; generate() keeps the lookup path


# ------------------------------------------------------------------------------------------------ generate()'s host loop on a stubbed session
V_FAKE = 23


class _Eng:
    dev = torch.device("cpu")
    cfg = None
    fz = {"lm_head": torch.zeros(V_FAKE, 4)}

    def quantized_weights(self):
        return None


def _fake_decode(monkeypatch, calls):
    """decode.DecodeSession whose model is a table (the next token's logits are a fixed function of the token fed) and ops stubs that restate
    the greedy half of vp_decode_select on the CPU; `calls` counts the selector's launches."""
    from visper_lm_amd import decode, ops
    table = torch.randn(V_FAKE, V_FAKE, generator=torch.Generator().manual_seed(5))

    class Sess(decode.DecodeSession):
        def prefill(self, input_ids, attention_mask=None, images=None, group_sizes=None, max_new_tokens=16):
            B = input_ids.shape[0]
            self.tok = torch.zeros(B, dtype=torch.int32)
            self.cache = types.SimpleNamespace(lens_host=np.zeros(B, np.int64))
            self.logits = table[input_ids[:, -1]].clone()
            return self.logits.clone()

        def _launch(self):
            self.logits.copy_(table[self.tok.long()])
            if self.sel is not None:
                self._select(self.logits)

    def select(logits, tok, out, col, finished, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seen=None,
               u=None, eos=None, pad=0, scores_out=None):
        calls.append(int(col))
        assert not do_sample and repetition_penalty == 1.0
        t = logits.argmax(-1).to(torch.int32)
        tok.copy_(t)
        o = torch.where(finished != 0, torch.full_like(t, pad), t)
        out[:, int(col)] = o
        if eos is not None:
            finished |= torch.isin(o, eos).to(torch.int32)

    monkeypatch.setattr(decode, "DecodeSession", Sess)
    monkeypatch.setattr(ops, "decode_select", select)
    monkeypatch.setattr(ops, "add_i32_", lambda x, delta=1: x.add_(delta))
    return decode


def test_generate_without_the_new_arguments_never_reaches_the_selector(monkeypatch):
    calls = []
    decode = _fake_decode(monkeypatch, calls)
    ids = torch.tensor([[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    plain = decode.generate(_Eng(), ids, max_new_tokens=12)
    assert plain.shape == (3, 12) and plain.dtype == torch.long and not calls
    decode.generate(_Eng(), ids, max_new_tokens=5, do_sample=True, temperature=0.8, top_p=0.9, generator=torch.Generator().manual_seed(0))
    decode.generate(_Eng(), ids, max_new_tokens=5, top_k=0, repetition_penalty=1.0, device_sampling=False)
    assert not calls
    dev = decode.generate(_Eng(), ids, max_new_tokens=12, device_sampling=True)
    assert calls == list(range(12)) and torch.equal(dev, plain) and dev.dtype == torch.long
    assert torch.equal(decode.generate(_Eng(), ids, max_new_tokens=12, top_k=50), plain)      # greedy: top_k changes nothing but the path
    assert len(calls) == 24


def test_device_loop_stops_and_truncates_like_the_plain_loop(monkeypatch):
    calls = []
    decode = _fake_decode(monkeypatch, calls)
    ids = torch.tensor([[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    free = decode.generate(_Eng(), ids, max_new_tokens=12)
    # EOS ids taken from the free run's own output, so the rows finish at different steps (and one case in which not every row finishes)
    for eos in ([int(free[0, 2])], [int(free[0, 2]), int(free[1, 5]), int(free[2, 3])], int(free[1, 1]), [V_FAKE + 5]):
        for pad in (None, 0):
            plain, klog, _ = decode.generate(_Eng(), ids, max_new_tokens=12, eos_token_id=eos, pad_token_id=pad, return_logits=True)
            for sync in (1, 4, 5, 16):
                del calls[:]
                dev, dlog, sess = decode.generate(_Eng(), ids, max_new_tokens=12, eos_token_id=eos, pad_token_id=pad, return_logits=True,
                                                  device_sampling=True, sync_every=sync)
                assert torch.equal(dev, plain), (eos, pad, sync)
                assert len(dlog) == len(klog) and all(torch.equal(a, b) for a, b in zip(dlog, klog))
                n = plain.shape[1]
                assert len(calls) == (n if sync == 1 else min(12, -(-n // sync) * sync)), (eos, sync, n, len(calls))
    assert decode.generate(_Eng(), ids, max_new_tokens=0, device_sampling=True).shape == (3, 0)


def test_streamer_sees_every_column_and_forces_sync(monkeypatch):
    calls = []
    decode = _fake_decode(monkeypatch, calls)

    class St:
        def __init__(self):
            self.got, self.ended = [], False

        def put(self, t):
            self.got.append(t.clone())

        def end(self):
            self.ended = True

    ids = torch.tensor([[1, 2, 3], [4, 5, 6]])
    free = decode.generate(_Eng(), ids, max_new_tokens=10)
    eos = [int(free[0, 1]), int(free[1, 3])]
    a, b = St(), St()
    plain = decode.generate(_Eng(), ids, max_new_tokens=10, eos_token_id=eos, streamer=a)
    dev = decode.generate(_Eng(), ids, max_new_tokens=10, eos_token_id=eos, streamer=b, device_sampling=True, sync_every=8)
    assert torch.equal(dev, plain) and b.ended and len(a.got) == len(b.got) == plain.shape[1] + 1
    assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a.got, b.got))
    assert len(calls) == plain.shape[1]
