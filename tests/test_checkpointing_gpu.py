"""Gradient checkpointing on the GPU.  The yardstick is the same step with the switch off, on the same weights and batch; the recompute
launches the forward's own kernels with the forward's own arguments, so every comparison is torch.equal (no tolerance)."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
MODES = ("full", "keep_attn")
KEPT_BYTES = 94344 - 8196        # per token and layer: what the step saves today minus the layer input + its 1/rms that stay


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _to_gpu(batch):
    return {k: (v.cuda() if (k == "images" or k.endswith("_target") or k.endswith("_mask")) else v) for k, v in batch.items()}


def _step(eng, batch, mode, lr=1e-3, optimizer=True, info=None):
    """One train step under `mode` (+ one optimizer step): everything the comparisons read, cloned.  info: dict that receives the
    step's peak allocation above what was allocated before it, S and eng.last_fold."""
    eng.gradient_checkpointing = mode
    gb = _to_gpu(batch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = eng.train_step(gb)
    torch.cuda.synchronize()
    if info is not None:
        info.update(peak=torch.cuda.max_memory_allocated() - base, S=out["plan"]["S"], fold=eng.last_fold)
    res = {k: out[k].detach().clone() for k in ("loss", "text_loss", "seg_loss", "depth_loss", "gen_loss", "d_inputs_embeds") if k in out}
    for key, v in out["layer_losses"].items():
        res[f"layer_loss/{key}"] = v.detach().clone()
    res["grad"] = eng.ps.grad.detach().clone()
    if optimizer:
        eng.optimizer_step(lr=lr)
        torch.cuda.synchronize()
        res["master"] = eng.ps.master.detach().clone()
    return res


def _assert_same(got, want, tag):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k)
        assert torch.equal(got[k], want[k]), f"{tag}: {k} differs (max abs {float((got[k].float() - want[k].float()).abs().max()):.3e})"
    assert float(want["grad"].abs().max()) > 0 and bool(torch.isfinite(want["loss"]).all()), tag


def _tiny(case):
    from oracle import cases
    from visper_lm_amd.config import VisperConfig
    if case == "ift":
        ocfg, W, batch, _ = cases.tiny_ift_case()
        return VisperConfig(**vars(ocfg), train_llm=True), W, batch
    ocfg, W, batch, _ = cases.tiny_llama_case(case)
    return VisperConfig(**vars(ocfg)), W, batch


@pytest.mark.parametrize("padded", [False, True], ids=["full_batch", "right_padded"])
@pytest.mark.parametrize("case", ["llama", "phi3", "ift"])
def test_tiny_step_is_bit_identical_with_checkpointing(case, padded):
    """oracle/cases.py tiny Llama (GQA), Phi-3 (sliding window) and IFT (cfg.train_llm: weight gradients, per-layer buckets) steps, full and
    right-padded: losses, d_inputs_embeds, the whole flat gradient buffer and the fp32 master after one optimizer step."""
    _need_gpu()
    from visper_lm_amd.engine import Engine, _Ckpt
    cfg, W, batch = _tiny(case)
    batch = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
    if padded:
        batch["attention_mask"][1, -17:] = False          # sample 1 is 17 tokens shorter: its tail rows are padding (kv_len masks the keys)
    runs = {}
    for mode in (False,) + MODES:
        eng = Engine(cfg)
        eng.load_weights(W)
        seen = []
        inner = eng._decoder_bwd
        eng._decoder_bwd = lambda d_hidden, dec, *a, _s=seen, _f=inner: (_s.extend(type(s) for s in dec["saved"]), _f(d_hidden, dec, *a))[1]
        runs[mode] = _step(eng, batch, mode)
        assert len(seen) == cfg.num_hidden_layers and all((t is _Ckpt) == bool(mode) for t in seen), (mode, seen)
        del eng
    for mode in MODES:
        _assert_same(runs[mode], runs[False], f"tiny {case} {'padded' if padded else 'full'} {mode}")


def test_toggling_between_steps_on_one_engine():
    """off, full, off, keep_attn, True on ONE engine (Engine.gradient_checkpointing may change between steps): bit-identical gradient buffers."""
    _need_gpu()
    from visper_lm_amd.engine import Engine
    cfg, W, batch = _tiny("llama")
    eng = Engine(cfg)
    eng.load_weights(W)
    grads = [_step(eng, batch, mode, optimizer=False)["grad"] for mode in (False, "full", False, "keep_attn", True)]
    for i, g in enumerate(grads[1:], 1):
        assert torch.equal(g, grads[0]), i
    eng.gradient_checkpointing = "everything"
    with pytest.raises(ValueError, match="gradient_checkpointing"):
        eng.train_step(_to_gpu(batch))


def _fullwidth_case():
    from test_fullwidth_gpu import _weights, _batch
    from visper_lm_amd.config import llama3_8b
    cfg = llama3_8b(num_hidden_layers=4, vit_layers=4)
    cfg.image_seg = dict(cfg.image_seg, seg_layer_indices="1")
    cfg.image_depth = dict(cfg.image_depth, depth_layer_indices="2")
    cfg.image_gen = dict(cfg.image_gen, img_layer_indices="4")
    return cfg, _weights(cfg), _batch(cfg, 2, 169)         # B = 2, S = 768: 1536 tokens, the shape test_fold_norm_step_matches_unfolded_step folds at


def _fullwidth_runs(cfg, W, batch, fold):
    from visper_lm_amd.engine import Engine
    runs, peaks = {}, {}
    for mode in (False,) + MODES:
        eng = Engine(cfg)
        eng.load_weights(W)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        info = {}
        runs[mode] = _step(eng, batch, mode, info=info)
        assert info["S"] == 768 and info["fold"] == fold, info
        peaks[mode] = info["peak"]
        del eng
        torch.cuda.empty_cache()
    return runs, peaks


def test_fullwidth_folded_step_is_bit_identical_and_saves_the_derived_memory():
    """Llama-3-8B width, 4 layers, M = 1536 tokens: the folded-norm branch with its fused epilogues (eng.last_fold).  Bit-identity as above, and
    the step's peak allocation falls by at least half of what the checkpoints no longer keep: (L - 1) x M x 86 148 B (94 344 B saved per
    token and layer without the switch, 8 196 B — the layer input and its 1/rms — with it; one layer's recomputed set is alive in the
    backward).  0.5 is a condition, not a measurement: the feature cannot be silently off, while the peak may sit elsewhere in the step."""
    _need_gpu()
    cfg, W, batch = _fullwidth_case()
    t0 = time.time()
    runs, peaks = _fullwidth_runs(cfg, W, batch, fold=True)
    for mode in MODES:
        _assert_same(runs[mode], runs[False], f"full-width folded {mode}")
    L, M = cfg.num_hidden_layers, 1536
    derived = (L - 1) * M * KEPT_BYTES
    for mode in MODES:
        saved = peaks[False] - peaks[mode]
        print(f"[checkpointing] full-width folded L={L} M={M} {mode}: step peak {peaks[False] / 1e6:.1f} MB -> {peaks[mode] / 1e6:.1f} MB, saved "
              f"{saved / 1e6:.1f} MB = {saved / derived:.3f} of the derived {derived / 1e6:.1f} MB")
    print(f"[checkpointing] full-width folded test: {time.time() - t0:.1f} s")
    assert peaks[False] - peaks["full"] >= 0.5 * derived, (peaks, derived)


def test_fullwidth_plain_branch_step_is_bit_identical(monkeypatch):
    """The same case with VP_FOLD_NORM=0: the plain branch (RMSNorm kernels, HF's rounding points) at full width."""
    _need_gpu()
    monkeypatch.setenv("VP_FOLD_NORM", "0")
    cfg, W, batch = _fullwidth_case()
    runs, _ = _fullwidth_runs(cfg, W, batch, fold=False)
    for mode in MODES:
        _assert_same(runs[mode], runs[False], f"full-width plain {mode}")


def test_generate_and_labelless_forward_do_not_change():
    """Nothing is saved without gradients: generate() and a label-less forward return the same bits with the switch on."""
    _need_gpu()
    from test_model_api_gpu import _mirror_from_tiny
    model, kw = _mirror_from_tiny()
    ids, img = kw["input_ids"][:1], kw["images"][:1]
    nolab = {k: v for k, v in kw.items() if k in ("input_ids", "attention_mask", "images")}
    with torch.no_grad():
        toks0 = model.generate(ids, images=img, max_new_tokens=8)
        out0 = model(**nolab)
    for mode in MODES:
        model.config.gradient_checkpointing = mode
        model.gradient_checkpointing_enable()
        assert model._get_engine().gradient_checkpointing == mode and model.is_gradient_checkpointing
        with torch.no_grad():
            toks = model.generate(ids, images=img, max_new_tokens=8)
            out = model(**nolab)
        assert torch.equal(toks, toks0) and out.loss is None
        assert torch.equal(out.logits, out0.logits)
        assert len(out.hidden_states) == len(out0.hidden_states) and all(torch.equal(a, b) for a, b in zip(out.hidden_states, out0.hidden_states))
    model.gradient_checkpointing_disable()
    assert model._get_engine().gradient_checkpointing is False and not model.is_gradient_checkpointing


def test_model_api_backward_is_bit_identical_for_pt_and_ift_mirrors():
    """model(**batch).loss.backward() through the drop-in classes (autograd hand-over of the engine's gradients): the same .grad bits."""
    _need_gpu()
    from oracle import cases
    from test_model_api_gpu import _mirror_from_tiny
    from test_generate_gpu import _sd
    from visper_lm_amd.model import LlavaConfig, LlavaLlamaForCausalLM
    pt, kw = _mirror_from_tiny()
    ocfg, W, batch, _ = cases.tiny_ift_case()
    ift = LlavaLlamaForCausalLM(LlavaConfig(**vars(ocfg)), init="empty")
    ift.load_state_dict(_sd(W), strict=True)
    ift.reload_frozen()
    ikw = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"], images=batch["images"].cuda())
    for model, args in ((pt, kw), (ift, ikw)):
        def grads():
            model.zero_grad(set_to_none=True)
            out = model(**args)
            out.loss.backward()
            return out.loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        l0, g0 = grads()
        model.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})
        l1, g1 = grads()
        assert model._get_engine().gradient_checkpointing == "full"
        assert torch.equal(l0, l1) and sorted(g0) == sorted(g1) and len(g0) > 0
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n


def _trainer_run(gradient_checkpointing):
    import tempfile
    from oracle import cases
    from transformers import Trainer, TrainingArguments
    from test_model_api_gpu import _mirror_from_tiny, _teacher_hooks, _instances
    from visper_lm_amd import data
    _, _, batch, _ = cases.tiny_llama_case()
    model, kw = _mirror_from_tiny()
    _teacher_hooks(model, batch)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 8

        def __getitem__(self, i):
            return _instances(batch)[i % 2]
    with tempfile.TemporaryDirectory() as d:
        args = TrainingArguments(output_dir=d, per_device_train_batch_size=2, max_steps=3, learning_rate=1e-3, weight_decay=0.0,
                                 lr_scheduler_type="constant", logging_steps=1, save_strategy="no", report_to=[], bf16=True,
                                 remove_unused_columns=False, dataloader_num_workers=0, dataloader_pin_memory=False, seed=0,
                                 gradient_checkpointing=gradient_checkpointing)
        trainer = Trainer(model=model, args=args, train_dataset=DS(), data_collator=data.Collator(0, 4096, pin_memory=False))
        res = trainer.train()
    assert res.global_step == 3 and torch.isfinite(torch.tensor(res.training_loss))
    return model, {n: p.detach().clone() for n, p in model.named_parameters() if "mm_projector" in n}


def test_hf_trainer_with_gradient_checkpointing_flag():
    """transformers.Trainer with TrainingArguments(gradient_checkpointing=True), otherwise as test_hf_trainer_drives_the_pt_mirror: it runs
    (it calls model.gradient_checkpointing_enable(gradient_checkpointing_kwargs=...)), the model reports the switch on, and its projector
    after 3 steps is bit-equal to a run with the flag off and the same seed."""
    _need_gpu()
    model_on, proj_on = _trainer_run(True)
    assert model_on.is_gradient_checkpointing is True and model_on._get_engine().gradient_checkpointing == "full"
    model_off, proj_off = _trainer_run(False)
    assert model_off.is_gradient_checkpointing is False
    assert sorted(proj_on) == sorted(proj_off) and len(proj_on) == 4
    for n in proj_on:
        assert torch.equal(proj_on[n], proj_off[n]), n
