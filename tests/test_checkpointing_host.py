"""Gradient checkpointing without a GPU: the surface transformers.Trainer and the reference's entry points call on a model
(ola_vlm_train.py:1049-1055, train.py:975-977, trainer.py `gradient_checkpointing_enable`) and the config flag's round trip."""
import pytest

MIRRORS = ["OlaLlavaLlamaForCausalLM", "LlavaLlamaForCausalLM"]


def _cpu_model(cls_name):
    from oracle import cases
    from visper_lm_amd import model as M
    ocfg, W, batch, g = cases.tiny_llama_case()
    cfg_cls = {"OlaLlavaLlamaForCausalLM": M.OlaLlavaLlamaConfig, "LlavaLlamaForCausalLM": M.LlavaConfig}[cls_name]
    return getattr(M, cls_name)(cfg_cls(**vars(ocfg)), device="cpu", init="empty")


@pytest.mark.parametrize("cls_name", MIRRORS)
def test_trainer_surface_exists(cls_name):
    model = _cpu_model(cls_name)
    for name in ("gradient_checkpointing_enable", "gradient_checkpointing_disable", "is_gradient_checkpointing",
                 "supports_gradient_checkpointing", "enable_input_require_grads", "get_input_embeddings"):
        assert hasattr(model, name), name
    assert model.supports_gradient_checkpointing is True
    assert model.is_gradient_checkpointing is False
    # both branches of ola_vlm_train.py:1049-1055
    assert model.enable_input_require_grads() is None
    emb = model.get_input_embeddings()
    assert emb is model.model.embed_tokens and tuple(emb.weight.shape) == (model.config.vocab_size, model.config.hidden_size)


@pytest.mark.parametrize("cls_name", MIRRORS)
def test_enable_disable_flip_the_flag(cls_name):
    model = _cpu_model(cls_name)
    model.gradient_checkpointing_enable()
    assert model.is_gradient_checkpointing is True and model.config.gradient_checkpointing == "full"
    model.gradient_checkpointing_disable()
    assert model.is_gradient_checkpointing is False and model.config.gradient_checkpointing is False
    model.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})      # what HF passes
    assert model.is_gradient_checkpointing is True and model.config.gradient_checkpointing == "full"
    model.gradient_checkpointing_disable()
    model.config.gradient_checkpointing = "keep_attn"                  # a mode the config already names is kept
    model.gradient_checkpointing_enable()
    assert model.config.gradient_checkpointing == "keep_attn" and model.is_gradient_checkpointing is True
    model.config.gradient_checkpointing = True                         # HF-style boolean: the default mode
    model.gradient_checkpointing_enable()
    assert model.config.gradient_checkpointing == "full"


def test_config_flag_round_trips_and_defaults_to_off():
    from visper_lm_amd.config import VisperConfig
    from visper_lm_amd.model import LlavaConfig, OlaLlavaLlamaConfig
    for cls in (VisperConfig, OlaLlavaLlamaConfig, LlavaConfig):
        assert cls().gradient_checkpointing is False
        on = cls(gradient_checkpointing="keep_attn")
        d = on.to_dict()
        assert d["gradient_checkpointing"] == "keep_attn"
        assert cls(**d).gradient_checkpointing == "keep_attn"
        d.pop("gradient_checkpointing")                                # a config dict written before the flag existed
        assert cls(**d).gradient_checkpointing is False


def test_save_and_load_pretrained_carry_the_flag(tmp_path):
    import json
    from visper_lm_amd.model import OlaLlavaLlamaForCausalLM
    model = _cpu_model("OlaLlavaLlamaForCausalLM")
    for p in model.parameters():
        p.data.zero_()
    model.gradient_checkpointing_enable()
    model.save_pretrained(str(tmp_path / "on"))
    assert json.load(open(tmp_path / "on" / "config.json"))["gradient_checkpointing"] == "full"
    assert OlaLlavaLlamaForCausalLM.from_pretrained(str(tmp_path / "on"), device="cpu").is_gradient_checkpointing is True
    # a directory saved before the flag existed loads with it off
    cfgd = json.load(open(tmp_path / "on" / "config.json"))
    cfgd.pop("gradient_checkpointing")
    json.dump(cfgd, open(tmp_path / "on" / "config.json", "w"))
    old = OlaLlavaLlamaForCausalLM.from_pretrained(str(tmp_path / "on"), device="cpu")
    assert old.is_gradient_checkpointing is False and old.config.gradient_checkpointing is False
