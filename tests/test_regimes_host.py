"""CPU proof that tests/test_kernels_regimes_gpu.py would notice a subtly wrong kernel.  For every operation of tests/regimes.py and every
regime group: the honest reference, evaluated in fp32 and rounded to bf16 at the documented points (what a correct kernel computes), passes
`group_err` within the computed bound; every mutant (the same reference with one plausible mistake) fails it in at least one group.  And,
once, the claim the regime tests rest on: the same mutants pass the comparisons of tests/test_kernels_gpu.py (`close()` with that test's
arguments on that test's own unit-Gaussian inputs), except the few listed in OLD_CATCHES."""
import math

import pytest
import torch

import regimes as R
from regimes import NS
from test_kernels_gpu import close, rnd

BF = torch.bfloat16


def _honest_passes_mutants_fail(op, inp, label, must_catch=None):
    res = R.evaluate(op, inp, R.simulate(op, inp))
    assert not R.failures(res), (label, {k: res[k] for k in R.failures(res)})
    caught = {}
    for mut in op.mutants:
        bad = R.failures(R.evaluate(op, inp, R.simulate(op, inp, mut)))
        caught[mut] = bad
    for mut in (op.mutants if must_catch is None else must_catch):
        assert caught[mut], f"{label}: mutant {mut} passes every group"
    return caught


@pytest.mark.parametrize("H", [64, 1024, 4096])
def test_rmsnorm_regimes(H):
    c = _honest_passes_mutants_fail(R.RMSNORM, R.rmsnorm_inputs(H), f"rmsnorm H={H}")
    assert ("y", "zero") in c["eps_dropped"] and ("y", "scale0.001") in c["eps_dropped"]            # NaN on the zero row, 1.00 instead of 0.30 rms
    assert ("y", "scale0.001") in c["eps_outside_sqrt"]


@pytest.mark.parametrize("H", [64, 1024, 4096])
def test_layernorm_regimes(H):
    c = _honest_passes_mutants_fail(R.LAYERNORM, R.layernorm_inputs(H), f"layernorm H={H}")
    assert any(g in ("mean100", "mean1000") for _, g in c["var_one_pass"])


def test_swiglu_regimes():
    c = _honest_passes_mutants_fail(R.SWIGLU, R.swiglu_inputs(), "swiglu")
    assert ("act", "+90") in c["sigmoid_exp_pos"] and ("dgate", "-90") in c["silu_grad_exp_neg"]


def test_act_regimes():
    _honest_passes_mutants_fail(R.ACT, R.act_inputs(R.ACT_GELU), "gelu")
    quick = NS(**{**vars(R.ACT), "mutants": ["sigmoid_exp_pos"]})
    _honest_passes_mutants_fail(quick, R.act_inputs(R.ACT_QUICK_GELU), "quick_gelu")
    _honest_passes_mutants_fail(NS(**{**vars(R.ACT), "mutants": []}), R.act_inputs(R.ACT_RELU), "relu")


@pytest.mark.parametrize("V", [1000, 1003, 32064])
def test_ce_regimes(V):
    tail = V % 8 != 0
    must = ["no_max_subtraction", "onehot_missing_last_chunk"] + (["onehot_missing_scalar_tail"] if tail else [])
    c = _honest_passes_mutants_fail(R.CE, R.ce_inputs(V), f"ce V={V}", must_catch=must)
    if not tail:
        assert not c["onehot_missing_scalar_tail"]               # no scalar tail at V % 8 == 0: that mutant IS the honest kernel there
    ref = R.CE.ref(R.ce_inputs(V), torch.float64)
    kinds = R.ce_inputs(V).kinds
    assert abs(float(ref["row_loss"][kinds.index("constant")]) - math.log(V)) < 1e-9
    assert float(ref["row_loss"][kinds.index("dominant")]) < 1e-30 and float(ref["dlogits"][kinds.index("dominant")].abs().max()) < 1e-30


EMB_SHAPES = [(3, 1, 0, 40 * 1024, [1., 0., 1.]), (20, 4, 3, 7 * 24, [0.5] * 20)]


@pytest.mark.parametrize("B,world,rank,D,mask", EMB_SHAPES)
def test_emb_loss_regimes(B, world, rank, D, mask):
    caught = {m: [] for m in R.EMB.mutants}
    for ls in R.EMB_SCALES:
        inp = R.emb_inputs(B, world, rank, D, mask, ls)
        c = _honest_passes_mutants_fail(R.EMB, inp, f"emb ls={ls}", must_catch=[])
        for m, bad in c.items():
            caught[m] += [(ls,) + k for k in bad]
        ref = R.EMB.ref(inp, torch.float64)
        if ls is not None and ls > R.LN100:
            assert float(ref["dls"]) == 0.0                      # exactly zero above the clamp
        elif ls is not None:
            assert float(ref["dls"].abs()) > 1e-3
    above = [ls for ls in R.EMB_SCALES if ls is not None and ls > R.LN100]
    assert {k[0] for k in caught["clamp_ignored_fwd"]} == set(above)
    assert {(k[0], k[1]) for k in caught["clamp_ignored_in_dls"]} == {(ls, "dls") for ls in above}
    assert any(k[0] is None and k[1] == "dpred" for k in caught["backward_clamp_missing"])
    assert any(k[1] == "out3" for k in caught["smooth_l1_threshold_half"])
    if any(m > 0 and k == "quad" for m, k in zip(mask, inp.kinds)):        # (B = 3: the only all-quadratic row is the masked one)
        assert any(k[1:] == ("dpred", "quad") for k in caught["smooth_l1_threshold_half"])
    zero = R.emb_inputs(B, world, rank, D, [0.0] * B, 2.0)
    out = R.simulate(R.EMB, zero)
    assert float(out["out3"].abs().max()) == 0.0 and float(out["dpred"].abs().max()) == 0.0


@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_regimes(step, wd):
    must = ["eps_inside_sqrt"] + (["bias_correction_missing"] if step <= 1000 else []) + (["weight_decay_after_update"] if wd else [])
    c = _honest_passes_mutants_fail(R.ADAMW, R.adamw_inputs(5003, step, wd), f"adamw step={step} wd={wd}", must_catch=must)
    if step == 100000:
        assert not c["bias_correction_missing"]                  # 1 - beta^step == 1 in fp32 and to 1e-44 in fp64: nothing to miss
    if not wd:
        assert not c["weight_decay_after_update"]


def test_group_err_conventions():
    ref = torch.tensor([[1.0, 2.0], [0.0, 0.0], [1e-3, 2e-3]], dtype=torch.float64)
    groups = {"big": [0], "zero": [1], "small": [2]}
    got = ref.clone(); got[2, 1] = 3e-3
    e = R.group_err(got, ref, groups)
    assert e["big"] == 0.0 and e["zero"] == 0.0 and abs(e["small"] - 0.5) < 1e-12           # 1e-3 / 2e-3: not hidden by the big row
    assert parity_max_rel(got, ref) < 1e-3                                                    # ... as the tensor-wide maximum hides it
    got = ref.clone(); got[1, 0] = 1e-30
    assert R.group_err(got, ref, groups)["zero"] == R.INF                                     # all-zero reference: exact zeros
    got = ref.clone(); got[0, 0] = float("nan")
    assert R.group_err(got, ref, groups)["big"] == R.INF
    got = ref.clone(); got[2, 0] += 2.0 ** -121
    assert R.group_err(got, ref, groups)["small"] == 0.0                                      # the one absolute allowance
    assert R.bound(R.out_spec(r=2), 0.0) == 3 * 2.0 ** -8 and R.bound(R.out_spec(), 1e-6) == 16 * 2.0 ** -24 + 4e-6
    assert R.bound(R.out_spec(n=1024), 0.0) == 2e-5 * 2.0


def parity_max_rel(got, ref):
    import parity
    return parity.max_rel(got, ref)


# ------------------------------------------------------------------------------------------------ the old comparisons on the old inputs
def _passes(fn):
    try:
        fn()
        return True
    except AssertionError:
        return False


def _old_rmsnorm(mut):
    M, H = 37, 64
    x, w, dy, dres = rnd(M, H, seed=10), (1 + 0.1 * rnd(H, seed=11).float()).to(BF), rnd(M, H, seed=12), rnd(M, H, seed=13)
    inp = NS(x=x, w=w, dy=dy, dres=dres, eps=1e-5, kinds=["all"] * M, H=H)
    got, ref = R.simulate(R.RMSNORM, inp, mut), R.RMSNORM.ref(inp, torch.float32)
    close(got["y"], ref["y"]); close(got["dx"], ref["dx"])


def _old_layernorm(mut):
    M, H = 37, 64
    x, w, b, dy = rnd(M, H, seed=14), (1 + 0.1 * rnd(H, seed=15).float()).to(BF), rnd(H, scale=0.1, seed=16), rnd(M, H, seed=17)
    inp = NS(x=x, w=w, b=b, dy=dy, eps=1e-5, kinds=["all"] * M, H=H)
    got, ref = R.simulate(R.LAYERNORM, inp, mut), R.LAYERNORM.ref(inp, torch.float32)
    close(got["y"], ref["y"]); close(got["dx"], ref["dx"]); close(got["dw"], ref["dw"], rtol=1e-2); close(got["db"], ref["db"], rtol=1e-2)


def _old_swiglu(mut):
    M, Fd = 33, 136
    gu, d = rnd(M, 2 * Fd, seed=20), rnd(M, Fd, seed=21)
    inp = NS(gate=gu[:, :Fd], up=gu[:, Fd:], dact=d, kinds=["all"] * Fd, Fd=Fd)
    got, ref = R.simulate(R.SWIGLU, inp, mut), R.SWIGLU.ref(inp, torch.float32)
    close(got["act"], ref["act"])
    close(torch.cat([got["dgate"], got["dup"]], 1), torch.cat([ref["dgate"], ref["dup"]], 1))


def _old_act(mut):
    x, d = rnd(40, 64, seed=22), rnd(40, 64, seed=23)
    for kind in (R.ACT_GELU, R.ACT_QUICK_GELU):                   # (quick-GELU: test_gemm_epilogues' pre-activations are of the same size)
        inp = NS(x=x, dy=d, kind=kind, kinds=["all"] * 64)
        got, ref = R.simulate(R.ACT, inp, mut), R.ACT.ref(inp, torch.float32)
        close(got["y"], ref["y"]); close(got["dx"], ref["dx"])


def _old_ce(mut):
    rows, V = 37, 1000
    lg = rnd(rows, V, scale=2.0, seed=39)
    labels = torch.randint(0, V, (rows,), generator=R.gen(0))
    labels[::5] = -100
    n = int((labels != -100).sum())
    inp = NS(logits=lg, labels=labels, gs=1.0 / n, kinds=["all"] * rows, V=V)
    got, ref = R.simulate(R.CE, inp, mut), R.CE.ref(inp, torch.float32)
    close(got["row_loss"].sum()[None], ref["row_loss"].sum()[None], rtol=1e-4, atol=1e-3)
    close(got["dlogits"], ref["dlogits"], rtol=2e-2, atol=2e-3 * float(ref["dlogits"].abs().max()))


def _old_emb(mut):
    B, D = 3, 40 * 1024
    pred, tg_all = rnd(3, 40, 1024, scale=1.3, seed=40).reshape(B, D), rnd(B, D, seed=41)
    inp = NS(pred=pred, tg_all=tg_all, mask=torch.tensor([1., 0., 1.]), ls=2.0, w_con=0.3, rank=0, gout=0.5, kinds=["all"] * B, D=D, B=B)
    got, ref = R.simulate(R.EMB, inp, mut), R.EMB.ref(inp, torch.float32)
    close(got["out3"], ref["out3"], rtol=2e-3, atol=1e-5)
    close(got["dpred"], ref["dpred"], rtol=3e-2, atol=2e-2 * float(ref["dpred"].abs().max()))
    close(got["dls"] * 0.5, ref["dls"] * 0.5, rtol=5e-3, atol=1e-6)


def _old_adamw(mut):
    n = 5000
    p0, g = torch.randn(n, generator=R.gen(1)), torch.randn(n, generator=R.gen(2))
    state = {}
    for which in (mut, None):
        p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
        for step in (1, 2, 3):
            inp = NS(p=p, g=g * step, m=m, v=v, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, step=step, gs=1.0, kinds=["all"] * n)
            out = R.ADAMW.ref(inp, torch.float32, which)
            p, m, v = p + out["dp"], out["m"], out["v"]
        state[which] = p
    close(state[mut], state[None], rtol=1e-5, atol=1e-6)


OLD = {"rmsnorm": _old_rmsnorm, "layernorm": _old_layernorm, "swiglu": _old_swiglu, "act": _old_act, "ce": _old_ce, "emb_loss": _old_emb,
       "adamw": _old_adamw}
# the exceptions: mutants that today's comparison on today's inputs does notice (all others pass it)
OLD_CATCHES = {
    ("ce", "onehot_missing_last_chunk"),          # by luck: one of the 30 random labels drawn here is in the last 8 columns (about one draw in five;
                                                  # test_ce draws its labels unseeded)
    ("emb_loss", "smooth_l1_threshold_half"),     # differences of std 1.6 land on both sides of the kink, so both smooth-L1 mistakes move the
    ("emb_loss", "backward_clamp_missing"),       # loss and d-pred by tens of percent there too; what the old inputs miss is the clamp on exp(s)
    ("adamw", "eps_inside_sqrt"),                 # a handful of the 5000 unit-Gaussian gradients are below 1e-3, where eps placement shows
    ("adamw", "bias_correction_missing"),         # steps 1-3: the corrections are far from 1
    ("adamw", "weight_decay_after_update"),       # 1e-5 of p after three steps, just above test_adamw's rtol
}


def test_mutants_pass_the_old_comparisons():
    seen = set()
    for op in (R.RMSNORM, R.LAYERNORM, R.SWIGLU, R.ACT, R.CE, R.EMB, R.ADAMW):
        assert _passes(lambda: OLD[op.name](None)), op.name
        muts = op.mutants + (["sigmoid_exp_pos"] if op is R.ACT else [])
        for mut in muts:
            if not _passes(lambda: OLD[op.name](mut)):
                seen.add((op.name, mut))
            print(f"[mutant] {op.name:10s} {mut:28s} old comparison: {'CAUGHT' if (op.name, mut) in seen else 'passes'}")
    assert seen == set(OLD_CATCHES), (sorted(seen), sorted(OLD_CATCHES))
