"""Input regimes where eps, clamps and saturation act, shared by tests/test_regimes_host.py (CPU) and tests/test_kernels_regimes_gpu.py.

Per operation: a seeded builder of bf16-rounded inputs with named regime GROUPS, a reference of the operation that runs in any float
dtype with the kernel's documented bf16 rounding points restated (the LAST rounding of a bf16 output is left out), and MUTANTS: the same
reference with one plausible mistake.  One comparator, `group_err`, normalises per group (a tensor-wide maximum lets a large row hide a
small one), and the bound is computed, never typed in:

    bf16 output, r roundings on the path:   (2 r - 1) * 2^-8 + 4 y
    fp32 output, element-wise:              16 * 2^-24       + 4 y
    fp32 output that sums n terms:          2e-5 * max(1, n / 256)^0.5 + 4 y     (the form of the fp32 GEMM checks in test_kernels_gpu.py)

y, the yardstick, is group_err of the honest reference evaluated in fp32 with torch against the same reference in fp64, on the same inputs.
Nothing in a bound comes from the code under test."""
import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

import parity

BF = torch.bfloat16
ABS_ALLOW = 2.0 ** -120         # |x| e^-|x| < 2^-121 once fp32 exp overflows (|x| > 88.7): a kernel may return 0 where fp64 does not
INF = float("inf")


def bfr(t):
    """round to bf16, keep the dtype (a restated rounding point)"""
    return t.to(BF).to(t.dtype)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ comparator and bound
def group_err(got, ref64, groups=None, norm=None):
    """{group: max |got - ref| / max |ref| of that group}.  A group whose reference is all zero requires exact zeros; a non-finite value where
    the reference is finite is an error of infinity; `norm` replaces the group maximum (a fixed scale, e.g. CE's grad_scale).
    groups: {name: index into the first dim(s)} (anything `tensor[idx]` accepts); default one group over everything."""
    got, ref = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out = {}
    for name, idx in ({"all": Ellipsis} if groups is None else groups).items():
        g, r = got[idx].reshape(-1), ref[idx].reshape(-1)
        fin = torch.isfinite(r)
        g, r = g[fin], r[fin]
        if r.numel() == 0:
            out[name] = 0.0
        elif not bool(torch.isfinite(g).all()):
            out[name] = INF
        else:
            rmax = float(r.abs().max()) if norm is None else float(norm)
            if rmax == 0.0:
                out[name] = 0.0 if bool((g == 0).all()) else INF
            else:
                out[name] = float(((g - r).abs() - ABS_ALLOW).clamp_min(0).max()) / rmax
    return out


def bound(spec, y):
    if spec.r > 0:
        return (2 * spec.r - 1) * 2.0 ** -8 + 4.0 * y
    floor = 16 * 2.0 ** -24 if spec.n is None else 2e-5 * max(1.0, spec.n / 256.0) ** 0.5
    return floor + 4.0 * y


def out_spec(r=0, n=None, groups=None, norm=None):
    """r: bf16 roundings on the path to a bf16 output (0 = fp32 output); n: terms summed by an fp32 output (None = element-wise)"""
    return NS(r=r, n=n, groups=groups, norm=norm)


def evaluate(op, inp, got):
    """{(output, group): (error of `got`, bound)} for every output of `op` present in `got`"""
    ref64, ref32 = op.ref(inp, torch.float64), op.ref(inp, torch.float32)
    res = {}
    for name, spec in op.outputs(inp).items():
        if name not in got:
            continue
        y = group_err(ref32[name], ref64[name], spec.groups, spec.norm)
        e = group_err(got[name], ref64[name], spec.groups, spec.norm)
        for g in e:
            res[(name, g)] = (e[g], bound(spec, y[g]))
    return res


def check_all(label, res):
    """every comparison through parity.check (so the measured value is recorded), all of them before the first failure is raised"""
    fails = []
    for (name, g), (e, b) in res.items():
        try:
            parity.check(f"regime {label} {name}[{g}]", e if math.isfinite(e) else 1e30, b)
        except AssertionError as ex:
            fails.append(str(ex))
    assert not fails, "\n".join(fails)


def failures(res):
    return [k for k, (e, b) in res.items() if not e <= b]


def simulate(op, inp, mut=None):
    """what a kernel with fp32 math would return: the reference (or a mutant of it) in fp32, bf16 outputs rounded"""
    out = op.ref(inp, torch.float32, mut)
    return {k: (bfr(v) if op.outputs(inp)[k].r > 0 else v) for k, v in out.items()}


def row_groups(kinds):
    names = []
    for k in kinds:
        if k not in names:
            names.append(k)
    return {k: torch.tensor([i for i, kk in enumerate(kinds) if kk == k]) for k in names}


# ------------------------------------------------------------------------------------------------ norms
def norm_rows(H, seed, layer):
    """rows of scale 1e-3, 1e-2, 1, 1e2 (3 each), an all-zero row, a row with one channel 500 times the rest; LayerNorm also rows with mean 100
    / std 1 and mean 1000 / std 4 (where a one-pass fp32 variance cancels)."""
    base = torch.randn(20, H, generator=gen(seed))
    rows, kinds = [], []
    for i, s in enumerate((1e-3, 1e-2, 1.0, 1e2)):
        for j in range(3):
            rows.append(base[3 * i + j] * s)
            kinds.append(f"scale{s:g}")
    rows.append(torch.zeros(H)); kinds.append("zero")
    spike = base[12].clone(); spike[H // 3] = 500.0
    rows.append(spike); kinds.append("spike")
    if layer:
        for j in range(2):
            rows.append(100.0 + base[13 + j]); kinds.append("mean100")
        for j in range(2):
            rows.append(1000.0 + 4.0 * base[15 + j]); kinds.append("mean1000")
    return torch.stack(rows).to(BF), kinds


def rmsnorm_inputs(H, seed=0):
    x, kinds = norm_rows(H, 100 + seed, False)
    M = x.shape[0]
    w = (1 + 0.1 * torch.randn(H, generator=gen(101 + seed))).to(BF)
    dy = randn(M, H, seed=102 + seed)
    # the residual-stream gradient at the size of the norm's own dx (rstd * dy), so it does not drown it in the large-rstd rows
    rs = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    dres = (torch.randn(M, H, generator=gen(103 + seed)) * rs).to(BF)
    return NS(x=x, w=w, dy=dy, dres=dres, eps=1e-5, kinds=kinds, H=H)


def rmsnorm_ref(inp, dt, mut=None):
    """HF LlamaRMSNorm: y = w * bf16(x * rsqrt(mean(x^2) + eps)) (norm.hip: two roundings); dx = rstd (g - x rstd^2 mean(g x)) + dres, g = w dy;
    dw = sum_rows dy x rstd."""
    x, w, dy, dres = (t.to(dt) for t in (inp.x, inp.w, inp.dy, inp.dres))
    ms = x.pow(2).mean(-1, keepdim=True)
    if mut == "eps_dropped":
        rstd = torch.rsqrt(ms)
    elif mut == "eps_outside_sqrt":
        rstd = 1.0 / (ms.sqrt() + inp.eps)
    else:
        rstd = torch.rsqrt(ms + inp.eps)
    y = w * bfr(x * rstd)
    g = w * dy
    coef = (g * x).mean(-1, keepdim=True) * rstd * rstd
    dx = rstd * (g - x * coef) + dres
    return dict(y=y, rstd=rstd[:, 0], dx=dx, dw=(dy * x * rstd).sum(0))


def rmsnorm_outputs(inp):
    gr = row_groups(inp.kinds)
    return dict(y=out_spec(r=2, groups=gr), rstd=out_spec(n=inp.H, groups=gr), dx=out_spec(r=1, groups=gr), dw=out_spec(n=len(inp.kinds)))


RMSNORM = NS(name="rmsnorm", ref=rmsnorm_ref, outputs=rmsnorm_outputs, mutants=["eps_dropped", "eps_outside_sqrt"])


def layernorm_inputs(H, seed=0):
    x, kinds = norm_rows(H, 110 + seed, True)
    M = x.shape[0]
    w = (1 + 0.1 * torch.randn(H, generator=gen(111 + seed))).to(BF)
    b = randn(H, seed=112 + seed, scale=0.1)
    dy = randn(M, H, seed=113 + seed)
    return NS(x=x, w=w, b=b, dy=dy, eps=1e-5, kinds=kinds, H=H)


def layernorm_ref(inp, dt, mut=None):
    """torch layer_norm, one rounding (norm.hip); dx = rstd (g - mean(g) - xhat mean(g xhat)), g = w dy; dw = sum_rows dy xhat, db = sum_rows dy"""
    x, w, b, dy = (t.to(dt) for t in (inp.x, inp.w, inp.b, inp.dy))
    mean = x.mean(-1, keepdim=True)
    if mut == "var_one_pass":
        var = (x * x).mean(-1, keepdim=True) - mean * mean
    else:
        var = (x - mean).pow(2).mean(-1, keepdim=True)
    if mut == "eps_dropped":
        rstd = torch.rsqrt(var)
    elif mut == "eps_outside_sqrt":
        rstd = 1.0 / (var.sqrt() + inp.eps)
    else:
        rstd = torch.rsqrt(var + inp.eps)
    xh = (x - mean) * rstd
    y = xh * w + b
    g = w * dy
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dw=(dy * xh).sum(0), db=dy.sum(0))


def layernorm_outputs(inp):
    gr = row_groups(inp.kinds)
    M = len(inp.kinds)
    return dict(y=out_spec(r=1, groups=gr), mean=out_spec(n=inp.H, groups=gr), rstd=out_spec(n=inp.H, groups=gr), dx=out_spec(r=1, groups=gr),
                dw=out_spec(n=M), db=out_spec(n=M))


LAYERNORM = NS(name="layernorm", ref=layernorm_ref, outputs=layernorm_outputs, mutants=["eps_dropped", "eps_outside_sqrt", "var_one_pass"])


# ------------------------------------------------------------------------------------------------ activations
GRID = [0.0, 2.0 ** -20, 1.0, 5.0, 20.0, 60.0, 90.0, 120.0, 300.0]


def act_grid():
    """the value grid, both signs, each value with its three bf16 neighbours on either side (so that a group's yardstick is not one sample).
    -> values bf16 [n], {group: indices}"""
    vals, kinds = [], []
    for v in GRID:
        for sgn in ((1.0,) if v == 0 else (1.0, -1.0)):
            c = torch.tensor([v * sgn]).to(BF)
            nb = [c]
            if v != 0:
                bits = c.view(torch.int16)
                nb += [(bits + k).view(BF) for k in (-3, -2, -1, 1, 2, 3)]
            for t in nb:
                vals.append(t)
                kinds.append(f"{'-' if sgn < 0 else '+'}{v:g}")
    return torch.cat(vals), kinds


def _sigmoid(x, mut, name):
    if mut == name:
        e = torch.exp(x)
        return e / (1 + e)                    # NaN once exp overflows
    return torch.sigmoid(x)


def swiglu_inputs(Fd=None, seed=0):
    """gate = the grid repeated along F columns (default: the grid size padded to a multiple of 8), 8 rows of up / dact patterns in +-[0.25, 1]"""
    vals, kinds = act_grid()
    n = vals.numel()
    Fd = (n + 7) // 8 * 8 if Fd is None else Fd
    R = 8
    col = torch.arange(Fd) % n
    gate = vals.float()[col][None].expand(R, Fd)
    mag = lambda s: (torch.rand(R, Fd, generator=gen(s)) * 0.75 + 0.25) * torch.where(torch.rand(R, Fd, generator=gen(s + 1)) < 0.5, -1.0, 1.0)
    up, dact = mag(120 + seed), mag(122 + seed)
    return NS(gate=gate.contiguous().to(BF), up=up.to(BF), dact=dact.to(BF), kinds=[kinds[int(c)] for c in col], Fd=Fd)


def swiglu_ref(inp, dt, mut=None):
    """act = bf16(silu(gate)) * up (elementwise.hip swiglu_fwd_kernel: two roundings); dgate = dact up s (1 + g (1 - s)), dup = dact g s (one)"""
    g, u, d = (t.to(dt) for t in (inp.gate, inp.up, inp.dact))
    s = _sigmoid(g, mut, "sigmoid_exp_pos")
    act = bfr(g * s) * u
    if mut == "silu_grad_exp_neg":
        e = torch.exp(-g)
        ss = 1 / (1 + e)
        ds = ss * (1 + g * e * ss)                # inf * 0 once exp(-x) overflows
    else:
        ds = s * (1 + g * (1 - s))
    return dict(act=act, dgate=d * u * ds, dup=d * g * s)


def col_groups(kinds):
    return {k: (Ellipsis, idx) for k, idx in row_groups(kinds).items()}


def swiglu_outputs(inp):
    gr = col_groups(inp.kinds)
    return dict(act=out_spec(r=2, groups=gr), dgate=out_spec(r=1, groups=gr), dup=out_spec(r=1, groups=gr))


SWIGLU = NS(name="swiglu", ref=swiglu_ref, outputs=swiglu_outputs, mutants=["sigmoid_exp_pos", "silu_grad_exp_neg"])

ACT_GELU, ACT_QUICK_GELU, ACT_RELU = 1, 2, 3


def act_inputs(kind, Fd=None, seed=0):
    vals, kinds = act_grid()
    n = vals.numel()
    Fd = (n + 7) // 8 * 8 if Fd is None else Fd
    col = torch.arange(Fd) % n
    x = vals.float()[col][None].expand(8, Fd).contiguous()
    dy = (torch.rand(8, Fd, generator=gen(130 + seed)) * 0.75 + 0.25) * torch.where(torch.rand(8, Fd, generator=gen(131 + seed)) < 0.5, -1.0, 1.0)
    return NS(x=x.to(BF), dy=dy.to(BF), kind=kind, kinds=[kinds[int(c)] for c in col])


def act_ref(inp, dt, mut=None):
    """erf GELU / quick-GELU x sigmoid(1.702 x) / ReLU and their gradients, one rounding each (elementwise.hip act_*_kernel, common.h)"""
    x, dy = inp.x.to(dt), inp.dy.to(dt)
    if inp.kind == ACT_GELU:
        if mut == "gelu_tanh":
            y = F.gelu(x, approximate="tanh")
            xr = x.clone().requires_grad_(True)
            gr, = torch.autograd.grad(F.gelu(xr, approximate="tanh").sum(), xr)
        else:
            cdf = 0.5 * (1 + torch.erf(x * 0.70710678118654752))
            y = x * cdf
            gr = cdf + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
    elif inp.kind == ACT_QUICK_GELU:
        s = _sigmoid(1.702 * x, mut, "sigmoid_exp_pos")
        y, gr = x * s, s * (1 + 1.702 * x * (1 - s))
    else:
        y, gr = x.clamp_min(0), (x > 0).to(dt)
    return dict(y=y, dx=dy * gr)


def act_outputs(inp):
    gr = col_groups(inp.kinds)
    return dict(y=out_spec(r=1, groups=gr), dx=out_spec(r=1, groups=gr))


ACT = NS(name="act", ref=act_ref, outputs=act_outputs, mutants=["gelu_tanh"])


# ------------------------------------------------------------------------------------------------ cross entropy
def ce_inputs(V, seed=0, rows=24):
    """logits of std 30; one row with a dominant logit; one constant row; the row maximum in the last 8-wide chunk and in the last element (the
    scalar tail when V % 8 != 0); labels 0, V - 1, the dominant index, -100."""
    lg = torch.randn(rows, V, generator=gen(140 + seed)) * 30.0
    labels = torch.randint(0, V, (rows,), generator=gen(141 + seed))
    kinds = ["random"] * rows
    lg[1] = torch.randn(V, generator=gen(142 + seed)); lg[1, V // 2 + 3] = 200.0; labels[1] = V // 2 + 3; kinds[1] = "dominant"
    lg[2] = 3.0; labels[2] = 5; kinds[2] = "constant"
    lg[3, V - 6] = 400.0; labels[3] = V - 1; kinds[3] = "max_last_chunk"            # the label is NOT the maximum: loss ~ 400, p_label ~ 0
    lg[4, V - 1] = 400.0; labels[4] = V - 1; kinds[4] = "max_last_elem"
    lg[5, V - 1] = lg[5].max() + 1.0; labels[5] = V - 1; kinds[5] = "label_last"       # p_label of order 0.5: the onehot term matters
    lg[6, 0] = lg[6].max() + 1.0; labels[6] = 0; kinds[6] = "label_first"
    labels[7] = -100; kinds[7] = "ignored"
    labels[8] = V - 1; labels[9] = 0
    labels[rows - 1] = -100; kinds[rows - 1] = "ignored"
    return NS(logits=lg.to(BF), labels=labels, gs=1.0 / 16, kinds=kinds, V=V)


def ce_ref(inp, dt, mut=None):
    """row_loss = logsumexp - logit[label] (0 for ignored rows); dlogits = (softmax - onehot) grad_scale, one rounding (loss.hip)"""
    x = inp.logits.to(dt)
    V = x.shape[1]
    lab = inp.labels
    keep = (lab >= 0)
    safe = lab.clamp_min(0)
    if mut == "no_max_subtraction":
        e = torch.exp(x)
        S = e.sum(-1, keepdim=True)
        lse, p = torch.log(S), e / S
    else:
        lse = torch.logsumexp(x, -1, keepdim=True)
        p = torch.exp(x - lse)
    loss = (lse[:, 0] - x.gather(1, safe[:, None])[:, 0]) * keep
    onehot = F.one_hot(safe, V).to(dt)
    if mut == "onehot_missing_last_chunk":
        onehot = onehot * (safe < (V - 1) // 8 * 8)[:, None]
    elif mut == "onehot_missing_scalar_tail":
        onehot = onehot * (safe < V // 8 * 8)[:, None]
    return dict(row_loss=loss, dlogits=(p - onehot) * inp.gs * keep[:, None])


def ce_outputs(inp):
    return dict(row_loss=out_spec(n=inp.V), dlogits=out_spec(r=1, groups=row_groups(inp.kinds), norm=inp.gs))


CE = NS(name="ce", ref=ce_ref, outputs=ce_outputs, mutants=["no_max_subtraction", "onehot_missing_last_chunk", "onehot_missing_scalar_tail"])


# ------------------------------------------------------------------------------------------------ embedding loss
LN100 = math.log(100.0)
EMB_SCALES = [2.0, LN100 - 0.01, LN100 + 0.01, 5.0, None]


def emb_inputs(B, world, rank, D, mask, logit_scale, seed=0):
    """pred on a 1/8 grid in [-1.625, 1.625]; the local targets are pred + d with |d| all below 1 (row kind `quad`), all above 1 (`lin`), exactly +-1
    (`kink`) or mixed (`mixed`), d on the same grid so the bf16 difference is exact; the other ranks' targets are unit Gaussians."""
    g = gen(150 + seed)
    q = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float() / 8.0
    pred = q(-12, 12, (1, D)) + q(-1, 1, (B, D))             # a shared direction + a small own part: the B x Bw softmax is not saturated at scale 100
    sign = torch.where(torch.rand(B, D, generator=g) < 0.5, -1.0, 1.0)
    kinds, d = [], torch.empty(B, D)
    for b in range(B):
        k = ("lin", "quad", "kink", "mixed")[b % 4]
        kinds.append(k)
        d[b] = {"quad": q(0, 7, (D,)), "lin": q(9, 24, (D,)), "kink": torch.ones(D), "mixed": q(0, 24, (D,))}[k] * sign[b]
    tg_all = torch.randn(B * world, D, generator=g)
    tg_all[rank * B:(rank + 1) * B] = pred + d
    return NS(pred=pred.to(BF), tg_all=tg_all.to(BF), mask=torch.tensor(mask, dtype=torch.float32), ls=logit_scale, w_con=0.3, rank=rank, gout=0.5,
              kinds=kinds, D=D, B=B)


def emb_ref(inp, dt, mut=None):
    """_emb_loss + calculate_contrastive_loss as oracle.visper_oracle.emb_loss states them (the oracle itself casts to fp32, so it is restated
    here to run in fp64): out3 = (sl1 + con, sl1, con), dpred = d (gout * loss) / d pred (one rounding, emb_loss.hip:579), dls = d loss / d logit_scale."""
    B = inp.B
    p = inp.pred.to(dt).clone().requires_grad_(True)
    t_all = inp.tg_all.to(dt)
    m = inp.mask.to(dt)
    d = p - t_all[inp.rank * B:(inp.rank + 1) * B]
    thr = 0.5 if mut == "smooth_l1_threshold_half" else 1.0
    quad, lin = 0.5 * d * d / thr, d.abs() - 0.5 * thr
    el = torch.where(d.abs() < thr, quad, lin)
    if mut == "backward_clamp_missing":
        el = el.detach() + (0.5 * d * d - (0.5 * d * d).detach())
    sl1 = (el * m[:, None]).mean()
    con = torch.zeros((), dtype=dt)
    ls = None
    if inp.ls is not None:
        ls = torch.tensor(inp.ls, dtype=dt, requires_grad=True)
        e = ls.exp()
        sc = torch.clamp(e, max=100.0)
        if mut == "clamp_ignored_fwd":
            sc = e
        elif mut == "clamp_ignored_in_dls":
            sc = sc.detach() + (e - e.detach())
        z = (F.normalize(p, dim=-1) @ F.normalize(t_all, dim=-1).t()) * sc
        ce = F.cross_entropy(z, torch.arange(B) + B * inp.rank, reduction="none")
        con = inp.w_con * ce.mean() * m.mean()
    loss = sl1 + con
    grads = torch.autograd.grad(loss, [p] + ([ls] if ls is not None else []), allow_unused=True)
    dp = grads[0] if grads[0] is not None else torch.zeros_like(p)
    dls = grads[1] if ls is not None else torch.zeros((), dtype=dt)
    return dict(out3=torch.stack([loss, sl1, con]).detach(), dpred=dp.detach() * inp.gout, dls=dls.detach().reshape(1))


def emb_outputs(inp):
    return dict(out3=out_spec(n=inp.D, groups={"loss": [0], "sl1": [1], "con": [2]}), dpred=out_spec(r=1, groups=row_groups(inp.kinds)),
                dls=out_spec(n=inp.D))


EMB = NS(name="emb_loss", ref=emb_ref, outputs=emb_outputs,
         mutants=["clamp_ignored_fwd", "clamp_ignored_in_dls", "smooth_l1_threshold_half", "backward_clamp_missing"])


# ------------------------------------------------------------------------------------------------ AdamW
ADAM_LADDER = [0.0, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-4, 1e-2, 1.0]


def adamw_inputs(n, step, wd, seed=0):
    """per-element gradient ladder 0, 1e-10 ... 1 (element i takes rung i % 9, random sign and a factor in [0.5, 1.5]) so that sqrt(v) / bc2
    straddles eps = 1e-8; for step > 1 the moments are seeded with fp32 values of the gradient's size (no iteration to get there)."""
    g_ = gen(160 + seed)
    rung = torch.tensor(ADAM_LADDER)[torch.arange(n) % len(ADAM_LADDER)]
    fac = lambda: (torch.rand(n, generator=g_) + 0.5)
    sign = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    g = (rung * fac() * sign).float()
    p = torch.randn(n, generator=g_).float()
    if step > 1:
        m, v = (rung * fac() * sign * 0.5).float(), (rung * rung * fac()).float()
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    kinds = [f"g{ADAM_LADDER[i % len(ADAM_LADDER)]:g}" for i in range(n)]
    return NS(p=p, g=g, m=m, v=v, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=wd, step=step, gs=0.5, kinds=kinds)


def adamw_ref(inp, dt, mut=None):
    """torch.optim.AdamW's update restated: p *= 1 - lr wd; m, v EMAs; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  Hyper-parameters and the
    bias corrections are formed in `dt` (the launcher forms them with powf in fp32, elementwise.hip vp_adamw).  dp = p_new - p_old."""
    c = lambda s: torch.tensor(s, dtype=dt)
    p, g, m, v = (t.to(dt) for t in (inp.p, inp.g, inp.m, inp.v))
    lr, b1, b2, eps, wd = c(inp.lr), c(inp.b1), c(inp.b2), c(inp.eps), c(inp.wd)
    gr = g * c(inp.gs)
    m1 = b1 * m + (1 - b1) * gr
    v1 = b2 * v + (1 - b2) * gr * gr
    one = c(1.0)
    bc1, bc2 = (one, one) if mut == "bias_correction_missing" else (1 - torch.pow(b1, c(float(inp.step))), 1 - torch.pow(b2, c(float(inp.step))))
    if mut == "eps_inside_sqrt":
        den = (v1 / bc2 + eps).sqrt()
    else:
        den = v1.sqrt() / bc2.sqrt() + eps
    upd = (lr / bc1) * m1 / den
    if mut == "weight_decay_after_update":
        p1 = (p - upd) * (1 - lr * wd)
    else:
        p1 = p * (1 - lr * wd) - upd
    return dict(dp=p1 - p, m=m1, v=v1)


def adamw_outputs(inp):
    gr = row_groups(inp.kinds)
    return dict(dp=out_spec(groups=gr), m=out_spec(groups=gr), v=out_spec(groups=gr))


ADAMW = NS(name="adamw", ref=adamw_ref, outputs=adamw_outputs, mutants=["eps_inside_sqrt", "bias_correction_missing", "weight_decay_after_update"])


# ------------------------------------------------------------------------------------------------ attention with a late large maximum
def late_max_attention_inputs(D, S=512, B=1, Hq=4, Hkv=2, seed=0):
    """The construction of test_attention_d128_rescale_branch_mid_sequence at any head dim: a few keys aligned with a few query rows so that
    their scores jump by ~30 and then ~16 more log2 units in LATER key tiles; the other rows stay ordinary."""
    q, k, v, do = (randn(B, S, h, D, seed=170 + seed + i) for i, h in enumerate((Hq, Hkv, Hkv, Hq)))
    u = torch.ones(D) / math.sqrt(D)
    for j, mag in ((130, 16.0), (140, 16.0), (170, 16.0), (300, 24.0), (450, 32.0)):
        k[0, j, :, :] = (mag * u).to(BF)
        v[0, j, :, :] = (v[0, j, :, :].float() * 3.0).to(BF)
    rows = (5, 135, 200, 260, 310, 400, 460, 511)
    for r in rows:
        q[0, r, :, :] = (16.0 * u + 0.5 * q[0, r, :, :].float()).to(BF)
    kinds = ["aligned" if r in rows else "ordinary" for r in range(S)]
    return NS(q=q, k=k, v=v, do=do, kinds=kinds, D=D)


def attention_ref(q, k, v, do, dt, causal, bias=None):
    """softmax(q k^T / sqrt(D) [+ bias]) v with HF-eager semantics in `dt`, and its gradients for the output gradient `do`.
    q [B,S,Hq,D], k / v [B,S,Hkv,D]; bias broadcastable to [B,Hq,S,S]."""
    q, k, v = (t.to(dt).clone().requires_grad_(True) for t in (q, k, v))
    B, S, Hq, D = q.shape
    rep = Hq // k.shape[2]
    kk = k.transpose(1, 2).repeat_interleave(rep, dim=1)
    vv = v.transpose(1, 2).repeat_interleave(rep, dim=1)
    s = q.transpose(1, 2) @ kk.transpose(-1, -2) / math.sqrt(D)
    if bias is not None:
        s = s + bias.to(dt)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    o = (torch.softmax(s, -1) @ vv).transpose(1, 2)
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], do.to(dt))
    return dict(o=o.detach(), dq=dq, dk=dk, dv=dv)
