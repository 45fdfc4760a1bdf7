"""The kernels where eps, clamps and saturation act.  Inputs, fp64 references, the per-group comparator and the computed bounds come from
tests/regimes.py; tests/test_regimes_host.py proves on the CPU that these comparisons reject a kernel with eps dropped or misplaced, a
clamp ignored, an overflowing sigmoid, a missing onehot term in the last chunk, ...  Next to each comparison: r, the number of bf16
roundings on the path to a bf16 output, with the kernel line it comes from (r = 0: an fp32 output)."""
import math
import os
import subprocess
import sys

import pytest
import torch

import parity
import regimes as R
from regimes import NS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops as o
    return o


def dev(t):
    return t.cuda()


def ileave(t, Fd):
    """[gate | up] column halves -> the library's 8-wide chunk interleave"""
    g, u = t[..., :Fd], t[..., Fd:]
    return torch.stack([g.reshape(*g.shape[:-1], Fd // 8, 8), u.reshape(*u.shape[:-1], Fd // 8, 8)], -2).reshape(*t.shape)


def unleave(t, Fd):
    t = t.reshape(*t.shape[:-1], Fd // 8, 2, 8)
    return torch.cat([t[..., 0, :].reshape(*t.shape[:-3], Fd), t[..., 1, :].reshape(*t.shape[:-3], Fd)], -1)


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("H", [64, 1024, 4096])
def test_rmsnorm_regimes(ops, H):
    """y: r = 2 (norm.hip:47, bf16(x rstd) then bf16(w .)); rstd: fp32, sums H terms; dx: r = 1 (norm.hip:106); dw: fp32, sums M rows."""
    inp = R.rmsnorm_inputs(H)
    y, rstd = ops.rmsnorm_fwd(dev(inp.x), dev(inp.w), inp.eps)
    dx = ops.rmsnorm_bwd(dev(inp.dy), dev(inp.x), dev(inp.w), rstd, dres=dev(inp.dres))
    dw = ops.rmsnorm_bwd_w(dev(inp.dy), dev(inp.x), rstd)
    R.check_all(f"rmsnorm H={H}", R.evaluate(R.RMSNORM, inp, dict(y=y, rstd=rstd, dx=dx, dw=dw)))
    assert float(y[inp.kinds.index("zero")].float().abs().max()) == 0.0


@pytest.mark.parametrize("H", [64, 1024, 4096])
def test_layernorm_regimes(ops, H):
    """y: r = 1 (norm.hip:171); mean, rstd: fp32, sum H terms; dx: r = 1 (norm.hip:221); dw, db: fp32, sum M rows."""
    inp = R.layernorm_inputs(H)
    y, mean, rstd = ops.layernorm_fwd(dev(inp.x), dev(inp.w), dev(inp.b), inp.eps)
    dx, dw, db = ops.layernorm_bwd(dev(inp.dy), dev(inp.x), dev(inp.w), mean, rstd)
    R.check_all(f"layernorm H={H}", R.evaluate(R.LAYERNORM, inp, dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db)))


def _ladder_rows(M, K, seed):
    """[M, K] rows of scale 1e-3, 1e-2, 1, 1e2 and all-zero rows, in turn -> bf16 rows, kinds"""
    scales = [1e-3, 1e-2, 1.0, 1e2, 0.0]
    s = torch.tensor(scales)[torch.arange(M) % len(scales)]
    x = (torch.randn(M, K, generator=R.gen(seed)) * s[:, None]).to(BF)
    return x, [("zero" if scales[i % len(scales)] == 0 else f"scale{scales[i % len(scales)]:g}") for i in range(M)]


def _rstd_check(label, rstd, rows64, eps, kinds, extra=0.0, why=""):
    """rstd against fp64 rsqrt(mean(x^2) + eps) of the given rows: fp32 output that sums H terms (+ a stated extra term)"""
    H = rows64.shape[1]
    ref64 = torch.rsqrt(rows64.pow(2).mean(-1) + eps)
    ref32 = torch.rsqrt(rows64.float().pow(2).mean(-1) + eps)
    gr = R.row_groups(kinds)
    y, e = R.group_err(ref32, ref64, gr), R.group_err(rstd, ref64, gr)
    for g in e:
        parity.check(f"regime {label} rstd[{g}]{why}", e[g] if math.isfinite(e[g]) else 1e30, R.bound(R.out_spec(n=H), y[g]) + extra)


def test_gemm_sumsq_rstd_regimes(ops):
    """vp_gemm_bf16_sumsq + vp_rstd_from_sumsq on rows of scale 1e-3 .. 1e2 and zero rows, against fp64 rsqrt(mean(x^2) + eps) of the STORED row.
    The partial sums of squares are taken from the fp32 values before the row's bf16 rounding (gemm.hip, asserted by test_gemm_sumsq_and_rstd):
    every stored element is within 2^-9 of the summed one, so sum x^2 moves by at most 2^-8 and rstd by at most 2^-9 relative; that documented
    rounding is added to the fp32 bound."""
    M, N, K, eps = 512, 512, 128, 1e-5
    a, kinds = _ladder_rows(M, K, 200)
    w = R.randn(N, K, seed=201, scale=0.1)
    sc = a.float().abs().amax(1, keepdim=True)
    res = (torch.randn(M, N, generator=R.gen(202)) * sc).to(BF)
    out, part = ops.gemm_sumsq(dev(a), dev(w), dev(res))
    rstd = ops.rstd_from_sumsq(part, N, eps)
    _rstd_check("gemm_sumsq", rstd, out.double().cpu(), eps, kinds, extra=2.0 ** -9, why=" (+2^-9: partials precede the row's rounding)")
    assert float(out[kinds.index("zero")].float().abs().max()) == 0.0


@pytest.mark.parametrize("H", [64, 1024, 4096])
@pytest.mark.parametrize("M", [1, 14])
def test_decode_gemm_norm_prologue_regimes(ops, H, M):
    """vp_decode_gemm's RMSNorm prologue on the regime rows: the normalised A must be vp_rmsnorm_fwd's (decode.hip's dg_rstd_rows claims its rstd bit-identical;
    test_rmsnorm_regimes holds that kernel to fp64), so the fp32 product is compared with fp64 `rmsnorm_fwd(x) @ w^T`: r = 0, sums K = H terms."""
    inp = R.rmsnorm_inputs(H)
    x, kinds = inp.x[-M:], inp.kinds[-M:]                        # M = 1: the spike row; M = 14: every regime
    w = R.randn(136, H, seed=210, scale=0.02)
    xn, _ = ops.rmsnorm_fwd(dev(x), dev(inp.w), inp.eps)
    got = ops.decode_gemm(dev(x), dev(w), norm_w=dev(inp.w), eps=inp.eps, out_f32=True)
    ref64 = xn.double().cpu() @ w.double().t()
    ref32 = xn.float().cpu() @ w.float().t()
    gr = R.row_groups(kinds)
    y, e = R.group_err(ref32, ref64, gr), R.group_err(got, ref64, gr)
    for g in e:
        parity.check(f"regime decode_gemm norm prologue H={H} M={M} [{g}]", e[g] if math.isfinite(e[g]) else 1e30, R.bound(R.out_spec(n=H), y[g]))


def test_folded_norm_row_scale_regimes(ops):
    """RMSNorm folded away: the consuming GEMM multiplies its fp32 accumulators by rstd (vp_gemm_bf16_rope with rope_cols = 0, and the fused
    SwiGLU forward), on the scale ladder.  Reference: fp64 (h @ w^T) * rsqrt(mean(h^2) + eps).  gate_up / the plain product: r = 1 (one rounding
    of acc * scale, gemm.hip); act = bf16(bf16(silu(gate_up)) * up): r = 3."""
    eps = 1e-5
    for name, (M, N, K) in (("gemm_rope", (2048, 2048, 1024)), ("gemm_swiglu_fwd", (4096, 6144, 256))):
        h, kinds = _ladder_rows(M, K, 220)
        w = R.randn(N, K, seed=221, scale=0.1)
        hd = dev(h)
        _, rstd = ops.rmsnorm_fwd(hd, torch.ones(K, device="cuda", dtype=BF), eps)
        _rstd_check(f"folded {name}", rstd, h.double(), eps, kinds)
        gr = R.row_groups(kinds)
        prod = lambda dt: (dev(h).to(dt) @ dev(w).to(dt).t()) * torch.rsqrt(dev(h).to(dt).pow(2).mean(-1, keepdim=True) + eps)      # torch on the GPU: checker only
        ref64, ref32 = prod(torch.float64).cpu(), prod(torch.float32).cpu()
        if name == "gemm_rope":
            assert ops.gemm_rowscale_ok(M, N, K)
            cs, sn = ops.rope_tables(M, 128, 10000.0, "cuda")                  # (not read with rope_cols = 0; sized for every row all the same)
            got = ops.gemm_rope(hd, dev(w), M, 0, cs, sn, row_scale=rstd)
            outs = {"out": (got, ref64, ref32, 1)}
        else:
            gu, act = ops.gemm_swiglu_fwd(hd, dev(w), row_scale=rstd)
            Fd = N // 2

            def sw(r):
                t = unleave(R.bfr(r), Fd)
                return R.bfr(t[:, :Fd] * torch.sigmoid(t[:, :Fd])) * t[:, Fd:]
            outs = {"gate_up": (gu, ref64, ref32, 1), "act": (act, sw(ref64), sw(ref32), 3)}
        for oname, (got, r64, r32, r) in outs.items():
            y, e = R.group_err(r32, r64, gr), R.group_err(got, r64, gr)
            for g in e:
                parity.check(f"regime folded {name} {oname}[{g}]", e[g] if math.isfinite(e[g]) else 1e30, R.bound(R.out_spec(r=r), y[g]))


# ------------------------------------------------------------------------------------------------ activations
def test_swiglu_regimes(ops):
    """act: r = 2 (elementwise.hip:53, bf16(silu) then the product); dgate, dup: r = 1 (elementwise.hip:74-75).  Both layouts."""
    inp = R.swiglu_inputs()
    Fd = inp.Fd
    gu = torch.cat([inp.gate, inp.up], 1)
    for il in (True, False):
        g_in = dev(ileave(gu, Fd) if il else gu)
        act = ops.swiglu_fwd(g_in, interleaved=il)
        dgu = ops.swiglu_bwd(dev(inp.dact), g_in, interleaved=il)
        dgu = unleave(dgu, Fd) if il else dgu
        R.check_all(f"swiglu {'interleaved' if il else 'halves'}", R.evaluate(R.SWIGLU, inp, dict(act=act, dgate=dgu[:, :Fd], dup=dgu[:, Fd:])))


@pytest.mark.parametrize("kind", [R.ACT_GELU, R.ACT_RELU])
def test_act_regimes(ops, kind):
    """y, dx: r = 1 (elementwise.hip:91, :105)"""
    inp = R.act_inputs(kind)
    y, dx = ops.act_fwd(dev(inp.x), kind), ops.act_bwd(dev(inp.dy), dev(inp.x), kind)
    R.check_all(f"act kind={kind}", R.evaluate(R.ACT, inp, dict(y=y, dx=dx)))


def _onehot(M, K):
    x = torch.zeros(M, K)
    x[torch.arange(M), torch.arange(M) % K] = 1.0
    return x.to(BF)


@pytest.mark.parametrize("M,N,K,force", [(64, 128, 64, 0), (256, 256, 128, 7), (256, 256, 128, 14)])
@pytest.mark.parametrize("epi", [R.ACT_GELU, R.ACT_QUICK_GELU, R.ACT_RELU])
def test_gemm_activation_epilogue_regimes(ops, M, N, K, force, epi):
    """One-hot activation rows (x[m, m % K] = 1) make the accumulator equal a chosen weight entry exactly, so the GEMM's activation epilogue sees
    the value grid: out = bf16(act(bf16(acc))) with acc exactly bf16: r = 1."""
    inp = R.act_inputs(epi, Fd=N)
    w = inp.x[torch.arange(K) % 8].t().contiguous()              # w[n, k] = grid pattern row k % 8, column n
    out = ops.gemm(dev(_onehot(M, K)), dev(w), epi=epi, force_generic=force)
    R.check_all(f"gemm epi={epi} {M}x{N}x{K} force={force}", R.evaluate(R.ACT, inp, dict(y=out[:8])))      # row m holds pattern row (m % K) % 8 = m % 8
    assert torch.equal(out.view(M // 8, 8, N), out.view(M // 8, 8, N)[:1].expand(M // 8, 8, N))


@pytest.mark.parametrize("M,Fd,K", [(256, 256, 64), (4096, 3072, 256)])
def test_gemm_swiglu_fused_regimes(ops, M, Fd, K):
    """The fused SwiGLU epilogues on the value grid: (256, 256, 64) routes to the 8-phase kernel, (4096, 3072, 256) to the one-wave-per-SIMD
    kernel ((M / 256) (Fd / 256) >= 192).  Forward: one-hot rows put the grid into gate_up exactly: act r = 2.  Backward: gate_up is an input,
    d_act = dy @ w_down^T with one-hot dy is exact: dgate, dup r = 1 (gemm.hip:348 / :728)."""
    inp = R.swiglu_inputs(Fd=Fd)
    gu_pat = ileave(torch.cat([inp.gate, inp.up], 1), Fd)                     # [8, 2 Fd]
    x = dev(_onehot(M, K))
    w_gu = dev(gu_pat[torch.arange(K) % 8].t().contiguous())                  # [2 Fd, K], already interleaved
    gu, act = ops.gemm_swiglu_fwd(x, w_gu)
    assert torch.equal(gu.view(M // 8, 8, 2 * Fd), dev(gu_pat)[None].expand(M // 8, 8, 2 * Fd))
    R.check_all(f"gemm_swiglu_fwd {M}x{Fd}x{K}", R.evaluate(R.SWIGLU, inp, dict(act=act[:8])))
    assert torch.equal(act.view(M // 8, 8, Fd), act[:8][None].expand(M // 8, 8, Fd))
    w_down_T = dev(inp.dact[torch.arange(K) % 8].t().contiguous())            # [Fd, K]: d_act[m, f] = dact pattern row m % 8
    dgu = ops.gemm_swiglu_bwd(x, w_down_T, gu.contiguous())
    d8 = unleave(dgu[:8], Fd)
    R.check_all(f"gemm_swiglu_bwd {M}x{Fd}x{K}", R.evaluate(R.SWIGLU, inp, dict(dgate=d8[:, :Fd], dup=d8[:, Fd:])))
    assert torch.equal(dgu.view(M // 8, 8, 2 * Fd), dgu[:8][None].expand(M // 8, 8, 2 * Fd))


@pytest.mark.parametrize("il", [True, False])
def test_decode_gemm_swiglu_epilogue_regimes(ops, il):
    """vp_decode_gemm's SwiGLU epilogue (decode.hip's dg_store: bf16(bf16(silu(bf16(gate))) * bf16(up))) with one-hot A rows: r = 2."""
    inp = R.swiglu_inputs()
    Fd, K, M = inp.Fd, 64, 8
    pat = torch.cat([inp.gate, inp.up], 1)
    pat = ileave(pat, Fd) if il else pat
    w = dev(pat[torch.arange(K) % 8].t().contiguous())                         # [2 Fd, K]
    got = ops.decode_gemm(dev(_onehot(M, K)), w, epi=ops.EPI_SWIGLU_IL if il else ops.EPI_SWIGLU_HALVES)
    R.check_all(f"decode_gemm swiglu {'il' if il else 'halves'}", R.evaluate(R.SWIGLU, inp, dict(act=got)))


# ------------------------------------------------------------------------------------------------ cross entropy
CE_VOCABS = [1000, 1003, 32064, 50272, 128256, 131080]      # NCH 8 short, fallback with scalar tail, NCH 8, NCH 16, NCH 32, fallback by size


def _ce_buffers(inp, pad=8):
    """the logits as a column view of a wider sentinel-filled buffer (ld > V, ld % 8 == 0)"""
    rows, V = inp.logits.shape
    ld = (V + 7) // 8 * 8 + pad
    buf = torch.full((rows, ld), 7.0, dtype=BF)
    buf[:, :V] = inp.logits
    return buf.cuda()


@pytest.mark.parametrize("V", CE_VOCABS)
def test_ce_regimes(ops, V):
    """row_loss: fp32, sums V terms, the rows of one call are one group; dlogits: r = 1 (loss.hip:56 / :118), normalised by grad_scale.
    ld > V with the pad columns bit-unchanged, write_grad = 0 leaves the logits bit-unchanged, a call where every row is ignored."""
    inp = R.ce_inputs(V)
    buf = _ce_buffers(inp)
    before = buf.clone()
    lab = dev(inp.labels)
    rl0 = ops.ce_fwd_bwd(buf[:, :V], lab, inp.gs, write_grad=False)
    assert torch.equal(buf, before)
    rl = ops.ce_fwd_bwd(buf[:, :V], lab, inp.gs)
    assert torch.equal(rl, rl0)
    assert torch.equal(buf[:, V:], before[:, V:])
    R.check_all(f"ce V={V}", R.evaluate(R.CE, inp, dict(row_loss=rl, dlogits=buf[:, :V])))
    ign = [i for i, k in enumerate(inp.kinds) if k == "ignored"]
    assert float(rl[ign].abs().max()) == 0.0 and float(buf[ign][:, :V].float().abs().max()) == 0.0
    # every row ignored
    buf2 = before.clone()
    rl2 = ops.ce_fwd_bwd(buf2[:, :V], torch.full_like(lab, -100), inp.gs)
    assert float(rl2.abs().max()) == 0.0 and float(buf2[:, :V].float().abs().max()) == 0.0 and torch.equal(buf2[:, V:], before[:, V:])


_CE_CHILD = """
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import regimes as R
from visper_lm_amd import ops
out = {{}}
for V in (32064, 128256):
    inp = R.ce_inputs(V)
    lg = inp.logits.cuda()
    rl = ops.ce_fwd_bwd(lg, inp.labels.cuda(), inp.gs)
    out[V] = (rl.cpu(), lg.cpu())
torch.save(out, {dst!r})
"""


def test_ce_register_path_bit_identical_to_fallback(ops, tmp_path):
    """loss.hip:69: the register-resident kernels (NCH 8 / 32 here) are bit-identical to the two-pass kernel.  The launcher reads VP_CE_REG once
    per process, so the two-pass side runs in a child process."""
    dst = str(tmp_path / "ce_fallback.pt")
    code = _CE_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), dst=dst)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, VP_CE_REG="0"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    other = torch.load(dst)
    for V in (32064, 128256):
        inp = R.ce_inputs(V)
        lg = dev(inp.logits)
        rl = ops.ce_fwd_bwd(lg, dev(inp.labels), inp.gs)
        assert torch.equal(rl.cpu(), other[V][0]) and torch.equal(lg.cpu(), other[V][1]), V


# ------------------------------------------------------------------------------------------------ embedding loss
EMB_SHAPES = [(3, 1, 0, 40 * 1024, [1., 0., 1.]), (20, 4, 3, 7 * 24, [0.5] * 20)]


def _emb_run(ops, inp):
    ls = None if inp.ls is None else torch.tensor([inp.ls], device="cuda")
    out3, coef = ops.emb_loss_fwd(dev(inp.pred), dev(inp.tg_all), dev(inp.mask), ls, inp.w_con, rank=inp.rank)
    dp = ops.emb_loss_bwd(dev(inp.pred), dev(inp.tg_all), coef, inp.gout, rank=inp.rank)
    return out3, coef, dp


@pytest.mark.parametrize("B,world,rank,D,mask", EMB_SHAPES)
@pytest.mark.parametrize("ls", R.EMB_SCALES)
def test_emb_loss_regimes(ops, B, world, rank, D, mask, ls):
    """logit_scale below / just below / just above / far above the clamp at ln 100, and no contrastive term; local targets all in the quadratic
    zone, all in the linear zone, exactly on the kink.  out3, d loss / d logit_scale (coef[-1]): fp32, sum D terms; dpred: r = 1 (emb_loss.hip:579)."""
    inp = R.emb_inputs(B, world, rank, D, mask, ls)
    out3, coef, dp = _emb_run(ops, inp)
    R.check_all(f"emb_loss B={B} world={world} ls={ls}", R.evaluate(R.EMB, inp, dict(out3=out3, dpred=dp, dls=coef[-1:])))
    if ls is None or ls > R.LN100:
        assert float(coef[-1]) == 0.0                                        # exactly zero above the clamp (emb_loss.hip:136)
    if ls is None:
        assert float(out3[2]) == 0.0


@pytest.mark.parametrize("B,world,rank,D,mask", EMB_SHAPES)
def test_emb_loss_all_zero_mask(ops, B, world, rank, D, mask):
    inp = R.emb_inputs(B, world, rank, D, [0.0] * B, 2.0)
    out3, coef, dp = _emb_run(ops, inp)
    assert float(out3.abs().max()) == 0.0 and float(dp.float().abs().max()) == 0.0
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(coef).all()) and bool(torch.isfinite(dp.float()).all())


def test_emb_loss_multi_launch_mixes_clamped_unclamped_and_scaleless(ops):
    B, world, rank = 8, 2, 1
    heads = [R.emb_inputs(B, world, rank, D, [1., 0., 1., 1., 0.5, 1., 1., 1.], ls, seed=i) for i, (D, ls) in enumerate(((1024, 5.0), (7 * 24, 2.0), (576 * 8, None)))]
    single = [_emb_run(ops, h) for h in heads]
    scales = [None if h.ls is None else torch.tensor([h.ls], device="cuda") for h in heads]
    preds, tgts = [dev(h.pred) for h in heads], [dev(h.tg_all) for h in heads]
    multi = ops.emb_loss_fwd_multi(preds, tgts, [dev(h.mask) for h in heads], scales, [h.w_con for h in heads], rank=rank)
    dps = ops.emb_loss_bwd_multi(preds, tgts, [c for _, c in multi], [h.gout for h in heads], rank=rank)
    for (o1, c1, d1), (o2, c2), d2 in zip(single, multi, dps):
        assert torch.equal(o1, o2) and torch.equal(c1, c2) and torch.equal(d1, d2)
    assert float(multi[0][1][-1]) == 0.0 and float(multi[1][1][-1]) != 0.0 and float(multi[2][1][-1]) == 0.0


# ------------------------------------------------------------------------------------------------ AdamW
def _adamw_run(ops, inp, n, offset, shadow):
    """the kernel on copies of the inputs placed `offset` floats into 16-byte aligned buffers"""
    buf = lambda t: torch.cat([torch.zeros(offset), t]).cuda()[offset:]
    p, g, m, v = buf(inp.p), buf(inp.g), buf(inp.m), buf(inp.v)
    sh = torch.zeros(n + 4, device="cuda", dtype=BF)[4 * (offset > 0):][:n] if shadow else None
    ops.adamw_(p, g, m, v, sh, inp.lr, inp.b1, inp.b2, inp.eps, inp.wd, inp.step, grad_scale=inp.gs)
    return p, m, v, sh


@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_regimes(ops, step, wd):
    """The update p_new - p_old, m and v (fp32, element-wise) per gradient rung, against fp64 AdamW; n = 3 / 5003 / 65536 and views offset by one
    float run the scalar kernel alone, the vector kernel with its n & 3 tail launch, the vector kernel alone and the unaligned scalar path:
    the elements they share agree bit for bit (elementwise.hip:309)."""
    for n in (3, 5003, 1 << 16):
        inp = R.adamw_inputs(n, step, wd)
        p, m, v, sh = _adamw_run(ops, inp, n, 0, True)
        got = dict(dp=p.double().cpu() - inp.p.double(), m=m, v=v)
        R.check_all(f"adamw n={n} step={step} wd={wd}", R.evaluate(R.ADAMW, inp, got))
        assert torch.equal(sh, p.to(BF))
        p1, m1, v1, _ = _adamw_run(ops, inp, n, 1, False)                   # unaligned: scalar kernel, no shadow
        assert torch.equal(p1, p) and torch.equal(m1, m) and torch.equal(v1, v)
        if n > 3:                                                          # the first 3 elements again, as a launch of their own
            p3, m3, v3, _ = _adamw_run(ops, NS(**{**vars(inp), "p": inp.p[:3], "g": inp.g[:3], "m": inp.m[:3], "v": inp.v[:3]}), 3, 0, True)
            assert torch.equal(p3, p[:3]) and torch.equal(m3, m[:3]) and torch.equal(v3, v[:3])


# ------------------------------------------------------------------------------------------------ attention: a late large maximum
def _attn_check(label, got, ref64, ref32, groups, r, norm=None):
    y, e = R.group_err(ref32, ref64, groups, norm), R.group_err(got, ref64, groups, norm)
    for g in e:
        parity.check(f"regime {label}[{g}]", e[g] if math.isfinite(e[g]) else 1e30, R.bound(R.out_spec(r=r), y[g]))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 32])
def test_attention_generic_kernels_late_maximum(ops, D, causal):
    """The generic forward / backward kernels (attention.hip, D = 64 / 32) with the running maximum jumping by ~30 and then ~16 more log2
    units in later key tiles.  The fp64 reference restates no rounding, so every rounding on the path counts half an ulp at most and (2 r - 1) 2^-8
    is generous: o: r = 2 (P as a bf16 MFMA operand, the output); dv: r = 2 (P, the output); dq, dk: r = 4 (P, dS, delta from the bf16 o, the
    output).  Query rows aligned with the large keys / ordinary rows, and the large keys / ordinary keys, are separate groups.  The gradients are
    normalised by the maximum of the whole tensor, not of the group (as CE's d-logits are by grad_scale): in a row whose softmax is saturated,
    dS = P (dP - delta) cancels terms of the size of |dO| |V| to almost nothing, and the honest fp32 reference itself is 85 % away from fp64
    relative to that row's own maximum (its yardstick); the size such an error has to be small against is the ordinary rows' gradient."""
    inp = R.late_max_attention_inputs(D)
    ref64 = R.attention_ref(inp.q, inp.k, inp.v, inp.do, torch.float64, causal)
    ref32 = R.attention_ref(inp.q, inp.k, inp.v, inp.do, torch.float32, causal)
    qd, kd, vd = dev(inp.q), dev(inp.k), dev(inp.v)
    o, lse = ops.attn_fwd(qd, kd, vd, causal)
    dq, dk, dv = ops.attn_bwd(qd, kd, vd, o, lse, dev(inp.do), causal)
    qg = {k: (slice(None), idx) for k, idx in R.row_groups(inp.kinds).items()}
    big = (130, 140, 170, 300, 450)
    kg = {k: (slice(None), idx) for k, idx in R.row_groups(["large" if j in big else "ordinary" for j in range(inp.q.shape[1])]).items()}
    with torch.no_grad():
        sc = (inp.q[0, 511, 0].double() @ inp.k[0, :, 0].double().T) / math.sqrt(D)
        assert float(sc.max() - sc[:128].max()) * 1.4427 > 16.0             # the aligned rows really are dominated by a late key
    for name, got, groups, r in (("o", o, qg, 2), ("dq", dq, qg, 4), ("dk", dk, kg, 4), ("dv", dv, kg, 2)):
        norm = None if name == "o" else float(ref64[name].abs().max())
        _attn_check(f"attn late max D={D} causal={causal} {name}", got, ref64[name], ref32[name], groups, r, norm)


@pytest.mark.parametrize("D", [64, 32])
def test_attention_bias_kernel_late_maximum(ops, D):
    """vp_attn_fwd_bias on the same construction with a per-head bias and a -100 mask block over the early keys of the aligned rows' window: o r = 2."""
    S, H = 512, 4
    inp = R.late_max_attention_inputs(D, S=S, Hq=H, Hkv=H)
    bh = R.randn(H, S, S, seed=180).float() * 2.0
    mask = torch.zeros(1, S, S)
    mask[0, 256:, :128] = -100.0
    bias = bh[None] + mask[:, None]
    ref64 = R.attention_ref(inp.q, inp.k, inp.v, inp.do, torch.float64, False, bias=bias)
    ref32 = R.attention_ref(inp.q, inp.k, inp.v, inp.do, torch.float32, False, bias=bias)
    got = ops.attn_fwd_bias(dev(inp.q), dev(inp.k), dev(inp.v), bias_h=dev(bh).contiguous(), bias_b=dev(mask).contiguous())
    qg = {k: (slice(None), idx) for k, idx in R.row_groups(inp.kinds).items()}
    _attn_check(f"attn bias late max D={D} o", got, ref64["o"], ref32["o"], qg, 2)


# ------------------------------------------------------------------------------------------------ decode kernels
@pytest.mark.parametrize("K", [72, 200, 264, 1000, 4104])
@pytest.mark.parametrize("M", [1, 16])
def test_decode_gemm_k_tails_and_strides(ops, K, M):
    """K tails inside a 64-wide lane group, with and without the norm prologue, row-strided A / W / C (ld > K, ld > N; the pad is not written).
    Bounds of tests/test_generate_gpu.py (fp32 out 5e-6, bf16 out 5e-3, norm prologue 1e-6 against vp_rmsnorm_fwd's rows), per tensor and per row."""
    N = 136
    a_buf, w_buf = dev(R.randn(M, K + 16, seed=230)), dev(R.randn(N, K + 24, seed=231, scale=0.02))
    a, w = a_buf[:, :K], w_buf[:, :K]
    gamma = dev((1 + 0.1 * torch.randn(K, generator=R.gen(232))).to(BF))
    ref = a.float() @ w.float().t()
    rows = {f"row{m}": [m] for m in range(M)}
    c32 = torch.full((M, N + 8), 7.0, device="cuda")
    ops.decode_gemm(a, w, out=c32[:, :N])
    parity.check(f"regime decode_gemm fp32 M={M} K={K}", parity.max_rel(c32[:, :N], ref), 5e-6)
    parity.check(f"regime decode_gemm fp32 M={M} K={K} worst row", max(R.group_err(c32[:, :N], ref.double(), rows).values()), 5e-6)
    assert float((c32[:, N:] - 7.0).abs().max()) == 0.0
    assert torch.equal(c32[:, :N], ops.decode_gemm(a.contiguous(), w.contiguous(), out_f32=True))          # strided == contiguous, bit for bit
    cb = torch.full((M, N + 8), 7.0, device="cuda", dtype=BF)
    ops.decode_gemm(a, w, out=cb[:, :N])
    parity.check(f"regime decode_gemm bf16 M={M} K={K}", parity.max_rel(cb[:, :N], ref), 5e-3)
    assert float((cb[:, N:].float() - 7.0).abs().max()) == 0.0
    xn, _ = ops.rmsnorm_fwd(a.contiguous(), gamma, 1e-5)
    got = ops.decode_gemm(a, w, norm_w=gamma, eps=1e-5, out_f32=True)
    refn = xn.float() @ w.float().t()
    parity.check(f"regime decode_gemm norm prologue M={M} K={K}", parity.max_rel(got, refn), 1e-6)
    parity.check(f"regime decode_gemm norm prologue M={M} K={K} worst row", max(R.group_err(got, refn.double(), rows).values()), 1e-6)


def _ref_decode_attn(q, k, v, lens, window, scale, dt=torch.float64):
    B, Hq, D = q.shape
    Hkv = k.shape[2]
    out = torch.zeros(B, Hq, D, dtype=dt)
    for b in range(B):
        L = int(lens[b])
        lo = max(0, L - window) if window else 0
        if L - lo <= 0:
            continue
        kk = k[b, lo:L].to(dt).repeat_interleave(Hq // Hkv, 1)
        vv = v[b, lo:L].to(dt).repeat_interleave(Hq // Hkv, 1)
        s = torch.einsum("hd,nhd->hn", q[b].to(dt), kk) * scale
        out[b] = torch.einsum("hn,nhd->hd", s.softmax(-1), vv)
    return out


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 1), (64, 8, 1), (64, 4, 4), (32, 16, 2)])
def test_decode_attn_split_boundaries_windows_strides(ops, D, Hq, Hkv):
    """G = Hq / Hkv = 8 and D = 64; lengths 0 / 1 / 511 / 512 / 513 / 1024 / Smax in one batch (length 0: exact zeros); windows 1, 512 and longer
    than any length; q / o rows strided wider than Hq D; the smallest legal nsplit against a larger one.  Per tensor the bound of
    test_generate_gpu.py (1e-3 of the tensor maximum, which the one-key sequence sets); per sequence, relative to that sequence's own maximum, no
    bf16 output can hold 1e-3 (half an ulp is up to 2^-8), so there the computed bound applies: r = 1 (fp32 softmax and P V, decode.hip:341)."""
    lens = [0, 1, 511, 512, 513, 1024, 1536]
    B, Smax = len(lens), max(lens)
    k, v = R.randn(B, Smax, Hkv, D, seed=240), R.randn(B, Smax, Hkv, D, seed=241)
    q = R.randn(B, Hq * D, seed=242)
    q_buf = torch.zeros(B, Hq * D + 64, dtype=BF); q_buf[:, :Hq * D] = q
    kd, vd, qd = dev(k), dev(v), dev(q_buf)[:, :Hq * D]
    kl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    seqs = {f"len{L}": [b] for b, L in enumerate(lens)}
    ns_min = -(-Smax // 512)
    for window in (0, 1, 512, 4096):
        want = _ref_decode_attn(q.view(B, Hq, D), k, v, lens, window, scale)
        o_buf = torch.full((B, Hq * D + 64), 7.0, device="cuda", dtype=BF)
        ops.decode_attn(qd, kd, vd, kl, Hq, window=window, nsplit=ns_min, out=o_buf[:, :Hq * D])
        got = o_buf[:, :Hq * D]
        assert float((o_buf[:, Hq * D:].float() - 7.0).abs().max()) == 0.0
        parity.check(f"regime decode_attn D={D} {Hq}:{Hkv} window={window}", parity.max_rel(got.view(B, Hq, D).cpu(), want), 1e-3)
        errs = R.group_err(got.view(B, Hq, D), want, seqs)
        y = R.group_err(_ref_decode_attn(q.view(B, Hq, D), k, v, lens, window, scale, torch.float32), want, seqs)
        for g, e in errs.items():
            parity.check(f"regime decode_attn D={D} {Hq}:{Hkv} window={window} [{g}]", e if math.isfinite(e) else 1e30,
                         R.bound(R.out_spec(r=1), y[g]) if g != "len0" else 0.0)
        for ns in (ns_min + 5, 64):
            other = ops.decode_attn(qd, kd, vd, kl, Hq, window=window, nsplit=ns)
            parity.check(f"regime decode_attn D={D} {Hq}:{Hkv} window={window} nsplit={ns} vs {ns_min}", parity.max_rel(other.view(B, Hq, D).cpu(), want), 1e-3)
            assert float(other[0].float().abs().max()) == 0.0


def test_decode_rope_append_out_of_range_positions(ops):
    """pos = -1 and pos = Smax: the caches stay bit-unchanged (include/visper_hip.h: rows with pos outside [0, Smax) are not written) and q is
    still written, every element of it."""
    B, Hq, Hkv, D, Smax = 3, 8, 2, 32, 40
    qkv = dev(R.randn(B, (Hq + 2 * Hkv) * D, seed=250))
    cache = torch.full((B, Smax, 2, Hkv * D), 7.0, device="cuda", dtype=BF)
    k4, v4 = cache[:, :, 0].unflatten(-1, (Hkv, D)), cache[:, :, 1].unflatten(-1, (Hkv, D))
    q = torch.full((B, Hq * D), float("nan"), device="cuda", dtype=BF)
    pos = torch.tensor([-1, 17, Smax], device="cuda", dtype=torch.int32)
    cos, sin = ops.rope_tables(64, D, 10000.0, "cuda")
    ops.decode_rope_append(qkv, q, k4, v4, cos, sin, pos, Hq, Hkv, D)
    assert bool(torch.isfinite(q.float()).all())
    want = qkv.clone()
    ops.rope_(want, B, 64, Hq + Hkv, D, cos, sin, pos=torch.tensor([17, 17, 17], device="cuda", dtype=torch.int32))
    assert torch.equal(q[1], want[1, :Hq * D])
    assert torch.equal(cache[1, 17, 0], want[1, Hq * D:(Hq + Hkv) * D]) and torch.equal(cache[1, 17, 1], qkv[1, (Hq + Hkv) * D:])
    cache[1, 17] = 7.0
    assert bool((cache == 7.0).all())                                        # nothing else was touched, for any of the three sequences
