"""The generic attention kernels (D = 32 / 64: attn_fwd_kernel, attn_delta_kernel, attn_bwd_dkdv_kernel, attn_bwd_dq_kernel of
csrc/attention.hip), which produce the gradients of the resampler heads, on the mask branches, the GQA loop, the head permutation and the
strided layouts that tests/test_kernels_gpu.py enters only at D = 128 / 96.  Forward and backward against `attn_ref` in fp32 on the CPU with
the comparisons test_attention_d128_dma_kernels_edges applies to the same operation (tests/helpers_ref.py attention_failures; the CPU proof
that they reject a dK / dV pass that ignores kv_len and a window that is off by one is tests/test_helpers_host.py).

Not tested: kv_len = 0 and causal with Sq > Skv; include/visper_hip.h does not define them for the training kernels."""
import pytest
import torch

import helpers_ref as HR
from test_kernels_gpu import attn_ref, close, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops as o
    return o


def dev(t):
    return t.cuda()


def _reference(q, k, v, do, causal, kvl, window):
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    o = attn_ref(qr, kr, vr, causal, kv_len=kvl, window=window)
    o.backward(do.float())
    return dict(o=o.detach(), dq=qr.grad, dk=kr.grad, dv=vr.grad)


EDGES = [   # the seven edge shapes of test_attention_d128_dma_kernels_edges
    (2, 4, 2, 77, 77, True, 0, None),            # ragged, GQA (rep = 2)
    (1, 4, 4, 200, 333, False, 0, None),         # cross attention, Skv != Sq
    (1, 4, 1, 130, 190, True, 0, None),          # causal with offset Skv - Sq, 4 q heads per kv head
    (2, 2, 2, 161, 161, True, 50, None),         # sliding window: qend trimming in dK / dV
    (2, 4, 2, 96, 96, True, 0, [96, 41]),        # right-padded batch: keys >= kv_len masked, their dK / dV exactly zero
    (1, 2, 2, 31, 31, True, 0, None),            # shorter than one tile
    (1, 2, 1, 257, 257, False, 0, [200]),        # non-causal + padding, one key past two 128-key blocks
]
PERMUTED = [   # Hq % 8 == 0: the XCD head permutation of the forward and dQ kernels, together with GQA
    (1, 8, 2, 140, 140, True, 0, None),
    (1, 16, 4, 140, 140, True, 0, None),
]


@pytest.mark.parametrize("D", [64, 32])
@pytest.mark.parametrize("B,Hq,Hkv,Sq,Skv,causal,window,kvl", EDGES + PERMUTED)
def test_attn_generic_masks_gqa_views(ops, B, Hq, Hkv, Sq, Skv, causal, window, kvl, D):
    q, k, v, do = rnd(B, Sq, Hq, D, seed=81), rnd(B, Skv, Hkv, D, seed=82), rnd(B, Skv, Hkv, D, seed=83), rnd(B, Sq, Hq, D, seed=84)
    ref = _reference(q, k, v, do, causal, kvl, window)
    kv = None if kvl is None else torch.tensor(kvl, dtype=torch.int32).cuda()
    qd, kd, vd = dev(q), dev(k), dev(v)
    o, lse = ops.attn_fwd(qd, kd, vd, causal, window=window, kv_len=kv)
    dq, dk, dv = ops.attn_bwd(qd, kd, vd, o, lse, dev(do), causal, window=window, kv_len=kv)
    got = dict(o=o.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())
    assert not HR.attention_failures(got, ref, kvl, close)
    if (B, Hq, Hkv, Sq) == (2, 4, 2, 96):
        # the same case with the outputs as strided views of one NaN-filled buffer (fused-QKV gradient layout): every element is written
        dqkv = torch.full((B, Sq, (Hq + 2 * Hkv) * D), float("nan"), device="cuda", dtype=BF)
        a = dqkv[..., :Hq * D].unflatten(-1, (Hq, D))
        b_ = dqkv[..., Hq * D:(Hq + Hkv) * D].unflatten(-1, (Hkv, D))
        c = dqkv[..., (Hq + Hkv) * D:].unflatten(-1, (Hkv, D))
        obuf = torch.full((B, Sq, Hq * D + 8), float("nan"), device="cuda", dtype=BF)
        o2, lse2 = ops.attn_fwd(qd, kd, vd, causal, window=window, kv_len=kv, out=obuf[..., :Hq * D].unflatten(-1, (Hq, D)))
        ops.attn_bwd(qd, kd, vd, o2, lse2, dev(do), causal, window=window, kv_len=kv, dq=a, dk=b_, dv=c)
        assert torch.isfinite(dqkv.float()).all() and torch.isfinite(o2.float()).all()
        assert torch.isnan(obuf[..., Hq * D:].float()).all()
        assert torch.equal(o2, o) and torch.equal(lse2, lse) and torch.equal(a, dq) and torch.equal(b_, dk) and torch.equal(c, dv)


@pytest.mark.parametrize("D", [64, 32])
@pytest.mark.parametrize("nq", [8, 70])
def test_attn_generic_resampler_layout(ops, nq, D):
    """The engine's resampler block (Engine._head_bwd): q = the latent rows n: of a fused [B, n + nq, 3 H D] projection, k / v = all of its rows;
    dq / dk / dv are views of ONE zero-filled buffer of the same shape whose first n dq rows no kernel may touch.  Non-causal, Sq = nq != Skv."""
    B, H, n = 2, 4, 130
    T, inner = n + nq, H * D
    qkv = rnd(B, T, 3 * inner, seed=90)
    do = rnd(B, nq, H, D, seed=91)
    q, k, v = qkv[:, n:, :inner].unflatten(-1, (H, D)), qkv[..., inner:2 * inner].unflatten(-1, (H, D)), qkv[..., 2 * inner:].unflatten(-1, (H, D))
    ref = _reference(q, k, v, do, False, None, 0)
    d = dev(qkv)
    qd, kd, vd = d[:, n:, :inner].unflatten(-1, (H, D)), d[..., inner:2 * inner].unflatten(-1, (H, D)), d[..., 2 * inner:].unflatten(-1, (H, D))
    o, lse = ops.attn_fwd(qd, kd, vd, False)
    dQKV = torch.zeros(B, T, 3 * inner, device="cuda", dtype=BF)
    dq, dk, dv = dQKV[:, n:, :inner].unflatten(-1, (H, D)), dQKV[..., inner:2 * inner].unflatten(-1, (H, D)), dQKV[..., 2 * inner:].unflatten(-1, (H, D))
    ops.attn_bwd(qd, kd, vd, o, lse, dev(do), False, dq=dq, dk=dk, dv=dv)
    assert not HR.attention_failures(dict(o=o.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu()), ref, None, close)
    assert float(dQKV[:, :n, :inner].float().abs().max()) == 0.0              # the token rows carry no queries: their dq stays zero
    assert torch.isfinite(dQKV.float()).all()
    # bit for bit what the contiguous call gives
    qc, kc, vc = qd.contiguous(), kd.contiguous(), vd.contiguous()
    oc, lsec = ops.attn_fwd(qc, kc, vc, False)
    dqc, dkc, dvc = ops.attn_bwd(qc, kc, vc, oc, lsec, dev(do), False)
    assert torch.equal(oc, o) and torch.equal(lsec, lse) and torch.equal(dqc, dq) and torch.equal(dkc, dk) and torch.equal(dvc, dv)
