"""The D = 128 / 96 attention kernels (attn_fwd128m_kernel of csrc/attention_d128.h, attn_bwd_dq64w_kernel / attn_bwd_dkdv64w_kernel of
csrc/attention_bwd64.h and, in child processes, the 16-row forward behind VP_ATTN_FWDM=0 and the DMA-ring pair behind VP_ATTN_BWD64=0 / 2) at
the edges of their 256-row / 256-key blocks: lse against fp64, exact masks, query rows that see no key, guard bands round every tensor.
tests/ATTENTION_D128.md maps each case of helpers_ref.D128_CASES to the path it enters; tests/test_helpers_host.py proves on the CPU that the
comparisons made here (helpers_ref.d128_compare) reject every mutant and that the bit equality of the exact pass is within reach of fp32.

Layout, every case: q, k, v, do, o, lse, dq, dk, dv are views inside allocations filled with the sentinel of tests/test_gemm_layouts_gpu.py, row
strides 8 elements above H * D, 64 guard rows (lse: 64 floats) before and after.  After the calls every byte outside the views holds the sentinel,
the inputs are bit-unchanged, every element inside the output views has been written.
  random   N(0, 1) inputs: lse (absolute, fp32 sum form, n = Skv) and o / dq / dk / dv (r = 2 / 4 / 4 / 2) against fp64 per 256-row / 256-key block
           through parity.check; exact zeros in dk / dv at keys >= kv_len and in o / dq on empty rows, lse = -1e30 there; everything finite;
           causal cases: vp_attn_bwd_rope bit-identical to vp_attn_bwd + vp_rope(inverse); offset-across-blocks: bit-equal to the contiguous call
  exact    q = 0, one-hot v: round(2^lse) = the number of visible keys of every row, o bit-equal to bf16(cnt / n); dk exactly zero, dq / dv bounded"""
import os
import subprocess
import sys
import time

import pytest
import torch

import gemm_cases as G
import helpers_ref as HR
import parity

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GUARD, PADC = 64, 8
VARIANT = " ".join(f"{k[8:]}={os.environ[k]}" for k in ("VP_ATTN_FWDM", "VP_ATTN_BWD64") if k in os.environ) or "default"
CASES = [(n, D) for n in HR.D128_CASES for D in HR.D128_DIMS]
IDS = [f"{n}-{D}" for n, D in CASES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visper_lm_amd import ops as o
    return o


class Guarded:
    """a view of `shape` / `strides` (elements) `offset` elements into a sentinel-filled device allocation of n elements"""

    def __init__(self, n, shape, strides, offset, dtype, fill=None):
        self.it, self.bits = G.SENT[dtype]
        self.buf = torch.full((n,), self.bits, dtype=self.it, device="cuda").view(dtype)
        self.geom = (shape, strides, offset)
        self.view = torch.as_strided(self.buf, *self.geom)
        self.before = None
        if fill is not None:
            self.view.copy_(fill)
            self.before = self.buf.clone()

    @classmethod
    def bshd(cls, B, S, H, D, fill=None):
        ts = H * D + PADC
        return cls((2 * GUARD + B * S) * ts, (B, S, H, D), (S * ts, ts, D, 1), GUARD * ts, BF, fill)

    @classmethod
    def stats(cls, B, H, S):
        return cls(2 * GUARD + B * H * S, (B, H, S), (H * S, S, 1), GUARD, F32)

    def problems(self, what):
        flat = self.buf.view(self.it)
        if self.before is not None:
            return [] if torch.equal(flat, self.before.view(self.it)) else [f"{what}: the input allocation changed"]
        inside = torch.zeros(flat.numel(), dtype=torch.bool, device="cuda")
        torch.as_strided(inside, *self.geom).fill_(True)
        bad = []
        if not bool((flat[~inside] == self.bits).all()):
            bad.append(f"{what}: a sentinel element outside the view changed")
        if bool((flat[inside] == self.bits).any()):
            bad.append(f"{what}: an element of the view was not written")
        return bad


def forward(ops, q, k, v, o, lse, kv, causal, window):
    """ops.attn_fwd with lse as a destination"""
    from visper_lm_amd import _lib
    B, Sq, Hq, D = q.shape
    _, Skv, Hkv, _ = k.shape
    s = ops._bshd
    _lib.call("vp_attn_fwd", B, Hq, Hkv, Sq, Skv, D, ops._p(q), *s(q), ops._p(k), *s(k), ops._p(v), *s(v), ops._p(o), *s(o), ops._p(lse), ops._p(kv),
              1 if causal else 0, window, 1.0 / D ** 0.5, ops._stream())


def run(ops, name, D, kind):
    """forward + backward of one case inside guarded allocations -> (outputs on the CPU, the device inputs, layout problems)"""
    B, Hq, Hkv, Sq, Skv, causal, window, kvl = HR.D128_CASES[name]
    inp = HR.d128_refs(name, D, kind)[0]
    kv = None if kvl is None else torch.tensor(kvl, dtype=torch.int32, device="cuda")
    gi = {n: Guarded.bshd(*t.shape, fill=t.cuda()) for n, t in inp.items()}
    go = dict(o=Guarded.bshd(B, Sq, Hq, D), lse=Guarded.stats(B, Hq, Sq), dq=Guarded.bshd(B, Sq, Hq, D), dk=Guarded.bshd(B, Skv, Hkv, D),
              dv=Guarded.bshd(B, Skv, Hkv, D))
    q, k, v, do = (gi[n].view for n in ("q", "k", "v", "do"))
    forward(ops, q, k, v, go["o"].view, go["lse"].view, kv, causal, window)
    ops.attn_bwd(q, k, v, go["o"].view, go["lse"].view, do, causal, window=window, kv_len=kv, dq=go["dq"].view, dk=go["dk"].view, dv=go["dv"].view)
    torch.cuda.synchronize()
    bad = [p for n, g in {**gi, **go}.items() for p in g.problems(n)]
    return {n: g.view.cpu() for n, g in go.items()}, (q, k, v, do, kv), bad


def check(name, D, kind, got, layout):
    res, bad = HR.d128_compare(name, D, kind, got)
    fails = list(layout) + bad
    for label, (e, b) in res.items():
        try:
            parity.check(f"attn_d128 {VARIANT} {name} D={D} {kind} {label}", e if e == e and e != float("inf") else 1e30, b)
        except AssertionError as ex:
            fails.append(str(ex))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,D", CASES, ids=IDS)
def test_d128_random(ops, name, D):
    B, Hq, Hkv, Sq, Skv, causal, window, kvl = HR.D128_CASES[name]
    got, (q, k, v, do, kv), layout = run(ops, name, D, "random")
    check(name, D, "random", got, layout)
    o, lse = got["o"].cuda(), got["lse"].cuda()
    if name == "offset-across-blocks":                   # the same case contiguous, every tensor its own allocation: bit-equal in all five outputs
        qc, kc, vc, dc = (t.contiguous() for t in (q, k, v, do))
        oc, lsec = ops.attn_fwd(qc, kc, vc, causal, window=window, kv_len=kv)
        twin = dict(zip(("dq", "dk", "dv"), ops.attn_bwd(qc, kc, vc, oc, lsec, dc, causal, window=window, kv_len=kv)), o=oc, lse=lsec)
        assert not [n for n, t in twin.items() if not HR.exact(t, got[n])]
    if causal:                                           # the header's claim: vp_attn_bwd_rope == vp_attn_bwd, then vp_rope(inverse = 1) on dq and dk
        cos_t, sin_t = ops.rope_tables(Skv, D, 500000.0 if D == 128 else 10000.0, "cuda")
        dq, dk, dv = (got[n].cuda().contiguous() for n in ("dq", "dk", "dv"))
        pos = (torch.arange(Sq, device="cuda", dtype=torch.int32) + (Skv - Sq)).repeat(B).contiguous()      # a query's position: its row + Skv - Sq
        ops.rope_(dq.view(B * Sq, Hq * D), B * Sq, Skv, Hq, D, cos_t, sin_t, pos=pos, inverse=True)
        ops.rope_(dk.view(B * Skv, Hkv * D), B * Skv, Skv, Hkv, D, cos_t, sin_t, inverse=True)
        fq, fk, fv = ops.attn_bwd(q, k, v, o, lse, do, causal, window=window, kv_len=kv, rope=(cos_t, sin_t))
        assert HR.exact(fq, dq) and HR.exact(fk, dk) and HR.exact(fv, dv)


@pytest.mark.parametrize("name,D", CASES, ids=IDS)
def test_d128_exact(ops, name, D):
    got, _, layout = run(ops, name, D, "exact")
    check(name, D, "exact", got, layout)


@pytest.mark.parametrize("env", [{"VP_ATTN_FWDM": "0"}, {"VP_ATTN_BWD64": "0"}, {"VP_ATTN_BWD64": "2"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_d128_fallback_kernels(env):
    """The 16-row forward (VP_ATTN_FWDM=0), the DMA-ring dQ + dK/dV pair (VP_ATTN_BWD64=0) and the DMA-ring dQ in front of the one-wave dK/dV
    (VP_ATTN_BWD64=2) through the random and the exact pass of this file.  The launchers read their switches once per process: a child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_d128_random or test_d128_exact"],
                       capture_output=True, text=True, timeout=900, cwd=root, env=dict(os.environ, **env))
    parity.log(f"attn_d128 child {env} seconds", time.time() - t0)
    assert r.returncode == 0 and " passed" in r.stdout, (env, r.stdout[-3000:], r.stderr[-500:])
