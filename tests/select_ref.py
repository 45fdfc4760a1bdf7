"""The contract of vp_decode_select restated in plain torch / numpy on the CPU (include/visper_hip.h): fp32 for the penalty, the temperature
and top-k (the device must reproduce those bits), fp64 for the top-p masses and the sampling CDF (the device's fixed-point masses may differ
from them by DELTA of the row's mass).  test_decode_select_host.py holds it against HF's processors; the GPU tests hold the kernel against it."""
import numpy as np
import torch

DELTA = 2.0 ** -19                                               # the band of the top-p threshold and of a CDF boundary (fraction of the row's mass)


def seen_mask(ids, V):
    """token ids [R, n] -> bool [R, V]"""
    m = torch.zeros(ids.shape[0], V, dtype=torch.bool)
    return m.scatter_(1, ids.long(), True)


def pack_bits(mask):
    """bool [R, V] -> int32 [R, ceil(V / 32)] (bit v % 32 of word v // 32), the kernel's bitmap"""
    R, V = mask.shape
    W = (V + 31) // 32
    m = np.zeros((R, W * 32), np.uint64)
    m[:, :V] = mask.numpy()
    words = (m.reshape(R, W, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def unpack_bits(words, V):
    w = words.cpu().numpy().view(np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return torch.from_numpy(bits.reshape(w.shape[0], -1)[:, :V].astype(bool))


def ref_scores(logits, seen=None, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0):
    """logits fp32 [R, V] (CPU), seen bool [R, V] or None -> dict:
      s       fp32 [R, V]: penalty then temperature (steps 1-2)
      keep    bool: survives top-k (ties kept) and top-p (tail mass of the survivors with s_u <= s_v, ties included, > 1 - top_p; max kept)
      scores  s where kept, -inf elsewhere (step 5)
      band    bool: the tokens top-p may decide either way: the fp64 tail mass within DELTA of 1 - top_p, or an exact tie whose members
              straddle it when taken one by one (HF's sort order decides those); never the row maximum
      tail    fp64 [R, V]: that tail mass as a fraction (nan where top-p did not look)"""
    x = logits.clone()
    if seen is not None and penalty != 1.0:
        th = torch.tensor(penalty, dtype=torch.float32)
        x = torch.where(seen, torch.where(x < 0, x * th, x / th), x)
    s = x / torch.tensor(temperature, dtype=torch.float32)
    R, V = s.shape
    keep = torch.ones(R, V, dtype=torch.bool)
    if top_k > 0:
        k = min(max(int(top_k), 1), V)
        kth = torch.topk(s, k, dim=-1)[0][:, -1:]
        keep = ~(s < kth)
    band = torch.zeros(R, V, dtype=torch.bool)
    tail = torch.full((R, V), float("nan"), dtype=torch.float64)
    if top_p < 1.0:
        thr = 1.0 - float(np.float32(top_p))
        sn, kn = s.double().numpy(), keep.numpy().copy()
        for r in range(R):
            idx = np.flatnonzero(kn[r])
            v = sn[r, idx]
            m = np.exp(v - v.max())
            order = np.argsort(v, kind="stable")
            vs, cs = v[order], np.cumsum(m[order])
            hi = np.searchsorted(vs, v, side="right") - 1        # the last survivor with a value <= v: ties included
            lo = np.searchsorted(vs, v, side="left")             # the first survivor with the value v
            incl = cs[hi] / cs[-1]
            lower = (np.where(lo > 0, cs[np.maximum(lo - 1, 0)], 0.0) + m) / cs[-1]
            top = v == v.max()
            kn[r, idx] = (incl > thr) | top
            band[r, idx] = torch.from_numpy((lower <= thr + DELTA) & (incl >= thr - DELTA) & ~top)
            tail[r, idx] = torch.from_numpy(incl)
        keep = torch.from_numpy(kn)
    return dict(s=s, keep=keep, scores=s.masked_fill(~keep, float("-inf")), band=band, tail=tail)


def ref_greedy(scores):
    return torch.argmax(scores, dim=-1)


def ref_cdf(scores_row):
    """fp32 [V] processed scores -> (idx, lo, hi): the kept tokens of nonzero mass in ascending index order and their fp64 CDF intervals"""
    sc = scores_row.double().numpy()
    idx = np.flatnonzero(np.isfinite(sc) | (sc == np.inf))
    m = np.exp(sc[idx] - sc[idx].max())
    idx, m = idx[m > 0], m[m > 0]
    c = np.cumsum(m) / m.sum()
    return idx, np.concatenate([[0.0], c[:-1]]), c


def accepted(scores_row, u, delta=DELTA):
    """the tokens whose CDF interval, widened by delta, contains u"""
    idx, lo, hi = ref_cdf(scores_row)
    return idx[(lo - delta <= u) & (u < hi + delta)]
