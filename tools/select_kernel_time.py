"""Per-launch time of decode_select_kernel by shape and configuration.

  rocprofv3 --kernel-trace --stats -d <dir> -o select -f csv -- python tools/select_kernel_time.py      the launches, in a fixed order
  python tools/select_kernel_time.py --parse <dir>/.../select_kernel_trace.csv --out profiles/decode_select_kernel_time.json

The first form launches, for each (rows, vocabulary, configuration) of CASES, REPS back-to-back calls of ops.decode_select on N(0, sigma^2)
logits (sigma 3: a peaked row; sigma 0.02: a nearly flat row, what a random-init model emits, where top_p 0.9 keeps most of the vocabulary)
and prints a device-event time per call.  The second form reads the trace of that run: the kernel's dispatches in start order are the cases
in order, REPS each; the first of each case is dropped as warm-up."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 21
CONFIGS = {
    "greedy": dict(),
    "sample_T0.8_p0.9": dict(do_sample=True, temperature=0.8, top_p=0.9),
    "sample_T0.8_p0.9_k50_pen1.1": dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=50, repetition_penalty=1.1),
}
CASES = [(R, V, sigma, c) for V in (128256, 32064) for R in (1, 8, 64) for sigma in (3.0, 0.02) for c in CONFIGS]


def launch():
    import torch
    from visper_lm_amd import ops
    assert torch.cuda.is_available(), "select_kernel_time needs a GPU"
    I32 = torch.int32
    for R, V, sigma, c in CASES:
        g = torch.Generator(device="cuda").manual_seed(R + V)
        x = torch.randn(R, V, device="cuda", generator=g) * sigma
        u = torch.rand(R, device="cuda", generator=g)
        tok, fin = torch.zeros(R, device="cuda", dtype=I32), torch.zeros(R, device="cuda", dtype=I32)
        out, col = torch.zeros(R, 1, device="cuda", dtype=I32), torch.zeros(1, device="cuda", dtype=I32)
        seen = torch.zeros(R, (V + 31) // 32, device="cuda", dtype=I32)
        kw = dict(CONFIGS[c], seen=seen, u=u)
        ops.decode_select(x, tok, out, col, fin, **kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS - 1):
            ops.decode_select(x, tok, out, col, fin, **kw)
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(R=R, V=V, sigma=sigma, config=c, event_us_per_call=round(e0.elapsed_time(e1) * 1e3 / (REPS - 1), 2))), flush=True)


def parse(path, out):
    rows = [r for r in csv.DictReader(open(path)) if "decode_select_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == REPS * len(CASES), (len(rows), REPS * len(CASES))
    res = []
    for i, (R, V, sigma, c) in enumerate(CASES):
        d = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * REPS + 1:(i + 1) * REPS])
        res.append(dict(R=R, V=V, sigma=sigma, config=c, calls=len(d), median_us=round(d[len(d) // 2], 2), min_us=round(d[0], 2),
                        max_us=round(d[-1], 2)))
        print(json.dumps(res[-1]))
    if out:
        with open(out, "w") as fh:
            fh.write(json.dumps(dict(kernel="decode_select_kernel", source="rocprofv3 --kernel-trace", cases=res)) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parse", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parse(a.parse, a.out) if a.parse else launch()
