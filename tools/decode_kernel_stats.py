"""Per-kernel, per-grid statistics of a `rocprofv3 --kernel-trace` database of tools/decode_bench.py --profile, with the decode kernels'
algorithmic bytes over kernel time against 8 TB/s.  Writes a CSV.

  python tools/decode_kernel_stats.py <run_results.db> --model llama3 --out profiles/decode_kernel_stats_llama3.csv
"""
import argparse
import csv
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(model):
    """grid (x, y) of decode_gemm_kernel at M rows -> (name, N, K) for the model's decoder shapes and lm_head."""
    from visper_lm_amd.config import llama3_8b, phi3_mini
    cfg = llama3_8b() if model == "llama3" else phi3_mini()
    H, I = cfg.hidden_size, cfg.intermediate_size
    nqkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim
    return cfg, [("qkv", nqkv, H, False), ("wo", H, cfg.num_attention_heads * cfg.head_dim, False), ("gate_up", 2 * I, H, True),
                 ("down", H, I, False), ("lm_head", cfg.vocab_size, H, False)]


def ksplit_w8(N, K, swiglu, query="vp_decode_gemm_w8_workspace_bytes"):
    """(tiles, split-K factor) of decode_gemm_w8_kernel (decode_gemm_w4_kernel with its own query), asked of the library itself: the
    workspace is ks fp32 slabs [M, N] (none: ks = 1)"""
    from visper_lm_amd import _lib
    nb = int(_lib.raw(query, 1, N, K, 4 if swiglu else 0))
    # M = 1: ks = bytes / (4 N).  This holds only while the workspace is EXACTLY ks slabs of M x N fp32 (include/visper_hip.h); a header, padding
    # or a different slab type in the library would make the rows below attach to the wrong grid (they would then simply find no match)
    assert nb % (4 * N) == 0, (N, K, nb)
    return (N // 16 if swiglu else (N + 15) // 16), max(1, nb // (4 * N))


def ksplit(N, K, swiglu):
    tiles = N // 16 if swiglu else (N + 15) // 16
    ks = 1
    while tiles * ks < 512 and ks < 8 and K % (2 * ks * 256) == 0:
        ks *= 2
    return tiles, ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--model", default="llama3")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    cfg, shp = shapes(a.model)
    by_grid = {}
    for name, N, K, sw in shp:                                   # shapes that launch the same grid (wo and down: 256 tiles, split-K 2) share a row
        tiles, ks = ksplit(N, K, sw)
        by_grid.setdefault((tiles * 256, ks), []).append((name, N, K))
    by_grid8 = {}                                                 # the FP8 weight-only kernel: its own split rule, one byte per weight
    for name, N, K, sw in shp:
        tiles, ks = ksplit_w8(N, K, sw)
        by_grid8.setdefault((tiles * 256, ks), []).append((name, N, K))
    by_grid4 = {}                                                 # the MXFP4 weight-only kernel: half a byte per weight + a scale byte per 32
    for name, N, K, sw in shp:
        tiles, ks = ksplit_w8(N, K, sw, "vp_decode_gemm_w4_workspace_bytes")
        by_grid4.setdefault((tiles * 256, ks), []).append((name, N, K))
    c = sqlite3.connect(a.db)
    rows = c.execute("select name, grid_x, grid_y, grid_z, duration from kernels").fetchall()
    agg = {}
    for name, gx, gy, gz, dur in rows:
        short = name.split("(")[0]
        key = (short, gx, gy, gz)
        n, t = agg.get(key, (0, 0))
        agg[key] = (n + 1, t + dur)
    out = []
    for (short, gx, gy, gz), (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        avg_us = t / n / 1e3
        shape, gbps_share, nbytes = "", "", ""
        if "decode_gemm_kernel" in short and (gx, gy) in by_grid:
            grp = by_grid[(gx, gy)]
            # M = 1 and 8 (the --profile run's two batch sizes) share a grid; bytes = the weights (A and C add < 0.5 %), averaged over the
            # shapes of a shared grid (each is launched equally often per token)
            nbytes = sum(N * K * 2 for _, N, K in grp) // len(grp)
            shape = " + ".join(f"{nm} N={N} K={K}" for nm, N, K in grp) + f" (split-K {gy})"
            gbps_share = round(nbytes / (avg_us * 1e-6) / 8e12, 3)
        if "decode_gemm_w8_kernel" in short and (gx, gy) in by_grid8:
            grp = by_grid8[(gx, gy)]
            nbytes = sum(N * K for _, N, K in grp) // len(grp)
            shape = " + ".join(f"{nm} N={N} K={K}" for nm, N, K in grp) + f" (fp8, split-K {gy})"
            gbps_share = round(nbytes / (avg_us * 1e-6) / 8e12, 3)
        if "decode_gemm_w4_kernel" in short and (gx, gy) in by_grid4:
            grp = by_grid4[(gx, gy)]
            nbytes = sum(N * K // 2 + N * K // 32 for _, N, K in grp) // len(grp)
            shape = " + ".join(f"{nm} N={N} K={K}" for nm, N, K in grp) + f" (mxfp4, split-K {gy})"
            gbps_share = round(nbytes / (avg_us * 1e-6) / 8e12, 3)
        out.append(dict(kernel=short, grid=f"{gx}x{gy}x{gz}", calls=n, total_ms=round(t / 1e6, 3), avg_us=round(avg_us, 2), shape=shape,
                        weight_bytes=nbytes, share_of_8TBps=gbps_share))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=list(out[0]))
        w.writeheader()
        w.writerows(out)
    for r in out[:25]:
        print(r)


if __name__ == "__main__":
    main()
