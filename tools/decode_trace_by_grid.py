"""The decode kernels of a `rocprofv3 --kernel-trace --output-format csv` run grouped by (kernel, grid, workgroup): calls, average
microseconds, total milliseconds.  Writes a CSV (profiles/decode_kernel_stats_llama3_wide_*.csv).

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/decode_bench.py --model llama3 --wide --profile --batches 64 --new 6
  python tools/decode_trace_by_grid.py <dir> profiles/decode_kernel_stats_llama3_wide_bf16.csv
"""
import csv
import glob
import sys


def main(d, out):
    agg = {}
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0]
            if "decode" not in name and "gather" not in name and "add_i32" not in name:      # the prefill's kernels are left out
                continue
            key = (name, r["Grid_Size_X"], r["Grid_Size_Y"], r["Workgroup_Size_X"])
            n, t = agg.get(key, (0, 0))
            agg[key] = (n + 1, t + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(out, "w") as fh:
        fh.write("kernel,grid_x,grid_y,workgroup_x,calls,avg_us,total_ms\n")
        for k, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            fh.write(",".join(['"%s"' % k[0], k[1], k[2], k[3], str(n), "%.2f" % (t / n / 1e3), "%.3f" % (t / 1e6)]) + "\n")
    print(open(out).read())


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
