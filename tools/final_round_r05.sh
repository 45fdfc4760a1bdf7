# Round-5 final evidence, one box, in this order (from the repo root; $1 = output directory).
out=${1:-final}
mkdir -p "$out"
python bench.py --full --steps 10 --warmup 3 > $out/bench_default.log 2>&1; tail -1 $out/bench_default.log > $out/r05_bench.json
python bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-probes 2>/dev/null | tail -1 > $out/r05_bench_plain.json
for w in phi3 convnext ift pt6; do python bench.py --full --workload $w --steps 6 --warmup 2 --no-cpu-baseline 2>/dev/null | tail -1 > $out/r05_bench_$w.json; done
python bench.py --steps 6 --warmup 2 --no-cpu-baseline --no-probes --reference-outputs 2>/dev/null | tail -1 > $out/r05_bench_reference_outputs.json
bash tools/profile_round.sh r05f > $out/profile_round.log 2>&1
bash tools/pmc_round.sh r05f > $out/pmc_round.log 2>&1
bash tools/attn_bwd64_clock.sh > $out/attn_clock.log 2>&1
bash tools/attn_kernel_times.sh > $out/attn_kernel_times.log 2>&1
