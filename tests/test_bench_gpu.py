"""bench.py's two kinds of run (GPU): a plain run prints the headline line and nothing that takes a run of its own; `--full` adds the
one-stream schedule, the K11 / shader-clock probes and the CPU baseline after the timed steps.  A shallow debug model keeps both short."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--layers", "2", *extra],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-1500:] + r.stderr[-2500:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    res = _line()
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["unit"] == "images/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert abs(res["value"] - 8 / (res["ms_per_step"] / 1e3)) < 0.01 * res["value"]
    assert "cpu_baseline" not in res and "extras" not in res
    roof = res["roofline"]                                   # priced on the timed steps' own HIP events: part of the plain line
    assert roof["launches_per_step"] > 0
    for k in ("one_stream_schedule", "k11", "clock"):
        assert k not in roof, k


def test_full_run_adds_the_other_legs():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    res = _line("--full")
    roof = res["roofline"]
    for k in ("one_stream_schedule", "k11", "clock"):
        assert k in roof and "error" not in roof[k], (k, roof.get(k))
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["extrapolated"] is False
