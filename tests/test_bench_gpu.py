"""bench.py as it is run for the headline figure: a plain run prints ONE line with the figure and what the timed steps give for
free, and none of the legs that take runs of their own (those are behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("parity", "cpu_baseline", "reference_default_coupling_interval", "strong_scaling_workload_on_one_gpu",
             "kernel_ms_per_step", "kernel_ms_per_step_note", "tiled_parity", "one_gpu_same_workload")


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_and_nothing_that_needs_runs_of_its_own(tmp_path):
    steps, repeats = 5, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--repeats", str(repeats), "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("floe_steps_per_sec", "floe-steps/s", True, "f64")
    assert (d["steps"], d["warmup"], d["repeats"]) == (steps, 2, repeats)
    assert d["value"] == pytest.approx(d["config"]["n_floes"] / (1e-3 * d["ms_per_step"]), rel=1e-12)
    assert d["ms_per_step_min"] <= d["ms_per_step"] <= d["ms_per_step_max"]
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["kernel_launches_timed"] == steps
    assert not [k for k in FULL_ONLY if k in d]
    assert "measured_copy_ceiling" not in d["roofline"]
    # the outputs of the last timed step are written all the same
    cx = np.load(tmp_path / "out" / "cx.npy")
    assert len(cx) == d["dumped_outputs"]["floes"] > 0 and np.all(np.isfinite(cx))
