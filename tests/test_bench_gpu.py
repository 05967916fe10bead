"""bench.py end to end on a small patch: what a plain run leaves out and what --full adds to the one JSON line."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(*extra):
    """-> (the line, stderr, seconds from start to exit of the whole process)."""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--size", "32", *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines                           # the contract: ONE JSON line on stdout
    return json.loads(lines[0]), r.stderr, wall


def check_headline(d):
    assert all(k in d for k in HEADLINE_KEYS)
    assert d["unit"] == "voxels/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["launch"] == "hipgraph"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(32 ** 3 / (d["ms_per_step"] * 1e-3), rel=1e-9)


@pytest.mark.gpu
def test_plain_run_is_the_headline_only(tmp_path):
    d, err, wall = run_bench("--dump-outputs", str(tmp_path))
    check_headline(d)
    assert "cpu_baseline" not in d and d["kernels"] == {} and d["roofline"] is None
    assert d["config"]["comm_ms_exposed"] is None
    assert "cpu baseline" not in err                        # the oracle never ran
    # a plain run may spend at most 30 s outside its warm-up and timed steps, start to exit, first-step costs included
    outside = wall - (d["steps"] + d["warmup"]) * d["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s in all, {outside:.2f} s outside its steps")
    assert outside <= 30.0
    # --dump-outputs still writes what the last timed step left: loss terms, parameters, buffers
    names = sorted(os.listdir(tmp_path))
    assert "loss_terms.npy" in names
    assert any(n.startswith("param.") for n in names) and any(n.startswith("buffer.") for n in names)


@pytest.mark.gpu
def test_full_run_adds_every_leg():
    d, _, _ = run_bench("--full")
    check_headline(d)
    assert d["kernels"] and d["roofline"]["kernel"] in d["kernels"]
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and "checkpoint_default" in cb
    assert cb["dice_vs_cpu_ref"] > 0.999 and cb["max_rel_output_err"] < 1e-4
