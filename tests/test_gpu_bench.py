"""bench.py's command line: a plain run times its steps and prints the headline fields only,
--dump-outputs writes the last timed frame, --full adds the other measurements.  Both runs render
the same seeded scene (a 64x48 bunny frame), so their dumped frames must be equal bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "cpu_baseline", "parity", "multi", "end_to_end_ms", "ms_per_frame_to_host",
             "kernel_ms_rank0_streams1"}
ARGS = ["--gpus", "1", "--workload", "bunny", "--width", "64", "--height", "48"]


def run_bench(extra, out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra, "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr, np.load(os.path.join(out_dir, "frame.npy"))


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    return (run_bench(["--steps", "3", "--warmup", "2"], d / "plain"),
            run_bench(["--steps", "2", "--warmup", "1", "--full", "--cpu-rows", "16"], d / "full"))


@pytest.mark.gpu
def test_plain_run_is_lean(runs):
    line, err, frame = runs[0]
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line)
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 2
    assert line["unit"] == "Mray/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # every timed frame logs one line: --steps sets their number, and no second timed loop runs
    assert [ln.split(":")[0] for ln in err.split("\n") if "] step " in ln] == [f"[rank 0] step {i}" for i in range(3)]
    assert "cpu baseline" not in err
    assert frame.dtype == np.float32 and frame.shape == (48, 64, 3)
    assert np.isfinite(frame).all() and frame.max() > 0


@pytest.mark.gpu
def test_full_run_adds_the_rest_and_renders_the_same_frame(runs):
    line, _, frame = runs[1]
    assert HEADLINE | FULL_ONLY <= set(line) and line["full"] is True and line["steps"] == 2
    assert line["parity"]["differing"] == 0 and line["parity"]["nan_mismatch"] == 0
    assert line["cpu_baseline"]["value"] > 0 and line["roofline"]["launches"] > 0
    assert np.array_equal(frame.view(np.int32), runs[0][2].view(np.int32))
