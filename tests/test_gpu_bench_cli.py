"""GPU: bench.py's command line on a tiny workload -- a plain run times --steps steps and reports only
the headline record; --dump-outputs writes the last timed step's samples, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--num-samples", "2112", "--timesteps", "3"]


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *TINY, *extra], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_reports_headline_only_and_dumps_reproducible_outputs(torch_cuda, tmp_path):
    a = run_bench("--dump-outputs", str(tmp_path / "a"))
    b = run_bench("--dump-outputs", str(tmp_path / "b"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["steps"] == 2 and a["warmup"] == 1 and a["dtype"] == "bf16" and a["unit"] == "audio_s/s"
    assert a["ms_per_step"] > 0
    # value is the audio of the timed steps over their wall time, ms_per_step that wall time per step
    assert a["value"] == pytest.approx(2 * 2112 / 16000.0 / (a["ms_per_step"] * 1e-3), rel=1e-2)
    assert a["roofline"] is None and a["cpu_baseline"] is None and "variants" not in a
    assert os.listdir(tmp_path / "a") == ["out.npy"]
    xa, xb = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert xa.dtype == np.float32 and xa.shape == (2, 1, 2112) and np.isfinite(xa).all()
    assert np.array_equal(xa, xb)
    assert b["metric"] == a["metric"]


def test_full_run_adds_roofline_and_cpu_baseline(torch_cuda, tmp_path):
    d = run_bench("--full", "--cpu-steps", "1", "--dump-outputs", str(tmp_path / "f"))
    assert d["roofline"] is not None and d["roofline"]["kernel"]
    assert d["cpu_baseline"] is not None and d["cpu_baseline"]["value"] > 0
    assert np.load(tmp_path / "f" / "out.npy").shape == (2, 1, 2112)
