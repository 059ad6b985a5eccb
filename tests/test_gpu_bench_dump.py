"""GPU: bench.py as the driver runs it -- a plain run (set up, warm up, time exactly --steps steps, the line) and a --full run --
each writing what its last timed step computed (--dump-outputs).  The two runs see the same seeded inputs, so their outputs
agree; the plain run replays the hipGraph, the --full run launches eagerly: the dumps hold the same step both ways."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--draws-per-gpu", "64", "--steps", "7", "--warmup", "2",
           "--dump-outputs", str(out_dir)] + args
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_and_full_runs_dump_the_same_step(tmp_path):
    plain = _bench([], tmp_path / "plain")
    full = _bench(["--full", "--no-extras", "--no-cpu-baseline", "--no-stats", "--no-graph"], tmp_path / "full")
    for line in (plain, full):
        assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1
        assert line["unit"] == "evals/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["ms_per_step"] > 0 and abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
        assert line["configs_ms"]["c2"] == round(line["ms_per_step"], 4)
    # what moved behind --full
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["full_record"] is None
    assert full["roofline"]["bound"] == "hbm" and full["roofline"]["active_cadences_per_launch"] > 0
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "full"))
    assert {"flux.npy", "flux_rows.npy", "flux_dot_gbar.npy", "grad_period.npy", "grad_u1.npy", "grad_u2.npy"} <= set(files)
    assert sum((tmp_path / "plain" / f).stat().st_size for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.dtype == np.float64 and a.shape == b.shape, f
        assert np.all(np.isfinite(a)), f
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300, err_msg=f)
    flux = np.load(tmp_path / "plain" / "flux.npy")
    assert flux.shape[1] == 150_000 and flux.min() < -1e-3        # whole rows of the dense flux, transits in them
    assert np.any(np.load(tmp_path / "plain" / "grad_period.npy") != 0)
