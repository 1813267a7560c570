"""bench.py as the driver runs it, on the box's one GPU.

``python bench.py --gpus 2`` (no WORLD_SIZE) must start two ranks itself; with
``--dist-backend gloo`` both share cuda:0, so the launcher, the strong / weak
scaling runs, the per-rank phase breakdown and the C3 CV line all execute
the same code the driver's 8-GPU RCCL run takes (only the backend differs).
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def test_bench_two_ranks_gloo_one_gpu():
    out = _run(["--full", "--gpus", "2", "--dist-backend", "gloo", "--rows", "65536", "--steps", "2", "--warmup", "1",
                "--no-cpu", "--no-vae", "--cv-reps", "1", "--phase-steps", "1"])
    assert out["n_gpus"] == 2
    assert out["scaling"] == "strong"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["rows_total"] == 65536 and out["config"]["rows_per_gpu"] == 32768
    assert set(out["phases_ms"]) == {"rank0", "rank1"}
    for ph in out["phases_ms"].values():
        assert {"gram", "allreduce", "eig", "fit_score", "limits", "predict_score"} <= set(ph)
    assert out["weak"]["rows_total"] == 131072 and out["weak"]["value"] > 0
    cv = out["cv"]
    assert "error" not in cv, cv
    assert cv["value"] > 0 and 0 <= cv["spec"] <= 100 and 0 <= cv["sens"] <= 100
    assert 0.8 < out["checks"]["accept_rate"] <= 1.0


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times the steps and prints the headline line only; the
    secondary measurements need --full.  --dump-outputs writes the last timed
    step's results: pred is predict's (n, 1) matrix of 0/1 whose mean is the
    line's accept rate, T2 / Q are the fit-set statistics (n rows)."""
    import numpy as np

    out = _run(["--rows", "65536", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["roofline"]["launches"] == 3  # --steps is the number of timed steps
    # value = rows / step time; ms_per_step is rounded to 3 decimals
    assert out["value"] == pytest.approx(65536 / (out["ms_per_step"] * 1e-3), rel=1e-3 / out["ms_per_step"])
    for key in ("phases_ms", "prep_fit_score", "cv", "cpu_baseline", "vae", "weak"):
        assert key not in out
    arrays = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert {"pred", "T", "T2", "Q", "P", "xmean", "evals", "limits"} <= set(arrays)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["pred"].shape == (65536, 1) and set(np.unique(arrays["pred"])) <= {0.0, 1.0}
    assert round(float(arrays["pred"].mean()), 4) == out["checks"]["accept_rate"]
    assert arrays["T"].shape == (65536, 20) and arrays["P"].shape == (20, 2048)
    assert arrays["T2"].shape == (65536,) and arrays["Q"].shape == (65536,)
    np.testing.assert_array_equal(arrays["limits"][:2], [out["checks"]["T2_limit"], out["checks"]["Q_limit"]])


def test_bench_single_gpu_small():
    out = _run(["--full", "--rows", "65536", "--steps", "2", "--warmup", "1", "--no-cpu", "--no-vae",
                "--cv-reps", "1", "--phase-steps", "1"])
    assert out["n_gpus"] == 1 and out["value"] > 0
    assert {"gram", "eig", "fit_score", "limits", "predict_score"} <= set(out["phases_ms"]["rank0"])
    assert out["roofline"]["launches"] == 2 and out["roofline"]["frac"] > 0
    assert "error" not in out["cv"], out["cv"]
