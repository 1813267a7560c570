"""bench.py's launcher logic on the CPU (no device is touched).

``--gpus N`` without WORLD_SIZE re-launches itself under
torch.distributed.run with N processes on 127.0.0.1 and returns the child's
status; under a launcher, a WORLD_SIZE that disagrees with --gpus is an error.
"""
import os
import sys

import pytest

import bench


def test_parse_defaults():
    a = bench.parse([])
    assert (a.gpus, a.scaling, a.dist_backend, a.rows) == (1, "strong", "nccl", 1_000_000)


def test_full_and_dump_outputs_are_off_by_default():
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float_arrays_with_a_fixed_row_sample(tmp_path):
    """Small arrays go out whole; one above DUMP_ARRAY_BYTES is cut to the same
    sorted row sample on every call, with the rows beside it."""
    import types

    import numpy as np
    import torch

    n = bench.DUMP_ARRAY_BYTES // 8 + 1000  # one float64 column of n rows is just over the cap
    g = torch.Generator().manual_seed(0)
    fit = types.SimpleNamespace(T=torch.rand(64, 3, generator=g), T2=torch.rand(n, dtype=torch.float64, generator=g),
                                Q=torch.rand(64, generator=g), P64=torch.rand(3, 8, dtype=torch.float64, generator=g),
                                mean64=torch.zeros(8, dtype=torch.float64), evals=torch.ones(3, dtype=torch.float64))
    result = {"fit": fit, "pred": torch.ones(64, 1, dtype=torch.float64), "T2_limit": 1.5, "Q_limit": 2.5,
              "D_limit": 3.5}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), result)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert set(a) == {"pred", "T", "T2", "T2_rows", "Q", "P", "xmean", "evals", "limits"} == set(b)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[name], b[name])
    rows = a["T2_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ARRAY_BYTES // 8 and np.all(np.diff(rows) > 0) and rows[-1] < n
    np.testing.assert_array_equal(a["T2"], fit.T2.numpy()[rows])
    np.testing.assert_array_equal(a["T"], fit.T.numpy())
    np.testing.assert_array_equal(a["limits"], [1.5, 2.5, 3.5])
    assert sum(v.nbytes for v in a.values()) <= 64 << 20


def test_launch_builds_torchrun_command(monkeypatch):
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"] = cmd
        return 7

    import subprocess

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--rows", "1000"])
    rc = bench.launch(bench.parse(["--gpus", "4", "--rows", "1000"]))
    assert rc == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr=127.0.0.1" in cmd and "--nnodes=1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--rows", "1000"] and cmd[-5].endswith("bench.py")


def test_main_routes_to_launcher_without_world_size(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setattr(bench, "launch", lambda args: 3)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 3


def test_world_size_must_match_gpus(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        bench.Ranks(bench.parse(["--gpus", "3"]))
