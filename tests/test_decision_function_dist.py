"""decision_function under a process group on the CPU (gloo, world 2): with the
same X on both ranks a row-sharded model scores its block on each rank and
gathers, and every rank returns the single-process (m, C) matrix, consistent
with predict row for row.  Device entry points: tests/fake_engine.py, as in
tests/test_dropin_dist_logic.py."""
import numpy as np
import torch.multiprocessing as mp

from test_dropin_dist_logic import _data, _free_port, _patch, restore  # noqa: F401  (restore: fixture)


def _run(X, y):
    from utils.SIMCA import SIMCA

    m = SIMCA(n_components=[4, 3], verbose=False, type="alt").fit(X, y)
    return {"df": np.asarray(m.decision_function(X)), "pred": np.asarray(m.predict(X)),
            "sharded": np.array(getattr(m, "_sharded", False))}


def _worker(rank, world, port, path):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        _patch()
        np.savez(f"{path}.{rank}.npz", **_run(*_data(7)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_decision_function_sharded_gloo_world2(tmp_path, restore):  # noqa: F811
    path = str(tmp_path / "r")
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, path)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    for p in procs:
        if p.exitcode is None:
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    _patch()
    ref = _run(*_data(7))
    assert not bool(ref["sharded"]) and ref["df"].shape == (1300, 2)
    for r in range(2):
        got = np.load(f"{path}.{r}.npz")
        assert bool(got["sharded"])
        np.testing.assert_allclose(got["df"], ref["df"], rtol=1e-9, atol=1e-12)
        np.testing.assert_array_equal(got["pred"], (got["df"] > 0).astype(np.float64))
        np.testing.assert_array_equal(got["pred"], ref["pred"])
