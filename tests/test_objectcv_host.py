"""Object-wise cross-validation (ocm/objectcv.py) on the CPU.

The splitter against scikit-learn's GroupKFold, the guard against row folds,
and the host logic of ``cross_validate_objects_grid`` (per-fold object tables →
decisions → the reference's aggregation at the object level) with the device
entry points replaced by tests/fake_engine.py plus a NumPy ``cv_objects``
defined here, against a refit loop written in this file, alone and under a
gloo world of two ranks (per-process: no collective).
"""
import contextlib
import io
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fake_engine
from oracle import simca_oracle as O


def object_data(seed=6, p=96, n_obj0=40, n_obj1=20, amp0=3.0, amp1=8.0):
    """Two classes of one spectral family (label 0: n_obj0 objects, label 1:
    n_obj1), about 900 rows in objects of 1..40 rows (most of 5..25, one of 40
    in each class, one of 1 row and one of 2 rows); every object is shifted by its
    own amount in its own direction (class 1 further on average), so that
    objects of both classes fall on both sides of the decision.
    → X float32, y, ids (m,)."""
    rng = np.random.default_rng(seed)

    def lengths(g, small):
        ln = rng.integers(5, 26, size=g)
        ln[rng.choice(g, size=2, replace=False)] = [small, 40]
        return ln

    ln0, ln1 = lengths(n_obj0, 1), lengths(n_obj1, 2)
    ln = np.concatenate([ln0, ln1])
    X = O.synth_spectra(int(ln.sum()), p, 4, rank=12, seed=seed, dtype=np.float64)
    y = np.repeat([0, 1], [ln0.sum(), ln1.sum()]).astype(np.int64)
    ids = np.repeat(np.arange(ln.size) + 100, ln)  # ids need not start at 0
    shift = rng.standard_normal((ln.size, p))
    shift /= np.linalg.norm(shift, axis=1, keepdims=True)
    shift *= (np.abs(rng.standard_normal(ln.size)) * np.repeat([amp0, amp1], [n_obj0, n_obj1]))[:, None]
    X = X + np.repeat(shift, ln, axis=0)
    return X.astype(np.float32), y, ids


# ------------------------------------------------------------------ splitter

def _cv(ids, n_splits=4, **kw):
    from ocm.objectcv import ObjectKFoldWithExternalVal

    return ObjectKFoldWithExternalVal(n_splits=n_splits, objects=ids, cls_label=0, **kw)


def test_fold_membership_is_groupkfolds():
    from sklearn.model_selection import GroupKFold

    X, y, ids = object_data()
    target = np.flatnonzero(y == 0)
    others = np.flatnonzero(y != 0)
    ref = list(GroupKFold(n_splits=4).split(target, groups=ids[target]))
    got = list(_cv(ids).split(X, y))
    assert len(got) == len(ref) == 4
    for (tr, te), (rtr, rte) in zip(got, ref):
        np.testing.assert_array_equal(tr, target[rtr])
        # held-out target rows, then every non-target row
        np.testing.assert_array_equal(te, np.concatenate([target[rte], others]))
        # no object on both sides
        assert not set(ids[tr]) & set(ids[te])
    folds = _cv(ids).target_folds(X, y)
    for f, (_, rte) in zip(folds, ref):
        np.testing.assert_array_equal(f, target[rte])


def test_objects_and_offsets_give_the_same_splits():
    from ocm.objectcv import ObjectKFoldWithExternalVal
    from ocm.objects import segment_offsets

    X, y, ids = object_data()
    a = list(_cv(ids).split(X, y))
    b = list(ObjectKFoldWithExternalVal(n_splits=4, offsets=segment_offsets(ids), cls_label=0).split(X, y))
    c = list(ObjectKFoldWithExternalVal(n_splits=4, offsets=segment_offsets(ids),
                                        cls_idx=np.flatnonzero(y == 0)).split(X))  # no y: indices given
    for (tr, te), (tr2, te2), (tr3, te3) in zip(a, b, c):
        np.testing.assert_array_equal(tr, tr2)
        np.testing.assert_array_equal(te, te2)
        np.testing.assert_array_equal(tr, tr3)
        np.testing.assert_array_equal(te, te3)


def test_splitter_errors():
    from ocm.objectcv import ObjectKFoldWithExternalVal
    from ocm.objects import segment_offsets

    X, y, ids = object_data()
    off = segment_offsets(ids)
    with pytest.raises(ValueError, match="exactly one"):
        ObjectKFoldWithExternalVal(n_splits=3, objects=ids, offsets=off, cls_label=0)
    with pytest.raises(ValueError, match="exactly one"):
        ObjectKFoldWithExternalVal(n_splits=3, cls_label=0)
    y_mixed = y.copy()
    y_mixed[off[2]] = 1  # one row of object 2 (two or more rows) changes label
    assert off[3] - off[2] >= 2
    with pytest.raises(ValueError, match="more than one label"):
        list(_cv(ids).split(X, y_mixed))
    with pytest.raises(ValueError, match="more than one label"):  # without y: target and other rows in one object
        list(ObjectKFoldWithExternalVal(n_splits=3, objects=ids, cls_idx=np.flatnonzero(y_mixed == 0)).split(X))
    with pytest.raises(ValueError, match="fewer than"):
        list(_cv(ids, n_splits=41).split(X, y))  # 40 target objects
    with pytest.raises(ValueError, match="shape"):
        list(_cv(ids[:-1]).split(X, y))
    with pytest.raises(ValueError, match="from 0 to"):
        list(ObjectKFoldWithExternalVal(n_splits=3, offsets=off[:-1], cls_label=0).split(X, y))
    with pytest.raises(ValueError, match="empty"):
        list(ObjectKFoldWithExternalVal(n_splits=3, offsets=np.insert(off, 1, off[1]), cls_label=0).split(X, y))


# ------------------------------------------------------- fake-engine plumbing

def np_cv_objects(T, Q, inv_evals, offsets, configs, want_votes=True, want_dsum=True, checked=False):
    """NumPy stand-in for ocm.engine.cv_objects (exact float64)."""
    off = np.asarray(offsets.numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
    first = off[:-1]
    votes = np.zeros((len(configs), first.size), dtype=np.int64)
    dsum = np.zeros((len(configs), first.size))
    for c, (lv, ty, a, b, dl) in enumerate(configs):
        t2, q = fake_engine._prefix(T, Q, inv_evals, lv)
        t, qq = t2 * a, q.astype(np.float64) * b
        d = {"sim": np.maximum(t, qq), "alt": np.sqrt(t * t + qq * qq)}.get(ty, t + qq)
        votes[c] = np.add.reduceat((d < dl).astype(np.int64), first)
        dsum[c] = np.add.reduceat(dl - d, first)
    return (torch.from_numpy(votes) if want_votes else None), (torch.from_numpy(dsum) if want_dsum else None)


def np_segment_sums(X, offsets, checked=False):
    """NumPy stand-in for ocm.engine.segment_sums (predict_objects in the generic loop)."""
    off = np.asarray(offsets.numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
    return torch.from_numpy(np.add.reduceat(X.numpy().astype(np.float64), off[:-1], axis=0))


def _simca_module():
    import utils.SIMCA  # noqa: F401

    return sys.modules["utils.SIMCA"]


def _patch():
    import ocm.cv as fe
    import ocm.dist as od

    fake_engine.cv_objects = np_cv_objects
    fe.engine = od.engine = _simca_module().engine = fake_engine


@pytest.fixture
def fake(monkeypatch):
    import ocm.cv as fe
    import ocm.dist as od

    monkeypatch.setattr(fake_engine, "cv_objects", np_cv_objects, raising=False)
    monkeypatch.setattr(fake_engine, "segment_sums", np_segment_sums, raising=False)
    for mod in (fe, od, _simca_module()):
        monkeypatch.setattr(mod, "engine", fake_engine)


GRID = {"type": ["alt", "dd"], "t2lim": ["Fdist"], "qlim": ["jm"]}


def _objects_grid(X, y, ids, rule, grid=GRID, **kw):
    from ocm.objectcv import cross_validate_objects_grid
    from utils.SIMCA import SIMCA

    with contextlib.redirect_stdout(io.StringIO()):
        return cross_validate_objects_grid(SIMCA(verbose=False), X, y, _cv(ids, n_splits=3), LV_min=2, LV_max=4,
                                           param_grid=grid, rule=rule, min_fraction=0.5, print_summary=False,
                                           store_predictions=True, **kw)


def test_not_a_row_fold_splitter_and_engine_gets_whole_objects(fake, monkeypatch):
    import ocm.cv as fe
    from utils.CVSIMCA import ClasswiseKFoldWithExternalVal, cross_validate_simca_grid
    from utils.SIMCA import SIMCA

    X, y, ids = object_data()
    cv = _cv(ids, n_splits=3)
    assert not isinstance(cv, ClasswiseKFoldWithExternalVal)
    seen = []
    orig = fe.cv_grid

    def spy(*a, **k):
        seen.append([np.asarray(f) for f in a[2]])
        return orig(*a, **k)

    monkeypatch.setattr(fe, "cv_grid", spy)
    with contextlib.redirect_stdout(io.StringIO()):
        res = cross_validate_simca_grid(SIMCA(verbose=False), X, y, cv, LV_min=2, LV_max=3, print_summary=False)
    assert len(seen) == 1 and len(seen[0]) == 3
    rows_of = {i: np.flatnonzero(ids == i) for i in np.unique(ids)}
    covered = np.concatenate(seen[0])
    np.testing.assert_array_equal(np.sort(covered), np.flatnonzero(y == 0))
    for f in seen[0]:
        for i in np.unique(ids[f]):
            assert np.isin(rows_of[i], f).all()  # a union of whole objects
    assert [r["LV"] for r in res["results"]] == [2, 3]


def _loop(X, y, ids, rule, grid, lvs, n_splits, min_fraction=0.5):
    """The refit loop: per setting and fold, fit, decision_function, per-object
    fraction and mean, predict_objects' decision, the reference's aggregation."""
    from sklearn.model_selection import GroupKFold, ParameterGrid
    from utils.SIMCA import SIMCA

    target, others = np.flatnonzero(y == 0), np.flatnonzero(y != 0)
    splits = [(target[tr], np.concatenate([target[te], others]), np.unique(ids[target[te]]).size)
              for tr, te in GroupKFold(n_splits=n_splits).split(target, groups=ids[target])]
    uniq, first = np.unique(ids, return_index=True)
    order = np.argsort(first)
    index_of = {int(uniq[j]): g for g, j in enumerate(order)}
    G = uniq.size
    label = y[np.sort(first)]
    out = []
    for combo in ParameterGrid(grid):
        for lv in lvs:
            pooled, frac, score = np.zeros(G), np.full(G, np.nan), np.full(G, np.nan)
            pooled_px = np.zeros(y.size)
            spec, spec_px = [], []
            for f, (tr, te, n_t) in enumerate(splits):
                m = SIMCA(n_components=lv, verbose=False, **combo).fit(X[tr], y[tr])
                D = np.asarray(m.decision_function(X[te])).reshape(-1)
                tid = ids[te]
                st = np.concatenate([[0], np.flatnonzero(tid[1:] != tid[:-1]) + 1])
                cnt = np.diff(np.concatenate([st, [tid.size]])).astype(np.float64)
                fr = np.add.reduceat((D > 0).astype(np.float64), st) / cnt
                sc = np.add.reduceat(D, st) / cnt
                dec = (fr >= min_fraction) if rule == "vote" else (sc > 0)
                g = np.array([index_of[int(i)] for i in tid[st]])
                neg = label[g] != 0
                spec.append(100.0 * np.sum(~dec & neg) / np.sum(neg))
                neg_px = y[te] != 0
                spec_px.append(100.0 * np.sum((D <= 0) & neg_px) / np.sum(neg_px))
                keep = slice(0, n_t) if f < len(splits) - 1 else slice(None)
                pooled[g[keep]], frac[g[keep]], score[g[keep]] = dec[keep], fr[keep], sc[keep]
                keep_px = slice(0, np.sum(y[te] == 0)) if f < len(splits) - 1 else slice(None)
                pooled_px[te[keep_px]] = (D > 0)[keep_px]
            sens = 100.0 * np.sum((pooled == 1) & (label == 0)) / np.sum(label == 0)
            sens_px = 100.0 * np.sum((pooled_px == 1) & (y == 0)) / np.sum(y == 0)
            out.append({"params": combo, "LV": lv, "spec": float(np.mean(spec)), "sens": float(sens),
                        "spec_px": float(np.mean(spec_px)), "sens_px": float(sens_px), "prediction": pooled,
                        "fraction": frac, "score": score})
    return out


@pytest.mark.parametrize("rule", ["vote", "mean_distance"])
def test_aggregation_vs_refit_loop(fake, rule):
    X, y, ids = object_data()
    res = _objects_grid(X, y, ids, rule)
    ref = _loop(X, y, ids, rule, GRID, [2, 3, 4], 3)
    assert set(res) == {"results", "best_params", "best_LV", "best_score", "best_estimator", "by_combo"}
    assert len(res["results"]) == len(ref) == 6
    mixed = 0
    for r, b, e in zip(res["results"], res["by_combo"], ref):
        assert r["params"] == e["params"] == b["params"] and r["LV"] == e["LV"] == b["LV"]
        np.testing.assert_array_equal(b["prediction"], e["prediction"])
        np.testing.assert_allclose(b["fraction"], e["fraction"], rtol=0, atol=1e-12)
        # both sides hold T and Q in float32 (2⁻²⁴ relative each), the engine at LV_max and the loop at LV
        np.testing.assert_allclose(b["score"], e["score"], rtol=1e-5, atol=1e-6)
        for key in ("spec", "sens", "spec_px", "sens_px"):
            assert abs(r[key] - e[key]) <= 1e-12, (key, r[key], e[key])
        assert abs(r["eff"] - np.sqrt(e["sens"] * e["spec"])) <= 1e-12
        assert abs(r["eff_px"] - np.sqrt(e["sens_px"] * e["spec_px"])) <= 1e-12
        mixed += 0.0 < r["spec"] < 100.0 and 0.0 < r["sens"] < 100.0
    assert mixed  # accepted and rejected objects in both classes somewhere
    best = max(res["results"], key=lambda r: r["eff"])
    assert res["best_score"] == best["eff"]
    assert res["best_estimator"].is_fitted_


def test_pixel_records_match_simca_grid(fake):
    """spec_px / sens_px / eff_px are what cross_validate_simca_grid returns for the same splitter."""
    from utils.CVSIMCA import cross_validate_simca_grid
    from utils.SIMCA import SIMCA

    X, y, ids = object_data()
    res = _objects_grid(X, y, ids, "vote")
    with contextlib.redirect_stdout(io.StringIO()):
        px = cross_validate_simca_grid(SIMCA(verbose=False), X, y, _cv(ids, n_splits=3), LV_min=2, LV_max=4,
                                       param_grid=GRID, print_summary=False)
    for r, q in zip(res["results"], px["results"]):
        assert (r["params"], r["LV"]) == (q["params"], q["LV"])
        assert (r["spec_px"], r["sens_px"], r["eff_px"]) == (q["spec"], q["sens"], q["eff"])


def test_unsupported_rule_and_splitter(fake):
    from ocm.objectcv import cross_validate_objects_grid
    from utils.CVSIMCA import ClasswiseKFoldWithExternalVal
    from utils.SIMCA import SIMCA

    X, y, ids = object_data()
    for rule in ("mean_spectrum", "median"):
        with pytest.raises(ValueError, match="vote, mean_distance"):
            _objects_grid(X, y, ids, rule)
    with pytest.raises(TypeError, match="ObjectKFoldWithExternalVal"):
        cross_validate_objects_grid(SIMCA(verbose=False), X, y, ClasswiseKFoldWithExternalVal(n_splits=3, cls_label=0))


def test_generic_loop_for_float64(fake, monkeypatch):
    """float64 spectra are declined by the fold engine: the refit loop gives the same layout."""
    import ocm.cv as fe

    X, y, ids = object_data()
    monkeypatch.setattr(fe, "cv_grid", lambda *a, **k: pytest.fail("the fold engine ran on float64 spectra"))
    grid = {"type": ["alt"]}
    res = _objects_grid(X.astype(np.float64), y, ids, "vote", grid=grid)
    ref = _loop(X.astype(np.float64), y, ids, "vote", grid, [2, 3, 4], 3)
    for r, b, e in zip(res["results"], res["by_combo"], ref):
        assert set(r) == {"params", "LV", "spec", "sens", "eff", "spec_px", "sens_px", "eff_px"}
        np.testing.assert_array_equal(b["prediction"], e["prediction"])
        np.testing.assert_allclose(b["fraction"], e["fraction"], atol=1e-12)
        for key in ("spec", "sens", "spec_px", "sens_px"):
            assert abs(r[key] - e[key]) <= 1e-9


# ------------------------------------------------------------- process group

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, path):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        _patch()
        issued = []
        for name in ("all_reduce", "all_gather", "broadcast", "reduce", "all_gather_object"):
            orig = getattr(dist, name)

            def spy(*a, _name=name, _orig=orig, **k):
                issued.append(_name)
                return _orig(*a, **k)

            setattr(dist, name, spy)
        X, y, ids = object_data()
        res = _objects_grid(X, y, ids, "vote")
        np.savez(f"{path}.{rank}.npz", spec=[r["spec"] for r in res["results"]],
                 sens=[r["sens"] for r in res["results"]], spec_px=[r["spec_px"] for r in res["results"]],
                 pred=np.stack([b["prediction"] for b in res["by_combo"]]), issued=np.array(issued, dtype="U32"),
                 best=np.array(res["best_LV"]))
    finally:
        dist.destroy_process_group()


def test_per_process_under_gloo_world2(tmp_path, fake):
    path = str(tmp_path / "o")
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
    X, y, ids = object_data()
    res = _objects_grid(X, y, ids, "vote")
    for r in range(2):
        got = np.load(f"{path}.{r}.npz")
        assert got["issued"].size == 0, got["issued"]
        np.testing.assert_array_equal(got["spec"], [x["spec"] for x in res["results"]])
        np.testing.assert_array_equal(got["sens"], [x["sens"] for x in res["results"]])
        np.testing.assert_array_equal(got["spec_px"], [x["spec_px"] for x in res["results"]])
        np.testing.assert_array_equal(got["pred"], np.stack([b["prediction"] for b in res["by_combo"]]))
        assert int(got["best"]) == res["best_LV"]
