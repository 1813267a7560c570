"""Object-wise cross-validation on the GPU: ocm_cv_objects against NumPy
float64 and against ocm_cv_counts on the same scores, and the fold engine under
object-wise folds against refit loops, pixel level and object level.

Kernel boundaries reached (csrc/ocm_cv.hip): one row; an object across the
256-row chunk boundary; one object over more than two chunks and over more than
16 following chunks (the final pass's interleaved chains); one-row objects;
several pieces per 64-lane wave; the three KB instantiations (k = 1, 20, 64);
ncfg = 1, 7 and 1024.
"""
import contextlib
import io
import math

import numpy as np
import pytest

from conftest import gpu_available
from test_objectcv_host import object_data

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

TYPES = ("alt", "sim", "ci", "dd")


def _dyadic_scores(m, k, seed):
    """Scores on a dyadic grid: every intermediate of the decision arithmetic
    (t², the prefix sums in any order, the float32 rounding of Q, the scaled
    distances and t² + q²) is exact in float64, so the rows' d = dlim − d_red are
    the same on the device and in NumPy up to the one rounding of sqrt and of
    the subtraction, and the comparison below tests the summation alone."""
    rng = np.random.default_rng(seed)
    T = (rng.integers(-12, 13, size=(m, k)) / 4.0).astype(np.float32)
    Q = (rng.integers(0, 200, size=m) / 8.0).astype(np.float32)
    inv = 2.0 ** -(np.arange(k) % 5).astype(np.float64)
    return T, Q, inv


def _configs(k, ncfg, T, Q, inv, seed):
    """ncfg configurations: every decision type, lv = 1 and lv = k among them,
    dyadic scales, and a dlim that is one row's own d_red (a tie: not accepted)."""
    rng = np.random.default_rng(seed)
    lvs = [1, k] + [int(v) for v in rng.integers(1, k + 1, size=max(ncfg - 2, 0))]
    cfgs = []
    for c in range(ncfg):
        lv, ty = lvs[c % len(lvs)] if ncfg > 1 else k, TYPES[c % 4]
        a, b = 2.0 ** -(2 + int(lv).bit_length()), 2.0 ** -4
        d = _rows_dred(T, Q, inv, (lv, ty, a, b, 0.0))
        dl = float(np.sort(d)[(c * 7 + d.size // 2) % d.size]) if d.size else 1.0
        cfgs.append((lv, ty, a, b, dl))
    return cfgs


def _rows_dred(T, Q, inv, cfg, exact=True):
    """The restatement of test_gpu_cv.test_fold_engine_counts_kernel_exact, per row."""
    lv, ty, a, b, _ = cfg
    t2sq = T.astype(np.float64) ** 2
    t2 = (t2sq[:, :lv] * inv[:lv]).sum(1)
    q = (Q.astype(np.float64) + t2sq[:, lv:].sum(1)).astype(np.float32).astype(np.float64)
    if exact:  # the dyadic grid: no rounding, whatever the order
        assert np.array_equal(t2, (t2sq[:, :lv][:, ::-1] * inv[:lv][::-1]).sum(1))
        assert np.array_equal(q, Q.astype(np.float64) + t2sq[:, lv:][:, ::-1].sum(1))
    t, qq = t2 * a, q * b
    return {"sim": np.maximum(t, qq), "alt": np.sqrt(t * t + qq * qq)}.get(ty, t + qq)


def _lengths(spec, m, seed):
    if spec == "ones":
        return np.ones(m, np.int64)
    if spec == "random":
        rng = np.random.default_rng(seed)
        ln = []
        while sum(ln) < m:
            ln.append(int(rng.integers(1, 91)))
        ln[-1] -= sum(ln) - m
        return np.array([v for v in ln if v > 0], np.int64)
    return np.array(spec, np.int64)


CASES = [
    (1, [1], 1, 1),
    (257, [200, 57], 20, 7),            # the second object crosses row 256
    (700, [700], 64, 7),                # one object over three chunks
    (4700, [4500, 200], 20, 7),         # a chain of 17 heads: two rounds of the final pass
    (300, "ones", 20, 1024),
    (1000, "random", 20, 7),            # lengths 1..90: several pieces per wave
    (1000, "random", 1, 7),
    (1000, "random", 64, 1),
]


@pytest.mark.parametrize("m,spec,k,ncfg", CASES, ids=[f"m{c[0]}-k{c[2]}-c{c[3]}" for c in CASES])
def test_cv_objects_vs_numpy(m, spec, k, ncfg):
    import torch
    from ocm import engine

    T, Q, inv = _dyadic_scores(m, k, seed=m + k)
    cfgs = _configs(k, ncfg, T, Q, inv, seed=ncfg)
    ln = _lengths(spec, m, seed=m)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    assert off[-1] == m
    dev = torch.device("cuda", 0)
    Td, Qd, invd = (torch.from_numpy(a).to(dev) for a in (T, Q, inv))
    votes, dsum = engine.cv_objects(Td, Qd, invd, off, cfgs)
    assert votes.shape == dsum.shape == (ncfg, ln.size)
    votes, dsum = votes.cpu().numpy(), dsum.cpu().numpy()
    first = off[:-1]
    worst = 0.0
    for c, cfg in enumerate(cfgs):
        dred = _rows_dred(T, Q, inv, cfg)
        d = cfg[4] - dred
        np.testing.assert_array_equal(votes[c], np.add.reduceat((dred < cfg[4]).astype(np.int64), first))
        # any summation order of L terms: |error| <= L·2⁻⁵³·Σ|d_i| (to first order), against the exact sum
        ref = np.array([math.fsum(d[a:b]) for a, b in zip(off[:-1], off[1:])])
        bound = ln * 2.0 ** -53 * np.add.reduceat(np.abs(d), first)
        err = np.abs(dsum[c] - ref)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert (err <= bound).all(), (c, cfg, int(np.argmax(err - bound)), float(np.max(err - bound)))
    print(f"cv_objects m={m} k={k} ncfg={ncfg}: worst |dsum - sum| / bound = {worst:.3f}")


def test_cv_objects_empty_and_errors():
    import torch
    from ocm import _lib, engine

    dev = torch.device("cuda", 0)
    T = torch.zeros((0, 5), dtype=torch.float32, device=dev)
    Q = torch.zeros(0, dtype=torch.float32, device=dev)
    inv = torch.ones(5, dtype=torch.float64, device=dev)
    cfg = [(2, "alt", 1.0, 1.0, 1.0)]
    votes, dsum = engine.cv_objects(T, Q, inv, np.zeros(1, np.int64), cfg)
    assert votes.shape == dsum.shape == (1, 0)
    T1 = torch.ones((3, 5), dtype=torch.float32, device=dev)
    Q1 = torch.ones(3, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        engine.cv_objects(T1, Q1, inv, [0, 2], cfg)       # does not reach m
    with pytest.raises(ValueError):
        engine.cv_objects(T1, Q1, inv, [0, 2, 2, 3], cfg)  # an empty object
    with pytest.raises(ValueError):
        engine.cv_objects(T1, Q1, inv, [0, 3], cfg, want_votes=False, want_dsum=False)
    # the C entry itself: both outputs NULL, LV outside [1, k]
    lib = _lib.load()
    ctx = _lib.Context.get(0).handle
    off = torch.tensor([0, 3], dtype=torch.int64, device=dev)
    one = (_lib.OcmCvConfig * 1)(_lib.OcmCvConfig(2, 1, 1.0, 1.0, 1.0))
    bad = (_lib.OcmCvConfig * 1)(_lib.OcmCvConfig(6, 1, 1.0, 1.0, 1.0))
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (ctx, T1.data_ptr(), 3, 5, Q1.data_ptr(), inv.data_ptr(), off.data_ptr(), 1)
    assert lib.ocm_cv_objects(*args, one, 1, None, None, None) == _lib.OCM_ERR_ARG
    assert lib.ocm_cv_objects(*args, bad, 1, out.data_ptr(), None, None) == _lib.OCM_ERR_ARG
    assert lib.ocm_cv_objects(*args, one, 1, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert int(out[0]) == 0  # √(5² + 1²) ≥ 1: no row accepted


def _random_scores(m, k, seed):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((m, k)).astype(np.float32) * np.linspace(3, 0.5, k).astype(np.float32)
    Q = rng.gamma(2.0, 1.0, m).astype(np.float32)
    return T, Q, 1.0 / np.linspace(9, 0.3, k)


def test_cv_objects_vs_cv_counts_and_reproducible():
    """The accept of ocm_cv_counts bit for bit: votes = per-object sums of its
    accept_out and Σ_g votes = TP + FP, on scores that do round; and the same
    dsum bits on every call, with and without votes."""
    import torch
    from ocm import engine

    m, k = 1000, 12
    T, Q, inv = _random_scores(m, k, seed=5)
    rng = np.random.default_rng(6)
    pos = rng.random(m) < 0.7
    cfgs = [(lv, ty, 1.0 / (2.0 * lv), 1.0 / 5.0, dl) for lv in (1, 3, 7, 12) for ty, dl in
            (("alt", np.sqrt(2)), ("sim", 1.0), ("ci", 1.7), ("dd", 2.5))]
    off = np.concatenate([[0], np.cumsum(_lengths("random", m, seed=9))]).astype(np.int64)
    dev = torch.device("cuda", 0)
    Td, Qd, invd = (torch.from_numpy(a).to(dev) for a in (T, Q, inv))
    posd = torch.from_numpy(pos.astype(np.uint8)).to(dev)
    cnt, acc = engine.cv_counts(Td, Qd, invd, posd, 600, cfgs, want_accept=True)
    votes, dsum = engine.cv_objects(Td, Qd, invd, off, cfgs)
    cnt, acc, v = cnt.cpu().numpy(), acc.cpu().numpy(), votes.cpu().numpy()
    np.testing.assert_array_equal(v, np.add.reduceat(acc, off[:-1], axis=1).astype(np.int64))
    np.testing.assert_array_equal(v.sum(1), cnt[:, :, 0].sum(1) + cnt[:, :, 2].sum(1))
    assert 0 < v.sum() < m * len(cfgs)
    # the decision sums against NumPy on rounding scores: the rows' own rounding (≈ k + 6 operations)
    # comes on top of the summation's, so this is a sanity check, not the kernel's bound
    for c, cfg in enumerate(cfgs):
        d = cfg[4] - _rows_dred(T, Q, inv, cfg, exact=False)
        np.testing.assert_allclose(dsum[c].cpu().numpy(), np.add.reduceat(d, off[:-1]), rtol=1e-12,
                                   atol=1e-12 * float(np.abs(d).max()) * 90)
    _, dsum2 = engine.cv_objects(Td, Qd, invd, off, cfgs)
    _, dsum3 = engine.cv_objects(Td, Qd, invd, off, cfgs, want_votes=False)
    votes4, none = engine.cv_objects(Td, Qd, invd, off, cfgs, want_dsum=False)
    assert torch.equal(dsum, dsum2) and torch.equal(dsum, dsum3)
    assert none is None and torch.equal(votes4, votes)


# ------------------------------------------------------------------ fold engine

FAMILIES = [
    {"type": ["alt"], "t2lim": ["Fdist"], "qlim": ["jm"]},
    {"type": ["alt"], "t2lim": ["perc"], "qlim": ["chi2pom"]},
    {"type": ["dd"]},
]


def _splitter(ids, n_splits=3):
    from ocm.objectcv import ObjectKFoldWithExternalVal

    return ObjectKFoldWithExternalVal(n_splits=n_splits, objects=ids, cls_label=0)


def _fast_used(monkeypatch):
    import ocm.cv as fe

    calls = {"n": 0}
    orig = fe.cv_grid

    def wrapped(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)

    monkeypatch.setattr(fe, "cv_grid", wrapped)
    return calls


@pytest.fixture(scope="module")
def data():
    return object_data()


@pytest.mark.parametrize("gi", range(len(FAMILIES)))
def test_pixel_level_under_object_folds(data, gi, monkeypatch):
    """cross_validate_simca_grid with the object splitter: the fold engine
    against the refit loop, by the yardsticks of test_gpu_cv for row folds."""
    import utils.CVSIMCA as CVmod
    from utils import SIMCA, cross_validate_simca_grid

    X, y, ids = data

    def run():
        with contextlib.redirect_stdout(io.StringIO()):
            return cross_validate_simca_grid(SIMCA(verbose=False), X, y, _splitter(ids), LV_min=2, LV_max=5,
                                             param_grid=FAMILIES[gi], print_summary=False, store_predictions=True)

    calls = _fast_used(monkeypatch)
    fast = run()
    assert calls["n"] == 1
    monkeypatch.setattr(CVmod, "_fast_grid", lambda *a, **k: (None, None))
    slow = run()
    assert calls["n"] == 1
    assert [r["params"] for r in fast["results"]] == [r["params"] for r in slow["results"]]
    assert [r["LV"] for r in fast["results"]] == [r["LV"] for r in slow["results"]] == [2, 3, 4, 5]
    pf = np.stack([b["prediction"] for b in fast["by_combo"]])
    ps = np.stack([b["prediction"] for b in slow["by_combo"]])
    diff = (pf != ps).sum(axis=1)
    assert diff.max() <= 2, diff
    np.testing.assert_allclose([r["spec"] for r in fast["results"]], [r["spec"] for r in slow["results"]], atol=0.5)
    np.testing.assert_allclose([r["sens"] for r in fast["results"]], [r["sens"] for r in slow["results"]], atol=0.5)


_LOOPS = {}


def _refit_loop(data, gi, rule, min_fraction=0.5):
    """Per setting and fold: SIMCA.fit on the training rows, predict_objects on
    the fold's test rows; the reference's aggregation on the object vectors.
    Computed once per (family, rule)."""
    if (gi, rule) in _LOOPS:
        return _LOOPS[gi, rule]
    from sklearn.model_selection import ParameterGrid
    from utils import SIMCA

    X, y, ids = data
    uniq, first = np.unique(ids, return_index=True)
    index_of = {int(uniq[j]): g for g, j in enumerate(np.argsort(first))}
    first = np.sort(first)
    G = first.size
    label = y[first]
    counts = np.diff(np.concatenate([first, [y.size]])).astype(np.float64)
    splits = list(_splitter(ids).split(X, y))
    out = []
    for combo in ParameterGrid(FAMILIES[gi]):
        for lv in (2, 3, 4, 5):
            pooled, frac, score, dlim = np.zeros(G), np.zeros(G), np.zeros(G), np.zeros(G)
            spec = []
            for f, (tr, te) in enumerate(splits):
                with contextlib.redirect_stdout(io.StringIO()):
                    model = SIMCA(n_components=lv, verbose=False, **combo).fit(X[tr], y[tr])
                    res = model.predict_objects(X[te], objects=ids[te], rule=rule, min_fraction=min_fraction)
                tid = ids[te]
                st = np.concatenate([[0], np.flatnonzero(tid[1:] != tid[:-1]) + 1])
                g = np.array([index_of[int(i)] for i in tid[st]])
                dec = np.asarray(res.pred).reshape(-1)
                neg = label[g] != 0
                spec.append(100.0 * np.sum((dec == 0) & neg) / np.sum(neg))
                keep = label[g] == 0 if f < len(splits) - 1 else np.ones(g.size, bool)
                pooled[g[keep]] = dec[keep]
                frac[g[keep]] = np.asarray(res.fraction).reshape(-1)[keep]
                score[g[keep]] = np.asarray(res.score).reshape(-1)[keep]
                dlim[g[keep]] = float(model._model[0]["D_limit"])
            sens = 100.0 * np.sum((pooled == 1) & (label == 0)) / np.sum(label == 0)
            out.append({"params": combo, "LV": lv, "spec": float(np.mean(spec)), "sens": float(sens),
                        "prediction": pooled, "fraction": frac, "score": score, "dlim": dlim})
    _LOOPS[gi, rule] = (out, label, counts)
    return _LOOPS[gi, rule]


@pytest.mark.parametrize("rule", ["vote", "mean_distance"])
@pytest.mark.parametrize("gi", range(len(FAMILIES)))
def test_object_level_vs_refit_loop(data, gi, rule, monkeypatch):
    from ocm.objectcv import cross_validate_objects_grid
    from utils import SIMCA

    X, y, ids = data
    ref, label, counts = _refit_loop(data, gi, rule)
    calls = _fast_used(monkeypatch)
    with contextlib.redirect_stdout(io.StringIO()):
        res = cross_validate_objects_grid(SIMCA(verbose=False), X, y, _splitter(ids), LV_min=2, LV_max=5,
                                          param_grid=FAMILIES[gi], rule=rule, min_fraction=0.5,
                                          print_summary=False, store_predictions=True)
    assert calls["n"] == 1
    assert set(res) == {"results", "best_params", "best_LV", "best_score", "best_estimator", "by_combo"}
    assert len(res["results"]) == len(ref) == 4
    G = label.size
    n_pos, n_neg = int(np.sum(label == 0)), int(np.sum(label != 0))
    both_sides = False
    for r, b, e in zip(res["results"], res["by_combo"], ref):
        assert r["params"] == e["params"] and r["LV"] == e["LV"]
        assert b["prediction"].shape == b["fraction"].shape == b["score"].shape == (G,)
        # at most two pixels of an object decided differently (the yardstick of the pixel-level test)
        assert (np.abs(b["fraction"] - e["fraction"]) <= 2.0 / counts + 1e-15).all()
        if rule == "vote":
            border = np.abs(e["fraction"] - 0.5) <= 2.0 / counts
        else:
            border = np.abs(e["score"]) < 1e-4 * e["dlim"]
        assert border.sum() <= 0.1 * G, int(border.sum())
        differs = b["prediction"] != e["prediction"]
        assert not (differs & ~border).any(), np.flatnonzero(differs & ~border)
        assert abs(r["spec"] - e["spec"]) <= 100.0 / n_neg + 1e-9
        assert abs(r["sens"] - e["sens"]) <= 100.0 / n_pos + 1e-9
        assert abs(r["eff"] - np.sqrt(r["sens"] * r["spec"])) <= 1e-9
        acc = e["prediction"] == 1
        both_sides |= all(0 < np.sum(acc & sel) < np.sum(sel) for sel in (label == 0, label != 0))
    assert both_sides  # accepted and rejected objects in the target class and in the other class
    assert res["best_score"] == max(r["eff"] for r in res["results"])


def test_object_level_pixel_fields_and_fallback(data, monkeypatch):
    """spec_px / sens_px are cross_validate_simca_grid's values for the same
    splitter; float64 spectra, which the fold engine declines, take the refit
    loop and return the same layout."""
    from ocm.objectcv import cross_validate_objects_grid
    from utils import SIMCA, cross_validate_simca_grid

    X, y, ids = data
    kw = dict(LV_min=3, LV_max=4, param_grid=FAMILIES[0], print_summary=False)
    with contextlib.redirect_stdout(io.StringIO()):
        obj = cross_validate_objects_grid(SIMCA(verbose=False), X, y, _splitter(ids), **kw)
        px = cross_validate_simca_grid(SIMCA(verbose=False), X, y, _splitter(ids), **kw)
    for r, q in zip(obj["results"], px["results"]):
        assert (r["spec_px"], r["sens_px"], r["eff_px"]) == (q["spec"], q["sens"], q["eff"])
    assert "by_combo" not in obj
    calls = _fast_used(monkeypatch)
    with contextlib.redirect_stdout(io.StringIO()):
        slow = cross_validate_objects_grid(SIMCA(verbose=False), X.astype(np.float64), y, _splitter(ids),
                                           store_predictions=True, **kw)
    assert calls["n"] == 0
    assert set(slow) == set(obj) | {"by_combo"}
    G = np.unique(ids).size
    for r, s, b in zip(obj["results"], slow["results"], slow["by_combo"]):
        assert set(r) == set(s) and (r["params"], r["LV"]) == (s["params"], s["LV"])
        assert b["prediction"].shape == b["fraction"].shape == b["score"].shape == (G,)
        assert abs(r["spec"] - s["spec"]) <= 100.0 / 20 + 1e-9 and abs(r["sens"] - s["sens"]) <= 100.0 / 40 + 1e-9
    assert slow["best_estimator"].is_fitted_
