"""Robust calibration on the GPU (ocm_l1median_*, ocm_sphere_rows_*, ocm.robust,
the "chi2rob" limits) against the fp64 NumPy oracle of tests/robust_oracle.py.

Tolerances.  A Weiszfeld step is the same fp64 arithmetic on both sides in a
different summation order: reordering moves a sum of n positive terms by at
most n·2⁻⁵³ relative (1.1e-13 at n = 1024), the inputs lie in [0.5, 2], so the
step is compared at rtol 1e-12.  A converged median is compared with the
oracle's at tol = 1e-13: the step lengths contract by ≤ 0.49 per step on the
fixtures (tests/test_robust_host.py asserts it), so a stop at tol = 1e-9 lies
within tol·c/(1 − c) < 1e-9 of the median, bound 2e-9.  The float32 sphered rows
are one rounding of an fp64 value whose own error is a few 2⁻⁵³: within one ulp
of the dtype of the oracle rounded to it.  For float64 there is no finer oracle
to round, and two fp64 evaluations that differ in the order of Σ(x − m)² can be
2 ulp apart (measured: 2), so that case is bounded by the roundings of both
sides, (p + 10)·2⁻⁵³ relative (test_sphere_rows).

The spherical PCA's λ, h, q and f have no derivable tolerance: the sphered
rows are stored in float32 and their Gram's error reaches the loadings through
the eigengaps.  Two figures were measured on the ten fixtures, as the largest
relative difference over the fixtures and rows (λ: over the components):

    GPU against the oracle (MI355X)             λ 1.12e-6, h 7.23e-6, q 2.21e-6, f 1.72e-6
    the oracle with U rounded to float32        λ 4.6e-8, h 3.9e-7, q 7.4e-8, f 6.4e-8
      against itself with float64 U

and the tolerance is 8 × the larger of the two per quantity (the margin covers
ten fixtures being a small sample): λ 9.0e-6, h 5.8e-5, q 1.8e-5, f 1.4e-5.  The
device's share is float32 work: the scores and Q leave the scoring kernel in
float32 (2⁻²⁴ = 6e-8 a value, and h of a row near the centre is a small sum of
squares of such values)."""
import contextlib
import io

import numpy as np
import pytest
import torch
from scipy import stats

import robust_oracle as O
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

RTOL = 1e-12
NP_DT = {"f32": np.float32, "f64": np.float64}
TILE_LIMIT = {"f32": 2048, "f64": 1024}  # csrc/ocm_robust.hip: 16 rows · p elements ≤ 128 KiB stay in LDS

# largest relative GPU − oracle differences measured on the ten fixtures (MI355X), and the
# oracle's own float32-U gap (module docstring); the tolerance is 8 × the larger
PCA_MEASURED = {"lam": 1.12e-6, "h": 7.23e-6, "q": 2.21e-6, "f": 1.72e-6}
PCA_U32_GAP = {"lam": 4.6e-8, "h": 3.9e-7, "q": 7.4e-8, "f": 6.4e-8}
PCA_TOL = {key: 8.0 * max(PCA_MEASURED[key], PCA_U32_GAP[key]) for key in PCA_U32_GAP}


def on_device(Z, dt="f32", pad=0, lead=0):
    """Z on the device in the dtype: contiguous, or (pad > 0) columns
    [lead, lead + p) of a wider tensor whose other columns hold NaN."""
    t = torch.from_numpy(np.asarray(Z).astype(NP_DT[dt])).cuda()
    if pad == 0:
        return t
    n, p = t.shape
    buf = torch.full((n, p + pad), float("nan"), dtype=t.dtype, device="cuda")
    buf[:, lead:lead + p] = t
    Zd = buf[:, lead:lead + p]
    assert Zd.stride(0) == p + pad
    return Zd


def uniform(n, p, dt, seed):
    """(n, p) in [0.5, 2], rounded to the dtype, as float64."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, size=(n, p)).astype(NP_DT[dt]).astype(np.float64)


def one_step(Xd, start, rows=None):
    from ocm import engine

    c, info, d = engine.l1_median(Xd, rows, torch.from_numpy(np.asarray(start, dtype=np.float64)), 0.0, 1)
    return c.cpu().numpy(), info.cpu().numpy(), d.cpu().numpy()


def check_step(X64, got, start):
    c, info, d = got
    want, _ = O.weiszfeld_step(X64, start)
    np.testing.assert_allclose(c, want, rtol=RTOL)
    assert info[0] == 1.0
    np.testing.assert_allclose(info[2], np.linalg.norm(want - start), rtol=1e-10)
    dist = O.distances(X64, c)  # at the returned centre
    np.testing.assert_allclose(d, dist, rtol=RTOL)
    np.testing.assert_allclose(info[3], dist.sum(), rtol=RTOL)
    assert info[4] == float((dist == 0).sum())


# the chunk edge on both sides (256 rows), scalar / 8-byte / 16-byte loads, p not a multiple of 4,
# p above the LDS tile (2052 float32; 2052 and 1030 float64), more than 64 chunks (the group pass)
STEP_SHAPES = [(1, 1), (2, 3), (255, 5), (257, 4), (513, 130), (300, 2052), (40, 4100), (16700, 6)]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n,p", STEP_SHAPES + [(40, 1030)])
def test_one_weiszfeld_step(n, p, dt):
    X = uniform(n, p, dt, seed=n + p)
    start = np.random.default_rng(p).uniform(0.5, 2.0, size=p)
    check_step(X, one_step(on_device(X, dt), start), start)


def test_read_twice_path_is_taken():
    """The shapes above cross the LDS-tile limit of both dtypes."""
    for dt in ("f32", "f64"):
        ps = [p for _, p in STEP_SHAPES + [(40, 1030)]]
        assert any(p > TILE_LIMIT[dt] for p in ps) and any(p <= TILE_LIMIT[dt] for p in ps)
        assert any(n > 16 and p > TILE_LIMIT[dt] for n, p in STEP_SHAPES + [(40, 1030)])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("p,pad,lead", [(8, 3, 0), (8, 4, 0), (8, 4, 1), (130, 2, 0), (2052, 4, 0), (2052, 5, 2)])
def test_step_on_a_column_slice(p, pad, lead, dt):
    X = uniform(300, p, dt, seed=p + pad)
    start = X.mean(axis=0) + 0.05
    check_step(X, one_step(on_device(X, dt, pad, lead), start), start)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n,p", [(700, 12), (300, 2052)])
def test_step_on_a_shuffled_row_subset(n, p, dt):
    X = uniform(n, p, dt, seed=7)
    rows = np.random.default_rng(8).permutation(n)[:n // 2 + 3]
    start = X.mean(axis=0)
    c, info, d = one_step(on_device(X, dt, pad=4), start, torch.from_numpy(rows).cuda())
    check_step(X[rows], (c, info, d), start)
    assert d.shape == (rows.size,)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_coincident_rows(dt):
    from ocm import robust

    X = uniform(12, 5, dt, seed=3)
    X[2:9] = X[2]
    r = robust.l1_median(on_device(X, dt), start=X[2])
    np.testing.assert_array_equal(r.center.cpu().numpy(), X[2])  # bit for bit
    assert r.n_coincident == 7 and r.converged and r.n_iter == 1 and r.step == 0.0
    # one coincident row among generic rows: the Vardi–Zhang weight γ = 1/r < 1
    Y = uniform(9, 4, dt, seed=4)
    want, (_, eta, _, gamma, _) = O.weiszfeld_step(Y, Y[3])
    assert eta == 1 and 0.0 < gamma < 1.0
    c, info, _ = one_step(on_device(Y, dt), Y[3])
    np.testing.assert_allclose(c, want, rtol=RTOL)
    assert info[4] == 0.0  # none at the returned centre
    # every row on the centre
    Z = np.tile(Y[0], (3, 1))
    r = robust.l1_median(on_device(Z, dt), start=Y[0])
    np.testing.assert_array_equal(r.center.cpu().numpy(), Y[0])
    assert r.n_coincident == 3 and r.converged and r.objective == 0.0


@pytest.fixture(scope="module")
def refs():
    """The oracle's results on the ten fixtures, computed once."""
    out = {}
    for kind in O.KINDS:
        for seed in O.SEEDS:
            X, clean, B = O.make_fixture(kind, seed)
            out[kind, seed] = {"X": X, "clean": clean, "B": B, "exact": O.l1_median(X, tol=1e-13, max_iter=500),
                               "tol9": O.l1_median(X, tol=1e-9, max_iter=200), "screen": O.outlier_screen(X, 3)}
    return out


ALL_FIXTURES = [(kind, seed) for kind in O.KINDS for seed in O.SEEDS]


@pytest.mark.parametrize("kind,seed", ALL_FIXTURES)
def test_convergence_on_the_fixtures(refs, kind, seed):
    from ocm import robust

    ref = refs[kind, seed]
    r = robust.l1_median(torch.from_numpy(ref["X"]).cuda(), tol=1e-9, max_iter=200)
    m = r.center.cpu().numpy()
    exact = ref["exact"]["center"]
    print(f"{kind} {seed}: n_iter {r.n_iter} (oracle {ref['tol9']['n_iter']}), "
          f"|m - m*|/|m| = {np.linalg.norm(m - exact) / np.linalg.norm(m):.3e}, step {r.step:.3e}")
    assert r.converged
    assert np.linalg.norm(m - exact) <= 2e-9 * np.linalg.norm(m)
    assert abs(r.n_iter - ref["tol9"]["n_iter"]) <= 1 and r.n_iter < 30  # the done flag ended the work
    d = O.distances(ref["X"], m)
    np.testing.assert_allclose(r.distances.cpu().numpy(), d, rtol=RTOL)
    np.testing.assert_allclose(r.objective, d.sum(), rtol=RTOL)
    assert r.n_coincident == 0


@pytest.mark.parametrize("shape", ["fixture", "groups", "wide"])
def test_reproducible_bit_for_bit(shape):
    from ocm import engine

    if shape == "fixture":
        X = O.make_fixture("scatter", 0)[0]
    else:
        n, p = (16700, 6) if shape == "groups" else (300, 2052)
        X = uniform(n, p, "f32", seed=1) + np.random.default_rng(2).standard_normal((n, 1))
    Xd = torch.from_numpy(X.astype(np.float32)).cuda()
    start = engine.colmean(Xd, None, Xd.shape[0])
    runs = [engine.l1_median(Xd, None, start, 1e-9, 60) for _ in range(2)]
    torch.zeros(1 << 20, device="cuda").sum().item()  # other work in between
    runs.append(engine.l1_median(Xd, None, start, 1e-9, 60))
    for c, info, d in runs[1:]:
        assert torch.equal(c, runs[0][0]) and torch.equal(info, runs[0][1]) and torch.equal(d, runs[0][2])
    assert runs[0][1][1].item() == 1.0  # converged


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n,p,pad", [(257, 5, 0), (64, 130, 0), (9, 2052, 0), (33, 8, 3)])
def test_sphere_rows(n, p, pad, dt):
    from ocm import engine

    X = uniform(n, p, dt, seed=n)
    center = X[n // 2].copy()  # one row lies on the centre
    U, d = engine.sphere_rows(on_device(X, dt, pad), None, torch.from_numpy(center), want_dist=True)
    assert U.dtype == (torch.float32 if dt == "f32" else torch.float64) and tuple(U.shape) == (n, p)
    want, dist = O.sphere_rows(X, center)
    ref = want.astype(NP_DT[dt])
    got = U.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    if dt == "f32":  # the oracle rounded to the dtype: within one ulp of the dtype
        assert (err <= np.spacing(np.abs(ref)).astype(np.float64)).all()
    else:
        # float64 has no finer oracle to round: both sides carry fp64 rounding.  With u = 2⁻⁵³:
        # x − m one rounding (u), Σ of p squares in any order (p + 2)·u, its root half of that + u,
        # the reciprocal u, the product u: (p/2 + 5)·u a side, (p + 10)·u between the two
        assert (err <= (p + 10) * 2.0 ** -53 * np.abs(want)).all()
    assert dist[n // 2] == 0.0 and not got[n // 2].any()
    np.testing.assert_allclose(d.cpu().numpy(), dist, rtol=RTOL)
    rows = torch.from_numpy(np.random.default_rng(1).permutation(n)[:max(1, n // 3)]).cuda()
    U2, _ = engine.sphere_rows(on_device(X, dt, pad), rows, torch.from_numpy(center))
    assert torch.equal(U2, U[rows])


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))


@pytest.mark.parametrize("kind,seed", ALL_FIXTURES)
def test_screen_on_the_fixtures(refs, kind, seed):
    from ocm import engine, robust

    ref = refs[kind, seed]
    X, clean, want = ref["X"], ref["clean"], ref["screen"]
    Xd = torch.from_numpy(X).cuda()
    sc = robust.outlier_screen(Xd, 3)
    np.testing.assert_array_equal(sc.keep.cpu().numpy(), clean)
    cat = sc.category.cpu().numpy()
    assert cat.dtype == np.uint8
    np.testing.assert_array_equal(cat, want["category"])
    np.testing.assert_array_equal(sc.keep.cpu().numpy(), cat < 2)
    pca = sc.pca
    np.testing.assert_array_equal(pca.candidate_order.cpu().numpy(), want["model"]["order"])
    P = pca.components.cpu().numpy()
    np.testing.assert_allclose(P @ P.T, np.eye(3), atol=1e-9)
    robust_angle = O.subspace_angle_deg(P, ref["B"])
    if kind == "scatter":
        fit = engine.fit_class(Xd, None, X.shape[0], 3, 0, want_T=False)
        classical = O.subspace_angle_deg(fit.P64.cpu().numpy(), ref["B"])
        assert robust_angle <= classical / 10.0, (robust_angle, classical)
    h, q = pca.distances(Xd)
    figures = {"lam": rel(pca.explained_variance.cpu().numpy(), want["model"]["explained_variance"]),
               "h": rel(h.cpu().numpy(), want["h"]), "q": rel(q.cpu().numpy(), want["q"]),
               "f": rel(sc.f.cpu().numpy(), want["f"])}
    print(f"{kind} {seed}: angle {robust_angle:.2f} deg, GPU - oracle (relative): "
          + ", ".join(f"{key} {v:.2e}" for key, v in figures.items()))
    assert (sc.Nh, sc.Nq) == (want["Nh"], want["Nq"])
    assert sc.cut_extreme == pytest.approx(want["cut_extreme"], rel=RTOL)
    assert sc.cut_outlier == pytest.approx(want["cut_outlier"], rel=RTOL)
    np.testing.assert_allclose([sc.h0, sc.q0], [want["h0"], want["q0"]], rtol=max(PCA_TOL["h"], PCA_TOL["q"]))
    for key, v in figures.items():
        assert v <= PCA_TOL[key], (key, v, PCA_TOL[key])


def test_spherical_pca_api():
    from ocm import robust

    X, clean, B = O.make_fixture("cluster", 0)
    Xd = torch.from_numpy(X).cuda()
    full = robust.spherical_pca(Xd, 3)
    assert tuple(full.components.shape) == (3, 40) and full.components.dtype == torch.float64
    assert tuple(full.candidate_variance.shape) == (6,) and full.median.converged
    ev = full.explained_variance.cpu().numpy()
    assert (np.diff(ev) <= 0).all() and (ev > 0).all()
    # without spare candidates the cluster's direction is kept and the plane is lost
    tight = robust.spherical_pca(Xd, 3, n_candidates=3)
    assert O.subspace_angle_deg(tight.components.cpu().numpy(), B) > 45.0
    assert O.subspace_angle_deg(full.components.cpu().numpy(), B) < 10.0
    # rows: the clean rows alone, as a mask and as indices
    idx = np.flatnonzero(clean)
    a = robust.spherical_pca(Xd, 3, rows=clean)
    b = robust.spherical_pca(X, 3, rows=idx)  # NumPy in
    assert torch.equal(a.center, b.center) and torch.equal(a.explained_variance, b.explained_variance)
    h, q = a.distances(Xd, rows=idx[:50])
    h2, q2 = a.distances(Xd[idx[:50]])
    assert torch.equal(h, h2) and torch.equal(q, q2)
    # a constant direction has no robust variance
    Z = np.zeros((50, 4), dtype=np.float32)
    Z[:, 0] = np.random.default_rng(0).standard_normal(50)
    with pytest.raises(ValueError, match="positive robust variance"):
        robust.spherical_pca(Z, 2)


# ------------------------------------------------------------------ SIMCA with the robust limits

def _two_classes(seed=0, n0=300, n1=100, p=12):
    rng = np.random.default_rng(seed)
    B = np.linalg.qr(rng.standard_normal((p, 2)))[0].T
    X0 = 1.0 + (rng.standard_normal((n0, 2)) * [4.0, 2.0]) @ B + 0.1 * rng.standard_normal((n0, p))
    X0[:15] += rng.standard_normal((15, p)) * 3.0  # a few bad calibration rows
    X1 = 1.6 + (rng.standard_normal((n1, 2)) * [3.0, 3.0]) @ B + 0.3 * rng.standard_normal((n1, p))
    X = np.vstack([X0, X1]).astype(np.float32)
    y = np.r_[np.zeros(n0, np.int64), np.ones(n1, np.int64)]
    perm = rng.permutation(n0 + n1)
    return X[perm], y[perm]


DD_ROB = dict(model_class=0, type="dd", t2lim="chi2rob", qlim="chi2rob", t2cl=0.95, qcl=0.95, dcl=0.95,
              verbose=False)


def test_simca_dd_chi2rob_limits_and_predict():
    from utils.SIMCA import SIMCA

    X, y = _two_classes()
    with contextlib.redirect_stdout(io.StringIO()) as out:
        m = SIMCA(n_components=2, **DD_ROB).fit(X, y)
    assert "set as chi2pom" not in out.getvalue() and (m.t2lim, m.qlim) == ("chi2rob", "chi2rob")
    md = m._model[0]
    T2, Q = np.asarray(md["T2"]), np.asarray(md["Q"])
    assert T2.dtype == np.float64 and Q.dtype == np.float32 and T2.shape == (300,)
    t2l, Nh, h0 = O.chi2rob_limit(T2, 0.95)
    ql, Nq, q0 = O.chi2rob_limit(Q, 0.95)
    assert (m._t2dof, m._qdof) == (Nh, Nq)
    np.testing.assert_allclose([m._t2scfact, m._qscfact], [h0, q0], rtol=RTOL)
    np.testing.assert_allclose([md["T2_limit"], md["Q_limit"]], [t2l, ql], rtol=RTOL)
    np.testing.assert_allclose(md["D_limit"], stats.chi2.ppf(0.95, Nh + Nq), rtol=RTOL)
    df = m.decision_function(X)
    pred = np.asarray(m.predict(X))
    np.testing.assert_array_equal(pred.reshape(df.shape).astype(bool), df > 0)
    # the moment estimators are moved by the 15 bad rows, the robust ones are not
    with contextlib.redirect_stdout(io.StringIO()):
        pom = SIMCA(n_components=2, model_class=0, type="dd", verbose=False).fit(X, y)
    assert pom._qscfact > 2.0 * m._qscfact


def test_cv_grid_dd_chi2rob_equals_a_loop_of_fits(monkeypatch):
    from utils import SIMCA, ClasswiseKFoldWithExternalVal, cross_validate_simca_grid
    import ocm.cv as fe

    X, y = _two_classes(seed=1)
    assert X.shape[0] == 400
    calls = {"n": 0}
    orig = fe.cv_grid

    def wrapped(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)

    monkeypatch.setattr(fe, "cv_grid", wrapped)
    cv = ClasswiseKFoldWithExternalVal(n_splits=2, cls_label=0)
    grid = {"type": ["dd"], "t2lim": ["chi2rob"], "qlim": ["chi2rob"]}
    with contextlib.redirect_stdout(io.StringIO()):
        res = cross_validate_simca_grid(SIMCA(model_class=0, verbose=False), X, y, cv, LV_min=2, LV_max=3,
                                        param_grid=grid, print_summary=False, store_predictions=True)
    assert calls["n"] == 1  # the fold engine, not the generic loop
    assert [r["LV"] for r in res["results"]] == [2, 3]
    assert (res["best_estimator"].t2lim, res["best_estimator"].qlim) == ("chi2rob", "chi2rob")
    for rec, by in zip(res["results"], res["by_combo"]):
        pooled = np.zeros(X.shape[0])
        margin = np.zeros(X.shape[0])
        spec = []
        for fit_rows, test_rows in cv.split(X, y):
            with contextlib.redirect_stdout(io.StringIO()):
                m = SIMCA(n_components=rec["LV"], **DD_ROB).fit(X[fit_rows], y[fit_rows])
            df = m.decision_function(X[test_rows])[:, 0]
            pooled[test_rows] = df > 0
            margin[test_rows] = np.abs(df) / m._model[0]["D_limit"]
            other = y[test_rows] != 0
            spec.append(100.0 * np.mean(~(df[other] > 0)))
        diff = by["prediction"] != pooled
        # the fold engine's Grams are downdated, the loop's are fresh: a decision may
        # differ only for a row on the boundary, |D_limit − dred| < 1e-4·D_limit
        assert (margin[diff] < 1e-4).all(), (int(diff.sum()), margin[diff])
        if not diff.any():
            assert rec["spec"] == pytest.approx(np.mean(spec), abs=1e-9)
