"""Host side of robust calibration: the NumPy oracle of tests/robust_oracle.py
against a literal transcription, limits.robust_dof and the "chi2rob" limits,
the dd override, ocm.robust's argument checks, and the preconditions of the
fixtures the GPU tests use (so that a GPU failure cannot hide in the inputs).
No device: SIMCA's device entry points are tests/fake_engine.py."""
import math
import sys

import numpy as np
import pytest
from scipy import stats

import fake_engine
import robust_oracle as O


# ------------------------------------------------------------------ the oracle against a literal transcription

def _literal_step(X, m):
    """The step of include/ocm.h spelled out with loops."""
    n, p = len(X), len(m)
    W, eta, S = 0.0, 0, [0.0] * p
    for i in range(n):
        d = math.sqrt(sum((float(X[i][j]) - m[j]) ** 2 for j in range(p)))
        if d == 0.0:
            eta += 1
            continue
        W += 1.0 / d
        for j in range(p):
            S[j] += float(X[i][j]) * (1.0 / d)
    R = [S[j] - W * m[j] for j in range(p)]
    r = math.sqrt(sum(v * v for v in R))
    gamma = 0.0 if eta == 0 else (1.0 if r == 0.0 else min(1.0, eta / r))
    if gamma == 1.0 or W == 0.0:
        return list(m)
    return [(1.0 - gamma) * (S[j] / W) + gamma * m[j] for j in range(p)]


@pytest.mark.parametrize("n,p,seed", [(1, 1, 0), (2, 3, 1), (7, 4, 2), (12, 5, 3)])
def test_oracle_step_vs_literal(n, p, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.5, 2.0, size=(n, p))
    m = X.mean(axis=0) + 0.1
    got, _ = O.weiszfeld_step(X, m)
    np.testing.assert_allclose(got, _literal_step(X.tolist(), m.tolist()), rtol=1e-14)


def test_oracle_step_coincident_rows():
    rng = np.random.default_rng(5)
    X = rng.uniform(0.5, 2.0, size=(12, 5))
    X[:7] = X[0]
    got, (W, eta, r, gamma, _) = O.weiszfeld_step(X, X[0])
    assert eta == 7 and gamma == 1.0 and r <= 5.0
    np.testing.assert_array_equal(got, X[0])
    np.testing.assert_array_equal(got, _literal_step(X.tolist(), X[0].tolist()))
    # one coincident row among generic rows: γ = 1/r < 1, the centre moves
    Y = rng.uniform(0.5, 2.0, size=(9, 4))
    got, (W, eta, r, gamma, _) = O.weiszfeld_step(Y, Y[3])
    assert eta == 1 and 0.0 < gamma < 1.0
    np.testing.assert_allclose(got, _literal_step(Y.tolist(), Y[3].tolist()), rtol=1e-14)
    # every row on the centre: it stays
    Z = np.tile(Y[0], (3, 1))
    got, (W, eta, _, gamma, _) = O.weiszfeld_step(Z, Y[0])
    assert W == 0.0 and eta == 3 and gamma == 1.0
    np.testing.assert_array_equal(got, Y[0])


def test_oracle_median_is_a_minimum():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((40, 3)) * [3.0, 1.0, 0.2] + 1.0
    r = O.l1_median(X, tol=1e-13, max_iter=500)
    assert r["converged"]
    U, d = O.sphere_rows(X, r["center"])
    assert np.abs(U.sum(axis=0)).max() < 1e-9  # Σ u_i = 0 at the L1 median
    np.testing.assert_allclose(np.sqrt((U * U).sum(axis=1)), 1.0, rtol=1e-14)
    for _ in range(20):
        assert O.distances(X, r["center"] + 1e-3 * rng.standard_normal(3)).sum() > r["objective"]
    assert r["objective"] == d.sum()


def test_oracle_mad_variance_of_a_normal_sample():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((20000, 4)) * [4.0, 2.0, 1.0, 0.5]
    m = O.spherical_pca(X, 2)
    np.testing.assert_allclose(m["explained_variance"], [16.0, 4.0], rtol=0.06)
    assert O.subspace_angle_deg(m["components"], np.eye(4)[:2]) < 2.0


# ------------------------------------------------------------------ limits.robust_dof, "chi2rob"

@pytest.mark.parametrize("N", [1, 2, 5, 12, 40])
def test_robust_dof_recovers_chi2_samples(N):
    from ocm import limits

    u = stats.chi2.rvs(N, size=20000, random_state=1) * 3.0 / N
    q1, M, q3 = np.percentile(u, [25, 50, 75])
    got_N, got_u0 = limits.robust_dof(M, q3 - q1)
    assert abs(got_N - N) <= 1
    assert abs(got_u0 - 3.0) <= 0.02 * 3.0
    assert (got_N, got_u0) == pytest.approx(O.robust_dof(M, q3 - q1), rel=1e-13)


def test_robust_ratio_strictly_decreasing():
    from ocm import limits

    r = np.array([limits.robust_ratio(N) for N in range(1, limits.ROBUST_DOF_MAX + 1)])
    assert r.size == 250 and (np.diff(r) < 0).all()
    np.testing.assert_allclose(r, [O.chi2_ratio(N) for N in range(1, 251)], rtol=1e-15)
    # the ends of the table: a ratio beyond either end gives the end
    assert limits.robust_dof(1.0, 10.0)[0] == 1
    assert limits.robust_dof(1.0, 1e-3)[0] == 250
    with pytest.raises(ValueError):
        limits.robust_dof(0.0, 1.0)


class _Est:
    def __init__(self, **kw):
        self.type, self.t2lim, self.qlim = "dd", "chi2rob", "chi2rob"
        self.t2cl, self.qcl, self.dcl = 0.95, 0.9, 0.99
        self.__dict__.update(kw)


def _moments(u):
    from ocm import limits

    return limits.Moments(len(u), float(np.sum(u)), float(np.sum(u * u)), lambda pct: float(np.percentile(u, pct)))


def test_chi2rob_limits_vs_scipy():
    from ocm import limits

    rng = np.random.default_rng(3)
    h = stats.chi2.rvs(3, size=501, random_state=4) * 0.7
    q = stats.chi2.rvs(9, size=501, random_state=5) * 2e-3
    h[:25] *= 50.0  # outlying rows move the moments, hardly the quartiles
    est = _Est()
    t2l = limits.t2_limit(est, _moments(h), 3)
    ql = limits.q_limit(est, _moments(q), (0.0, 0.0, 0.0))
    dl = limits.critic_distance(est, t2l, ql, (0.0, 0.0, 0.0), 3)
    for u, cl, lim, dof, sc in ((h, 0.95, t2l, est._t2dof, est._t2scfact), (q, 0.9, ql, est._qdof, est._qscfact)):
        q1, M, q3 = np.percentile(u, [25, 50, 75])
        S = q3 - q1
        ratios = [(stats.chi2.ppf(.75, N) - stats.chi2.ppf(.25, N)) / stats.chi2.ppf(.5, N) for N in range(1, 251)]
        N = 1 + int(np.argmin(np.abs(np.array(ratios) - S / M)))
        u0 = 0.5 * N * (M / stats.chi2.ppf(.5, N) + S / (stats.chi2.ppf(.75, N) - stats.chi2.ppf(.25, N)))
        assert dof == N
        assert sc == pytest.approx(u0, rel=1e-14)
        assert lim == pytest.approx(u0 * stats.chi2.ppf(cl, N) / N, rel=1e-14)
        assert (lim, dof, sc) == pytest.approx(O.chi2rob_limit(u, cl), rel=1e-13)
    assert dl == stats.chi2.ppf(0.99, est._t2dof + est._qdof)
    assert abs(est._t2dof - 3) <= 1  # the 5 % of inflated rows do not move it
    pom = _Est(t2lim="chi2pom")
    limits.t2_limit(pom, _moments(h), 3)
    assert pom._t2dof == 1 and pom._t2scfact > 2.0 * est._t2scfact  # the moment estimators give way
    assert rng is not None


# ------------------------------------------------------------------ the dd override

OTHER_NAMES = ["perc", "Fdist", "Fdistrig", "chi2", "chi2pom", "jm", "chi2box", "nonsense"]


@pytest.mark.parametrize("t2lim,qlim", [("chi2rob", "chi2rob"), ("chi2rob", "jm"), ("Fdist", "chi2rob")])
def test_cv_spec_dd_keeps_chi2rob(t2lim, qlim):
    from ocm.cv import _Spec

    s = _Spec({"type": "dd", "t2lim": t2lim, "qlim": qlim})
    assert s.t2lim == (t2lim if t2lim == "chi2rob" else "chi2pom")
    assert s.qlim == (qlim if qlim == "chi2rob" else "chi2pom")
    assert s.needs_train_stats() and s.needs_percentile()


@pytest.mark.parametrize("name", OTHER_NAMES)
def test_cv_spec_dd_forces_chi2pom_over_other_names(name):
    from ocm.cv import _Spec

    s = _Spec({"type": "dd", "t2lim": name, "qlim": name})
    assert (s.t2lim, s.qlim) == ("chi2pom", "chi2pom")
    assert s.needs_train_stats() and not s.needs_percentile()
    a = _Spec({"type": "alt", "t2lim": "chi2rob", "qlim": "jm"})
    assert (a.t2lim, a.qlim) == ("chi2rob", "jm") and a.needs_percentile()


@pytest.fixture
def fake():
    import ocm.cv as ocv
    import ocm.engine as real
    import utils.SIMCA  # noqa: F401

    mod = sys.modules["utils.SIMCA"]
    mod.engine, ocv.engine = fake_engine, fake_engine
    yield
    mod.engine, ocv.engine = real, real


def _class_data(seed=0, n=300, p=12):
    rng = np.random.default_rng(seed)
    B = np.linalg.qr(rng.standard_normal((p, 2)))[0].T
    X = 1.0 + (rng.standard_normal((n, 2)) * [4.0, 2.0]) @ B + 0.1 * rng.standard_normal((n, p))
    return X.astype(np.float32), np.zeros(n, dtype=np.int64)


def test_simca_dd_keeps_chi2rob_and_fits(fake, capsys):
    from utils.SIMCA import SIMCA

    X, y = _class_data()
    m = SIMCA(n_components=2, model_class=0, type="dd", t2lim="chi2rob", qlim="chi2rob", verbose=False).fit(X, y)
    assert (m.t2lim, m.qlim) == ("chi2rob", "chi2rob")
    assert "set as chi2pom" not in capsys.readouterr().out
    md = m._model[0]
    T2, Q = np.asarray(md["T2"], dtype=np.float64), np.asarray(md["Q"])
    t2l, Nh, h0 = O.chi2rob_limit(T2, 0.95)
    ql, Nq, q0 = O.chi2rob_limit(Q, 0.95)
    assert (m._t2dof, m._qdof) == (Nh, Nq)
    assert md["T2_limit"] == pytest.approx(t2l, rel=1e-12)
    assert md["Q_limit"] == pytest.approx(ql, rel=1e-12)
    assert md["D_limit"] == pytest.approx(stats.chi2.ppf(0.95, Nh + Nq), rel=1e-12)


@pytest.mark.parametrize("name", OTHER_NAMES)
def test_simca_dd_forces_chi2pom_over_other_names(fake, capsys, name):
    from utils.SIMCA import SIMCA

    X, y = _class_data(1)
    m = SIMCA(n_components=2, model_class=0, type="dd", t2lim=name, qlim=name, verbose=False).fit(X, y)
    assert (m.t2lim, m.qlim) == ("chi2pom", "chi2pom")
    out = capsys.readouterr().out
    assert ("t2lim set as chi2pom" in out) == (name != "chi2pom")
    # one of the two robust: the other is still forced
    m = SIMCA(n_components=2, model_class=0, type="dd", t2lim="chi2rob", qlim=name, verbose=False).fit(X, y)
    assert (m.t2lim, m.qlim) == ("chi2rob", "chi2pom")


# ------------------------------------------------------------------ ocm.robust: argument errors, no device

def test_robust_argument_errors_need_no_device(monkeypatch):
    from ocm import engine, robust

    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(engine, "require_device", no_device)
    monkeypatch.setattr(engine, "as_device_x", no_device)
    X = np.ones((10, 4), dtype=np.float32)
    bad_l1 = [dict(X=np.ones(4)), dict(X=np.ones((0, 4))), dict(rows=[0, 10]), dict(rows=[-1]), dict(rows=[]),
              dict(rows=np.ones(9, bool)), dict(rows=[0.5]), dict(start=np.zeros(3)), dict(tol=-1.0),
              dict(tol=float("nan")), dict(tol="x"), dict(max_iter=-1), dict(max_iter=1.5), dict(max_iter=100001)]
    for kw in bad_l1:
        with pytest.raises(ValueError):
            robust.l1_median(**{"X": X, **kw})
    bad_pca = [dict(n_components=0), dict(n_components=5), dict(n_components=1.5), dict(n_components=2, rows=[0, 1]),
               dict(n_components=2, n_candidates=1), dict(n_components=2, n_candidates=5),
               dict(n_components=2, n_candidates=2.5), dict(n_components=2, rows=[0, 99])]
    for kw in bad_pca:
        with pytest.raises(ValueError):
            robust.spherical_pca(X, **kw)
        with pytest.raises(ValueError):
            robust.outlier_screen(X, **kw)
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(gamma=0.0), dict(gamma=1.5), dict(alpha="a")):
        with pytest.raises(ValueError):
            robust.outlier_screen(X, 2, **kw)
    # good arguments get as far as the device
    with pytest.raises(AssertionError, match="a device was asked for"):
        robust.l1_median(X, rows=np.arange(5), start=np.zeros(4))
    with pytest.raises(AssertionError, match="a device was asked for"):
        robust.outlier_screen(X, 2, n_candidates=3)


def test_default_candidates():
    from ocm import robust

    X = np.ones((10, 4))
    assert robust._check_pca(X, 1, None, None)[3:] == (1, 2)
    assert robust._check_pca(X, 3, None, None)[3:] == (3, 4)          # p caps it
    assert robust._check_pca(X, 2, None, [0, 1, 2])[3:] == (2, 2)     # n − 1 caps it
    assert O.default_candidates(3, 10, 4) == 4 and O.default_candidates(2, 3, 4) == 2


# ------------------------------------------------------------------ fixture preconditions

@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for kind in O.KINDS:
        for seed in O.SEEDS:
            X, clean, B = O.make_fixture(kind, seed)
            out[kind, seed] = (X, clean, B, O.outlier_screen(X, 3))
    return out


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("seed", O.SEEDS)
def test_fixture_screen_keeps_exactly_the_clean_rows(fixtures, kind, seed):
    X, clean, B, sc = fixtures[kind, seed]
    assert X.dtype == np.float32 and X.shape == (600, 40) and clean.sum() == 480
    np.testing.assert_array_equal(sc["keep"], clean)
    assert (sc["category"][~clean] == 2).all()
    # the planted rows lie far beyond the cut, the clean rows inside it
    assert (sc["f"][~clean] / sc["cut_outlier"]).min() > 20.0
    assert (sc["f"][clean] / sc["cut_outlier"]).max() < 0.95
    if kind == "cluster":  # the cluster's direction is a candidate, and is dropped
        assert sorted(sc["model"]["order"].tolist()) != [0, 1, 2]


@pytest.mark.parametrize("seed", O.SEEDS)
def test_fixture_robust_angle_vs_classical(fixtures, seed):
    X, clean, B, sc = fixtures["scatter", seed]
    robust = O.subspace_angle_deg(sc["model"]["components"], B)
    classical = O.subspace_angle_deg(O.classical_pca(X, 3), B)
    assert robust <= classical / 10.0
    assert robust < 2.0 and classical > 60.0


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("seed", O.SEEDS)
def test_fixture_weiszfeld_contracts(kind, seed):
    """The GPU test's bound on ‖m − m*‖ rests on the step lengths contracting by
    at most 0.49 per step: a stop at tol lies within tol·c/(1 − c) < tol."""
    X = O.make_fixture(kind, seed)[0]
    r = O.l1_median(X, tol=1e-13, max_iter=500)
    assert r["converged"]
    st = np.array(r["steps"])
    st = st[st > 1e-11 * np.linalg.norm(r["center"])]  # above the rounding floor
    assert (st[1:] / st[:-1]).max() <= 0.49
    assert 15 <= O.l1_median(X, tol=1e-9)["n_iter"] <= 23
