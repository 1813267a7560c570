"""PLS-DA on the host: the Gram-space recursion (ocm.plsda.pls_from_moments, the
kernels' oracle) against an explicit NIPALS that deflates X, against scikit-learn's
PLSRegression, the moment-space LDA tables against LinearDiscriminantAnalysis,
macro F1 from counts against f1_score, and the early stop.

Data (shared with test_gpu_plsda.py): one synth_spectra(n + m, p, 6, rank=16, seed) call split
into fit and test rows, y uniform over C classes, class c's rows shifted by sep·B_c with B_c a
unit-norm Gaussian band of width 0.05 at linspace(0.2, 0.8, C)[c].

Bounds: 1e-10 of the per-component maximum for everything that is the same arithmetic in another
order (measured 1.4e-14); the one-hot target against scikit-learn within 4 × the deviation the
test measures between scikit-learn and the exact NIPALS on the same case (scikit-learn's power
iteration stops at tol; that stop, about 5e-6, is its error and not this code's)."""
import functools

import numpy as np
import pytest

from ocm.plsda import lda_tables, macro_f1_from_counts, pls_from_moments
from oracle.simca_oracle import synth_spectra

A = 12
SHAPES = [(400, 37), (600, 64), (2000, 300)]
CLASSES = [2, 3, 4]
TARGETS = ["label", "onehot"]
BOUND = 1e-10


@functools.lru_cache(maxsize=None)
def plsda_data(n, m, p, C, sep, seed):
    """(X_fit, y_fit, X_test, y_test): float32-valued spectra, int64 labels 0..C−1 (read-only).
    The synthetic loadings are Gaussian bands on a p-point axis, which vanish at p < 8: narrower
    cases take the leading columns of 8."""
    pp = max(p, 8)
    X = synth_spectra(n + m, pp, 6, rank=16, seed=seed).astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    y = rng.integers(0, C, size=n + m)
    wl = np.linspace(0.0, 1.0, pp)
    for c, ctr in enumerate(np.linspace(0.2, 0.8, C)):
        B = np.exp(-0.5 * ((wl - ctr) / 0.05) ** 2)
        X[y == c] += sep * B / np.linalg.norm(B)
    X = X[:, :p].astype(np.float32)
    X.setflags(write=False)
    y.setflags(write=False)
    return X[:n], y[:n], X[n:], y[n:]


def targets(y, C, target):
    return y.astype(np.float64)[:, None] if target == "label" else np.eye(C)[y]


def standardise(X, Y):
    X = np.asarray(X, np.float64)
    xm, xs = X.mean(0), X.std(0, ddof=1)
    ym, ys = Y.mean(0), Y.std(0, ddof=1)
    xs[xs == 0] = 1.0
    ys[ys == 0] = 1.0
    return (X - xm) / xs, (Y - ym) / ys, xm, xs


def nipals_explicit(Xc, Yc, ncomp):
    """NIPALS that deflates X and Y explicitly, the weight vector being the exact first left
    singular vector of XᵀY (np.linalg.svd), sign as sklearn's _svd_flip_1d."""
    Xk, Yk = Xc.copy(), Yc.copy()
    n, p = Xc.shape
    W, P, T = np.zeros((ncomp, p)), np.zeros((ncomp, p)), np.zeros((n, ncomp))
    Q = np.zeros((ncomp, Yc.shape[1]))
    for a in range(ncomp):
        w = np.linalg.svd(Xk.T @ Yk, full_matrices=False)[0][:, 0]
        w = w * np.sign(w[np.argmax(np.abs(w))])
        t = Xk @ w
        tt = t @ t
        P[a], Q[a], W[a], T[:, a] = Xk.T @ t / tt, Yk.T @ t / tt, w, t
        Xk = Xk - np.outer(t, P[a])
        Yk = Yk - np.outer(t, Q[a])
    R = np.linalg.solve((P @ W.T).T, W)  # rows: the columns of Wᵀ (P Wᵀ)⁻¹, sklearn's x_rotations_
    return {"W": W, "P": P, "q": Q, "T": T, "tt": (T * T).sum(0), "R": R}


@functools.lru_cache(maxsize=None)
def case(n, p, C, target, sep=1.0):
    X, y, _, _ = plsda_data(n, 64, p, C, sep, 100 + p + C)
    Xc, Yc, xm, xs = standardise(X, targets(y, C, target))
    fit = pls_from_moments(Xc.T @ Xc, Xc.T @ Yc, A)
    return X, y, Xc, Yc, fit, nipals_explicit(Xc, Yc, A)


def rel_dev(got, want, axis):
    """max |got − want| per component over the component's max |want|."""
    return np.max(np.abs(got - want), axis=axis) / np.max(np.abs(want), axis=axis)


def deviations(Xc, fit, ref):
    d = {"T": rel_dev(Xc @ fit["R"].T, ref["T"], 0), "tt": np.abs(fit["tt"] - ref["tt"]) / ref["tt"]}
    for k in ("W", "P", "q"):
        d[k] = rel_dev(fit[k], ref[k], 1)
    return d


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n,p", SHAPES)
def test_moments_match_explicit_nipals(n, p, C, target):
    _, _, Xc, _, fit, ref = case(n, p, C, target)
    assert fit["ncomp"] == A
    for name, dev in deviations(Xc, fit, ref).items():
        print(f"{name}: max {dev.max():.3g}")
        assert dev.max() <= BOUND, (name, dev)
    T = Xc @ fit["R"].T
    off = T.T @ T - np.diag(fit["tt"])
    assert np.abs(off).max() <= BOUND * fit["tt"].max()


def sklearn_pls(Xc_raw, Y, ncomp):
    from sklearn.cross_decomposition import PLSRegression

    pls = PLSRegression(n_components=ncomp, tol=1e-12, max_iter=5000).fit(Xc_raw, Y)
    return {"W": pls.x_weights_.T, "P": pls.x_loadings_.T, "q": pls.y_loadings_.T,
            "T": pls.transform(Xc_raw), "R": pls.x_rotations_.T}


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n,p", SHAPES)
def test_label_target_matches_sklearn(n, p, C):
    X, y, Xc, _, fit, _ = case(n, p, C, "label")
    ref = sklearn_pls(X.astype(np.float64), y.astype(np.float64), A)
    ref["tt"] = (ref["T"] * ref["T"]).sum(0)
    for name, dev in deviations(Xc, fit, ref).items():
        print(f"{name}: max {dev.max():.3g}")
        assert dev.max() <= BOUND, (name, dev)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n,p", SHAPES)
def test_onehot_target_matches_sklearn_within_its_own_stop(n, p, C):
    X, y, Xc, _, fit, exact = case(n, p, C, "onehot")
    sk = sklearn_pls(X.astype(np.float64), np.eye(C)[y], A)
    sk["tt"] = (sk["T"] * sk["T"]).sum(0)
    own = deviations(Xc, exact, sk)  # scikit-learn against the exact NIPALS
    got = deviations(Xc, fit, sk)
    for name in got:
        print(f"{name}: ours {got[name].max():.3g}, sklearn's own {own[name].max():.3g}")
        assert got[name].max() <= 4 * own[name].max() + BOUND, name


def class_moments(T, y, C):
    nc = np.bincount(y, minlength=C).astype(np.float64)
    mc = np.stack([T[y == c].mean(0) for c in range(C)])
    return mc, nc


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("sep", [1.0, 0.3])
def test_lda_tables_predict_as_sklearn_lda(C, target, sep):
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis

    n, p = 600, 64
    _, y, Xc, _, fit, _ = case(n, p, C, target, sep)
    T = Xc @ fit["R"].T
    mc, nc = class_moments(T, y, C)
    lvs = list(range(1, A + 1))
    coef, icpt = lda_tables(fit["tt"], mc, nc, lvs)
    wrong = 0
    for l, a in enumerate(lvs):
        D = T[:, :a] @ coef[l, :, :a].T + icpt[l]
        ref = LinearDiscriminantAnalysis().fit(T[:, :a], y).predict(T[:, :a])
        wrong += int((np.argmax(D, 1) != ref).sum())
    assert wrong == 0


def test_macro_f1_from_counts_matches_sklearn():
    from sklearn.metrics import f1_score

    rng = np.random.default_rng(5)
    cases = []
    for C in (2, 3, 5):
        yt = rng.integers(0, C, 300)
        yp = np.where(rng.random(300) < 0.7, yt, rng.integers(0, C, 300))
        cases.append((C, yt, yp))
    yt = rng.integers(0, 3, 200)
    cases.append((3, yt, np.where(yt == 2, 0, yt)))                # class 2 is never predicted
    cases.append((4, rng.integers(0, 2, 100), rng.integers(0, 2, 100)))  # classes 2, 3 in neither
    cases.append((3, np.zeros(50, int), np.full(50, 1)))           # nothing right
    for C, yt, yp in cases:
        counts = np.zeros((C, C), np.int64)
        np.add.at(counts, (yt, yp), 1)
        want = f1_score(yt, yp, average="macro", zero_division=0)
        assert macro_f1_from_counts(counts) == pytest.approx(want, abs=1e-14)
    stack = np.zeros((2, 3, 3), np.int64)
    stack[0] = [[5, 1, 0], [2, 7, 0], [1, 1, 0]]
    stack[1] = np.diag([4, 4, 4])
    f = macro_f1_from_counts(stack)
    assert f.shape == (2,) and f[1] == 1.0


def one_component_moments(p):
    """Moments of a y that is the first score itself, in exact arithmetic: S = diag(4, 2, 1, 1, …),
    s = 4 e₁, so w = r = p₁ = e₁, tt = 4, q = 1 and s − tt p₁ q is exactly 0."""
    S = np.diag(np.r_[4.0, 2.0, np.ones(p - 2)])
    s = np.zeros((p, 1))
    s[0, 0] = 4.0
    return S, s


def test_early_stop_when_one_component_explains_y():
    S, s = one_component_moments(20)
    fit = pls_from_moments(S, s, 6)
    assert fit["ncomp"] == 1 and fit["tt"][0] == 4.0
    for k in ("W", "R", "P", "q"):
        assert fit[k][0].any() and not fit[k][1:].any()
    assert not fit["tt"][1:].any()
    p = 20
    fit0 = pls_from_moments(S, np.zeros((p, 2)), 3)  # a constant target: nothing to fit
    assert fit0["ncomp"] == 0 and not fit0["R"].any()


def test_longdouble_oracle_agrees():
    _, _, Xc, Yc, fit, _ = case(400, 37, 3, "onehot")
    ld = pls_from_moments(Xc.T @ Xc, Xc.T @ Yc, A, dtype=np.longdouble)
    assert ld["R"].dtype == np.longdouble
    assert rel_dev(fit["R"], ld["R"].astype(np.float64), 1).max() <= BOUND
