"""NumPy float64 reference of the element-wise PCA cross-validation
(ocm/pcacv.py, include/ocm.h ocm_press_*): the closed form, the brute-force
variable-deleted least squares it replaces, the Gram identity of the row-wise
sums, the full k-fold CV with an SVD per fold, and the fixtures the host and
GPU tests share."""
import functools

import numpy as np

DEGENERATE = 1e-8


def leverage_weights(P, k):
    """w_k[j] = 1/(1 − h_j)², h_j = Σ_{a<k} P_aj²; 0 (and counted) where 1 − h ≤ 1e-8."""
    P = np.asarray(P, dtype=np.float64)
    h = (P[:k] ** 2).sum(axis=0) if k else np.zeros(P.shape[1])
    d = 1.0 - h
    ok = d > DEGENERATE
    w = np.zeros_like(d)
    w[ok] = 1.0 / d[ok] ** 2
    return w, int((~ok).sum()), h


def press_closed(X, P, mu, exclude=None):
    """(press, naive, ndegen), each K + 1: PRESS_k = Σ_rows Σ_j (r_j/(1 − h_j))²
    with the explicit residual r = y − Σ_{a≤k} t_a·P_a.  ``exclude``: a variable
    left out of press[k] for k ≥ 1 by hand (no weight rule involved)."""
    P = np.asarray(P, dtype=np.float64)
    K, p = P.shape
    Y = np.asarray(X, dtype=np.float64) - np.asarray(mu, dtype=np.float64)
    T = Y @ P.T
    press, naive, nd = np.zeros(K + 1), np.zeros(K + 1), np.zeros(K + 1, dtype=np.int64)
    R = Y.copy()
    for k in range(K + 1):
        if k:
            R = R - np.outer(T[:, k - 1], P[k - 1])
        col = (R * R).sum(axis=0)
        naive[k] = col.sum()
        if exclude is not None and k >= 1:
            keep = np.arange(p) != exclude
            h = (P[:k, keep] ** 2).sum(axis=0)
            press[k] = (col[keep] / (1.0 - h) ** 2).sum()
        else:
            w, nd[k], _ = leverage_weights(P, k)
            press[k] = (w * col).sum()
    return press, naive, nd


def press_brute(X, P, mu):
    """PRESS_k by the definition: for every variable j fit the scores by least
    squares to the other p − 1 variables (loadings with column j deleted) and
    predict y_j from them."""
    P = np.asarray(P, dtype=np.float64)
    K, p = P.shape
    Y = np.asarray(X, dtype=np.float64) - np.asarray(mu, dtype=np.float64)
    press = np.zeros(K + 1)
    press[0] = (Y * Y).sum()
    for k in range(1, K + 1):
        Pk = P[:k]
        for j in range(p):
            keep = np.arange(p) != j
            t = np.linalg.lstsq(Pk[:, keep].T, Y[:, keep].T, rcond=None)[0]  # (k, rows)
            e = Y[:, j] - Pk[:, j] @ t
            press[k] += (e * e).sum()
    return press


def press_gram(X, P, mu):
    """(press, naive) from the scatter S = YᵀY alone:
    Σ_rows (r_j⁽ᵏ⁾)² = [(I − Π_k) S (I − Π_k)]_jj, Π_k = P_kᵀP_k."""
    P = np.asarray(P, dtype=np.float64)
    K, p = P.shape
    Y = np.asarray(X, dtype=np.float64) - np.asarray(mu, dtype=np.float64)
    S = Y.T @ Y
    press, naive = np.zeros(K + 1), np.zeros(K + 1)
    for k in range(K + 1):
        A = np.eye(p) - P[:k].T @ P[:k]
        col = np.diag(A @ S @ A)
        w, _, _ = leverage_weights(P, k)
        naive[k] = col.sum()
        press[k] = (w * col).sum()
    return press, naive


def f32_error_bound(X, P, mu):
    """Worst-case relative error of press[k] (largest over k) when the residual
    is formed in float32, to first order, with u = 2⁻²⁴ per rounding: the casts of
    μ, P and t (u·|μ_j|, and 2u·|t_a·P_aj| with the product's own rounding 3u),
    the subtraction x − μ (u·|y_j|, twice with the cast of x's partner) and every
    update r ← r − t_a·P_aj (u·|r_j|) give |δr_j| ≤ δ_j, and
    |δ PRESS_k| ≤ Σ_rows Σ_j w_k[j]·2·|r_j|·δ_j.  It grows like |y_j|/|r_j|: a
    variable the model reproduces almost alone (h_j → 1) has a tiny residual and a
    huge weight.  The tests pick float32 inputs whose bound is inside the
    tolerance, so a failure is the kernel's and not the format's."""
    u = 2.0 ** -24
    P = np.asarray(P, dtype=np.float64)
    Y = np.asarray(X, dtype=np.float64) - mu
    T = Y @ P.T
    R = Y.copy()
    delta = u * np.abs(mu) + 2 * u * np.abs(Y)
    worst = 0.0
    for k in range(1, P.shape[0] + 1):
        tp = np.outer(T[:, k - 1], P[k - 1])
        R = R - tp
        delta = delta + 3 * u * np.abs(tp) + u * np.abs(R)
        w = leverage_weights(P, k)[0]
        worst = max(worst, float((w * 2 * np.abs(R) * delta).sum() / (w * R * R).sum()))
    return worst


def kfold(n, nfolds):
    """scikit-learn's KFold without shuffling: contiguous folds, the first n % nfolds one longer."""
    sizes = np.full(nfolds, n // nfolds, dtype=np.int64)
    sizes[: n % nfolds] += 1
    stops = np.cumsum(sizes)
    return [np.arange(b - s, b, dtype=np.int64) for s, b in zip(sizes, stops)]


def pca_model(Xtrain, K):
    """(μ, P) of the training rows: mean and the leading K right singular vectors."""
    Xt = np.asarray(Xtrain, dtype=np.float64)
    mu = Xt.mean(axis=0)
    P = np.linalg.svd(Xt - mu, full_matrices=False)[2][:K]
    return mu, np.ascontiguousarray(P)


def full_cv(X, K, folds, fn=press_closed):
    """The whole cross-validation on the host: an SVD per fold, ``fn`` on the
    held-out rows.  Returns (press, naive, press_folds, models, max leverage)."""
    X = np.asarray(X, dtype=np.float64)
    allr = np.concatenate(folds)
    pf, nv, models, hmax = [], np.zeros(K + 1), [], 0.0
    for f in folds:
        train = np.setdiff1d(allr, f)
        mu, P = pca_model(X[train], K)
        out = fn(X[f], P, mu)
        pf.append(out[0] if isinstance(out, tuple) else out)
        if isinstance(out, tuple):
            nv += out[1]
        models.append((mu, P))
        hmax = max(hmax, float((P ** 2).sum(axis=0).max()))
    pf = np.asarray(pf)
    return pf.sum(axis=0), nv, pf, models, hmax


def lowrank(n, p, rank, seed, noise=0.1, dtype=np.float64, row_seed=0):
    """n rows of a rank-``rank`` signal (orthonormal loadings spread over all
    variables, score scales 2 → 1 times √p, so a variable's signal is of order
    √rank) plus a mean of order 1 plus white noise of deviation ``noise``.
    ``seed`` fixes the loadings and the mean, (seed, row_seed) the rows."""
    rng = np.random.default_rng(seed)
    L = np.linalg.qr(rng.standard_normal((p, rank)))[0].T
    mean = 1.0 + 0.25 * rng.standard_normal(p)
    s = np.sqrt(p) * np.linspace(2.0, 1.0, rank)
    rng = np.random.default_rng([seed, row_seed])
    X = (rng.standard_normal((n, rank)) * s) @ L + mean
    X += noise * rng.standard_normal((n, p))
    return np.ascontiguousarray(X.astype(dtype))


# (n, p, true rank): the shapes of the host check; the first two are the GPU end-to-end fixtures
SHAPES = ((240, 24, 4), (600, 40, 6), (300, 33, 5))
NFOLDS = 4
EXTRA = 4  # components past the true rank: K = rank + EXTRA


@functools.lru_cache(maxsize=None)
def fixture(n, p, rank, seed=0, dtype="float64"):
    """(X, K, folds, reference) of one end-to-end fixture; the reference is the
    full float64 CV of the array the device is given (after the cast to dtype)."""
    X = lowrank(n, p, rank, 100 + seed, dtype=np.dtype(dtype))
    X.setflags(write=False)
    K = rank + EXTRA
    folds = kfold(n, NFOLDS)
    ref = full_cv(X, K, folds)
    return X, K, folds, ref


KERNEL_NOISE = 0.5  # the kernel-level inputs need no sharp rank, only a benign |y|/|r|


@functools.lru_cache(maxsize=None)
def kernel_case(m, p, K, dtype="float32"):
    """(X, μ, P) of one kernel-level case: μ and P from the SVD of a training set
    (rank min(4, p − 1) plus noise), X = m rows the model has not seen.  The seed
    is the first whose float32 worst-case bound is at most half the float32
    tolerance of 1e-4 (``f32_error_bound``); the float64 runs share it."""
    r = min(4, p - 1)
    for seed in range(16):
        mu, P = pca_model(lowrank(max(2 * K, 96), p, r, 7 + seed, noise=KERNEL_NOISE), K)
        X32 = lowrank(m, p, r, 7 + seed, noise=KERNEL_NOISE, dtype=np.float32, row_seed=1)
        if m == 0 or f32_error_bound(X32, P, mu) <= 0.5e-4:
            X = X32 if np.dtype(dtype) == np.float32 else \
                lowrank(m, p, r, 7 + seed, noise=KERNEL_NOISE, dtype=np.float64, row_seed=1)
            return np.ascontiguousarray(X), mu, P
    raise AssertionError(f"no well-conditioned float32 case for m={m} p={p} K={K}")
