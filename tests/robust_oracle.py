"""float64 NumPy oracle of ocm.robust (the L1 median, spherical PCA, the outlier
screen) and of limits.robust_dof / the "chi2rob" limits, written from the
definitions in include/ocm.h and ocm/robust.py, and the fixtures the robust
tests share.  No device, no ocm import."""
import numpy as np
from scipy import stats

MAD_SCALE = 1.4826


# ------------------------------------------------------------------ the L1 median

def weiszfeld_step(X, m):
    """One Vardi–Zhang step from m: (m⁺, info) with info = (W, η, r, γ, Σd)."""
    X = np.asarray(X, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    D = X - m
    d = np.sqrt((D * D).sum(axis=1))
    nz = d > 0
    eta = int((~nz).sum())
    w = np.zeros_like(d)
    w[nz] = 1.0 / d[nz]
    W = w.sum()
    S = (X[nz] * w[nz, None]).sum(axis=0)
    R = S - W * m
    r = np.sqrt((R * R).sum())
    if eta == 0:
        gamma = 0.0
    elif r == 0.0:
        gamma = 1.0
    else:
        gamma = min(1.0, eta / r)
    if gamma == 1.0 or W == 0.0:
        mp = m.copy()
    else:
        mp = (1.0 - gamma) * (S / W) + gamma * m
    return mp, (W, eta, r, gamma, d.sum())


def distances(X, m):
    D = np.asarray(X, dtype=np.float64) - np.asarray(m, dtype=np.float64)
    return np.sqrt((D * D).sum(axis=1))


def l1_median(X, start=None, tol=1e-9, max_iter=200):
    """dict(center, n_iter, converged, step, objective, n_coincident, distances, steps)."""
    X = np.asarray(X, dtype=np.float64)
    m = X.mean(axis=0) if start is None else np.asarray(start, dtype=np.float64).copy()
    n_iter, conv, step, steps = 0, False, 0.0, []
    for it in range(max_iter):
        mp, _ = weiszfeld_step(X, m)
        step = float(np.sqrt(((mp - m) ** 2).sum()))
        steps.append(step)
        m = mp
        n_iter = it + 1
        if step <= tol * np.sqrt((m * m).sum()):
            conv = True
            break
    d = distances(X, m)
    return {"center": m, "n_iter": n_iter, "converged": conv, "step": step, "objective": float(d.sum()),
            "n_coincident": int((d == 0).sum()), "distances": d, "steps": steps}


def sphere_rows(X, m):
    """U (fp64) with u_i = (x_i − m)·(1/‖x_i − m‖), zeros where the distance is 0."""
    D = np.asarray(X, dtype=np.float64) - np.asarray(m, dtype=np.float64)
    d = np.sqrt((D * D).sum(axis=1))
    w = np.zeros_like(d)
    w[d > 0] = 1.0 / d[d > 0]
    return D * w[:, None], d


# ------------------------------------------------------------------ spherical PCA

def default_candidates(k, n, p):
    return min(2 * k, n - 1, p)


def spherical_pca(X, k, n_candidates=None, center=None, round_u=None):
    """dict(center, components (k, p), explained_variance (k,), candidate_variance,
    order).  ``round_u``: a dtype U is rounded to before the Gram (the device
    stores U in the input dtype)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    kc = default_candidates(k, n, p) if n_candidates is None else int(n_candidates)
    m = l1_median(X, tol=1e-13, max_iter=500)["center"] if center is None else np.asarray(center, np.float64)
    U, _ = sphere_rows(X, m)
    if round_u is not None:
        U = U.astype(round_u).astype(np.float64)
    G = U.T @ U / n
    lam_g, V = np.linalg.eigh(G)
    V = V[:, ::-1][:, :kc].T  # (kc, p), descending eigenvalue
    T = (X - m) @ V.T
    med = np.median(T, axis=0)
    mad = np.median(np.abs(T - med), axis=0)
    lam = (MAD_SCALE * mad) ** 2
    order = np.argsort(-lam, kind="stable")
    if int((lam > 0).sum()) < k:
        raise ValueError("fewer than k candidates with a positive robust variance")
    keep = order[:k]
    return {"center": m, "components": V[keep], "explained_variance": lam[keep], "candidate_variance": lam,
            "order": keep}


def pca_distances(X, model):
    """(h, q) of the rows of X in a spherical_pca model."""
    Xc = np.asarray(X, dtype=np.float64) - model["center"]
    P = model["components"]
    T = Xc @ P.T
    h = (T * T / model["explained_variance"]).sum(axis=1)
    E = Xc - T @ P
    return h, (E * E).sum(axis=1)


# ------------------------------------------------------------------ robust data-driven limits

DOF_MAX = 250


def chi2_ratio(N):
    return (stats.chi2.ppf(0.75, N) - stats.chi2.ppf(0.25, N)) / stats.chi2.ppf(0.5, N)


def robust_dof(M, S):
    Ns = np.arange(1, DOF_MAX + 1)
    ratios = np.array([chi2_ratio(N) for N in Ns])
    N = int(Ns[np.argmin(np.abs(ratios - S / M))])
    u0 = 0.5 * N * (M / stats.chi2.ppf(0.5, N) + S / (stats.chi2.ppf(0.75, N) - stats.chi2.ppf(0.25, N)))
    return N, float(u0)


def robust_params(u):
    """np.percentile (linear) in the dtype of u, as the device's radix select
    does for a float32 Q; the rest in fp64."""
    q1, M, q3 = (float(np.percentile(np.asarray(u), pct)) for pct in (25, 50, 75))
    return robust_dof(M, q3 - q1)


def chi2rob_limit(u, cl):
    """(limit, N, u0) of the "chi2rob" limit of the fit-set distances u."""
    N, u0 = robust_params(u)
    return float(u0 * stats.chi2.ppf(cl, N) / N), N, u0


def outlier_screen(X, k, alpha=0.05, gamma=0.01, n_candidates=None, model=None, round_u=None):
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    if model is None:
        model = spherical_pca(X, k, n_candidates, round_u=round_u)
    h, q = pca_distances(X, model)
    Nh, h0 = robust_params(h)
    Nq, q0 = robust_params(q)
    f = Nh * h / h0 + Nq * q / q0
    cut_e = float(stats.chi2.ppf(1.0 - alpha, Nh + Nq))
    cut_o = float(stats.chi2.ppf((1.0 - gamma) ** (1.0 / n), Nh + Nq))
    cat = np.where(f > cut_o, 2, (f > cut_e).astype(np.int64)).astype(np.uint8)
    return {"keep": cat < 2, "category": cat, "f": f, "h": h, "q": q, "cut_extreme": cut_e, "cut_outlier": cut_o,
            "Nh": Nh, "Nq": Nq, "h0": h0, "q0": q0, "model": model}


# ------------------------------------------------------------------ fixtures

N_ROWS, N_COLS, RANK, N_BAD = 600, 40, 3, 120
KINDS = ("scatter", "cluster")
SEEDS = (0, 1, 2, 3, 4)


def make_fixture(kind, seed):
    """(X float32 (600, 40), clean mask (600,), B (3, 40) the true orthonormal
    signal basis).  A rank-3 signal with score scales (5, 3, 2), noise 0.05,
    offset 1.0; the first 120 rows are replaced by outliers: "scatter"
    1 + N(0, 1)·U(5, 15) per row, "cluster" 1 + 40·v + 0.5·N(0, 1) with v a unit
    vector orthogonal to the signal."""
    rng = np.random.default_rng(seed)
    Qm, _ = np.linalg.qr(rng.standard_normal((N_COLS, RANK + 1)))
    B, v = Qm[:, :RANK].T, Qm[:, RANK]
    scores = rng.standard_normal((N_ROWS, RANK)) * np.array([5.0, 3.0, 2.0])
    X = 1.0 + scores @ B + 0.05 * rng.standard_normal((N_ROWS, N_COLS))
    if kind == "scatter":
        X[:N_BAD] = 1.0 + rng.standard_normal((N_BAD, N_COLS)) * rng.uniform(5.0, 15.0, size=(N_BAD, 1))
    elif kind == "cluster":
        X[:N_BAD] = 1.0 + 40.0 * v + 0.5 * rng.standard_normal((N_BAD, N_COLS))
    else:
        raise ValueError(kind)
    clean = np.ones(N_ROWS, dtype=bool)
    clean[:N_BAD] = False
    return X.astype(np.float32), clean, B


def subspace_angle_deg(P, B):
    """The largest principal angle between the row spaces of P and B, in degrees."""
    Qp, _ = np.linalg.qr(np.asarray(P, dtype=np.float64).T)
    Qb, _ = np.linalg.qr(np.asarray(B, dtype=np.float64).T)
    s = np.linalg.svd(Qp.T @ Qb, compute_uv=False)
    return float(np.degrees(np.arccos(np.clip(s.min(), -1.0, 1.0))))


def classical_pca(X, k):
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    return Vt[:k]
