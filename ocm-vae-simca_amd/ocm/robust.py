"""Robust calibration on the device: the L1 median, spherical PCA and an
outlier screen built on them (csrc/ocm_robust.hip).

Every estimate a SIMCA model rests on is a classical one (the column mean, the
covariance behind the loadings, the moment estimators of ``chi2pom``), and a few
percent of bad calibration rows move all of them: edge pixels, specular spots,
a foreign particle.  ``preprocess.mahalanobis_outlier_mask`` reproduces the
drivers' screen, a classical PCA plus a fixed 95th-percentile cut: it always
discards 5 % of the rows, and the outliers shape the model that is to find
them.  This module is the robust counterpart.

Definitions (``tests/robust_oracle.py`` is their NumPy transcription):

    L1 median   m = argmin Σ_i ‖x_i − m‖, by Weiszfeld's iteration with the
                Vardi–Zhang correction for rows that coincide with the centre
                (include/ocm.h; fp64 throughout, a fixed summation order)
    sphering    u_i = (x_i − m)/‖x_i − m‖: every row pulls with unit weight, so
                an outlier can turn the second-moment matrix only as far as one
                row can.  At the L1 median Σ u_i = 0, so G = UᵀU/n is the
                covariance of the sphered rows
    candidates  the first n_candidates eigenvectors of G (``engine.eig_topk``)
    variances   λ_j = (1.4826·MAD_j)² of the scores t_ij = (x_i − m)·v_j about
                their median; the candidates are ordered by λ, descending (ties
                to the lower index), and the first k are kept.  A tight cluster
                of outliers does become a sphered eigenvector, but more than
                half of the rows have a near-zero score on it, so its MAD is tiny
                and it sorts last: the spare candidates are what drops it
    distances   h_i = Σ_j t_ij²/λ_j,  q_i = ‖x_i − m − Σ_j t_ij v_j‖²
    screen      (N_h, h0), (N_q, q0) = ``limits.robust_dof`` of the median and IQR
                of h and q;  f_i = N_h·h_i/h0 + N_q·q_i/q0;  extreme above
                χ²⁻¹(1 − α, N_h + N_q), outlier above χ²⁻¹((1 − γ)^(1/n), N_h + N_q)

The row passes are HIP kernels (the Weiszfeld steps, the sphering, the Gram,
the scoring, the sorts and the radix select); torch carries the results and
does the O(n·k) arithmetic on the scores.  Each process works on the rows it was
given.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

__all__ = ["L1Median", "RobustPCA", "Screen", "l1_median", "spherical_pca", "outlier_screen"]

MAD_SCALE = 1.4826  # 1/Φ⁻¹(3/4): the MAD of a normal sample estimates σ/1.4826


@dataclass
class L1Median:
    """``center`` (p,) float64 device tensor; ``n_iter`` steps done, ``converged``
    (the last step met ``tol``), ``step`` its length; ``objective`` Σ‖x_i − m‖ and
    ``n_coincident`` (rows that lie exactly on m) at the returned centre;
    ``distances`` (n,) float64 device tensor of ‖x_i − m‖."""
    center: object
    n_iter: int
    converged: bool
    step: float
    objective: float
    n_coincident: int
    distances: object


@dataclass
class Screen:
    """``keep`` (n,) bool and ``category`` (n,) uint8 device tensors (0 regular,
    1 extreme, 2 outlier; keep = category < 2); ``f`` (n,) float64 the full
    distances; the two cuts; the robust degrees of freedom and scale factors of
    h and q; ``pca`` the ``RobustPCA`` they were measured in."""
    keep: object
    category: object
    f: object
    cut_extreme: float
    cut_outlier: float
    Nh: int
    Nq: int
    h0: float
    q0: float
    pca: object


# ------------------------------------------------------------------ argument checks (no device)

def _shape(X):
    sh = tuple(X.shape)
    if len(sh) != 2 or sh[0] < 1 or sh[1] < 1:
        raise ValueError(f"X must be a non-empty 2-D matrix, got shape {sh}")
    return sh


def _rows_host(rows, n_x):
    """rows as an int64 host index array (None: all rows), checked against X."""
    if rows is None:
        return None
    r = rows.detach().cpu().numpy() if hasattr(rows, "detach") else np.asarray(rows)
    if r.dtype == np.bool_:
        if r.shape != (n_x,):
            raise ValueError(f"rows: a mask must have shape ({n_x},), got {r.shape}")
        r = np.flatnonzero(r)
    if r.ndim != 1 or r.size < 1 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("rows: expected a non-empty 1-D integer index array or a boolean mask")
    r = r.astype(np.int64)
    if r.min() < 0 or r.max() >= n_x:
        raise ValueError(f"rows: indices must lie in [0, {n_x})")
    return r


def _check_l1(X, rows, start, tol, max_iter):
    n_x, p = _shape(X)
    rh = _rows_host(rows, n_x)
    if start is not None and tuple(np.shape(start)) != (p,):
        raise ValueError(f"start has shape {tuple(np.shape(start))}, X has {p} columns")
    if not (isinstance(tol, (int, float, np.floating)) and tol >= 0):
        raise ValueError(f"tol={tol!r} must be a number >= 0")
    if int(max_iter) != max_iter or not (0 <= max_iter <= 100000):
        raise ValueError(f"max_iter={max_iter!r} must be an integer in [0, 100000]")
    return n_x, p, rh


def _check_pca(X, n_components, n_candidates, rows):
    n_x, p = _shape(X)
    rh = _rows_host(rows, n_x)
    n = n_x if rh is None else int(rh.size)
    if int(n_components) != n_components or not (1 <= n_components <= p):
        raise ValueError(f"n_components={n_components!r} must be an integer in [1, {p}]")
    k = int(n_components)
    if n < 2 or k > n - 1:
        raise ValueError(f"n_components={k} needs at least {k + 1} rows, got {n}")
    if n_candidates is None:
        kc = min(2 * k, n - 1, p)
    else:
        if int(n_candidates) != n_candidates or not (k <= n_candidates <= min(n - 1, p)):
            raise ValueError(f"n_candidates={n_candidates!r} must be an integer in [{k}, {min(n - 1, p)}]")
        kc = int(n_candidates)
    return n, p, rh, k, kc


def _check_screen(alpha, gamma):
    for name, v in (("alpha", alpha), ("gamma", gamma)):
        if not (isinstance(v, (int, float, np.floating)) and 0.0 < v < 1.0):
            raise ValueError(f"{name}={v!r} must lie in (0, 1)")


# ------------------------------------------------------------------ device side

def _device_x(X):
    from . import engine
    from .prepview import PrepView

    Xd = engine.as_device_x(X)
    if isinstance(Xd, PrepView):  # no lazy form: the median of preprocessed rows needs the rows
        Xd = Xd.materialize()
    return Xd


def _rows_dev(rh, dev):
    import torch

    return None if rh is None else torch.from_numpy(rh).to(dev)


def l1_median(X, rows=None, start=None, tol=1e-9, max_iter=200) -> L1Median:
    """The spatial (L1) median of the rows of X (``rows``: an index array or a
    mask, None for all).  ``start``: (p,) the first centre, by default the column
    mean.  The iteration stops when a step is no longer than ``tol``·‖m‖ or after
    ``max_iter`` steps; all of them are queued at once, a step that finds the work
    done returns at once, and the five scalars are read back once at the end."""
    import torch

    from . import engine

    _, p, rh = _check_l1(X, rows, start, tol, max_iter)
    Xd = _device_x(X)
    rd = _rows_dev(rh, Xd.device)
    n = Xd.shape[0] if rd is None else int(rd.numel())
    if start is None:
        s64 = engine.colmean(Xd, rd, n)
    else:
        s64 = torch.as_tensor(np.asarray(start.detach().cpu() if hasattr(start, "detach") else start,
                                         dtype=np.float64)).to(Xd.device)
    center, info, dist = engine.l1_median(Xd, rd, s64, float(tol), int(max_iter))
    h = info.cpu().numpy()
    return L1Median(center, int(h[0]), bool(h[1] != 0.0), float(h[2]), float(h[3]), int(h[4]), dist)


def _column_medians(S):
    """Medians of the columns of the column-sorted (n, c) float64 matrix S."""
    n = S.shape[0]
    return 0.5 * (S[(n - 1) // 2] + S[n // 2])


class RobustPCA:
    """A spherical PCA: ``center`` (p,) float64 the L1 median, ``components``
    (k, p) float64 orthonormal rows, ``explained_variance`` (k,) float64 their
    robust variances (1.4826·MAD)², descending, ``candidate_variance``
    (n_candidates,) the same of every candidate in eigenvector order and
    ``candidate_order`` the indices kept.  Device tensors; ``median`` is the
    ``L1Median`` behind the centre."""

    def __init__(self, center, components, explained_variance, candidate_variance, candidate_order, median):
        self.center = center
        self.components = components
        self.explained_variance = explained_variance
        self.candidate_variance = candidate_variance
        self.candidate_order = candidate_order
        self.median = median
        self.n_components = int(components.shape[0])

    def distances(self, X, rows=None):
        """(h, q) of rows of X: h_i = Σ_j t_ij²/λ_j (float64), q_i = the squared
        residual (X's dtype), device tensors (``engine.score``)."""
        from . import engine

        n_x, p = _shape(X)
        if p != self.components.shape[1]:
            raise ValueError(f"X has {p} columns, the model has {self.components.shape[1]}")
        rh = _rows_host(rows, n_x)
        Xd = _device_x(X)
        rd = _rows_dev(rh, Xd.device)
        n = Xd.shape[0] if rd is None else int(rd.numel())
        out = engine.score(Xd, rd, n, self.components, self.center, 1.0 / self.explained_variance)
        return out["T2"], out["Q"]


def _spherical_pca(Xd, rd, n, k, kc, tol=1e-9, max_iter=200) -> RobustPCA:
    import torch

    from . import engine

    p = Xd.shape[1]
    dev = Xd.device
    center, info, _ = engine.l1_median(Xd, rd, engine.colmean(Xd, rd, n), tol, max_iter, want_dist=False)
    U, _ = engine.sphere_rows(Xd, rd, center)
    G, _ = engine.gram(U, None, [0, n], torch.zeros(p, dtype=torch.float32, device=dev))
    del U
    C = G[0] / float(n)
    _, V, _, _ = engine.eig_topk(C, kc, 0)
    one = torch.ones(kc, dtype=torch.float64, device=dev)
    T = engine.score(Xd, rd, n, V, center, one, want_T=True, want_T2=False, want_Q=True)["T"].to(torch.float64)
    from . import roc

    med = _column_medians(roc.sort_values(T, axis=0))
    mad = _column_medians(roc.sort_values((T - med).abs(), axis=0))
    lam = (MAD_SCALE * mad) ** 2
    order = torch.sort(lam, descending=True, stable=True).indices
    h = torch.cat([info, lam, order.to(torch.float64)]).cpu().numpy()
    lam_h = h[engine.L1_INFO:engine.L1_INFO + kc]
    if int((lam_h > 0).sum()) < k:
        raise ValueError(f"spherical_pca: only {int((lam_h > 0).sum())} of the {kc} candidate directions have a "
                         f"positive robust variance, n_components={k}")
    keep = order[:k]
    median = L1Median(center, int(h[0]), bool(h[1] != 0.0), float(h[2]), float(h[3]), int(h[4]), None)
    return RobustPCA(center, V[keep].contiguous(), lam[keep].contiguous(), lam, keep, median)


def spherical_pca(X, n_components, n_candidates=None, rows=None) -> RobustPCA:
    """Spherical PCA of the rows of X about their L1 median, with the
    components chosen among ``n_candidates`` (default min(2k, n − 1, p)) sphered
    eigenvectors by their robust variance.  ValueError when fewer than
    ``n_components`` candidates have a positive one."""
    n, _, rh, k, kc = _check_pca(X, n_components, n_candidates, rows)
    Xd = _device_x(X)
    return _spherical_pca(Xd, _rows_dev(rh, Xd.device), n, k, kc)


def outlier_screen(X, n_components, alpha=0.05, gamma=0.01, n_candidates=None, rows=None) -> Screen:
    """The robust counterpart of ``preprocess.mahalanobis_outlier_mask``: a
    spherical PCA of the rows, their full distances f under the robust
    data-driven parameters (``limits.robust_dof``) and the DD-SIMCA categories.
    Fit the class model on ``keep``.  Nothing is discarded from clean data
    beyond the γ tail."""
    import torch

    from . import engine, limits

    n, _, rh, k, kc = _check_pca(X, n_components, n_candidates, rows)
    _check_screen(alpha, gamma)
    Xd = _device_x(X)
    rd = _rows_dev(rh, Xd.device)
    pca = _spherical_pca(Xd, rd, n, k, kc)
    out = engine.score(Xd, rd, n, pca.components, pca.center, 1.0 / pca.explained_variance)
    h, q = out["T2"], out["Q"]

    def params(v):
        q1, med, q3 = (engine.percentile(v, pct) for pct in (25.0, 50.0, 75.0))
        return limits.robust_dof(med, q3 - q1)

    Nh, h0 = params(h)
    Nq, q0 = params(q)
    f = (Nh / h0) * h + (Nq / q0) * q.to(torch.float64)
    cut_e = float(limits._chi2_ppf(1.0 - float(alpha), float(Nh + Nq)))
    cut_o = float(limits._chi2_ppf((1.0 - float(gamma)) ** (1.0 / n), float(Nh + Nq)))
    category = torch.where(f > cut_o, 2, (f > cut_e).to(torch.int64)).to(torch.uint8)
    return Screen(category < 2, category, f, cut_e, cut_o, Nh, Nq, h0, q0, pca)
