"""Cross-validation of the PCA itself: PRESS of every number of components.

Choosing LV by specificity, efficiency or AUC needs rows of other classes
(``cross_validate_simca_grid``, ``cross_validate_objects_grid``,
``roc.cross_validate_auc_grid``).  With the target class alone the tool is the
predicted residual sum of squares of held-out target rows as a function of the
number of components, in its element-wise form (ekf: Bro, Kjeldahl, Smilde,
Kiers 2008; the row-wise form sums the Q of left-out rows, falls monotonically
and always ends at LV_max):

* fit the PCA without a fold's rows: the fold engine's pass 1 and eigen-models
  (``cv.fold_models``: one Gram pass for all folds, one eigensolve per fold at
  ``max_components``);
* for every held-out row predict each variable j from the other p − 1 through
  the loadings; with y = x − μ, t = P·y, r⁽ᵏ⁾ = y − Σ_{a≤k} t_a·P_a and
  h_j⁽ᵏ⁾ = Σ_{a≤k} P_aj² the error is exactly r_j⁽ᵏ⁾/(1 − h_j⁽ᵏ⁾);
* PRESS_k = Σ_folds Σ_rows Σ_j (r_j⁽ᵏ⁾/(1 − h_j⁽ᵏ⁾))², k = 0..K, from one read of
  each fold's rows (``ocm_press_f32`` / ``_f64``); the row-wise curve
  naive_k = Σ (r_j⁽ᵏ⁾)² comes from the same pass.

A variable with 1 − h_j⁽ᵏ⁾ ≤ 1e-8 is reproduced by the model alone: it is left
out of PRESS_k and counted in ``ndegen[k]``.  Single process only.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

__all__ = ["pca_press", "press_variables", "PcaCvResult", "make_folds", "select_components", "DEGENERATE"]

DEGENERATE = 1e-8  # include/ocm.h: 1 − h at or below this leaves the variable out
RULES = ("min", "first_min", "wold")


def select_components(press, rule: str = "min", r_threshold: float = 0.95) -> int:
    """The number of components a PRESS curve (k = 0..K) selects.

    ``"min"``: the global argmin over 0..K; ``"first_min"``: the first k with
    press[k + 1] ≥ press[k]; ``"wold"``: the first k with
    press[k + 1]/press[k] > r_threshold (Wold's R).  Where nothing qualifies (no
    rise, no ratio above the threshold, or a minimum only at K itself) the
    answer is K with a warning: the curve was still falling at max_components."""
    press = np.asarray(press, dtype=np.float64)
    if press.ndim != 1 or press.size < 2:
        raise ValueError("select: press must hold at least press[0] and press[1]")
    if rule not in RULES:
        raise ValueError(f"select: rule={rule!r} (one of {RULES})")
    K = press.size - 1
    if rule == "min":
        k = int(np.argmin(press))
        found = k < K
    else:
        if rule == "first_min":
            hit = press[1:] >= press[:-1]
        else:
            if not r_threshold > 0:
                raise ValueError("select: r_threshold must be positive")
            hit = press[1:] > r_threshold * press[:-1]
        idx = np.flatnonzero(hit)
        found = idx.size > 0
        k = int(idx[0]) if found else K
    if not found:
        warnings.warn(f"select({rule!r}): PRESS has no qualifying point below max_components={K}; returning {K} "
                      "(raise max_components to see where the curve turns)", RuntimeWarning, stacklevel=2)
    return k


@dataclass
class PcaCvResult:
    """``pca_press``'s curves (NumPy float64, index k = 0..K components)."""
    press: np.ndarray         # (K + 1,) Σ over the folds
    naive: np.ndarray         # (K + 1,) the row-wise curve Σ (r_j)²
    ndegen: np.ndarray        # (K + 1,) variables left out (Σ over the folds)
    press_folds: np.ndarray   # (folds, K + 1)
    rmsecv: np.ndarray        # sqrt(press / (n·p))
    q2: np.ndarray            # 1 − press/press[0]
    n: int                    # held-out rows in all (every target row once)
    p: int
    models: list = field(default_factory=list)  # per fold: {"mean", "loadings", "evals"} device tensors
    folds: list = field(default_factory=list)   # per fold: the held-out row indices (NumPy int64)

    def select(self, rule: str = "min", r_threshold: float = 0.95) -> int:
        return select_components(self.press, rule, r_threshold)


def make_folds(X, cv=5, rows=None, folds=None, shuffle=False, random_state=None, y=None):
    """The held-out target rows of every fold (NumPy int64 arrays of row indices
    of X).  ``folds``: an explicit list of index arrays (disjoint, at least
    two).  ``cv`` an int: KFold over ``rows`` (default: every row), dealt as
    ``ClasswiseKFoldWithExternalVal`` deals the target rows; a
    ``ClasswiseKFoldWithExternalVal`` or ``ObjectKFoldWithExternalVal``: its
    target folds only (an object splitter holds out whole objects).  Host only."""
    from utils.CVSIMCA import ClasswiseKFoldWithExternalVal

    from .objectcv import ObjectKFoldWithExternalVal

    n = int(X.shape[0])
    if folds is not None:
        if rows is not None:
            raise ValueError("pca_press: give rows= or folds=, not both")
        out = [np.asarray(f, dtype=np.int64).reshape(-1) for f in folds]
        if len(out) < 2:
            raise ValueError("pca_press: folds= needs at least two folds")
        if any(f.size == 0 for f in out):
            raise ValueError("pca_press: a fold is empty")
        allr = np.concatenate(out)
        if allr.min() < 0 or allr.max() >= n:
            raise ValueError(f"pca_press: folds= holds a row index outside [0, {n})")
        if np.unique(allr).size != allr.size:
            raise ValueError("pca_press: folds= must be disjoint")
        return out
    if isinstance(cv, ObjectKFoldWithExternalVal):
        if rows is not None:
            raise ValueError("pca_press: a splitter names its own target rows (rows= must be None)")
        return [np.asarray(f, dtype=np.int64) for f in cv.target_folds(X, y)]
    if isinstance(cv, ClasswiseKFoldWithExternalVal):
        if rows is not None:
            raise ValueError("pca_press: a splitter names its own target rows (rows= must be None)")
        target = np.asarray(cv.target_indices(X, y), dtype=np.int64)
        return [target[held] for _, held in cv.kf.split(target)]
    if isinstance(cv, (bool, np.bool_)) or not isinstance(cv, (int, np.integer)):
        raise ValueError("pca_press: cv must be an int, a ClasswiseKFoldWithExternalVal or an "
                         "ObjectKFoldWithExternalVal")
    if cv < 2:
        raise ValueError(f"pca_press: cv={cv} (at least 2 folds)")
    if rows is None:
        target = np.arange(n, dtype=np.int64)
    else:
        target = np.asarray(rows.detach().cpu().numpy() if hasattr(rows, "detach") else rows)
        if target.dtype == bool:
            if target.shape != (n,):
                raise ValueError(f"pca_press: a boolean rows= has shape {target.shape}, X has {n} rows")
            target = np.flatnonzero(target)
        target = target.astype(np.int64).reshape(-1)
        if target.size and (target.min() < 0 or target.max() >= n):
            raise ValueError(f"pca_press: rows= holds an index outside [0, {n})")
        if np.unique(target).size != target.size:
            raise ValueError("pca_press: rows= holds a row twice")
    split = ClasswiseKFoldWithExternalVal(n_splits=int(cv), cls_idx=target, shuffle=shuffle,
                                          random_state=random_state)
    target = np.asarray(split.target_indices(X, y), dtype=np.int64)
    return [target[held] for _, held in split.kf.split(target)]


def _check_k(max_components, p):
    if isinstance(max_components, (bool, np.bool_)) or not isinstance(max_components, (int, np.integer)):
        raise ValueError(f"pca_press: max_components={max_components!r} must be an int")
    K = int(max_components)
    if K < 1 or K > 64:
        raise ValueError(f"pca_press: max_components={K} must lie in 1..64")
    if p < 2:
        raise ValueError("pca_press: X needs at least 2 columns (a variable is predicted from the others)")
    return K


def pca_press(X, max_components, cv=5, rows=None, folds=None, shuffle=False, random_state=None, y=None,
              group=None) -> PcaCvResult:
    """Element-wise k-fold cross-validation of the PCA of the target rows of X
    for 0..max_components components (module docstring).  X: NumPy, a device
    tensor or a lazy ``PrepView``; float64 X takes the fp64 Gram and
    ``ocm_press_f64``, anything else float32.  ``cv`` / ``rows`` / ``folds`` /
    ``shuffle`` / ``random_state`` / ``y``: ``make_folds``.  ``check_components``
    applies per fold, as in the fold engine.  Returns a ``PcaCvResult``."""
    import torch

    from utils.SIMCA import check_components

    from . import cv as cvmod
    from . import engine

    if group is not None:
        raise ValueError("pca_press is single-process: call it without a process group (every rank may run it on "
                         "its own rows)")
    if len(X.shape) != 2:
        raise ValueError(f"pca_press: X has shape {tuple(X.shape)}")
    p = int(X.shape[1])
    K = _check_k(max_components, p)
    fl = make_folds(X, cv, rows, folds, shuffle, random_state, y)
    n_target = int(sum(f.size for f in fl))
    for f_ in fl:
        check_components(K, n_target - int(f_.size), p)
    Xd = engine.as_device_x(X)
    dev = Xd.device
    fm = cvmod.fold_models(Xd, fl, fl, n_target, K, 0)
    outs = []
    for f, rows_f in enumerate(fl):
        rt = torch.from_numpy(np.ascontiguousarray(rows_f)).to(dev)
        outs.append(engine.press(Xd, rt, int(rows_f.size), fm.evecs[f], fm.mean[f]))
    press_folds = torch.stack([o[0] for o in outs]).cpu().numpy()
    naive = torch.stack([o[1] for o in outs]).sum(dim=0).cpu().numpy()
    ndegen = torch.stack([o[2] for o in outs]).to(torch.int64).sum(dim=0).cpu().numpy()
    press = press_folds.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q2 = 1.0 - press / press[0]
    models = [{"mean": fm.mean[f], "loadings": fm.evecs[f], "evals": fm.evals[f]} for f in range(len(fl))]
    return PcaCvResult(press=press, naive=naive, ndegen=ndegen, press_folds=press_folds,
                       rmsecv=np.sqrt(press / (float(n_target) * p)), q2=q2, n=n_target, p=p, models=models,
                       folds=fl)


def press_variables(X, result: PcaCvResult, k: int):
    """The per-variable PRESS at ``k`` components, (p,) float64 on the device:
    Σ_folds w_k[j] · Σ_rows (r_j⁽ᵏ⁾)², the column profile of the residual
    (``ocm_contrib_*``) of every fold's held-out rows against its model times
    the weights 1/(1 − h_j⁽ᵏ⁾)² (0 for a degenerate variable).  Its sum is
    ``result.press[k]``.  X: the matrix ``pca_press`` was given."""
    import torch

    from . import engine

    K = result.press.size - 1
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 0 or k > K:
        raise ValueError(f"press_variables: k={k!r} must lie in 0..{K}")
    k = int(k)
    if int(X.shape[1]) != result.p:
        raise ValueError(f"press_variables: X has {int(X.shape[1])} columns, the result {result.p}")
    Xd = engine.as_device_x(X)
    dev = Xd.device
    total = torch.zeros(result.p, dtype=torch.float64, device=dev)
    for model, rows_f in zip(result.models, result.folds):
        P = model["loadings"]
        if k:
            Pk = P[:k].contiguous()
            h = (Pk * Pk).sum(dim=0)
        else:  # no component: the residual is the centred row itself
            Pk = torch.zeros((1, result.p), dtype=torch.float64, device=dev)
            h = torch.zeros(result.p, dtype=torch.float64, device=dev)
        d = 1.0 - h
        w = torch.where(d > DEGENERATE, 1.0 / (d * d), torch.zeros_like(d))
        rt = torch.from_numpy(np.ascontiguousarray(rows_f)).to(dev)
        ones = torch.ones(Pk.shape[0], dtype=torch.float64, device=dev)
        res = engine.contributions(Xd, rt, int(rows_f.size), Pk, model["mean"], ones, want_rows=False)
        total += w * res["profiles"][0, 0, :]
    return total
