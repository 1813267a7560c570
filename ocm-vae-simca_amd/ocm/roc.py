"""Threshold-free evaluation on the device: exact ROC AUC, ROC points, a
keys-only sort (csrc/ocm_roc.hip).

The reference scores a trial of its hyper-parameter search with
``roc_auc_score(labels_true, f_all)`` (optim_bce_nuts.py:241,279).  ``auc`` is
that call for scores that are already in HBM — ``SIMCA.decision_function``,
``ClassifyResult.ratio``, the fold engine's per-configuration decision values,
the VAE's ``f`` — without a copy to the host:

    u2  = Σ over (positive i, negative j) of 2·[s_i > s_j] + [s_i == s_j]
    AUC = u2 / (2·P·N)

``u2`` is an exact integer (``ocm_auc``), so the AUC is the correctly rounded
quotient of two integers; scikit-learn's trapezoid sum agrees with it to its own
rounding (m·2⁻⁵²).  Scores compare by value: −0.0 == +0.0, ±inf in order, a
float32 score as its exact double.

``u2_host`` and ``roc_counts_host`` are the NumPy statements of what the kernels
compute; the tests compare the kernels with them bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

__all__ = ["auc", "roc_points", "sort_values", "u2_host", "roc_counts_host", "roc_points_host",
           "cross_validate_auc_grid", "AucResult", "RocPoints", "tile_keys", "last_passes", "MAX_THRESHOLDS"]

MAX_THRESHOLDS = 4096  # ocm_roc_counts: 1 ≤ K ≤ 4096


@dataclass
class AucResult:
    """``auc`` (C,) float64; ``u2`` (C,) int64, exact; ``n_pos``, ``n_neg`` ints."""
    auc: np.ndarray
    u2: np.ndarray
    n_pos: int
    n_neg: int


@dataclass
class RocPoints:
    """Points of the ROC curve at ``thresholds`` (ascending, the last one +inf):
    ``tp`` / ``fp`` = positives / negatives with score ≥ threshold (int64),
    ``tpr`` = tp / P, ``fpr`` = fp / N.  One column: (K,) arrays; C columns:
    (C, K), a column with fewer distinct thresholds padded with +inf."""
    thresholds: np.ndarray
    tp: np.ndarray
    fp: np.ndarray
    tpr: np.ndarray
    fpr: np.ndarray


# ------------------------------------------------------------------ host mirrors

def _host_1d(scores, positive):
    s = np.asarray(scores).astype(np.float64)  # a float32 score is taken as its exact double
    pos = np.asarray(positive).astype(bool)
    if s.ndim != 1 or pos.shape != s.shape:
        raise ValueError(f"scores {s.shape} and positive {pos.shape} must be 1-D and of one length")
    return s, pos


def u2_host(scores, positive) -> int:
    """Σ over (positive i, negative j) of 2·[s_i > s_j] + [s_i == s_j] as a Python
    integer, NaN rows left out: ``np.sort`` of the negatives and two
    ``np.searchsorted`` per positive (lt = negatives below, le = not above)."""
    s, pos = _host_1d(scores, positive)
    keep = ~np.isnan(s)
    neg = np.sort(s[~pos & keep])
    sp = s[pos & keep]
    lt = np.searchsorted(neg, sp, side="left").astype(np.int64)
    le = np.searchsorted(neg, sp, side="right").astype(np.int64)
    # each partial sum is below m² < 2^62, the doubling is done on Python integers
    return 2 * int(lt.sum(dtype=np.int64)) + int((le - lt).sum(dtype=np.int64))


def roc_counts_host(scores, positive, thresholds) -> np.ndarray:
    """(K, 2) int64 {positives with s ≥ thr, negatives with s ≥ thr}; a NaN score
    counts nowhere."""
    s, pos = _host_1d(scores, positive)
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    keep = ~np.isnan(s)
    out = np.empty((thr.size, 2), dtype=np.int64)
    for j, sel in enumerate((pos & keep, ~pos & keep)):
        v = np.sort(s[sel])
        out[:, j] = v.size - np.searchsorted(v, thr, side="left")
    return out


def _rank_grid(n_neg: int, n_points: int) -> np.ndarray:
    """Evenly spaced ranks into the sorted negatives: n_points − 1 of them (the
    +inf threshold is the last point), duplicates dropped."""
    if n_points < 2:
        raise ValueError(f"roc_points: n_points={n_points} must be at least 2")
    if n_points > MAX_THRESHOLDS:
        raise ValueError(f"roc_points: n_points={n_points} exceeds {MAX_THRESHOLDS}")
    return np.unique(np.round(np.linspace(0, n_neg - 1, n_points - 1)).astype(np.int64))


def _thresholds_from(order_stats: np.ndarray) -> np.ndarray:
    """Ascending order statistics of the negatives → distinct thresholds + inf."""
    return np.concatenate([np.unique(np.asarray(order_stats, dtype=np.float64)), [np.inf]])


def _check_thresholds(thresholds) -> np.ndarray:
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if thr.size < 1 or thr.size > MAX_THRESHOLDS:
        raise ValueError(f"roc_points: K={thr.size} thresholds; 1 <= K <= {MAX_THRESHOLDS}")
    if np.isnan(thr).any() or (np.diff(thr) < 0).any():
        raise ValueError("roc_points: thresholds must be ascending and free of NaN")
    return thr


def _points(thr, cnt, n_pos, n_neg) -> RocPoints:
    tp, fp = cnt[..., 0], cnt[..., 1]
    return RocPoints(thr, tp, fp, tp / np.float64(n_pos), fp / np.float64(n_neg))


def roc_points_host(scores, positive, n_points=257, thresholds=None) -> RocPoints:
    """``roc_points`` for one column of scores, in NumPy."""
    s, pos = _host_1d(scores, positive)
    _check_classes(int(pos.sum()), int((~pos).sum()))
    if np.isnan(s).any():
        raise ValueError("roc_points: a score is NaN")
    if thresholds is None:
        neg = np.sort(s[~pos])
        thr = _thresholds_from(neg[_rank_grid(neg.size, n_points)])
    else:
        thr = _check_thresholds(thresholds)
    return _points(thr, roc_counts_host(s, pos, thr), int(pos.sum()), int((~pos).sum()))


# ------------------------------------------------------------------ device side

def _check_classes(n_pos: int, n_neg: int):
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in `positive`: the ROC AUC is not defined in that case "
                         f"(P = {n_pos}, N = {n_neg})")


def _torch():
    import torch

    return torch


def _device_scores(scores):
    """(tensor on the device in float32 / float64, came-from-NumPy)."""
    torch = _torch()
    from .engine import require_device

    if isinstance(scores, torch.Tensor):
        t = scores
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        if not t.is_cuda:
            require_device()
            t = t.to(torch.device("cuda", torch.cuda.current_device()))
        return t, False
    a = np.asarray(scores)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    require_device()
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", torch.cuda.current_device())), True


def _layout(shape, strides, axis):
    """(m, ncol, col_stride, row_stride) of a 1-D or 2-D array whose rows run along ``axis``."""
    if len(shape) == 1:
        return int(shape[0]), 1, 0, int(strides[0])
    if len(shape) != 2:
        raise ValueError(f"scores must be 1-D or 2-D, got shape {tuple(shape)}")
    if axis not in (0, 1, -1, -2):
        raise ValueError(f"axis={axis} for 2-D scores")
    ax = axis % 2
    return int(shape[ax]), int(shape[1 - ax]), int(strides[1 - ax]), int(strides[ax])


def _positive_host_or_dev(positive, m):
    """positive as given → (device uint8 tensor maker, host bool array or None)."""
    torch = _torch()
    if isinstance(positive, torch.Tensor):
        if tuple(positive.shape) != (m,):
            raise ValueError(f"positive has shape {tuple(positive.shape)}, the scores have {m} rows")
        return positive, None
    ph = np.asarray(positive)
    if ph.shape != (m,):
        raise ValueError(f"positive has shape {ph.shape}, the scores have {m} rows")
    return None, ph.astype(bool)


def _positive_dev(pt, ph, dev):
    torch = _torch()
    if pt is not None:
        return (pt != 0).to(device=dev, dtype=torch.uint8).contiguous()
    return torch.from_numpy(ph.astype(np.uint8)).to(dev)


def tile_keys() -> int:
    """Keys one workgroup ranks per sort tile (``ocm_roc_tile_keys``)."""
    from . import _lib

    return int(_lib.load().ocm_roc_tile_keys())


def last_passes() -> int:
    """Radix passes the last ``ocm_sort_f`` / ``ocm_auc`` of this thread executed."""
    from . import _lib

    return int(_lib.load().ocm_roc_last_passes())


def _call_auc(t, m, ncol, cs, rs, pos):
    """ocm_auc on the tensor ``t`` → (u2 (C,) int64, P, N, nnan (C,) int64), host."""
    torch = _torch()
    from . import _lib

    dev = t.device
    u2 = torch.empty(ncol, dtype=torch.int64, device=dev)  # u2 ≤ 2·P·N < 2^62: the uint64 bits as int64
    pn = torch.empty(2, dtype=torch.int64, device=dev)
    nnan = torch.empty(ncol, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().ocm_auc(_lib.Context.get(dev.index).handle, _lib.ptr(t),
                                   0 if t.dtype == torch.float64 else 1, m, ncol, cs, rs, _lib.ptr(pos), _lib.ptr(u2),
                                   _lib.ptr(pn), _lib.ptr(nnan), _lib.stream_handle(dev)), "ocm_auc")
    host = torch.cat([pn, u2, nnan]).cpu().numpy()
    return host[2:2 + ncol].copy(), int(host[0]), int(host[1]), host[2 + ncol:].copy()


def auc(scores, positive, axis=0, lower_is_positive=False) -> AucResult:
    """Exact ROC AUC of every column of ``scores`` against the mask ``positive``.

    ``scores``: (m,) or 2-D, NumPy or torch, float32 or float64; ``axis`` names
    the row axis of a 2-D input, so an (m, C) matrix (axis=0) and a (ncfg, m)
    table (axis=1) are both read in place, whatever their torch strides.
    ``positive``: m flags shared by the columns.  ``lower_is_positive``: the
    positives are the rows with the lower scores (a distance): u2 becomes
    2·P·N − u2.  Raises ValueError when a class is absent or a score is NaN, as
    scikit-learn does.  The results are small host arrays."""
    torch = _torch()
    is_t = isinstance(scores, torch.Tensor)
    shape = tuple(scores.shape) if is_t else np.shape(scores)
    if len(shape) not in (1, 2):
        raise ValueError(f"scores must be 1-D or 2-D, got shape {shape}")
    m = _layout(shape, (0,) * len(shape), axis)[0]
    pt, ph = _positive_host_or_dev(positive, m)
    if ph is not None:  # host labels: the classes are checked before anything is moved
        _check_classes(int(ph.sum()), int(m - ph.sum()))
    if not is_t and np.isnan(np.asarray(scores, dtype=np.float64)).any():
        raise ValueError("auc: a score is NaN")
    t, _ = _device_scores(scores)
    m, ncol, cs, rs = _layout(t.shape, t.stride(), axis)
    pos = _positive_dev(pt, ph, t.device)
    u2, P, N, nnan = _call_auc(t, m, ncol, cs, rs, pos)
    _check_classes(P, N)
    if nnan.any():
        raise ValueError(f"auc: {int(nnan.sum())} scores are NaN (column {int(np.flatnonzero(nnan)[0])} first)")
    if lower_is_positive:
        u2 = 2 * P * N - u2
    return AucResult(np.array([int(u) / (2 * P * N) for u in u2], dtype=np.float64), u2, P, N)


def sort_values(v, axis=0):
    """Ascending sorted copy along ``axis`` (``ocm_sort_f``: keys only, −0.0
    before +0.0, NaNs last), of the shape of ``v``.  NumPy in, NumPy out."""
    torch = _torch()
    from . import _lib

    t, was_np = _device_scores(v)
    n, ncol, cs, rs = _layout(t.shape, t.stride(), axis)
    out = torch.empty((ncol, n), dtype=t.dtype, device=t.device)
    _lib.check(_lib.load().ocm_sort_f(_lib.Context.get(t.device.index).handle, _lib.ptr(t),
                                      0 if t.dtype == torch.float64 else 1, n, ncol, cs, rs, _lib.ptr(out),
                                      _lib.stream_handle(t.device)), "ocm_sort_f")
    if t.dim() == 1:
        out = out.reshape(n)
    elif axis % 2 == 0:
        out = out.t()
    return out.cpu().numpy() if was_np else out


def roc_counts(t, positive_dev, thr, axis=0):
    """``ocm_roc_counts``: ``thr`` (C, K) float64 device tensor, ascending per
    column → (C, K, 2) int64 device tensor."""
    torch = _torch()
    from . import _lib

    m, ncol, cs, rs = _layout(t.shape, t.stride(), axis)
    K = int(thr.shape[1])
    if not 1 <= K <= MAX_THRESHOLDS:
        raise ValueError(f"roc_counts: K={K} thresholds; 1 <= K <= {MAX_THRESHOLDS}")
    if tuple(thr.shape) != (ncol, K) or thr.dtype != torch.float64:
        raise ValueError(f"roc_counts: thr must be ({ncol}, K) float64")
    thr = thr.contiguous()
    cnt = torch.empty((ncol, K, 2), dtype=torch.int64, device=t.device)
    _lib.check(_lib.load().ocm_roc_counts(_lib.Context.get(t.device.index).handle, _lib.ptr(t),
                                          0 if t.dtype == torch.float64 else 1, m, ncol, cs, rs,
                                          _lib.ptr(positive_dev), _lib.ptr(thr), K, _lib.ptr(cnt),
                                          _lib.stream_handle(t.device)), "ocm_roc_counts")
    return cnt


def roc_points(scores, positive, n_points=257, thresholds=None) -> RocPoints:
    """Exact points of the ROC curve of ``scores`` ((m,) or (m, C)).

    Without ``thresholds`` they are the order statistics of the negatives at
    ``n_points − 1`` evenly spaced ranks (``ocm_sort_f`` on the negatives), with
    duplicates dropped and +inf added: the FPR grid is even and every point is a
    point of the full curve.  ``thresholds``: K ≤ 4096 ascending values used for
    every column."""
    torch = _torch()
    is_t = isinstance(scores, torch.Tensor)
    shape = tuple(scores.shape) if is_t else np.shape(scores)
    if len(shape) not in (1, 2):
        raise ValueError(f"scores must be 1-D or 2-D, got shape {shape}")
    m = int(shape[0])
    pt, ph = _positive_host_or_dev(positive, m)
    if ph is not None:
        _check_classes(int(ph.sum()), int(m - ph.sum()))
    thr_h = None if thresholds is None else _check_thresholds(thresholds)
    if thresholds is None:
        _rank_grid(1, n_points)  # the argument check
    if not is_t and np.isnan(np.asarray(scores, dtype=np.float64)).any():
        raise ValueError("roc_points: a score is NaN")
    t, _ = _device_scores(scores)
    if torch.isnan(t).any():
        raise ValueError("roc_points: a score is NaN")
    pos = _positive_dev(pt, ph, t.device)
    P = int(pos.sum())
    N = m - P
    _check_classes(P, N)
    ncol = 1 if t.dim() == 1 else int(t.shape[1])
    if thr_h is None:
        srt = sort_values(t[pos == 0], axis=0)  # (N,) or (N, C)
        picks = srt[torch.from_numpy(_rank_grid(N, n_points)).to(t.device)].to(torch.float64).cpu().numpy()
        cols = [_thresholds_from(picks.reshape(-1, ncol)[:, c]) for c in range(ncol)]
        K = max(c.size for c in cols)
        thr_h = np.full((ncol, K), np.inf)
        for c, v in enumerate(cols):
            thr_h[c, :v.size] = v
    else:
        thr_h = np.broadcast_to(thr_h, (ncol, thr_h.size)).copy()
    cnt = roc_counts(t, pos, torch.from_numpy(thr_h).to(t.device), axis=0).cpu().numpy()
    if t.dim() == 1:
        thr_h, cnt = thr_h[0], cnt[0]
    return _points(thr_h, cnt, P, N)


# ------------------------------------------------------------------ cross-validation by AUC

class _RowScores:
    """The fold engine's object hook with every test row its own object: it is
    handed ``ocm_cv_objects``' decision sums, which are then the per-row decision
    values ``dlim − dred`` of every configuration, (ncfg, m) on the device, and
    turns them into ncfg AUCs with one ``ocm_auc`` call per fold."""

    want_votes = False
    want_dsum = True

    def __init__(self, positive: np.ndarray, store_scores: bool):
        self.positive = positive
        self.store_scores = store_scores
        self.folds = {}

    def test_runs(self, test_rows: np.ndarray, n_fold_rows: int):
        return np.arange(test_rows.size + 1, dtype=np.int64), np.asarray(test_rows, dtype=np.int64)

    def add_fold(self, f, rows, off, votes, dsum):
        res = auc(dsum, self.positive[rows], axis=1)
        self.folds[f] = {"rows": rows, "auc": res.auc, "u2": res.u2, "n_pos": res.n_pos, "n_neg": res.n_neg,
                         "scores": dsum.cpu().numpy() if self.store_scores else None}


def _positive_of(y, ci):
    """The rows whose label is ``ci``, or one of ``ci`` when it is a list of labels."""
    return np.isin(y, np.ravel(np.asarray(ci))).reshape(y.shape[0])


def _engine_auc(template, X, y, cv, lv_values, param_grid, class_index, store_scores):
    from . import cv as fold_engine
    from .objectcv import ObjectKFoldWithExternalVal

    app = fold_engine._applicable(template, X, y, cv, lv_values, param_grid)
    if app is None:
        return None
    cls_idx, tl, combos, base = app
    if isinstance(cv, ObjectKFoldWithExternalVal):
        folds = cv.target_folds(X, y)
    else:
        folds = [cls_idx[held] for _, held in cv.kf.split(cls_idx)]
    ci = [tl] if class_index is None else class_index
    hook = _RowScores(_positive_of(y, ci), store_scores)
    fold_engine.cv_grid(X, y, folds, cls_idx, lv_values, combos, base, ci, False, objects=hook)
    K = len(folds)
    lvs = sorted(set(int(v) for v in lv_values))
    records, by_combo = [], []
    for ci_, combo in enumerate(combos):
        for lv in lv_values:
            c = ci_ * len(lvs) + lvs.index(int(lv))
            per = [float(hook.folds[f]["auc"][c]) for f in range(K)]
            records.append({"params": combo.copy(), "LV": lv, "auc": float(np.mean(per)), "auc_folds": per})
            if store_scores:
                by_combo.append({"params": combo.copy(), "LV": lv,
                                 "folds": [{"rows": hook.folds[f]["rows"], "scores": hook.folds[f]["scores"][c],
                                            "u2": int(hook.folds[f]["u2"][c]), "n_pos": hook.folds[f]["n_pos"],
                                            "n_neg": hook.folds[f]["n_neg"]} for f in range(K)]})
    return records, by_combo


def _decision_of(model, X):
    """(decision values of the last SIMCA step, that step) of a fitted estimator."""
    from sklearn.pipeline import Pipeline

    from utils.CVSIMCA import _get_simca

    if isinstance(model, Pipeline):
        for _, step in model.steps[:-1]:
            X = step.transform(X)
    simca = _get_simca(model)
    if not hasattr(simca, "decision_function"):
        raise TypeError(f"cross_validate_auc_grid: {type(simca).__name__} has no decision_function")
    return simca.decision_function(X), simca


def _loop_auc(template, X, y, cv, lv_values, param_grid, ncomp_key, class_index, store_scores):
    """Generic path: a refit per (setting, fold), ``decision_function`` on the
    fold's test rows and ``auc`` of its one column."""
    from sklearn.base import clone

    from utils.CVSIMCA import _configured, _settings

    splits = list(cv.split(X, y))
    records, by_combo = [], []
    for combo, lv in _settings(param_grid, lv_values):
        est = _configured(template, combo, ncomp_key, lv)
        per, kept = [], []
        for fit_rows, test_rows in splits:
            model = clone(est)
            model.fit(X[fit_rows, :], y[fit_rows])
            D, simca = _decision_of(model, X[test_rows, :])
            if D.shape[1] != 1:
                raise ValueError("cross_validate_auc_grid: the fold models must have one class "
                                 f"(got {D.shape[1]}); set model_class")
            ci = class_index if class_index is not None else getattr(simca, "model_class", 1)
            res = auc(D[:, 0], _positive_of(y[test_rows], ci))
            per.append(float(res.auc[0]))
            if store_scores:
                s = D[:, 0]
                kept.append({"rows": np.asarray(test_rows), "scores": s.cpu().numpy() if hasattr(s, "cpu") else s,
                             "u2": int(res.u2[0]), "n_pos": res.n_pos, "n_neg": res.n_neg})
        LV = combo.get(ncomp_key) if lv is None else lv
        records.append({"params": combo.copy(), "LV": LV, "auc": float(np.mean(per)), "auc_folds": per})
        if store_scores:
            by_combo.append({"params": combo.copy(), "LV": LV, "folds": kept})
    return records, by_combo


def cross_validate_auc_grid(estimator, X, y, cv, LV_min=2, LV_max=10, param_grid=None, class_index=None,
                            store_scores=False):
    """Grid × LV class-wise CV scored by ROC AUC, with refit on all rows.

    Each fold's AUC ranks its held-out target rows against the other-class
    rows — the rows the fold's specificity is computed on — by the decision
    value ``D_limit − dred``; a record's ``auc`` is the mean over folds,
    ``auc_folds`` the list.  Records come in ``cross_validate_simca_grid``'s
    order and ``best`` is the first maximum of ``auc``.  Parameter combinations
    that differ only in ``dcl`` rank alike, so their AUCs are equal.

    ``cv``: a ``ClasswiseKFoldWithExternalVal`` or ``ObjectKFoldWithExternalVal``.
    This package's SIMCA on float32 rows runs on the fold engine (one scoring
    per fold at LV_max, one batched ``ocm_auc`` per fold for all configurations);
    anything else refits per (setting, fold).  ``store_scores`` adds
    ``by_combo[i]["folds"][f]`` = {rows, scores, u2, n_pos, n_neg}.  Per-process
    under a process group."""
    from sklearn.base import clone

    from utils.CVSIMCA import _find_ncomp_param_name

    from .replica import per_process

    param_grid = {} if param_grid is None else param_grid
    template = clone(estimator)
    ncomp_key = _find_ncomp_param_name(template)
    lv_in_grid = any(name.endswith("n_components") for name in param_grid)
    lv_values = None if lv_in_grid else list(range(LV_min, LV_max + 1))
    y = np.asarray(y.detach().cpu().numpy() if hasattr(y, "detach") else y)
    with per_process():
        got = _engine_auc(template, X, y, cv, lv_values, param_grid, class_index, store_scores)
        if got is None:
            got = _loop_auc(template, X, y, cv, lv_values, param_grid, ncomp_key, class_index, store_scores)
        records, by_combo = got
        best = records[int(np.argmax([r["auc"] for r in records]))]
        refit = clone(estimator)
        refit.set_params(**best["params"])
        if not lv_in_grid:
            refit.set_params(**{_find_ncomp_param_name(refit): best["LV"]})
        refit.fit(X, y)
    result = {"results": records, "best_params": best["params"].copy(), "best_LV": best["LV"],
              "best_score": best["auc"], "best_estimator": refit}
    if store_scores:
        result["by_combo"] = by_combo
    return result
