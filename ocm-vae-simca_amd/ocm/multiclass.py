"""Multi-class reading of a SIMCA model: which class a sample is assigned to,
how many classes accept it, the true-class × assigned-class table and the
distance between two class models.

The reference's SIMCA fits every class (``model_class=None``,
utils/SIMCA.py:27-59) and its ``predict`` returns the (m, C) matrix of 0/1
(utils/SIMCA.py:120-145); data_cheese.py:193-328 reads those one-class results
against PLS-DA on the same rows.  This module holds what ``SIMCA.classify``
returns (``ClassifyResult``), the assignment rule as NumPy (``assign``,
``count_tables``: the twin of ocm_score_multi_f32's epilogue, for tests and
host data), the composition of the per-class kernels that serves the inputs the
fused kernel does not take (``classify_composed``), the rule that picks between
the two (``fused_is_faster``) and Wold's inter-class distance
(``wold_distance``).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import engine

__all__ = ["ClassifyResult", "assign", "count_tables", "classify_composed", "fused_is_faster", "wold_distance"]


@dataclass
class ClassifyResult:
    """What ``SIMCA.classify`` returns (NumPy arrays or device tensors),
    columns in ``model_class`` order as in ``predict``.  ``pred`` (m, C) float64
    0/1, ``predict``'s matrix; ``ratio`` (m, C) float64 ``dred / D_limit`` (< 1:
    accepted); ``index`` (m,) int64, the accepting class at the smallest ratio
    (the lowest on a tie), −1 when no class accepts; ``label`` (m,) int64
    ``model_class[index]`` (``none_label`` where index is −1); ``nearest`` (m,)
    int64, the class at the smallest ratio whether it accepts or not (NaN counts
    as +inf; 0 when every ratio is NaN); ``n_accept`` (m,) int64.  With
    ``distances=True``: ``T2`` (m, C) float64 and ``Q`` (m, C) in the input's
    arithmetic.  With ``y_true``, int64 counts whose row C gathers the rows of no
    modelled class: ``table`` (C + 1, C + 1) [true][index, column C = none],
    ``accept_counts`` (C + 1, C) [true][class] accepted, ``n_accept_hist``
    (C + 1, C + 1) [true][n_accept]; and ``metrics`` {class: TP / TN / FP / FN
    and the rates}, what ``predict(X, y_true)`` stores in ``self.metrics``."""
    pred: object
    ratio: object
    index: object
    label: object
    nearest: object
    n_accept: object
    T2: object = None
    Q: object = None
    table: object = None
    accept_counts: object = None
    n_accept_hist: object = None
    metrics: object = None


def assign(ratio, accept):
    """(index, nearest, n_accept), int64 (m,) each, from the (m, C) ``ratio`` and
    0/1 ``accept`` matrices: the rule of ocm_score_multi_f32.  A NaN ratio counts
    as +inf; ``nearest`` is the lowest class at the smallest ratio (0 when all
    are NaN); ``index`` the lowest accepting class at the smallest ratio among
    the accepting ones, −1 when none accepts."""
    r = np.asarray(ratio, dtype=np.float64)
    a = np.asarray(accept) != 0
    r = np.where(np.isnan(r), np.inf, r)
    m, C = r.shape
    best_all = np.full(m, np.inf)
    best_acc = np.full(m, np.inf)
    nearest = np.zeros(m, dtype=np.int64)
    index = np.full(m, -1, dtype=np.int64)
    for c in range(C):
        up = r[:, c] < best_all
        best_all[up], nearest[up] = r[up, c], c
        up = a[:, c] & ((index < 0) | (r[:, c] < best_acc))
        best_acc[up], index[up] = r[up, c], c
    return index, nearest, a.sum(1).astype(np.int64)


def count_tables(y_index, index, accept):
    """(table, accept_counts, n_accept_hist) int64 from the true class indices
    ``y_index`` (m,; a value outside [0, C) is the row "other" = C), the assigned
    ``index`` (−1: the column "none" = C) and the (m, C) 0/1 ``accept`` matrix."""
    a = np.asarray(accept) != 0
    m, C = a.shape
    y = np.asarray(y_index).astype(np.int64)
    y = np.where((y < 0) | (y >= C), C, y)
    col = np.where(np.asarray(index) < 0, C, np.asarray(index)).astype(np.int64)
    table = np.zeros((C + 1, C + 1), dtype=np.int64)
    acc = np.zeros((C + 1, C), dtype=np.int64)
    hist = np.zeros((C + 1, C + 1), dtype=np.int64)
    np.add.at(table, (y, col), 1)
    np.add.at(hist, (y, a.sum(1)), 1)
    for c in range(C):
        np.add.at(acc[:, c], y[a[:, c]], 1)
    return table, acc, hist


def confusion_from_counts(table, accept_counts, i: int):
    """TP, TN, FP, FN (np.int64) of class column i from the count blocks."""
    table, acc = np.asarray(table), np.asarray(accept_counts)
    n_true = np.int64(table[i].sum())
    n_other = np.int64(table.sum()) - n_true
    TP = np.int64(acc[i, i])
    FP = np.int64(acc[:, i].sum()) - TP
    return TP, n_other - FP, FP, n_true - TP


# ---- the rule that picks the route ------------------------------------------
# Measured on one MI355X, 1M float32 rows, device events, median of 7, the
# variants alternating in one process (scripts/bench_classify.py,
# profiles/classify_ab.json), with the count tables:
FUSED_AB_MS = {
    # (p, k per class, C): (ocm_score_multi_f32, classify_composed)
    (2048, 20, 3): (24.76, 7.30),   # per-class route: k_score_1p, one read of X per class
    (2048, 12, 4): (18.61, 7.83),
    (1000, 12, 4): (8.04, 7.79),    # per-class route: the two-sweep kernel; the fused tile stays in LDS
    (1536, 12, 4): (14.25, 10.97),  # per-class route: the two-sweep kernel; the fused tile does not fit the LDS
}


def fused_is_faster(p: int, ks) -> bool:
    """True on the shape classes where the A/B (``FUSED_AB_MS``) shows
    ocm_score_multi_f32 faster than ``classify_composed``.  It shows none: the
    fused kernel takes 3.4× / 2.4× the composition's time at p = 2048, 1.30× at
    p = 1536 and 1.03× at p = 1000, so ``SIMCA.classify`` takes the per-class
    kernels unless ``route="fused"`` asks for the one launch."""
    return False


def _assign_torch(ratio: torch.Tensor, accept: torch.Tensor):
    """``assign`` on device tensors (the epilogue of ``classify_composed``)."""
    m, C = ratio.shape
    dev = ratio.device
    r = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    a = accept != 0
    best_all = torch.full((m,), float("inf"), dtype=torch.float64, device=dev)
    best_acc = best_all.clone()
    nearest = torch.zeros(m, dtype=torch.int64, device=dev)
    index = torch.full((m,), -1, dtype=torch.int64, device=dev)
    for c in range(C):
        rc = r[:, c]
        up = rc < best_all
        best_all = torch.where(up, rc, best_all)
        nearest = torch.where(up, torch.full_like(nearest, c), nearest)
        up = a[:, c] & ((index < 0) | (rc < best_acc))
        best_acc = torch.where(up, rc, best_acc)
        index = torch.where(up, torch.full_like(index, c), index)
    return index, nearest, a.sum(1)


def _counts_torch(y_index: torch.Tensor, index: torch.Tensor, accept: torch.Tensor, n_accept: torch.Tensor):
    """The three count blocks in ocm_score_multi_f32's layout, from one bincount."""
    C = accept.shape[1]
    C1 = C + 1
    y = y_index.to(torch.int64).clamp(max=C)
    col = torch.where(index < 0, torch.full_like(index, C), index)
    rows, cols = torch.nonzero(accept, as_tuple=True)
    o_acc, o_hist = C1 * C1, C1 * C1 + C1 * C
    keys = torch.cat([y * C1 + col, o_acc + y[rows] * C + cols, o_hist + y * C1 + n_accept])
    cnt = torch.bincount(keys, minlength=C1 * (3 * C + 2))
    return cnt[:o_acc].view(C1, C1), cnt[o_acc:o_hist].view(C1, C), cnt[o_hist:].view(C1, C1)


def classify_composed(X, fits, decisions, y_index: torch.Tensor | None = None, distances: bool = False) -> dict:
    """What ocm_score_multi_f32 computes, from the per-class kernels
    (``engine.score`` + ``engine.decide``, one pass over X per class) and a torch
    epilogue: the route of the inputs the fused kernel does not take (float64
    spectra, a lazy ``PrepView``, more than 64 components or 8 classes) and the
    baseline of its tests and timings.  ``X``: what ``engine.as_device_x``
    returns; ``y_index``: uint8 device tensor of class indices (≥ C: other).
    Returns device tensors under the keys of ``engine.score_multi`` (``index``,
    ``nearest`` and ``n_accept`` int64)."""
    m = int(X.shape[0])
    C = len(fits)
    dev = X.device
    vdt = torch.float64 if X.dtype == torch.float64 else torch.float32
    pred = torch.zeros((m, C), dtype=torch.float64, device=dev)
    ratio = torch.zeros((m, C), dtype=torch.float64, device=dev)
    T2 = torch.zeros((m, C), dtype=torch.float64, device=dev) if distances else None
    Q = torch.zeros((m, C), dtype=vdt, device=dev) if distances else None
    for i, (fit, dec) in enumerate(zip(fits, decisions)):
        if m == 0:
            break
        sc = engine.score(X, None, m, fit.P64, fit.mean64, fit.inv_diag)
        acc = pred[:, i:] if C > 1 else pred
        _, _, dred = engine.decide(sc["T2"], sc["Q"], dec, want_red=False, want_dred=True, accept_out=acc,
                                   accept_stride=C)
        ratio[:, i] = dred / dec.dlim
        if distances:
            T2[:, i], Q[:, i] = sc["T2"], sc["Q"]
    index, nearest, n_accept = _assign_torch(ratio, pred)
    out = {"T2": T2, "Q": Q, "ratio": ratio, "pred": pred, "index": index, "nearest": nearest, "n_accept": n_accept,
           "table": None, "accept_counts": None, "n_accept_hist": None}
    if y_index is not None:
        out["table"], out["accept_counts"], out["n_accept_hist"] = _counts_torch(y_index, index, pred, n_accept)
    return out


def wold_distance(S, n, k, p: int) -> np.ndarray:
    """Wold's inter-class distance (Wold & Sjöström 1977) from the residual
    sums ``S[r, q] = Σ_{i∈r} Q_q(x_i)`` (the rows of class r against the model of
    class q), the class sizes ``n`` and the components ``k`` per class:
      s²[r|q] = S[r, q] / (n_r·(p − k_q))                  r ≠ q
      s²[q|q] = S[q, q] / ((n_q − k_q − 1)·(p − k_q))
      D[a, b] = sqrt((s²[a|b] + s²[b|a]) / (s²[a|a] + s²[b|b])),  D[a, a] = 1.
    (C, C) float64."""
    S = np.asarray(S, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    C = S.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = S / (n[:, None] * (p - k)[None, :])
        d = np.arange(C)
        s2[d, d] = S[d, d] / ((n - k - 1.0) * (p - k))
        D = np.sqrt((s2 + s2.T) / (s2[d, d][:, None] + s2[d, d][None, :]))
    D[d, d] = 1.0
    return D
