"""Object-wise cross-validation of SIMCA: folds that never cut an object, and
CV records from object decisions.

The pixels of one object (one nut, nut_data.py:131-185) are strongly
correlated, so a row fold that runs through an object leaks it into its own
training set.  ``ObjectKFoldWithExternalVal`` deals whole objects of the target
class to the folds (scikit-learn's ``GroupKFold`` on the object index) and keeps
the reference's external-validation test sets (held-out target rows followed by
every other row, utils/CVSIMCA.py:77-80).  Passed to
``utils.cross_validate_simca_grid`` it gives pixel-level records under
object-wise folds on the fold engine (ocm/cv.py).

``cross_validate_objects_grid`` selects LV and limits by *object* decisions,
those of ``SIMCA.predict_objects`` (utils/SIMCA.py:560-564): the fold engine
scores each fold's test rows once at LV_max, and ``ocm_cv_objects`` reduces them
to per-object votes and decision sums for every (param combo, LV) at once
(nothing of size configurations × rows exists).  Decisions and confusion counts
on the (configurations, objects) tables are torch operations.  Aggregation is
the reference's pixel rule at the object level (utils/CVSIMCA.py:190-208): spec
= mean over folds of TN/(TN+FP)·100 over the fold's test objects, sens from the
pooled object vector (target objects carry their own fold's decision, other
objects the last fold's), eff = √(sens·spec).

The object path is per-process: under a process group every rank computes the
rows it was given, with no fingerprint exchange and no collective.
"""
from __future__ import annotations

import numpy as np
from sklearn.model_selection import BaseCrossValidator, GroupKFold

from .objects import check_offsets, segment_offsets

__all__ = ["ObjectKFoldWithExternalVal", "cross_validate_objects_grid", "ObjectTables", "CV_OBJECT_RULES"]

CV_OBJECT_RULES = ("vote", "mean_distance")


def _host(a):
    if hasattr(a, "detach"):
        return a.detach().cpu().numpy()
    return np.asarray(a)


class ObjectKFoldWithExternalVal(BaseCrossValidator):
    """GroupKFold over the objects of the target class; every test set = the
    held-out target objects' rows + all other rows.

    Objects are runs of adjacent rows (``ocm.objects.segment_offsets``,
    ``SIMCA.predict_objects``): give exactly one of ``objects`` (m ids, one per
    row) and ``offsets`` (G + 1 row offsets from 0 to m).  Every row belongs to
    an object, no object is empty, and an object holds rows of one label only.
    The target rows come from ``cls_idx`` / ``cls_label`` as in
    ``ClasswiseKFoldWithExternalVal``."""

    def __init__(self, n_splits=5, objects=None, offsets=None, cls_idx=None, cls_label=None):
        if (objects is None) == (offsets is None):
            raise ValueError("ObjectKFoldWithExternalVal: give exactly one of objects= (m ids) and offsets= "
                             "(G + 1 row offsets)")
        self.n_splits = int(n_splits)
        self.objects = None if objects is None else _host(objects)
        self.offsets = None if offsets is None else _host(offsets)
        self.cls_idx = None if cls_idx is None else np.asarray(cls_idx)
        self.cls_label = cls_label

    def get_n_splits(self, X=None, y=None, groups=None):
        return self.n_splits

    def object_offsets(self, X) -> np.ndarray:
        """The (G + 1,) int64 row offsets of the objects, validated against X."""
        m = int(X.shape[0])
        if self.objects is not None:
            if self.objects.shape != (m,):
                raise ValueError(f"ObjectKFoldWithExternalVal: objects has shape {self.objects.shape}, X has {m} rows")
            off = segment_offsets(self.objects)
        else:
            off = check_offsets(self.offsets, m)
            if off[0] != 0 or off[-1] != m:
                raise ValueError(f"ObjectKFoldWithExternalVal: every row belongs to an object: offsets must run "
                                 f"from 0 to {m}, got {int(off[0])} to {int(off[-1])}")
        counts = np.diff(off)
        if (counts == 0).any():
            raise ValueError(f"ObjectKFoldWithExternalVal: object {int(np.flatnonzero(counts == 0)[0])} is empty")
        return off

    def target_indices(self, X, y=None) -> np.ndarray:
        """Ascending indices of the target-class rows (``cls_idx`` / ``cls_label``
        as ClasswiseKFoldWithExternalVal reads them)."""
        from utils.CVSIMCA import ClasswiseKFoldWithExternalVal

        rows = ClasswiseKFoldWithExternalVal(n_splits=self.n_splits, cls_idx=self.cls_idx, cls_label=self.cls_label)
        return np.sort(np.asarray(rows.target_indices(X, y), dtype=np.int64))

    def _layout(self, X, y):
        """(offsets, target rows, object index of every row, target objects)."""
        off = self.object_offsets(X)
        m = int(X.shape[0])
        G = off.size - 1
        obj = np.repeat(np.arange(G, dtype=np.int64), np.diff(off))
        first = off[:-1]
        if y is not None:
            yh = _host(y)
            if yh.shape[0] != m:
                raise ValueError(f"ObjectKFoldWithExternalVal: y has {yh.shape[0]} rows, X has {m}")
            mixed = np.flatnonzero(np.add.reduceat((yh != yh[first][obj]).astype(np.int64), first) > 0)
            if mixed.size:
                raise ValueError(f"ObjectKFoldWithExternalVal: object {int(mixed[0])} holds rows of more than one "
                                 "label")
        target = self.target_indices(X, y)
        if target.size and (target[0] < 0 or target[-1] >= m):
            raise ValueError(f"ObjectKFoldWithExternalVal: cls_idx is out of range for {m} rows")
        is_t = np.zeros(m, dtype=bool)
        is_t[target] = True
        n_t = np.add.reduceat(is_t.astype(np.int64), first)
        part = np.flatnonzero((n_t > 0) & (n_t < np.diff(off)))
        if part.size:
            raise ValueError(f"ObjectKFoldWithExternalVal: object {int(part[0])} holds rows of more than one label "
                             "(target and other rows)")
        t_objs = np.flatnonzero(n_t > 0)
        if t_objs.size < self.n_splits:
            raise ValueError(f"ObjectKFoldWithExternalVal: the target class has {t_objs.size} objects, fewer than "
                             f"n_splits={self.n_splits}")
        return off, target, obj, t_objs

    def target_folds(self, X, y=None):
        """The target rows of every fold (ascending), whole objects each:
        ``GroupKFold(n_splits)`` over the target rows, grouped by object."""
        _, target, obj, _ = self._layout(X, y)
        gkf = GroupKFold(n_splits=self.n_splits)
        return [target[held] for _, held in gkf.split(target, groups=obj[target])]

    def split(self, X, y=None, groups=None):
        _, target, obj, _ = self._layout(X, y)
        external = np.setdiff1d(np.arange(X.shape[0]), target)
        gkf = GroupKFold(n_splits=self.n_splits)
        for fit_pos, held_pos in gkf.split(target, groups=obj[target]):
            yield target[fit_pos], np.concatenate([target[held_pos], external])


class ObjectTables:
    """What the fold engine hands over per fold when it is asked for object-level
    results (``cv_grid(..., objects=tables)``): for the fold's test objects, in
    test-row order (held-out target objects, then the others), their global
    object index and row counts and the (configurations, objects) votes and
    decision sums.  Configurations are ordered combos outer, ascending LV inner."""

    def __init__(self, offsets: np.ndarray):
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.obj_of_row = np.repeat(np.arange(self.offsets.size - 1, dtype=np.int64), np.diff(self.offsets))
        self.want_votes = True  # fraction and score are reported under either rule
        self.want_dsum = True
        self.folds = {}

    def test_runs(self, test_rows: np.ndarray, n_fold_rows: int):
        """(offsets, object indices) of the runs of a fold's test rows (the
        first ``n_fold_rows`` are the held-out target rows); the rows of every
        object met must all be there, adjacent and in order."""
        ids = self.obj_of_row[test_rows]
        starts = np.concatenate([[0], np.flatnonzero(ids[1:] != ids[:-1]) + 1]).astype(np.int64)
        off = np.concatenate([starts, [ids.size]]).astype(np.int64)
        objs = ids[starts]
        if not np.array_equal(np.diff(off), np.diff(self.offsets)[objs]):
            raise ValueError("object-wise CV: a fold cuts an object (folds must be unions of whole objects)")
        return off, objs

    def add_fold(self, f, objs, off, votes, dsum):
        self.folds[f] = {"objs": objs, "counts": np.diff(off), "votes": votes, "dsum": dsum}


def _rates(TP, TN, FP, FN):
    """utils/SIMCA.py:246-250 on counts (NaN on an empty denominator)."""
    TP, TN, FP, FN = (np.float64(v) for v in (TP, TN, FP, FN))
    with np.errstate(divide="ignore", invalid="ignore"):
        return TP / (TP + FN) * 100, TN / (TN + FP) * 100


def _decide(fraction, score, rule, min_fraction):
    """predict_objects' decision (utils/SIMCA.py:564) on float64 fraction / score."""
    return (fraction >= float(min_fraction)) if rule == "vote" else (score > 0)


def _aggregate(per_fold, G, K, positive_obj, n_target_objs):
    """Object-level spec / sens of one configuration from its per-fold object
    decisions: ``per_fold[f]`` = (object indices, 0/1 decisions, fraction,
    score), the held-out target objects first (``n_target_objs[f]`` of them).
    → (spec, sens, pooled prediction, fraction, score) with (G,) vectors."""
    pooled = np.zeros(G)
    frac = np.full(G, np.nan)
    score = np.full(G, np.nan)
    step_spec = np.zeros(K)
    for f in range(K):
        objs, dec, fr, sc = per_fold[f]
        pos = positive_obj[objs]
        acc = dec == 1
        step_spec[f] = _rates(np.sum(acc & pos), np.sum(~acc & ~pos), np.sum(acc & ~pos), np.sum(~acc & pos))[1]
        keep = slice(0, n_target_objs[f]) if f < K - 1 else slice(0, objs.size)
        pooled[objs[keep]] = dec[keep]
        frac[objs[keep]] = fr[keep]
        score[objs[keep]] = sc[keep]
    acc = pooled == 1
    sens = _rates(np.sum(acc & positive_obj), np.sum(~acc & ~positive_obj), np.sum(acc & ~positive_obj),
                  np.sum(~acc & positive_obj))[0]
    return float(np.mean(step_spec)), float(sens), pooled, frac, score


def _engine_grid(template, X, y, cv, lv_values, param_grid, rule, min_fraction, class_index, store_predictions):
    """The fold-engine path: (records, by_combo), or None when ocm.cv does not
    cover the configuration."""
    import torch

    from . import cv as fold_engine

    app = fold_engine._applicable(template, X, y, cv, lv_values, param_grid)
    if app is None:
        return None
    cls_idx, tl, combos, base = app
    y = np.asarray(_host(y))
    off, _, obj, _ = cv._layout(X, y)
    folds = cv.target_folds(X, y)
    ci = [tl] if class_index is None else class_index
    tables = ObjectTables(off)
    px, _ = fold_engine.cv_grid(X, y, folds, cls_idx, lv_values, combos, base, ci, False, objects=tables)
    G, K = off.size - 1, len(folds)
    positive = (y == np.asarray(ci)) if np.ndim(ci) else (y == ci)
    positive_obj = np.asarray(positive, dtype=bool).reshape(y.shape[0])[off[:-1]]
    lvs = sorted(set(int(v) for v in lv_values))
    # decisions of every configuration on the (ncfg, objects) tables, fold by fold
    dec, frac, score, n_t = [], [], [], []
    for f in range(K):
        t = tables.folds[f]
        n = torch.from_numpy(t["counts"].astype(np.float64)).to(t["votes"].device)
        fr = t["votes"].to(torch.float64) / n
        sc = t["dsum"] / n
        dec.append(_decide(fr, sc, rule, min_fraction).to(torch.float64).cpu().numpy())
        frac.append(fr.cpu().numpy())
        score.append(sc.cpu().numpy())
        n_t.append(int(np.unique(obj[folds[f]]).size))
    records, by_combo = [], []
    for ci_, combo in enumerate(combos):
        for lv in lv_values:
            c = ci_ * len(lvs) + lvs.index(int(lv))
            per_fold = [(tables.folds[f]["objs"], dec[f][c], frac[f][c], score[f][c]) for f in range(K)]
            spec, sens, pooled, fr, sc = _aggregate(per_fold, G, K, positive_obj, n_t)
            p = px[len(records)]
            records.append({"params": combo.copy(), "LV": lv, "spec": spec, "sens": sens,
                            "eff": float(np.sqrt(sens * spec)), "spec_px": p["spec"], "sens_px": p["sens"],
                            "eff_px": p["eff"]})
            if store_predictions:
                by_combo.append({"params": combo.copy(), "LV": lv, "prediction": pooled, "fraction": fr,
                                 "score": sc})
    return records, by_combo


def _predict_objects_of(model, X, ids, rule, min_fraction):
    """``predict_objects`` of a fitted estimator (a Pipeline: its last step on
    the rows transformed by the steps before it) → host (pred, fraction, score)."""
    from sklearn.pipeline import Pipeline

    if isinstance(model, Pipeline):
        for _, step in model.steps[:-1]:
            X = step.transform(X)
        model = model.steps[-1][1]
    if not hasattr(model, "predict_objects"):
        raise TypeError(f"cross_validate_objects_grid: {type(model).__name__} has no predict_objects")
    res = model.predict_objects(X, objects=ids, rule=rule, min_fraction=min_fraction)
    pred, fr, sc = (np.asarray(_host(v), dtype=np.float64) for v in (res.pred, res.fraction, res.score))
    if pred.ndim == 2 and pred.shape[1] != 1:
        raise ValueError("cross_validate_objects_grid: the fold models must have one class "
                         f"(got {pred.shape[1]}); set model_class")
    return pred.reshape(-1), fr.reshape(-1), sc.reshape(-1)


def _loop_grid(template, X, y, cv, lv_values, param_grid, ncomp_key, rule, min_fraction, class_index,
               store_predictions):
    """Generic path: a refit per (setting, fold) and ``predict_objects`` on the
    fold's test rows; the pixel-level values come from ``predict`` on the same
    fold models (the reference's loop, utils/CVSIMCA.py:145-222)."""
    from sklearn.base import clone

    from utils.CVSIMCA import _configured, _fold_predictions, _get_simca, _settings

    yh = np.asarray(_host(y))
    off, _, obj, _ = cv._layout(X, yh)
    G = off.size - 1
    splits = list(cv.split(X, yh))
    K = len(splits)
    folds = cv.target_folds(X, yh)
    n_t = [int(np.unique(obj[f]).size) for f in folds]
    records, by_combo = [], []
    for combo, lv in _settings(param_grid, lv_values):
        est = _configured(template, combo, ncomp_key, lv)
        per_fold, pooled_px, spec_px = [], np.zeros(X.shape[0]), np.zeros(K)
        simca = None
        for f, (fit_rows, test_rows) in enumerate(splits):
            model = clone(est)
            model.fit(X[fit_rows, :], yh[fit_rows])
            simca = _get_simca(model)
            ci = class_index if class_index is not None else getattr(simca, "model_class", 1)
            pred_px = _fold_predictions(model, X[test_rows, :], yh[test_rows])
            pooled_px[test_rows] = pred_px
            spec_px[f] = simca._metrics_simca_conformity(y_true=yh[test_rows], y_pred=pred_px,
                                                         class_index=ci)["specificity"]
            ids = obj[test_rows]
            pred, fr, sc = _predict_objects_of(model, X[test_rows, :], ids, rule, min_fraction)
            starts = np.concatenate([[0], np.flatnonzero(ids[1:] != ids[:-1]) + 1])
            per_fold.append((ids[starts], pred, fr, sc))
        ci = class_index if class_index is not None else getattr(simca, "model_class", 1)
        sens_px = float(simca._metrics_simca_conformity(y_true=yh, y_pred=pooled_px, class_index=ci)["sensitivity"])
        positive = (yh == np.asarray(ci)) if np.ndim(ci) else (yh == ci)
        positive_obj = np.asarray(positive, dtype=bool).reshape(yh.shape[0])[off[:-1]]
        spec, sens, pooled, fr, sc = _aggregate(per_fold, G, K, positive_obj, n_t)
        spx = float(np.mean(spec_px))
        LV = combo.get(ncomp_key) if lv is None else lv
        records.append({"params": combo.copy(), "LV": LV, "spec": spec, "sens": sens,
                        "eff": float(np.sqrt(sens * spec)), "spec_px": spx, "sens_px": sens_px,
                        "eff_px": float(np.sqrt(sens_px * spx))})
        if store_predictions:
            by_combo.append({"params": combo.copy(), "LV": LV, "prediction": pooled, "fraction": fr, "score": sc})
    return records, by_combo


def cross_validate_objects_grid(estimator, X, y, cv, LV_min=2, LV_max=10, param_grid=None, rule="vote",
                                min_fraction=0.5, refit_metric="eff", class_index=None, print_summary=True,
                                store_predictions=False):
    """Grid × LV class-wise CV by object decisions, with refit on all rows.

    ``cv``: an ``ObjectKFoldWithExternalVal``.  Returns the dictionary of
    ``utils.cross_validate_simca_grid`` ({results, best_params, best_LV,
    best_score, best_estimator[, by_combo]}); each record's ``spec`` / ``sens``
    / ``eff`` are object-level (``rule``: "vote" = accepted pixels / count ≥
    ``min_fraction``, "mean_distance" = mean decision value > 0, as
    ``SIMCA.predict_objects``) and ``spec_px`` / ``sens_px`` / ``eff_px`` the
    pixel-level values of the same pass.  ``by_combo[i]`` holds ``prediction``,
    ``fraction`` and ``score`` per object (G,).

    This package's SIMCA (not in a Pipeline, one target label, float32 or a
    lazy view, LV ≤ 64) runs on the fold engine; anything else refits per
    (setting, fold).  Per-process under a process group."""
    from sklearn.base import clone

    from utils.CVSIMCA import _REFIT_KEYS, _find_ncomp_param_name, _summary_lines

    from .replica import per_process

    if rule not in CV_OBJECT_RULES:
        raise ValueError(f"cross_validate_objects_grid: rule={rule!r} (one of {', '.join(CV_OBJECT_RULES)})")
    if not 0.0 < float(min_fraction) <= 1.0:
        raise ValueError(f"cross_validate_objects_grid: min_fraction={min_fraction!r} must lie in (0, 1]")
    if not isinstance(cv, ObjectKFoldWithExternalVal):
        raise TypeError("cross_validate_objects_grid: cv must be an ObjectKFoldWithExternalVal")
    param_grid = {} if param_grid is None else param_grid
    template = clone(estimator)
    ncomp_key = _find_ncomp_param_name(template)
    lv_in_grid = any(name.endswith("n_components") for name in param_grid)
    lv_values = None if lv_in_grid else list(range(LV_min, LV_max + 1))

    with per_process():
        got = _engine_grid(template, X, y, cv, lv_values, param_grid, rule, min_fraction, class_index,
                           store_predictions)
        if got is None:
            got = _loop_grid(template, X, y, cv, lv_values, param_grid, ncomp_key, rule, min_fraction, class_index,
                             store_predictions)
        records, by_combo = got
        metric = _REFIT_KEYS[refit_metric]
        best = records[int(np.argmax([r[metric] for r in records]))]  # first maximum, as the pixel-level grid
        if print_summary:
            for line in _summary_lines(records, refit_metric, best):
                print(line)
        refit = clone(estimator)
        refit.set_params(**best["params"])
        if not lv_in_grid:
            refit.set_params(**{_find_ncomp_param_name(refit): best["LV"]})
        refit.fit(X, y)

    result = {"results": records, "best_params": best["params"].copy(), "best_LV": best["LV"],
              "best_score": best[metric], "best_estimator": refit}
    if store_predictions:
        result["by_combo"] = by_combo
    return result
