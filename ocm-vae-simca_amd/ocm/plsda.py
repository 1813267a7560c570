"""PLS-DA: Gram-space PLS, LDA on the scores, the component sweep in one pass.

The discriminant baseline of data_cheese.py:193-328: ``PLSRegression(a)`` on
the class target, ``LinearDiscriminantAnalysis`` on the PLS scores, for every
a = 1..25 on the calibration set and on each of 5 stratified folds (150
scikit-learn fits).  Here:

* **Gram-space PLS** (Dayal & MacGregor's improved kernel algorithm): the
  recursion needs only S = XcᵀXc and s = XcᵀYc of the centred, scaled training
  rows.  One segmented Gram over (fold, class) segments gives both (the column
  sums of a class segment are the class sums); a fold's training moments are
  the totals minus the fold's segments.  ``ocm_pls_fit_f64`` runs the
  recursion of the full fit and of every fold in one call.
* **Orthogonal scores**: TᵀT = diag(tt), so the LDA on T[:, :a] needs only
  tt[:a] and the class means of the scores Rᵀ(m_c − m): no further pass over X.
* **Nested rotations**: R_a is the first a columns of R_A, so one projection at
  A gives the scores of every a ≤ A and one epilogue applies each a's LDA
  (``ocm_plsda_predict_f32``: one read of X for the whole sweep).

``pls_from_moments`` is the same recursion in NumPy (the kernels' oracle).
"""
from __future__ import annotations

import numpy as np

__all__ = ["PLSDA", "plsda_cv_curve", "pls_from_moments", "lda_tables", "macro_f1_from_counts", "pls_moments"]

MAX_COMPONENTS = 64
MAX_CLASSES = 8


# --------------------------------------------------------------------------- host oracle
def jacobi_dominant(G, dtype=np.float64):
    """Dominant eigenvector of the symmetric matrix G by cyclic Jacobi (the
    arithmetic of csrc/ocm_pls.hip's jacobi_dominant, in ``dtype``)."""
    G = np.array(G, dtype=dtype)
    M = G.shape[0]
    V = np.eye(M, dtype=dtype)
    eps2 = dtype(np.finfo(dtype).eps) ** 2 * dtype(0.25) if dtype is not np.float64 else dtype(2.0 ** -104)
    one = dtype(1)
    for _ in range(30):
        off = sum(G[i, j] * G[i, j] for i in range(M) for j in range(i + 1, M))
        dg = sum(G[i, i] * G[i, i] for i in range(M))
        if not off > eps2 * dg:
            break
        for i in range(M - 1):
            for j in range(i + 1, M):
                gij = G[i, j]
                if gij == 0:
                    continue
                theta = (G[j, j] - G[i, i]) / (2 * gij)
                t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                sn = t * c
                a, b = G[:, i].copy(), G[:, j].copy()
                G[:, i], G[:, j] = c * a - sn * b, sn * a + c * b
                a, b = G[i, :].copy(), G[j, :].copy()
                G[i, :], G[j, :] = c * a - sn * b, sn * a + c * b
                G[i, j] = G[j, i] = 0
                a, b = V[:, i].copy(), V[:, j].copy()
                V[:, i], V[:, j] = c * a - sn * b, sn * a + c * b
    return V[:, int(np.argmax(np.diag(G)))]


def pls_from_moments(S, s, A: int, dtype=np.float64) -> dict:
    """The PLS recursion on S = XcᵀXc (p, p) and s = XcᵀYc (p, M) in ``dtype``
    (float64, or ``np.longdouble`` to measure float64's own rounding).  For
    a = 0..A−1: w = s (M = 1) or s·c with c the dominant eigenvector of sᵀs,
    unit norm, largest-magnitude entry positive (sklearn's ``_svd_flip_1d``);
    r = w − Σ_{j<a} (p_jᵀw) r_j; v = S r; tt = rᵀv; p = v/tt; q = sᵀr/tt;
    s −= tt p qᵀ.  Stops where ‖s‖² ≤ 2⁻¹⁰⁰‖s₀‖² or tt ≤ 0 (sklearn's "y residual
    is constant").  Returns ``W``, ``R``, ``P`` (A, p), ``q`` (A, M), ``tt`` (A,),
    ``ncomp``; rows past ``ncomp`` are zeros."""
    S = np.asarray(S, dtype=dtype)
    s = np.array(s, dtype=dtype)
    if s.ndim == 1:
        s = s[:, None]
    p, M = s.shape
    W = np.zeros((A, p), dtype)
    R = np.zeros((A, p), dtype)
    P = np.zeros((A, p), dtype)
    q = np.zeros((A, M), dtype)
    tt = np.zeros(A, dtype)
    ss0 = (s * s).sum()
    ncomp = 0
    for a in range(A):
        if (s * s).sum() <= dtype(2.0 ** -100) * ss0:
            break
        w = s[:, 0].copy() if M == 1 else s @ jacobi_dominant(s.T @ s, dtype)
        bi = int(np.argmax(np.abs(w)))
        w = w * ((-1 if w[bi] < 0 else 1) / np.sqrt(w @ w))
        r = w.copy()
        for j in range(a):
            r = r - (P[j] @ w) * R[j]
        v = S @ r
        t2 = r @ v
        if not t2 > 0:
            break
        W[a], R[a], P[a], q[a], tt[a] = w, r, v / t2, (s.T @ r) / t2, t2
        s = s - t2 * np.outer(P[a], q[a])
        ncomp = a + 1
    return {"W": W, "R": R, "P": P, "q": q, "tt": tt, "ncomp": ncomp}


def lda_tables(tt, class_means, class_counts, lv_values, k: int | None = None):
    """The LDA of the first a score columns for every a in ``lv_values``, from
    moments alone: the scores are centred and orthogonal with TᵀT = diag(tt), so
    the pooled within-class covariance is (diag(tt[:a]) − Σ n_c m_c m_cᵀ)/(n − C)
    with m_c (C, A) the class means of the scores; priors n_c/n;
    coef_c = Σ_w⁻¹ m_c; b_c = −½ m_cᵀcoef_c + log prior_c (fp64, on the host).
    Returns ``coef`` (nlv, C, k) zero past a, and ``intercept`` (nlv, C)."""
    tt = np.asarray(tt, np.float64)
    mc = np.asarray(class_means, np.float64)
    nc = np.asarray(class_counts, np.float64)
    C, A = mc.shape
    k = A if k is None else k
    n = nc.sum()
    coef = np.zeros((len(lv_values), C, k))
    icpt = np.zeros((len(lv_values), C))
    for l, a in enumerate(lv_values):
        a = int(a)
        m = mc[:, :a]
        Sw = (np.diag(tt[:a]) - (m.T * nc) @ m) / (n - C)
        cf = np.linalg.solve(Sw, m.T).T
        coef[l, :, :a] = cf
        icpt[l] = -0.5 * np.einsum("ca,ca->c", m, cf) + np.log(nc / n)
    return coef, icpt


def macro_f1_from_counts(counts) -> np.ndarray:
    """Macro F1 from confusion counts (..., C, C) = [true][pred], as
    ``sklearn.metrics.f1_score(average="macro")``: the mean over the labels
    present in truth or prediction of 2tp/(2tp + fp + fn), an empty denominator
    giving 0."""
    c = np.asarray(counts, np.float64)
    tp = np.diagonal(c, axis1=-2, axis2=-1)
    den = c.sum(-1) + c.sum(-2)  # (tp + fn) + (tp + fp)
    present = den > 0
    f1 = np.where(present, 2 * tp / np.where(present, den, 1.0), 0.0)
    npres = present.sum(-1)
    return np.where(npres > 0, f1.sum(-1) / np.maximum(npres, 1), 0.0)


def _targets(classes, target: str) -> np.ndarray:
    """(C, M) target rows per class: the class value (label) or the indicator."""
    if target == "label":
        try:
            return np.asarray(classes, np.float64)[:, None]
        except (TypeError, ValueError):
            raise ValueError('PLSDA(target="label") regresses on the class values: they must be numeric') from None
    if target == "onehot":
        return np.eye(len(classes))
    raise ValueError('target must be "label" or "onehot"')


def _class_index(y, classes=None):
    y = np.asarray(y).ravel()
    if classes is None:
        classes, yi = np.unique(y, return_inverse=True)
    else:
        yi = np.searchsorted(classes, y)
        yi = np.where((yi < len(classes)) & (classes[np.minimum(yi, len(classes) - 1)] == y), yi, 255)
    return classes, yi.astype(np.int64)


# --------------------------------------------------------------------------- moments on the device
def pls_moments(G, cs, shift32, counts, Yv, scale: bool):
    """Centred, scaled PLS moments of the rows of some class segments, all on the
    device in fp64.  G (p, p) and cs (C, p): the Gram and per-class column sums
    of x − shift; counts (C,) rows per class; Yv (C, M) target rows per class.
    Returns S (p, p), s (p, M), mean (p,), sd (p,), class_dev (C, p) = the
    standardised class means minus the mean, ybar (M,), ysd (M,)."""
    import torch

    from . import engine

    n = float(counts.sum())
    nc = torch.as_tensor(np.asarray(counts, np.float64), device=G.device)
    C_, mean = engine.cov_from_gram([(1.0, G, cs.sum(0))], shift32, int(n))
    var = torch.diagonal(C_)
    sd = torch.sqrt(var.clamp_min(0.0)) if scale else torch.ones_like(var)
    sd = torch.where(sd == 0.0, torch.ones_like(sd), sd)  # sklearn: a constant column is left unscaled
    S = (n - 1.0) * C_ / (sd[:, None] * sd[None, :])
    d = cs.sum(0) / n  # mean of x − shift
    dev_sum = cs - nc[:, None] * d[None, :]  # Σ_{rows of c} (x − mean)
    Y = torch.as_tensor(np.asarray(Yv, np.float64), device=G.device)
    ybar = (nc[:, None] * Y).sum(0) / n
    Yc = Y - ybar
    ysd = torch.sqrt((nc[:, None] * Yc * Yc).sum(0) / (n - 1.0)) if scale else torch.ones_like(ybar)
    ysd = torch.where(ysd == 0.0, torch.ones_like(ysd), ysd)
    s = (dev_sum / sd[None, :]).T @ (Yc / ysd)
    class_dev = dev_sum / nc[:, None] / sd[None, :]
    return S, s, mean, sd, class_dev, ybar, ysd


def _device_x(X):
    """Host or device spectra -> (float32 device matrix, came from the host).
    A lazy ``PrepView`` is materialised; float64 input is converted to float32
    (``engine.as_device_f32``): the kernels read float32."""
    import torch

    from . import engine
    from .prepview import PrepView

    host = not isinstance(X, (torch.Tensor, PrepView)) or (isinstance(X, torch.Tensor) and not X.is_cuda)
    if isinstance(X, PrepView):
        X = engine._plain(X)
        if isinstance(X, PrepView):
            X = X.materialize()
    X = engine.as_device_f32(X)
    if X.dim() != 2:
        raise ValueError("X must be 2-D (rows × variables)")
    return X, host


def _segment_gram(X, seg_id, nseg):
    """One Gram pass over the rows of X grouped by ``seg_id`` (host int array in
    [0, nseg)): per-segment Grams (nseg, p, p), column sums (nseg, p), the shift."""
    import torch

    from . import engine

    order = np.argsort(seg_id, kind="stable")
    sizes = np.bincount(seg_id, minlength=nseg)
    if (sizes == 0).any():
        raise ValueError("every (fold, class) segment needs at least one row")
    offs = np.concatenate([[0], np.cumsum(sizes)])
    rows = torch.from_numpy(order.astype(np.int64)).to(X.device)
    n = len(seg_id)
    shift = engine.cast_f32(engine.colmean(X, rows, max(1, min(n, engine.SHIFT_SAMPLE))))
    G, cs = engine.gram(X, rows, offs, shift)
    return G, cs, shift, sizes


class _Model:
    """One fitted PLS + LDA (device projection, host tables)."""

    def __init__(self, fit, b, mean, sd, class_dev, counts):
        import torch

        self.ncomp = int(fit["ncomp"][b].item())
        self.R = fit["R"][b]  # (A, p) device
        self.mean, self.sd = mean, sd
        self.proj = (self.R / sd[None, :]).contiguous()  # t = proj (x − mean)
        self.tt = fit["tt"][b].cpu().numpy()
        self.class_means = (class_dev @ self.R.T).cpu().numpy()  # (C, A): Rᵀ(m_c − m)
        self.counts = np.asarray(counts, np.float64)
        self._torch = torch

    def table(self, lv_values):
        """LDA table of the prefixes (device, float64) and the effective lvs."""
        if self.ncomp < 1:
            raise ValueError("PLS completed no component: the target is constant")
        k = self.R.shape[0]
        lv = [min(int(a), self.ncomp) for a in lv_values]
        coef, icpt = lda_tables(self.tt, self.class_means, self.counts, lv, k)
        tab = np.concatenate([coef.ravel(), icpt.ravel()])
        return self._torch.from_numpy(tab).to(self.R.device), lv


class PLSDA:
    """PLS regression on the class target, LDA on the scores (data_cheese.py:200-207).

    ``target="label"`` regresses on the class values as one column (the
    reference's ``pls.fit(Xtr_data, Xtr_label)``), ``"onehot"`` on the indicator
    matrix.  ``scale`` as ``PLSRegression(scale=)``: X and the target are
    centred and divided by their standard deviation (ddof = 1; a zero one is 1).

    Host input gives host output, device input device output.  A lazy
    ``PrepView`` is materialised first; float64 input is converted to float32
    (``engine.as_device_f32``).  Under a process group every call is
    per-process (no sharding).

    After ``fit``: ``classes_``, ``x_mean_``, ``x_std_``, ``x_weights_``,
    ``x_rotations_``, ``x_loadings_`` (p, A), ``y_loadings_`` (M, A),
    ``score_ss_`` (A,) = tᵀt per component, ``n_components_`` (completed), and
    the LDA of every prefix a ≤ A: ``lda_coef_`` (A, C, A), ``lda_intercept_``
    (A, C)."""

    def __init__(self, n_components: int = 10, target: str = "label", scale: bool = True):
        self.n_components = n_components
        self.target = target
        self.scale = scale

    def fit(self, X, y):
        import torch

        from . import engine

        Xd, _ = _device_x(X)
        n, p = Xd.shape
        A = int(self.n_components)
        if not 1 <= A <= min(p, MAX_COMPONENTS):
            raise ValueError(f"n_components={A} must be in [1, min(p, {MAX_COMPONENTS})]")
        self.classes_, yi = _class_index(y)
        C = len(self.classes_)
        if len(yi) != n:
            raise ValueError("X and y differ in length")
        if not 2 <= C <= MAX_CLASSES:
            raise ValueError(f"PLSDA needs 2..{MAX_CLASSES} classes, got {C}")
        if n <= C:
            raise ValueError("PLSDA needs more rows than classes")
        Yv = _targets(self.classes_, self.target)
        G, cs, shift, sizes = _segment_gram(Xd, yi, C)
        S, s, mean, sd, class_dev, ybar, ysd = pls_moments(G.sum(0), cs, shift, sizes, Yv, self.scale)
        fit = engine.pls_fit(S[None], s[None], A)
        self._model = _Model(fit, 0, mean, sd, class_dev, sizes)
        self._set_attributes(fit, 0, ybar, ysd)
        return self

    def _set_attributes(self, fit, b, ybar, ysd):
        mdl = self._model
        A = mdl.R.shape[0]
        self.n_components_ = mdl.ncomp
        self.x_mean_ = mdl.mean.cpu().numpy()
        self.x_std_ = mdl.sd.cpu().numpy()
        self.y_mean_ = ybar.cpu().numpy()
        self.y_std_ = ysd.cpu().numpy()
        self.x_weights_ = fit["W"][b].T.cpu().numpy()
        self.x_rotations_ = fit["R"][b].T.cpu().numpy()
        self.x_loadings_ = fit["P"][b].T.cpu().numpy()
        self.y_loadings_ = fit["q"][b].T.cpu().numpy()
        self.score_ss_ = mdl.tt.copy()
        self.class_count_ = mdl.counts.copy()
        self.class_score_means_ = mdl.class_means.copy()
        lvs = list(range(1, max(mdl.ncomp, 1) + 1))
        self.lda_coef_ = np.zeros((A, len(self.classes_), A))
        self.lda_intercept_ = np.zeros((A, len(self.classes_)))
        if mdl.ncomp >= 1:
            coef, icpt = lda_tables(mdl.tt, mdl.class_means, mdl.counts, lvs, A)
            self.lda_coef_[:len(lvs)], self.lda_intercept_[:len(lvs)] = coef, icpt
            self.lda_coef_[len(lvs):], self.lda_intercept_[len(lvs):] = coef[-1], icpt[-1]

    @staticmethod
    def _out(t, host):
        return t.cpu().numpy() if host and t is not None else t

    def transform(self, X):
        """The PLS scores (m, A), float32."""
        from . import engine

        Xd, host = _device_x(X)
        out = engine.plsda_predict(Xd, None, Xd.shape[0], self._model.proj, self._model.mean, want_T=True,
                                   want_pred=False)
        return self._out(out["T"], host)

    def _lv(self, n_components):
        a = self._model.R.shape[0] if n_components is None else int(n_components)
        if not 1 <= a <= self._model.R.shape[0]:
            raise ValueError(f"n_components={a} must be in [1, {self._model.R.shape[0]}]")
        return a

    def decision_function(self, X, n_components=None):
        """The C class scores (m, C) of the LDA on the first ``n_components``
        PLS scores (all of them by default), float32."""
        from . import engine

        Xd, host = _device_x(X)
        tab, lv = self._model.table([self._lv(n_components)])
        out = engine.plsda_predict(Xd, None, Xd.shape[0], self._model.proj, self._model.mean, lv, len(self.classes_),
                                   tab, want_D=True, want_pred=False)
        return self._out(out["D"][:, 0, :], host)

    def predict(self, X, n_components=None):
        """Class labels (m,)."""
        pred = self.predict_sweep(X, [self._lv(n_components)])
        return pred[:, 0]

    def predict_sweep(self, X, lv_values, y_true=None, rows=None):
        """Predicted labels (m, nlv) for every number of components in
        ``lv_values`` (ascending) from one launch, and with ``y_true`` also the
        confusion counts (nlv, C, C) = [lv][true][pred] (a label outside
        ``classes_`` counts nowhere).  ``rows``: optional row indices into X (the
        rows scored, without a gather copy); ``y_true`` then belongs to them."""
        import torch

        from . import engine

        Xd, host = _device_x(X)
        lv_values = [int(a) for a in lv_values]
        if any(b <= a for a, b in zip(lv_values, lv_values[1:])):
            raise ValueError("lv_values must be ascending")
        if not lv_values or lv_values[0] < 1 or lv_values[-1] > self._model.R.shape[0]:
            raise ValueError(f"lv_values must lie in [1, {self._model.R.shape[0]}]")
        tab, lv = self._model.table(lv_values)
        if rows is not None:
            rows = torch.as_tensor(np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows, np.int64)
                                   ).to(Xd.device)
        m = Xd.shape[0] if rows is None else rows.numel()
        yt = None
        if y_true is not None:
            if isinstance(y_true, torch.Tensor) and y_true.is_cuda and y_true.dtype == torch.uint8:
                yt = y_true.contiguous()  # class indices already
            else:
                yh = y_true.cpu().numpy() if isinstance(y_true, torch.Tensor) else y_true
                yt = torch.from_numpy(_class_index(yh, self.classes_)[1].astype(np.uint8)).to(Xd.device)
        out = engine.plsda_predict(Xd, rows, m, self._model.proj, self._model.mean, lv, len(self.classes_), tab,
                                   y_true=yt)
        idx = out["pred"]
        if host:
            labels = self.classes_[idx.cpu().numpy()]
            return labels if y_true is None else (labels, out["counts"].cpu().numpy())
        try:
            cls = torch.as_tensor(self.classes_, device=Xd.device)
            labels = cls[idx.long()]
        except (TypeError, ValueError, RuntimeError):  # labels torch cannot hold: the class indices
            labels = idx
        return labels if y_true is None else (labels, out["counts"])


def plsda_cv_curve(X, y, lv_values=range(1, 26), n_splits: int = 5, shuffle: bool = True, random_state=42,
                   target: str = "label", scale: bool = True) -> dict:
    """The macro-F1 curves of data_cheese.py:193-224 from one Gram pass.

    Folds from ``StratifiedKFold(n_splits, shuffle, random_state)`` (:195); one
    Gram over (fold, class) segments; one ``ocm_pls_fit_f64`` over the full fit
    and the ``n_splits`` fold fits (a fold trains on the totals minus its own
    segments); one ``predict_sweep`` per fold on its held-out rows by index and
    one on all rows with the full model.  Returns ``f1_cal`` (nlv,), ``f1_cv``
    (nlv,) = the mean over folds of the fold's macro F1 (:210-224),
    ``counts_cal`` (nlv, C, C), ``counts_cv`` (n_splits, nlv, C, C),
    ``lv_values``, ``classes`` and the fitted full-data ``model``."""
    import torch
    from sklearn.model_selection import StratifiedKFold

    from . import engine

    Xd, _ = _device_x(X)
    n, p = Xd.shape
    lv_values = [int(a) for a in lv_values]
    A = max(lv_values)
    if not 1 <= min(lv_values) or A > min(p, MAX_COMPONENTS):
        raise ValueError(f"lv_values must lie in [1, min(p, {MAX_COMPONENTS})]")
    classes, yi = _class_index(y)
    C = len(classes)
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"PLSDA needs 2..{MAX_CLASSES} classes, got {C}")
    Yv = _targets(classes, target)
    skf = StratifiedKFold(n_splits=n_splits, shuffle=shuffle, random_state=random_state if shuffle else None)
    fold = np.empty(n, np.int64)
    for f, (_, val) in enumerate(skf.split(np.zeros((n, 1)), yi)):
        fold[val] = f
    G, cs, shift, sizes = _segment_gram(Xd, fold * C + yi, n_splits * C)
    Gf = G.view(n_splits, C, p, p).sum(1)  # per-fold Grams
    csf = cs.view(n_splits, C, p)
    szf = sizes.reshape(n_splits, C)
    Gtot, cstot, sztot = Gf.sum(0), csf.sum(0), szf.sum(0)
    probs = [pls_moments(Gtot, cstot, shift, sztot, Yv, scale)]
    for f in range(n_splits):  # fp64 downdating: the fold's training rows are all rows but its own
        probs.append(pls_moments(Gtot - Gf[f], cstot - csf[f], shift, sztot - szf[f], Yv, scale))
    del G, Gf
    fit = engine.pls_fit(torch.stack([q[0] for q in probs]), torch.stack([q[1] for q in probs]), A)
    models = [_Model(fit, b, q[2], q[3], q[4], (sztot if b == 0 else sztot - szf[b - 1]))
              for b, q in enumerate(probs)]
    est = PLSDA(A, target, scale)
    est.classes_ = classes
    est._model = models[0]
    est._set_attributes(fit, 0, probs[0][5], probs[0][6])
    yt = torch.from_numpy(yi.astype(np.uint8)).to(Xd.device)
    _, counts_cal = est.predict_sweep(Xd, lv_values, y_true=yt)
    counts_cv = []
    fold_est = PLSDA(A, target, scale)
    fold_est.classes_ = classes
    for f in range(n_splits):
        rows = torch.from_numpy(np.flatnonzero(fold == f)).to(Xd.device)
        fold_est._model = models[1 + f]
        _, cnt = fold_est.predict_sweep(Xd, lv_values, y_true=yt[rows].contiguous(), rows=rows)
        counts_cv.append(cnt)
    counts_cal = counts_cal.cpu().numpy()
    counts_cv = torch.stack(counts_cv).cpu().numpy()
    return {"f1_cal": macro_f1_from_counts(counts_cal), "f1_cv": macro_f1_from_counts(counts_cv).mean(0),
            "counts_cal": counts_cal, "counts_cv": counts_cv, "lv_values": lv_values, "classes": classes,
            "model": est, "folds": fold}
