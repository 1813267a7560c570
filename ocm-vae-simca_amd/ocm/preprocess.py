"""Spectral preprocessing on the GPU.

``snv_savgol(X, window_length, polyorder, deriv, delta, snv=True)`` applies
the drivers' preprocessing as ONE HBM pass per row (``ocm_snv_savgol_f32``):

    SNV (simca_nuts.py:47-49, utils/data_utils.py:57):
        x ← (x − mean_row) / (std_row + 1e-8)      np.std ddof 0, float32 result
    Savitzky–Golay (simca_nuts.py:51, simca_new_cheese.py:37-38):
        scipy.signal.savgol_filter(x, window_length, polyorder, deriv, delta,
                                   axis=1, mode='interp')

``mode='interp'`` is linear in the samples, so it is a set of taps: the
interior correlation coefficients (``savgol_coeffs(..., use='dot')``) and,
for the first / last ``window_length // 2`` outputs, the rows of the map
"least-squares polynomial fit of the first / last window, differentiated
``deriv`` times, evaluated there" (scipy's ``_fit_edge``), built here by
fitting the identity.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
from scipy.signal import savgol_coeffs

from . import _lib, engine
from ._lib import Context, check, ptr
from .prepview import PrepView

__all__ = ["savgol_taps", "snv_savgol", "snv", "savgol_filter", "mahalanobis_outlier_mask", "PrepView",
           "MSC", "EMSC", "scatter_basis", "scatter_weights", "whittaker_bands", "whittaker", "asls", "AsLS"]


@functools.lru_cache(maxsize=64)
def savgol_taps(window_length: int, polyorder: int, deriv: int = 0, delta: float = 1.0) -> np.ndarray:
    """[interior (w)] ++ [left edge (half × w)] ++ [right edge (half × w)] fp64 taps."""
    w = int(window_length)
    if w % 2 != 1 or w < 1:
        raise ValueError("window_length must be a positive odd integer")
    if polyorder >= w:
        raise ValueError("polyorder must be less than window_length.")
    half = w // 2
    interior = savgol_coeffs(w, polyorder, deriv=deriv, delta=delta, use="dot")
    t = np.arange(w, dtype=np.float64)
    # polynomial fit of each unit vector (columns of I), differentiated, evaluated at the edge points
    coeffs = np.polyfit(t, np.eye(w), polyorder)  # (polyorder+1, w)
    for _ in range(deriv):
        coeffs = (coeffs[:-1] * np.arange(coeffs.shape[0] - 1, 0, -1)[:, None]) if coeffs.shape[0] > 1 \
            else np.zeros((1, w))
    ev_left = np.arange(0, half, dtype=np.float64)
    ev_right = np.arange(w - half, w, dtype=np.float64)
    left = np.stack([np.polyval(coeffs, x) for x in ev_left]) / delta ** deriv if half else np.zeros((0, w))
    right = np.stack([np.polyval(coeffs, x) for x in ev_right]) / delta ** deriv if half else np.zeros((0, w))
    return np.ascontiguousarray(np.concatenate([interior, left.ravel(), right.ravel()]), dtype=np.float64)


def snv_savgol(X, window_length: int | None = None, polyorder: int = 2, deriv: int = 0, delta: float = 1.0,
               snv: bool = True, out: torch.Tensor | None = None, lazy: bool = False):
    """SNV (optional) then Savitzky–Golay (optional: ``window_length=None``)
    along the wavelength axis of a (m, p) float32 matrix in HBM.

    ``lazy=True`` returns a ``PrepView``: nothing is computed here (SNV row
    statistics on first use), and ``utils.SIMCA`` fit / predict / transform,
    the CV engine and the engine entry points apply the transform in their
    load paths, so the preprocessed matrix is never written to HBM.

    ``lazy="write"`` returns a write-through ``PrepView``: the first Gram over
    all its rows (a fit) forms X′ in its quantiser and writes it as a side
    output, and every later consumer reads that X′ (the stencil runs once; X′
    costs its memory, as the eager pass does)."""
    Xd = engine.as_device_f32(X)
    if isinstance(Xd, PrepView):
        Xd = Xd.materialize()
    m, p = Xd.shape
    if window_length is not None and int(window_length) > p:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    if lazy not in (False, True, "write"):
        raise ValueError('snv_savgol: lazy must be False, True or "write"')
    if lazy:
        if out is not None:
            raise ValueError("snv_savgol: `out` and a lazy view exclude each other")
        tp = savgol_taps(int(window_length), int(polyorder), int(deriv), float(delta)) if window_length else None
        return PrepView(Xd, window_length, polyorder, deriv, delta, snv, tp, through=(lazy == "write"))
    if out is None:
        out = torch.empty((m, p), dtype=torch.float32, device=Xd.device)
    w = 0
    taps = None
    if window_length is not None:
        w = int(window_length)
        tp = savgol_taps(w, int(polyorder), int(deriv), float(delta))
        taps = tp.ctypes.data_as(_lib.ctypes.POINTER(_lib.c_f64))
    check(_lib.load().ocm_snv_savgol_f32(Context.get(Xd.device.index).handle, ptr(Xd), Xd.stride(0), m, p,
                                         1 if snv else 0, w, taps, ptr(out), out.stride(0),
                                         engine._stream(Xd.device)), "ocm_snv_savgol_f32")
    return out


def snv(X, out=None) -> torch.Tensor:
    """(x − mean_row) / (std_row + 1e-8)."""
    return snv_savgol(X, None, snv=True, out=out)


def savgol_filter(X, window_length, polyorder, deriv=0, delta=1.0, out=None) -> torch.Tensor:
    """scipy.signal.savgol_filter(X, ..., axis=1, mode='interp') on the GPU."""
    return snv_savgol(X, window_length, polyorder, deriv, delta, snv=False, out=out)


SCATTER_QMAX = 8  # rows of the EMSC basis the kernels take (include/ocm.h)


def scatter_basis(reference, degree: int = 0, wavelengths=None, interferents=None) -> np.ndarray:
    """The (q, p) fp64 basis of MSC / EMSC (include/ocm.h, scatter correction):
    row 0 ones, row 1 the reference spectrum, then λ¹..λ^degree with
    λ = linspace(−1, 1, p) (``wavelengths``, if given, mapped affinely to
    [−1, 1]), then the interferent spectra.  ``degree=0`` without
    interferents is the MSC basis.  A pure host function (no device)."""
    ref = np.asarray(reference, dtype=np.float64)
    if ref.ndim != 1 or ref.size < 1:
        raise ValueError("scatter correction: the reference must be a 1-D spectrum")
    p = ref.size
    if not np.isfinite(ref).all():
        raise ValueError("scatter correction: the reference has non-finite values")
    degree = int(degree)
    if degree < 0:
        raise ValueError("scatter correction: degree must be >= 0")
    inter = np.zeros((0, p)) if interferents is None else np.atleast_2d(np.asarray(interferents, dtype=np.float64))
    if inter.ndim != 2 or inter.shape[1] != p:
        raise ValueError(f"scatter correction: interferents must have {p} columns, like the reference")
    q = 2 + degree + inter.shape[0]
    if q > SCATTER_QMAX:
        raise ValueError(f"scatter correction: the basis has q = {q} rows (ones, reference, {degree} polynomial, "
                         f"{inter.shape[0]} interferent); at most {SCATTER_QMAX} are supported")
    if p < q:
        raise ValueError(f"scatter correction: p = {p} columns cannot determine q = {q} coefficients")
    if np.ptp(ref) == 0.0:
        raise ValueError("scatter correction: the reference spectrum is constant (collinear with the offset term)")
    if wavelengths is None:
        lam = np.linspace(-1.0, 1.0, p)
    else:
        wl = np.asarray(wavelengths, dtype=np.float64)
        if wl.shape != (p,):
            raise ValueError(f"scatter correction: wavelengths must have length {p}, like the reference")
        lo, hi = float(wl.min()), float(wl.max())
        if not (np.isfinite(wl).all() and hi > lo):
            raise ValueError("scatter correction: wavelengths must be finite and not all equal")
        lam = (2.0 * wl - (hi + lo)) / (hi - lo)
    rows = [np.ones(p), ref] + [lam ** d for d in range(1, degree + 1)] + list(inter)
    return np.ascontiguousarray(np.stack(rows), dtype=np.float64)


def scatter_weights(basis) -> np.ndarray:
    """W = pinv(Bᵀ), (q, p) fp64: ``W @ x`` are the least-squares coefficients
    of x on the rows of B (for the MSC basis: ``np.polyfit(ref, x, 1)[::-1]``).
    The rows of B are scaled to unit norm for the pseudo-inverse (the
    reference's level does not enter the conditioning) and the scaling is
    undone on W.  A pure host function (no device)."""
    B = np.asarray(basis, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] < 2 or B.shape[0] > SCATTER_QMAX or B.shape[1] < B.shape[0]:
        raise ValueError(f"scatter correction: the basis must be (q, p) with 2 <= q <= {SCATTER_QMAX} and p >= q")
    norm = np.linalg.norm(B, axis=1)
    if not (np.isfinite(norm).all() and (norm > 0).all()):
        raise ValueError("scatter correction: the basis has a zero or non-finite row")
    Bn = B / norm[:, None]
    if np.linalg.matrix_rank(Bn.T) < B.shape[0]:
        raise ValueError("scatter correction: the basis rows are linearly dependent")
    return np.ascontiguousarray(np.linalg.pinv(Bn.T) / norm[:, None], dtype=np.float64)


def _weights_key(W: np.ndarray) -> int:
    from .replica import _array_hash

    return _array_hash(W)


def _device_rows(X):
    """A float32 device matrix the scatter kernels read in place: a row slice
    of a wider tensor keeps its row stride."""
    if isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and \
            X.stride(1) == 1 and X.stride(0) >= X.shape[1]:
        return X
    Xd = engine.as_device_f32(X)
    return Xd.materialize() if isinstance(Xd, PrepView) else Xd


def _row_statistics(X: torch.Tensor, W_dev: torch.Tensor) -> torch.Tensor:
    """``ocm_rowfit_f32``: the (m, 2) float32 pairs (m_r, s_r) = (c0, 1/c1) of
    the rows of a float32 device matrix against the (q, p) fp64 device weights."""
    m, p = X.shape
    rs = torch.empty((m, 2), dtype=torch.float32, device=X.device)
    check(_lib.load().ocm_rowfit_f32(Context.get(X.device.index).handle, ptr(X), X.stride(0), m, p, ptr(W_dev),
                                     int(W_dev.shape[0]), None, ptr(rs), engine._stream(X.device)), "ocm_rowfit_f32")
    return rs


class EMSC:
    """Extended multiplicative scatter correction against a reference spectrum
    (include/ocm.h, scatter correction): each row x is fitted by least squares
    on the basis ``basis_`` (ones, the reference, λ¹..λ^degree, interferents),
    c = ``weights_`` @ x in fp64 on the GPU, and
    y = (x − c0 − Σ_{t≥2} c_t·B_t) / c1.

    ``fit(X, rows=None)`` takes the reference as the fp64 column mean of the
    training rows unless ``reference=`` was given.  ``transform(X)`` is eager:
    one read and one write of X (``ocm_emsc_apply_f32``); with
    ``window_length=`` it then runs ``savgol_filter`` on the result, a second
    pass over the matrix.  A basis with baseline or interferent rows has no
    lazy view (the correction depends on the column): ``lazy=True`` raises,
    use the eager ``transform(X)``; with only the two MSC rows (``degree=0``,
    no interferents) the weights and every path are those of ``MSC``."""

    def __init__(self, degree: int = 2, reference=None, wavelengths=None, interferents=None):
        self.degree = int(degree)
        self.wavelengths = wavelengths
        self.interferents = interferents
        n_int = 0 if interferents is None else np.atleast_2d(np.asarray(interferents)).shape[0]
        if self.degree < 0:
            raise ValueError("scatter correction: degree must be >= 0")
        if 2 + self.degree + n_int > SCATTER_QMAX:
            raise ValueError(f"scatter correction: the basis would have q = {2 + self.degree + n_int} rows; at most "
                             f"{SCATTER_QMAX} are supported")
        self.reference_ = self.basis_ = self.weights_ = None
        self._dev = {}
        if reference is not None:
            self._set_reference(reference)

    def _set_reference(self, reference):
        B = scatter_basis(reference, self.degree, self.wavelengths, self.interferents)
        W = scatter_weights(B)
        self.reference_ = B[1].copy()
        self.basis_, self.weights_ = B, W
        self._key = _weights_key(W)
        self._dev = {}

    def _on_device(self, device):
        """(W, B) as fp64 device tensors, uploaded once per device."""
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.weights_).to(device), torch.from_numpy(self.basis_).to(device))
        return self._dev[device]

    def fit(self, X, rows=None):
        if self.reference_ is None:
            Xd = _device_rows(X)
            if Xd.stride(0) != Xd.shape[1]:
                Xd = Xd.contiguous()
            if rows is not None:
                rows = torch.as_tensor(rows, device=Xd.device).to(torch.int64)
            n = Xd.shape[0] if rows is None else int(rows.numel())
            self._set_reference(engine.colmean(Xd, rows, n).cpu().numpy())
        return self

    def _check(self, X):
        if self.weights_ is None:
            raise ValueError(f"{type(self).__name__}: call fit(X) first, or pass reference=")
        if len(X.shape) != 2 or X.shape[1] != self.reference_.size:
            raise ValueError(f"{type(self).__name__}: X must be (m, {self.reference_.size}) like the reference, got "
                             f"{tuple(X.shape)}")

    def _eager(self, Xd):
        m, p = Xd.shape
        W, B = self._on_device(Xd.device)
        out = torch.empty((m, p), dtype=torch.float32, device=Xd.device)
        check(_lib.load().ocm_emsc_apply_f32(Context.get(Xd.device.index).handle, ptr(Xd), Xd.stride(0), m, p, ptr(W),
                                             ptr(B), int(W.shape[0]), ptr(out), p, None,
                                             engine._stream(Xd.device)), "ocm_emsc_apply_f32")
        return out

    def _view(self, Xd, window_length, polyorder, deriv, delta, through):
        """The lazy MSC view: the row statistics come from ocm_rowfit_f32 here,
        the consumers apply (x − m_r)·s_r and the filter in their load paths."""
        # the fit reads the rows where they are, as the eager pass does (both then sum in the same order)
        rs = _row_statistics(Xd, self._on_device(Xd.device)[0])
        if Xd.stride(0) != Xd.shape[1]:
            Xd = Xd.contiguous()
        tp =savgol_taps(int(window_length), int(polyorder), int(deriv), float(delta)) if window_length else None
        return PrepView(Xd, window_length, polyorder, deriv, delta, False, tp, through=through, rowstat=rs,
                        kind="msc", stat_key=self._key)

    def transform(self, X, window_length: int | None = None, polyorder: int = 2, deriv: int = 0, delta: float = 1.0,
                  lazy=False):
        """The corrected rows as a float32 device tensor (``lazy=False``), or
        — for a basis of the two MSC rows only — a ``PrepView``
        (``lazy=True`` / ``"write"``, as ``snv_savgol`` returns).  With
        ``window_length`` the Savitzky–Golay filter follows the correction."""
        self._check(X)
        if lazy not in (False, True, "write"):
            raise ValueError(f'{type(self).__name__}.transform: lazy must be False, True or "write"')
        p = self.reference_.size
        if window_length is not None:
            if int(window_length) > p:
                raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
            savgol_taps(int(window_length), int(polyorder), int(deriv), float(delta))  # validates the filter
        q = self.basis_.shape[0]
        if lazy and q > 2:
            raise ValueError(f"{type(self).__name__}.transform: a basis with baseline or interferent rows (q = {q}) "
                             "has no lazy view, its correction depends on the column; use the eager transform(X) "
                             "(lazy=False), or MSC / EMSC(degree=0) for a lazy view")
        Xd = _device_rows(X)
        if lazy:
            return self._view(Xd, window_length, polyorder, deriv, delta, lazy == "write")
        if window_length is None:
            return self._eager(Xd)
        if q == 2:  # one pass: the view's formula, written out
            return self._view(Xd, window_length, polyorder, deriv, delta, False).materialize()
        return savgol_filter(self._eager(Xd), window_length, polyorder, deriv, delta)


class MSC(EMSC):
    """Multiplicative scatter correction: y = (x − a_r) / b_r with
    (b_r, a_r) = ``np.polyfit(reference, x, 1)``, the fit in fp64 on the GPU.

    ``transform(X)`` is one read and one write of X (``ocm_emsc_apply_f32``,
    q = 2); with ``window_length=`` the Savitzky–Golay filter runs in the
    same pass (the materialised view).  ``lazy=True`` returns a ``PrepView``
    the SIMCA fit / predict / transform, the CV engine and the engine entry
    points read in place, as they read an SNV view: only the (m, 2) row
    statistics are computed here (``ocm_rowfit_f32``, one read of X).
    ``lazy="write"`` is the write-through view.  Eager and lazy values are
    bit-identical."""

    def __init__(self, reference=None):
        super().__init__(degree=0, reference=reference)


def whittaker_bands(p: int, d: int = 2) -> np.ndarray:
    """The (d + 1, p) fp64 lower-banded form of DᵀD, D the d-th difference
    matrix ``np.diff(np.eye(p), d, axis=0)``, as
    ``scipy.linalg.solveh_banded(..., lower=True)`` takes it: row k holds the
    k-th sub-diagonal, padded with zeros at the end.  A pure host function."""
    p, d = int(p), int(d)
    if d not in (1, 2):
        raise ValueError("baseline: d must be 1 or 2")
    if p < d + 1:
        raise ValueError(f"baseline: p = {p} columns are too few for differences of order d = {d} (p >= d + 1)")
    j = np.arange(p)
    ab = np.zeros((d + 1, p), dtype=np.float64)
    if d == 1:
        ab[0] = (j >= 1).astype(float) + (j <= p - 2)
        ab[1, :p - 1] = -1.0
    else:
        first, mid, last = j <= p - 3, (j >= 1) & (j <= p - 2), j >= 2  # the rows of D that touch column j
        ab[0] = first + 4.0 * mid + last
        ab[1] = -2.0 * (first.astype(float) + mid)
        ab[2] = first
    return ab


def _baseline_shape(who: str, X, lam, d) -> tuple[int, int]:
    """The checks of λ, d and the shape of X, before any device work."""
    lam, d = float(lam), int(d)
    if not (np.isfinite(lam) and lam > 0.0):
        raise ValueError(f"{who}: lam must be positive and finite, got {lam}")
    if d not in (1, 2):
        raise ValueError(f"{who}: d must be 1 or 2, got {d}")
    shape = tuple(X.shape) if hasattr(X, "shape") else np.asarray(X).shape
    if len(shape) != 2:
        raise ValueError(f"{who}: X must be a (m, p) matrix, got shape {shape}")
    if shape[1] < d + 1:
        raise ValueError(f"{who}: p = {shape[1]} columns are too few for differences of order d = {d} (p >= d + 1)")
    return int(shape[0]), int(shape[1])


def _extent(t: torch.Tensor) -> tuple[int, int]:
    """[first, last) byte of a 2-D tensor's elements."""
    n = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1 if t.numel() else 0
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


def _baseline_out(who: str, out, X, m: int, p: int):
    """``out`` must be a (m, p) float32 device tensor with unit column stride
    that shares no memory with X; checked before any device work."""
    if out is None:
        return
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != (m, p):
        raise ValueError(f"{who}: out must be a ({m}, {p}) tensor, got "
                         f"{tuple(out.shape) if hasattr(out, 'shape') else type(out).__name__}")
    if out.dtype != torch.float32:
        raise ValueError(f"{who}: out must be float32, got {out.dtype}")
    if out.stride(1) != 1 or out.stride(0) < p:
        raise ValueError(f"{who}: out must have unit column stride and a row stride >= p")
    src = X.X if isinstance(X, PrepView) else X
    if isinstance(src, torch.Tensor) and src.device == out.device:
        (a0, a1), (b0, b1) = _extent(src), _extent(out)
        if a0 < b1 and b0 < a1:
            raise ValueError(f"{who}: out overlaps X (the rows are read again after the first are written)")
    if not out.is_cuda or (isinstance(src, torch.Tensor) and src.is_cuda and src.device != out.device):
        raise ValueError(f"{who}: out must be on the device of X, got {out.device}")


def _baseline_weights(weights, m: int, p: int, d: int):
    """None, or the weights as given with their kind ("vector" / "rows").
    Host weights are checked here; device weights are checked by the kernel
    (a bad row is counted and ``whittaker`` raises)."""
    if weights is None:
        return None, None
    on_device = isinstance(weights, torch.Tensor) and weights.is_cuda
    w = weights if on_device else np.asarray(weights.numpy() if isinstance(weights, torch.Tensor) else weights)
    shape = tuple(w.shape)
    if shape not in ((p,), (m, p)):
        raise ValueError(f"whittaker: weights must be None, ({p},) or ({m}, {p}), got shape {shape}")
    kind = "vector" if shape == (p,) else "rows"  # m == 1 and a (p,) vector: the shared path
    if not on_device:
        w = w.astype(np.float64)
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("whittaker: weights must be finite and >= 0")
        if kind == "vector" and int((w > 0).sum()) < d:
            raise ValueError(f"whittaker: fewer than d = {d} positive weights: the system is singular")
    return kind, w


def whittaker(X, lam, d: int = 2, weights=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The Whittaker smooth of every row of a (m, p) float32 matrix
    (include/ocm.h, baseline correction): z solves
    (diag(w) + λ·DᵀD) z = w ∘ x in fp64 on the GPU (``ocm_whittaker_f32``),
    D the d-th difference matrix.  ``weights``: None (w = 1), a (p,) vector
    shared by all rows (both factorise once), or a (m, p) matrix.  Raises
    ``ValueError`` when a row's system is not positive definite (fewer than d
    positive weights, a negative or NaN weight).  Eager only: a row's solve is
    global along the wavelengths, it cannot run inside another kernel's loads,
    so there is no lazy view."""
    m, p = _baseline_shape("whittaker", X, lam, d)
    kind, w = _baseline_weights(weights, m, p, int(d))
    _baseline_out("whittaker", out, X, m, p)
    Xd = _device_rows(X)
    W, ldw = None, 0
    if kind is not None:
        W = (w if isinstance(w, torch.Tensor) else torch.from_numpy(w)).to(device=Xd.device, dtype=torch.float32)
        if kind == "vector":
            W = W.contiguous()
        else:
            if W.stride(1) != 1 or W.stride(0) < p:
                W = W.contiguous()
            ldw = W.stride(0)
    if out is None:
        out = torch.empty((m, p), dtype=torch.float32, device=Xd.device)
    nbad = torch.zeros(1, dtype=torch.int32, device=Xd.device)
    check(_lib.load().ocm_whittaker_f32(Context.get(Xd.device.index).handle, ptr(Xd), Xd.stride(0), m, p, ptr(W), ldw,
                                        float(lam), int(d), ptr(out), out.stride(0), ptr(nbad),
                                        engine._stream(Xd.device)), "ocm_whittaker_f32")
    bad = int(nbad.item())
    if bad:
        raise ValueError(f"whittaker: {bad} of {m} rows have a system that is not positive definite (fewer than "
                         f"d = {int(d)} positive weights, or a negative or NaN weight); they were written as NaN")
    return out


def asls(X, lam: float = 1e5, asym: float = 0.01, n_iter: int = 10, d: int = 2, subtract: bool = True,
         out: torch.Tensor | None = None, return_iters: bool = False):
    """Asymmetric least squares baseline (Eilers & Boelens 2005; include/ocm.h,
    baseline correction) of every row of a (m, p) float32 matrix, all
    iterations of a row in one kernel (``ocm_asls_f32``): start from w = 1,
    smooth (``whittaker``), set w_j = asym where x_j > z_j and 1 − asym
    elsewhere (a tie included), at most ``n_iter`` solves; a row stops when its
    weights no longer change.  Returns the corrected rows x − z
    (``subtract=True``) or the baselines z, float32 on the device, and with
    ``return_iters`` the (m,) int32 number of solves each row ran.  Eager only:
    a row's solve is global along the wavelengths, there is no lazy view."""
    m, p = _baseline_shape("asls", X, lam, d)
    asym = float(asym)
    if not (0.0 < asym < 1.0):
        raise ValueError(f"asls: asym must lie in (0, 1), got {asym}")
    if int(n_iter) < 1:
        raise ValueError(f"asls: n_iter must be >= 1, got {n_iter}")
    _baseline_out("asls", out, X, m, p)
    Xd = _device_rows(X)
    if out is None:
        out = torch.empty((m, p), dtype=torch.float32, device=Xd.device)
    iters = torch.empty(m, dtype=torch.int32, device=Xd.device) if return_iters else None
    check(_lib.load().ocm_asls_f32(Context.get(Xd.device.index).handle, ptr(Xd), Xd.stride(0), m, p, float(lam), asym,
                                   int(d), int(n_iter), 1 if subtract else 0, ptr(out), out.stride(0), ptr(iters),
                                   engine._stream(Xd.device)), "ocm_asls_f32")
    return (out, iters) if return_iters else out


class AsLS:
    """``asls`` as an estimator, in the style of ``MSC`` / ``EMSC``: nothing is
    learned (``fit`` is a no-op), ``transform(X)`` returns the corrected rows
    x − z and ``baseline(X)`` the baselines z; ``iters_`` holds the (m,) int32
    number of solves per row of the last call.  Eager only (no lazy view)."""

    def __init__(self, lam: float = 1e5, asym: float = 0.01, n_iter: int = 10, d: int = 2):
        self.lam, self.asym, self.n_iter, self.d = float(lam), float(asym), int(n_iter), int(d)
        if not (np.isfinite(self.lam) and self.lam > 0.0):
            raise ValueError(f"AsLS: lam must be positive and finite, got {self.lam}")
        if not (0.0 < self.asym < 1.0):
            raise ValueError(f"AsLS: asym must lie in (0, 1), got {self.asym}")
        if self.n_iter < 1:
            raise ValueError(f"AsLS: n_iter must be >= 1, got {self.n_iter}")
        if self.d not in (1, 2):
            raise ValueError(f"AsLS: d must be 1 or 2, got {self.d}")
        self.iters_ = None

    def fit(self, X=None, y=None):
        return self

    def _run(self, X, subtract):
        out, self.iters_ = asls(X, self.lam, self.asym, self.n_iter, self.d, subtract=subtract, return_iters=True)
        return out

    def transform(self, X) -> torch.Tensor:
        return self._run(X, True)

    def baseline(self, X) -> torch.Tensor:
        return self._run(X, False)


def mahalanobis_outlier_mask(X, n_components: int, percentile: float = 95.0, rows=None):
    """PCA-score Mahalanobis outlier screen of the drivers (simca_nuts.py:126-147,
    utils/data_utils.py:64-80): scores T of a PCA(n_components) fit, md_i =
    √((t_i − t̄)ᵀ pinv(cov T) (t_i − t̄)), keep md ≤ percentile(md, 95).

    On the engine: the Gram / eigensolver / scoring kernels give T² with
    pinv(cov T) = diag(1/λ) (exact PCA scores are centred and uncorrelated),
    md = √T², and the percentile is the device radix select on md (NumPy's
    linear interpolation in md).  Returns (keep mask bool (n,), threshold)."""
    import torch

    Xd = engine.as_device_f32(X)
    n = Xd.shape[0] if rows is None else int(rows.numel())
    fit = engine.fit_class(Xd, rows, n, int(n_components), theta_mode=0, want_T=False)
    md = torch.sqrt(fit.T2)
    thr = engine.percentile(md, float(percentile))
    return md <= thr, thr
