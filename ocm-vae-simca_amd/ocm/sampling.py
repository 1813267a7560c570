"""Choosing the calibration rows on the device: Kennard–Stone and Duplex
(csrc/ocm_kstone.hip).

The reference splits its rows at random (``train_test_split``,
simca_nuts.py:73-74; the object-level 70/15/15 split of utils/data_utils.py).
A one-class model's T²/Q limits describe only the region its calibration rows
cover, so the DD-SIMCA literature builds the calibration set with
**Kennard–Stone**: start from the two most distant rows (or from the row
nearest the mean), then keep adding the row whose distance to the nearest
selected row is largest.  **Duplex** (Snee) builds two such sets in turns, for a
test set as representative as the calibration set.

Definitions (the kernels follow them exactly, the tests compare bit for bit
with a NumPy transcription):

    d2(i, j) = Σ_c w_c (z_ic − z_jc)²          fp64, the difference form
    pair     (i*, j*) = argmax d2 over i < j, ties to the smallest i, then j
    mean     i* = argmin_i Σ_c w_c (z_ic − mean_c)², ties to the smallest i
    step     m_i = min over selected s of d2(i, s); next = argmax m_i over the
             unselected rows, ties to the smallest i; d2[t] = that m

Z is X as it stands (``n_components=None``) or the scores T of a PCA(k) of the
candidate rows (``engine.fit_class``); ``metric="mahalanobis"`` weights the
score columns by 1/λ inside the kernels, no scaled copy of T is written.

Everything is queued on the current stream and read back once, at the end; a
row with a non-finite coordinate raises ``ValueError`` with the count.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

__all__ = ["Selection", "kennard_stone", "duplex", "kennard_stone_split", "kennard_stone_objects"]

_BAD_START = 1 << 30  # csrc/ocm_kstone.hip KS_BAD_START


@dataclass
class Selection:
    """``order`` (n_select,) int64: indices into X in pick order; ``d2``
    (n_select,) float64: the squared min distance each pick had when it was
    taken (the pair's distance for both rows of a pair start, NaN for explicit
    starts).  ``scores`` / ``weights``: the device tensors Z = T and w the
    distances were taken on when a PCA was fitted (else None)."""
    order: np.ndarray
    d2: np.ndarray
    scores: object = None
    weights: object = None

    @property
    def distance(self) -> np.ndarray:
        return np.sqrt(self.d2)

    def mask(self, n: int) -> np.ndarray:
        """(n,) bool, True at the selected indices."""
        m = np.zeros(int(n), dtype=bool)
        m[self.order] = True
        return m

    def rest(self, n: int) -> np.ndarray:
        """The unselected indices of range(n), ascending."""
        return np.flatnonzero(~self.mask(n)).astype(np.int64)


# ------------------------------------------------------------------ argument checks (no device)

def _shape(X):
    sh = tuple(X.shape)
    if len(sh) != 2 or sh[0] < 1 or sh[1] < 1:
        raise ValueError(f"X must be a non-empty 2-D matrix, got shape {sh}")
    return sh


def _rows_host(rows, n_x):
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
    if np.unique(r).size != r.size:
        raise ValueError("rows: duplicate indices")
    return r


def _check_common(X, metric, n_components, rows):
    n_x, p = X if isinstance(X, tuple) else _shape(X)
    if metric not in ("euclidean", "mahalanobis"):
        raise ValueError(f"metric={metric!r}: expected 'euclidean' or 'mahalanobis'")
    if metric == "mahalanobis" and n_components is None:
        raise ValueError("metric='mahalanobis' needs n_components (the distance is taken on PCA scores)")
    rh = _rows_host(rows, n_x)
    n = n_x if rh is None else int(rh.size)
    if n_components is not None:
        k = int(n_components)
        if not (1 <= k <= p):
            raise ValueError(f"n_components={n_components} must be in [1, {p}]")
        if n < 2:
            raise ValueError("a PCA needs at least 2 candidate rows")
    return n, rh


def _check_start(start, n_x, rh):
    """Explicit start indices (into X) as positions among the candidates."""
    s = np.asarray(start)
    if s.ndim != 1 or s.size < 1 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError("start: expected at least one integer index")
    s = s.astype(np.int64)
    if s.min() < 0 or s.max() >= n_x:
        raise ValueError(f"start: indices must lie in [0, {n_x})")
    if np.unique(s).size != s.size:
        raise ValueError("start: duplicate indices")
    if rh is None:
        return s
    sorter = np.argsort(rh, kind="stable")
    loc = np.minimum(np.searchsorted(rh, s, sorter=sorter), rh.size - 1)
    if (rh[sorter[loc]] != s).any():
        raise ValueError("start: every start index must be one of rows")
    return sorter[loc].astype(np.int64)


def _check_ks(shape, n_select, metric="euclidean", n_components=None, init="pair", start=None, rows=None, _path=0):
    """kennard_stone's argument checks for an X of ``shape``: (n candidates, rows
    on the host or None, start positions or None, initial count, n_select)."""
    n, rh = _check_common(shape, metric, n_components, rows)
    if start is not None:
        sh = _check_start(start, shape[0], rh)
        n0 = int(sh.size)
    else:
        if init not in ("pair", "mean"):
            raise ValueError(f"init={init!r}: expected 'pair' or 'mean'")
        sh, n0 = None, (2 if init == "pair" else 1)
    if n0 > n:
        raise ValueError(f"init='pair' needs at least 2 candidate rows, there are {n}")
    return n, rh, sh, n0, _check_count("n_select", n_select, n0, n)


def _check_count(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name}={v!r} must be an integer")
    if not (lo <= int(v) <= hi):
        raise ValueError(f"{name}={int(v)} must be in [{lo}, {hi}]")
    return int(v)


# ------------------------------------------------------------------ device side

def _coordinates(X, rh, n, metric, n_components):
    """(Z, w) on the device: the candidate rows' coordinates and column weights."""
    import torch

    from . import engine
    from .image import gather_rows

    Xd = engine.as_device_x(X)
    rows = None if rh is None else torch.from_numpy(rh).to(Xd.device)
    if n_components is None:
        return (Xd if rows is None else gather_rows(Xd, rows)), None, False
    fit = engine.fit_class(Xd, rows, n, int(n_components), theta_mode=0, want_T=True)
    return fit.T, (fit.inv_diag if metric == "mahalanobis" else None), True


def _raise_bad(nbad: int):
    """nbad: the largest of the kernels' counters (bad rows, + 2^30 for a bad start)."""
    rows = nbad % _BAD_START
    if rows > 0:
        raise ValueError(f"{rows} candidate row(s) hold a non-finite coordinate (NaN or inf)")
    if nbad >= _BAD_START:
        raise ValueError("a start index is out of range")


def kennard_stone(X, n_select, *, metric="euclidean", n_components=None, init="pair", start=None, rows=None,
                  _path=0) -> Selection:
    """Kennard–Stone selection of ``n_select`` rows of X (host or device, float32
    or float64).  ``init``: "pair" starts from the two most distant rows, "mean"
    from the row nearest the column mean; ``start=[…]`` gives explicit first
    indices instead.  ``rows``: restrict the candidates (indices or a mask);
    ``start`` and ``order`` index X either way.
    ``n_components=k``: distances on the scores of a PCA(k) of the candidates,
    ``metric="mahalanobis"`` weighting them by 1/λ."""
    import torch

    from . import engine

    n, rh, sh, n0, n_select = _check_ks(_shape(X), n_select, metric, n_components, init, start, rows)

    Z, w, pca = _coordinates(X, rh, n, metric, n_components)
    dev = Z.device
    bad = []
    head = None
    if sh is not None:
        st = torch.from_numpy(sh).to(dev)
    elif init == "pair":
        st, head, nb = engine.ks_pair(Z, w)
        bad.append(nb)
    else:
        st, head, nb = engine.ks_nearest(Z, engine.colmean(Z, None, n), w)
        bad.append(nb)
    res = engine.ks_select(Z, st, n_select, w=w, path=_path)
    bad.append(res["nbad"])
    nbad = int(torch.stack([b.reshape(()) for b in bad]).max().item())  # the one wait of the selection
    _raise_bad(nbad)
    d2 = res["d2_a"]
    if head is not None:
        d2[:n0] = head
    order = res["order_a"].cpu().numpy()
    if rh is not None:
        order = rh[order]
    return Selection(order, d2.cpu().numpy(), Z if pca else None, w if pca else None)


def duplex(X, n_a, n_b=None, *, metric="euclidean", n_components=None, rows=None, _path=0):
    """Duplex (Snee): two sets built in turns.  A takes the farthest pair of all
    candidates, B the farthest pair of the rest, then A, B, A, … each add the
    unassigned row farthest from the set's own members until both are full (a
    full set is skipped).  ``n_b`` defaults to the remaining rows.  Returns
    ``(Selection A, Selection B)``."""
    import torch

    from . import engine

    n, rh = _check_common(X, metric, n_components, rows)
    if n < 4:
        raise ValueError(f"duplex needs at least 4 candidate rows, there are {n}")
    n_a = _check_count("n_a", n_a, 2, n - 2)
    n_b = n - n_a if n_b is None else _check_count("n_b", n_b, 2, n - n_a)

    Z, w, pca = _coordinates(X, rh, n, metric, n_components)
    dev = Z.device
    pa, da, bad_a = engine.ks_pair(Z, w)
    skip = torch.zeros(n, dtype=torch.uint8, device=dev)
    skip.index_fill_(0, pa.clamp(0, n - 1), 1)
    pb, db, bad_b = engine.ks_pair(Z, w, skip=skip)
    res = engine.ks_select(Z, pa, n_a, pb, n_b, w=w, path=_path)
    _raise_bad(int(torch.stack([bad_a[0], bad_b[0], res["nbad"][0]]).max().item()))
    out = []
    for key, head in (("a", da), ("b", db)):
        d2 = res["d2_" + key]
        d2[:2] = head
        order = res["order_" + key].cpu().numpy()
        out.append(Selection(order if rh is None else rh[order], d2.cpu().numpy(), Z if pca else None,
                             w if pca else None))
    return out[0], out[1]


def _size(name, v, n):
    """An int count, or a float fraction in (0, 1) of n (rounded down)."""
    if isinstance(v, (float, np.floating)):
        if not (0.0 < float(v) < 1.0):
            raise ValueError(f"{name}={v!r}: a fraction must lie in (0, 1)")
        return int(np.floor(float(v) * n))
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name}={v!r} must be an int or a float in (0, 1)")
    return int(v)


def split_sizes(n: int, train_size, test_size=None, method="ks"):
    """(n_train, n_test) of ``kennard_stone_split`` for n candidate rows."""
    if method not in ("ks", "duplex"):
        raise ValueError(f"method={method!r}: expected 'ks' or 'duplex'")
    n_train = _size("train_size", train_size, n)
    if method == "ks":
        if test_size is not None:
            raise ValueError("method='ks' takes the rest as the test set: test_size must be None")
        n_test = n - n_train
    else:
        n_test = n - n_train if test_size is None else _size("test_size", test_size, n)
    if n_train < 1 or n_test < 0 or n_train + n_test > n:
        raise ValueError(f"train_size={train_size!r}, test_size={test_size!r} give ({n_train}, {n_test}) of {n} rows")
    return n_train, n_test


def kennard_stone_split(X, train_size, method="ks", test_size=None, **kw):
    """``(train_idx, test_idx)`` in place of ``train_test_split``.  ``train_size``:
    an int, or a float in (0, 1) (rounded down).  method "ks": the training rows in
    pick order, the test set the rest, ascending.  method "duplex": both sets in
    pick order, ``test_size`` defaulting to the rest.  Other arguments as
    ``kennard_stone`` / ``duplex``."""
    n_x, _ = _shape(X)
    rh = _rows_host(kw.get("rows"), n_x)
    n = n_x if rh is None else int(rh.size)
    n_train, n_test = split_sizes(n, train_size, test_size, method)
    if method == "ks":
        sel = kennard_stone(X, n_train, **kw)
        cand = np.arange(n_x, dtype=np.int64) if rh is None else np.sort(rh)
        return sel.order, cand[~np.isin(cand, sel.order)]
    a, b = duplex(X, n_train, n_test, **kw)
    return a.order, b.order


def kennard_stone_objects(X, n_select, *, objects=None, offsets=None, **kw):
    """Kennard–Stone on the objects' mean spectra, so that whole objects go to one
    side (the object-aware split of utils/data_utils.py).  ``objects``: one id per
    row (runs of equal ids, ``ocm.objects.segment_offsets``) or ``offsets``: G + 1 row
    offsets.  Returns ``(Selection over object numbers, row_mask)``, ``row_mask``
    (rows of X,) bool: the rows of the selected objects."""
    from .objects import check_offsets, object_means, segment_offsets

    n_x, _ = _shape(X)
    if (objects is None) == (offsets is None):
        raise ValueError("kennard_stone_objects: give exactly one of objects= and offsets=")
    off = segment_offsets(objects) if offsets is None else check_offsets(offsets, n_x)
    if off.size < 2:
        raise ValueError("kennard_stone_objects: no objects")
    if objects is not None and off[-1] != n_x:
        raise ValueError(f"objects has {int(off[-1])} ids, X has {n_x} rows")
    _check_ks((int(off.size) - 1, _shape(X)[1]), n_select, **kw)
    sel = kennard_stone(object_means(X, off), n_select, **kw)
    row_mask = np.zeros(n_x, dtype=bool)
    for g in sel.order:
        row_mask[off[g]:off[g + 1]] = True
    return sel, row_mask
