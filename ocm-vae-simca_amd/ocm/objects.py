"""Objects: runs of adjacent rows of a spectra matrix (the pixels of one nut,
nut_data.py:131-185), described by G + 1 row offsets, and their sums and
means on the device (ocm_segsum_f32 / _f64, include/ocm.h "object-level
sums") in place of host loops over ``obj_ids == idx``
(utils/data_utils.py:79-82).

``segment_offsets``, ``check_offsets`` and ``stack_objects`` are host NumPy and
need no device.  ``segment_sums`` and ``object_means`` follow the estimator's
rule: NumPy in, NumPy out; tensor (or lazy view) in, device tensor out."""
from __future__ import annotations

import numpy as np

__all__ = ["segment_offsets", "check_offsets", "stack_objects", "segment_sums", "object_means"]


def _host(a):
    if hasattr(a, "detach"):  # a torch tensor, without importing torch here
        return a.detach().cpu().numpy()
    return np.asarray(a)


def segment_offsets(ids) -> np.ndarray:
    """Row offsets (G + 1,) int64 of the objects of ``ids`` (m object ids, one
    per row): every run of equal ids is an object, in order of appearance, and
    object g is rows [offsets[g], offsets[g + 1]).  The rows of an object must
    be adjacent: an id that returns after another run raises ValueError.  A
    0-length input gives [0]."""
    ids = _host(ids)
    if ids.ndim != 1:
        raise ValueError(f"segment_offsets: ids has shape {ids.shape}, expected (m,)")
    m = ids.shape[0]
    if m == 0:
        return np.zeros(1, dtype=np.int64)
    starts = np.concatenate([[0], np.flatnonzero(ids[1:] != ids[:-1]) + 1]).astype(np.int64)
    if np.unique(ids[starts]).size != starts.size:
        raise ValueError("segment_offsets: an object id returns after another object's rows; the rows of an "
                         "object must be adjacent (sort the rows by object first)")
    return np.concatenate([starts, [m]]).astype(np.int64)


def check_offsets(offsets, m: int) -> np.ndarray:
    """``offsets`` as a validated (G + 1,) int64 array for a matrix of m rows:
    integers, non-decreasing, 0 ≤ offsets[0], offsets[G] ≤ m.  ValueError
    otherwise (the device kernels do not check them)."""
    off = _host(offsets)
    if off.ndim != 1 or off.size < 1:
        raise ValueError(f"offsets: expected a 1-D array of G + 1 >= 1 row offsets, got shape {off.shape}")
    if not (np.issubdtype(off.dtype, np.integer) and off.dtype != np.bool_):
        raise ValueError(f"offsets: must hold integers, got dtype {off.dtype}")
    if off.dtype == np.uint64 and off.max() > np.iinfo(np.int64).max:
        raise ValueError("offsets: out of range")
    off = off.astype(np.int64)
    if off[0] < 0:
        raise ValueError(f"offsets: offsets[0] = {int(off[0])} is negative")
    if (np.diff(off) < 0).any():
        g = int(np.flatnonzero(np.diff(off) < 0)[0])
        raise ValueError(f"offsets: decreasing at {g} ({int(off[g])} then {int(off[g + 1])})")
    if off[-1] > m:
        raise ValueError(f"offsets: offsets[-1] = {int(off[-1])} is out of range for {int(m)} rows")
    return np.ascontiguousarray(off)


def stack_objects(objs):
    """(X, offsets) of a list of objects, each an (n_g, p) array or a dict with
    a ``'spectral_data'`` entry (what ``utils.data_utils.load_nut_objects_h5``
    returns per nut): the rows stacked in order and the (G + 1,) int64 offsets."""
    blocks = [np.asarray(o["spectral_data"] if isinstance(o, dict) else o) for o in objs]
    if not blocks:
        raise ValueError("stack_objects: no objects")
    for b in blocks:
        if b.ndim != 2 or b.shape[1] != blocks[0].shape[1]:
            raise ValueError(f"stack_objects: objects must be (n, p) arrays of one width, got {b.shape} beside "
                             f"{blocks[0].shape}")
    offsets = np.zeros(len(blocks) + 1, dtype=np.int64)
    np.cumsum([b.shape[0] for b in blocks], out=offsets[1:])
    return np.vstack(blocks), offsets


def _is_dev(X) -> bool:
    return not isinstance(X, np.ndarray) and hasattr(X, "device")


def segment_sums(X, offsets):
    """(G, p) float64 column sums of the rows of each object (fp64
    accumulation, the same bits on every call).  An empty object gives zeros.
    A lazy view is materialised first (``ocm.engine.segment_sums``)."""
    from . import engine

    dev_in = _is_dev(X)
    out = engine.segment_sums(engine.as_device_x(X), offsets)
    return out if dev_in else out.cpu().numpy()


def object_means(X, offsets):
    """(G, p) mean spectrum of each object: sum / count in fp64, rounded once to
    X's dtype (float64 stays float64, anything else is float32).  An empty
    object raises ValueError."""
    import torch

    from . import engine

    dev_in = _is_dev(X)
    off = check_offsets(offsets, int(X.shape[0]))
    counts = np.diff(off)
    if (counts == 0).any():
        raise ValueError(f"object_means: object {int(np.flatnonzero(counts == 0)[0])} is empty")
    Xd = engine.as_device_x(X)
    sums = engine.segment_sums(Xd, off, checked=True)
    n = torch.from_numpy(counts.astype(np.float64)).to(sums.device)
    mean = (sums / n[:, None]).to(torch.float64 if Xd.dtype == torch.float64 else torch.float32)
    return mean if dev_in else mean.cpu().numpy()
