"""Images into objects: the foreground mask of an (H, W, p) hyperspectral
cube, its connected components and the pixel rows of every component, on the
device (ocm_fgmask_f32 / _f64, ocm_label_u8, ocm_gather_rows_f32 / _f64;
include/ocm.h "images into objects") in place of nut_data.py:64-70
(``~(mean < thr)`` and ``scipy.ndimage.label``) and :131-144 (one
``hsi_image[labeled_array == obj]`` per object on the host).

``extract_objects`` gives what ``SIMCA.predict_objects`` takes::

    objs = extract_objects(cube)
    res = model.predict_objects(objs.X, offsets=objs.offsets, rule="vote")
    decided = objs.paint_objects(res.pred[:, 0])

Mask morphology (ocm_edt_u8; include/ocm.h "mask morphology") rests on the
exact squared Euclidean distance transform d² of a mask: ``erode`` by the disc
``disk(r)`` is d² > ⌊r²⌋, ``dilate`` the same on the complement, ``opening``
and ``closing`` two of these, ``distance_transform`` the depth √d² itself, all
equal to their scipy.ndimage counterparts bit for bit.  ``extract_objects(...,
erode=2, fill_holes=True)`` drops the mixed rim of every object before its
spectra are read and returns the depth of every kept pixel.

``objects_from_labels`` is host NumPy and needs no device.  The rest follows
the estimator's rule: NumPy in, NumPy out; tensor in, device tensor out."""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass

import numpy as np

__all__ = ["foreground_mask", "label", "objects_from_labels", "extract_objects", "gather_rows", "ObjectTable",
           "LabelObjects", "disk", "distance_transform", "erode", "dilate", "opening", "closing", "fill_holes"]

LabelObjects = namedtuple("LabelObjects", "order offsets n_pixels centroid bbox labels")


def _is_dev(a) -> bool:
    return not isinstance(a, np.ndarray) and hasattr(a, "device")


def _check_connectivity(connectivity):
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _check_cube(cube):
    if not hasattr(cube, "shape"):
        cube = np.asarray(cube)
    if len(cube.shape) != 3:
        raise ValueError(f"cube must be (H, W, p), got shape {tuple(cube.shape)}")
    H, W, p = (int(s) for s in cube.shape)
    if H < 1 or W < 1 or p < 1:
        raise ValueError(f"cube must have at least one pixel and one band, got shape {(H, W, p)}")
    return cube, H, W, p


def _check_mask(mask, shape=None):
    if not hasattr(mask, "shape"):
        mask = np.asarray(mask)
    if len(mask.shape) != 2:
        raise ValueError(f"mask must be (H, W), got shape {tuple(mask.shape)}")
    if shape is not None and tuple(mask.shape) != tuple(shape):
        raise ValueError(f"mask has shape {tuple(mask.shape)}, the cube's pixels are {tuple(shape)}")
    if mask.shape[0] < 1 or mask.shape[1] < 1:
        raise ValueError(f"mask must have at least one pixel, got shape {tuple(mask.shape)}")
    return mask


EDT_BORDER_BG, EDT_INVERT_IN, EDT_INVERT_OUT = 1, 2, 4  # include/ocm.h OCM_EDT_*
EDT_NONE = 2**31 - 1  # d² without any background pixel
EDT_MAX_SIDE = 32767  # H² + W² stays below 2³¹


def _check_radius(radius, what="radius") -> int:
    """⌊radius²⌋ of a real radius ≥ 0: the r2 that d² is compared with."""
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a real number >= 0, got {radius!r}") from None
    if not (r >= 0.0) or r == float("inf"):  # NaN fails the comparison
        raise ValueError(f"{what} must be a finite real number >= 0, got {radius!r}")
    return int(np.floor(r * r))


def _check_border(border) -> int:
    if border not in ("ignore", "background"):
        raise ValueError(f"border must be 'ignore' or 'background', got {border!r}")
    return EDT_BORDER_BG if border == "background" else 0


def _check_edt_shape(H, W, what):
    if H > EDT_MAX_SIDE or W > EDT_MAX_SIDE:
        raise ValueError(f"{what}: {H} x {W} exceeds {EDT_MAX_SIDE} pixels a side")


# ---------------------------------------------------------------- host
def objects_from_labels(labels, min_pixels: int = 1) -> LabelObjects:
    """The objects of an (H, W) integer label image from any source (0:
    background), on the host.  Labels with fewer than ``min_pixels`` pixels are
    dropped and the others renumbered 1..G in ascending order.  Returns

    ``order``     int64 linear indices of the kept foreground pixels, object
                  after object, raster order inside an object: the row order
                  of ``hsi_image[labeled_array == obj]`` for obj = 1, 2, …;
    ``offsets``   (G + 1,) int64 into ``order``;
    ``n_pixels``  (G,) int64;
    ``centroid``  (G, 2) float64, ``np.argwhere(labels == g).mean(axis=0)``;
    ``bbox``      (G, 4) int64 r0, r1, c0, c1: ``ndimage.find_objects``' slices;
    ``labels``    the relabelled (H, W) int32 image."""
    lab = _host(labels)
    if lab.ndim != 2:
        raise ValueError(f"labels must be (H, W), got shape {lab.shape}")
    if not (np.issubdtype(lab.dtype, np.integer) or lab.dtype == np.bool_):
        raise ValueError(f"labels must hold integers, got dtype {lab.dtype}")
    if lab.size and lab.min() < 0:
        raise ValueError("labels must be non-negative")
    H, W = lab.shape
    flat = lab.ravel().astype(np.int64)
    counts = np.bincount(flat)[1:] if flat.size else np.zeros(0, dtype=np.int64)
    keep = counts >= max(int(min_pixels), 1)
    G = int(keep.sum())
    remap = np.zeros(counts.size + 1, dtype=np.int32)
    remap[1:][keep] = np.arange(1, G + 1, dtype=np.int32)
    new = remap[flat]
    idx = np.flatnonzero(new)
    order = idx[np.argsort(new[idx], kind="stable")].astype(np.int64)
    n_pixels = counts[keep].astype(np.int64)
    offsets = np.zeros(G + 1, dtype=np.int64)
    np.cumsum(n_pixels, out=offsets[1:])
    centroid = np.zeros((G, 2), dtype=np.float64)
    bbox = np.zeros((G, 4), dtype=np.int64)
    if G:
        rows, cols = order // W, order % W
        first = offsets[:-1]
        centroid[:, 0] = np.add.reduceat(rows, first) / n_pixels
        centroid[:, 1] = np.add.reduceat(cols, first) / n_pixels
        bbox[:, 0] = np.minimum.reduceat(rows, first)
        bbox[:, 1] = np.maximum.reduceat(rows, first) + 1
        bbox[:, 2] = np.minimum.reduceat(cols, first)
        bbox[:, 3] = np.maximum.reduceat(cols, first) + 1
    return LabelObjects(order, offsets, n_pixels, centroid, bbox, new.reshape(H, W).astype(np.int32))


def _host(a):
    if hasattr(a, "detach"):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def disk(radius):
    """The bool (2⌊r⌋ + 1)² structuring element ``dx² + dy² ≤ ⌊r²⌋`` (host
    NumPy): the disc that ``erode``, ``dilate``, ``opening`` and ``closing``
    mean by ``radius``, for scipy.ndimage's ``structure=``."""
    r2 = _check_radius(radius)
    k = int(np.floor(float(radius)))
    d = np.arange(-k, k + 1)
    return d[:, None] ** 2 + d[None, :] ** 2 <= r2


# ---------------------------------------------------------------- device
def _call(name, *args):
    from . import _lib

    _lib.check(getattr(_lib.load(), name)(*args), name)


def _pixel_rows(cube, H, W, p):
    """The cube as (H·W, p) pixel rows in HBM, float32 or float64, and their row
    stride: a band slice of a wider contiguous cube is read in place."""
    import torch

    from . import engine

    if isinstance(cube, torch.Tensor) and cube.is_cuda and cube.dtype in (torch.float32, torch.float64):
        s0, s1, s2 = cube.stride()
        if (p == 1 or s2 == 1) and s1 >= p and (H == 1 or s0 == W * s1):
            return cube.as_strided((H * W, p), (s1, 1)), s1
    X = engine.as_device_x(cube.reshape(H * W, p))
    return X, p


def _fgmask_dev(X, ldx, threshold, want_mean=False):
    import torch

    from ._lib import Context, ptr, stream_handle

    m, p = X.shape
    mask = torch.empty(m, dtype=torch.uint8, device=X.device)
    mean = torch.empty(m, dtype=torch.float64, device=X.device) if want_mean else None
    fn = "ocm_fgmask_f64" if X.dtype == torch.float64 else "ocm_fgmask_f32"
    _call(fn, Context.get(X.device.index).handle, ptr(X), ldx, m, p, float(threshold), ptr(mask), ptr(mean),
          stream_handle(X.device))
    return mask, mean


def _label_dev(mask_u8, H, W, connectivity):
    """(labels (H·W,) int32, n (1,) int32) device tensors of a (H·W,) uint8 device mask."""
    import torch

    from ._lib import Context, ptr, stream_handle

    dev = mask_u8.device
    labels = torch.empty(H * W, dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    _call("ocm_label_u8", Context.get(dev.index).handle, ptr(mask_u8), H, W, connectivity, ptr(labels), ptr(n),
          stream_handle(dev))
    return labels, n


def _mask_u8(mask, device=None):
    import torch

    from . import engine

    engine.require_device()
    t = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(_host(mask)))
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return (t.to(device) != 0).to(torch.uint8).contiguous().view(-1)


def _edt_dev(mask_u8, H, W, flags, r2=0, want_d2=False, want_mask=False):
    """One ocm_edt_u8 call on a (H·W,) uint8 device mask: (d2 int32 or None, mask_out uint8 or None)."""
    import torch

    from ._lib import Context, ptr, stream_handle

    dev = mask_u8.device
    d2 = torch.empty(H * W, dtype=torch.int32, device=dev) if want_d2 else None
    out = torch.empty(H * W, dtype=torch.uint8, device=dev) if want_mask else None
    _call("ocm_edt_u8", Context.get(dev.index).handle, ptr(mask_u8), H, W, flags, r2, ptr(d2), ptr(out),
          stream_handle(dev))
    return d2, out


def _morph(mask, steps, what):
    """``steps``: (flags, r2) per ocm_edt_u8 call, each on the mask the one before wrote."""
    mask = _check_mask(mask)
    H, W = (int(s) for s in mask.shape)
    _check_edt_shape(H, W, what)
    dev_in = _is_dev(mask)
    m8 = _mask_u8(mask)
    for flags, r2 in steps:
        if r2 > 0:  # radius 0: the mask itself
            m8 = _edt_dev(m8, H, W, flags, r2, want_mask=True)[1]
    out = m8.view(H, W).bool()
    return out if dev_in else out.cpu().numpy()


def distance_transform(mask, border: str = "ignore", squared: bool = False):
    """The exact Euclidean distance of every foreground pixel (non-zero) of an
    (H, W) mask to the nearest background pixel, 0 on background (ocm_edt_u8).
    ``border="ignore"``: only the image's own pixels count, which is
    ``scipy.ndimage.distance_transform_edt(mask)`` whenever the mask has a
    background pixel; ``"background"``: the pixels just outside the image are
    background too (``distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1]``).
    ``squared=True`` gives the int32 d² (``EDT_NONE`` = 2³¹ − 1 where there is no
    background at all), else float64 √d² with ``inf`` there."""
    flags = _check_border(border)
    mask = _check_mask(mask)
    H, W = (int(s) for s in mask.shape)
    _check_edt_shape(H, W, "distance_transform")
    dev_in = _is_dev(mask)
    d2 = _edt_dev(_mask_u8(mask), H, W, flags, want_d2=True)[0].view(H, W)
    out = d2 if squared else _depth(d2)
    return out if dev_in else out.cpu().numpy()


def _depth(d2):
    import torch

    return torch.where(d2 == EDT_NONE, torch.full((), float("inf"), dtype=torch.float64, device=d2.device),
                       d2.double().sqrt())


def erode(mask, radius, border: str = "background"):
    """(H, W) bool erosion of a mask by ``disk(radius)``: d² > ⌊radius²⌋, one
    ocm_edt_u8 call.  ``border="background"`` is ``scipy.ndimage.binary_erosion(
    mask, disk(radius), border_value=0)``, ``"ignore"`` its ``border_value=1``."""
    return _morph(mask, [(_check_border(border), _check_radius(radius))], "erode")


def dilate(mask, radius):
    """(H, W) bool dilation by ``disk(radius)``, the erosion of the complement:
    ``scipy.ndimage.binary_dilation(mask, disk(radius))``."""
    return _morph(mask, [(EDT_INVERT_IN | EDT_INVERT_OUT, _check_radius(radius))], "dilate")


def opening(mask, radius):
    """Erosion (border "background"), then dilation, two ocm_edt_u8 calls with
    nothing between them: ``scipy.ndimage.binary_opening(mask, disk(radius))``."""
    r2 = _check_radius(radius)
    return _morph(mask, [(EDT_BORDER_BG, r2), (EDT_INVERT_IN | EDT_INVERT_OUT, r2)], "opening")


def closing(mask, radius):
    """Dilation, then erosion with border "ignore", so that the image edge does
    not eat the result: ``binary_erosion(binary_dilation(mask, disc), disc,
    border_value=1)`` with ``disc = disk(radius)``.  (``scipy.ndimage.
    binary_closing`` erodes with border_value=0 and so clears the pixels within
    ``radius`` of the edge.)"""
    r2 = _check_radius(radius)
    return _morph(mask, [(EDT_INVERT_IN | EDT_INVERT_OUT, r2), (0, r2)], "closing")


def _fill_holes_dev(m8, H, W):
    """(H·W,) uint8: the mask and its holes, the 4-connected components of the
    complement whose label appears on no image edge."""
    import torch

    lab = _label_dev((m8 == 0).to(torch.uint8), H, W, 4)[0].view(H, W).long()
    open_ = torch.zeros(H * W + 1, dtype=torch.bool, device=m8.device)  # labels ≤ H·W, whatever the image holds
    open_[torch.cat([lab[0], lab[-1], lab[:, 0], lab[:, -1]])] = True
    open_[0] = True  # label 0: the mask itself
    return (m8.view(H, W).bool() | ~open_[lab]).to(torch.uint8).view(-1)


def fill_holes(mask):
    """(H, W) bool mask with its holes filled: ``scipy.ndimage.binary_fill_holes
    (mask)``.  A hole is a 4-connected component of the complement that touches
    no image edge (ocm_label_u8 on the complement)."""
    mask = _check_mask(mask)
    H, W = (int(s) for s in mask.shape)
    if H * W > 2**31 - 1:
        raise ValueError(f"fill_holes: {H} x {W} pixels exceed 2^31 - 1")
    dev_in = _is_dev(mask)
    out = _fill_holes_dev(_mask_u8(mask), H, W).view(H, W).bool()
    return out if dev_in else out.cpu().numpy()


def foreground_mask(cube, threshold: float = 1e-6, return_mean: bool = False):
    """(H, W) bool mask ``~(cube.mean(axis=2) < threshold)`` of an (H, W, p)
    cube (nut_data.py:64-66) in one read of the cube; a NaN pixel is foreground,
    as in NumPy.  The band mean is the fp64 sum over p (ocm_fgmask_f32 / _f64),
    where the reference averages in the cube's dtype: the two can differ for a
    pixel whose mean lies within rounding of the threshold.  With
    ``return_mean`` also the (H, W) float64 band means."""
    cube, H, W, p = _check_cube(cube)
    dev_in = _is_dev(cube)
    X, ldx = _pixel_rows(cube, H, W, p)
    mask, mean = _fgmask_dev(X, ldx, threshold, want_mean=return_mean)
    mask = mask.view(H, W).bool()
    if return_mean:
        mean = mean.view(H, W)
        return (mask, mean) if dev_in else (mask.cpu().numpy(), mean.cpu().numpy())
    return mask if dev_in else mask.cpu().numpy()


def label(mask, connectivity: int = 8):
    """(labels, n): the connected components of an (H, W) mask (non-zero:
    foreground) as an int32 (H, W) image, 0 for background and 1..n numbered by
    first pixel in raster order, and their count n (a Python int: one 4-byte
    read).  Equal to ``scipy.ndimage.label`` with the cross (connectivity 4) or
    the full 3 × 3 structure (8), numbering included (ocm_label_u8)."""
    connectivity = _check_connectivity(connectivity)
    mask = _check_mask(mask)
    H, W = (int(s) for s in mask.shape)
    if H * W > 2**31 - 1:
        raise ValueError(f"label: {H} x {W} pixels exceed 2^31 - 1")
    dev_in = _is_dev(mask)
    labels, n = _label_dev(_mask_u8(mask), H, W, connectivity)
    labels = labels.view(H, W)
    return (labels if dev_in else labels.cpu().numpy()), int(n.item())


def gather_rows(X, rows):
    """``X[rows]`` of a 2-D float32 / float64 device tensor (row stride ≥ p) for an
    int64 device index tensor, bit for bit (ocm_gather_rows_f32 / _f64).  The
    indices are not checked on the device."""
    import torch

    from ._lib import Context, ptr, stream_handle

    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dim() == 2 and X.dtype in (torch.float32, torch.float64)):
        raise ValueError("gather_rows: X must be a 2-D float32 or float64 device tensor")
    m, p = X.shape
    if p < 1:
        raise ValueError("gather_rows: X has no columns")
    if (p > 1 and X.stride(1) != 1) or (m > 1 and X.stride(0) < p):
        X = X.contiguous()
    ldx = X.stride(0) if m > 1 else p
    rows = rows.to(device=X.device, dtype=torch.int64).contiguous()
    n = rows.numel()
    out = torch.empty((n, p), dtype=X.dtype, device=X.device)
    fn = "ocm_gather_rows_f64" if X.dtype == torch.float64 else "ocm_gather_rows_f32"
    _call(fn, Context.get(X.device.index).handle, ptr(X), ldx, ptr(rows), n, p, ptr(out), p, stream_handle(X.device))
    return out


@dataclass
class ObjectTable:
    """The objects of an image (``extract_objects``).  ``X`` (n_fg, p): the
    spectra of the kept foreground pixels, object after object, raster order
    inside an object; ``offsets`` (G + 1,) int64 rows of X per object;
    ``pixel_index`` (n_fg,) int64 linear pixel index of every row of X;
    ``labels`` (H, W) int32, 0 background, 1..G; ``n_pixels`` (G,) int64;
    ``centroid`` (G, 2) float64 (row, column); ``bbox`` (G, 4) int64 r0, r1, c0,
    c1; ``shape`` = (H, W); ``depth`` (n_fg,) float64 distance of every row's pixel
    to the background of the un-eroded mask, or None when it was not asked for.
    NumPy arrays or device tensors, as the cube was."""
    X: object
    offsets: object
    pixel_index: object
    labels: object
    n_pixels: object
    centroid: object
    bbox: object
    shape: tuple
    depth: object = None

    def _filled(self, count, values, fill, what):
        dev = _is_dev(self.labels)
        if dev:
            import torch

            vals = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
            vals = vals.to(self.labels.device).reshape(-1)
            floating = vals.dtype.is_floating_point
        else:
            vals = _host(values).reshape(-1)
            floating = np.issubdtype(vals.dtype, np.floating)
        if vals.shape[0] != count:
            raise ValueError(f"{what}: got {vals.shape[0]} values, expected {count}")
        if not floating and isinstance(fill, float) and fill != fill:  # NaN needs a floating map
            vals = vals.double() if dev else vals.astype(np.float64)
        return vals, dev

    def paint(self, values, fill=float("nan")):
        """(H, W) map with ``values[i]`` (one per row of X) at pixel
        ``pixel_index[i]`` and ``fill`` elsewhere."""
        vals, dev = self._filled(int(self.pixel_index.shape[0]), values, fill, "paint")
        H, W = self.shape
        if dev:
            import torch

            out = torch.full((H * W,), fill, dtype=vals.dtype, device=vals.device)
        else:
            out = np.full(H * W, fill, dtype=vals.dtype)
        out[self.pixel_index] = vals
        return out.reshape(H, W)

    def paint_objects(self, values, fill=float("nan")):
        """(H, W) map with ``values[g]`` (one per object) on the pixels of
        object g + 1 and ``fill`` elsewhere."""
        vals, dev = self._filled(int(self.n_pixels.shape[0]), values, fill, "paint_objects")
        if dev:
            import torch

            table = torch.cat([torch.full((1,), fill, dtype=vals.dtype, device=vals.device), vals])
            return table[self.labels.long()]
        return np.concatenate([np.full(1, fill, dtype=vals.dtype), vals])[self.labels]


def extract_objects(cube, mask=None, threshold: float = 1e-6, connectivity: int = 8,
                    min_pixels: int = 1, erode: float = 0.0, fill_holes: bool = False,
                    depth: bool = False) -> ObjectTable:
    """The objects of an (H, W, p) cube as an ``ObjectTable``: foreground mask
    (``foreground_mask`` unless ``mask`` is given), connected components
    (``label``), components of fewer than ``min_pixels`` pixels dropped and the
    rest renumbered 1..G in order, and the spectra of every object gathered
    into adjacent rows of ``X`` in the cube's dtype (float64 stays float64,
    anything else is float32): nut_data.py:64-70 and :131-144 without the
    per-object host loop.

    Everything runs on the device: ocm_fgmask_*, ocm_label_u8, integer tensor
    work on H·W elements for the per-label counts and the pixel order (a sort
    of the unique keys label·H·W + index), ocm_gather_rows_* for the spectra
    and ocm_segsum_f64 over the (n_fg, 2) pixel coordinates for the centroids
    (integer sums below 2⁵³: exact).  One small device-to-host read, the
    per-component pixel counts (n int64), sizes the outputs.  An image without
    foreground gives G = 0, ``X`` of shape (0, p) and ``offsets`` = [0].

    ``fill_holes`` fills the holes of the mask first (``fill_holes``).  ``erode``
    > 0 then keeps, of every object of the un-eroded mask, the pixels deeper than
    the disc: d² > ⌊erode²⌋ with the pixels outside the image as background
    (``erode(mask, radius)``), under the label they already have, so an object
    that erosion cuts through its neck stays one object; pixel counts, and with
    them ``min_pixels``, are taken after erosion, so an object that vanishes is
    dropped.  With ``erode`` > 0 or ``depth=True`` the table's ``depth`` holds √d²
    of every kept pixel (one more ocm_edt_u8 call); with the defaults nothing
    is added and ``depth`` is None."""
    connectivity = _check_connectivity(connectivity)
    r2 = _check_radius(erode, "erode")
    cube, H, W, p = _check_cube(cube)
    if mask is not None:
        mask = _check_mask(mask, (H, W))
    if H * W > 2**31 - 1:
        raise ValueError(f"extract_objects: {H} x {W} pixels exceed 2^31 - 1")
    want_depth = bool(depth) or float(erode) > 0  # a radius below 1 erodes nothing (r2 = 0) and still gives depth
    if want_depth:
        _check_edt_shape(H, W, "extract_objects(erode=, depth=)")
    import torch

    from . import engine

    dev_in = _is_dev(cube)
    X2, ldx = _pixel_rows(cube, H, W, p)
    dev = X2.device
    HW = H * W
    m8 = _fgmask_dev(X2, ldx, threshold)[0] if mask is None else _mask_u8(mask, dev)
    if fill_holes:
        m8 = _fill_holes_dev(m8, H, W)
    lab, _ = _label_dev(m8, H, W, connectivity)
    lab64 = lab.long()
    d2 = None
    if want_depth:
        d2, deep = _edt_dev(m8, H, W, EDT_BORDER_BG, r2, want_d2=True, want_mask=r2 > 0)
        if r2 > 0:
            lab64 = lab64 * deep
    counts = torch.bincount(lab64)[1:].cpu().numpy()  # the one read that sizes the outputs
    keep = counts >= max(int(min_pixels), 1)
    G = int(keep.sum())
    n_pixels = counts[keep].astype(np.int64)
    offsets = np.zeros(G + 1, dtype=np.int64)
    np.cumsum(n_pixels, out=offsets[1:])
    n_fg = int(offsets[-1])
    remap = np.full(counts.size + 1, G + 1, dtype=np.int64)  # background and dropped components sort last
    remap[1:][keep] = np.arange(1, G + 1)
    new = torch.from_numpy(remap).to(dev)[lab64]
    key = torch.sort(new * HW + torch.arange(HW, device=dev))[0][:n_fg]
    pixel_index = key % HW
    labels = torch.where(new <= G, new, torch.zeros_like(new)).to(torch.int32).view(H, W)
    off_d = torch.from_numpy(offsets).to(dev)
    npx_d = torch.from_numpy(n_pixels).to(dev)
    if n_fg:
        X = gather_rows(X2, pixel_index)
        rows, cols = pixel_index // W, pixel_index % W
        coords = torch.stack([rows, cols], dim=1).double()
        centroid = engine.segment_sums(coords, off_d, checked=True) / npx_d[:, None].double()
        seg = key // HW - 1
        c0 = torch.full((G,), W, dtype=torch.int64, device=dev).scatter_reduce_(0, seg, cols, "amin")
        c1 = torch.full((G,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, seg, cols, "amax") + 1
        # raster order inside an object: its first and last pixels hold its first and last rows
        bbox = torch.stack([rows[off_d[:-1]], rows[off_d[1:] - 1] + 1, c0, c1], dim=1)
    else:
        X = torch.empty((0, p), dtype=X2.dtype, device=dev)
        centroid = torch.empty((0, 2), dtype=torch.float64, device=dev)
        bbox = torch.empty((0, 4), dtype=torch.int64, device=dev)
    fields = (X, off_d, pixel_index, labels, npx_d, centroid, bbox)
    if want_depth:
        fields += (d2[pixel_index].double().sqrt(),)
    if not dev_in:
        fields = tuple(f.cpu().numpy() for f in fields)
    return ObjectTable(*fields[:7], shape=(H, W), depth=fields[7] if want_depth else None)
