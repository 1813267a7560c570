"""Mask morphology on the GPU (ocm.image; ocm_edt_u8) against scipy.ndimage:
the squared distance transform equal to SciPy's to the last integer, erosion,
dilation, opening, closing and hole filling equal to their SciPy expressions,
and extract_objects(erode=, fill_holes=, depth=) equal to the host route.

Shapes follow the kernel's constants, read from the source: the band of
EDT_BH rows that one word of column bits holds, the EDT_SEG columns of a
segment of the row pass and the EDT_NT threads that stride along a row; on,
one under and one over each, and widths that are and are not multiples of 4
(the 4-bytes-per-lane and the single-byte path)."""
import contextlib
import functools
import io
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(REPO, "ocm-vae-simca_amd", "csrc", "ocm_edt.hip")).read()
BH = int(re.search(r"constexpr int EDT_BH = (\d+);", SRC).group(1))
SEG = int(re.search(r"constexpr int EDT_SEG = (\d+);", SRC).group(1))
NT = int(re.search(r"constexpr int EDT_NT = (\d+);", SRC).group(1))
NONE = 2**31 - 1
FULL = np.ones((3, 3))
RADII = [0, 1, 1.5, 2, 3, 4.2]

WIDTHS = [3, SEG - 1, SEG, SEG + 1, 2 * SEG + 3]
HEIGHTS = [3, BH - 1, BH, BH + 1, 2 * BH + 3]
SHAPES = [(1, 1), (1, 2 * SEG + 3), (2 * BH + 3, 1), (5, NT + 3), (5, NT + 4)] + [(h, w) for h in HEIGHTS for w in WIDTHS]


def ref_d2(fg, border):
    """int64 d² of a bool mask by SciPy; NONE everywhere when there is no background at all."""
    fg = np.asarray(fg, dtype=bool)
    if border == "background":
        d = ndimage.distance_transform_edt(np.pad(fg, 1))[1:-1, 1:-1]
    elif fg.all():
        return np.full(fg.shape, NONE, dtype=np.int64)
    else:
        d = ndimage.distance_transform_edt(fg)
    return np.rint(d * d).astype(np.int64)


def ref_depth(d2):
    with np.errstate(invalid="ignore"):
        return np.where(d2 == NONE, np.inf, np.sqrt(d2.astype(np.float64)))


def check_d2(mask, tag=""):
    from ocm import image

    dev = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    for border in ("ignore", "background"):
        want = ref_d2(mask, border)
        got = image.distance_transform(dev, border=border, squared=True)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32 and got.shape == mask.shape
        bad = np.argwhere(got.cpu().numpy() != want)
        assert bad.size == 0, (tag, border, bad[:5].tolist())
        depth = image.distance_transform(dev, border=border)
        assert depth.dtype == torch.float64 and np.array_equal(depth.cpu().numpy(), ref_depth(want)), (tag, border)


# ------------------------------------------------------------------ 1. d² against SciPy
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_d2_equals_scipy(shape):
    H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    for density in (0.5, 0.9, 0.99):
        check_d2(rng.random(shape) < density, f"{shape} density {density}")


# ------------------------------------------------------------------ 2. one background pixel
def test_single_background_pixel_across_every_segment():
    from ocm import image

    H, W = 2 * BH + 3, 2 * SEG + 3
    yy, xx = np.mgrid[:H, :W]
    for py, px in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        mask = np.ones((H, W), dtype=bool)
        mask[py, px] = False
        want = (yy - py) ** 2 + (xx - px) ** 2  # the minimum comes from another band and another segment
        assert np.array_equal(ref_d2(mask, "ignore"), want)
        got = image.distance_transform(mask, squared=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want), (py, px)
        check_d2(mask, f"one background pixel at {(py, px)}")


# ------------------------------------------------------------------ 3. columns without background
def test_columns_without_background_and_uniform_masks():
    from ocm import image

    H, W = BH + 9, 2 * SEG + 3
    mask = np.ones((H, W), dtype=bool)
    mask[5, ::7] = False  # six of seven columns hold no background: g is "none" there
    mask[H - 2, 3] = False
    check_d2(mask, "sparse columns")
    lone = np.ones((H, W), dtype=bool)
    lone[:, SEG] = False  # whole segments of "none" either side of one background column
    lone[:, SEG] |= np.arange(H) % 2 == 0
    check_d2(lone, "one column")
    zeros, ones = np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool)
    assert not image.distance_transform(zeros, squared=True).any()
    assert not image.distance_transform(zeros, border="background").any()
    d2 = image.distance_transform(ones, squared=True)
    assert d2.dtype == np.int32 and (d2 == NONE).all()
    assert np.isposinf(image.distance_transform(ones)).all()
    yy, xx = np.mgrid[:H, :W]
    want = np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx)) ** 2
    assert np.array_equal(image.distance_transform(ones, border="background", squared=True), want)
    assert np.array_equal(image.distance_transform(ones, border="background"), np.sqrt(want))
    # erosion without any background: border "ignore" keeps everything, whatever the radius
    assert image.erode(ones, 1000, border="ignore").all()
    assert not image.dilate(zeros, 1000).any()


# ------------------------------------------------------------------ 4. morphology against SciPy
def scipy_morphology(mask, r):
    from ocm import image

    disc = image.disk(r)
    m = np.asarray(mask) != 0
    return {
        "erode": ndimage.binary_erosion(m, disc, border_value=0),
        "erode_ignore": ndimage.binary_erosion(m, disc, border_value=1),
        "dilate": ndimage.binary_dilation(m, disc),
        "opening": ndimage.binary_opening(m, disc),
        "closing": ndimage.binary_erosion(ndimage.binary_dilation(m, disc), disc, border_value=1),
    }


def ours(mask, r):
    from ocm import image

    return {"erode": image.erode(mask, r), "erode_ignore": image.erode(mask, r, border="ignore"),
            "dilate": image.dilate(mask, r), "opening": image.opening(mask, r), "closing": image.closing(mask, r)}


@functools.lru_cache(maxsize=None)
def morphology_masks():
    from ocm import synth

    rng = np.random.default_rng(11)
    H, W = BH + 7, 2 * SEG + 5
    out = {"random0.5": rng.random((H, W)) < 0.5, "random0.9": rng.random((H, W)) < 0.9,
           "random0.1": rng.random((H, W)) < 0.1}
    cube = synth.scene(H, W, 3, blobs=9, seed=4)
    out["scene"] = (cube.mean(dim=2) != 0).cpu().numpy()
    ring = synth.scene(H, W, 3, [(30, 40, 14), (36, 100, 9), (2, 2, 6)], seed=1).mean(dim=2).cpu().numpy() != 0
    yy, xx = np.mgrid[:H, :W]
    ring &= ~((yy - 30) ** 2 + (xx - 40) ** 2 <= 16)  # a hole, and specks in another disc
    ring[36, 100] = ring[33, 97] = False
    out["scene_with_holes"] = ring
    for v in out.values():
        assert 0 < v.sum() < v.size
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("name", ["random0.5", "random0.9", "random0.1", "scene", "scene_with_holes"])
def test_morphology_equals_scipy(name, r):
    mask = morphology_masks()[name]
    want = scipy_morphology(mask, r)
    got = ours(mask.copy(), r)  # NumPy in, NumPy out
    for k, v in got.items():
        assert isinstance(v, np.ndarray) and v.dtype == np.bool_ and np.array_equal(v, want[k]), (k, "numpy")
    got = ours(torch.from_numpy(mask.copy()).cuda(), r)  # tensor in, device tensor out
    for k, v in got.items():
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.bool, k
        assert np.array_equal(v.cpu().numpy(), want[k]), (k, "tensor")
    for nonbool in (mask * 7.5, (mask * 200).astype(np.uint8), torch.from_numpy(mask * -2).cuda()):
        got = ours(nonbool, r)  # non-zero is foreground
        for k, v in got.items():
            assert np.array_equal(v.cpu().numpy() if isinstance(v, torch.Tensor) else v, want[k]), (k, "non-bool")


@pytest.mark.parametrize("name", ["random0.5", "random0.9", "random0.1", "scene", "scene_with_holes"])
def test_fill_holes_equals_scipy(name):
    from ocm import image

    mask = morphology_masks()[name]
    want = ndimage.binary_fill_holes(mask)
    if name == "scene_with_holes":
        assert want.sum() > mask.sum()
    got = image.fill_holes(mask.copy())
    assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, want)
    dev = image.fill_holes(torch.from_numpy(mask * 3.0).cuda())
    assert dev.is_cuda and dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), want)
    frame = np.zeros((BH + 2, SEG + 2), dtype=bool)  # a frame on the image edge: everything inside is a hole
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    assert image.fill_holes(frame).all() and ndimage.binary_fill_holes(frame).all()
    assert np.array_equal(image.fill_holes(frame[1:]), ndimage.binary_fill_holes(frame[1:]))  # open at the top


# ------------------------------------------------------------------ 5. the raw entry
def raw_edt(mask_u8, H, W, flags, r2, want_d2, want_mask):
    from ocm import _lib

    lib, ctx = _lib.load(), _lib.Context.get(0).handle
    d2 = torch.full((H * W,), -7, dtype=torch.int32, device="cuda") if want_d2 else None
    out = torch.full((H * W,), 9, dtype=torch.uint8, device="cuda") if want_mask else None
    rc = lib.ocm_edt_u8(ctx, _lib.ptr(mask_u8), H, W, flags, r2, _lib.ptr(d2), _lib.ptr(out),
                        _lib.stream_handle(torch.device("cuda", 0)))
    assert rc == 0, (flags, r2)
    return (None if d2 is None else d2.cpu().numpy().reshape(H, W),
            None if out is None else out.cpu().numpy().reshape(H, W))


@pytest.mark.parametrize("shape,offset", [((BH + 5, SEG + 4), 0), ((BH + 5, SEG + 4), 1), ((BH + 5, SEG + 3), 0)],
                         ids=["w%4=0", "w%4=0,unaligned", "w%4=3"])
def test_raw_entry_every_flag_combination(shape, offset):
    """Bytes 0 / 1 / 255 as the mask; `offset` moves the mask off a 4-byte boundary, which sends a
    width that is a multiple of 4 down the single-byte path."""
    H, W = shape
    rng = np.random.default_rng(W + offset)
    mask = (rng.random(shape) < 0.8) * rng.choice(np.array([1, 255], dtype=np.uint8), size=shape)
    buf = torch.zeros(H * W + 8, dtype=torch.uint8, device="cuda")
    m8 = buf[offset:offset + H * W]
    m8.copy_(torch.from_numpy(mask.astype(np.uint8).ravel()))
    assert m8.data_ptr() % 4 == offset
    for flags in range(8):
        fg = (mask != 0) != bool(flags & 2)
        want_d2 = ref_d2(fg, "background" if flags & 1 else "ignore")
        for r2 in (0, 2, 9, 2**40):
            want_mask = (want_d2 > r2) != bool(flags & 4)
            both = raw_edt(m8, H, W, flags, r2, True, True)
            assert np.array_equal(both[0], want_d2) and np.array_equal(both[1], want_mask), (flags, r2)
            only_d2 = raw_edt(m8, H, W, flags, r2, True, False)
            only_mask = raw_edt(m8, H, W, flags, r2, False, True)
            assert np.array_equal(only_d2[0], both[0]) and np.array_equal(only_mask[1], both[1]), (flags, r2)
            again = raw_edt(m8, H, W, flags, r2, True, True)  # two runs give the same bytes
            assert np.array_equal(again[0], both[0]) and np.array_equal(again[1], both[1])
    # without any background OCM_EDT_NONE is greater than any r2, INT32_MAX and above included
    ones = torch.ones(H * W, dtype=torch.uint8, device="cuda")
    for r2 in (0, NONE - 1, NONE, 2**40):
        d2, out = raw_edt(ones, H, W, 0, r2, True, True)
        assert (d2 == NONE).all() and (out == 1).all(), r2
        assert (raw_edt(ones, H, W, 4, r2, False, True)[1] == 0).all(), r2


def test_raw_entry_argument_errors():
    from ocm import _lib

    lib, ctx = _lib.load(), _lib.Context.get(0).handle
    st = _lib.stream_handle(torch.device("cuda", 0))
    mask = torch.ones(16, dtype=torch.uint8, device="cuda")
    d2 = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((16,), 9, dtype=torch.uint8, device="cuda")
    bad = [(0, 4, 0, 1), (4, 0, 0, 1), (-1, 4, 0, 1), (4, -1, 0, 1), (32768, 4, 0, 1), (4, 32768, 0, 1),
           (4, 4, 8, 1), (4, 4, 15, 1), (4, 4, -1, 1), (4, 4, 0, -1), (4, 4, 1, -(2**40))]
    for H, W, flags, r2 in bad:
        assert lib.ocm_edt_u8(ctx, None, H, W, flags, r2, None, None, st) == _lib.OCM_ERR_ARG, (H, W, flags, r2)
        assert lib.ocm_edt_u8(ctx, _lib.ptr(mask), H, W, flags, r2, _lib.ptr(d2), _lib.ptr(out), st) == \
            _lib.OCM_ERR_ARG, (H, W, flags, r2)
    assert lib.ocm_edt_u8(ctx, _lib.ptr(mask), 4, 4, 0, 1, None, None, st) == _lib.OCM_ERR_ARG  # both outputs NULL
    assert lib.ocm_edt_u8(ctx, None, 4, 4, 0, 1, _lib.ptr(d2), _lib.ptr(out), st) == _lib.OCM_ERR_ARG
    torch.cuda.synchronize()
    assert (d2 == -7).all() and (out == 9).all()  # nothing was launched
    assert lib.ocm_edt_u8(ctx, _lib.ptr(mask), 4, 4, 1, 1, _lib.ptr(d2), _lib.ptr(out), st) == 0
    torch.cuda.synchronize()
    assert d2.view(4, 4).tolist() == [[1, 1, 1, 1], [1, 4, 4, 1], [1, 4, 4, 1], [1, 1, 1, 1]]
    assert out.view(4, 4).tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]


# ------------------------------------------------------------------ 6. extract_objects
FIELDS = ("offsets", "pixel_index", "labels", "n_pixels", "bbox", "centroid")


@functools.lru_cache(maxsize=None)
def object_scene():
    """A dumbbell (two discs of radius 6 joined by a neck one pixel wide), a disc of radius 1, a disc
    of radius 9 with a hole of radius 2, a disc cut by the image edge; float32 spectra in [1, 2] on
    the foreground, exact zeros elsewhere."""
    H, W, p = BH + 11, 2 * SEG + 9, 5
    yy, xx = np.mgrid[:H, :W]
    disc = lambda r, c, rad: (yy - r) ** 2 + (xx - c) ** 2 <= rad * rad
    mask = disc(12, 12, 6) | disc(12, 40, 6)
    mask[12, 12:40] = True
    mask |= disc(30, 8, 1)
    mask |= disc(50, 70, 9) & ~disc(50, 70, 2)
    mask |= disc(H - 3, W - 20, 7)
    rng = np.random.default_rng(3)
    cube = np.where(mask[:, :, None], rng.uniform(1.0, 2.0, size=(H, W, p)), 0.0).astype(np.float32)
    mask.setflags(write=False)
    cube.setflags(write=False)
    return mask, cube


def host_route(mask, erode=0.0, fill=False, min_pixels=1, conn=8):
    """SciPy's labels of the (filled) mask, SciPy's erosion, objects_from_labels on labels * eroded
    (labels that vanish are dropped and the rest renumbered), SciPy's depth of the kept pixels."""
    from ocm import image

    m = ndimage.binary_fill_holes(mask) if fill else mask
    lab, _ = ndimage.label(m, structure=FULL if conn == 8 else None)
    kept = ndimage.binary_erosion(m, image.disk(erode), border_value=0) if erode > 0 else m
    ref = image.objects_from_labels(lab * kept, min_pixels=min_pixels)
    depth = np.sqrt(ref_d2(m, "background").astype(np.float64)).ravel()[ref.order]
    return ref, depth


def check_table(t, cube, ref, depth):
    p = cube.shape[2]
    get = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v
    for name, want in zip(FIELDS, (ref.offsets, ref.order, ref.labels, ref.n_pixels, ref.bbox, ref.centroid)):
        got = get(getattr(t, name))
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    X = get(t.X)
    assert X.dtype == cube.dtype and X.shape == (ref.order.size, p)
    assert np.array_equal(X.view(np.int32), cube.reshape(-1, p)[ref.order].view(np.int32))
    assert t.shape == cube.shape[:2]
    if depth is None:
        assert t.depth is None
    else:
        got = get(t.depth)
        assert got.dtype == np.float64 and got.shape == depth.shape and np.array_equal(got, depth)


def test_extract_objects_eroded_equals_the_host_route():
    from ocm import image

    mask, cube = object_scene()
    dev = torch.from_numpy(cube.copy()).cuda()
    G0 = host_route(mask)[0].n_pixels.size
    assert G0 == 4
    for erode in (1, 1.5, 2, 4.2):
        for fill in (False, True):
            ref, depth = host_route(mask, erode, fill)
            t = image.extract_objects(dev, erode=erode, fill_holes=fill)
            assert all(isinstance(getattr(t, f), torch.Tensor) and getattr(t, f).is_cuda
                       for f in FIELDS + ("X", "depth"))
            check_table(t, cube, ref, depth)
            assert (depth > np.floor(erode * erode) ** 0.5).all()
            G = ref.n_pixels.size
            lab = ref.labels
            if erode == 1:  # the neck goes, its two discs stay one object; the radius-1 disc keeps its centre
                assert G == 4 and lab[12, 12] == lab[12, 40] == 1 and lab[12, 26] == 0 and ref.n_pixels[1] == 1
            else:  # the radius-1 disc vanishes (at 4.2 the unfilled ring too), the others are renumbered
                assert G == (2 if erode > 4 and not fill else 3) and lab[30, 8] == 0
                assert lab[12, 12] == lab[12, 40] == 1
            assert (lab[50, 70] != 0) == fill  # the hole's centre is kept only when filled
    # min_pixels counts after erosion; connectivity 4; an explicit mask; depth alone
    ref, depth = host_route(mask, 2, False, min_pixels=100)
    assert ref.n_pixels.size == 2  # of the three objects left, the one eroded below 100 pixels is dropped
    check_table(image.extract_objects(dev, erode=2, min_pixels=100), cube, ref, depth)
    rng = np.random.default_rng(5)
    rmask = rng.random(mask.shape) < 0.5
    ref, depth = host_route(rmask, 1, True, min_pixels=2, conn=4)
    assert ref.n_pixels.size >= 2
    for m_in in (rmask, torch.from_numpy(rmask).cuda()):
        check_table(image.extract_objects(dev, mask=m_in, connectivity=4, min_pixels=2, erode=1, fill_holes=True),
                    cube, ref, depth)
    ref, depth = host_route(mask)
    check_table(image.extract_objects(dev, depth=True), cube, ref, depth)
    check_table(image.extract_objects(dev, erode=0.5), cube, ref, depth)  # ⌊0.25⌋ = 0 erodes nothing
    # NumPy in, NumPy out
    ref, depth = host_route(mask, 2, True)
    th = image.extract_objects(cube.copy(), erode=2, fill_holes=True)
    assert all(isinstance(getattr(th, f), np.ndarray) for f in FIELDS + ("X", "depth"))
    check_table(th, cube, ref, depth)


def test_extract_objects_defaults_unchanged_and_without_foreground():
    from ocm import image

    mask, cube = object_scene()
    dev = torch.from_numpy(cube.copy()).cuda()
    ref, _ = host_route(mask)
    for t in (image.extract_objects(dev), image.extract_objects(dev, erode=0, fill_holes=False, depth=False)):
        check_table(t, cube, ref, None)
    filled, depth = host_route(mask, 0, True)
    assert filled.n_pixels.sum() > ref.n_pixels.sum()
    check_table(image.extract_objects(dev, fill_holes=True), cube, filled, None)
    zeros = torch.zeros((13, 17, 5), device="cuda")
    for kw in ({"erode": 2}, {"depth": True}, {"erode": 1.5, "fill_holes": True}):
        t = image.extract_objects(zeros, **kw)
        assert t.X.shape == (0, 5) and t.offsets.tolist() == [0] and not t.labels.any()
        assert t.depth.shape == (0,) and t.depth.dtype == torch.float64
    gone = image.extract_objects(dev, erode=50)  # every object vanishes
    assert gone.X.shape == (0, 5) and gone.n_pixels.shape == (0,) and gone.depth.shape == (0,)


# ------------------------------------------------------------------ 7. end to end
def test_eroded_scene_through_predict_objects():
    from ocm import image, synth
    from utils import SIMCA

    H, W, p = 64, 96, 64
    blobs = [(12, 12, 8), (12, 40, 7), (40, 14, 9), (44, 44, 6), (30, 80, 1)]
    cube = synth.scene(H, W, p, blobs, seed=5)
    full = image.extract_objects(cube)
    objs = image.extract_objects(cube, erode=2)
    assert full.n_pixels.numel() == 5 and objs.n_pixels.numel() == 4  # the radius-1 disc is gone
    assert (objs.n_pixels < full.n_pixels[full.n_pixels > 5]).all() and (objs.depth > 2).all()
    est = SIMCA(n_components=6, model_class=0, verbose=False)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(objs.X, np.zeros(objs.X.shape[0], dtype=np.int64))
    res = est.predict_objects(objs.X, offsets=objs.offsets, rule="vote")
    assert res.pred.shape[0] == 4
    painted = objs.paint_objects(res.pred[:, 0])
    assert torch.equal(torch.isnan(painted), objs.labels == 0)
    depth_map = objs.paint(objs.depth)
    assert torch.equal(torch.isnan(depth_map), objs.labels == 0)
    want = image.distance_transform(full.labels != 0, border="background")
    kept = objs.labels != 0
    assert torch.equal(depth_map[kept], want[kept])
