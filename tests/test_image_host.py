"""ocm.image on the host: objects_from_labels against the per-object loop of
the reference (np.argwhere per label, in order), ndimage.find_objects and
np.bincount on SciPy's labels, and the argument checks that need no device."""
import numpy as np
import pytest
from scipy import ndimage

from ocm import image

FULL = np.ones((3, 3))


def structured_masks():
    rng = np.random.default_rng(3)
    out = {f"random{d}": rng.random((37, 53)) < d for d in (0.1, 0.3, 0.45, 0.6)}
    yy, xx = np.mgrid[:37, :53]
    out["checkerboard"] = (yy + xx) % 2 == 0
    out["stripes"] = yy % 3 == 0
    discs = np.zeros((37, 53), dtype=bool)
    for r, c, rad in ((8, 9, 5), (20, 30, 7), (30, 8, 3), (5, 45, 1), (33, 40, 0)):
        discs |= (yy - r) ** 2 + (xx - c) ** 2 <= rad * rad
    out["discs"] = discs
    out["full"] = np.ones((4, 6), dtype=bool)
    out["row"] = np.array([[1, 0, 1, 1, 0, 1]], dtype=bool)
    return out


def check_against_loop(lab, objs, kept):
    """`kept`: the labels of `lab` that survive, ascending; objs must describe them as 1..G."""
    H, W = lab.shape
    G = len(kept)
    assert objs.offsets.shape == (G + 1,) and objs.offsets.dtype == np.int64 and objs.offsets[0] == 0
    assert objs.order.dtype == np.int64 and objs.n_pixels.dtype == np.int64 and objs.bbox.dtype == np.int64
    assert objs.centroid.shape == (G, 2) and objs.centroid.dtype == np.float64 and objs.bbox.shape == (G, 4)
    assert objs.labels.dtype == np.int32 and objs.labels.shape == (H, W)
    want_lab = np.zeros_like(lab)
    for g, old in enumerate(kept):
        m = lab == old
        want_lab[m] = g + 1
        coords = np.argwhere(m)  # raster order: the row order of hsi_image[labeled_array == obj]
        got = objs.order[objs.offsets[g]:objs.offsets[g + 1]]
        assert np.array_equal(got, coords[:, 0] * W + coords[:, 1])
        assert np.array_equal(objs.centroid[g], coords.mean(axis=0))
        assert objs.n_pixels[g] == m.sum()
    assert np.array_equal(objs.labels, want_lab)
    slices = ndimage.find_objects(objs.labels)
    assert len(slices) == G
    for g, (sr, sc) in enumerate(slices):
        assert objs.bbox[g].tolist() == [sr.start, sr.stop, sc.start, sc.stop]
    assert np.array_equal(objs.n_pixels, np.bincount(objs.labels.ravel(), minlength=G + 1)[1:])
    assert objs.offsets[-1] == objs.order.size == (objs.labels > 0).sum()


@pytest.mark.parametrize("name", sorted(structured_masks()))
@pytest.mark.parametrize("structure", [None, FULL], ids=["conn4", "conn8"])
def test_objects_from_labels_against_the_loop(name, structure):
    mask = structured_masks()[name]
    lab, n = ndimage.label(mask, structure=structure)
    check_against_loop(lab, image.objects_from_labels(lab), list(range(1, n + 1)))


@pytest.mark.parametrize("min_pixels", [2, 5, 40, 10_000])
def test_min_pixels_drops_and_renumbers(min_pixels):
    for name in ("random0.3", "random0.45", "discs"):
        lab, n = ndimage.label(structured_masks()[name], structure=FULL)
        counts = np.bincount(lab.ravel())[1:]
        kept = [g + 1 for g in range(n) if counts[g] >= min_pixels]
        assert len(kept) < n
        check_against_loop(lab, image.objects_from_labels(lab, min_pixels=min_pixels), kept)


def test_labels_with_gaps_and_other_dtypes():
    lab = np.array([[0, 5, 5, 0], [2, 0, 0, 9], [2, 0, 9, 9]], dtype=np.int64)
    check_against_loop(lab, image.objects_from_labels(lab), [2, 5, 9])
    check_against_loop(lab, image.objects_from_labels(lab.astype(np.uint8), min_pixels=3), [9])
    with pytest.raises(ValueError):
        image.objects_from_labels(lab.astype(np.float64))
    with pytest.raises(ValueError):
        image.objects_from_labels(lab - 1)
    with pytest.raises(ValueError):
        image.objects_from_labels(lab.ravel())


def test_no_objects_and_one_pixel():
    objs = image.objects_from_labels(np.zeros((5, 7), dtype=np.int32))
    assert objs.order.shape == (0,) and objs.offsets.tolist() == [0] and objs.n_pixels.shape == (0,)
    assert objs.centroid.shape == (0, 2) and objs.bbox.shape == (0, 4) and not objs.labels.any()
    one = image.objects_from_labels(np.ones((1, 1), dtype=np.int32))
    assert one.order.tolist() == [0] and one.offsets.tolist() == [0, 1] and one.n_pixels.tolist() == [1]
    assert one.centroid.tolist() == [[0.0, 0.0]] and one.bbox.tolist() == [[0, 1, 0, 1]]
    assert image.objects_from_labels(np.zeros((1, 1), dtype=np.int32)).offsets.tolist() == [0]


def host_table(lab, p=3):
    o = image.objects_from_labels(lab)
    X = np.arange(o.order.size * p, dtype=np.float32).reshape(-1, p)
    return image.ObjectTable(X, o.offsets, o.order, o.labels, o.n_pixels, o.centroid, o.bbox, lab.shape)


def test_paint_on_the_host():
    lab, n = ndimage.label(structured_masks()["discs"], structure=FULL)
    t = host_table(lab)
    per_pixel = np.repeat(np.arange(1, n + 1), t.n_pixels)
    assert np.array_equal(t.paint(per_pixel, fill=0), lab)
    nanmap = t.paint(per_pixel)
    assert nanmap.dtype == np.float64 and np.array_equal(np.isnan(nanmap), lab == 0)
    vals = np.linspace(-1.0, 1.0, n)
    got = t.paint_objects(vals)
    assert np.array_equal(np.isnan(got), lab == 0)
    for g in range(n):
        assert (got[lab == g + 1] == vals[g]).all()
    assert np.array_equal(t.paint_objects(np.arange(1, n + 1), fill=0), lab)


def test_value_errors_need_no_device():
    with pytest.raises(ValueError, match="cube"):
        image.extract_objects(np.zeros((5, 7), dtype=np.float32))
    with pytest.raises(ValueError, match="cube"):
        image.foreground_mask(np.zeros((2, 5, 7, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="connectivity"):
        image.label(np.ones((4, 4), dtype=bool), connectivity=3)
    with pytest.raises(ValueError, match="connectivity"):
        image.extract_objects(np.zeros((4, 4, 3), dtype=np.float32), connectivity=3)
    with pytest.raises(ValueError, match="mask"):
        image.extract_objects(np.zeros((4, 5, 3), dtype=np.float32), mask=np.ones((5, 4), dtype=bool))
    with pytest.raises(ValueError, match="mask"):
        image.label(np.ones(16, dtype=bool))
    lab, n = ndimage.label(structured_masks()["discs"], structure=FULL)
    t = host_table(lab)
    with pytest.raises(ValueError, match="paint"):
        t.paint(np.zeros(t.X.shape[0] + 1))
    with pytest.raises(ValueError, match="paint_objects"):
        t.paint_objects(np.zeros(n - 1))
