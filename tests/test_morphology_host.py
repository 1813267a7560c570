"""Mask morphology on the host (ocm.image): the structuring element ``disk``
against its formula, and the argument errors of the morphology functions,
which are raised before the device is touched (no device is present here)."""
import math

import numpy as np
import pytest


@pytest.mark.parametrize("r", [0, 1, 1.5, 2, math.sqrt(2), 4.2])
def test_disk_against_the_formula(r):
    from ocm import image

    d = image.disk(r)
    k, r2 = math.floor(r), math.floor(r * r)
    assert isinstance(d, np.ndarray) and d.dtype == np.bool_ and d.shape == (2 * k + 1, 2 * k + 1)
    want = np.array([[dy * dy + dx * dx <= r2 for dx in range(-k, k + 1)] for dy in range(-k, k + 1)])
    assert np.array_equal(d, want)
    assert d[k, k] and d[k, 0] and d[0, k]  # the centre and the ends of the axes
    assert np.array_equal(d, d.T) and np.array_equal(d, d[::-1]) and np.array_equal(d, d[:, ::-1])


def test_disk_known_elements():
    from ocm import image

    assert image.disk(0).tolist() == [[True]]
    assert image.disk(1).tolist() == [[False, True, False], [True, True, True], [False, True, False]]
    assert image.disk(math.sqrt(2)).all() and image.disk(1.5).all()  # the full 3 × 3 (⌊r²⌋ = 2)
    assert image.disk(2).sum() == 13 and image.disk(4.2).shape == (9, 9)


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library or of a device tensor fails the test."""
    from ocm import _lib, engine

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(engine, "require_device", boom)


MASK = np.ones((5, 7), dtype=bool)


@pytest.mark.parametrize("radius", [-1, -0.5, float("nan"), float("inf"), "wide", None])
def test_bad_radius(no_device, radius):
    from ocm import image

    for fn in (image.erode, image.dilate, image.opening, image.closing):
        with pytest.raises(ValueError, match="radius"):
            fn(MASK, radius)
    with pytest.raises(ValueError, match="radius"):
        image.disk(radius)


def test_unknown_border(no_device):
    from ocm import image

    for border in ("reflect", "bg", None, 0):
        with pytest.raises(ValueError, match="border"):
            image.erode(MASK, 1, border=border)
        with pytest.raises(ValueError, match="border"):
            image.distance_transform(MASK, border=border)


@pytest.mark.parametrize("shape", [(7,), (2, 3, 4), (0, 5), (5, 0)])
def test_mask_must_be_2d_and_non_empty(no_device, shape):
    from ocm import image

    mask = np.ones(shape, dtype=bool)
    for fn in (image.erode, image.dilate, image.opening, image.closing):
        with pytest.raises(ValueError, match="mask"):
            fn(mask, 1)
    for fn in (image.distance_transform, image.fill_holes):
        with pytest.raises(ValueError, match="mask"):
            fn(mask)


@pytest.mark.parametrize("shape", [(1, 32768), (32768, 1)])
def test_side_above_32767(no_device, shape):
    from ocm import image

    mask = np.ones(shape, dtype=bool)
    for fn in (image.erode, image.dilate, image.opening, image.closing):
        with pytest.raises(ValueError, match="32767"):
            fn(mask, 1)
    with pytest.raises(ValueError, match="32767"):
        image.distance_transform(mask)
    cube = np.zeros(shape + (1,), dtype=np.float32)
    with pytest.raises(ValueError, match="32767"):
        image.extract_objects(cube, erode=1)
    with pytest.raises(ValueError, match="32767"):
        image.extract_objects(cube, depth=True)


@pytest.mark.parametrize("erode", [-1, -1e-9, float("nan")])
def test_extract_objects_bad_erode(no_device, erode):
    from ocm import image

    with pytest.raises(ValueError, match="erode"):
        image.extract_objects(np.zeros((4, 4, 3), dtype=np.float32), erode=erode)


def test_object_table_depth_is_a_trailing_optional_field():
    import dataclasses

    from ocm import image

    names = [f.name for f in dataclasses.fields(image.ObjectTable)]
    assert names == ["X", "offsets", "pixel_index", "labels", "n_pixels", "centroid", "bbox", "shape", "depth"]
    t = image.ObjectTable(*([None] * 7), shape=(2, 3))
    assert t.depth is None and t.shape == (2, 3)
