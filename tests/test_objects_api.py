"""CPU-side checks of the object-level surface: the C ABI declares
ocm_segsum_f32 / _f64 and the binding lists them with the header's argument
count; ocm.objects' host helpers (segment_offsets, check_offsets,
stack_objects); SIMCA.predict_objects rejects bad arguments before any device
work."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ocm.h")


def header_argcount(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*int\s+" + name + r"\s*\((.*?)\)\s*;", txt, re.M | re.S)
    assert m, f"include/ocm.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ["ocm_segsum_f32", "ocm_segsum_f64"])
def test_header_and_binding_declare_segsum(name):
    from ocm import _lib

    n = header_argcount(name)
    assert n == 10
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_i32 and len(args) == n
    assert _lib.ABI_VERSION == 12


def test_segment_offsets():
    from ocm.objects import segment_offsets

    def eq(ids, want):
        got = segment_offsets(ids)
        assert got.dtype == np.int64 and got.tolist() == want, (ids, got)

    eq([7, 7, 7, 2, 2, 9, 4, 4, 4, 4], [0, 3, 5, 6, 10])  # typical: order of appearance, not of value
    eq(np.full(5, 3), [0, 5])                                # a single object
    eq(np.arange(6)[::-1], [0, 1, 2, 3, 4, 5, 6])            # all distinct
    eq(np.zeros(0, dtype=np.int64), [0])                     # empty
    eq([], [0])
    eq(np.array(["a", "a", "b"]), [0, 2, 3])                 # ids need not be integers
    with pytest.raises(ValueError, match="adjacent"):
        segment_offsets([1, 1, 2, 2, 1])
    with pytest.raises(ValueError, match="shape"):
        segment_offsets(np.zeros((3, 2), dtype=np.int64))


def test_check_offsets():
    from ocm.objects import check_offsets

    ok = check_offsets([0, 2, 2, 5], 5)
    assert ok.dtype == np.int64 and ok.tolist() == [0, 2, 2, 5]
    assert check_offsets(np.array([1, 3], dtype=np.int32), 5).tolist() == [1, 3]  # a sub-range of the rows
    assert check_offsets([0], 0).tolist() == [0]
    with pytest.raises(ValueError, match="decreasing"):
        check_offsets([0, 3, 2, 5], 5)
    with pytest.raises(ValueError, match="negative"):
        check_offsets([-1, 2, 5], 5)
    with pytest.raises(ValueError, match="out of range"):
        check_offsets([0, 2, 6], 5)
    with pytest.raises(ValueError, match="integers"):
        check_offsets(np.array([0.0, 2.0, 5.0]), 5)
    with pytest.raises(ValueError, match="integers"):
        check_offsets([0, 2.5, 5], 5)
    with pytest.raises(ValueError, match="1-D"):
        check_offsets(np.zeros((2, 2), dtype=np.int64), 5)
    with pytest.raises(ValueError):
        check_offsets([], 5)


def test_stack_objects_both_forms():
    from ocm.objects import stack_objects
    from utils import data_utils

    assert data_utils.stack_objects is stack_objects and "stack_objects" in data_utils.__all__
    rng = np.random.default_rng(0)
    blocks = [rng.standard_normal((n, 5)).astype(np.float32) for n in (3, 1, 0, 4)]
    Xa, oa = stack_objects(blocks)
    Xd, od = stack_objects([{"spectral_data": b, "obj_idx": i, "img_idx": 0} for i, b in enumerate(blocks)])
    assert oa.dtype == np.int64 and oa.tolist() == [0, 3, 4, 4, 8]
    assert Xa.dtype == np.float32 and Xa.shape == (8, 5)
    assert np.array_equal(Xa, np.vstack(blocks))
    assert np.array_equal(Xa, Xd) and np.array_equal(oa, od)
    with pytest.raises(ValueError, match="no objects"):
        stack_objects([])
    with pytest.raises(ValueError, match="width"):
        stack_objects([np.zeros((2, 5)), np.zeros((2, 4))])


def _stub(classes):
    """A fitted-state stub: no device, no arrays (the argument checks come first)."""
    from utils import SIMCA

    est = SIMCA(n_components=2, model_class=list(classes), verbose=False)
    est._model = {c: {"T2_limit": 1.0, "Q_limit": 1.0, "D_limit": 1.0} for c in classes}
    est._fits = {c: object() for c in classes}
    est._out_dtype = np.float32
    est._sharded = False
    return est


def test_predict_objects_argument_errors():
    from utils import SIMCA
    from utils.SIMCA import ObjectResult

    assert callable(getattr(SIMCA, "predict_objects", None))
    assert {"pred", "score", "fraction", "counts", "metrics"} <= set(ObjectResult.__dataclass_fields__)
    X = np.zeros((6, 8), dtype=np.float32)
    ids = np.array([0, 0, 1, 1, 1, 2])
    off = [0, 2, 5, 6]
    est = _stub([0])
    with pytest.raises(ValueError, match="exactly one"):
        est.predict_objects(X)
    with pytest.raises(ValueError, match="exactly one"):
        est.predict_objects(X, objects=ids, offsets=off)
    with pytest.raises(ValueError, match="rows"):
        est.predict_objects(X, objects=ids[:5])  # a wrong length
    with pytest.raises(ValueError, match="from 0 to 6"):
        est.predict_objects(X, offsets=[0, 2, 5])  # rows 5.. belong to no object
    with pytest.raises(ValueError, match="from 0 to 6"):
        est.predict_objects(X, offsets=[1, 2, 6])
    with pytest.raises(ValueError, match="out of range"):
        est.predict_objects(X, offsets=[0, 2, 7])
    with pytest.raises(ValueError, match="adjacent"):
        est.predict_objects(X, objects=[0, 0, 1, 1, 0, 0])
    with pytest.raises(ValueError, match="empty"):
        est.predict_objects(X, offsets=[0, 2, 2, 6])
    with pytest.raises(ValueError, match="rule="):
        est.predict_objects(X, objects=ids, rule="majority")
    for bad in (0, 1.5, -0.1):
        with pytest.raises(ValueError, match="min_fraction"):
            est.predict_objects(X, objects=ids, min_fraction=bad)
    with pytest.raises(ValueError, match="y_true"):
        est.predict_objects(X, offsets=off, y_true=np.zeros(6))  # one label per object, not per row
    with pytest.raises(ValueError, match="y_true"):
        est.predict_objects(X, objects=ids, rule="mean_spectrum", y_true=[0, 1])
