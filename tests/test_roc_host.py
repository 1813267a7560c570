"""The written specification of ocm.roc, on the CPU: the NumPy mirrors of the
kernels (u2_host, roc_counts_host, roc_points_host) against a brute-force count
in Python integers, against scikit-learn and against the recorded golden curves,
and the argument errors of the public calls, which are raised before anything
touches a device."""
import os

import numpy as np
import pytest
from sklearn.metrics import roc_auc_score

from ocm import roc


def _brute_u2(s, pos):
    """O(P·N) in Python integers; NaN rows left out; comparison by value."""
    s = [float(v) for v in np.asarray(s).astype(np.float64)]
    u2 = 0
    for i, a in enumerate(s):
        if not pos[i] or a != a:
            continue
        for j, b in enumerate(s):
            if pos[j] or b != b:
                continue
            u2 += 2 * (a > b) + (a == b)
    return u2


def _family(name, m, rng, dtype):
    if name == "normal":
        s = rng.standard_normal(m)
    elif name == "ties":
        s = np.round(rng.standard_normal(m) * 4) / 4
    elif name == "zeros":
        s = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), size=m)
    elif name == "special":
        s = rng.standard_normal(m)
        k = max(m // 6, 1)
        s[rng.integers(0, m, k)] = np.inf
        s[rng.integers(0, m, k)] = -np.inf
        s[rng.integers(0, m, k)] = -0.0
        s[rng.integers(0, m, k)] = 0.0
        s[rng.integers(0, m, k)] = np.finfo(dtype).tiny / 4  # a denormal
    else:
        raise KeyError(name)
    return s.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["normal", "ties", "zeros", "special"])
def test_u2_host_vs_brute_force(name, dtype):
    rng = np.random.default_rng(["normal", "ties", "zeros", "special"].index(name) * 2 + (dtype == np.float32))
    for m in (2, 3, 17, 150, 300):
        s = _family(name, m, rng, dtype)
        pos = rng.random(m) < 0.4
        pos[0], pos[1] = True, False
        assert roc.u2_host(s, pos) == _brute_u2(s, pos), (name, m)
    s = _family(name, 120, rng, dtype)
    pos = rng.random(120) < 0.5
    s[::7] = np.nan  # NaN rows count nowhere
    assert roc.u2_host(s, pos) == _brute_u2(s, pos)


def test_u2_host_returns_python_integers_and_extremes():
    pos = np.array([True, False])
    assert roc.u2_host(np.array([1.0, 0.0]), pos) == 2
    assert roc.u2_host(np.array([0.0, 1.0]), pos) == 0
    assert roc.u2_host(np.array([-0.0, 0.0]), pos) == 1  # −0.0 == +0.0: a tie
    assert type(roc.u2_host(np.array([1.0, 0.0]), pos)) is int
    with pytest.raises(ValueError):
        roc.u2_host(np.zeros(3), np.zeros(4, bool))


SKLEARN_SHAPES = [
    ("normal", 2, np.float64), ("normal", 101, np.float32), ("normal", 1000, np.float64),
    ("ties", 1000, np.float64), ("ties", 4097, np.float32), ("zeros", 513, np.float64),
    ("zeros", 2048, np.float32), ("normal", 20000, np.float32), ("ties", 30011, np.float64),
    ("normal", 70001, np.float64), ("ties", 70001, np.float32),
]


@pytest.mark.parametrize("name,m,dtype", SKLEARN_SHAPES, ids=[f"{n}-{m}-{np.dtype(d).name}" for n, m, d in
                                                              SKLEARN_SHAPES])
def test_auc_vs_sklearn(name, m, dtype):
    """|u2 / (2 P N) − roc_auc_score| ≤ m·2⁻⁵², the rounding bound of scikit-learn's
    m-term trapezoid sum (finite scores only: it refuses inf and NaN)."""
    rng = np.random.default_rng(m)
    s = _family(name, m, rng, dtype)
    pos = rng.random(m) < 0.3
    pos[0], pos[1] = True, False
    s = s + (0.5 * pos).astype(dtype) if name != "zeros" else s
    P, N = int(pos.sum()), int((~pos).sum())
    mine = roc.u2_host(s, pos) / (2 * P * N)
    ref = roc_auc_score(pos, s)
    diff = abs(mine - ref)
    print(f"{name} m={m}: |auc - sklearn| = {diff:.3e}, bound {m * 2.0 ** -52:.3e}")
    assert diff <= m * 2.0 ** -52


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "roc.npz"))


GOLDEN_NAMES = ["normal", "ties", "zeros", "f32"]


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_auc(golden, name):
    s, y = golden[f"{name}_s"], golden[f"{name}_y"]
    if name == "f32":
        assert s.dtype == np.float32 and set(np.unique(y)) == {0, 1}
    pos = y == 1
    P, N = int(pos.sum()), int((~pos).sum())
    assert abs(roc.u2_host(s, pos) / (2 * P * N) - float(golden[f"{name}_auc"])) <= s.size * 2.0 ** -52


def _curve_points(golden, name):
    y = golden[f"{name}_y"]
    P, N = int((y == 1).sum()), int((y != 1).sum())
    fp, tp = np.rint(golden[f"{name}_fpr"] * N).astype(np.int64), np.rint(golden[f"{name}_tpr"] * P).astype(np.int64)
    np.testing.assert_array_equal(fp / N, golden[f"{name}_fpr"])  # the integers are recovered exactly
    np.testing.assert_array_equal(tp / P, golden[f"{name}_tpr"])
    return set(zip(fp.tolist(), tp.tolist())), P, N


@pytest.mark.parametrize("n_points", [2, 9, 257])
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_roc_points_lie_on_the_golden_curve(golden, name, n_points):
    """Every (fp, tp) of roc_points' host mirror is a point of scikit-learn's
    full curve (drop_intermediate=False), compared as integers; the grid starts
    at (N, P) — the smallest negative as threshold — and ends at (0, 0)."""
    s, y = golden[f"{name}_s"], golden[f"{name}_y"]
    curve, P, N = _curve_points(golden, name)
    pts = roc.roc_points_host(s, y == 1, n_points=n_points)
    assert pts.thresholds[-1] == np.inf and (np.diff(pts.thresholds) > 0).all()
    assert 2 <= pts.thresholds.size <= n_points
    assert pts.tp.dtype == pts.fp.dtype == np.int64
    assert (int(pts.fp[-1]), int(pts.tp[-1])) == (0, 0) and int(pts.fp[0]) == N
    for fp, tp in zip(pts.fp.tolist(), pts.tp.tolist()):
        assert (fp, tp) in curve, (fp, tp)
    np.testing.assert_array_equal(pts.fpr, pts.fp / N)
    np.testing.assert_array_equal(pts.tpr, pts.tp / P)
    if name == "normal" and n_points == 257:  # distinct scores: an even FPR grid, one rank step apart at most
        assert np.abs(np.diff(pts.fpr[:-1]) + (N - 1) / 255 / N).max() <= 1.0 / N


def test_roc_counts_host_vs_brute_force():
    rng = np.random.default_rng(3)
    s = np.round(rng.standard_normal(200) * 2) / 2
    s[5], s[9] = np.nan, np.inf
    pos = rng.random(200) < 0.5
    thr = np.array([-np.inf, -1.0, -0.5, 0.0, 0.25, 3.0, np.inf])  # thresholds equal to data values: the ≥ edge
    cnt = roc.roc_counts_host(s, pos, thr)
    for k, t in enumerate(thr):
        assert cnt[k, 0] == sum(1 for v, p in zip(s, pos) if p and v >= t)
        assert cnt[k, 1] == sum(1 for v, p in zip(s, pos) if not p and v >= t)
    given = roc.roc_points_host(np.where(np.isnan(s), 0.0, s), pos, thresholds=thr)
    np.testing.assert_array_equal(given.thresholds, thr)


def test_positive_rows_of_one_label_or_a_list():
    y = np.array([0, 1, 2, 1, 3])
    np.testing.assert_array_equal(roc._positive_of(y, 1), [False, True, False, True, False])
    np.testing.assert_array_equal(roc._positive_of(y, [1]), [False, True, False, True, False])
    np.testing.assert_array_equal(roc._positive_of(y, np.array([1, 3])), [False, True, False, True, True])


def test_layout_reads_matrices_in_place():
    assert roc._layout((7,), (3,), 0) == (7, 1, 0, 3)
    assert roc._layout((7, 4), (4, 1), 0) == (7, 4, 1, 4)     # (m, C) row-major
    assert roc._layout((4, 7), (7, 1), 1) == (7, 4, 7, 1)     # (C, m)
    assert roc._layout((7, 4), (12, 2), 0) == (7, 4, 2, 12)   # a padded, strided view
    with pytest.raises(ValueError):
        roc._layout((2, 3, 4), (12, 4, 1), 0)
    with pytest.raises(ValueError):
        roc._layout((2, 3), (3, 1), 2)


def test_argument_errors_are_raised_before_the_device():
    s = np.linspace(0, 1, 10)
    y = np.arange(10) % 2 == 0
    with pytest.raises(ValueError, match="one class"):
        roc.auc(s, np.zeros(10, bool))
    with pytest.raises(ValueError, match="one class"):
        roc.auc(s, np.ones(10, bool))
    with pytest.raises(ValueError, match="one class"):
        roc.roc_points(s, np.ones(10, bool))
    bad = s.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        roc.auc(bad, y)
    with pytest.raises(ValueError, match="NaN"):
        roc.roc_points(bad, y)
    with pytest.raises(ValueError, match="shape"):
        roc.auc(s, y[:9])
    with pytest.raises(ValueError, match="shape"):
        roc.auc(np.zeros((10, 3)), y[:3], axis=0)
    with pytest.raises(ValueError, match="1-D or 2-D"):
        roc.auc(np.zeros((2, 5, 2)), y)
    with pytest.raises(ValueError, match="4096"):
        roc.roc_points(s, y, thresholds=np.arange(4097.0))
    with pytest.raises(ValueError, match="4096"):
        roc.roc_points(s, y, n_points=4097)
    with pytest.raises(ValueError, match="ascending"):
        roc.roc_points(s, y, thresholds=[1.0, 0.0])
    with pytest.raises(ValueError, match="one class"):
        roc.roc_points_host(s, np.zeros(10, bool))
    assert roc.MAX_THRESHOLDS == 4096
