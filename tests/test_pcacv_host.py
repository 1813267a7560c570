"""Host side of the PCA cross-validation (ocm/pcacv.py): the closed form of the
element-wise PRESS against its definition and against the Gram identity, the
preconditions of the GPU fixtures, the selection rules, fold construction,
argument errors and the ABI.  No device."""
import os
import re
import warnings

import numpy as np
import pytest

import pcacv_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ocm.h")
LIB = os.path.join(REPO, "ocm-vae-simca_amd", "ocm", "libocm.so")
SEEDS = range(5)


# ------------------------------------------------------------- the mathematics
@pytest.mark.parametrize("n,p,rank", O.SHAPES)
def test_closed_form_is_the_variable_deleted_least_squares(n, p, rank):
    """e_j = r_j/(1 − h_j) is exactly the error of predicting variable j from the
    other p − 1 through the loadings (Sherman–Morrison), and the row-wise sums
    are the diagonal of (I − Π)S(I − Π): three routes, rtol 1e-12."""
    for seed in SEEDS:
        X = O.lowrank(n, p, rank, 100 + seed)
        K = rank + O.EXTRA
        folds = O.kfold(n, O.NFOLDS)
        closed, naive, _, models, _ = O.full_cv(X, K, folds)
        brute = O.full_cv(X, K, folds, fn=O.press_brute)[0]
        np.testing.assert_allclose(closed, brute, rtol=1e-12)
        pg, ng = np.zeros(K + 1), np.zeros(K + 1)
        for f, (mu, P) in zip(folds, models):
            a, b = O.press_gram(X[f], P, mu)
            pg += a
            ng += b
        np.testing.assert_allclose(closed, pg, rtol=1e-12)
        np.testing.assert_allclose(naive, ng, rtol=1e-12)


@pytest.mark.parametrize("n,p,rank", O.SHAPES)
def test_fixture_preconditions(n, p, rank):
    """What the GPU tests take for granted about their inputs: PRESS has its
    minimum at the true rank with a margin of at least 2 % to the next
    component, no variable is near-degenerate, and the row-wise curve only ends
    at K.  Both the float64 arrays and their float32 casts."""
    for seed in SEEDS:
        for dtype in ("float64", "float32"):
            X, K, folds, (press, naive, pf, _, hmax) = O.fixture(n, p, rank, seed, dtype)
            assert X.dtype == np.dtype(dtype) and K == rank + O.EXTRA and len(folds) == O.NFOLDS
            assert int(np.argmin(press)) == rank
            assert press[rank + 1] / press[rank] >= 1.02
            assert hmax <= 0.9
            assert int(np.argmin(naive)) == K
            assert pf.shape == (O.NFOLDS, K + 1)
            if dtype == "float32":   # float32's own worst-case error is inside the GPU tolerance
                _, _, _, models, _ = O.fixture(n, p, rank, seed, dtype)[3]
                for f, (mu, P) in zip(folds, models):
                    assert O.f32_error_bound(X[f], P, mu) <= 1e-4


def test_degenerate_rule_of_the_oracle():
    """A loading row equal to e_j makes variable j degenerate from k = 1 on:
    weight 0, counted once, and the sum equals the one with j left out by hand."""
    rng = np.random.default_rng(3)
    p, K, j = 12, 3, 5
    Q = np.linalg.qr(rng.standard_normal((p - 1, K - 1)))[0].T
    P = np.zeros((K, p))
    P[0, j] = 1.0
    P[1:, np.arange(p) != j] = Q
    X = rng.standard_normal((30, p))
    mu = X.mean(axis=0)
    press, naive, nd = O.press_closed(X, P, mu)
    assert nd.tolist() == [0, 1, 1, 1]
    np.testing.assert_allclose(press, O.press_closed(X, P, mu, exclude=j)[0], rtol=1e-14)
    assert np.all(naive[1:] <= naive[:-1])


def test_kernel_cases_are_well_conditioned_in_float32():
    """The kernel-level inputs of the GPU tests: the seed search finds a case whose
    float32 worst-case bound is at most half the tolerance, and the near-degenerate
    loading it steps over (p = 2: a variable that is the component) is outside it."""
    for m, p, K in ((1, 2, 1), (773, 2, 1), (773, 8, 6), (257, 33, 6), (40, 580, 64)):
        X, mu, P = O.kernel_case(m, p, K)
        assert X.dtype == np.float32 and X.shape == (m, p) and P.shape == (K, p)
        assert O.f32_error_bound(X, P, mu) <= 0.5e-4
        np.testing.assert_allclose(P @ P.T, np.eye(K), atol=1e-12)
    P = np.array([[0.006, np.sqrt(1 - 0.006 ** 2)]])
    X = np.array([[0.7, -0.24]], dtype=np.float32)
    assert O.f32_error_bound(X, P, np.array([0.92, 1.13])) > 1e-4


# ------------------------------------------------------------------ selection
def test_select_rules():
    from ocm.pcacv import select_components

    curve = [10.0, 6.0, 3.0, 3.2, 2.5, 2.9]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert select_components(curve, "min") == 4
        assert select_components(curve, "first_min") == 2
        assert select_components(curve, "wold") == 2               # 3.2/3.0 > 0.95
        assert select_components(curve, "wold", r_threshold=0.55) == 0  # 6/10 > 0.55
        assert select_components([5.0, 5.0, 1.0], "first_min") == 0     # a tie counts as a rise
        assert select_components([1.0, 2.0], "min") == 0


def test_select_warns_when_nothing_qualifies():
    from ocm.pcacv import PcaCvResult, select_components

    falling = np.array([16.0, 8.0, 4.0, 2.0, 1.0])
    for rule in ("min", "first_min", "wold"):
        with pytest.warns(RuntimeWarning, match="max_components"):
            assert select_components(falling, rule, r_threshold=0.6) == 4
    res = PcaCvResult(press=falling, naive=falling, ndegen=np.zeros(5, np.int64), press_folds=falling[None],
                      rmsecv=np.sqrt(falling), q2=1 - falling / falling[0], n=1, p=1)
    with pytest.warns(RuntimeWarning):
        assert res.select("wold", r_threshold=0.6) == 4
    with pytest.raises(ValueError):
        select_components(falling, "median")
    with pytest.raises(ValueError):
        select_components([1.0], "min")


# ---------------------------------------------------------------------- folds
class _Shape:
    def __init__(self, n, p):
        self.shape = (n, p)


def test_folds_from_an_int_are_kfold_over_the_rows():
    from sklearn.model_selection import KFold

    from ocm.pcacv import make_folds

    X = _Shape(23, 4)
    folds = make_folds(X, 4)
    assert [f.tolist() for f in folds] == [f.tolist() for f in O.kfold(23, 4)]
    rows = np.array([20, 3, 5, 7, 11, 13, 2, 17, 19])
    folds = make_folds(X, 3, rows=rows)
    want = [rows[held] for _, held in KFold(3).split(rows)]
    assert [f.tolist() for f in folds] == [w.tolist() for w in want]
    mask = np.zeros(23, dtype=bool)
    mask[rows] = True
    assert np.concatenate(make_folds(X, 3, rows=mask)).tolist() == sorted(rows.tolist())
    a = make_folds(X, 4, shuffle=True, random_state=7)
    b = make_folds(X, 4, shuffle=True, random_state=7)
    assert [f.tolist() for f in a] == [f.tolist() for f in b]
    assert sorted(np.concatenate(a).tolist()) == list(range(23))
    assert [f.tolist() for f in a] != [f.tolist() for f in make_folds(X, 4)]


def test_folds_from_the_splitters_are_their_target_folds():
    from ocm.objectcv import ObjectKFoldWithExternalVal
    from ocm.pcacv import make_folds
    from utils.CVSIMCA import ClasswiseKFoldWithExternalVal

    n = 40
    y = np.array([0] * 26 + [1] * 14)
    X = _Shape(n, 5)
    cw = ClasswiseKFoldWithExternalVal(n_splits=4, cls_label=0)
    folds = make_folds(X, cw, y=y)
    target = np.flatnonzero(y == 0)
    want = [target[held] for _, held in cw.kf.split(target)]
    assert [f.tolist() for f in folds] == [w.tolist() for w in want]
    assert np.concatenate(folds).max() < 26          # no other-class row is ever held out
    objects = np.repeat(np.arange(10), 4)            # 10 objects of 4 rows; objects 0..6 are class 0
    y2 = np.array([0] * 28 + [1] * 12)
    ob = ObjectKFoldWithExternalVal(n_splits=3, objects=objects, cls_label=0)
    folds = make_folds(X, ob, y=y2)
    assert [f.tolist() for f in folds] == [f.tolist() for f in ob.target_folds(X, y2)]
    held = [set(objects[f].tolist()) for f in folds]
    assert sum(len(h) for h in held) == 7 and len(set.union(*held)) == 7   # every object in exactly one fold
    for f, h in zip(folds, held):
        assert sorted(f.tolist()) == np.flatnonzero(np.isin(objects, list(h))).tolist()  # whole objects
    with pytest.raises(ValueError, match="rows"):
        make_folds(X, cw, rows=np.arange(5), y=y)


def test_explicit_folds():
    from ocm.pcacv import make_folds

    X = _Shape(10, 3)
    folds = make_folds(X, folds=[[0, 1, 2], np.array([5, 4]), [9]])
    assert [f.tolist() for f in folds] == [[0, 1, 2], [5, 4], [9]] and all(f.dtype == np.int64 for f in folds)
    for bad, msg in (([[0, 1]], "two"), ([[0, 1], [1, 2]], "disjoint"), ([[0], [10]], "outside"),
                     ([[0], []], "empty")):
        with pytest.raises(ValueError, match=msg):
            make_folds(X, folds=bad)
    with pytest.raises(ValueError, match="not both"):
        make_folds(X, folds=[[0], [1]], rows=[0, 1])


# ------------------------------------------------------------ argument errors
def test_argument_errors_come_before_any_device_work():
    from ocm.pcacv import PcaCvResult, make_folds, pca_press, press_variables

    X = np.zeros((20, 6), dtype=np.float32)
    for K in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="max_components"):
            pca_press(X, K)
    with pytest.raises(ValueError, match="2 columns"):
        pca_press(np.zeros((20, 1), dtype=np.float32), 1)
    with pytest.raises(ValueError, match="shape"):
        pca_press(np.zeros(20, dtype=np.float32), 1)
    with pytest.raises(ValueError, match="single-process"):
        pca_press(X, 2, group=object())
    with pytest.raises(ValueError, match="n_components=7"):   # check_components: K > min(n_train, p)
        pca_press(np.zeros((20, 8), dtype=np.float32), 7, folds=[np.arange(14), np.arange(14, 20)])
    for cv in (1, 2.5, "5", True):
        with pytest.raises(ValueError, match="cv"):
            make_folds(X, cv)
    with pytest.raises(ValueError):      # more folds than rows
        make_folds(X, 5, rows=[1, 2, 3])
    with pytest.raises(ValueError, match="twice"):
        make_folds(X, 2, rows=[1, 2, 2, 3])
    with pytest.raises(ValueError, match="outside"):
        make_folds(X, 2, rows=[1, 2, 20])
    z = np.zeros(4)
    res = PcaCvResult(press=z, naive=z, ndegen=z, press_folds=z[None], rmsecv=z, q2=z, n=20, p=6)
    for k in (-1, 4, 1.0):
        with pytest.raises(ValueError, match="press_variables: k"):
            press_variables(X, res, k)
    with pytest.raises(ValueError, match="columns"):
        press_variables(np.zeros((20, 5), dtype=np.float32), res, 1)


def test_simca_press_argument_errors():
    from utils.SIMCA import SIMCA

    X = np.zeros((12, 5), dtype=np.float32)
    y = np.array([0] * 6 + [1] * 6)
    with pytest.raises(ValueError, match="name the class"):
        SIMCA(verbose=False).press(X, y)
    with pytest.raises(ValueError, match="no row"):
        SIMCA(verbose=False).press(X, y, cls=7)
    with pytest.raises(ValueError, match="cls= needs y"):
        SIMCA(verbose=False).press(X, cls=0)
    with pytest.raises(ValueError, match="y has shape"):
        SIMCA(verbose=False).press(X, y[:5], cls=0)
    with pytest.raises(ValueError, match="max_components"):
        SIMCA(verbose=False, maxPC=0).press(X)


# ------------------------------------------------------------------------ ABI
def test_header_declares_the_press_entries_and_the_degenerate_rule():
    txt = open(HEADER).read()
    for name in ("ocm_press_f32", "ocm_press_f64"):
        assert re.search(r"^int\s+%s\s*\(" % name, txt, re.M), f"include/ocm.h does not declare {name}"
    assert "1e-8" in txt and "ndegen_out" in txt
    assert re.search(r"#define OCM_ABI_VERSION 12\b", txt)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libocm.so not built")
def test_binding_matches_the_header():
    from ocm import _lib

    txt = open(HEADER).read()
    syms = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ocm_\w+)\s*\(", txt, re.M))
    assert set(_lib.SIGNATURES) == syms
    for name in ("ocm_press_f32", "ocm_press_f64"):
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, txt, re.M | re.S).group(1)
        assert len(args) == len(decl.split(",")) == 13
    lib = _lib.load()
    assert lib.ocm_abi_version() == _lib.ABI_VERSION == 12
    assert hasattr(lib, "ocm_press_f32") and hasattr(lib, "ocm_press_f64")
