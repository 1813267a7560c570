"""CPU-side checks of the multi-class SIMCA interface: the C ABI entry and its
binding, ``SIMCA.classify`` / ``model_distance`` argument errors (raised before
any device work), the assignment rule ``ocm.multiclass.assign`` with its count
tables, and Wold's model distance against a direct float64 evaluation."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ocm.h")


def test_header_and_binding_declare_score_multi():
    from ocm import _lib

    txt = open(HEADER).read()
    m = re.search(r"^int\s+ocm_score_multi_f32\s*\(([^;]*)\)\s*;", txt, re.M)
    assert m, "include/ocm.h does not declare ocm_score_multi_f32"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 23
    assert args[0] == "ocm_ctx* ctx" and args[-1] == "void* stream" and args[9] == "const int32_t* koff"
    res, argtypes = _lib.SIGNATURES["ocm_score_multi_f32"]
    assert res is _lib.c_i32 and len(argtypes) == 23
    assert int(re.search(r"#define OCM_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 12


def test_source_is_listed_for_the_build_id():
    mk = open(os.path.join(REPO, "ocm-vae-simca_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", mk, re.M).group(1).split()
    assert srcs[-1] == "ocm_multi.hip" and srcs.count("ocm_multi.hip") == 1


def _stub(classes, p=8):
    """A fitted-state stub: no device, no arrays (the argument checks come first)."""
    from utils import SIMCA

    est = SIMCA(n_components=2, model_class=list(classes), verbose=False)
    est._model = {c: {"T2_limit": 1.0, "Q_limit": 1.0, "D_limit": 1.0} for c in classes}
    est._fits = {c: object() for c in classes}
    est._out_dtype = np.float32
    est._sharded = False
    est.n_features_in_ = p
    return est


def test_classify_argument_errors():
    from sklearn.exceptions import NotFittedError
    from utils import SIMCA

    X = np.zeros((6, 8), dtype=np.float32)
    assert callable(SIMCA.classify) and callable(SIMCA.model_distance)
    with pytest.raises(NotFittedError):
        SIMCA(n_components=2, verbose=False).classify(X)
    with pytest.raises(NotFittedError):
        SIMCA(n_components=2, verbose=False).model_distance(X, np.zeros(6, dtype=np.int64))
    est = _stub([0, 1, 2])
    with pytest.raises(ValueError, match="columns"):
        est.classify(np.zeros((6, 7), dtype=np.float32))
    with pytest.raises(ValueError, match="columns"):
        est.classify(np.zeros(8, dtype=np.float32))
    with pytest.raises(ValueError, match="rows"):
        est.classify(X, y_true=np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match="rows"):
        est.model_distance(X, np.zeros((6, 1), dtype=np.int64))
    with pytest.raises(ValueError, match="route"):
        est.classify(X, route="quick")
    with pytest.raises(ValueError, match="255"):
        _stub(range(256)).classify(X)
    assert est.metrics == {} and "_multi_stack" not in est.__dict__


def test_assign_hand_table():
    from ocm.multiclass import assign, confusion_from_counts, count_tables

    nan = np.nan
    ratio = np.array([[0.50, 0.50, 2.00],   # a tie between two accepting classes: the lowest index
                      [1.50, 1.20, 3.00],   # nobody accepts; nearest = 1
                      [0.90, 0.30, 0.60],   # all accept; the smallest ratio
                      [nan, 0.80, 0.70],    # a NaN ratio never wins
                      [nan, nan, nan],      # all NaN: nearest 0, index −1
                      [0.20, 1.10, 0.20],   # a tie across a rejecting class
                      [2.00, 2.00, 2.00],   # a tie among rejecting classes
                      [0.95, 0.40, nan]])
    accept = (ratio < 1.0).astype(np.float64)
    index, nearest, n_accept = assign(ratio, accept)
    assert index.dtype == nearest.dtype == n_accept.dtype == np.int64
    assert index.tolist() == [0, -1, 1, 2, -1, 0, -1, 1]
    assert nearest.tolist() == [0, 1, 1, 2, 0, 0, 0, 1]
    assert n_accept.tolist() == [2, 0, 3, 2, 0, 2, 0, 2]
    # the assignment follows `accept`, not ratio < 1: an accepting class wins over a nearer rejecting one
    i2, n2, _ = assign(np.array([[0.4, 0.6]]), np.array([[0, 1]]))
    assert i2.tolist() == [1] and n2.tolist() == [0]

    y = np.array([0, 1, 1, 2, 7, 3, 0, -1])  # 7, 3 and −1 lie outside the classes: the row "other"
    table, acc, hist = count_tables(y, index, accept)
    want_table = np.zeros((4, 4), dtype=np.int64)
    for t, c in [(0, 0), (1, 3), (1, 1), (2, 2), (3, 3), (3, 0), (0, 3), (3, 1)]:
        want_table[t, c] += 1
    want_acc = np.array([[1, 1, 0],    # true 0: rows 0, 6
                         [1, 1, 1],    # true 1: rows 1, 2
                         [0, 1, 1],    # true 2: row 3
                         [2, 1, 1]])   # other: rows 4, 5, 7
    want_hist = np.array([[1, 0, 1, 0],
                          [1, 0, 0, 1],
                          [0, 0, 1, 0],
                          [1, 0, 2, 0]])
    assert table.tolist() == want_table.tolist()
    assert acc.tolist() == want_acc.tolist()
    assert hist.tolist() == want_hist.tolist()
    for blk in (table, acc, hist):
        assert blk.dtype == np.int64
    # TP / TN / FP / FN of each class column, as utils/SIMCA.py:238-245 counts them
    yc = np.where((y < 0) | (y >= 3), 3, y)
    for i in range(3):
        a, pos = accept[:, i] == 1, yc == i
        want = (np.sum(a & pos), np.sum(~a & ~pos), np.sum(a & ~pos), np.sum(~a & pos))
        assert tuple(int(v) for v in confusion_from_counts(table, acc, i)) == tuple(int(v) for v in want)


def test_wold_distance_against_direct_evaluation():
    from oracle import simca_oracle as O
    from ocm.multiclass import wold_distance
    from test_plsda_host import plsda_data

    C, p, ks = 3, 40, [4, 3, 5]
    X, y, _, _ = plsda_data(360, 0, p, C, 4.0, 11)
    X64 = X.astype(np.float64)
    orc = O.OracleSIMCA(n_components=list(ks), type="alt", precision="exact").fit(X64, y)
    Q = np.stack([O.project_scores(X64, orc._model[c]["P_pred"], orc._model[c]["mean_pred"],
                                   orc._model[c]["invcovT"])[2] for c in orc.model_class], axis=1)
    S = np.array([[Q[y == r, q].sum() for q in range(C)] for r in range(C)])
    n = np.bincount(y, minlength=C)
    D = wold_distance(S, n, ks, p)
    # the definition, term by term
    s2 = np.zeros((C, C))
    for r in range(C):
        for q in range(C):
            res = Q[y == r, q]
            s2[r, q] = res.sum() / ((n[q] - ks[q] - 1) * (p - ks[q])) if r == q else res.sum() / (n[r] * (p - ks[q]))
    for a in range(C):
        for b in range(C):
            want = 1.0 if a == b else np.sqrt((s2[a, b] + s2[b, a]) / (s2[a, a] + s2[b, b]))
            assert D[a, b] == pytest.approx(want, rel=1e-13)
    assert D.dtype == np.float64 and np.all(D[~np.eye(C, dtype=bool)] > 1.0)  # separated classes
