"""ocm_auc, ocm_sort_f and ocm_roc_counts on the GPU against the NumPy mirrors of
ocm.roc, by exact integer or byte equality (no tolerance anywhere but in the last
test), and the layers above them: SIMCA.roc_auc and cross_validate_auc_grid.

Kernel boundaries reached (csrc/ocm_roc.hip), with T = ocm_roc_tile_keys():
m = 0, 1, 2; one wave and its neighbours (63, 64, 65); one workgroup of the
row-strided kernels and its neighbours (255, 256, 257); one sort tile and its
neighbours (T − 1, T, T + 1), several tiles (2T + 1, 5T + 3: the scan's four
thread groups get 1–2 tiles each, the last one partly filled); one, three and
135 columns in the (m, C), (C, m) and padded layouts; every pass skipped, one
pass, the top pass with both signs, all passes; the sorted class being the
positives and the negatives.  The search keeps the last key of each bucket of
bs = ⌈n_s / SPLIT⌉ sorted keys in LDS (SPLIT = 4096 float64 / 8192 float32 keys):
n_s = SPLIT (bs = 1, every bucket full), SPLIT + 1 and 2·SPLIT (bs = 2, the last
bucket holding one key, then full) and 3·SPLIT + 1 (bs = 4, the last bucket
partly filled, fewer buckets than SPLIT), each with and without runs of equal
keys and with either class sorted.  ocm_sort_f also at 9T + 5, where every later
pass scans more than one tile per thread group on the ping-pong buffers.
"""
import contextlib
import io

import numpy as np
import pytest

from conftest import gpu_available
from test_objectcv_host import object_data
from test_plsda_host import plsda_data

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _T():
    from ocm import roc

    return roc.tile_keys()


def _kernel_auc(t, pos, axis=0):
    """ocm_auc on a device tensor (no Python-level raise) → (u2, P, N, nnan)."""
    from ocm import roc

    m, ncol, cs, rs = roc._layout(t.shape, t.stride(), axis)
    return roc._call_auc(t, m, ncol, cs, rs, _dev(pos.astype(np.uint8)))


def _mirror(S, pos):
    """u2_host of every column of the host (m, C) matrix."""
    from ocm import roc

    return np.array([roc.u2_host(S[:, c], pos) for c in range(S.shape[1])], dtype=np.int64)


def _uint(dtype):
    return np.uint32 if dtype == np.float32 else np.uint64


def family(name, m, C, dtype, seed):
    """(m, C) scores of one value family."""
    rng = np.random.default_rng(seed)
    u = _uint(dtype)
    nb = 8 * np.dtype(dtype).itemsize
    if name == "equal":
        return np.full((m, C), 1.25, dtype)
    if name == "low_byte":  # keys that differ in the lowest byte only
        base = np.array(1.5, dtype).view(u)
        return (base + rng.integers(0, 256, (m, C)).astype(u)).view(dtype)
    if name == "top_byte":  # keys that differ in the top byte only, both signs (finite: exponent < all ones)
        top = rng.integers(0, 0x7F, (m, C)).astype(u) | (rng.integers(0, 2, (m, C)).astype(u) << u(7))
        return ((top << u(nb - 8)) | u(0x1234)).view(dtype)
    if name == "normal":
        return rng.standard_normal((m, C)).astype(dtype)
    if name == "quarter":  # heavy ties
        return (np.round(rng.standard_normal((m, C)) * 4) / 4).astype(dtype)
    if name == "special":
        s = rng.standard_normal((m, C)).astype(dtype)
        if m == 0:
            return s
        k = max(m // 5, 1)
        for v in (0.0, -0.0, np.inf, -np.inf, np.finfo(dtype).tiny / 4, -np.finfo(dtype).tiny / 8):
            s[rng.integers(0, m, k), rng.integers(0, C, k)] = v
        return s
    raise KeyError(name)


FAMILIES = ["equal", "low_byte", "top_byte", "normal", "quarter", "special"]


def _mask(m, frac, seed):
    pos = np.random.default_rng(seed).random(m) < frac
    if m >= 2:
        pos[0], pos[1] = True, False
    return pos


# ------------------------------------------------------------------ ocm_auc

def _sizes():
    T = 2048  # ocm_roc_tile_keys(); checked in the test (a collection-time device call is not wanted)
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("m", _sizes())
def test_auc_sizes(m, dtype):
    T = _T()
    assert T == 2048 and set(_sizes()) >= {T - 1, T, T + 1, 2 * T + 1, 5 * T + 3}
    S = family("quarter" if m % 2 else "normal", m, 3, dtype, seed=m)
    for frac in (0.3, 0.7):  # the positives sorted, then the negatives
        pos = _mask(m, frac, seed=m + 1)
        u2, P, N, nnan = _kernel_auc(_dev(S), pos)
        assert (P, N) == (int(pos.sum()), int(m - pos.sum()))
        np.testing.assert_array_equal(u2, _mirror(S, pos))
        assert not nnan.any()


def _split(dtype):
    """Bucket splitters the search holds in LDS: 32 KiB of keys (include/ocm.h, ocm_auc's workspace)."""
    return 32768 // np.dtype(dtype).itemsize


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mult,extra", [(1, 0), (1, 1), (2, 0), (3, 1)], ids=["S", "S+1", "2S", "3S+1"])
def test_auc_search_buckets(mult, extra, dtype):
    """More sorted keys than splitters, so a bucket holds several keys: the offset
    of a bucket, the partly filled last one and the clamp at n_s, for the first
    search alone (distinct scores) and with the second one (runs of equal keys,
    ±0, ±inf), with the positives sorted and with the negatives sorted."""
    from ocm import roc

    ns = mult * _split(dtype) + extra
    m = 2 * ns + 777
    rng = np.random.default_rng(ns)
    for name in ("normal", "quarter", "special"):
        S = family(name, m, 2, dtype, seed=ns + len(name))
        small = np.zeros(m, bool)
        small[rng.permutation(m)[:ns]] = True
        for pos in (small, ~small):  # the positives sorted, then the negatives
            u2, P, N, nnan = _kernel_auc(_dev(S), pos)
            assert min(P, N) == ns and P + N == m and not nnan.any()
            np.testing.assert_array_equal(u2, _mirror(S, pos), err_msg=f"{name} P={P}")
        assert roc.last_passes() >= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", FAMILIES)
def test_auc_value_families(name, dtype):
    from ocm import roc

    m = 2 * _T() + 77
    S = family(name, m, 3, dtype, seed=len(name))
    pos = _mask(m, 0.35, seed=9)
    u2, P, N, _ = _kernel_auc(_dev(S), pos)
    np.testing.assert_array_equal(u2, _mirror(S, pos))
    passes = roc.last_passes()
    nd = np.dtype(dtype).itemsize
    if name == "equal":
        assert passes == 0 and (u2 == P * N).all()
    elif name == "low_byte":
        assert passes == 1
    elif name == "top_byte":  # a negative value's key is the complement: its low bytes differ from a positive's
        assert 1 <= passes <= nd
    elif name == "normal":
        assert 2 <= passes <= nd
    res = roc.auc(_dev(S), pos)
    np.testing.assert_array_equal(res.u2, u2)
    np.testing.assert_array_equal(res.auc, [int(v) / (2 * P * N) for v in u2])
    low = roc.auc(_dev(S), pos, lower_is_positive=True)
    np.testing.assert_array_equal(low.u2, 2 * P * N - u2)


@pytest.mark.parametrize("ncol", [1, 3, 135])
@pytest.mark.parametrize("layout", ["mC", "Cm", "padded"])
def test_auc_layouts(layout, ncol):
    """One host matrix behind three device layouts: the same u2, no copy."""
    m = 2 * _T() + 1
    for dtype in DTYPES:
        S = family("quarter", m, ncol, dtype, seed=ncol)
        pos = _mask(m, 0.4, seed=ncol + 1)
        want = _mirror(S, pos)
        if layout == "mC":
            t, axis = _dev(S), 0
            assert t.stride() == (ncol, 1)
        elif layout == "Cm":
            t, axis = _dev(S.T.copy()), 1
            assert t.shape == (ncol, m)
        else:  # every second column of a wider matrix whose rows are padded
            wide = np.full((m, 2 * ncol + 5), np.nan, dtype)
            wide[:, 1:2 * ncol + 1:2] = S
            t, axis = _dev(wide)[:, 1:2 * ncol + 1:2], 0
            assert t.stride() == (2 * ncol + 5, 2) and not t.is_contiguous()
        u2, _, _, nnan = _kernel_auc(t, pos, axis)
        np.testing.assert_array_equal(u2, want)
        assert not nnan.any()
    # a 1-D strided view
    from ocm import roc

    v = _dev(np.stack([S[:, 0], S[:, 0] + 1], axis=1))[:, 0]
    assert v.stride() == (2,) and roc.auc(v, pos).u2[0] == want[0]
    # a mask that starts off an 8-byte boundary (the flags are counted eight per load in between)
    for shift in (1, 5):
        p8 = _dev(np.concatenate([np.ones(shift, np.uint8), pos.astype(np.uint8)]))[shift:]
        assert p8.data_ptr() % 8 == shift
        u2, P, N, _ = roc._call_auc(t, *roc._layout(t.shape, t.stride(), axis), p8)
        assert (P, N) == (int(pos.sum()), int(m - pos.sum()))
        np.testing.assert_array_equal(u2, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_auc_class_balance(dtype):
    from ocm import roc

    m = 3 * _T() + 5
    S = family("quarter", m, 3, dtype, seed=4)
    one = np.zeros(m, bool)
    one[m // 2] = True
    masks = {"P=1": one, "N=1": ~one, "1%": _mask(m, 0.01, 5), "99%": _mask(m, 0.99, 6)}
    for name, pos in masks.items():
        u2, P, N, _ = _kernel_auc(_dev(S), pos)
        assert P == int(pos.sum()) and N == m - P, name
        np.testing.assert_array_equal(u2, _mirror(S, pos), err_msg=name)
    for pos in (np.zeros(m, bool), np.ones(m, bool)):  # P = 0, N = 0: the kernel succeeds with u2 = 0
        u2, P, N, nnan = _kernel_auc(_dev(S), pos)
        assert (P, N) == (int(pos.sum()), int(m - pos.sum())) and not u2.any() and not nnan.any()
        import torch

        with pytest.raises(ValueError, match="one class"):
            roc.auc(_dev(S), torch.from_numpy(pos).to("cuda:0"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_auc_nan_rows(dtype):
    from ocm import roc

    m = 2 * _T() + 9
    S = family("normal", m, 3, dtype, seed=12)
    rng = np.random.default_rng(13)
    S[rng.integers(0, m, 40), 0] = np.nan
    S[rng.integers(0, m, 7), 2] = -np.nan  # the sign bit set
    for frac in (0.3, 0.7):
        pos = _mask(m, frac, seed=14)
        u2, _, _, nnan = _kernel_auc(_dev(S), pos)
        np.testing.assert_array_equal(nnan, np.isnan(S).sum(0))
        assert nnan[0] > 0 and nnan[1] == 0 and nnan[2] > 0
        np.testing.assert_array_equal(u2, _mirror(S, pos))  # the mirror leaves NaN rows out
    with pytest.raises(ValueError, match="NaN"):
        roc.auc(_dev(S), pos)
    # NaN in one class only, and a degenerate mask still counts them
    _, _, _, nnan = _kernel_auc(_dev(S), np.zeros(m, bool))
    np.testing.assert_array_equal(nnan, np.isnan(S).sum(0))


# ------------------------------------------------------------------ ocm_sort_f

def _okey(a):
    """The order-preserving key of ocm_select.hip on the host."""
    u = a.view(_uint(a.dtype))
    top = u.dtype.type(1) << u.dtype.type(8 * u.itemsize - 1)
    return np.where(u & top, ~u, u | top)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", FAMILIES)
def test_sort_f(name, dtype):
    from ocm import roc

    T = _T()
    for m in (0, 1, 65, T, 2 * T + 1, 9 * T + 5):
        S = family(name, m, 3, dtype, seed=m + 3)
        if name == "special" and m > 10:
            S[3, 0] = S[7, 0] = np.nan
            S[5, 1] = -np.nan
        out = roc.sort_values(_dev(S), axis=0)
        assert out.shape == (m, 3)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got, np.sort(S, axis=0))  # as values (NaN == NaN here), NaNs last
        for c in range(3):  # as bits: the key order, so −0.0 before +0.0; the multiset of bit patterns
            keep = ~np.isnan(S[:, c])
            want = np.sort(_okey(S[keep, c]))
            np.testing.assert_array_equal(_okey(np.ascontiguousarray(got[:keep.sum(), c])), want)
            assert np.isnan(got[keep.sum():, c]).all()
    # the (C, m) layout and a 1-D input; NumPy in, NumPy out
    S = family("normal", T + 5, 3, dtype, seed=1)
    np.testing.assert_array_equal(roc.sort_values(_dev(S.T.copy()), axis=1).cpu().numpy(), np.sort(S.T, axis=1))
    host = roc.sort_values(S[:, 0].copy())
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, np.sort(S[:, 0]))
    z = roc.sort_values(np.array([0.0, -0.0, 0.0, -0.0, -1.0], dtype))
    np.testing.assert_array_equal(np.signbit(z), [True, True, True, False, False])


# ------------------------------------------------------------------ ocm_roc_counts

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", [1, 2, 257, 4096])
def test_roc_counts(K, dtype):
    import torch
    from ocm import roc

    m, C = 3000, 3
    S = family("quarter", m, C, dtype, seed=K)
    S[5, 0] = np.nan
    S[6, 1], S[7, 1] = np.inf, -np.inf
    pos = _mask(m, 0.4, seed=K + 1)
    rng = np.random.default_rng(K)
    thr = np.empty((C, K))
    for c in range(C):  # half of them data values (the ≥ edge), ascending, duplicates allowed
        vals = S[~np.isnan(S[:, c]), c].astype(np.float64)
        thr[c] = np.sort(np.concatenate([rng.choice(vals, K // 2), rng.standard_normal(K - K // 2)]))
    cnt = roc.roc_counts(_dev(S), _dev(pos.astype(np.uint8)), _dev(thr)).cpu().numpy()
    for c in range(C):
        np.testing.assert_array_equal(cnt[c], roc.roc_counts_host(S[:, c], pos, thr[c]))
    cnt_t = roc.roc_counts(_dev(S.T.copy()), _dev(pos.astype(np.uint8)), _dev(thr), axis=1).cpu().numpy()
    np.testing.assert_array_equal(cnt_t, cnt)
    with pytest.raises(ValueError, match="4096"):
        roc.roc_counts(_dev(S), _dev(pos.astype(np.uint8)), torch.zeros((C, 4097), dtype=torch.float64, device="cuda:0"))


def test_roc_points_device_vs_host():
    from ocm import roc

    m = 2 * _T() + 11
    for dtype in DTYPES:
        S = family("quarter", m, 2, dtype, seed=21) + family("normal", m, 2, dtype, seed=22) * dtype(0.01)
        pos = _mask(m, 0.3, seed=23)
        two = roc.roc_points(_dev(S), pos, n_points=33)
        for c in range(2):
            ref = roc.roc_points_host(S[:, c], pos, n_points=33)
            one = roc.roc_points(_dev(S)[:, c], pos, n_points=33)
            for f in ("thresholds", "tp", "fp", "tpr", "fpr"):
                np.testing.assert_array_equal(getattr(one, f), getattr(ref, f), err_msg=f)
                np.testing.assert_array_equal(getattr(two, f)[c][:ref.tp.size], getattr(ref, f), err_msg=f)
        given = roc.roc_points(S[:, 0], pos, thresholds=[-1.0, 0.0, 0.25])
        np.testing.assert_array_equal(np.stack([given.tp, given.fp], 1),
                                      roc.roc_counts_host(S[:, 0], pos, [-1.0, 0.0, 0.25]))


# ------------------------------------------------------------------ determinism

def test_two_calls_give_the_same_bytes():
    import torch
    from ocm import roc

    m = 5 * _T() + 3
    S = family("special", m, 5, np.float64, seed=31)
    S[11, 2] = np.nan
    pos = _mask(m, 0.45, seed=32)
    t, p8 = _dev(S), _dev(pos.astype(np.uint8))
    thr = _dev(np.sort(np.random.default_rng(33).standard_normal((5, 64)), axis=1))
    runs = []
    for _ in range(2):
        u2, P, N, nnan = _kernel_auc(t, pos)
        srt = roc.sort_values(t)
        cnt = roc.roc_counts(t, p8, thr)
        torch.cuda.synchronize()
        runs.append((u2.tobytes(), P, N, nnan.tobytes(), srt.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ estimator

@pytest.mark.parametrize("ty", ["alt", "sim", "ci", "dd"])
def test_simca_roc_auc(ty):
    from ocm import roc
    from utils import SIMCA

    Xf, yf, Xt, yt = plsda_data(360, 400, 24, 3, 4.0, 77)
    est = SIMCA(n_components=4, model_class=None, type=ty, verbose=False).fit(Xf, yf)
    D = est.decision_function(Xt)
    res = est.roc_auc(Xt, yt)
    assert list(res) == [0, 1, 2]
    for i, cls in enumerate(est.model_class):
        want = roc.u2_host(D[:, i], yt == cls)
        assert int(res[cls].u2[0]) == want
        assert res[cls].n_pos == int((yt == cls).sum()) and res[cls].n_neg == int((yt != cls).sum())
        assert res[cls].auc[0] == want / (2 * res[cls].n_pos * res[cls].n_neg)
        print(f"SIMCA.roc_auc type={ty} class {cls}: auc = {res[cls].auc[0]:.4f}")
    assert any(0 < int(r.u2[0]) < 2 * r.n_pos * r.n_neg for r in res.values())  # not every ranking is perfect
    one = est.roc_auc(_dev(Xt), yt, cls=1)
    assert int(one.u2[0]) == int(res[1].u2[0])
    pts = est.roc_points(Xt, yt, cls=2, n_points=17)
    ref = roc.roc_points_host(D[:, 2], yt == 2, n_points=17)
    np.testing.assert_array_equal(pts.tp, ref.tp)
    np.testing.assert_array_equal(pts.fp, ref.fp)
    with pytest.raises(ValueError, match="not fitted"):
        est.roc_auc(Xt, yt, cls=5)
    with pytest.raises(ValueError, match="rows"):
        est.roc_auc(Xt, yt[:-1])


# ------------------------------------------------------------------ cross-validation

@pytest.fixture(scope="module")
def data():
    return object_data()


def _splitters(ids):
    from ocm.objectcv import ObjectKFoldWithExternalVal
    from utils.CVSIMCA import ClasswiseKFoldWithExternalVal

    return {"rows": lambda: ClasswiseKFoldWithExternalVal(n_splits=3, cls_label=0),
            "objects": lambda: ObjectKFoldWithExternalVal(n_splits=3, objects=ids, cls_label=0)}


@pytest.mark.parametrize("split", ["rows", "objects"])
def test_cv_auc_grid_on_the_fold_engine(data, split, monkeypatch):
    import ocm.cv as fe
    from ocm import roc
    from utils import SIMCA, cross_validate_simca_grid

    X, y, ids = data
    make = _splitters(ids)[split]
    calls = {"n": 0}
    orig = fe.cv_grid
    monkeypatch.setattr(fe, "cv_grid", lambda *a, **k: (calls.__setitem__("n", calls["n"] + 1), orig(*a, **k))[1])
    grid = {"type": ["alt"], "dcl": [0.9, 0.99]}
    res = roc.cross_validate_auc_grid(SIMCA(verbose=False), X, y, make(), LV_min=2, LV_max=4, param_grid=grid,
                                      store_scores=True)
    assert calls["n"] == 1
    assert set(res) == {"results", "best_params", "best_LV", "best_score", "best_estimator", "by_combo"}
    with contextlib.redirect_stdout(io.StringIO()):
        px = cross_validate_simca_grid(SIMCA(verbose=False), X, y, make(), LV_min=2, LV_max=4, param_grid=grid,
                                       print_summary=False, store_predictions=True)
    assert [(r["params"], r["LV"]) for r in res["results"]] == [(r["params"], r["LV"]) for r in px["results"]]
    assert [r["LV"] for r in res["results"]] == [2, 3, 4, 2, 3, 4]
    positive = y == 0
    for r, b, q in zip(res["results"], res["by_combo"], px["by_combo"]):
        assert len(b["folds"]) == 3 and r["auc"] == float(np.mean(r["auc_folds"]))
        pooled = np.zeros(y.size)
        for f, fold in enumerate(b["folds"]):
            rows, s = fold["rows"], fold["scores"]
            pos = positive[rows]
            assert fold["n_pos"] == int(pos.sum()) and fold["n_neg"] == int((~pos).sum()) == int((y != 0).sum())
            assert pos[:fold["n_pos"]].all()  # the held-out target rows come first
            assert fold["u2"] == roc.u2_host(s, pos)
            assert r["auc_folds"][f] == fold["u2"] / (2 * fold["n_pos"] * fold["n_neg"])
            keep = slice(0, fold["n_pos"]) if f < 2 else slice(0, rows.size)
            pooled[rows[keep]] = s[keep] > 0
        np.testing.assert_array_equal(pooled, q["prediction"])
    # dcl moves the cut, not the ranking
    for a, b in zip(res["by_combo"][:3], res["by_combo"][3:]):
        assert a["LV"] == b["LV"] and a["params"]["dcl"] != b["params"]["dcl"]
        assert [f["u2"] for f in a["folds"]] == [f["u2"] for f in b["folds"]]
    aucs = [r["auc"] for r in res["results"]]
    assert res["best_score"] == max(aucs) and res["best_LV"] == res["results"][int(np.argmax(aucs))]["LV"]
    assert res["best_estimator"].is_fitted_


def test_cv_auc_engine_route_vs_refit_loop(data, monkeypatch):
    """The fold engine against a refit per fold: the same best LV, and AUCs within
    4 × the noise floor, which is the refit loop on float32 input against the
    same loop on float64 input (the engine's downdated Gram and a refit differ by
    summation order only).  Measured on an MI355X on these rows: max |ΔAUC| = 0 and
    floor = 0 over the 12 fold values (an AUC moves in steps of 1 / (2 P N) and no
    pair of rows changed order); every route chooses LV 5."""
    import ocm.cv as fe
    from ocm import roc
    from utils import SIMCA

    X, y, ids = data
    make = _splitters(ids)["rows"]
    kw = dict(LV_min=2, LV_max=5, param_grid={"type": ["alt"]})
    calls = {"engine": 0, "loop": 0}
    orig_grid, orig_loop = fe.cv_grid, roc._loop_auc
    monkeypatch.setattr(fe, "cv_grid", lambda *a, **k: (calls.__setitem__("engine", calls["engine"] + 1),
                                                        orig_grid(*a, **k))[1])
    monkeypatch.setattr(roc, "_loop_auc", lambda *a, **k: (calls.__setitem__("loop", calls["loop"] + 1),
                                                           orig_loop(*a, **k))[1])
    fast = roc.cross_validate_auc_grid(SIMCA(verbose=False), X, y, make(), **kw)
    assert calls == {"engine": 1, "loop": 0}  # float32 rows: the fold engine
    loop64 = roc.cross_validate_auc_grid(SIMCA(verbose=False), X.astype(np.float64), y, make(), **kw)
    assert calls == {"engine": 1, "loop": 1}  # float64 rows: a refit per (setting, fold)
    monkeypatch.setattr(fe, "_applicable", lambda *a, **k: None)
    loop32 = roc.cross_validate_auc_grid(SIMCA(verbose=False), X, y, make(), **kw)
    assert calls == {"engine": 1, "loop": 2}

    def folds(res):
        return np.array([r["auc_folds"] for r in res["results"]])

    floor = float(np.abs(folds(loop32) - folds(loop64)).max())
    delta = float(np.abs(folds(fast) - folds(loop32)).max())
    print(f"cv auc: engine vs refit loop max |dAUC| = {delta:.3e}; noise floor (loop f32 vs f64) = {floor:.3e}; "
          f"best LV engine {fast['best_LV']}, loop {loop32['best_LV']}, loop f64 {loop64['best_LV']}")
    assert fast["best_LV"] == loop32["best_LV"]
    assert delta <= 4 * floor
