"""Multi-class SIMCA on the GPU: ocm_score_multi_f32 against the float64 oracle
(the kernel fed the oracle's P, μ, 1/λ and limits: tested apart from the fit),
the exact identities among its own outputs, and ``SIMCA.classify`` /
``model_distance`` on the estimator.

Tolerances: T², Q and ratio rtol 1e-4 (test_headline_vs_fp64_oracle);
decisions compared outside the band |ratio₆₄ − 1| < 1e-4, assignments outside it
and where the two smallest float64 ratios differ by ≥ 2e-4 relative; at most 2
rows per case may fall in the bands (a property of the float64 reference)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import gpu_available
from test_plsda_host import plsda_data

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

RTOL = 1e-4
TYPES = ("alt", "sim", "ci", "dd")
CASES4 = [(8, 33, (2, 2)), (37, 65, (5, 3, 4)), (129, 257, (6,) * 4), (256, 300, (16,) * 3)]
CASES_ALT = [(1050, 65, (8,) * 8), (2048, 130, (20,) * 3), (2500, 40, (12, 12)),
             (37, 0, (5, 3, 4)), (37, 1, (5, 3, 4)), (37, 15, (5, 3, 4)), (37, 16, (5, 3, 4)), (37, 17, (5, 3, 4)),
             # the three- and four-tile variants of the kernel (k_c > 32, > 48)
             (70, 33, (40, 5)), (100, 33, (64,))]
OUTS = ("T2", "Q", "ratio", "pred", "index", "nearest", "n_accept", "counts")


@functools.lru_cache(maxsize=None)
def case_data(p, m, C, k):
    """(X_fit, y_fit, X_test, y_test) with the last m // 8 test rows carrying an extra band (true label C)."""
    n = max(200 * C, 12 * k * C)
    Xf, yf, Xt, yt = plsda_data(n, m, p, C, 4.0, 500 + p)
    Xt, yt = Xt.copy(), yt.copy()
    wl = np.linspace(0.0, 1.0, max(p, 8))[:p]
    B = np.exp(-0.5 * ((wl - 0.5) / 0.02) ** 2)
    no = m // 8
    if no:
        Xt[m - no:] += (6.0 * B / np.linalg.norm(B)).astype(np.float32)
        yt[m - no:] = C
    for a in (Xt, yt):
        a.setflags(write=False)
    return Xf, yf, Xt, yt


@functools.lru_cache(maxsize=None)
def oracle_case(p, m, ks, kind):
    """The float64 oracle's models and its per-class T², Q, ratio and decision of the test rows."""
    from oracle import simca_oracle as O
    from ocm import engine

    C = len(ks)
    Xf, yf, Xt, yt = case_data(p, m, C, max(ks))
    orc = O.OracleSIMCA(n_components=list(ks), type=kind, precision="exact").fit(Xf.astype(np.float64), yf)
    P, mu, a, decs = [], [], [], []
    T2 = np.zeros((m, C))
    Q = np.zeros((m, C))
    ratio = np.zeros((m, C))
    pred = np.zeros((m, C))
    X64 = Xt.astype(np.float64)
    for i, cls in enumerate(orc.model_class):
        md = orc._model[cls]
        k = md["n_components"]
        ai = np.diag(md["invcovT"])[:k].copy()
        P.append(np.asarray(md["P_pred"], np.float64))
        mu.append(np.asarray(md["mean_pred"], np.float64))
        a.append(ai)
        if kind == "dd":  # the last class's dof / scale for every class, as SIMCA._decision
            decs.append(engine.make_decision("dd", orc.st.t2dof / orc.st.t2scfact, orc.st.qdof / orc.st.qscfact,
                                             md["D_limit"]))
        else:
            decs.append(engine.make_decision(kind, 1.0 / md["T2_limit"], 1.0 / md["Q_limit"], md["D_limit"]))
        _, T2[:, i], Q[:, i] = O.project_scores(X64, P[-1], mu[-1], np.diag(ai))
        d = O.reduce_distances(kind, T2[:, i], Q[:, i], md["T2_limit"], md["Q_limit"], orc.st)[2]
        ratio[:, i] = d / md["D_limit"]
        pred[:, i] = d < md["D_limit"]
    return {"P": np.concatenate(P), "mu": np.stack(mu), "a": np.concatenate(a), "decs": decs,
            "koff": [0] + list(np.cumsum(ks)), "T2": T2, "Q": Q, "ratio": ratio, "pred": pred, "X": Xt, "y": yt}


def run_multi(X, rows, m, oc, y=None, skip=(), ldx=None):
    """Raw ocm_score_multi_f32 call; X a device tensor (may be wider than p), outputs in ``skip`` passed NULL."""
    from ocm import _lib
    from ocm._lib import OcmDecision

    dev = X.device
    p = oc["P"].shape[1]
    C = len(oc["decs"])
    f64 = dict(dtype=torch.float64, device=dev)
    P, mu, a = (torch.from_numpy(np.ascontiguousarray(oc[n])).to(dev) for n in ("P", "mu", "a"))
    o = {"T2": torch.full((m, C), -7.0, **f64), "Q": torch.full((m, C), -7.0, dtype=torch.float32, device=dev),
         "ratio": torch.full((m, C), -7.0, **f64), "pred": torch.full((m, C), -7.0, **f64),
         "index": torch.full((m,), 77, dtype=torch.int8, device=dev),
         "nearest": torch.full((m,), 77, dtype=torch.uint8, device=dev),
         "n_accept": torch.full((m,), 77, dtype=torch.uint8, device=dev),
         "counts": torch.full(((C + 1) * (3 * C + 2),), -7, dtype=torch.int64, device=dev) if y is not None else None}
    for name in skip:
        o[name] = None
    koff = (ctypes.c_int32 * (C + 1))(*[int(v) for v in oc["koff"]])
    dec = (OcmDecision * C)(*oc["decs"])
    ptr = _lib.ptr
    _lib.check(_lib.load().ocm_score_multi_f32(
        _lib.Context.get(dev.index).handle, ptr(X), X.stride(0) if ldx is None else ldx, ptr(rows), m, p, ptr(P),
        ptr(mu), ptr(a), koff, C, dec, ptr(o["T2"]), ptr(o["Q"]), ptr(o["ratio"]), ptr(o["pred"]), C,
        ptr(o["index"]), ptr(o["nearest"]), ptr(o["n_accept"]), ptr(y) if o["counts"] is not None else None,
        ptr(o["counts"]), _lib.stream_handle(dev)), "ocm_score_multi_f32")
    torch.cuda.synchronize()
    return {n: (v.cpu().numpy() if v is not None else None) for n, v in o.items()}


def y_dev(y, dev):
    return torch.from_numpy(np.minimum(y, 255).astype(np.uint8)).to(dev)


def check_against_oracle(out, oc, m, C, y):
    """Every assertion of a kernel case; prints the figures first."""
    from ocm import engine, multiclass as mc

    r64, p64 = oc["ratio"], oc["pred"]
    if m:
        e_t2 = np.max(np.abs(out["T2"] - oc["T2"]) / np.abs(oc["T2"]))
        e_q = np.max(np.abs(out["Q"] - oc["Q"]) / np.abs(oc["Q"]))
        e_r = np.max(np.abs(out["ratio"] - r64) / np.abs(r64))
        print(f"max rel err T2 {e_t2:.3g} Q {e_q:.3g} ratio {e_r:.3g}; n_accept hist "
              f"{np.bincount(out['n_accept'], minlength=C + 1).tolist()}")
    np.testing.assert_allclose(out["T2"], oc["T2"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(out["Q"], oc["Q"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(out["ratio"], r64, rtol=RTOL, atol=0)
    band = np.abs(r64 - 1.0) < 1e-4
    assert np.array_equal(out["pred"][~band], p64[~band])
    i64, n64, _ = mc.assign(r64, p64)
    srt = np.sort(r64, axis=1)
    close = (srt[:, 1] - srt[:, 0]) < 2e-4 * np.abs(srt[:, 1]) if C > 1 else np.zeros(m, dtype=bool)
    left_out = band.any(1) | close
    print(f"rows left out of the assignment check: {int(left_out.sum())}")
    assert left_out.sum() <= 2
    assert np.array_equal(out["index"][~left_out], i64[~left_out])
    assert np.array_equal(out["nearest"][~left_out], n64[~left_out])
    # exact identities among the kernel's own outputs
    assert set(np.unique(out["pred"])) <= {0.0, 1.0}
    assert np.array_equal(out["n_accept"], out["pred"].sum(1))
    ia, na, _ = mc.assign(out["ratio"], out["pred"])
    assert np.array_equal(out["index"], ia) and np.array_equal(out["nearest"], na)
    C1 = C + 1
    table, acc, hist = mc.count_tables(y, out["index"], out["pred"])
    cnt = out["counts"]
    assert np.array_equal(cnt[:C1 * C1].reshape(C1, C1), table)
    assert np.array_equal(cnt[C1 * C1:C1 * C1 + C1 * C].reshape(C1, C), acc)
    assert np.array_equal(cnt[C1 * C1 + C1 * C:].reshape(C1, C1), hist)
    assert table.sum() == m
    if m:
        dev = torch.device("cuda", 0)
        pred_d = torch.from_numpy(out["pred"]).to(dev)
        for i in range(C):
            pos = torch.from_numpy((y == i).astype(np.uint8)).to(dev)
            want = engine.confusion_counts(pred_d[:, i:] if C > 1 else pred_d, pos, stride=C).cpu().numpy()
            assert [int(v) for v in mc.confusion_from_counts(table, acc, i)] == [int(v) for v in want]


@pytest.mark.parametrize("kind", TYPES)
@pytest.mark.parametrize("p,m,ks", CASES4)
def test_kernel_vs_oracle_types(p, m, ks, kind):
    oc = oracle_case(p, m, ks, kind)
    dev = torch.device("cuda", 0)
    X = torch.tensor(oc["X"], device=dev)
    out = run_multi(X, None, m, oc, y=y_dev(oc["y"], dev))
    check_against_oracle(out, oc, m, len(ks), oc["y"])


@pytest.mark.parametrize("p,m,ks", CASES_ALT)
def test_kernel_vs_oracle_alt(p, m, ks):
    oc = oracle_case(p, m, ks, "alt")
    dev = torch.device("cuda", 0)
    X = torch.tensor(oc["X"], device=dev)
    out = run_multi(X, None, m, oc, y=y_dev(oc["y"], dev), ldx=p)
    check_against_oracle(out, oc, m, len(ks), oc["y"])


def test_kernel_rows_and_ldx():
    """rows = every other row of a matrix with ldx = p + 5 (unaligned rows: the element-load variant); the rows
    in between and the padding columns hold NaN and are never read."""
    p, m, ks = 300, 130, (17,) * 3
    oc = oracle_case(p, m, ks, "alt")
    dev = torch.device("cuda", 0)
    wide = torch.full((2 * m, p + 5), float("nan"), dtype=torch.float32, device=dev)
    wide[::2, :p] = torch.tensor(oc["X"], device=dev)
    rows = torch.arange(0, 2 * m, 2, dtype=torch.int64, device=dev)
    out = run_multi(wide, rows, m, oc, y=y_dev(oc["y"], dev), ldx=p + 5)
    check_against_oracle(out, oc, m, len(ks), oc["y"])


def test_kernel_argument_limits():
    oc = dict(oracle_case(37, 16, (5, 3, 4), "alt"))
    dev = torch.device("cuda", 0)
    X = torch.tensor(oc["X"], device=dev)
    bad = dict(oc)
    bad["koff"] = [0, 5, 5, 12]  # an empty class
    with pytest.raises(ValueError):
        run_multi(X, None, 16, bad)
    bad = dict(oc)
    bad["koff"] = [0, 5, 8, 65]  # K > 64
    with pytest.raises(ValueError):
        run_multi(X, None, 16, bad)
    bad = dict(oc)
    bad["decs"] = oc["decs"] * 3  # C = 9
    bad["koff"] = list(range(10))
    with pytest.raises(ValueError):
        run_multi(X, None, 16, bad)


def test_kernel_nan_row():
    from ocm import multiclass as mc

    p, m, ks = 37, 65, (5, 3, 4)
    C = len(ks)
    oc = oracle_case(p, m, ks, "alt")
    dev = torch.device("cuda", 0)
    X = torch.tensor(oc["X"], device=dev)
    y = y_dev(oc["y"], dev)
    base = run_multi(X, None, m, oc, y=y)
    r = 21
    Xn = X.clone()
    Xn[r, 5] = float("nan")
    out = run_multi(Xn, None, m, oc, y=y)
    assert np.all(out["pred"][r] == 0) and out["index"][r] == -1 and out["nearest"][r] == 0 and out["n_accept"][r] == 0
    assert np.all(np.isnan(out["ratio"][r]))
    keep = np.arange(m) != r
    for n in ("T2", "Q", "ratio", "pred", "index", "nearest", "n_accept"):
        assert np.array_equal(out[n][keep], base[n][keep]), n
    table, acc, hist = mc.count_tables(oc["y"], out["index"], out["pred"])
    C1 = C + 1
    assert np.array_equal(out["counts"][:C1 * C1].reshape(C1, C1), table)
    assert table[min(int(oc["y"][r]), C), C] >= 1  # the NaN row counts in the "none" column


def test_kernel_null_outputs_and_determinism():
    p, m, ks = 129, 257, (6,) * 4
    oc = oracle_case(p, m, ks, "alt")
    dev = torch.device("cuda", 0)
    X = torch.tensor(oc["X"], device=dev)
    y = y_dev(oc["y"], dev)
    full = run_multi(X, None, m, oc, y=y)
    again = run_multi(X, None, m, oc, y=y)
    for n in OUTS:
        assert full[n].tobytes() == again[n].tobytes(), n
    for skip in OUTS:
        part = run_multi(X, None, m, oc, y=y, skip=(skip,))
        assert part[skip] is None
        for n in OUTS:
            if n != skip:
                assert part[n].tobytes() == full[n].tobytes(), (skip, n)
    none = run_multi(X, None, m, oc, y=None)
    for n in OUTS[:-1]:
        assert none[n].tobytes() == full[n].tobytes(), n


# ------------------------------------------------------------------ estimator
@functools.lru_cache(maxsize=None)
def fitted(p, C=3, k=6, prep=False):
    from utils import SIMCA
    from ocm.preprocess import snv_savgol

    Xf, yf, Xt, yt = case_data(p, 160, C, k)
    dev = torch.device("cuda", 0)
    Xf_d, Xt_d = torch.tensor(Xf, device=dev), torch.tensor(Xt, device=dev)
    if prep:
        Xf_d = snv_savgol(Xf_d, 5, 2, 1, lazy=True).materialize()
    est = SIMCA(n_components=k, model_class=None, type="alt", verbose=False).fit(Xf_d, yf)
    return est, Xt_d, yt, Xf, yf


def close_results(a, b, C):
    """Two ClassifyResults (device) agree within the f32 tolerances."""
    from ocm import multiclass as mc

    ra, rb = a.ratio.cpu().numpy(), b.ratio.cpu().numpy()
    np.testing.assert_allclose(ra, rb, rtol=RTOL, atol=0)
    band = np.abs(rb - 1.0) < 1e-4
    pa, pb = a.pred.cpu().numpy(), b.pred.cpu().numpy()
    assert np.array_equal(pa[~band], pb[~band])
    srt = np.sort(rb, axis=1)
    left = band.any(1) | ((srt[:, 1] - srt[:, 0]) < 2e-4 * np.abs(srt[:, 1]))
    assert left.sum() <= 2
    for n in ("index", "nearest", "label"):
        assert np.array_equal(getattr(a, n).cpu().numpy()[~left], getattr(b, n).cpu().numpy()[~left]), n
    if a.T2 is not None and b.T2 is not None:
        np.testing.assert_allclose(a.T2.cpu().numpy(), b.T2.cpu().numpy(), rtol=RTOL, atol=0)
        np.testing.assert_allclose(a.Q.cpu().numpy(), b.Q.cpu().numpy(), rtol=RTOL, atol=0)


@pytest.mark.parametrize("p", [256, 300])
def test_classify_matches_predict_and_composed(p):
    est, Xt, yt, _, _ = fitted(p)
    C = 3
    fused = est.classify(Xt, y_true=yt, distances=True, route="fused")
    comp = est.classify(Xt, y_true=yt, distances=True, route="composed")
    auto = est.classify(Xt)
    close_results(fused, comp, C)
    close_results(auto, comp, C)
    before = dict(est.metrics)
    pred = est.predict(Xt, y_true=yt).cpu().numpy()
    metrics = dict(est.metrics)
    est.metrics = before
    for res in (fused, comp):
        ph = res.pred.cpu().numpy()
        band = np.abs(res.ratio.cpu().numpy() - 1.0) < 1e-4
        assert np.array_equal(ph[~band], pred[~band])
        assert res.index.dtype == torch.int64 and res.label.dtype == torch.int64
        assert np.array_equal(res.n_accept.cpu().numpy(), ph.sum(1))
        assert int(res.table.sum()) == Xt.shape[0] and int(res.table[C].sum()) == int((yt == C).sum())
        if np.array_equal(ph, pred):
            for cls in est.model_class:
                for key in ("TP", "TN", "FP", "FN", "sensitivity", "specificity", "accuracy", "efficiency"):
                    assert res.metrics[cls][key] == metrics[cls][key] or \
                        (np.isnan(res.metrics[cls][key]) and np.isnan(metrics[cls][key])), (cls, key)
    lab = fused.label.cpu().numpy()
    idx = fused.index.cpu().numpy()
    cls = np.asarray(est.model_class)
    assert np.array_equal(lab, np.where(idx < 0, -1, cls[np.maximum(idx, 0)]))
    # NumPy in, NumPy out, the same values
    host = est.classify(Xt.cpu().numpy(), y_true=yt, route="fused")
    assert isinstance(host.pred, np.ndarray) and host.index.dtype == np.int64 and host.T2 is None
    assert np.array_equal(host.pred, fused.pred.cpu().numpy()) and np.array_equal(host.table, fused.table.cpu().numpy())


@pytest.mark.parametrize("p", [256, 300])
def test_classify_fallbacks(p):
    from ocm.preprocess import snv_savgol

    C = 3
    est, Xt, yt, _, _ = fitted(p)
    f32 = est.classify(Xt, y_true=yt, distances=True, route="fused")
    # float64 spectra: the per-class float64 kernels
    r64 = est.classify(Xt.double(), y_true=yt, distances=True)
    assert r64.Q.dtype == torch.float64
    close_results(f32, r64, C)
    with pytest.raises(ValueError, match="float32"):
        est.classify(Xt.double(), route="fused")
    # a lazy view against its materialised rows
    estp, _, _, _, _ = fitted(p, prep=True)
    view = snv_savgol(Xt, 5, 2, 1, lazy=True)
    lazy = estp.classify(view, y_true=yt, distances=True)
    mat = estp.classify(snv_savgol(Xt, 5, 2, 1, lazy=True).materialize(), y_true=yt, distances=True, route="fused")
    close_results(mat, lazy, C)


def test_classify_k65_composed_matches_fused_parts():
    """K = 65 ([13] × 5) takes the composition; the fused kernel on classes 0..3 and on class 4 gives its columns."""
    from ocm import engine, multiclass as mc

    est, Xt, yt, _, _ = fitted(256, C=5, k=13)
    with pytest.raises(ValueError, match="64 components"):
        est.classify(Xt, route="fused")
    res = est.classify(Xt, y_true=yt, distances=True)
    fits = [est._fits[c] for c in est.model_class]
    decs = [est._decision(est._model[c]["T2_limit"], est._model[c]["Q_limit"], est._model[c]["D_limit"])
            for c in est.model_class]
    m = Xt.shape[0]
    a = engine.score_multi(Xt, None, m, fits[:4], decs[:4])
    b = engine.score_multi(Xt, None, m, fits[4:], decs[4:])
    for n in ("T2", "Q", "ratio"):
        got = torch.cat([a[n], b[n]], dim=1).cpu().numpy()
        np.testing.assert_allclose(getattr(res, n).cpu().numpy(), got, rtol=RTOL, atol=0)
    ratio = res.ratio.cpu().numpy()
    pred = torch.cat([a["pred"], b["pred"]], dim=1).cpu().numpy()
    band = np.abs(ratio - 1.0) < 1e-4
    assert np.array_equal(res.pred.cpu().numpy()[~band], pred[~band])
    idx, near, nacc = mc.assign(ratio, res.pred.cpu().numpy())
    assert np.array_equal(res.index.cpu().numpy(), idx) and np.array_equal(res.nearest.cpu().numpy(), near)
    table, acc, hist = mc.count_tables(yt, idx, res.pred.cpu().numpy())
    assert np.array_equal(res.table.cpu().numpy(), table) and np.array_equal(res.accept_counts.cpu().numpy(), acc)
    assert np.array_equal(res.n_accept_hist.cpu().numpy(), hist)


@pytest.mark.parametrize("p", [256, 300])
def test_model_distance_vs_oracle(p):
    from oracle import simca_oracle as O
    from ocm import multiclass as mc

    est, _, _, Xf, yf = fitted(p)
    C, k = 3, 6
    D = est.model_distance(Xf, yf)
    orc = O.OracleSIMCA(n_components=k, type="alt", precision="exact").fit(Xf.astype(np.float64), yf)
    S = np.zeros((C, C))
    X64 = Xf.astype(np.float64)
    for q, cls in enumerate(orc.model_class):
        md = orc._model[cls]
        _, _, Q = O.project_scores(X64, md["P_pred"], md["mean_pred"], md["invcovT"])
        for r in range(C):
            S[r, q] = Q[yf == r].sum()
    want = mc.wold_distance(S, np.bincount(yf, minlength=C), [k] * C, p)
    print("model distance\n", D, "\noracle\n", want)
    assert D.shape == (C, C) and D.dtype == np.float64
    np.testing.assert_allclose(D, want, rtol=RTOL, atol=0)
    assert np.all(np.diag(D) == 1.0) and np.allclose(D, D.T, rtol=0, atol=0)
