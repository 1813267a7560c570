"""PLS-DA on the GPU: ocm_plsda_predict_f32 and ocm_pls_fit_f64 against NumPy float64, the PLSDA
estimator against scikit-learn, and plsda_cv_curve against the per-fold loops.

Data: test_plsda_host.plsda_data (one synth_spectra call split into fit and test rows, class bands
of strength sep).

Predict kernel, derived bounds.  y = x − μ is formed as (x − hi) − lo (two roundings of y), the
projection matrix is rounded to float32 (one), and an f32 MFMA chain is an fmaf chain with one
rounding per product, PD_CHAIN = L of them before the sum goes to fp64:
    |t − t₆₄| ≤ (L + 3)·2⁻²⁴·Σ_j |y_j|·|P_aj| + 2⁻²⁴·|t₆₄|         (the last term: the float32 store)
    |D − D₆₄| ≤ Σ_a |coef_a|·(that bound) + 2⁻²⁴·|D₆₄|
and a prediction must be the float64 argmax wherever the float64 margin (top minus second) exceeds
twice the row's largest D bound; the other rows are at most 1 % of a case.

Fit kernel: the deviation from the float64 oracle per component is at most 16 × the deviation of
the float64 oracle from the same recursion in np.longdouble, plus 2⁻⁴⁰ (both are fp64 roundings of
one recursion in another order of summation; 16 covers the order).

Estimator against scikit-learn (float64 on the same float32-valued arrays), A = 12 (later
components amplify a 5e-8 perturbation of the Gram like late Lanczos vectors: at A = 25 the
comparison would test conditioning, not this code).  The constants below are 4 × the largest
deviation measured on an MI355X over the cases of this file ("PLS-DA")."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import gpu_available
from test_plsda_host import one_component_moments, plsda_data, rel_dev, standardise, targets

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24

# The largest deviations from scikit-learn measured on an MI355X over EST_CASES, per target, relative
# to the component's largest |score| (transform) and to the case's largest |class difference|
# (decision_function); the bounds are 4 × these, for the spread from seed to seed.
T_MEASURED = {"label": 2.34e-6, "onehot": 6.89e-6}
D_MEASURED = {"label": 1.26e-6, "onehot": 2.14e-6}
T_BOUND = {t: 4 * v for t, v in T_MEASURED.items()}
D_BOUND = {t: 4 * v for t, v in D_MEASURED.items()}


def chain_length():
    src = open(os.path.join(REPO, "ocm-vae-simca_amd", "csrc", "ocm_pls.hip")).read()
    return int(re.search(r"constexpr int PD_CHAIN = (\d+);", src).group(1))


def lv_list(k, nlv):
    lv = sorted(set(int(round(v)) for v in np.linspace(1, k, nlv)))
    assert len(lv) == nlv
    return lv


# --------------------------------------------------------------------------- predict kernel
PREDICT_CASES = [(1, 5, 1, 2, 1, 0, False), (3, 17, 3, 2, 3, 0, False), (37, 33, 5, 3, 5, 0, True),
                 (256, 129, 16, 3, 16, 0, False), (300, 257, 17, 4, 4, 3, True), (1050, 65, 21, 8, 21, 0, False),
                 (2048, 130, 25, 3, 25, 0, True), (260, 40, 64, 3, 7, 0, False), (2500, 20, 12, 2, 12, 0, False)]


@functools.lru_cache(maxsize=None)
def predict_reference(p, m, k, C, nlv):
    """A NumPy float64 PLS + LDA fit of the data and its float64 predictions of the test rows.
    The fit regresses on the indicator matrix: a regression on the class value cannot tell 8
    classes apart (accuracy 0.25 on the 8-class case), so its class scores tie on many rows, and
    rows inside the margin check nothing.  The share of such rows is a property of the float64
    reference and the derived bound alone; no kernel output enters it."""
    from ocm.plsda import lda_tables, pls_from_moments

    n = max(400, 4 * k)
    Xf, yf, Xt, yt = plsda_data(n, m, p, C, 1.0, 300 + p)
    Xc, Yc, xm, xs = standardise(Xf, targets(yf, C, "onehot"))
    fit = pls_from_moments(Xc.T @ Xc, Xc.T @ Yc, k)
    assert fit["ncomp"] == k
    T = Xc @ fit["R"].T
    mc = np.stack([T[yf == c].mean(0) for c in range(C)])
    lvs = lv_list(k, nlv)
    coef, icpt = lda_tables(fit["tt"], mc, np.bincount(yf, minlength=C), lvs, k)
    P = fit["R"] / xs[None, :]
    Y = Xt.astype(np.float64) - xm
    t64 = Y @ P.T
    tb = (chain_length() + 3) * U24 * (np.abs(Y) @ np.abs(P).T)
    D64 = np.einsum("ra,lca->rlc", t64, coef) + icpt[None]
    Db = np.einsum("ra,lca->rlc", tb + U24 * np.abs(t64), np.abs(coef))
    return {"Xt": Xt, "yt": yt, "P": P, "mu": xm, "lvs": lvs, "coef": coef, "icpt": icpt, "t64": t64,
            "tbound": tb + U24 * np.abs(t64), "D64": D64, "Dbound": Db + U24 * np.abs(D64)}


@pytest.mark.parametrize("p,m,k,C,nlv,pad,gather", PREDICT_CASES)
def test_predict_kernel(p, m, k, C, nlv, pad, gather):
    from ocm import engine

    ref = predict_reference(p, m, k, C, nlv)
    rng = np.random.default_rng(p + m)
    extra = 13 if gather else 0
    host = np.full((m + extra, p), 1e30, np.float32)  # rows the gather must not read as data
    rows_h = rng.permutation(m + extra)[:m] if gather else np.arange(m)
    host[rows_h] = ref["Xt"]
    buf = torch.full((m + extra, p + pad), 7e29, dtype=torch.float32, device="cuda")
    buf[:, :p] = torch.from_numpy(host).cuda()
    X = buf[:, :p]
    rows = torch.from_numpy(rows_h.astype(np.int64)).cuda() if gather else None
    yt = ref["yt"].astype(np.uint8).copy()
    yt[::7] = 255  # labels outside the classes count nowhere
    if m > 3:
        yt[3] = C
    P = torch.from_numpy(ref["P"]).cuda()
    mu = torch.from_numpy(ref["mu"]).cuda()
    table = torch.from_numpy(np.concatenate([ref["coef"].ravel(), ref["icpt"].ravel()])).cuda()
    PADR = 3

    def launch():
        T = torch.full((m + PADR, k), float("nan"), dtype=torch.float32, device="cuda")
        D = torch.full((m + PADR, nlv, C), float("nan"), dtype=torch.float32, device="cuda")
        pred = torch.full((m + PADR, nlv), 201, dtype=torch.uint8, device="cuda")
        out = engine.plsda_predict(X, rows, m, P, mu, ref["lvs"], C, table, y_true=torch.from_numpy(yt).cuda(),
                                   outs={"T": T, "D": D, "pred": pred})
        torch.cuda.synchronize()
        return T.cpu().numpy(), D.cpu().numpy(), pred.cpu().numpy(), out["counts"].cpu().numpy()

    T, D, pred, counts = launch()
    assert np.isnan(T[m:]).all() and np.isnan(D[m:]).all() and (pred[m:] == 201).all()
    T, D, pred = T[:m], D[:m], pred[:m]
    terr = np.abs(T - ref["t64"])
    print(f"T: max err/bound {np.max(terr / ref['tbound']):.3g}")
    assert (terr <= ref["tbound"]).all()
    derr = np.abs(D - ref["D64"])
    print(f"D: max err/bound {np.max(derr / ref['Dbound']):.3g}")
    assert (derr <= ref["Dbound"]).all()
    srt = np.sort(ref["D64"], axis=2)
    margin = srt[:, :, -1] - srt[:, :, -2]
    clear = margin > 2 * ref["Dbound"].max(axis=2)
    print(f"pred: {int((~clear).sum())} of {clear.size} inside the margin")
    assert (~clear).sum() <= 0.01 * clear.size
    assert (pred[clear] == np.argmax(ref["D64"], axis=2)[clear]).all()
    assert pred.max() < C
    want = np.zeros((nlv, C, C), np.int64)
    ok = yt < C
    for l in range(nlv):
        np.add.at(want[l], (yt[ok].astype(int), pred[ok, l].astype(int)), 1)
    assert (counts == want).all()
    T2, D2, pred2, counts2 = launch()
    assert T2[:m].tobytes() == T.tobytes() and D2[:m].tobytes() == D.tobytes()
    assert (pred2[:m] == pred).all() and (counts2 == counts).all()


def test_predict_scores_alone_and_empty():
    from ocm import engine

    ref = predict_reference(37, 33, 5, 3, 5)
    X = torch.from_numpy(ref["Xt"].copy()).cuda()
    P, mu = torch.from_numpy(ref["P"]).cuda(), torch.from_numpy(ref["mu"]).cuda()
    out = engine.plsda_predict(X, None, 33, P, mu, want_T=True, want_pred=False)
    assert (np.abs(out["T"].cpu().numpy() - ref["t64"]) <= ref["tbound"]).all()
    table = torch.from_numpy(np.concatenate([ref["coef"].ravel(), ref["icpt"].ravel()])).cuda()
    out = engine.plsda_predict(X[:0], None, 0, P, mu, ref["lvs"], 3, table,
                               y_true=torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert out["counts"].shape == (5, 3, 3) and not out["counts"].any()


# --------------------------------------------------------------------------- fit kernel
FIT_CASES = [(64, "label", 3), (64, "onehot", 3), (300, "onehot", 4), (37, "onehot", 2)]
A_FIT = 12


@functools.lru_cache(maxsize=None)
def fit_reference(p, target, C):
    from ocm.plsda import pls_from_moments

    probs = []
    for b, n in enumerate((600, 500, 700)):
        Xf, yf, _, _ = plsda_data(n, 8, p, C, (1.0, 0.3, 1.0)[b], 500 + 10 * b + p)
        Xc, Yc, _, _ = standardise(Xf, targets(yf, C, target))
        S, s = Xc.T @ Xc, Xc.T @ Yc
        f64 = pls_from_moments(S, s, A_FIT)
        ld = pls_from_moments(S, s, A_FIT, dtype=np.longdouble)
        probs.append((S, s, f64, ld))
    return probs


@pytest.mark.parametrize("p,target,C", FIT_CASES)
def test_fit_kernel(p, target, C):
    from ocm import engine

    probs = fit_reference(p, target, C)
    S = torch.from_numpy(np.stack([q[0] for q in probs])).cuda()
    s = torch.from_numpy(np.stack([q[1] for q in probs])).cuda()
    out = engine.pls_fit(S, s, A_FIT)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b, (_, _, f64, ld) in enumerate(probs):
        assert got["ncomp"][b] == f64["ncomp"] == A_FIT
        for name in ("W", "R", "P", "q", "tt"):
            want = f64[name] if name != "tt" else f64[name][:, None]
            have = got[name][b] if name != "tt" else got[name][b][:, None]
            e_ref = rel_dev(want, np.asarray(ld[name], np.float64).reshape(want.shape), 1)
            dev = rel_dev(have, want, 1)
            print(f"problem {b} {name}: max dev {dev.max():.3g}, max e_ref {e_ref.max():.3g}, "
                  f"max ratio {np.max(dev / (16 * e_ref + 2.0 ** -40)):.3g}")
            assert (dev <= 16 * e_ref + 2.0 ** -40).all(), (b, name)
    again = engine.pls_fit(S, s, A_FIT)
    for k in out:
        assert torch.equal(out[k], again[k]), k


def test_fit_kernel_early_stop():
    from ocm import engine
    from ocm.plsda import pls_from_moments

    p, A = 20, 6
    Xf, yf, _, _ = plsda_data(300, 8, p, 2, 1.0, 77)
    Xc, Yc, _, _ = standardise(Xf, targets(yf, 2, "label"))
    S1, s1 = one_component_moments(p)
    S = torch.from_numpy(np.stack([Xc.T @ Xc, S1, S1])).cuda()
    s = torch.from_numpy(np.stack([Xc.T @ Yc, s1, np.zeros((p, 1))])).cuda()
    out = {k: v.cpu().numpy() for k, v in engine.pls_fit(S, s, A).items()}
    assert list(out["ncomp"]) == [A, 1, 0]
    want = pls_from_moments(S1, s1, A)
    for k in ("W", "R", "P", "q", "tt"):
        assert np.array_equal(out[k][1], want[k]), k  # exact arithmetic: the same bits, zeros after row 0
        assert not out[k][2].any()


# --------------------------------------------------------------------------- estimator against scikit-learn
A_EST = 12
EST_CASES = [(3000, 256, 3, 1.0), (3000, 256, 3, 0.3), (1200, 64, 2, 1.0), (1200, 64, 4, 1.0)]


def sk_differences(lda, T):
    d = lda.decision_function(T)
    return np.stack([np.zeros_like(d), d], 1) if d.ndim == 1 else d - d[:, :1]


@pytest.mark.parametrize("target", ["label", "onehot"])
@pytest.mark.parametrize("n,p,C,sep", EST_CASES)
def test_estimator_matches_sklearn(n, p, C, sep, target):
    from sklearn.cross_decomposition import PLSRegression
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis

    from ocm.plsda import PLSDA

    m = 500
    Xf, yf, Xt, yt = plsda_data(n, m, p, C, sep, 900 + p + C)
    est = PLSDA(A_EST, target=target).fit(Xf, yf)
    assert est.n_components_ == A_EST and list(est.classes_) == list(range(C))
    pls = PLSRegression(n_components=A_EST, tol=1e-12, max_iter=5000)
    pls.fit(Xf.astype(np.float64), targets(yf, C, target))
    X_all = np.concatenate([Xf, Xt])
    T_sk = pls.transform(X_all.astype(np.float64))
    T = est.transform(X_all)
    assert T.dtype == np.float32 and T.shape == (n + m, A_EST)
    tdev = rel_dev(T, T_sk, 0)
    print(f"transform: max deviation per component {tdev.max():.3g} (bound {T_BOUND[target]:.3g})")
    pred = est.predict_sweep(X_all, range(1, A_EST + 1))
    worst_d, inside, total = 0.0, 0, 0
    for a in range(1, A_EST + 1):
        lda = LinearDiscriminantAnalysis().fit(T_sk[:n, :a], yf)
        dsk = sk_differences(lda, T_sk[:, :a])
        scale = np.abs(dsk).max()
        if a in (1, 5, A_EST):
            D = est.decision_function(X_all, a).astype(np.float64)
            worst_d = max(worst_d, np.abs((D - D[:, :1]) - dsk).max() / scale)
        srt = np.sort(dsk, axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > 2 * D_BOUND[target] * scale
        inside += int((~clear).sum())
        total += clear.size
        assert (pred[clear, a - 1] == lda.predict(T_sk[:, :a])[clear]).all(), a
    print(f"decision differences: max deviation {worst_d:.3g} (bound {D_BOUND[target]:.3g}); "
          f"{inside} of {total} predictions inside the margin")
    assert tdev.max() <= T_BOUND[target]
    assert worst_d <= D_BOUND[target]
    assert inside <= 0.01 * total
    assert (est.predict(X_all) == pred[:, -1]).all()


def test_estimator_device_in_device_out():
    from ocm.plsda import PLSDA

    Xf, yf, Xt, yt = plsda_data(1200, 500, 64, 4, 1.0, 900 + 64 + 4)
    est = PLSDA(6).fit(torch.from_numpy(Xf.copy()).cuda(), yf)
    Xd = torch.from_numpy(Xt.copy()).cuda()
    lab, counts = est.predict_sweep(Xd, [2, 6], y_true=yt)
    assert lab.is_cuda and counts.is_cuda and counts.shape == (2, 4, 4) and int(counts.sum()) == 2 * len(yt)
    lab_h, counts_h = est.predict_sweep(Xt, [2, 6], y_true=yt)  # the same model on host input
    assert isinstance(lab_h, np.ndarray) and isinstance(counts_h, np.ndarray)
    assert (lab.cpu().numpy() == lab_h).all() and (counts.cpu().numpy() == counts_h).all()
    assert est.transform(Xd).is_cuda and est.decision_function(Xd, 3).shape == (500, 4)
    assert isinstance(est.transform(Xt), np.ndarray) and est.x_rotations_.shape == (64, 6)


# --------------------------------------------------------------------------- CV curve
def counts_of(y_true, y_pred, C):
    c = np.zeros((C, C), np.int64)
    np.add.at(c, (y_true, y_pred), 1)
    return c


def test_cv_curve_matches_fold_loops():
    from sklearn.cross_decomposition import PLSRegression
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold

    from ocm.plsda import PLSDA, plsda_cv_curve

    n, p, C = 1500, 64, 3
    lvs = list(range(1, 11))
    X, y, _, _ = plsda_data(n, 8, p, C, 0.3, 4242)
    res = plsda_cv_curve(X, y, lv_values=lvs, n_splits=5, shuffle=True, random_state=42)
    assert res["counts_cal"].shape == (10, C, C) and res["counts_cv"].shape == (5, 10, C, C)
    assert (res["counts_cal"].sum((1, 2)) == n).all()
    skf = StratifiedKFold(n_splits=5, shuffle=True, random_state=42)
    own = np.zeros_like(res["counts_cv"])
    skl = np.zeros_like(res["counts_cv"])
    inside = 0
    for f, (tr, va) in enumerate(skf.split(X, y)):
        assert (res["folds"][va] == f).all()
        est = PLSDA(10).fit(X[tr], y[tr])
        _, own[f] = est.predict_sweep(X[va], lvs, y_true=y[va])
        pls = PLSRegression(n_components=10, tol=1e-12, max_iter=5000).fit(X[tr].astype(np.float64),
                                                                          y[tr].astype(np.float64))
        Ttr, Tva = pls.transform(X[tr].astype(np.float64)), pls.transform(X[va].astype(np.float64))
        for l, a in enumerate(lvs):
            lda = LinearDiscriminantAnalysis().fit(Ttr[:, :a], y[tr])
            skl[f, l] = counts_of(y[va], lda.predict(Tva[:, :a]), C)
            dsk = sk_differences(lda, Tva[:, :a])
            srt = np.sort(dsk, axis=1)
            inside += int(((srt[:, -1] - srt[:, -2]) <= 2 * D_BOUND["label"] * np.abs(dsk).max()).sum())
    d_own = int(np.abs(res["counts_cv"] - own).sum())
    d_skl = int(np.abs(res["counts_cv"] - skl).sum())
    print(f"counts: Σ|Δ| {d_own} against the estimator loop, {d_skl} against scikit-learn; {inside} rows inside the margin")
    assert d_own <= 2 * inside
    assert d_skl <= 2 * inside
    # the full model's calibration counts against scikit-learn on all rows
    pls = PLSRegression(n_components=10, tol=1e-12, max_iter=5000).fit(X.astype(np.float64), y.astype(np.float64))
    Tall = pls.transform(X.astype(np.float64))
    cal, inside_cal = np.zeros_like(res["counts_cal"]), 0
    for l, a in enumerate(lvs):
        lda = LinearDiscriminantAnalysis().fit(Tall[:, :a], y)
        cal[l] = counts_of(y, lda.predict(Tall[:, :a]), C)
        dsk = sk_differences(lda, Tall[:, :a])
        srt = np.sort(dsk, axis=1)
        inside_cal += int(((srt[:, -1] - srt[:, -2]) <= 2 * D_BOUND["label"] * np.abs(dsk).max()).sum())
    assert int(np.abs(res["counts_cal"] - cal).sum()) <= 2 * inside_cal

    def f1_of(counts):  # f1_score on label vectors rebuilt from the counts
        t, q = np.nonzero(counts)
        reps = counts[t, q]
        return f1_score(np.repeat(t, reps), np.repeat(q, reps), average="macro", zero_division=0)

    for l in range(len(lvs)):
        assert res["f1_cal"][l] == pytest.approx(f1_of(res["counts_cal"][l]), abs=1e-12)
        assert res["f1_cv"][l] == pytest.approx(np.mean([f1_of(res["counts_cv"][f, l]) for f in range(5)]), abs=1e-12)
