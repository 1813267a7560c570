"""MSC / EMSC on the GPU: ocm_rowfit_f32 and ocm_emsc_apply_f32 against the
definitions evaluated in NumPy float64 (include/ocm.h, scatter correction),
eager against lazy, and MSC views through the estimator and the CV engine.

Inputs: oracle.simca_oracle.synth_spectra rows x, distorted as
a + b·x + d1·λ + d2·λ² + 100 with b ∈ [0.5, 2], a ∈ [−2, 2], d ∈ [−1, 1],
λ = linspace(−1, 1, p); the reference spectrum is the fp64 column mean.

Largest f32 error ratio observed (kernel max abs error over the bound
2 × NumPy-float32 error + 8·eps·max|y|): see DESIGN.md, scatter correction."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

EPS32 = float(np.finfo(np.float32).eps)

# (m, p): smallest; odd p; odd p and > 32 rows; k_score_1p's fused view path; p no power of two; the
# headline p; the register-path limit; the any-p path
SHAPES = [(3, 2), (5, 7), (33, 37), (64, 256), (70, 1000), (40, 2048), (9, 4096), (17, 4100)]
PADS = [0, 3]  # ldx = p, and a row slice of a wider tensor (ldx = p + 3: rows not 16-byte aligned)


def distorted(m, p, seed, xseed=None, outlier_frac=0.0):
    from oracle.simca_oracle import synth_spectra

    rng = np.random.default_rng(seed)
    x = synth_spectra(m, p, 6, rank=16, seed=seed + 1 if xseed is None else xseed,
                      outlier_frac=outlier_frac).astype(np.float64)
    lam = np.linspace(-1.0, 1.0, p)
    a, b = rng.uniform(-2, 2, (m, 1)), rng.uniform(0.5, 2, (m, 1))
    d1, d2 = rng.uniform(-1, 1, (m, 1)), rng.uniform(-1, 1, (m, 1))
    return (a + b * x + d1 * lam + d2 * lam ** 2 + 100.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(m, p):
    """X (float32), and per q ∈ {2, 4} with p ≥ q the estimator (basis, weights) and the fp64
    coefficients; computed once and shared (read-only)."""
    from ocm.preprocess import EMSC

    X = distorted(m, p, seed=1000 + p)
    X.setflags(write=False)
    ref = X.astype(np.float64).mean(0)
    per_q = {}
    for q in (2, 4):
        if p < q:
            continue
        est = EMSC(degree=q - 2, reference=ref)
        assert est.basis_.shape == (q, p)
        C64 = X.astype(np.float64) @ est.weights_.T
        per_q[q] = (est, C64)
    return X, per_q


def on_device(X, pad):
    """The rows on the device, contiguous (pad = 0) or as a slice of a wider tensor."""
    m, p = X.shape
    buf = torch.zeros((m, p + pad), dtype=torch.float32, device="cuda")
    buf[:, :p] = torch.from_numpy(X.copy()).cuda()
    Xd = buf[:, :p]
    assert Xd.stride(0) == p + pad
    return Xd


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def raw_rowfit(Xd, W, q=None, p=None, want_coef=True, want_rowstat=True):
    """ocm_rowfit_f32 as the C ABI exposes it: (rc, coef, rowstat)."""
    from ocm import _lib

    m = Xd.shape[0]
    p = Xd.shape[1] if p is None else p
    q = W.shape[0] if q is None else q
    coef = torch.full((m, max(q, 1)), float("nan"), dtype=torch.float32, device="cuda") if want_coef else None
    rs = torch.full((m, 2), float("nan"), dtype=torch.float32, device="cuda") if want_rowstat else None
    rc = _lib.load().ocm_rowfit_f32(_lib.Context.get(Xd.device.index).handle, _lib.ptr(Xd), Xd.stride(0), m, p,
                                    _lib.ptr(W), q, _lib.ptr(coef), _lib.ptr(rs), _lib.stream_handle(Xd.device))
    torch.cuda.synchronize()
    return rc, coef, rs


def raw_apply(Xd, W, B, q=None, p=None, want_coef=False):
    from ocm import _lib

    m = Xd.shape[0]
    p = Xd.shape[1] if p is None else p
    q = W.shape[0] if q is None else q
    out = torch.full((m, Xd.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    coef = torch.full((m, max(q, 1)), float("nan"), dtype=torch.float32, device="cuda") if want_coef else None
    rc = _lib.load().ocm_emsc_apply_f32(_lib.Context.get(Xd.device.index).handle, _lib.ptr(Xd), Xd.stride(0), m, p,
                                        _lib.ptr(W), _lib.ptr(B), q, _lib.ptr(out), out.stride(0), _lib.ptr(coef),
                                        _lib.stream_handle(Xd.device))
    torch.cuda.synchronize()
    return rc, out, coef


# ------------------------------------------------------------------ 1. coefficients
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("m,p", SHAPES)
def test_rowfit_coefficients_vs_fp64(m, p, pad):
    """|c − c64| ≤ 1 ulp_f32(|c64|) + 1e-9·Σ_j |W_tj·x_j| (rounding to float32 plus slack; the fp64
    summation order).  rowstat = ((float)c0, (float)(1/c1)) within 1 ulp (plus the same summation
    term, carried through 1/c1: |Δ(1/c1)| = |Δc1| / c1²)."""
    X, per_q = case(m, p)
    Xd = on_device(X, pad)
    for q, (est, C64) in per_q.items():
        W = torch.from_numpy(est.weights_).cuda()
        rc, coef, rs = raw_rowfit(Xd, W)
        assert rc == 0
        got = coef.double().cpu().numpy()
        sabs = np.abs(X.astype(np.float64)) @ np.abs(est.weights_).T  # Σ_j |W_tj·x_j|
        bound = ulp32(C64) + 1e-9 * sabs
        err = np.abs(got - C64)
        print(f"rowfit m={m} p={p} ldx=p+{pad} q={q}: min |c1| {np.abs(C64[:, 1]).min():.4f}, "
              f"largest |c − c64| / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (q, float((err / bound).max()))
        rsn = rs.double().cpu().numpy()
        s64 = 1.0 / C64[:, 1]
        assert (np.abs(rsn[:, 0] - C64[:, 0]) <= bound[:, 0]).all()
        assert (np.abs(rsn[:, 1] - s64) <= ulp32(s64) + 1e-9 * sabs[:, 1] * s64 ** 2).all()
        # the pair is the rounded fp64 result the coefficients are rounded from
        assert torch.equal(rs[:, 0], coef[:, 0])


# ------------------------------------------------------------------ 2. eager values
def y_fp64(X, B, C64):
    X64 = X.astype(np.float64)
    return (X64 - C64[:, :1] - C64[:, 2:] @ B[2:]) / C64[:, 1:2]


def y_numpy_f32(X, B, W):
    """The same composition in NumPy float32."""
    W32, B32 = W.astype(np.float32), B.astype(np.float32)
    C = X @ W32.T
    Y = (X - C[:, :1] - C[:, 2:] @ B32[2:]) / C[:, 1:2]
    assert Y.dtype == np.float32
    return Y


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("m,p", SHAPES)
def test_eager_values_vs_fp64(m, p, pad):
    """The rule of tests/test_gpu_contrib.py: max abs error ≤ 2 × the error of the same composition
    in NumPy float32, plus 8·eps_f32·max|y|."""
    from ocm.preprocess import MSC

    X, per_q = case(m, p)
    Xd = on_device(X, pad)
    for q, (est, C64) in per_q.items():
        Y64 = y_fp64(X, est.basis_, C64)
        Y32 = y_numpy_f32(X, est.basis_, est.weights_)
        got = est.transform(Xd)
        assert got.shape == (m, p) and got.dtype == torch.float32 and got.is_contiguous()
        err = float(np.abs(got.double().cpu().numpy() - Y64).max())
        err32 = float(np.abs(Y32.astype(np.float64) - Y64).max())
        bound = 2.0 * err32 + 8.0 * EPS32 * float(np.abs(Y64).max())
        print(f"emsc apply m={m} p={p} ldx=p+{pad} q={q}: kernel err {err:.3e}, numpy-f32 err {err32:.3e} "
              f"(kernel / numpy-f32 {err / max(err32, 1e-300):.4f}), bound {bound:.3e}, ratio {err / bound:.4f}")
        assert err <= bound, (q, err, bound)
        # the coefficients the apply kernel reports are those of the read-only pass
        W, B = (torch.from_numpy(a).cuda() for a in (est.weights_, est.basis_))
        rc, out, coef = raw_apply(Xd, W, B, want_coef=True)
        assert rc == 0 and torch.equal(out, got)
        assert torch.equal(coef, raw_rowfit(Xd, W)[1])
        if q == 2:  # MSC is EMSC(degree=0)
            assert torch.equal(MSC(reference=est.reference_).transform(Xd), got)


# ------------------------------------------------------------------ 3. eager against lazy
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("m,p", SHAPES)
def test_eager_equals_lazy_bit_for_bit(m, p, pad):
    from ocm.prepview import PrepView

    X, per_q = case(m, p)
    est = per_q[2][0]
    Xd = on_device(X, pad)
    eager = est.transform(Xd)
    view = est.transform(Xd, lazy=True)
    assert isinstance(view, PrepView) and view.kind == "msc" and "kind='msc'" in repr(view)
    assert torch.equal(eager, view.materialize())
    assert torch.equal(eager, est.transform(Xd))  # two launches, the same bits
    assert torch.equal(view.rowstat(), est.transform(Xd, lazy=True).rowstat())
    rows = torch.arange(m - 1, -1, -2, device="cuda")  # row selection carries the statistics
    assert torch.equal(view[rows].materialize(), eager[rows])
    assert torch.equal(view.materialize(rows), eager[rows])
    if p >= 5:
        ef = est.transform(Xd, 5, 2, 1)
        vf = est.transform(Xd, 5, 2, 1, lazy=True)
        assert torch.equal(ef, vf.materialize()) and torch.equal(ef, est.transform(Xd, 5, 2, 1))
        # sanity only (the exact arithmetic is the view formula tests/test_gpu_prep.py pins, and the bit
        # identity above): SG is linear and maps the offset to 0, so the result is SG(x) / c1; 1e-4 of
        # the largest value would notice a missing filter, offset or scale
        from oracle.simca_oracle import preprocess_reference

        want = preprocess_reference(X.astype(np.float64), 5, 2, 1, 1.0, False) / per_q[2][1][:, 1:2]
        np.testing.assert_allclose(ef.double().cpu().numpy(), want, rtol=0, atol=1e-4 * np.abs(want).max())


# ------------------------------------------------------------------ 4. the view through the estimator
def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.fixture(scope="module")
def estimator_case():
    p, w, po, d, k = 256, 5, 2, 1, 6
    Xtr = torch.from_numpy(distorted(600, p, seed=77, xseed=11)).cuda()
    Xte = torch.from_numpy(distorted(200, p, seed=78, xseed=11, outlier_frac=0.3)).cuda()  # the same loadings
    return Xtr, Xte, np.zeros(600, dtype=np.int64), (w, po, d), k


def _fit_predict(train, test, y, k):
    from utils import SIMCA

    est = SIMCA(n_components=k, model_class=0, verbose=False)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(train, y)
        pred = _np(est.predict(test))
        tr = [_np(v) for v in est.transform(test)]
        df = _np(est.decision_function(test))
    return est, pred, tr, df


def _same_model(a, b):
    """What tests/test_gpu_prep.py asserts for SNV views at the estimator level: T², Q at rtol 1e-4
    (atol 1e-5·median), the limits at 1e-5, decisions equal outside the 1e-4 band of the limit."""
    (ea, pa, ta, da), (eb, pb, tb, db) = a, b
    ma, mb = ea._model[0], eb._model[0]
    for key in ("T2", "Q"):
        np.testing.assert_allclose(ma[key], mb[key], rtol=1e-4, atol=1e-5 * np.median(mb[key]), err_msg=key)
    for key in ("T2_limit", "Q_limit", "D_limit"):
        np.testing.assert_allclose(ma[key], mb[key], rtol=1e-5, err_msg=key)
    for va, vb in zip(ta, tb):
        np.testing.assert_allclose(va, vb, rtol=1e-4, atol=1e-5 * np.median(np.abs(vb)))
    dl = float(mb["D_limit"])
    np.testing.assert_allclose(da, db, rtol=1e-4, atol=1e-4 * dl)
    clear = np.abs(db[:, 0]) > 1e-4 * dl
    np.testing.assert_array_equal(pa[clear], pb[clear])
    assert 0 < pb.sum() < pb.size  # both decisions occur


def test_msc_view_through_estimator(estimator_case):
    from ocm.preprocess import MSC
    from ocm.prepview import materialised_count

    Xtr, Xte, y, (w, po, d), k = estimator_case
    msc = MSC().fit(Xtr)
    np.testing.assert_allclose(msc.reference_, Xtr.double().mean(0).cpu().numpy(), rtol=1e-12)
    mat = _fit_predict(msc.transform(Xtr, w, po, d), msc.transform(Xte, w, po, d), y, k)
    c0 = materialised_count(0)
    lazy = _fit_predict(msc.transform(Xtr, w, po, d, lazy=True), msc.transform(Xte, w, po, d, lazy=True), y, k)
    assert materialised_count(0) == c0  # fit, predict, transform, decision_function ran on the fused paths
    _same_model(lazy, mat)
    bits = all(np.array_equal(a, b) for a, b in zip([lazy[1], *lazy[2], lazy[3]], [mat[1], *mat[2], mat[3]]))
    print(f"MSC view vs materialised tensors: predict / transform / decision_function bit-identical: {bits}")
    vw_tr = msc.transform(Xtr, w, po, d, lazy="write")
    write = _fit_predict(vw_tr, msc.transform(Xte, w, po, d, lazy="write"), y, k)
    print(f"write-through MSC view written by the fit: {vw_tr.written() is not None}")
    if vw_tr.written() is not None:
        assert torch.equal(vw_tr.written(), msc.transform(Xtr, w, po, d))
    _same_model(write, mat)
    # contributions accept the view: bit for bit what its materialised rows give
    est = mat[0]
    rv = est.contributions(msc.transform(Xte, w, po, d, lazy=True), groups="decision", matrices=True)
    rm = est.contributions(msc.transform(Xte, w, po, d), groups="decision", matrices=True)
    for name in ("Q", "T2", "q_profile", "t2_profile", "counts", "E", "C"):
        assert torch.equal(getattr(rv, name), getattr(rm, name)), name


# ------------------------------------------------------------------ 5. CV
@pytest.mark.parametrize("fast", [True, False])
def test_cv_grid_on_msc_view(fast):
    """cross_validate_simca_grid on an MSC view (the fold engine, and the generic refit loop slicing
    X[rows, :]) = the run on the materialised tensor: row selection carries the statistics."""
    import utils.CVSIMCA as CVmod
    from ocm.preprocess import MSC
    from utils import SIMCA, ClasswiseKFoldWithExternalVal, cross_validate_simca_grid

    n, p = 300, 64
    Xd = torch.from_numpy(distorted(n, p, seed=21)).cuda()
    y = np.zeros(n, dtype=np.int64)
    y[::7] = 1
    v = MSC().fit(Xd).transform(Xd, 5, 2, 1, lazy=True)
    outs = []
    for data in (v, v.materialize()):
        saved = CVmod._fast_grid
        if not fast:
            CVmod._fast_grid = lambda *a, **k: (None, None)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                outs.append(cross_validate_simca_grid(
                    SIMCA(verbose=False), data, y, ClasswiseKFoldWithExternalVal(n_splits=3, cls_label=0),
                    LV_min=2, LV_max=4, param_grid={"type": ["alt", "sim"]}, print_summary=False,
                    store_predictions=True))
        finally:
            CVmod._fast_grid = saved
    a, b = outs
    assert [(r["LV"], r["spec"], r["sens"]) for r in a["results"]] == \
        [(r["LV"], r["spec"], r["sens"]) for r in b["results"]]
    assert a["best_LV"] == b["best_LV"]


# ------------------------------------------------------------------ 6. C ABI
def test_c_abi_argument_errors_and_null_outputs():
    from ocm._lib import OCM_ERR_ARG

    X, per_q = case(33, 37)
    Xd = on_device(X, 0)
    W2, B2 = (torch.from_numpy(a).cuda() for a in (per_q[2][0].weights_, per_q[2][0].basis_))
    W9 = torch.zeros((9, 37), dtype=torch.float64, device="cuda")
    for q, p, W, B in ((1, 37, W2, B2), (9, 37, W9, W9), (4, 3, W9, W9)):  # q = 1, q = 9, p < q
        assert raw_rowfit(Xd, W, q=q, p=p)[0] == OCM_ERR_ARG
        assert raw_apply(Xd, W, B, q=q, p=p)[0] == OCM_ERR_ARG
    rc, coef, rs = raw_rowfit(Xd, W2)
    assert rc == 0
    rc, coef_only, none = raw_rowfit(Xd, W2, want_rowstat=False)
    assert rc == 0 and none is None and torch.equal(coef_only, coef)
    rc, none, rs_only = raw_rowfit(Xd, W2, want_coef=False)
    assert rc == 0 and none is None and torch.equal(rs_only, rs)
    assert raw_rowfit(Xd, W2, want_coef=False, want_rowstat=False)[0] == OCM_ERR_ARG
    rc, out, none = raw_apply(Xd, W2, None)  # q = 2 reads no basis
    assert rc == 0 and none is None and torch.equal(out, per_q[2][0].transform(Xd))


def test_fingerprints_of_real_views():
    from ocm import replica
    from ocm.preprocess import MSC, snv_savgol

    X, per_q = case(64, 256)
    Xd = on_device(X, 0)
    y = np.zeros(64, dtype=np.int64)
    ref = per_q[2][0].reference_
    fa = replica.fingerprint(MSC(reference=ref).transform(Xd, 5, 2, 1, lazy=True), y)
    fa2 = replica.fingerprint(MSC(reference=ref.copy()).transform(Xd, 5, 2, 1, lazy=True), y)
    fb = replica.fingerprint(MSC(reference=ref[::-1].copy()).transform(Xd, 5, 2, 1, lazy=True), y)
    fs = replica.fingerprint(snv_savgol(Xd, 5, 2, 1, lazy=True), y)
    assert np.array_equal(fa, fa2) and not np.array_equal(fa, fb) and not np.array_equal(fa, fs)
