"""Contribution plots on the GPU: ocm_contrib_f32 / _f64 against the
definitions evaluated in NumPy float64, and the estimator's decision_function
/ contributions against the CPU oracle.

Largest f32 error ratio observed (kernel max abs error over the bound
2 × NumPy-float32 error + 8·eps·max|y|): see DESIGN.md, contribution kernel."""
import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

EPS32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------- kernel level
def make_case(p, m, k, seed, dtype=np.float32):
    """P from a QR of a seeded Gaussian, μ of order 1, a over three decades,
    X = low rank + noise + offset (oracle.simca_oracle.synth_spectra)."""
    from oracle import simca_oracle as O

    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((p, k)))[0].T)  # (k, p), orthonormal rows
    mu = 1.0 + 0.25 * rng.standard_normal(p)
    a = np.logspace(-3.0, 0.0, k) if k > 1 else np.array([0.37])
    X = O.synth_spectra(m, p, min(k, 6), rank=min(16, p), seed=seed + 1, dtype=dtype)
    return X, P, mu, a


def ref64(X, P, mu, a):
    """The definitions in float64 on the same arrays."""
    Y = X.astype(np.float64) - mu
    T = Y @ P.T
    E = Y - T @ P
    C = Y * ((T * a) @ P)
    return Y, E, C


def ref32(X, P, mu, a):
    """The same quantities composed in float32 as the reference composes them
    (T = (X − μ)·Pᵀ, E = X − (T·P + μ), utils/SIMCA.py:65-68)."""
    X32, P32, mu32, a32 = (np.asarray(v, dtype=np.float32) for v in (X, P, mu, a))
    Y = X32 - mu32
    T = Y @ P32.T
    E = X32 - (T @ P32 + mu32)
    C = Y * ((T * a32) @ P32)
    assert E.dtype == np.float32 and C.dtype == np.float32
    return E, C


def run_contrib(X, rows, m, P, mu, a, group=None, ngroups=1, lde=None, ldc=None, want_E=True, want_C=True,
                want_rows=True, want_prof=True, k=None, ldx=None):
    """Raw ocm_contrib call on device tensors (X may be a strided view)."""
    from ocm import _lib

    dev = X.device
    f64 = X.dtype == torch.float64
    vdt = X.dtype
    p = P.shape[1]
    k = P.shape[0] if k is None else k
    lde = p if lde is None else lde
    ldc = p if ldc is None else ldc
    E = torch.full((m, lde), float("nan"), dtype=vdt, device=dev) if want_E else None
    C = torch.full((m, ldc), float("nan"), dtype=vdt, device=dev) if want_C else None
    T2 = torch.empty(m, dtype=torch.float64, device=dev) if want_rows else None
    Q = torch.empty(m, dtype=vdt, device=dev) if want_rows else None
    prof = torch.empty((ngroups, 2, p), dtype=torch.float64, device=dev) if want_prof else None
    ctx = _lib.Context.get(dev.index)
    fn = "ocm_contrib_f64" if f64 else "ocm_contrib_f32"
    _lib.check(getattr(_lib.load(), fn)(ctx.handle, _lib.ptr(X), X.stride(0) if ldx is None else ldx, _lib.ptr(rows),
                                        m, p, _lib.ptr(P), _lib.ptr(mu), _lib.ptr(a), k, _lib.ptr(group), ngroups,
                                        _lib.ptr(E), lde, _lib.ptr(C), ldc, _lib.ptr(T2), _lib.ptr(Q),
                                        _lib.ptr(prof), _lib.stream_handle(dev)), fn)
    torch.cuda.synchronize()
    return {"E": E, "C": C, "T2": T2, "Q": Q, "prof": prof}


def dev64(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrs]


# (p, m, k, ldx pad): the smallest shapes at which the tiling can go wrong
SHAPES = [(1, 5, 1, 0), (3, 7, 3, 0), (37, 33, 5, 0), (256, 129, 20, 0), (300, 257, 21, 3), (1050, 65, 16, 0),
          (2048, 130, 20, 0), (260, 40, 64, 0),
          (2500, 20, 3, 0)]  # up to p = 1050 the row tile stays in LDS; beyond, the second sweep reads X again


def check_identities(out, Xd, rows, m, Pd, mud, ad, Y, group=None, ngroups=1):
    """Row sums, engine.score and the profiles, at the scoring tolerance (plain rtol 1e-4).
    One absolute floor, and only where k = p: there the residual is rounding noise in both
    kernels (every e_j an error of up to ~8·eps·max|y|, the floor of the E check), so Q from the
    scoring kernel and Q from this one are two different noises below p·(8·eps·max|y|)²."""
    from ocm import engine

    k, p = Pd.shape
    ymax = float(np.abs(Y).max())
    eps = EPS32 if Xd.dtype == torch.float32 else float(np.finfo(np.float64).eps)
    E = out["E"][:, :p].double().cpu().numpy()
    C = out["C"][:, :p].double().cpu().numpy()
    Q = out["Q"].double().cpu().numpy()
    T2 = out["T2"].cpu().numpy()
    np.testing.assert_allclose(Q, (E * E).sum(1), rtol=1e-4)
    np.testing.assert_allclose(T2, C.sum(1), rtol=1e-4)
    sc = engine.score(Xd, rows, m, Pd, mud, ad)
    np.testing.assert_allclose(Q, sc["Q"].double().cpu().numpy(), rtol=1e-4,
                               atol=p * (8 * eps * ymax) ** 2 if k == p else 0.0)
    np.testing.assert_allclose(T2, sc["T2"].cpu().numpy(), rtol=1e-4)
    g = np.zeros(m, dtype=np.int64) if group is None else group
    prof = out["prof"].cpu().numpy()
    for gi in range(ngroups):
        sel = g == gi
        np.testing.assert_allclose(prof[gi, 0], (E[sel] ** 2).sum(0), rtol=1e-4)
        np.testing.assert_allclose(prof[gi, 1], C[sel].sum(0), rtol=1e-4)


@pytest.mark.parametrize("p,m,k,pad", SHAPES)
def test_contrib_f32_matches_definitions(p, m, k, pad):
    X, P, mu, a = make_case(p, m, k, seed=100 + p)
    Y, E64, C64 = ref64(X, P, mu, a)
    E32, C32 = ref32(X, P, mu, a)
    ymax = float(np.abs(Y).max())
    Xbuf = torch.zeros((m, p + pad), dtype=torch.float32).cuda()
    Xbuf[:, :p] = torch.from_numpy(X).cuda()
    Xd = Xbuf[:, :p]  # row stride p + pad: unaligned rows when pad = 3
    Pd, mud, ad = dev64(P, mu, a)
    out = run_contrib(Xd, None, m, Pd, mud, ad)
    worst = 0.0
    for name, got, r64, r32 in (("E", out["E"], E64, E32), ("C", out["C"], C64, C32)):
        err = float(np.abs(got.double().cpu().numpy() - r64).max())
        err32 = float(np.abs(r32.astype(np.float64) - r64).max())
        bound = 2.0 * err32 + 8.0 * EPS32 * ymax
        worst = max(worst, err / bound)
        print(f"contrib f32 p={p} m={m} k={k} {name}: kernel err {err:.3e}, numpy-f32 err {err32:.3e} "
              f"(kernel / numpy-f32 {err / max(err32, 1e-300):.2f}), bound {bound:.3e}, ratio {err / bound:.3f}")
        assert err <= bound, (name, err, bound)
    print(f"contrib f32 p={p} m={m} k={k}: largest ratio {worst:.3f}")
    check_identities(out, Xd, None, m, Pd, mud, ad, Y)


@pytest.mark.parametrize("p,m,k,pad", [(37, 33, 5, 0), (300, 257, 21, 3), (1050, 65, 16, 0), (260, 40, 64, 0),
                                        (1200, 20, 3, 0)])  # p = 37, 300, 260: LDS tile; 1050, 1200: none in fp64
def test_contrib_f64_matches_definitions(p, m, k, pad):
    X, P, mu, a = make_case(p, m, k, seed=200 + p, dtype=np.float64)
    Y, E64, C64 = ref64(X, P, mu, a)
    ymax = float(np.abs(Y).max())
    Xbuf = torch.zeros((m, p + pad), dtype=torch.float64).cuda()
    Xbuf[:, :p] = torch.from_numpy(X).cuda()
    Xd = Xbuf[:, :p]
    Pd, mud, ad = dev64(P, mu, a)
    out = run_contrib(Xd, None, m, Pd, mud, ad)
    for name, got, r64 in (("E", out["E"], E64), ("C", out["C"], C64)):
        err = float(np.abs(got.cpu().numpy() - r64).max())
        print(f"contrib f64 p={p} m={m} k={k} {name}: err {err:.3e}, bound {1e-10 * ymax:.3e}")
        assert err <= 1e-10 * ymax, (name, err)
    check_identities(out, Xd, None, m, Pd, mud, ad, Y)


@pytest.fixture(scope="module")
def case300():
    p, m, k = 300, 257, 21
    X, P, mu, a = make_case(p, m, k, seed=400)
    Xd = torch.from_numpy(X).cuda()
    Pd, mud, ad = dev64(P, mu, a)
    return X, P, mu, a, Xd, Pd, mud, ad


def test_contrib_gather_and_output_strides(case300):
    """Repeated and descending row indices; lde != ldc != p (the padding stays untouched)."""
    X, P, mu, a, Xd, Pd, mud, ad = case300
    p = P.shape[1]
    idx = np.array([256, 200, 200, 7, 7, 7, 0, 131, 130, 129, 17, 16, 15, 3, 255, 1, 1, 64, 32, 31, 30], dtype=np.int64)
    m = idx.size
    rows = torch.from_numpy(idx).cuda()
    Y, E64, C64 = ref64(X[idx], P, mu, a)
    E32, C32 = ref32(X[idx], P, mu, a)
    ymax = float(np.abs(Y).max())
    out = run_contrib(Xd, rows, m, Pd, mud, ad, lde=p + 5, ldc=p + 2)
    assert out["E"].shape == (m, p + 5) and out["C"].shape == (m, p + 2)
    assert torch.isnan(out["E"][:, p:]).all() and torch.isnan(out["C"][:, p:]).all()
    for got, r64, r32 in ((out["E"][:, :p], E64, E32), (out["C"][:, :p], C64, C32)):
        err = float(np.abs(got.double().cpu().numpy() - r64).max())
        bound = 2.0 * float(np.abs(r32.astype(np.float64) - r64).max()) + 8.0 * EPS32 * ymax
        print(f"contrib gather: kernel err {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    # rows 1 and 2 (and 3..5) are the same spectrum: the same results
    assert torch.equal(out["E"][1, :p], out["E"][2, :p]) and torch.equal(out["C"][3, :p], out["C"][5, :p])
    check_identities(out, Xd, rows, m, Pd, mud, ad, Y)


def test_contrib_groups(case300):
    X, P, mu, a, Xd, Pd, mud, ad = case300
    m = X.shape[0]
    rng = np.random.default_rng(5)
    g = rng.integers(0, 2, size=m) * 2  # ids 0 and 2: group 1 stays empty
    g[-3:] = 9  # ids >= ngroups contribute to no profile
    gd = torch.from_numpy(g.astype(np.uint8)).cuda()
    out3 = run_contrib(Xd, None, m, Pd, mud, ad, group=gd, ngroups=3)
    prof3 = out3["prof"]
    assert torch.count_nonzero(prof3[1]) == 0, "the empty group's profile is exactly 0"
    Y = ref64(X, P, mu, a)[0]
    check_identities(out3, Xd, None, m, Pd, mud, ad, Y, group=g, ngroups=3)
    # all rows in three groups against one group
    g2 = rng.integers(0, 3, size=m)
    outg = run_contrib(Xd, None, m, Pd, mud, ad, group=torch.from_numpy(g2.astype(np.uint8)).cuda(), ngroups=3)
    out1 = run_contrib(Xd, None, m, Pd, mud, ad)
    tot = outg["prof"].sum(0).cpu().numpy()
    one = out1["prof"][0].cpu().numpy()
    cabs = np.abs(out1["C"].double().cpu().numpy()).sum(0)  # signed sums: fp64 rounding of Σ|c|
    np.testing.assert_allclose(tot[0], one[0], rtol=1e-12)
    np.testing.assert_allclose(tot[1], one[1], rtol=1e-12, atol=16 * np.finfo(np.float64).eps * cabs.max())


def test_contrib_deterministic_and_null_outputs():
    p, m, k = 2048, 1300, 20
    X, P, mu, a = make_case(p, m, k, seed=7)
    Xd = torch.from_numpy(X).cuda()
    Pd, mud, ad = dev64(P, mu, a)
    g = torch.from_numpy((np.arange(m) % 2).astype(np.uint8)).cuda()
    full = run_contrib(Xd, None, m, Pd, mud, ad, group=g, ngroups=2)
    again = run_contrib(Xd, None, m, Pd, mud, ad, group=g, ngroups=2)
    assert torch.equal(full["prof"], again["prof"])
    assert torch.equal(full["Q"], again["Q"]) and torch.equal(full["T2"], again["T2"])
    # profile mode: no m×p output, the same profiles, and no m×p buffer behind the scenes
    small = run_contrib(Xd[:130], None, 130, Pd, mud, ad, group=g[:130].contiguous(), ngroups=2, want_E=False,
                        want_C=False)
    assert small["prof"].shape == (2, 2, p)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    prof = run_contrib(Xd, None, m, Pd, mud, ad, group=g, ngroups=2, want_E=False, want_C=False)
    grew = torch.cuda.max_memory_allocated() - base
    assert grew < m * p * 4
    assert torch.equal(prof["prof"], full["prof"])
    assert torch.equal(prof["Q"], full["Q"]) and torch.equal(prof["T2"], full["T2"])
    # the library's own workspace is outside torch's allocator: watch the device's free memory over a
    # profile-mode call with eight times the rows of any call so far (the workspace only ever grows, so
    # an m×p buffer would have to be allocated now); the partial profiles grow with the grid, not with m
    m8 = 8 * m
    X8, g8 = Xd.repeat(8, 1), g.repeat(8)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    big = run_contrib(X8, None, m8, Pd, mud, ad, group=g8, ngroups=2, want_E=False, want_C=False)
    taken = free0 - torch.cuda.mem_get_info()[0]
    grew = torch.cuda.max_memory_allocated() - base
    print(f"profile mode m={m8} p={p}: torch peak growth {grew} B, device free memory taken {taken} B "
          f"(m·p·4 = {m8 * p * 4} B)")
    assert grew < m8 * p * 4 and taken < m8 * p * 4
    assert torch.equal(big["Q"][:m], full["Q"]) and torch.equal(big["Q"][7 * m:], full["Q"])
    only = run_contrib(Xd, None, m, Pd, mud, ad, group=g, ngroups=2, want_E=False, want_C=False, want_rows=False)
    assert torch.equal(only["prof"], full["prof"])


def test_contrib_argument_errors(case300):
    from ocm._lib import OcmError

    X, P, mu, a, Xd, Pd, mud, ad = case300
    m = 16
    with pytest.raises((OcmError, ValueError)):
        run_contrib(Xd, None, m, Pd, mud, ad, k=0)
    with pytest.raises((OcmError, ValueError)):
        run_contrib(Xd, None, m, Pd, mud, ad, k=65)
    with pytest.raises((OcmError, ValueError)):
        run_contrib(Xd, None, m, Pd, mud, ad, ngroups=5, want_prof=False)
    with pytest.raises((OcmError, ValueError)):
        run_contrib(Xd, None, m, Pd, mud, ad, ldx=Pd.shape[1] - 1)
    with pytest.raises((OcmError, ValueError)):
        run_contrib(Xd, None, m, Pd, mud, ad, lde=Pd.shape[1] - 1)
    with pytest.raises((OcmError, ValueError)):
        run_contrib(Xd, None, 0, Pd, mud, ad)


# ------------------------------------------------------------- estimator level
def smoke_data(seed=11):
    from oracle import simca_oracle as O

    X = O.synth_spectra(3000, 256, 6, rank=16, seed=seed, outlier_frac=0.1)
    Xt = O.synth_spectra(600, 256, 6, rank=16, seed=seed, outlier_frac=0.3)
    return X[:2700], np.zeros(2700, dtype=np.int64), Xt


@pytest.fixture(scope="module")
def fitted():
    """The data of smoke(): one class, k = 6, 600 test rows of which the last 180 are outliers."""
    from oracle import simca_oracle as O
    from utils import SIMCA

    X, y, Xt = smoke_data()
    est = SIMCA(n_components=6, model_class=0, verbose=False).fit(X, y)
    orc = O.OracleSIMCA(n_components=6, model_class=0).fit(X, y)
    return est, orc, Xt


@pytest.mark.parametrize("kind", ["sim", "alt", "ci", "dd"])
def test_decision_function_vs_oracle(kind):
    from oracle import simca_oracle as O
    from utils import SIMCA

    X, y, Xt = smoke_data()
    est = SIMCA(n_components=6, model_class=0, type=kind, verbose=False).fit(X, y)
    orc = O.OracleSIMCA(n_components=6, model_class=0, type=kind).fit(X, y)
    df = est.decision_function(Xt)
    assert isinstance(df, np.ndarray) and df.shape == (600, 1) and df.dtype == np.float64
    dlim = float(orc._model[0]["D_limit"])
    ref = dlim - orc.dred(Xt, 0)
    np.testing.assert_allclose(df[:, 0], ref, rtol=1e-4, atol=1e-4 * dlim)
    assert np.array_equal(est.predict(Xt)[:, 0], (df[:, 0] > 0).astype(np.float64))
    dft = est.decision_function(torch.from_numpy(Xt).cuda())
    assert isinstance(dft, torch.Tensor) and dft.is_cuda and np.array_equal(dft.cpu().numpy(), df)


def test_decision_function_two_classes():
    from oracle import simca_oracle as O
    from utils import SIMCA

    Xa = O.synth_spectra(1500, 256, 4, rank=16, seed=21)
    Xb = O.synth_spectra(1500, 256, 6, rank=16, seed=22) + np.float32(0.5)
    X = np.concatenate([Xa, Xb])
    y = np.repeat([0, 1], 1500)
    Xt = np.concatenate([O.synth_spectra(200, 256, 4, rank=16, seed=21, outlier_frac=0.3),
                         O.synth_spectra(200, 256, 6, rank=16, seed=22, outlier_frac=0.3) + np.float32(0.5)])
    est = SIMCA(n_components=[4, 6], verbose=False).fit(X, y)
    orc = O.OracleSIMCA(n_components=[4, 6]).fit(X, y)
    df = est.decision_function(Xt)
    pred = est.predict(Xt)
    assert df.shape == (400, 2)
    assert np.array_equal(pred, (df > 0).astype(np.float64))
    for i, cls in enumerate([0, 1]):
        dlim = float(orc._model[cls]["D_limit"])
        np.testing.assert_allclose(df[:, i], dlim - orc.dred(Xt, cls), rtol=1e-4, atol=1e-4 * dlim)
    with pytest.raises(ValueError):
        est.contributions(Xt)
    r = est.contributions(Xt, cls=1, groups="decision")
    assert np.array_equal(r.counts, [int(pred[:, 1].sum()), 400 - int(pred[:, 1].sum())])


def outlier_columns(p):
    """The columns synth_spectra's outlier band lifts by at least half its peak
    (a Gaussian at wl = 0.5, σ = 0.03)."""
    wl = np.linspace(0.0, 1.0, p)
    return np.flatnonzero(np.exp(-0.5 * ((wl - 0.5) / 0.03) ** 2) >= 0.5)


def test_contributions_decision_groups():
    """smoke()'s shapes with seed 19 instead of 11: with seed 11 the model's loadings absorb most
    of the outlier band (the class accepts 177 of the 180 outliers) and the fp64 reference
    profiles of the two decision groups do not separate there (ratio 0.42 on the worst column);
    with seed 19 they separate by 4.4× or more on every band column."""
    from oracle import simca_oracle as O
    from utils import SIMCA

    X, y, Xt = smoke_data(seed=19)
    est = SIMCA(n_components=6, model_class=0, verbose=False).fit(X, y)
    orc = O.OracleSIMCA(n_components=6, model_class=0).fit(X, y)
    pred = est.predict(Xt)[:, 0]
    r = est.contributions(Xt, groups="decision")
    assert all(isinstance(v, np.ndarray) for v in (r.Q, r.T2, r.q_profile, r.t2_profile, r.counts))
    assert r.E is None and r.C is None
    n_acc = int(pred.sum())
    assert np.array_equal(r.counts, [n_acc, 600 - n_acc]) and 0 < n_acc < 600
    T2, _, Q, _ = est.transform(Xt)
    np.testing.assert_allclose(r.T2, T2, rtol=1e-4, atol=1e-5 * np.median(T2))
    np.testing.assert_allclose(r.Q, Q, rtol=1e-4, atol=1e-5 * np.median(Q))
    assert r.q_profile.shape == (2, 256) and r.q_profile.dtype == np.float64
    # the fp64 reference separates the groups on the outlier band by more than 2×
    cols = outlier_columns(256)
    mo = orc._model[0]
    Y = Xt.astype(np.float64) - mo["mean_pred"]
    E = Y - (Y @ mo["P_pred"].T) @ mo["P_pred"]
    acc = orc.predict(Xt)[:, 0] == 1
    ref_acc, ref_rej = (E[acc] ** 2).mean(0), (E[~acc] ** 2).mean(0)
    assert (ref_rej[cols] >= 2.0 * ref_acc[cols]).all()
    mean_acc, mean_rej = r.q_profile[0] / r.counts[0], r.q_profile[1] / r.counts[1]
    assert (mean_rej[cols] > mean_acc[cols]).all()


def test_contributions_matrices_and_return_types(fitted):
    est, _, Xt = fitted
    fit = est._fits[0]
    P, mu, a = (t.cpu().numpy() for t in (fit.P64, fit.mean64, fit.inv_diag))
    gid = np.arange(600) % 3
    r = est.contributions(Xt, groups=gid, matrices=True)
    assert isinstance(r.E, np.ndarray) and r.E.dtype == np.float32 and r.E.shape == (600, 256)
    assert isinstance(r.C, np.ndarray) and r.C.dtype == np.float32
    assert np.array_equal(r.counts, [200, 200, 200]) and r.t2_profile.shape == (3, 256)
    Y, E64, C64 = ref64(Xt, P, mu, a)
    E32, C32 = ref32(Xt, P, mu, a)
    ymax = float(np.abs(Y).max())
    for got, r64, r32 in ((r.E, E64, E32), (r.C, C64, C32)):
        bound = 2.0 * float(np.abs(r32.astype(np.float64) - r64).max()) + 8.0 * EPS32 * ymax
        assert float(np.abs(got.astype(np.float64) - r64).max()) <= bound
    rt = est.contributions(torch.from_numpy(Xt).cuda(), groups=gid, matrices=True)
    for name in ("Q", "T2", "q_profile", "t2_profile", "counts", "E", "C"):
        v = getattr(rt, name)
        assert isinstance(v, torch.Tensor) and v.is_cuda, name
        assert np.array_equal(v.cpu().numpy(), getattr(r, name)), name
    r64_ = est.contributions(Xt.astype(np.float64), matrices=True)
    assert r64_.E.dtype == np.float64 and r64_.C.dtype == np.float64 and r64_.Q.dtype == np.float64
    assert float(np.abs(r64_.E - E64).max()) <= 1e-10 * ymax
    assert float(np.abs(r64_.C - C64).max()) <= 1e-10 * ymax


def test_contributions_lazy_view_bit_identical():
    """A lazy view against the eagerly preprocessed tensor, two ways.

    Bit for bit against the view's materialised rows (ocm_prep_apply_f32, what a write-through view
    stores as X′): the view's groups come from the fused scoring path, its E / C from the plain kernel
    on the rows the engine materialises.

    Against the stand-alone eager pass `snv_savgol(X, 5, 2, 1)` the issue asks for bit identity too, on
    the premise that both give bit-identical rows.  They do not: that pass (ocm_snv_savgol_f32, fp64
    taps) and the view's transform round differently, and tests/test_gpu_prep.py holds them to
    d = 3e-6·max|X′|.  So this comparison is at the tolerance that input difference allows:
    E = (I − PᵀP)·y is a projection, so |ΔE_j| ≤ ‖Δy‖₂ ≤ √p·d; with s = Pᵀ(a·t), |Δs_j| ≤ max(a)·√p·d
    and ΔC = Δy·s + y·Δs; plus the f32 rounding floor of the kernel checks (8·eps·max|y|, and times
    max|s| for C), once for each side.  Decisions must agree on every row that is not within 1e-4 of
    the limit (smoke()'s margin)."""
    from ocm.preprocess import snv_savgol
    from utils import SIMCA

    X, y, Xt = smoke_data()
    Xd, Xtd = torch.from_numpy(X).cuda(), torch.from_numpy(Xt).cuda()
    est = SIMCA(n_components=6, model_class=0, verbose=False).fit(snv_savgol(Xd, 5, 2, 1), y)
    view = snv_savgol(Xtd, 5, 2, 1, lazy=True)
    mat = est.contributions(view.materialize(), groups="decision", matrices=True)
    lazy = est.contributions(snv_savgol(Xtd, 5, 2, 1, lazy=True), groups="decision", matrices=True)
    assert 0 < int(mat.counts[0]) and int(mat.counts.sum()) == 600
    for name in ("Q", "T2", "q_profile", "t2_profile", "counts", "E", "C"):
        assert torch.equal(getattr(mat, name), getattr(lazy, name)), name
    # the independent eager pass
    Xe = snv_savgol(Xtd, 5, 2, 1)
    eager = est.contributions(Xe, groups="decision", matrices=True)
    fit = est._fits[0]
    P, mu, a = (t.cpu().numpy() for t in (fit.P64, fit.mean64, fit.inv_diag))
    Ye = Xe.double().cpu().numpy() - mu
    S = ((Ye @ P.T) * a) @ P
    p = Ye.shape[1]
    d = 3e-6 * float(Xe.abs().max())
    ymax, smax = float(np.abs(Ye).max()), float(np.abs(S).max())
    tol_E = np.sqrt(p) * d + 2 * 8 * EPS32 * ymax
    tol_C = d * smax + ymax * float(a.max()) * np.sqrt(p) * d + 2 * 8 * EPS32 * ymax * smax
    dE = float((lazy.E - eager.E).abs().max())
    dC = float((lazy.C - eager.C).abs().max())
    print(f"lazy view vs eager pass: max |ΔE| {dE:.3e} (tolerance {tol_E:.3e}), max |ΔC| {dC:.3e} ({tol_C:.3e})")
    assert dE <= tol_E and dC <= tol_C
    assert float(lazy.E.abs().max()) > 100 * tol_E  # the comparison would notice a missing transform
    df_e = est.decision_function(Xe)[:, 0]
    df_v = est.decision_function(snv_savgol(Xtd, 5, 2, 1, lazy=True))[:, 0]
    clear = df_e.abs() > 1e-4 * float(est._model[0]["D_limit"])
    assert torch.equal(df_e[clear] > 0, df_v[clear] > 0)
    if bool(clear.all()):
        assert torch.equal(lazy.counts, eager.counts)
