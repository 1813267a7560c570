"""Whittaker smoothing and AsLS baselines on the GPU (ocm_whittaker_f32,
ocm_asls_f32) against the fp64 banded oracle of tests/baseline_oracle.py.

Bound (derived, not tuned): a backward-stable banded solve has forward error
≤ c·κ·ε₆₄ with κ ≤ (w_max + 4ᵈλ) / w_min.  Per row s = 4·κ·ε₆₄·max|x_row| and
|out − ref₆₄| ≤ ulp₃₂(|ref₆₄|) + s, likewise for x − z.  The tests assert
worst_ratio ≤ 1, the largest error in units of that bound."""
import contextlib
import io

import numpy as np
import pytest
import torch

from baseline_oracle import ORDERS, PADS, SHAPES, asls_case, slack, spectra, whittaker_ref, worst_ratio
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

LAMS = [1e2, 1e5]  # the second for p ≤ 256 only
ASLS_SETTINGS = [(1e2, 0.05), (1e5, 0.01)]  # (λ, asym); the second for p ≤ 256 only


def lams_for(p, settings=LAMS):
    return settings if p <= 256 else settings[:1]


def on_device(X, pad=0):
    """The rows on the device, contiguous (pad = 0) or as a slice of a wider tensor."""
    m, p = X.shape
    buf = torch.zeros((m, p + pad), dtype=torch.float32, device="cuda")
    buf[:, :p] = torch.from_numpy(np.array(X, dtype=np.float32)).cuda()
    Xd = buf[:, :p]
    assert Xd.stride(0) == p + pad
    return Xd


def host(t):
    return t.detach().cpu().numpy()


def raw_whittaker(Xd, lam, d, W=None, ldw=0):
    """ocm_whittaker_f32 as the C ABI exposes it: (rc, out, nbad); out is a padded tensor's slice."""
    from ocm import _lib

    m, p = Xd.shape
    buf = torch.full((m, p + 5), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[:, :p]
    nbad = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.load().ocm_whittaker_f32(_lib.Context.get(Xd.device.index).handle, _lib.ptr(Xd), Xd.stride(0), m, p,
                                       _lib.ptr(W), ldw, lam, d, _lib.ptr(out), out.stride(0), _lib.ptr(nbad),
                                       _lib.stream_handle(Xd.device))
    torch.cuda.synchronize()
    assert torch.isnan(buf[:, p:]).all()  # nothing written past the rows
    return rc, out, int(nbad.item())


def raw_asls(Xd, lam, asym, d, n_iter, subtract):
    from ocm import _lib

    m, p = Xd.shape
    buf = torch.full((m, p + 5), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[:, :p]
    iters = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.load().ocm_asls_f32(_lib.Context.get(Xd.device.index).handle, _lib.ptr(Xd), Xd.stride(0), m, p, lam,
                                  asym, d, n_iter, subtract, _lib.ptr(out), out.stride(0), _lib.ptr(iters),
                                  _lib.stream_handle(Xd.device))
    torch.cuda.synchronize()
    assert torch.isnan(buf[:, p:]).all()
    return rc, out, iters


# ------------------------------------------------------------------ 1. shared weights
@pytest.mark.parametrize("d", ORDERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("m,p", SHAPES)
def test_whittaker_shared_weights(m, p, pad, d):
    """w = None and a (p,) vector uniform in [0.05, 1], through the C ABI and through Python."""
    from ocm.preprocess import whittaker

    X = spectra(m, p)
    Xd = on_device(X, pad)
    wv = np.random.default_rng(3000 + p).uniform(0.05, 1.0, p).astype(np.float32)
    wd = torch.from_numpy(wv).cuda()
    for lam in lams_for(p):
        for w, w_dev, w_min in ((None, None, 1.0), (wv, wd, float(wv.min()))):
            ref = whittaker_ref(X, lam, d, w)
            s = slack(X, lam, d, w_min)
            rc, out, nbad = raw_whittaker(Xd, lam, d, w_dev, 0)
            assert rc == 0 and nbad == 0
            r_raw = worst_ratio(host(out), ref, s)
            got = whittaker(Xd, lam, d, weights=w)
            assert got.shape == (m, p) and got.dtype == torch.float32 and got.is_contiguous()
            r_py = worst_ratio(host(got), ref, s)
            print(f"whittaker shared m={m} p={p} pad={pad} d={d} lam={lam:g} w={'1' if w is None else 'vec'}: "
                  f"ratio raw {r_raw:.3f} python {r_py:.3f}")
            assert r_raw <= 1.0 and r_py <= 1.0
            assert torch.equal(got, out)


# ------------------------------------------------------------------ 2. shared weights with zeros
@pytest.mark.parametrize("d", ORDERS)
@pytest.mark.parametrize("m,p,run", [(5, 7, 2), (33, 37, 8), (64, 256, 8)])
def test_whittaker_shared_weights_with_zeros(m, p, run, d):
    """The first d, the last d and an interior run of columns carry no weight; κ is np.linalg.cond of
    the dense fp64 matrix."""
    from ocm.preprocess import whittaker

    X = spectra(m, p)
    wv = np.random.default_rng(3100 + p).uniform(0.05, 1.0, p).astype(np.float32)
    wv[:d] = 0.0
    wv[p - d:] = 0.0
    # p = 7, d = 2: the edges leave three columns, and a run of two would leave one weight (a singular
    # system, which the host check refuses): the run is one column there, so that d weights remain
    run = min(run, p - 3 * d)
    mid = d if p == 7 else p // 2 - run // 2
    wv[mid:mid + run] = 0.0
    assert (wv > 0).sum() >= d and (wv[d:p - d] == 0).sum() == run
    D = np.diff(np.eye(p), d, axis=0)
    for lam in LAMS:
        kappa = np.linalg.cond(np.diag(wv.astype(np.float64)) + lam * D.T @ D)
        ref = whittaker_ref(X, lam, d, wv)
        s = slack(X, lam, d, None, kappa=kappa)
        for pad in PADS:
            got = whittaker(on_device(X, pad), lam, d, weights=wv)
            r = worst_ratio(host(got), ref, s)
            print(f"whittaker zeros m={m} p={p} pad={pad} d={d} lam={lam:g} cond={kappa:.3g}: ratio {r:.3f}")
            assert r <= 1.0


# ------------------------------------------------------------------ 3. per-row weights
ASYM_W = 0.01  # the weights of the per-row test are uniform in [ASYM_W, 1]


def row_weights(m, p):
    return np.random.default_rng(3200 + p).uniform(ASYM_W, 1.0, (m, p)).astype(np.float32)


@pytest.mark.parametrize("d", ORDERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("m,p", SHAPES)
def test_whittaker_row_weights(m, p, pad, d):
    """The row-specific factorisation AsLS runs, with no weight decisions in the way; ldw = p and padded."""
    from ocm.preprocess import whittaker

    X = spectra(m, p)
    Xd = on_device(X, pad)
    W = row_weights(m, p)
    for lam in lams_for(p):
        ref = whittaker_ref(X, lam, d, W)
        s = slack(X, lam, d, ASYM_W)
        Wd = on_device(W, pad)
        rc, out, nbad = raw_whittaker(Xd, lam, d, Wd, Wd.stride(0))
        assert rc == 0 and nbad == 0
        r_raw = worst_ratio(host(out), ref, s)
        got = whittaker(Xd, lam, d, weights=Wd)
        r_py = worst_ratio(host(got), ref, s)
        got_h = whittaker(Xd, lam, d, weights=W)  # host weights
        print(f"whittaker rows m={m} p={p} pad={pad} d={d} lam={lam:g}: ratio raw {r_raw:.3f} python {r_py:.3f}")
        assert r_raw <= 1.0 and r_py <= 1.0
        assert torch.equal(got, out) and torch.equal(got_h, out)


# ------------------------------------------------------------------ 4. AsLS
@pytest.mark.parametrize("d", ORDERS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("m,p", SHAPES)
def test_asls_vs_oracle(m, p, pad, d):
    """Baseline and corrected rows after at most ten solves.  A weight decision within rounding of a tie
    may differ from the oracle's and changes the later iterates: a row whose oracle margin is below 4·s
    is left out, at most one per case; the compared rows ran the oracle's number of solves."""
    from ocm.preprocess import asls

    X = spectra(m, p)
    Xd = on_device(X, pad)
    X64 = X.astype(np.float64)
    for lam, asym in lams_for(p, ASLS_SETTINGS):
        Z, iters, margin = asls_case(m, p, lam, asym, d)
        s = slack(X, lam, d, min(asym, 1.0 - asym))
        keep = margin >= 4.0 * s[:, 0]
        assert (~keep).sum() <= 1, f"{(~keep).sum()} rows near a tie"
        base, it_b = asls(Xd, lam, asym, 10, d, subtract=False, return_iters=True)
        corr, it_c = asls(Xd, lam, asym, 10, d, subtract=True, return_iters=True)
        rc, raw, it_r = raw_asls(Xd, lam, asym, d, 10, 1)
        assert rc == 0 and torch.equal(raw, corr) and torch.equal(it_r, it_c) and torch.equal(it_b, it_c)
        assert base.is_contiguous() and base.dtype == torch.float32 and it_b.dtype == torch.int32
        r_b = worst_ratio(host(base)[keep], Z[keep], s[keep])
        r_c = worst_ratio(host(corr)[keep], (X64 - Z)[keep], s[keep])
        print(f"asls m={m} p={p} pad={pad} d={d} lam={lam:g} asym={asym}: ratio baseline {r_b:.3f} corrected "
              f"{r_c:.3f}, left out {(~keep).sum()}, iters {iters.min()}..{iters.max()}")
        assert r_b <= 1.0 and r_c <= 1.0
        np.testing.assert_array_equal(host(it_b)[keep], iters[keep])


@pytest.mark.parametrize("d", ORDERS)
def test_asls_stops_early_and_counts_solves(d):
    """n_iter far above what the rows need: the result and iters are those of the oracle's early stop,
    and equal the run with n_iter = max(iters) bit for bit."""
    from baseline_oracle import asls_ref
    from ocm.preprocess import asls

    m, p, lam, asym = 70, 256, 1e2, 0.05
    X = spectra(m, p)
    Z, iters, margin = asls_ref(X, lam, asym, 40, d)
    assert iters.max() < 40  # every row stopped by itself
    s = slack(X, lam, d, asym)
    keep = margin >= 4.0 * s[:, 0]
    assert (~keep).sum() <= 1
    Xd = on_device(X)
    base, it = asls(Xd, lam, asym, 40, d, subtract=False, return_iters=True)
    np.testing.assert_array_equal(host(it)[keep], iters[keep])
    assert worst_ratio(host(base)[keep], Z[keep], s[keep]) <= 1.0
    again, it2 = asls(Xd, lam, asym, int(it.max()), d, subtract=False, return_iters=True)
    assert torch.equal(again, base) and torch.equal(it2, it)


# ------------------------------------------------------------------ 5. one iteration is the smoother
@pytest.mark.parametrize("d", ORDERS)
@pytest.mark.parametrize("m,p", [(5, 7), (70, 1000)])
def test_asls_one_iteration_is_whittaker(m, p, d):
    from ocm.preprocess import asls, whittaker

    Xd = on_device(spectra(m, p), 3)
    z, it = asls(Xd, 1e2, 0.05, 1, d, subtract=False, return_iters=True)
    assert torch.equal(z, whittaker(Xd, 1e2, d))
    assert (it == 1).all()


# ------------------------------------------------------------------ 6. row independence
@pytest.mark.parametrize("d", ORDERS)
def test_rows_are_independent_and_runs_repeat(d):
    """Rows 0, 32 and 69 computed alone, from another leading dimension, equal the batch bit for bit."""
    from ocm.preprocess import asls, whittaker

    m, p, lam, asym = 70, 1000, 1e2, 0.05
    X, W = spectra(m, p), row_weights(m, p)
    Xd, Wd = on_device(X), on_device(W)
    zw = whittaker(Xd, lam, d, weights=Wd)
    za, ia = asls(Xd, lam, asym, 10, d, return_iters=True)
    assert torch.equal(zw, whittaker(Xd, lam, d, weights=Wd))
    za2, ia2 = asls(Xd, lam, asym, 10, d, return_iters=True)
    assert torch.equal(za, za2) and torch.equal(ia, ia2)
    for r in (0, 32, 69):
        x1, w1 = on_device(X[r:r + 1], 3), on_device(W[r:r + 1], 3)
        assert torch.equal(whittaker(x1, lam, d, weights=w1)[0], zw[r])
        z1, i1 = asls(x1, lam, asym, 10, d, return_iters=True)
        assert torch.equal(z1[0], za[r]) and int(i1[0]) == int(ia[r])


# ------------------------------------------------------------------ 7. polynomials are reproduced
@pytest.mark.parametrize("d", ORDERS)
@pytest.mark.parametrize("m,p", [(5, 7), (33, 37), (64, 256)])
def test_polynomials_are_reproduced(m, p, d):
    """D annihilates a constant (d = 1) or an affine row (d = 2): z = x for every λ and every weight
    vector.  The rows are exact in float32 (half-integer offsets, slopes −1, 0, 1 per column).
    whittaker: the bound of test 1 (w = 1).  asls: its weights are asym and 1 − asym, so its κ has
    w_min = asym; the baseline is within that bound of x and the corrected row within it of 0."""
    from ocm.preprocess import asls, whittaker

    i, j = np.arange(m, dtype=np.float64)[:, None], np.arange(p, dtype=np.float64)
    E64 = i - 2.5 + (j * (i % 3 - 1) if d == 2 else 0.0 * j)
    E = E64.astype(np.float32)
    assert np.array_equal(E.astype(np.float64), E64)
    Ed = on_device(E, 3)
    for lam in LAMS:
        r_w = worst_ratio(host(whittaker(Ed, lam, d)), E64, slack(E, lam, d, 1.0))
        print(f"polynomial m={m} p={p} d={d} lam={lam:g}: ratio whittaker {r_w:.3f}")
        assert r_w <= 1.0
        for asym in (0.05, 0.01):
            sa = slack(E, lam, d, asym)
            r_b = worst_ratio(host(asls(Ed, lam, asym, 10, d, subtract=False)), E64, sa)
            r_c = worst_ratio(host(asls(Ed, lam, asym, 10, d)), np.zeros_like(E64), sa)
            print(f"polynomial m={m} p={p} d={d} lam={lam:g} asym={asym}: ratio asls baseline {r_b:.3f} corrected "
                  f"{r_c:.3f}")
            assert r_b <= 1.0 and r_c <= 1.0


# ------------------------------------------------------------------ 8. failed rows
@pytest.mark.parametrize("d", ORDERS)
def test_a_row_without_weights_fails_alone(d):
    from ocm.preprocess import whittaker

    m, p, lam, bad = 70, 37, 1e2, 41
    X, W = spectra(m, p), row_weights(m, p)
    Xd = on_device(X)
    rc, good, nbad = raw_whittaker(Xd, lam, d, on_device(W), p)
    assert rc == 0 and nbad == 0 and torch.isfinite(good).all()
    W0 = W.copy()
    W0[bad] = 0.0
    W0d = on_device(W0)
    rc, out, nbad = raw_whittaker(Xd, lam, d, W0d, p)
    assert rc == 0 and nbad == 1
    assert torch.isnan(out[bad]).all()
    others = [r for r in range(m) if r != bad]
    assert torch.equal(out[others], good[others])
    with pytest.raises(ValueError, match="not positive definite"):
        whittaker(Xd, lam, d, weights=W0d)
    Wn = W.copy()
    Wn[3, 5] = np.nan
    Wn[9, 0] = -1.0
    rc, out, nbad = raw_whittaker(Xd, lam, d, on_device(Wn), p)
    assert rc == 0 and nbad == 2 and torch.isnan(out[3]).all() and torch.isnan(out[9]).all()
    # a shared vector that leaves the system singular fails every row
    wz = torch.zeros(p, dtype=torch.float32, device="cuda")
    rc, out, nbad = raw_whittaker(Xd, lam, d, wz, 0)
    assert rc == 0 and nbad == m and torch.isnan(out).all()


def test_argument_checks_of_the_c_abi():
    from ocm import _lib

    Xd = on_device(spectra(5, 7))
    lib, h, st = _lib.load(), _lib.Context.get(0).handle, _lib.stream_handle(Xd.device)
    out = torch.empty_like(Xd)
    P = _lib.ptr
    for args in ((7, 7, 1e2, 3, 7), (7, 7, 0.0, 2, 7), (7, 7, float("nan"), 2, 7), (6, 7, 1e2, 2, 7),
                 (7, 7, 1e2, 2, 6), (7, 2, 1e2, 2, 7)):
        ldx, p, lam, d, ldo = args
        assert lib.ocm_whittaker_f32(h, P(Xd), ldx, 5, p, None, 0, lam, d, P(out), ldo, None, st) == _lib.OCM_ERR_ARG
        assert lib.ocm_asls_f32(h, P(Xd), ldx, 5, p, lam, 0.05, d, 10, 1, P(out), ldo, None, st) == _lib.OCM_ERR_ARG
    assert lib.ocm_whittaker_f32(h, P(Xd), 7, 5, 7, P(Xd), 3, 1e2, 2, P(out), 7, None, st) == _lib.OCM_ERR_ARG
    assert lib.ocm_whittaker_f32(h, P(Xd), 7, 1 << 31, 7, None, 0, 1e2, 2, P(out), 7, None, st) == _lib.OCM_ERR_ARG
    for asym, n_iter in ((0.0, 10), (1.0, 10), (0.05, 0)):
        assert lib.ocm_asls_f32(h, P(Xd), 7, 5, 7, 1e2, asym, 2, n_iter, 1, P(out), 7, None, st) == _lib.OCM_ERR_ARG
    assert lib.ocm_asls_f32(h, P(Xd), 7, 0, 7, 1e2, 0.05, 2, 10, 1, P(out), 7, None, st) == 0  # m = 0: nothing to do


# ------------------------------------------------------------------ 9. composition
def test_result_feeds_the_downstream_stages():
    """asls(X) is an ordinary contiguous float32 device matrix: the filter and the estimator give the
    same on it as on a copy made through the host."""
    from ocm.preprocess import AsLS, asls, snv_savgol
    from utils import SIMCA

    n, p, k = 600, 256, 4
    X = spectra(n, p)
    Xd = on_device(X, 3)
    est = AsLS(1e2, 0.05, 10, 2).fit(Xd)
    Y = est.transform(Xd)
    assert Y.is_cuda and Y.dtype == torch.float32 and Y.shape == (n, p) and Y.is_contiguous()
    assert est.iters_.shape == (n,) and int(est.iters_.min()) >= 2 and int(est.iters_.max()) <= 10
    assert torch.equal(Y, asls(Xd, 1e2, 0.05, 10, 2))
    assert torch.equal(est.baseline(Xd), asls(Xd, 1e2, 0.05, 10, 2, subtract=False))
    out = torch.empty((n, p + 2), dtype=torch.float32, device="cuda")[:, :p]
    assert asls(Xd, 1e2, 0.05, 10, 2, out=out) is out and torch.equal(out, Y)
    copy = torch.from_numpy(host(Y).copy()).cuda()
    assert torch.equal(snv_savgol(Y, 5, 2, 1), snv_savgol(copy, 5, 2, 1))
    y = np.zeros(n, dtype=np.int64)
    res = []
    for data in (Y, copy):
        with contextlib.redirect_stdout(io.StringIO()):
            model = SIMCA(n_components=k, model_class=0, verbose=False).fit(data[:500], y[:500])
            pred = model.predict(data[500:])
            res.append(host(pred) if isinstance(pred, torch.Tensor) else np.asarray(pred))
    np.testing.assert_array_equal(res[0], res[1])
    assert res[0].size == 100
