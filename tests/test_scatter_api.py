"""MSC / EMSC on the host: the weight builder against NumPy's least squares,
the argument checks (raised before any device work) and the replica
fingerprint of views built from different references."""
import numpy as np
import pytest
import torch

from ocm import replica
from ocm.preprocess import EMSC, MSC, scatter_basis, scatter_weights
from ocm.prepview import PrepView


def _reference(p, seed=0):
    """A smooth positive spectrum on a raw baseline."""
    rng = np.random.default_rng(seed)
    wl = np.linspace(0.0, 1.0, p)
    return 100.0 + np.exp(-0.5 * ((wl - 0.4) / 0.15) ** 2) + 0.3 * np.sin(7.0 * wl) + 0.01 * rng.standard_normal(p)


def _rows(p, n=6, seed=1):
    rng = np.random.default_rng(seed)
    ref = _reference(p)
    lam = np.linspace(-1.0, 1.0, p)
    a, b = rng.uniform(-2, 2, (n, 1)), rng.uniform(0.5, 2, (n, 1))
    d1, d2 = rng.uniform(-1, 1, (n, 1)), rng.uniform(-1, 1, (n, 1))
    return a + b * ref + d1 * lam + d2 * lam ** 2 + 0.01 * rng.standard_normal((n, p))


@pytest.mark.parametrize("p", [7, 37, 256])
def test_msc_weights_match_polyfit(p):
    ref = _reference(p)
    W = MSC(reference=ref).weights_
    assert W.shape == (2, p) and W.dtype == np.float64
    for x in _rows(p):
        slope, icpt = np.polyfit(ref, x, 1)
        np.testing.assert_allclose(W @ x, [icpt, slope], rtol=1e-9)


@pytest.mark.parametrize("p", [7, 37, 256])
def test_emsc_weights_match_lstsq(p):
    ref = _reference(p)
    inter = np.cos(5.0 * np.linspace(0.0, 1.0, p))
    for est in (EMSC(degree=2, reference=ref), EMSC(degree=1, reference=ref, interferents=inter),
                EMSC(degree=2, reference=ref, wavelengths=np.linspace(900.0, 1700.0, p))):
        B, W = est.basis_, est.weights_
        assert B.dtype == np.float64 and W.shape == B.shape
        np.testing.assert_array_equal(B[0], np.ones(p))
        np.testing.assert_array_equal(B[1], ref)
        np.testing.assert_array_equal(est.reference_, ref)
        X = _rows(p)
        want = np.linalg.lstsq(B.T, X.T, rcond=None)[0].T
        np.testing.assert_allclose(X @ W.T, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    # the default abscissa, and a user's wavelengths mapped affinely onto it
    np.testing.assert_allclose(EMSC(degree=2, reference=ref).basis_[2], np.linspace(-1.0, 1.0, p), atol=1e-15)
    np.testing.assert_allclose(EMSC(degree=2, reference=ref, wavelengths=np.linspace(900.0, 1700.0, p)).basis_[3],
                               np.linspace(-1.0, 1.0, p) ** 2, atol=1e-12)


def test_emsc_degree0_is_msc():
    ref = _reference(37)
    a, b = EMSC(degree=0, reference=ref), MSC(reference=ref)
    np.testing.assert_array_equal(a.weights_, b.weights_)
    np.testing.assert_array_equal(a.basis_, b.basis_)
    np.testing.assert_array_equal(scatter_weights(scatter_basis(ref)), b.weights_)


def test_validation_errors_need_no_device():
    ref = _reference(37)
    X = np.zeros((4, 36), dtype=np.float32)
    for est in (MSC(reference=ref), EMSC(degree=2, reference=ref)):
        with pytest.raises(ValueError, match="like the reference"):  # a reference of the wrong length
            est.transform(X)
    with pytest.raises(ValueError, match="at most 8"):  # q = 9
        EMSC(degree=7, reference=ref)
    with pytest.raises(ValueError, match="at most 8"):
        EMSC(degree=7)
    with pytest.raises(ValueError, match="at most 8"):
        EMSC(degree=2, reference=ref, interferents=np.random.default_rng(0).standard_normal((5, 37)))
    with pytest.raises(ValueError, match="cannot determine"):  # p < q
        EMSC(degree=2, reference=ref[:3])
    with pytest.raises(ValueError, match="constant"):
        MSC(reference=np.full(37, 3.0))
    with pytest.raises(ValueError, match="constant"):
        EMSC(degree=2, reference=np.full(37, 3.0))
    with pytest.raises(ValueError, match="linearly dependent"):
        EMSC(degree=1, reference=ref, interferents=2.0 * ref)
    with pytest.raises(ValueError, match="fit"):
        MSC().transform(np.zeros((4, 37), dtype=np.float32))
    with pytest.raises(ValueError, match="lazy must be"):
        MSC(reference=ref).transform(np.zeros((4, 37), dtype=np.float32), lazy="yes")
    with pytest.raises(ValueError):  # the filter's own checks come before the device too
        MSC(reference=ref).transform(np.zeros((4, 37), dtype=np.float32), window_length=4)


def test_emsc_lazy_raises_and_names_the_eager_route():
    ref = _reference(37)
    X = np.zeros((4, 37), dtype=np.float32)
    for lazy in (True, "write"):
        with pytest.raises(ValueError, match=r"eager transform\(X\)"):
            EMSC(degree=2, reference=ref).transform(X, lazy=lazy)


def _host_view(X, kind, snv, stat_key, rowstat):
    """A PrepView over host rows (the class wraps device tensors only): the
    fields ocm.replica.fingerprint reads."""
    v = PrepView.__new__(PrepView)
    v.__dict__.update(X=X, window=5, polyorder=2, deriv=1, delta=1.0, snv=snv, kind=kind, stat_key=stat_key,
                      through=False, _taps=None, _rowstat=rowstat, _xp=None)
    return v


def test_views_from_different_references_have_different_fingerprints():
    p = 37
    X = torch.from_numpy(_rows(p, n=40).astype(np.float32))
    y = np.zeros(40, dtype=np.int64)
    a, b = MSC(reference=_reference(p, seed=0)), MSC(reference=_reference(p, seed=5))
    assert a._key != b._key
    rs = torch.zeros((40, 2))
    va, va2, vb = (_host_view(X, "msc", False, m._key, rs) for m in (a, MSC(reference=_reference(p, seed=0)), b))
    fa, fa2, fb = (replica.fingerprint(v, y) for v in (va, va2, vb))
    assert np.array_equal(fa, fa2)  # the same reference on two ranks: replicated
    assert not np.array_equal(fa, fb)  # different references: not taken for replicated
    snv = _host_view(X, "snv", True, 0, None)
    assert not np.array_equal(replica.fingerprint(snv, y), fa)
    assert np.array_equal(replica.fingerprint(snv, y), replica.fingerprint(_host_view(X, "snv", True, 0, None), y))
    assert "kind='msc'" in repr(va)
