"""Whittaker / AsLS on the host: the band builder against np.diff, the fp64
oracle against a dense solve, and the argument checks, all raised before any
device work (this file needs no device)."""
import numpy as np
import pytest
import torch

from baseline_oracle import asls_ref, whittaker_ref
from ocm import preprocess
from ocm.preprocess import AsLS, asls, whittaker, whittaker_bands


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("p", [3, 7, 37])
def test_bands_match_np_diff(p, d):
    D = np.diff(np.eye(p), d, axis=0)
    A = D.T @ D
    ab = whittaker_bands(p, d)
    assert ab.shape == (d + 1, p) and ab.dtype == np.float64
    for k in range(d + 1):
        np.testing.assert_array_equal(ab[k, :p - k], np.diagonal(A, -k))
        np.testing.assert_array_equal(ab[k, p - k:], 0.0)  # solveh_banded's padding
    for k in range(d + 1, p):
        assert not np.diagonal(A, -k).any()  # half bandwidth d


def test_names_are_exported():
    for name in ("whittaker_bands", "whittaker", "asls", "AsLS"):
        assert name in preprocess.__all__ and hasattr(preprocess, name)


@pytest.mark.parametrize("d", [1, 2])
def test_oracle_matches_a_dense_solve(d):
    rng = np.random.default_rng(5)
    p, lam = 37, 50.0
    X = rng.standard_normal((4, p)).cumsum(axis=1)
    w = rng.uniform(0.05, 1.0, (4, p))
    D = np.diff(np.eye(p), d, axis=0)
    for i in range(4):
        z = np.linalg.solve(np.diag(w[i]) + lam * D.T @ D, w[i] * X[i])
        np.testing.assert_allclose(whittaker_ref(X[i:i + 1], lam, d, w[i:i + 1])[0], z, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(whittaker_ref(X[i:i + 1], lam, d, w[i])[0], z, rtol=1e-9, atol=1e-12)
    Z, iters, margin = asls_ref(X, lam, 0.05, 10, d)
    assert Z.shape == X.shape and ((iters >= 2) & (iters <= 10)).all() and (margin >= 0).all()
    # the baseline lies below most of the row
    assert ((X > Z).mean(axis=1) > 0.5).all()


def test_validation_errors_need_no_device():
    X = np.zeros((4, 37), dtype=np.float32)
    for fn in (whittaker, asls):
        for lam in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="lam must be positive and finite"):
                fn(X, lam)
        for d in (0, 3):
            with pytest.raises(ValueError, match="d must be 1 or 2"):
                fn(X, 10.0, d=d)
        with pytest.raises(ValueError, match="too few"):  # p < d + 1
            fn(np.zeros((4, 2), dtype=np.float32), 10.0, d=2)
        with pytest.raises(ValueError, match="too few"):
            fn(np.zeros((4, 1), dtype=np.float32), 10.0, d=1)
        with pytest.raises(ValueError, match=r"\(m, p\) matrix"):
            fn(np.zeros(37, dtype=np.float32), 10.0)
    for asym in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="asym must lie in"):
            asls(X, 10.0, asym=asym)
        with pytest.raises(ValueError, match="asym must lie in"):
            AsLS(10.0, asym, 10, 2)
    for n_iter in (0, -3):
        with pytest.raises(ValueError, match="n_iter must be >= 1"):
            asls(X, 10.0, n_iter=n_iter)
        with pytest.raises(ValueError, match="n_iter must be >= 1"):
            AsLS(10.0, 0.01, n_iter, 2)
    with pytest.raises(ValueError, match="lam must be positive"):
        AsLS(0.0, 0.01, 10, 2)
    with pytest.raises(ValueError, match="d must be 1 or 2"):
        AsLS(10.0, 0.01, 10, 3)
    with pytest.raises(ValueError, match="too few"):
        AsLS(10.0, 0.01, 10, 2).transform(np.zeros((4, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="too few"):
        whittaker_bands(2, 2)
    with pytest.raises(ValueError, match="d must be 1 or 2"):
        whittaker_bands(7, 3)


def test_weight_errors_need_no_device():
    X = np.zeros((4, 37), dtype=np.float32)
    good = np.ones(37)
    for bad in (-good, np.where(np.arange(37) == 5, np.nan, good), np.where(np.arange(37) == 5, np.inf, good)):
        with pytest.raises(ValueError, match="finite and >= 0"):
            whittaker(X, 10.0, weights=bad)
        with pytest.raises(ValueError, match="finite and >= 0"):
            whittaker(X, 10.0, weights=np.tile(bad, (4, 1)))
        with pytest.raises(ValueError, match="finite and >= 0"):
            whittaker(X, 10.0, weights=torch.from_numpy(bad))
    for shape in ((36,), (4, 36), (3, 37), (4, 37, 1), ()):
        with pytest.raises(ValueError, match="weights must be None"):
            whittaker(X, 10.0, weights=np.ones(shape))
    one = np.zeros(37)
    one[3] = 1.0
    with pytest.raises(ValueError, match="fewer than d = 2 positive"):
        whittaker(X, 10.0, d=2, weights=one)
    with pytest.raises(ValueError, match="fewer than d = 1 positive"):
        whittaker(X, 10.0, d=1, weights=np.zeros(37))


def test_out_errors_need_no_device():
    X = torch.zeros((4, 37), dtype=torch.float32)
    for fn in (whittaker, asls):
        with pytest.raises(ValueError, match=r"out must be a \(4, 37\) tensor"):
            fn(X, 10.0, out=torch.zeros((4, 36)))
        with pytest.raises(ValueError, match=r"out must be a \(4, 37\) tensor"):
            fn(X, 10.0, out=np.zeros((4, 37), dtype=np.float32))
        with pytest.raises(ValueError, match="out must be float32"):
            fn(X, 10.0, out=torch.zeros((4, 37), dtype=torch.float64))
        with pytest.raises(ValueError, match="unit column stride"):
            fn(X, 10.0, out=torch.zeros((37, 4)).t())
        with pytest.raises(ValueError, match="overlaps X"):
            fn(X, 10.0, out=X)
        wide = torch.zeros((5, 40))
        with pytest.raises(ValueError, match="overlaps X"):  # a shifted window of the same buffer
            fn(wide[:4, :37], 10.0, out=wide[1:, 3:])
        with pytest.raises(ValueError, match="on the device of X"):  # a host tensor
            fn(X, 10.0, out=torch.zeros((4, 37)))
