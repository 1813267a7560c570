"""The fp64 reference of the Whittaker smoother and of AsLS (include/ocm.h,
baseline correction), on scipy.linalg.solveh_banded, with the test inputs and
the error bound the GPU tests share.  A helper module, not a test file."""
import functools

import numpy as np
from scipy.linalg import solveh_banded

EPS64 = float(np.finfo(np.float64).eps)

# (m, p): smallest for d = 2; odd p below the 32-column tile; p no multiple of the tile and m < 64;
# exactly one 64-row block and full tiles; two row blocks, the second partial; the headline p; p > 4096
SHAPES = [(3, 3), (5, 7), (33, 37), (64, 256), (70, 1000), (40, 2048), (9, 4100)]
PADS = [0, 3]  # ldx = p, and a row slice of a wider tensor (ldx = p + 3: rows not 16-byte aligned)
ORDERS = [1, 2]


@functools.lru_cache(maxsize=None)
def spectra(m, p):
    """Synthetic spectra on a curved baseline a + d1·λ + d2·λ², λ = linspace(−1, 1, p), float32 (read-only)."""
    from oracle.simca_oracle import synth_spectra

    rng = np.random.default_rng(2000 + p)
    x = synth_spectra(m, p, 6, rank=16, seed=2001 + p).astype(np.float64)
    lam = np.linspace(-1.0, 1.0, p)
    a = rng.uniform(-2, 2, (m, 1))
    d1 = rng.uniform(-1, 1, (m, 1))
    d2 = rng.uniform(-1, 1, (m, 1))
    X = (x + a + d1 * lam + d2 * lam ** 2).astype(np.float32)
    X.setflags(write=False)
    return X


def whittaker_ref(X, lam, d, w=None):
    """z of (diag(w) + λ·DᵀD) z = w ∘ x per row, fp64.  w: None, (p,) or (m, p)."""
    from ocm.preprocess import whittaker_bands

    X = np.asarray(X, dtype=np.float64)
    m, p = X.shape
    ab0 = lam * whittaker_bands(p, d)
    w = np.ones(p) if w is None else np.asarray(w, dtype=np.float64)
    if w.ndim == 1:
        ab = ab0.copy()
        ab[0] += w
        return solveh_banded(ab, (w * X).T, lower=True).T
    Z = np.empty_like(X)
    for i in range(m):
        ab = ab0.copy()
        ab[0] += w[i]
        Z[i] = solveh_banded(ab, w[i] * X[i], lower=True)
    return Z


def asls_ref(X, lam, asym, n_iter, d):
    """(Z, iters, margin): the baselines of the last solve, the solves each row ran, and per row the
    min over its iterations and columns of |x_j − z_j| (how far its closest weight decision was from a tie)."""
    from ocm.preprocess import whittaker_bands

    X = np.asarray(X, dtype=np.float64)
    m, p = X.shape
    ab0 = lam * whittaker_bands(p, d)
    Z = np.empty_like(X)
    iters = np.zeros(m, dtype=np.int32)
    margin = np.full(m, np.inf)
    for i in range(m):
        x = X[i]
        w = np.ones(p)
        for it in range(1, n_iter + 1):
            ab = ab0.copy()
            ab[0] += w
            z = solveh_banded(ab, w * x, lower=True)
            iters[i] = it
            margin[i] = min(margin[i], np.abs(x - z).min())
            w_new = np.where(x > z, asym, 1.0 - asym)
            if np.array_equal(w_new, w):
                break
            w = w_new
        Z[i] = z
    return Z, iters, margin


@functools.lru_cache(maxsize=None)
def asls_case(m, p, lam, asym, d, n_iter=10):
    out = asls_ref(spectra(m, p), lam, asym, n_iter, d)
    for a in out:
        a.setflags(write=False)
    return out


def slack(X, lam, d, w_min, w_max=1.0, kappa=None):
    """Per row s = 4·κ·ε₆₄·max|x_row| with κ ≤ (w_max + 4ᵈ·λ) / w_min (the largest eigenvalue of DᵀD is below
    4ᵈ, the smallest of the matrix is at least w_min), or a given κ: the forward error of a backward-stable
    solve is at most c·κ·ε₆₄ relative to the solution, which is of the size of the row."""
    k = (w_max + 4.0 ** d * lam) / w_min if kappa is None else kappa
    return 4.0 * k * EPS64 * np.abs(np.asarray(X, dtype=np.float64)).max(axis=1, keepdims=True)


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def worst_ratio(got, ref, s):
    """max of |got − ref| / (ulp₃₂(|ref|) + s): at most 1 within the bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / (ulp32(ref) + s)).max())
