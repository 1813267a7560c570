"""ocm_eig_topk off the fused b = 32 path, against numpy.linalg.eigh.

ocm_eig::make_plan (csrc/ocm_eig_plan.h) picks one of four paths from the
width b of the subspace block, and eig_topk_impl (csrc/ocm_linalg.hip) hands
over to that path's driver.  ``_block`` restates the choice independently
(tests/test_eig_plan.py holds make_plan to it over a grid of (p, k)):

* small (p ≤ 64), eig_small: one Jacobi on C itself, k_small_finish;
* fused (b = 32, k ≤ 21), eig_fused32: what every other eigensolver test
  runs;
* plain device (b = 48 for k = 22..32, b = 64 for k = 33..64), eig_block:
  split-K dgemm for C·V, orth_block (k_colnormalize + k_atb_part /
  k_sum_planes + k_chol + k_trsm_rows<48/64>), ritz (k_jacobi_blk<48/64> on
  the projection), dgemm Ritz rotations, k_ritz_residual, the stand-alone
  k_extract_signfix and theta_deflated on k < b columns for θ;
* wide (k > 64), eig_block with host b×b steps; here only the clamped blocks
  near p (b no multiple of 16, b = p = k).

Every reference is eigh of the same fp64 matrix.  Tolerances are those of
the eigensolver tests in test_gpu_kernels.py (same solver contract,
tol = 1e-10·λ₁ on the Ritz residuals): eigenvalues rtol 1e-10, eigenvectors
atol 1e-7, θ rtol 1e-8.  Two checks are new: the loadings are orthonormal to
1e-10 (a broken second CholQR pass shows there first), and θ gets an
absolute term 1e-12·Σ_i λ_iᵐ over the whole spectrum — the fp64 cancellation
floor p·eps·trace of a trace that is a difference of O(trace C) terms, which
only matters where the tail is empty or a few values (k = p, k = p − 4).
"""
import functools

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


def _block(p, k):
    """The path ocm_eig_topk takes for (p, k): "small", the device block
    width 32 (fused) / 48 / 64, or ("wide", b)."""
    if p <= 64:
        return "small"
    b = -(-(k + max(8, k // 2)) // 16) * 16
    b = max(b, 32)
    if k <= 64 and b > 64:
        b = 64
    if b > p:
        b = max(k, (p // 16) * 16)
    assert b >= k and b >= 16
    return ("wide", b) if b > 64 else b


def _small_jacobi(n):
    """The kernel the small path's Jacobi dispatches to for an n×n matrix."""
    if n == 32:
        return "k_jacobi_1b<32>"
    if n in (48, 64):
        return "k_jacobi_blk"
    return "k_jacobi<0,64>" if n < 32 else "k_jacobi<0,256>"


def _id(pk):
    b = _block(*pk[:2])
    tag = b if isinstance(b, str) else (f"wide{b[1]}" if isinstance(b, tuple) else f"b{b}")
    return "-".join(str(v) for v in pk) + "-" + tag


BLOCK_CASES = [(300, 22), (300, 32), (1000, 25), (70, 30),                 # b = 48
               (256, 33), (1000, 48), (520, 64), (70, 40), (65, 64),       # b = 64
               (100, 70), (70, 66), (66, 66)]                              # wide, clamped to p
SMALL_CASES = [(1, 1), (2, 1), (5, 5), (31, 31), (32, 7), (33, 10), (50, 50), (63, 7), (64, 64)]
RANK_CASES = [(256, 25, 40), (256, 40, 50)]
MODE_CASES = [(300, 30), (256, 40), (100, 70), (50, 20)]


def test_case_lists_hit_the_paths_they_claim():
    """Tests the test: if the block formula in ocm_eig_plan.h changes, the
    lists above must be revisited (this restatement with them)."""
    assert [_block(p, k) for p, k in BLOCK_CASES] == [48] * 4 + [64] * 5 + [("wide", 96), ("wide", 66), ("wide", 66)]
    assert (66, 66) in BLOCK_CASES and _block(66, 66)[1] % 16 != 0  # b = p = k, no multiple of 16
    # the fused path starts right below the first case, the wide one right above the last b = 64
    assert _block(300, 21) == 32 and _block(300, 65) == ("wide", 112)
    assert all(_block(p, k) == "small" for p, k in SMALL_CASES)
    kernels = {(_small_jacobi(p), p % 2) for p, _ in SMALL_CASES}
    assert kernels >= {("k_jacobi<0,64>", 0), ("k_jacobi<0,64>", 1), ("k_jacobi_1b<32>", 0),
                       ("k_jacobi<0,256>", 0), ("k_jacobi<0,256>", 1), ("k_jacobi_blk", 0)}
    assert [(_block(p, k), r < _block(p, k)) for p, k, r in RANK_CASES] == [(48, True), (64, True)]
    assert [_block(p, k) for p, k in MODE_CASES] == [48, 64, ("wide", 96), "small"]
    assert [_block(256, k) for k in (30, 48, 64)] == [48, 64, 64]
    assert _block(128, 24) == 48


@pytest.fixture(scope="module")
def eng():
    from ocm import engine

    return engine


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared cases are read-only)


def _solve(eng, Cd, k, theta_mode, **kw):
    """engine.eig_topk with the dense fallback off: a block path that misses
    the tolerance raises OcmNotConverged here, it is never answered by
    ocm_eigh_f64 (whose exact results would pass every check below); and the
    iteration count shows that the device solver stopped at its tolerance."""
    out = eng.eig_topk(Cd, k, theta_mode, dense_fallback=False, **kw)
    assert 1 <= out[3] < eng.EIG_MAX_ITER, out[3]
    return out


def _eigh_desc(C):
    w, V = np.linalg.eigh(C)
    return w[::-1].copy(), V[:, ::-1].copy()


@functools.lru_cache(maxsize=None)
def _gap_case(p, k):
    """C with the spectrum linspace(50, 10, k) ++ geomspace(1, 1e-3, p − k) (a
    gap at k, gaps ≥ 40/(k − 1) ≥ 0.58 inside the top k, a long tail) in a
    random orthogonal basis, and its eigh (descending).  Read-only."""
    rng = np.random.default_rng(p * 31 + k)
    lam = np.concatenate([np.linspace(50, 10, k), np.geomspace(1.0, 1e-3, p - k)])
    Qm, _ = np.linalg.qr(rng.standard_normal((p, p)))
    C = (Qm * lam) @ Qm.T
    C = 0.5 * (C + C.T)
    w, V = _eigh_desc(C)
    for a in (C, w, V):
        a.setflags(write=False)
    return C, w, V


def _moments(x):
    x = np.asarray(x, dtype=np.float64)
    return np.array([x.sum(), (x ** 2).sum(), (x ** 3).sum()])


def _check_eig(out, k, w, V, tail, label):
    """The checks every case makes on eig_topk's (evals, evecs, theta, iters):
    eigenvalues, sign-fixed eigenvectors, orthonormal loadings, θ1..θ3 against
    the moments of ``tail`` (absolute term from the whole spectrum ``w``)."""
    evals, evecs, theta, iters = out
    ev, P, th = evals.cpu().numpy(), evecs.cpu().numpy(), theta.cpu().numpy()
    idx = np.argmax(np.abs(V[:, :k]), axis=0)
    Vk = (V[:, :k] * np.sign(V[idx, np.arange(k)])).T
    want_th, floor = _moments(tail), 1e-12 * _moments(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{label}: iters {iters}  evals rel {np.abs(ev / w[:k] - 1).max():.2e}  "
              f"evecs abs {np.abs(P - Vk).max():.2e}  orth {np.abs(P @ P.T - np.eye(k)).max():.2e}  "
              f"theta abs {np.abs(th - want_th)}  rel {np.abs(th - want_th) / np.abs(want_th)}  floor {floor}")
    np.testing.assert_allclose(ev, w[:k], rtol=1e-10, err_msg=label)
    np.testing.assert_allclose(P, Vk, rtol=0, atol=1e-7, err_msg=label)
    np.testing.assert_allclose(P @ P.T, np.eye(k), rtol=0, atol=1e-10, err_msg=label)
    for m in range(3):
        np.testing.assert_allclose(th[m], want_th[m], rtol=1e-8, atol=floor[m], err_msg=f"{label} theta{m + 1}")
    assert iters >= 1


@pytest.mark.parametrize("p,k", BLOCK_CASES, ids=[_id(c) for c in BLOCK_CASES])
def test_eig_block_paths(eng, p, k):
    """b = 48, b = 64 and the clamped wide blocks against eigh.  p = 300, 520,
    1000, 70, 65 are no multiples of 64 (row tails of k_atb_part and
    k_trsm_rows, the K tail of the split-K planes; 300 and 1000 differ in
    kper / nz); (65, 64) and the wide cases with b = k test the Ritz pair at
    the block's edge."""
    C, w, V = _gap_case(p, k)
    _check_eig(_solve(eng, _dev(C), k, 2), k, w, V, w[k:], f"p={p} k={k} {_block(p, k)}")


@pytest.mark.parametrize("p,k", SMALL_CASES, ids=[_id(c) for c in SMALL_CASES])
def test_eig_small_path_sizes(eng, p, k):
    """p ≤ 64: every kernel the Jacobi dispatch can pick (k_jacobi<0,64> and
    k_jacobi<0,256> at odd and even n, k_jacobi_1b<32>, k_jacobi_blk<64>) on
    a Wishart matrix A·Aᵀ, A (p, p + 5); k = p leaves an empty tail (θ = 0).
    The smallest gap next to a wanted eigenvalue over these matrices is 0.069
    at λ₁ ≤ 270, so the Jacobi's stop (off-diagonal norm ≤ 1e-13 of the
    diagonal's) leaves the vectors within ≈ 1e-9 of eigh's."""
    rng = np.random.default_rng(1000 + p * 31 + k)
    A = rng.standard_normal((p, p + 5))
    C = A @ A.T
    C = 0.5 * (C + C.T)
    w, V = _eigh_desc(C)
    _check_eig(_solve(eng, _dev(C), k, 2), k, w, V, w[k:], f"p={p} k={k} {_small_jacobi(p)}")


@pytest.mark.parametrize("p,k,rank", RANK_CASES, ids=[_id(c) for c in RANK_CASES])
def test_eig_rank_deficient_wide_block(eng, p, k, rank):
    """C of rank < b on the plain device path (a class with fewer spectra than
    the block is wide; test_eig_rank_deficient_block is its b = 32 twin):
    C·V has dependent columns, so k_chol's pivot clamp and k_colnormalize's
    replacement of zero columns carry the iteration.  θ against the known
    nonzero tail."""
    rng = np.random.default_rng(100 + rank)
    lam = np.concatenate([np.linspace(40, 20, k), np.geomspace(1.0, 1e-2, rank - k)])
    Qm, _ = np.linalg.qr(rng.standard_normal((p, rank)))
    C = (Qm * lam) @ Qm.T
    C = 0.5 * (C + C.T)
    w, V = _eigh_desc(C)
    _check_eig(_solve(eng, _dev(C), k, 2), k, w, V, lam[k:], f"p={p} k={k} rank={rank} {_block(p, k)}")


@pytest.mark.parametrize("p,k", MODE_CASES, ids=[_id(c) for c in MODE_CASES])
def test_eig_theta_modes_and_slices(eng, p, k):
    """theta_mode 0 / 1 / 2, the θ3 slices of ocm_eig_topk_ex (include/ocm.h:
    every output but theta[2] complete on every slice, the slices' theta[2]
    sum to θ3; p ≤ 64: slice 0 carries it all) and inv_out on each path.

    Σ_s theta[2] against the unsliced theta[2]: rtol 2.5e-9, set from a
    measurement, not 1e-12.  The Δ terms of θ3 are exact fp64 row sums, but
    its O∘O² term is an i8×3 Gram (≈ 4e-8 relative per entry) whose scale
    blocks follow the slice's row count, so a sliced and an unsliced call
    round that term differently on every path.  On the fused path (k ≤ 21,
    the one every earlier eigensolver test runs) the same figure on the same
    spectrum family, (p, k) = (300, 8), (256, 20), (1000, 12), (300, 21),
    (1000, 21), (70, 20), (100, 21), (65, 16), measured 4.0e-12 … 2.47e-10
    on an MI355X; the bound is 10× the largest.  The paths here measured
    5.2e-10 (b = 48), 1.3e-11 (b = 64), 6.3e-10 (wide), 0 (small)."""
    import torch

    C, w, _ = _gap_case(p, k)
    Cd = _dev(C)
    tail3 = (w[k:] ** 3).sum()

    def bits(t):
        return t.cpu().numpy().tobytes()

    ev2, P2, th2, _ = _solve(eng, Cd, k, 2)
    _, _, th0, _ = _solve(eng, Cd, k, 0)
    assert bits(th0) == np.zeros(3).tobytes()
    ev1, P1, th1, _ = _solve(eng, Cd, k, 1)
    assert bits(th1[:2]) == bits(th2[:2]) and bits(ev1) == bits(ev2) and bits(P1) == bits(P2)

    parts = []
    for s in range(3):
        ev, P, th, _ = _solve(eng, Cd, k, 2, theta3_slice=(s, 3))
        assert bits(ev) == bits(ev2) and bits(P) == bits(P2), f"slice {s}"
        assert bits(th[:2]) == bits(th2[:2]), f"slice {s}"
        parts.append(float(th[2]))
    print(f"p={p} k={k} {_block(p, k)}: theta3 slices {parts}  sum/tail3-1 {sum(parts) / tail3 - 1:.2e}  "
          f"sum/unsliced-1 {sum(parts) / float(th2[2]) - 1:.2e}")
    np.testing.assert_allclose(sum(parts), tail3, rtol=1e-8)
    np.testing.assert_allclose(sum(parts), float(th2[2]), rtol=2.5e-9)
    if p <= 64:
        assert parts[0] == float(th2[2]) and parts[1] == 0.0 and parts[2] == 0.0
    else:  # every slice did its rows' share on the device (PSD deflated matrix: each share > 0)
        assert all(t > 0.0 for t in parts), parts

    inv = torch.full((k,), -1.0, dtype=torch.float64, device="cuda")
    ev, P, th, _ = _solve(eng, Cd, k, 2, inv_out=inv)
    assert bits(ev) == bits(ev2) and bits(P) == bits(P2) and bits(th) == bits(th2)
    assert bits(inv) == bits(eng.inv_evals(ev))


def test_eig_first_product_test_converges(eng):
    """max_iter = 1 on the fused path: eig_fused32 orthonormalises the start
    block (k_cq_gram32 twice, k_cq_apply32), forms C·V by k_cv32 and runs the
    Rayleigh–Ritz step on that first product.  C = 3·I: every orthonormal
    block is invariant, so that one test converges, whatever the block."""
    p, k = 128, 6
    assert _block(p, k) == 32
    evals, evecs, theta, iters = eng.eig_topk(_dev(3.0 * np.eye(p)), k, 2, max_iter=1, dense_fallback=False)
    ev, P, th = evals.cpu().numpy(), evecs.cpu().numpy(), theta.cpu().numpy()
    want_th, floor = (p - k) * np.array([3.0, 9.0, 27.0]), 1e-12 * p * np.array([3.0, 9.0, 27.0])
    print(f"iters {iters}  evals abs {np.abs(ev - 3).max():.2e}  orth {np.abs(P @ P.T - np.eye(k)).max():.2e}  "
          f"theta rel {np.abs(th / want_th - 1)}")
    assert iters == 1
    np.testing.assert_allclose(ev, 3.0, rtol=1e-10)
    np.testing.assert_allclose(P @ P.T, np.eye(k), rtol=0, atol=1e-10)
    for m in range(3):
        np.testing.assert_allclose(th[m], want_th[m], rtol=1e-8, atol=floor[m], err_msg=f"theta{m + 1}")


@pytest.mark.parametrize("p,k", [(128, 6), (128, 24)], ids=["128-6-b32", "128-24-b48"])
def test_eig_first_product_test_fails_cleanly(eng, p, k):
    """max_iter = 1 on a matrix with a spectrum: one product of a random block
    is nowhere near the tolerance, so the call reports OcmNotConverged (fused
    path and b = 48), and the next ordinary solve in the same process is
    unaffected by the state it left (tickets, the in-flight flag's epoch)."""
    from ocm._lib import OcmNotConverged

    C, w, V = _gap_case(p, k)
    Cd = _dev(C)
    assert _block(p, k) == (32 if k == 6 else 48)
    with pytest.raises(OcmNotConverged):
        eng.eig_topk(Cd, k, 2, max_iter=1, dense_fallback=False)
    _check_eig(_solve(eng, Cd, k, 2), k, w, V, w[k:], f"p={p} k={k} after max_iter=1")


def _spy_eig_topk(monkeypatch):
    """Record the (p, k) of every engine.eig_topk call, and fail the call if
    the device solver did not answer it: engine.eig_topk otherwise hands a
    solve that missed its tolerance to the dense solver with only a
    RuntimeWarning, and the drop-in's results would then pass unnoticed."""
    import warnings

    from ocm import engine

    seen = []
    orig = engine.eig_topk

    def wrapped(C, k, *a, **kw):
        seen.append((int(C.shape[0]), int(k)))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            out = orig(C, k, *a, **kw)
        assert 1 <= out[3] < engine.EIG_MAX_ITER, out[3]
        return out

    monkeypatch.setattr(engine, "eig_topk", wrapped)
    return seen


@pytest.mark.parametrize("k", [30, 48, 64])
def test_dropin_k_30_48_64_vs_oracle(k, monkeypatch):
    """utils.SIMCA at n_components on the b = 48 and b = 64 paths against the
    fp64 oracle (Gram + eigh), with the north-star test's assertions and
    tolerances; ocm_score_f32_diag then runs at k = 30, 48, 64 on fitted
    loadings.  Random orthonormal loadings: the band loadings have no gap at
    these k (λ_k/λ_{k+1} = 1.01 at k = 30), these have λ_k/λ_{k+1} ≈ 15."""
    from oracle.simca_oracle import synth_spectra
    from test_gpu_northstar import _check_vs_oracle

    seen = _spy_eig_topk(monkeypatch)
    X = synth_spectra(3600, 256, k, rank=int(1.5 * k), seed=k, outlier_frac=0.1, loadings="random")
    _check_vs_oracle(X[:3000], X[3000:], k, [("alt", "Fdist", "jm"), ("ci", "chi2", "chi2box")])
    assert seen and set(seen) == {(256, k)} and _block(256, k) == (48 if k == 30 else 64)


def test_fold_engine_lv_24_vs_refit_loop(monkeypatch):
    """The CV fold engine with LV_max = 24: every fold's eigensolve runs at
    b = 48 and the LV prefixes (k_cv_prefix / k_cv_counts) at their 32-wide
    instantiation; compared with the per-fold refit loop as
    test_gpu_cv.test_fold_engine_vs_refit_loop does."""
    from oracle.simca_oracle import synth_spectra
    from test_gpu_cv import _fast_used, _run

    Xa = synth_spectra(1200, 128, 24, rank=36, seed=24, loadings="random")
    Xb = synth_spectra(400, 128, 24, rank=36, seed=24, loadings="random", outlier_frac=1.0)
    X = np.concatenate([Xa, Xb])
    y = np.concatenate([np.zeros(1200, dtype=np.int64), np.ones(400, dtype=np.int64)])
    grid = {"type": ["alt", "sim"]}
    calls = _fast_used(monkeypatch)
    seen = _spy_eig_topk(monkeypatch)
    fast = _run(X, y, 5, 22, 24, grid, fast=True)
    assert calls["n"] == 1 and (128, 24) in seen and _block(128, 24) == 48
    slow = _run(X, y, 5, 22, 24, grid, fast=False)
    assert calls["n"] == 1
    assert [r["params"] for r in fast["results"]] == [r["params"] for r in slow["results"]]
    assert [r["LV"] for r in fast["results"]] == [r["LV"] for r in slow["results"]] == [22, 23, 24] * 2
    pf = np.stack([b["prediction"] for b in fast["by_combo"]])
    ps = np.stack([b["prediction"] for b in slow["by_combo"]])
    diff = (pf != ps).sum(axis=1)
    print("differing rows per record:", diff, " spec", [r["spec"] for r in fast["results"]],
          " sens", [r["sens"] for r in fast["results"]])
    assert diff.max() <= 2, diff
    np.testing.assert_allclose([r["spec"] for r in fast["results"]], [r["spec"] for r in slow["results"]],
                               atol=0.5)
    np.testing.assert_allclose([r["sens"] for r in fast["results"]], [r["sens"] for r in slow["results"]],
                               atol=0.5)
