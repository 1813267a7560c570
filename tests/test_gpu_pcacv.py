"""PCA cross-validation on the GPU: ocm_press_f32 / _f64 against the closed
form in NumPy float64 (tests/pcacv_oracle.py) with P and μ from a host SVD,
then ``pca_press`` end to end against the oracle recomputed from the models it
returns and against the full NumPy CV's choice of components.

Tolerances (press and naive): float32 rtol 1e-4, the project's scoring
tolerance (tests/test_gpu_contrib.py); float64 rtol 1e-10.  The inputs'
preconditions are asserted on the host (tests/test_pcacv_host.py); the
kernel-level inputs are picked so that float32's own worst-case error is inside
the tolerance (pcacv_oracle.f32_error_bound)."""
import numpy as np
import pytest
import torch

import pcacv_oracle as O
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

RTOL = {torch.float32: 1e-4, torch.float64: 1e-10}
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = [torch.float32, torch.float64]


# ---------------------------------------------------------------- kernel level
def run_press(Xd, rows, m, P, mu, want_naive=True, want_ndegen=True):
    """Raw ocm_press call on device tensors (Xd may be a strided view)."""
    from ocm import _lib

    dev = Xd.device
    K, p = P.shape
    Pd = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
    mud = torch.from_numpy(np.ascontiguousarray(mu)).to(dev)
    press = torch.full((K + 1,), float("nan"), dtype=torch.float64, device=dev)
    naive = torch.full((K + 1,), float("nan"), dtype=torch.float64, device=dev) if want_naive else None
    nd = torch.full((K + 1,), -1, dtype=torch.int32, device=dev) if want_ndegen else None
    fn = "ocm_press_f64" if Xd.dtype == torch.float64 else "ocm_press_f32"
    _lib.check(getattr(_lib.load(), fn)(_lib.Context.get(dev.index).handle, _lib.ptr(Xd), Xd.stride(0) if m else p,
                                        _lib.ptr(rows), m, p, _lib.ptr(Pd), _lib.ptr(mud), K, _lib.ptr(press),
                                        _lib.ptr(naive), _lib.ptr(nd), _lib.stream_handle(dev)), fn)
    torch.cuda.synchronize()
    return press, naive, nd


def check_case(m, p, K, dtype, shuffled=False, ldx=None):
    dev = torch.device("cuda", 0)
    Xh, mu, P = O.kernel_case(m, p, K, np.dtype(NP[dtype]).name)
    want_p, want_n, want_d = O.press_closed(Xh, P, mu)
    if shuffled:  # the m rows scattered through a larger matrix, taken by index
        rng = np.random.default_rng(5)
        big = rng.standard_normal((2 * m + 3, p)).astype(NP[dtype])
        idx = rng.permutation(2 * m + 3)[:m].astype(np.int64)
        big[idx] = Xh
        Xd, rows = torch.from_numpy(big).to(dev), torch.from_numpy(idx).to(dev)
    else:
        Xd, rows = torch.from_numpy(Xh.copy()).to(dev), None
    if ldx is not None:  # a row pitch wider than p
        wide = torch.full((Xd.shape[0], ldx), float("nan"), dtype=dtype, device=dev)
        wide[:, :p] = Xd
        Xd = wide[:, :p]
        assert Xd.stride(0) == ldx
    press, naive, nd = run_press(Xd, rows, m, P, mu)
    got_p, got_n = press.cpu().numpy(), naive.cpu().numpy()
    worst = max(np.max(np.abs(got_p - want_p) / want_p), np.max(np.abs(got_n - want_n) / want_n))
    print(f"press m={m} p={p} K={K} {dtype}: worst relative error {worst:.3e} (bound {RTOL[dtype]:.0e})")
    np.testing.assert_allclose(got_p, want_p, rtol=RTOL[dtype])
    np.testing.assert_allclose(got_n, want_n, rtol=RTOL[dtype])
    assert nd.cpu().numpy().tolist() == want_d.tolist()
    return press, naive


def k_for(p):
    return {2: 1, 33: 6, 257: 20, 1024: 20}[p]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [2, 33, 257, 1024])
@pytest.mark.parametrize("m", [1, 17, 255, 257, 3 * 256 + 5])
def test_kernel_against_closed_form(m, p, dtype):
    """Tile tails (m % 16), chunk tails (m % 256), one and several chunks; odd
    widths, widths below one column block and of several; 16-byte and scalar loads."""
    check_case(m, p, k_for(p), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,K", [(33, 1), (8, 6), (257, 64), (64, 17), (96, 33), (128, 49)])
def test_kernel_component_counts(p, K, dtype):
    """K = 1, K close to p, K = 64, and the first K of every component tile of 16."""
    check_case(3 * 256 + 5, p, K, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,ldx", [(33, None), (33, 40), (1024, None), (1024, 1028), (1024, 1027)])
def test_kernel_row_index_and_pitch(p, ldx, dtype):
    """``rows`` a shuffled index vector into a larger matrix, and ldx > p (a
    pitch that keeps 16-byte loads and one that does not)."""
    check_case(3 * 256 + 5, p, k_for(p), dtype, shuffled=True, ldx=ldx)
    if ldx is not None:
        check_case(257, p, k_for(p), dtype, shuffled=False, ldx=ldx)


# the widest p whose 16-row tile waits in LDS and the next width that is read a
# second time from L2 (include/ocm.h), per element type and component tile
BOUNDARY = [(torch.float32, 6, 1088, 1092), (torch.float32, 20, 896, 900), (torch.float32, 40, 768, 772),
            (torch.float32, 64, 576, 580), (torch.float64, 6, 1152, 1153), (torch.float64, 20, 1088, 1089),
            (torch.float64, 40, 960, 961), (torch.float64, 64, 896, 897)]


@pytest.mark.parametrize("dtype,K,p_lds,p_l2", BOUNDARY)
def test_kernel_both_sides_of_the_tile_boundary(dtype, K, p_lds, p_l2):
    check_case(40, p_lds, K, dtype)
    check_case(40, p_l2, K, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_wide_rows(dtype):
    """p > 2048: a float32 lane hands its sums on inside a chunk (after 14 of its
    16 tiles at nine column blocks per wave), not only at its end."""
    check_case(256 + 44, 2304, 6, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_variable_is_left_out_and_counted(dtype):
    """A P whose first row is exactly e_j: 1 − h_j = 0 from k = 1 on."""
    rng = np.random.default_rng(3)
    p, K, j, m = 37, 5, 11, 300
    Q = np.linalg.qr(rng.standard_normal((p - 1, K - 1)))[0].T
    P = np.zeros((K, p))
    P[0, j] = 1.0
    P[1:, np.arange(p) != j] = Q
    Xh = (1.0 + rng.standard_normal((m, p))).astype(NP[dtype])
    mu = Xh.astype(np.float64).mean(axis=0)
    press, naive, nd = run_press(torch.from_numpy(Xh).cuda(), None, m, P, mu)
    assert nd.cpu().numpy().tolist() == [0] + [1] * K
    want = O.press_closed(Xh, P, mu, exclude=j)
    np.testing.assert_allclose(press.cpu().numpy(), want[0], rtol=RTOL[dtype])
    np.testing.assert_allclose(naive.cpu().numpy(), want[1], rtol=RTOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_rows_gives_zeros(dtype):
    _, mu, P = O.kernel_case(257, 33, 6)
    X = torch.empty((0, 33), dtype=dtype, device="cuda")
    press, naive, nd = run_press(X, None, 0, P, mu)
    assert press.cpu().numpy().tolist() == [0.0] * 7 and naive.cpu().numpy().tolist() == [0.0] * 7
    assert nd.cpu().numpy().tolist() == [0] * 7
    press, naive, nd = run_press(X, None, 0, P, mu, want_naive=False, want_ndegen=False)
    assert naive is None and nd is None and press.cpu().numpy().tolist() == [0.0] * 7


@pytest.mark.parametrize("dtype", DTYPES)
def test_optional_outputs_and_argument_errors(dtype):
    Xh, mu, P = O.kernel_case(257, 33, 6, np.dtype(NP[dtype]).name)
    Xd = torch.from_numpy(Xh.copy()).cuda()
    full = run_press(Xd, None, 257, P, mu)
    only = run_press(Xd, None, 257, P, mu, want_naive=False, want_ndegen=False)
    assert torch.equal(full[0], only[0])
    with pytest.raises(ValueError):   # K > p
        run_press(Xd[:, :4].contiguous(), None, 257, np.zeros((5, 4)), np.zeros(4))
    with pytest.raises(ValueError):   # K > 64
        run_press(torch.zeros((4, 80), dtype=dtype, device="cuda"), None, 4, np.zeros((65, 80)), np.zeros(80))
    with pytest.raises(ValueError):   # p < 2
        run_press(torch.zeros((4, 1), dtype=dtype, device="cuda"), None, 4, np.zeros((1, 1)), np.zeros(1))
    with pytest.raises(ValueError):   # m < 0
        run_press(Xd, None, -1, P, mu)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_launches_give_the_same_bits(dtype):
    m, p, K = 5 * 256 + 77, 257, 20
    Xh, mu, P = O.kernel_case(m, p, K, np.dtype(NP[dtype]).name)
    Xd = torch.from_numpy(Xh.copy()).cuda()
    a = run_press(Xd, None, m, P, mu)
    b = run_press(Xd, None, m, P, mu)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ------------------------------------------------------------------ end to end
E2E = [O.SHAPES[0], O.SHAPES[1]]


def from_models(Xh, res):
    """press_folds recomputed in float64 from the models a result carries."""
    out = []
    for mdl, rows in zip(res.models, res.folds):
        P, mu = mdl["loadings"].cpu().numpy(), mdl["mean"].cpu().numpy()
        out.append(O.press_closed(Xh[rows], P, mu))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,p,rank", E2E)
def test_pca_press_end_to_end(n, p, rank, dtype):
    from ocm.pcacv import pca_press

    Xh, K, folds, (ref_press, _, _, _, _) = O.fixture(n, p, rank, 0, np.dtype(NP[dtype]).name)
    res = pca_press(torch.from_numpy(np.array(Xh)).cuda(), K, cv=O.NFOLDS)
    assert [f.tolist() for f in res.folds] == [f.tolist() for f in folds]
    assert res.n == n and res.p == p and res.press_folds.shape == (O.NFOLDS, K + 1)
    assert all(m["loadings"].shape == (K, p) and m["loadings"].dtype == torch.float64 and m["loadings"].is_cuda
               and m["mean"].shape == (p,) and m["evals"].shape == (K,) for m in res.models)
    want = from_models(Xh, res)
    np.testing.assert_allclose(res.press_folds, np.array([w[0] for w in want]), rtol=RTOL[dtype])
    np.testing.assert_allclose(res.press, sum(w[0] for w in want), rtol=RTOL[dtype])
    np.testing.assert_allclose(res.naive, sum(w[1] for w in want), rtol=RTOL[dtype])
    assert res.ndegen.tolist() == [0] * (K + 1)
    np.testing.assert_allclose(res.rmsecv, np.sqrt(res.press / (n * p)), rtol=1e-15)
    np.testing.assert_allclose(res.q2, 1.0 - res.press / res.press[0], rtol=1e-15)
    # the choice: the full NumPy CV's, and the rank the data was made with
    assert res.select("min") == int(np.argmin(ref_press)) == rank
    assert int(np.argmin(res.naive)) == K


def test_pca_press_takes_host_arrays_and_explicit_folds():
    from ocm.pcacv import pca_press

    n, p, rank = O.SHAPES[0]
    Xh, K, folds, _ = O.fixture(n, p, rank, 0, "float32")
    a = pca_press(Xh, K, cv=O.NFOLDS)
    b = pca_press(torch.from_numpy(np.array(Xh)).cuda(), K, folds=folds)
    assert np.array_equal(a.press_folds, b.press_folds) and np.array_equal(a.naive, b.naive)


def test_object_wise_folds_hold_out_whole_objects():
    from ocm.objectcv import ObjectKFoldWithExternalVal
    from ocm.pcacv import pca_press

    n, p, rank = O.SHAPES[0]
    Xh, K, _, _ = O.fixture(n, p, rank, 0, "float32")
    other = O.lowrank(60, p, 2, 55, dtype=np.float32)
    X = np.concatenate([Xh, other])
    y = np.array([0] * n + [1] * 60)
    objects = np.concatenate([np.repeat(np.arange(n // 8), 8), n // 8 + np.repeat(np.arange(6), 10)])
    cv = ObjectKFoldWithExternalVal(n_splits=3, objects=objects, cls_label=0)
    res = pca_press(X, K, cv=cv, y=y)
    held = [set(objects[f].tolist()) for f in res.folds]
    assert sum(len(h) for h in held) == len(set.union(*held)) == n // 8   # no object on both sides of a fold
    for f, h in zip(res.folds, held):
        assert sorted(f.tolist()) == np.flatnonzero(np.isin(objects, list(h))).tolist()
        assert y[f].max() == 0
    want = from_models(X, res)
    np.testing.assert_allclose(res.press_folds, np.array([w[0] for w in want]), rtol=1e-4)
    assert res.n == n and res.select("min") == rank


def test_simca_press_is_pca_press_on_the_class_rows():
    from ocm.pcacv import pca_press
    from utils.SIMCA import SIMCA

    n, p, rank = O.SHAPES[0]
    Xh, K, _, _ = O.fixture(n, p, rank, 0, "float32")
    rng = np.random.default_rng(9)
    X = np.concatenate([Xh, O.lowrank(50, p, 2, 55, dtype=np.float32)])
    y = np.array([0] * n + [1] * 50)
    perm = rng.permutation(n + 50)
    X, y = np.ascontiguousarray(X[perm]), y[perm]
    a = SIMCA(n_components=2, model_class=0, verbose=False).press(X, y, max_components=K, cv=O.NFOLDS)
    b = pca_press(X, K, cv=O.NFOLDS, rows=np.flatnonzero(y == 0))
    assert np.array_equal(a.press_folds, b.press_folds) and np.array_equal(a.naive, b.naive)
    assert a.n == n and a.select("min") == b.select("min") == rank
    c = SIMCA(verbose=False).press(X, y, cls=0, max_components=K, cv=O.NFOLDS)
    assert np.array_equal(a.press, c.press)
    d = SIMCA(verbose=False, maxPC=K).press(X[y == 0], cv=O.NFOLDS)   # every row, maxPC components
    assert d.press.shape == (K + 1,) and d.n == n


@pytest.mark.parametrize("dtype", DTYPES)
def test_press_variables_sums_to_press(dtype):
    from ocm.pcacv import press_variables, pca_press

    n, p, rank = O.SHAPES[1]
    Xh, K, _, _ = O.fixture(n, p, rank, 0, np.dtype(NP[dtype]).name)
    Xd = torch.from_numpy(np.array(Xh)).cuda()
    res = pca_press(Xd, K, cv=O.NFOLDS)
    for k in (0, 1, rank, K):
        v = press_variables(Xd, res, k)
        assert v.shape == (p,) and v.dtype == torch.float64 and v.is_cuda
        np.testing.assert_allclose(float(v.sum()), res.press[k], rtol=1e-4)
    # per variable against the oracle on the returned models
    want = np.zeros(p)
    for mdl, rows in zip(res.models, res.folds):
        P, mu = mdl["loadings"].cpu().numpy(), mdl["mean"].cpu().numpy()
        R = (Xh[rows].astype(np.float64) - mu) @ (np.eye(p) - P[:rank].T @ P[:rank])
        want += O.leverage_weights(P, rank)[0] * (R * R).sum(axis=0)
    np.testing.assert_allclose(press_variables(Xd, res, rank).cpu().numpy(), want, rtol=1e-4)


def test_lazy_view_is_materialised():
    """A PrepView input: the fold models come from the view's Gram, the PRESS
    pass reads the fold's materialised rows."""
    from ocm.pcacv import pca_press
    from ocm.preprocess import snv_savgol

    n, p, rank = O.SHAPES[0]
    Xh, K, _, _ = O.fixture(n, p, rank, 0, "float32")
    Xd = torch.from_numpy(np.array(Xh)).cuda()
    view = snv_savgol(Xd, lazy=True)   # SNV in the load path
    res = pca_press(view, K, cv=O.NFOLDS)
    Xm = view.materialize(None).cpu().numpy()
    want = from_models(Xm, res)
    np.testing.assert_allclose(res.press_folds, np.array([w[0] for w in want]), rtol=1e-4)
