"""Kennard–Stone and Duplex on the GPU (ocm_ks_pair_*, ocm_ks_nearest_*,
ocm_ks_select_*, ocm.sampling) against the fp64 NumPy oracle of
tests/ks_oracle.py.

The device's ``order`` must EQUAL the oracle's and ``d2`` agree to rtol 1e-13.
No tolerance on the order is needed: every continuous fixture keeps its best
and second-best candidates ≥ 1e-10 apart (relative) at the start and at every
step, which the tests assert on the oracle, and fp64 rounding of a q-term
weighted sum of squares is below (q + 3)·2⁻⁵³ ≈ 1.5e-14 at q = 130, so no
summation order can flip a comparison.  The tie fixtures (integer grids,
identical rows) have exact distances in any order."""
import numpy as np
import pytest
import torch

import ks_oracle as O
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

RTOL = 1e-13
SMALL, WIDE = 1, 2
NP_DT = {"f32": np.float32, "f64": np.float64}


def on_device(Z, dt="f32", pad=0):
    """Z on the device as float32 / float64: contiguous, or (pad > 0) the left
    columns of a wider tensor whose other columns hold NaN."""
    Z = np.asarray(Z).astype(NP_DT[dt])
    n, q = Z.shape
    t = torch.from_numpy(Z).cuda()
    if pad == 0:
        return t
    buf = torch.full((n, q + pad), float("nan"), dtype=t.dtype, device="cuda")
    buf[:, :q] = t
    Zd = buf[:, :q]
    assert Zd.stride(0) == q + pad
    return Zd


def host(t):
    return t.detach().cpu().numpy()


def engine_ks(Zd, n_select, init="pair", start=None, w=None, path=0):
    """Kennard–Stone through the engine wrappers (Z read in place): (order, d2, nbad)."""
    from ocm import engine

    wd = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64)).cuda()
    head = None
    nbad0 = 0
    if start is not None:
        st = torch.tensor(list(start), dtype=torch.int64, device="cuda")
    elif init == "pair":
        st, head, nb = engine.ks_pair(Zd, wd)
        nbad0 = int(nb.item())
    else:
        center = Zd.to(torch.float64).mean(dim=0)
        st, head, nb = engine.ks_nearest(Zd, center, wd)
        nbad0 = int(nb.item())
    res = engine.ks_select(Zd, st, n_select, w=wd, path=path)
    d2 = res["d2_a"]
    if head is not None:
        d2[:st.numel()] = head
    return host(res["order_a"]), host(d2), max(nbad0, int(res["nbad"].item()))


def check(ref, order, d2):
    assert np.array_equal(order, ref["order"]), (
        f"first difference at step {int(np.flatnonzero(order != ref['order'])[0])}")
    nan = np.isnan(ref["d2"])
    assert np.array_equal(np.isnan(d2), nan)
    np.testing.assert_allclose(d2[~nan], ref["d2"][~nan], rtol=RTOL, atol=0)


# ------------------------------------------------------------------ the fixtures

@pytest.mark.parametrize("path", [SMALL, WIDE])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("init", ["pair", "mean"])
@pytest.mark.parametrize("n,q,seed", O.FIXTURES)
def test_fixture_all_rows(n, q, seed, init, dt, path):
    from ocm import sampling as S

    ref = O.fixture_oracle(n, q, seed, init)
    assert ref["min_rel_gap"] >= O.MIN_GAP
    sel = S.kennard_stone(on_device(O.fixture_data(n, q, seed), dt), n, init=init, _path=path)
    check(ref, sel.order, sel.d2)
    t0 = 2 if init == "pair" else 1
    assert (np.diff(sel.d2[t0:]) <= 0).all()
    np.testing.assert_array_equal(sel.distance, np.sqrt(sel.d2))


@pytest.mark.parametrize("path", [0, SMALL, WIDE])
def test_host_input_and_partial_counts(path):
    """NumPy in; n_select = 2, n − 1 and n; the auto path equals each forced path."""
    from ocm import sampling as S

    n, q, seed = O.FIXTURES[2]
    Z = O.fixture_data(n, q, seed)
    ref = O.fixture_oracle(n, q, seed, "pair")
    for n_select in (2, n - 1, n):
        sel = S.kennard_stone(Z, n_select, _path=path)
        check({"order": ref["order"][:n_select], "d2": ref["d2"][:n_select]}, sel.order, sel.d2)
        assert sel.mask(n).sum() == n_select and sel.rest(n).size == n - n_select
    sel = S.kennard_stone(Z, 1, init="mean", _path=path)
    refm = O.fixture_oracle(n, q, seed, "mean")
    check({"order": refm["order"][:1], "d2": refm["d2"][:1]}, sel.order, sel.d2)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_auto_path_equals_forced_paths_bitwise(dt):
    n, q, seed = O.FIXTURES[3]
    Zd = on_device(O.fixture_data(n, q, seed), dt)
    runs = [engine_ks(Zd, n, path=p) for p in (0, SMALL, WIDE, 0)]
    for order, d2, nbad in runs[1:]:
        assert nbad == 0
        assert np.array_equal(order, runs[0][0])
        assert np.array_equal(d2.view(np.int64), runs[0][1].view(np.int64))  # the same bits, run to run too


@pytest.mark.parametrize("path", [SMALL, WIDE])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_padded_ldz_is_read_in_place(dt, path):
    n, q, seed = O.FIXTURES[2]
    Zd = on_device(O.fixture_data(n, q, seed), dt, pad=3)
    base = Zd._base if Zd._base is not None else Zd
    for init in ("pair", "mean"):
        order, d2, nbad = engine_ks(Zd, n, init=init, path=path)
        assert nbad == 0  # the NaN padding was not read
        check(O.fixture_oracle(n, q, seed, init), order, d2)
    assert torch.isnan(base[:, q:]).all()


@pytest.mark.parametrize("path", [SMALL, WIDE])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_q130_crosses_a_chunk_edge_with_weights(dt, path):
    rng = np.random.default_rng(21)
    Z = rng.standard_normal((200, 130)).astype(np.float32)
    w = rng.uniform(0.1, 4.0, 130)
    w[5] = 0.0  # a column that does not count
    for init in ("pair", "mean"):
        for ww in (None, w):
            ref = O.kennard_stone(Z, 200, w=ww, init=init)
            assert ref["min_rel_gap"] >= O.MIN_GAP
            order, d2, nbad = engine_ks(on_device(Z, dt), 200, init=init, w=ww, path=path)
            assert nbad == 0
            check(ref, order, d2)


@pytest.mark.parametrize("path", [SMALL, WIDE])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 129])
def test_tile_and_wave_edges(n, path):
    Z = np.random.default_rng(100 + n).standard_normal((n, 5)).astype(np.float32)
    w = np.array([1.0, 0.5, 2.0, 3.0, 0.25])
    # two rows are equally far from their mean: that start is a tie no arithmetic decides
    for init in (("pair",) if n == 2 else ("pair", "mean")):
        ref = O.kennard_stone(Z, n, w=w, init=init)
        assert ref["min_rel_gap"] >= O.MIN_GAP
        for dt in ("f32", "f64"):
            order, d2, nbad = engine_ks(on_device(Z, dt), n, init=init, w=w, path=path)
            assert nbad == 0
            check(ref, order, d2)


@pytest.mark.parametrize("path", [SMALL, WIDE])
def test_explicit_start(path):
    from ocm import sampling as S

    n, q, seed = O.FIXTURES[0]
    Z = O.fixture_data(n, q, seed)
    for start, n_select in (([11], 40), ([700, 3, 1499], 200), ([5, 6], 2)):
        ref = O.kennard_stone(Z, n_select, start=start)
        assert ref["min_rel_gap"] >= O.MIN_GAP
        sel = S.kennard_stone(on_device(Z), n_select, start=start, _path=path)
        check(ref, sel.order, sel.d2)
        assert sel.order[:len(start)].tolist() == start and np.isnan(sel.d2[:len(start)]).all()


def test_rows_restrict_the_candidates():
    from ocm import sampling as S

    n, q, seed = O.FIXTURES[1]
    Z = O.fixture_data(n, q, seed)
    rows = np.random.default_rng(4).permutation(n)[:400]
    ref = O.kennard_stone(Z[rows], 150)
    assert ref["min_rel_gap"] >= O.MIN_GAP
    sel = S.kennard_stone(on_device(Z), 150, rows=rows)
    check({"order": rows[ref["order"]], "d2": ref["d2"]}, sel.order, sel.d2)
    ref = O.kennard_stone(Z[rows], 50, start=[7, 2])
    sel = S.kennard_stone(Z, 50, rows=rows, start=[int(rows[7]), int(rows[2])])
    check({"order": rows[ref["order"]], "d2": ref["d2"]}, sel.order, sel.d2)


# ------------------------------------------------------------------ exact ties

@pytest.mark.parametrize("path", [SMALL, WIDE])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_integer_grid_ties(dt, path):
    """Z ∈ {0..3}³, n = 500: many duplicates, every distance an exact small integer
    in any summation order, zero-distance picks at the end."""
    Z = np.random.default_rng(17).integers(0, 4, size=(500, 3)).astype(np.float64)
    for init in ("pair", "mean"):
        ref = O.kennard_stone(Z, 500, init=init)
        order, d2, nbad = engine_ks(on_device(Z, dt), 500, init=init, path=path)
        assert nbad == 0
        assert np.array_equal(order, ref["order"])
        if init == "pair":
            assert np.array_equal(d2, ref["d2"])  # exact
        else:
            np.testing.assert_allclose(d2, ref["d2"], rtol=RTOL, atol=0)
        assert (d2[-100:] == 0).all()  # 64 distinct points: the rest are duplicates


@pytest.mark.parametrize("path", [SMALL, WIDE])
def test_identical_rows_go_in_index_order(path):
    Z = np.full((150, 4), 0.3, dtype=np.float32)
    for init in ("pair", "mean"):
        order, d2, nbad = engine_ks(on_device(Z), 150, init=init, path=path)
        assert nbad == 0
        assert order.tolist() == list(range(150))
        assert (d2[1:] == 0).all() and abs(d2[0]) < 1e-12


def test_pair_tie_rule_on_a_grid():
    """The farthest pair of a full integer grid is attained by several pairs: the
    smallest i, then the smallest j wins, over a grid of many tiles."""
    from ocm import engine

    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    Z = np.tile(g, (9, 1)).astype(np.float32)  # 576 rows, every point nine times
    i, j, d, gap = O.farthest_pair(Z)
    assert gap == 0.0 and d == 27.0
    pair, d2, nbad = engine.ks_pair(on_device(Z))
    assert host(pair).tolist() == [i, j] and float(d2.item()) == 27.0 and int(nbad.item()) == 0


# ------------------------------------------------------------------ larger grids

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pair_large_grid_and_skip_mask(dt):
    from ocm import engine

    n, q = 5000, 5
    Z = np.random.default_rng(31).standard_normal((n, q)).astype(np.float32)
    Zd = on_device(Z, dt)
    i, j, d, gap = O.farthest_pair(Z)
    assert gap >= O.MIN_GAP
    pair, d2, nbad = engine.ks_pair(Zd)
    assert host(pair).tolist() == [i, j] and int(nbad.item()) == 0
    np.testing.assert_allclose(float(d2.item()), d, rtol=RTOL)
    skip = np.zeros(n, dtype=np.uint8)
    skip[i] = 1  # the winner's first row leaves
    skip[::7] = 1
    i2, j2, d_2, gap2 = O.farthest_pair(Z, skip=skip)
    assert gap2 >= O.MIN_GAP and i2 != i and not skip[i2] and not skip[j2]
    pair, d2, nbad = engine.ks_pair(Zd, skip=torch.from_numpy(skip).cuda())
    assert host(pair).tolist() == [i2, j2] and int(nbad.item()) == 0
    np.testing.assert_allclose(float(d2.item()), d_2, rtol=RTOL)


def test_wide_path_many_workgroups():
    n, q = 40000, 4
    Z = np.random.default_rng(41).standard_normal((n, q)).astype(np.float32)
    ref = O.kennard_stone(Z, 300, start=[7, 31000])
    assert ref["min_rel_gap"] >= O.MIN_GAP
    Zd = on_device(Z)
    for path in (WIDE, 0):
        order, d2, nbad = engine_ks(Zd, 300, start=[7, 31000], path=path)
        assert nbad == 0
        check(ref, order, d2)


# ------------------------------------------------------------------ Duplex

@pytest.mark.parametrize("path", [SMALL, WIDE])
@pytest.mark.parametrize("fx,sizes", [(1, "half"), (1, (100, 37)), (2, "half"), (2, (100, 37)), (2, (37, 100))])
def test_duplex(fx, sizes, path):
    from ocm import sampling as S

    n, q, seed = O.FIXTURES[fx]
    n_a, n_b = (n // 2, n - n // 2) if sizes == "half" else sizes
    Z = O.fixture_data(n, q, seed)
    ref = O.duplex(Z, n_a, n_b)
    assert ref["min_rel_gap"] >= O.MIN_GAP
    a, b = S.duplex(on_device(Z), n_a, None if sizes == "half" else n_b, _path=path)
    check({"order": ref["order_a"], "d2": ref["d2_a"]}, a.order, a.d2)
    check({"order": ref["order_b"], "d2": ref["d2_b"]}, b.order, b.d2)
    assert a.order.size == n_a and b.order.size == n_b
    assert not set(a.order.tolist()) & set(b.order.tolist())
    # the turns the oracle took: A, B in turn while both have room, then the larger set alone
    mn = min(n_a, n_b) - 2
    assert ref["turns"][:2 * mn].tolist() == [0, 1] * mn
    assert (ref["turns"][2 * mn:] == (0 if n_a > n_b else 1)).all()


def test_split():
    from ocm import sampling as S

    n, q, seed = O.FIXTURES[2]
    Z = O.fixture_data(n, q, seed)
    ref = O.fixture_oracle(n, q, seed, "pair")
    tr, te = S.kennard_stone_split(Z, 0.7)
    k = int(np.floor(0.7 * n))
    assert np.array_equal(tr, ref["order"][:k])
    assert np.array_equal(te, np.setdiff1d(np.arange(n), tr)) and te.size == n - k
    tr, te = S.kennard_stone_split(Z, 200, method="duplex", test_size=0.2)
    d = O.duplex(Z, 200, int(np.floor(0.2 * n)))
    assert np.array_equal(tr, d["order_a"]) and np.array_equal(te, d["order_b"])


# ------------------------------------------------------------------ PCA scores, objects

@pytest.mark.parametrize("metric", ["euclidean", "mahalanobis"])
def test_pca_route_matches_oracle_on_the_devices_scores(metric):
    from ocm import sampling as S
    from ocm import synth

    X = synth.spectra_shard(2000, 128, 0, 1, torch.device("cuda"), seed=77)
    sel = S.kennard_stone(X, 200, n_components=6, metric=metric)
    T = host(sel.scores)
    assert T.shape == (2000, 6)
    w = None
    if metric == "mahalanobis":
        w = host(sel.weights)
        assert w.shape == (6,) and (w > 0).all()
    else:
        assert sel.weights is None
    ref = O.kennard_stone(T, 200, w=w)
    assert ref["min_rel_gap"] >= O.MIN_GAP
    check(ref, sel.order, sel.d2)


def test_objects():
    from ocm import sampling as S
    from ocm.objects import object_means

    rng = np.random.default_rng(51)
    lens = rng.integers(3, 40, size=60)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    X = (rng.standard_normal((int(off[-1]), 24)) + np.repeat(rng.standard_normal((60, 24)) * 3, lens, axis=0)
         ).astype(np.float32)
    means = object_means(X, off)
    ref = O.kennard_stone(means, 25)
    assert ref["min_rel_gap"] >= O.MIN_GAP
    sel, row_mask = S.kennard_stone_objects(X, 25, offsets=off)
    check(ref, sel.order, sel.d2)
    want = np.zeros(X.shape[0], dtype=bool)
    for g in ref["order"]:
        want[off[g]:off[g + 1]] = True
    assert np.array_equal(row_mask, want) and row_mask.sum() == lens[ref["order"]].sum()
    sel2, mask2 = S.kennard_stone_objects(X, 25, objects=np.repeat(np.arange(60), lens))
    assert np.array_equal(sel2.order, sel.order) and np.array_equal(mask2, row_mask)


# ------------------------------------------------------------------ non-finite input

@pytest.mark.parametrize("path", [SMALL, WIDE])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_non_finite_rows_are_counted_and_nothing_is_written(dt, path):
    from ocm import engine
    from ocm import sampling as S

    Z = np.random.default_rng(61).standard_normal((700, 6)).astype(np.float32)
    Z[5, 2] = np.nan
    Z[300, 0] = np.inf
    Z[699, 5] = -np.inf
    Z[300, 3] = np.nan  # still one row
    Zd = on_device(Z, dt)
    out = {"order_a": torch.full((100,), -7, dtype=torch.int64, device="cuda"),
           "d2_a": torch.full((100,), -7.0, dtype=torch.float64, device="cuda")}
    res = engine.ks_select(Zd, torch.tensor([1, 2], dtype=torch.int64, device="cuda"), 100, path=path, out=out)
    assert int(res["nbad"].item()) == 3
    assert (host(out["order_a"]) == -7).all() and (host(out["d2_a"]) == -7.0).all()
    pair, d2, nbad = engine.ks_pair(Zd)
    assert int(nbad.item()) == 3
    skip = torch.zeros(700, dtype=torch.uint8, device="cuda")
    skip[300] = 1
    assert int(engine.ks_pair(Zd, skip=skip)[2].item()) == 2  # a skipped row is no candidate
    for kw in ({"init": "pair"}, {"init": "mean"}, {"start": [0, 9]}):
        with pytest.raises(ValueError, match=r"\b3 candidate row"):
            S.kennard_stone(Zd, 100, _path=path, **kw)
    with pytest.raises(ValueError, match=r"\b3 candidate row"):
        S.duplex(Zd, 50, 50, _path=path)


def test_start_out_of_range_writes_nothing():
    from ocm import engine

    Zd = on_device(np.random.default_rng(62).standard_normal((90, 3)))
    for path in (SMALL, WIDE):
        out = {"order_a": torch.full((10,), -7, dtype=torch.int64, device="cuda")}
        res = engine.ks_select(Zd, torch.tensor([3, 90], dtype=torch.int64, device="cuda"), 10, path=path, out=out)
        assert int(res["nbad"].item()) >= 1 << 30
        assert (host(out["order_a"]) == -7).all()


def test_c_abi_argument_errors():
    from ocm import engine

    Zd = on_device(np.zeros((10, 2)))
    st = torch.tensor([0], dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        engine.ks_select(Zd, st, 11)
    with pytest.raises(ValueError):
        engine.ks_select(Zd, st, 5, st, 6)
    with pytest.raises(ValueError):
        engine.ks_select(Zd, st, 5, path=3)
    big = torch.zeros((30000, 1), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="small path"):
        engine.ks_select(big, st, 5, path=SMALL)  # 30000 min distances do not fit the LDS
    with pytest.raises(ValueError):
        engine.ks_pair(on_device(np.zeros((1, 2))))
