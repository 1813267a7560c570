"""Host-side checks of ocm.sampling: the NumPy oracle against a literal O(n³)
transcription of the definitions, the Selection helpers, the split arithmetic,
the argument errors (raised before a device is asked for) and the preconditions
of the fixtures the GPU tests compare on."""
import numpy as np
import pytest

import ks_oracle as O
from ocm import sampling as S


@pytest.mark.parametrize("n,q,seed", [(2, 3, 0), (3, 1, 1), (7, 2, 2), (12, 5, 3), (11, 4, 4)])
@pytest.mark.parametrize("init", ["pair", "mean"])
def test_oracle_matches_literal_definition(n, q, seed, init):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, q)).astype(np.float32)
    w = rng.uniform(0.2, 3.0, q) if seed % 2 else None
    got = O.kennard_stone(Z, n, w=w, init=init)
    order, d2 = O.literal_kennard_stone(Z, n, w=w, init=init)
    assert np.array_equal(got["order"], order)
    np.testing.assert_allclose(got["d2"], d2, rtol=1e-13)
    assert sorted(order.tolist()) == list(range(n))


def test_oracle_explicit_start_and_partial_selection():
    Z = np.random.default_rng(8).standard_normal((12, 3))
    got = O.kennard_stone(Z, 7, start=[5, 2])
    order, d2 = O.literal_kennard_stone(Z, 7, start=[5, 2])
    assert np.array_equal(got["order"], order) and order[:2].tolist() == [5, 2]
    assert np.isnan(got["d2"][:2]).all()
    np.testing.assert_allclose(got["d2"][2:], d2[2:], rtol=1e-13)


@pytest.mark.parametrize("n,n_a,n_b", [(12, 6, 6), (12, 7, 3), (11, 2, 6), (9, 4, 5)])
def test_oracle_duplex_matches_literal_definition(n, n_a, n_b):
    Z = np.random.default_rng(n + n_a).standard_normal((n, 3)).astype(np.float32)
    got = O.duplex(Z, n_a, n_b)
    oa, da, ob, db = O.literal_duplex(Z, n_a, n_b)
    assert np.array_equal(got["order_a"], oa) and np.array_equal(got["order_b"], ob)
    np.testing.assert_allclose(got["d2_a"], da, rtol=1e-13)
    np.testing.assert_allclose(got["d2_b"], db, rtol=1e-13)
    assert not set(oa.tolist()) & set(ob.tolist())
    # the sets alternate A, B while both have room, then the larger one runs alone
    mn = min(n_a, n_b) - 2
    assert got["turns"][:2 * mn].tolist() == [0, 1] * mn
    assert len(set(got["turns"][2 * mn:].tolist())) <= 1


def test_oracle_ties_go_to_the_smallest_index():
    Z = np.zeros((6, 2))
    got = O.kennard_stone(Z, 6)
    assert got["order"].tolist() == [0, 1, 2, 3, 4, 5] and (got["d2"] == 0).all()
    assert got["min_rel_gap"] == 0.0
    g = np.stack(np.meshgrid(np.arange(3), np.arange(3)), -1).reshape(-1, 2).astype(np.float64)
    order, _ = O.literal_kennard_stone(g, 9)
    assert np.array_equal(O.kennard_stone(g, 9)["order"], order)


@pytest.mark.parametrize("init", ["pair", "mean"])
def test_d2_is_monotone(init):
    got = O.kennard_stone(np.random.default_rng(1).standard_normal((200, 4)), 200, init=init)
    t0 = 2 if init == "pair" else 1
    assert (np.diff(got["d2"][t0:]) <= 0).all()
    assert got["d2"][t0] <= got["d2"][0] or init == "mean"


@pytest.mark.parametrize("n,q,seed", O.FIXTURES)
@pytest.mark.parametrize("init", ["pair", "mean"])
def test_fixture_preconditions(n, q, seed, init):
    """Every continuous fixture of tests/test_gpu_sampling.py keeps its best and
    second-best candidates ≥ 1e-10 apart (relative) at the start and at every step;
    fp64 rounding of a q-term sum is below (q + 3)·2⁻⁵³, so no summation order can
    change the order."""
    r = O.fixture_oracle(n, q, seed, init)
    assert r["min_rel_gap"] >= O.MIN_GAP, r["min_rel_gap"]
    assert sorted(r["order"].tolist()) == list(range(n))


def test_selection_helpers():
    sel = S.Selection(np.array([4, 0, 2], dtype=np.int64), np.array([9.0, 9.0, 4.0]))
    assert sel.mask(6).tolist() == [True, False, True, False, True, False]
    assert sel.rest(6).tolist() == [1, 3, 5] and sel.rest(6).dtype == np.int64
    np.testing.assert_array_equal(sel.distance, [3.0, 3.0, 2.0])


def test_split_size_arithmetic():
    assert S.split_sizes(100, 70) == (70, 30)
    assert S.split_sizes(100, 0.7) == (70, 30)
    assert S.split_sizes(10, 0.75) == (7, 3)          # a fraction rounds down
    assert S.split_sizes(100, 0.7, 0.15, "duplex") == (70, 15)
    assert S.split_sizes(100, 60, None, "duplex") == (60, 40)
    assert S.split_sizes(100, 60, 10, "duplex") == (60, 10)
    for bad in (0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError):
            S.split_sizes(100, bad)
    with pytest.raises(ValueError):
        S.split_sizes(100, 70, 20, "ks")              # ks: the test set is the rest
    with pytest.raises(ValueError):
        S.split_sizes(100, 70, 40, "duplex")          # more rows than there are
    with pytest.raises(ValueError):
        S.split_sizes(100, 70, None, "random")


def test_argument_errors_come_before_the_device():
    """Each of these raises ValueError from the host checks: none of them reaches
    the device (there is none where the CPU tests run, and that would be an
    OcmError)."""
    X = np.random.default_rng(0).standard_normal((20, 4)).astype(np.float32)
    for n_select in (1, 21, 0, -3):                   # init="pair" starts with 2
        with pytest.raises(ValueError, match="n_select"):
            S.kennard_stone(X, n_select)
    with pytest.raises(ValueError, match="n_select"):
        S.kennard_stone(X, 0, init="mean")
    with pytest.raises(ValueError, match="n_select"):
        S.kennard_stone(X, 2, start=[1, 2, 3])        # below len(start)
    with pytest.raises(ValueError, match="n_select"):
        S.kennard_stone(X, 5, rows=[0, 1, 2])         # above the candidates
    with pytest.raises(ValueError, match="duplicate"):
        S.kennard_stone(X, 5, start=[3, 7, 3])
    with pytest.raises(ValueError, match="start"):
        S.kennard_stone(X, 5, start=[20])
    with pytest.raises(ValueError, match="start"):
        S.kennard_stone(X, 5, start=[])
    with pytest.raises(ValueError, match="start"):
        S.kennard_stone(X, 3, start=[9], rows=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="n_components"):
        S.kennard_stone(X, 5, metric="mahalanobis")
    with pytest.raises(ValueError, match="metric"):
        S.kennard_stone(X, 5, metric="cosine")
    with pytest.raises(ValueError, match="init"):
        S.kennard_stone(X, 5, init="random")
    with pytest.raises(ValueError, match="n_components"):
        S.kennard_stone(X, 5, n_components=5)
    for frac in (0.0, 1.0, 1.2):
        with pytest.raises(ValueError, match="train_size"):
            S.kennard_stone_split(X, frac)
    with pytest.raises(ValueError, match="n_a"):
        S.duplex(X, 19)
    with pytest.raises(ValueError, match="n_b"):
        S.duplex(X, 10, 11)
    with pytest.raises(ValueError, match="mahalanobis"):
        S.duplex(X, 10, metric="mahalanobis")
    with pytest.raises(ValueError):
        S.kennard_stone_objects(X, 2)                 # neither objects nor offsets
    with pytest.raises(ValueError, match="n_select"):
        S.kennard_stone_objects(X, 9, offsets=[0, 5, 12, 20])
