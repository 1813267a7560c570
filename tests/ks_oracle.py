"""fp64 NumPy statements of Kennard–Stone and Duplex selection, written from the
definitions (ocm/sampling.py's docstring), for the sampling tests:

    d2(i, j) = Σ_c w_c (z_ic − z_jc)²     every input value as its exact double

Each call also returns ``min_rel_gap``: the smallest relative gap between the
best and the second-best candidate over the start and every step (Duplex's
second pair included).  A fixture whose gap is well above fp64 rounding of the
sum cannot change its order with the summation order.

``literal_*`` are O(n³) transcriptions (every distance recomputed from scratch in
Python loops) the fast forms are checked against at small n.
"""
import numpy as np


def _prep(Z, w):
    Z = np.asarray(Z).astype(np.float64)
    if Z.ndim != 2:
        raise ValueError("Z must be 2-D")
    w = np.ones(Z.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    return Z, w


def d2_to(Z, w, z):
    """d2 of every row of Z to the point z."""
    t = Z - z
    return (w * t * t).sum(axis=1)


def _gap(best, second):
    if second is None or not np.isfinite(second):
        return np.inf
    den = max(abs(best), abs(second))
    return 0.0 if den == 0.0 else abs(best - second) / den


def _top2_max(v, valid):
    """(index of the max over valid, ties to the smallest index; its value; the runner-up's value)."""
    vv = np.where(valid, v, -np.inf)
    i = int(np.argmax(vv))
    best = vv[i]
    vv[i] = -np.inf
    second = vv.max() if valid.sum() > 1 else None
    return i, float(best), (None if second is None else float(second))


def farthest_pair(Z, w=None, skip=None, chunk_elems=4_000_000):
    """(i, j, d2, rel_gap): argmax of d2 over i < j among the rows not skipped, ties to
    the smallest i, then the smallest j.  Chunked over rows."""
    Z, w = _prep(Z, w)
    n, q = Z.shape
    keep = np.ones(n, dtype=bool) if skip is None else ~np.asarray(skip).astype(bool)
    rows_per = max(1, int(chunk_elems // max(1, n * q)))
    best, bi, bj = -np.inf, -1, -1
    seconds = []
    for i0 in range(0, n, rows_per):
        i1 = min(n, i0 + rows_per)
        t = Z[i0:i1, None, :] - Z[None, :, :]
        D = (w * t * t).sum(axis=2)
        ii = np.arange(i0, i1)[:, None]
        jj = np.arange(n)[None, :]
        ok = (jj > ii) & keep[ii] & keep[jj]
        D = np.where(ok, D, -np.inf)
        flat = D.ravel()
        k = int(np.argmax(flat))
        v = flat[k]
        if flat.size > 1:
            two = np.partition(flat, flat.size - 2)[-2:]
            seconds.append(float(two[0]))
        if v > best:
            if np.isfinite(best):
                seconds.append(float(best))
            best, bi, bj = float(v), i0 + k // n, k % n
        elif np.isfinite(v):
            seconds.append(float(v))
    if not np.isfinite(best):
        raise ValueError("fewer than two rows")
    second = max([s for s in seconds if np.isfinite(s)], default=None)
    return bi, bj, best, _gap(best, second)


def _start(Z, w, init, start):
    """(order list, d2 list, gap) of the start."""
    n = Z.shape[0]
    if start is not None:
        s = [int(v) for v in start]
        assert len(s) >= 1 and len(set(s)) == len(s)
        return s, [np.nan] * len(s), np.inf
    if init == "pair":
        i, j, d, g = farthest_pair(Z, w)
        return [i, j], [d, d], g
    if init == "mean":
        v = d2_to(Z, w, Z.mean(axis=0))
        i, best, second = _top2_max(-v, np.ones(n, dtype=bool))
        return [i], [-best], _gap(best, second)
    raise ValueError(init)


def kennard_stone(Z, n_select, w=None, init="pair", start=None):
    """dict(order int64, d2 float64, min_rel_gap)."""
    Z, w = _prep(Z, w)
    n = Z.shape[0]
    order, d2, gap = _start(Z, w, init, start)
    assert len(order) <= n_select <= n
    free = np.ones(n, dtype=bool)
    free[order] = False
    m = np.full(n, np.inf)
    for s in order:
        m = np.minimum(m, d2_to(Z, w, Z[s]))
    while len(order) < n_select:
        i, best, second = _top2_max(m, free)
        gap = min(gap, _gap(best, second))
        order.append(i)
        d2.append(best)
        free[i] = False
        m = np.minimum(m, d2_to(Z, w, Z[i]))
    return {"order": np.asarray(order, dtype=np.int64), "d2": np.asarray(d2, dtype=np.float64),
            "min_rel_gap": float(gap)}


def duplex(Z, n_a, n_b, w=None):
    """dict(order_a, d2_a, order_b, d2_b, turns, min_rel_gap); ``turns``: the set
    (0 = A, 1 = B) of every step after the two pairs."""
    Z, w = _prep(Z, w)
    n = Z.shape[0]
    assert n_a >= 2 and n_b >= 2 and n_a + n_b <= n
    ia, ja, da, ga = farthest_pair(Z, w)
    skip = np.zeros(n, dtype=bool)
    skip[[ia, ja]] = True
    ib, jb, db, gb = farthest_pair(Z, w, skip=skip)
    gap = min(ga, gb)
    order = [[ia, ja], [ib, jb]]
    d2 = [[da, da], [db, db]]
    size = [n_a, n_b]
    free = np.ones(n, dtype=bool)
    free[[ia, ja, ib, jb]] = False
    m = []
    for s in range(2):
        ms = np.full(n, np.inf)
        for r in order[s]:
            ms = np.minimum(ms, d2_to(Z, w, Z[r]))
        m.append(ms)
    turns = []
    while len(order[0]) < n_a or len(order[1]) < n_b:
        for s in range(2):
            if len(order[s]) >= size[s]:
                continue  # a full set is skipped
            i, best, second = _top2_max(m[s], free)
            gap = min(gap, _gap(best, second))
            order[s].append(i)
            d2[s].append(best)
            free[i] = False
            m[s] = np.minimum(m[s], d2_to(Z, w, Z[i]))
            turns.append(s)
    return {"order_a": np.asarray(order[0], dtype=np.int64), "d2_a": np.asarray(d2[0]),
            "order_b": np.asarray(order[1], dtype=np.int64), "d2_b": np.asarray(d2[1]),
            "turns": np.asarray(turns, dtype=np.int64), "min_rel_gap": float(gap)}


# ------------------------------------------------------------------ literal O(n³) forms

def _d2_literal(Z, w, i, j):
    acc = 0.0
    for c in range(Z.shape[1]):
        t = float(Z[i, c]) - float(Z[j, c])
        acc += float(w[c]) * t * t
    return acc


def _literal_pair(Z, w, allowed):
    best, pair = -1.0, None
    for i in allowed:
        for j in allowed:
            if i < j:
                d = _d2_literal(Z, w, i, j)
                if d > best:  # strict: the first (smallest i, then j) of equal pairs stays
                    best, pair = d, (i, j)
    return pair, best


def _literal_next(Z, w, members, free):
    best, pick = -1.0, None
    for i in free:  # ascending: strict > keeps the smallest index of a tie
        mi = min(_d2_literal(Z, w, i, s) for s in members)
        if mi > best:
            best, pick = mi, i
    return pick, best


def literal_kennard_stone(Z, n_select, w=None, init="pair", start=None):
    Z, w = _prep(Z, w)
    n = Z.shape[0]
    if start is not None:
        order, d2 = [int(v) for v in start], [np.nan] * len(start)
    elif init == "pair":
        (i, j), d = _literal_pair(Z, w, list(range(n)))
        order, d2 = [i, j], [d, d]
    else:
        c = Z.mean(axis=0)
        best, pick = np.inf, None
        for i in range(n):
            d = sum(float(w[k]) * (float(Z[i, k]) - float(c[k])) ** 2 for k in range(Z.shape[1]))
            if d < best:
                best, pick = d, i
        order, d2 = [pick], [best]
    while len(order) < n_select:
        free = [i for i in range(n) if i not in order]
        pick, best = _literal_next(Z, w, order, free)
        order.append(pick)
        d2.append(best)
    return np.asarray(order, dtype=np.int64), np.asarray(d2, dtype=np.float64)


def literal_duplex(Z, n_a, n_b, w=None):
    Z, w = _prep(Z, w)
    n = Z.shape[0]
    (i, j), d = _literal_pair(Z, w, list(range(n)))
    order, d2 = [[i, j], []], [[d, d], []]
    (i, j), d = _literal_pair(Z, w, [r for r in range(n) if r not in order[0]])
    order[1], d2[1] = [i, j], [d, d]
    size = [n_a, n_b]
    while len(order[0]) < n_a or len(order[1]) < n_b:
        for s in range(2):
            if len(order[s]) >= size[s]:
                continue
            free = [r for r in range(n) if r not in order[0] and r not in order[1]]
            pick, best = _literal_next(Z, w, order[s], free)
            order[s].append(pick)
            d2[s].append(best)
    return (np.asarray(order[0], dtype=np.int64), np.asarray(d2[0]), np.asarray(order[1], dtype=np.int64),
            np.asarray(d2[1]))


# ------------------------------------------------------------------ shared fixtures

# (n, q, seed): standard normal float32 rows, all n rows selected
FIXTURES = [(1500, 7, 3), (1000, 20, 5), (513, 33, 7), (300, 64, 9), (130, 1, 11), (2100, 3, 13)]
MIN_GAP = 1e-10  # precondition on a continuous fixture (a condition on the inputs, not an allowance)

_cache = {}


def fixture_data(n, q, seed):
    return np.random.default_rng(seed).standard_normal((n, q)).astype(np.float32)


def fixture_oracle(n, q, seed, init):
    """The oracle's full-length run on a fixture, computed once per session."""
    key = (n, q, seed, init)
    if key not in _cache:
        _cache[key] = kennard_stone(fixture_data(n, q, seed), n, init=init)
    return _cache[key]
