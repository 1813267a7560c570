"""The persistent i8×3 Gram launch (k_gram8e) with its item count set around
the boundaries of the work map's rounds (ocm_gram_map.h: a round is one item
per workgroup, C workgroups on a device of C CUs), against k_gram8d (mode
"i8x3k32", one item per workgroup, untouched): the same exact int32 digit sums
flushed to f32 in the same order whichever workgroup runs an item, so G and the
column sums are bit for bit equal.

Data recipe of test_gpu_gram_persistent.py (one ×800 outlier row, a sorted
gather list with an empty segment).  p = 512 with chunk_rows = 1536 gives 9
items per chunk; n = 1536·m + 1 rows are m full chunks and a one-row chunk,
9·(m + 1) items, for the device's own C (multi_processor_count):

    m = ⌊C/9⌋        one round, within 9 items of its end (C = 256: 261 items, one round and 5)
    m = ⌊C/9⌋ + 1    one round plus a few items (C = 256: 270)
    m = ⌊3C/9⌋ + 1   three rounds plus a remainder (C = 256: 783)

and one shape at the bench tile count, p = 2048, n = 20,000 (132 items per
chunk).  The largest is ≈ 130k × 512.
"""
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CASES = ["under_one_round", "one_round_and_some", "three_rounds_and_some", "p2048"]


@pytest.fixture(scope="module")
def eng():
    from ocm import engine

    return engine


def _shape(case):
    import torch

    C = torch.cuda.get_device_properties(0).multi_processor_count
    if case == "p2048":
        return 20000, 2048, 0
    m = {"under_one_round": C // 9, "one_round_and_some": C // 9 + 1, "three_rounds_and_some": 3 * C // 9 + 1}[case]
    return 1536 * m + 1, 512, 1536


_data = {}


def _case(eng, n, p):
    """X (one ×800 outlier row), its shift and a sorted gather list of n − 100
    rows, made once per shape on the device and never written again."""
    import torch

    if (n, p) not in _data:
        g = torch.Generator(device="cuda").manual_seed(n + p)
        X = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float32)
        X = X * (0.1 + 2.9 * torch.rand(p, generator=g, device="cuda")) + 1.0
        X[n // 5] *= 800.0  # one screened row (exact fix-up in both kernels)
        shift = eng.cast_f32(eng.colmean(X, None, 4096))
        rows = torch.sort(torch.randperm(n, generator=g, device="cuda")[: n - 100]).values.to(torch.int64)
        _data[(n, p)] = (X, shift, rows)
    return _data[(n, p)]


@pytest.mark.parametrize("case", CASES)
def test_one_segment_bit_identical(eng, case):
    import torch

    n, p, chunk = _shape(case)
    X, shift, _ = _case(eng, n, p)
    Ga, ca = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=chunk)
    Gb, cb = eng.gram(X, None, [0, n], shift, mode="i8x3k32", chunk_rows=chunk)
    assert torch.equal(Ga, Gb)
    assert torch.equal(ca, cb)


@pytest.mark.parametrize("case", CASES)
def test_segments_over_gather_list_bit_identical(eng, case):
    import torch

    n, p, chunk = _shape(case)
    X, shift, rows = _case(eng, n, p)
    m = n - 100
    seg = [0, m // 3, m // 3, m]  # the middle segment is empty
    Ga, ca = eng.gram(X, rows, seg, shift, mode="i8x3", chunk_rows=chunk)
    Gb, cb = eng.gram(X, rows, seg, shift, mode="i8x3k32", chunk_rows=chunk)
    assert torch.equal(Ga, Gb)
    assert torch.equal(ca, cb)
    assert not Ga[1].any() and not ca[1].any()
