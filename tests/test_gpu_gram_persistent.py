"""The persistent i8×3 Gram launch (k_gram8e: one workgroup per CU walking its
share of the (chunk, tile) items, the next item's first stage prefetched by the
current item's last, an item's partials stored under the next item's MFMAs)
against k_gram8d (mode "i8x3k32", one item per workgroup, untouched): the same
exact int32 digit sums flushed to f32 in the same order, so G and the column
sums are bit for bit equal.  Method of test_gram_i8_kernels_bit_identical (one
×800 outlier row, a gather list with an empty segment); the shapes take every
path of the item loop:

    n              p     chunk_rows
    3 000          512   1536   18 items < workgroups: one item or none each
    1536·90 + 700  512   1536   91 chunks × 9 items: ≥ 3 items per workgroup, a remainder mod 8, a ragged last chunk
    9 000          257   auto   dead waves, padded columns
    20 000         2048  auto   the bench tile count (136 tiles)
"""
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SHAPES = [(3000, 512, 1536), (1536 * 90 + 700, 512, 1536), (9000, 257, 0), (20000, 2048, 0)]


@pytest.fixture(scope="module")
def eng():
    from ocm import engine

    return engine


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


@pytest.mark.parametrize("n,p,chunk", SHAPES)
def test_one_segment_bit_identical(eng, n, p, chunk):
    import torch

    X, shift, _ = _case(eng, n, p)
    Ga, ca = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=chunk)
    Gb, cb = eng.gram(X, None, [0, n], shift, mode="i8x3k32", chunk_rows=chunk)
    assert torch.equal(Ga, Gb)
    assert torch.equal(ca, cb)


@pytest.mark.parametrize("n,p,chunk", SHAPES)
def test_segments_over_gather_list_bit_identical(eng, n, p, chunk):
    import torch

    X, shift, rows = _case(eng, n, p)
    m = n - 100
    seg = [0, m // 3, m // 3, m]  # the middle segment is empty
    Ga, ca = eng.gram(X, rows, seg, shift, mode="i8x3", chunk_rows=chunk)
    Gb, cb = eng.gram(X, rows, seg, shift, mode="i8x3k32", chunk_rows=chunk)
    assert torch.equal(Ga, Gb)
    assert torch.equal(ca, cb)
    assert not Ga[1].any() and not ca[1].any()


@pytest.mark.parametrize("n,p,chunk", SHAPES)
def test_two_calls_in_a_row_equal(eng, n, p, chunk):
    import torch

    X, shift, _ = _case(eng, n, p)
    G1, c1 = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=chunk)
    G2, c2 = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=chunk)
    assert torch.equal(G1, G2)
    assert torch.equal(c1, c2)


def test_captured_gram_replays_equal_eager(eng):
    """The launch derives every item from blockIdx alone (no counter to reset),
    so a Gram captured into a graph gives the eager result on every replay."""
    import torch

    n, p, chunk = SHAPES[0]
    X, shift, _ = _case(eng, n, p)
    Ge, ce = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=chunk)  # eager (also sizes the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Gg, cg = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=chunk)
    for _ in range(2):
        Gg.zero_()
        cg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Gg, Ge)
        assert torch.equal(cg, ce)
