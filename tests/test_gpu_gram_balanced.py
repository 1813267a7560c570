"""Balanced chunks of the i8×3 Gram (chunk_rows < 0: −chunk_rows chunks of
⌊B/N⌋ or ⌈B/N⌉ scale blocks over block-major digit planes, include/ocm.h).

Equality, torch.equal on G and the column sums:
  * k_gram8e (mode "i8x3") against k_gram8d ("i8x3k32") at forced counts: the
    same exact int32 digit sums flushed to f32 in the same order, so the two
    are bit for bit equal at any chunk length.  One ×800 outlier row goes
    through the screen and the exact fix-up.
        p = 256, n = 7·1536 + 100 (B = 8): N = 3 (3, 3, 2), 5 (2, 2, 2, 1, 1),
                                           8 (one block each), 20 (clamped to 8)
        p = 200 (padded columns), same n:  N = 3
        p = 2048, n = 3·1536 (B = 3):      N = 2 (2, 1)
  * a negative count with a gather list, or with three segments, is the uniform
    automatic choice.  The shape makes that choice 4608 rows on the device's
    own CU count (p = 2048: ⌈4·CUs / 136⌉ chunks wanted, 4608 rows once a
    chunk would exceed 3072), so the result must equal chunk_rows = 4608 to
    the bit.  This needs n > 3072·⌈4·CUs / 136⌉ rows, 26,000 × 2048 on 256 CUs:
    the one shape here above 100 MB.
  * the lazy-view quantiser (SNV + window 5; window 15 without SNV) against
    the materialised rows at N = 3 on the first shape.

Accuracy: n = 12·1536, p = 256, e = max|G − G64| / max|G64| with G64 the
float64 matmul of the shifted rows.  One 12-block chunk (N = 1) against
chunk_rows = 4608 (3-block chunks): e(N = 1) ≤ 4 · e(4608).  The int32 sums are
exact per scale block at any chunk length; what grows with the length is the
f32 running sum of a chunk's block flushes, by at most 12/3 = 4 if it were the
only error.  Both values are printed.
"""
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

N8 = 7 * 1536 + 100


@pytest.fixture(scope="module")
def eng():
    from ocm import engine

    return engine


_data = {}


def _case(eng, n, p, outlier=True):
    """X (recipe of test_gpu_gram_roundsweep.py: one ×800 outlier row) and its
    shift, made once per shape on the device and never written again."""
    import torch

    key = (n, p, outlier)
    if key not in _data:
        g = torch.Generator(device="cuda").manual_seed(n + p)
        X = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float32)
        X = X * (0.1 + 2.9 * torch.rand(p, generator=g, device="cuda")) + 1.0
        if outlier:
            X[n // 5] *= 800.0
        shift = eng.cast_f32(eng.colmean(X, None, 4096))
        _data[key] = (X, shift)
    return _data[key]


@pytest.mark.parametrize("n,p,N", [(N8, 256, 3), (N8, 256, 5), (N8, 256, 8), (N8, 256, 20), (N8, 200, 3),
                                   (3 * 1536, 2048, 2)])
def test_forced_counts_bit_identical_between_kernels(eng, n, p, N):
    import torch

    X, shift = _case(eng, n, p)
    Ga, ca = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=-N)
    assert eng.last_gram_marks(0) > 0
    Gb, cb = eng.gram(X, None, [0, n], shift, mode="i8x3k32", chunk_rows=-N)
    assert torch.equal(Ga, Gb)
    assert torch.equal(ca, cb)
    assert torch.isfinite(Ga).all()


def test_clamped_count_is_one_block_per_chunk(eng):
    """N = 20 on B = 8 blocks is N = 8; single-block chunks are also what
    chunk_rows = 1536 cuts (the last block holds 100 rows either way)."""
    import torch

    X, shift = _case(eng, N8, 256)
    G20, c20 = eng.gram(X, None, [0, N8], shift, mode="i8x3", chunk_rows=-20)
    G8, c8 = eng.gram(X, None, [0, N8], shift, mode="i8x3", chunk_rows=-8)
    Gu, cu = eng.gram(X, None, [0, N8], shift, mode="i8x3", chunk_rows=1536)
    assert torch.equal(G20, G8) and torch.equal(c20, c8)
    assert torch.equal(G8, Gu) and torch.equal(c8, cu)


def _fallback_shape():
    """(n, p) at which the uniform automatic choice is 4608 rows, for n − 100
    gathered rows as for n rows in three segments."""
    import torch

    C = torch.cuda.get_device_properties(0).multi_processor_count
    p, ntiles = 2048, 136
    want = max(1, (4 * C + ntiles - 1) // ntiles)
    n = 3072 * want + 1424
    for m in (n, n - 100):
        assert 3072 < min(4096, -(-m // want))  # → 4608 after rounding up to whole blocks
    return n, p


@pytest.mark.parametrize("kind", ["gather", "segments"])
def test_negative_count_falls_back_to_uniform(eng, kind):
    import torch

    n, p = _fallback_shape()
    X, shift = _case(eng, n, p)
    if kind == "gather":
        g = torch.Generator(device="cuda").manual_seed(3)
        rows = torch.sort(torch.randperm(n, generator=g, device="cuda")[: n - 100]).values.to(torch.int64)
        seg = [0, n - 100]
    else:
        rows = None
        seg = [0, n // 3 + 11, 2 * n // 3 - 700, n]
    Ga, ca = eng.gram(X, rows, seg, shift, mode="i8x3", chunk_rows=-3)
    Gb, cb = eng.gram(X, rows, seg, shift, mode="i8x3", chunk_rows=4608)
    assert torch.equal(Ga, Gb)
    assert torch.equal(ca, cb)


@pytest.mark.parametrize("snv,w", [(True, 5), (False, 15)])
def test_lazy_view_bit_identical_at_forced_count(eng, snv, w):
    import torch

    from ocm import preprocess
    from ocm.prepview import materialised_count

    X, _ = _case(eng, N8, 256)
    v = preprocess.snv_savgol(X, w, 2, 1, 1.0, snv=snv, lazy=True)
    Y = v.materialize()
    sa = eng.cast_f32(eng.colmean(v, None, 4096))
    sb = eng.cast_f32(eng.colmean(Y, None, 4096))
    assert torch.equal(sa, sb)
    c0 = materialised_count(0)
    Ga, ca = eng.gram(v, None, [0, N8], sa, mode="i8x3", chunk_rows=-3)
    assert materialised_count(0) == c0  # the fused quantiser ran
    Gb, cb = eng.gram(Y, None, [0, N8], sb, mode="i8x3", chunk_rows=-3)
    assert torch.equal(Ga, Gb)
    assert torch.equal(ca, cb)


def test_one_long_chunk_accuracy_against_float64(eng):
    """Measured on MI355X: e(N = 1) = 1.49e-7, e(4608) = 4.78e-8, ratio 3.1
    (precision choices)."""
    n, p = 12 * 1536, 256
    X, shift = _case(eng, n, p, outlier=False)
    Y = X.double() - shift.double()
    G64 = Y.T @ Y

    def err(chunk_rows):
        G, _ = eng.gram(X, None, [0, n], shift, mode="i8x3", chunk_rows=chunk_rows)
        return ((G[0] - G64).abs().max() / G64.abs().max()).item()

    e1, e3 = err(-1), err(4608)
    print(f"balanced N=1 (12 blocks per chunk): e = {e1:.3e}; chunk_rows 4608 (3 blocks): e = {e3:.3e}; "
          f"ratio {e1 / e3:.2f}")
    assert e1 <= 4 * e3
