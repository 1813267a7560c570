"""Images into objects on the GPU (ocm.image; ocm_fgmask_f32 / _f64,
ocm_label_u8, ocm_gather_rows_f32 / _f64) against scipy.ndimage.label and
NumPy: label images equal to SciPy's to the last number, the mask equal to
NumPy's, gathered rows equal bit for bit, extract_objects equal to
objects_from_labels(SciPy's labels) on the host, and the objects of a scene
through SIMCA.predict_objects.

Shapes follow the labelling kernel's tile (LB_TH × LB_TW, read from the
source): below, at and past one tile, and several tiles with a ragged edge."""
import contextlib
import functools
import io
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(REPO, "ocm-vae-simca_amd", "csrc", "ocm_label.hip")).read()
TH = int(re.search(r"constexpr int LB_TH = (\d+);", SRC).group(1))
TW = int(re.search(r"constexpr int LB_TW = (\d+);", SRC).group(1))
FULL = np.ones((3, 3))
STRUCTURE = {4: None, 8: FULL}  # ndimage.label's default structure is the cross

SHAPES = [(1, 1), (1, 200), (200, 1), (2, 2), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 3)]


def check_label(mask, conn, tag=""):
    from ocm import image

    ref, n_ref = ndimage.label(mask, structure=STRUCTURE[conn])
    got, n = image.label(torch.from_numpy(np.ascontiguousarray(mask)).cuda(), conn)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32 and got.shape == mask.shape
    assert isinstance(n, int) and n == n_ref, (tag, n, n_ref)
    assert np.array_equal(got.cpu().numpy(), ref), tag
    return n


# ------------------------------------------------------------------ 1. label parity
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("conn", [4, 8])
def test_label_equals_scipy(conn, shape):
    H, W = shape
    rng = np.random.default_rng(100 * H + W)
    yy, xx = np.mgrid[:H, :W]
    masks = {"empty": np.zeros(shape, dtype=bool), "full": np.ones(shape, dtype=bool),
             "checkerboard": (yy + xx) % 2 == 0}
    for d in (0.3, 0.45, 0.6, 0.8):
        masks[f"random{d}"] = rng.random(shape) < d
    for name, mask in masks.items():
        n = check_label(mask, conn, f"{shape} conn={conn} {name}")
        if name == "checkerboard" and conn == 4:  # every foreground pixel its own object: the largest G
            assert n == mask.sum()
        if name == "full":
            assert n == 1


def test_label_numpy_in_numpy_out_and_nonbool_masks():
    from ocm import image

    rng = np.random.default_rng(7)
    mask = rng.random((TH + 5, TW + 9)) < 0.5
    ref, n_ref = ndimage.label(mask, structure=FULL)
    got, n = image.label(mask)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and n == n_ref and np.array_equal(got, ref)
    got_f, n_f = image.label(torch.from_numpy(mask * 7.5).cuda())  # non-zero is foreground
    assert n_f == n_ref and np.array_equal(got_f.cpu().numpy(), ref)


def spiral(n):
    """A one-pixel path from (0, 0) inwards with one-pixel gaps between its turns."""
    m = np.zeros((n, n), dtype=bool)
    y = x = 0
    m[0, 0] = True
    lengths = [n - 1, n - 1, n - 1] + [v for k in range(n - 3, 0, -2) for v in (k, k)]
    for i, length in enumerate(lengths):
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[i % 4]
        for _ in range(length):
            y, x = y + dy, x + dx
            m[y, x] = True
    return m


def structured():
    H, W = 4 * TH + 1, 2 * TW + 1  # 129 × 129 at the 32 × 64 tile
    n = min(H, W)
    out = {"spiral": spiral(n)}
    serp = np.zeros((H, W), dtype=bool)
    serp[0::2, :] = True
    serp[1::4, -1] = True
    serp[3::4, 0] = True
    out["serpentine"] = serp
    # whole tiles down the diagonal: consecutive steps touch only across a tile corner
    stair = np.zeros((H, W), dtype=bool)
    for k in range(min(H // TH, W // TW)):
        stair[k * TH:(k + 1) * TH, k * TW:(k + 1) * TW] = True
    out["staircase"] = stair
    anti = np.zeros((H, W), dtype=bool)
    ntx = W // TW
    for k in range(min(H // TH, ntx)):
        anti[k * TH:(k + 1) * TH, (ntx - 1 - k) * TW:(ntx - k) * TW] = True
    out["staircase_anti"] = anti
    # thin steps: single pixels either side of every tile corner, both diagonals
    thin = np.zeros((H, W), dtype=bool)
    for y in range(TH, H, TH):
        for x in range(TW, W, TW):
            thin[y - 1, x - 1] = thin[y, x] = True
            if y + TH // 2 < H:
                thin[y + TH // 2 - 1, x] = thin[y + TH // 2, x - 1] = True
    out["corner_pixels"] = thin
    combs = np.zeros((H, W), dtype=bool)
    combs[0, :] = combs[H - 1, :] = True
    combs[0:H - 2, 0::4] = True
    combs[2:H, 2::4] = True
    out["combs"] = combs
    frame = np.zeros((H, W), dtype=bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    yy, xx = np.mgrid[:H, :W]
    frame |= (yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= (n // 4) ** 2
    out["frame_island"] = frame
    return out


@pytest.mark.parametrize("name", ["spiral", "serpentine", "staircase", "staircase_anti", "corner_pixels", "combs",
                                  "frame_island"])
def test_structured_masks(name):
    mask = structured()[name]
    n4 = check_label(mask, 4, name)
    n8 = check_label(mask, 8, name)
    check_label(mask.T.copy(), 4, name + " transposed")
    check_label(mask.T.copy(), 8, name + " transposed")
    if name in ("spiral", "serpentine"):
        assert n4 == n8 == 1
    if name in ("staircase", "staircase_anti"):
        assert n8 == 1 and n4 > 1  # one component through the corners, one per step without them
    if name in ("combs", "frame_island"):
        assert n4 == n8 == 2


@pytest.mark.parametrize("conn,density", [(4, 0.59), (8, 0.41)])
def test_label_large_near_percolation(conn, density):
    mask = np.random.default_rng(conn).random((1024, 1024)) < density
    n = check_label(mask, conn, f"1024x1024 conn={conn}")
    assert n > 1000


def test_label_argument_errors():
    from ocm import _lib

    lib, ctx = _lib.load(), _lib.Context.get(0).handle
    st = _lib.stream_handle(torch.device("cuda", 0))
    mask = torch.ones(16, dtype=torch.uint8, device="cuda")
    lab = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    call = lambda H, W, c: lib.ocm_label_u8(ctx, _lib.ptr(mask), H, W, c, _lib.ptr(lab), _lib.ptr(n), st)
    for H, W, c in ((4, 4, 3), (4, 4, 0), (0, 4, 8), (4, 0, 8), (-1, 4, 4), (65536, 32768, 8), (65536, 32768, 4)):
        assert call(H, W, c) == _lib.OCM_ERR_ARG, (H, W, c)
        assert lib.ocm_label_u8(ctx, None, H, W, c, None, None, st) == _lib.OCM_ERR_ARG
    torch.cuda.synchronize()
    assert (lab == -7).all() and int(n) == -7  # nothing was launched
    assert lib.ocm_label_u8(ctx, None, 4, 4, 8, _lib.ptr(lab), _lib.ptr(n), st) == _lib.OCM_ERR_ARG
    assert call(4, 4, 8) == 0
    torch.cuda.synchronize()
    assert (lab == 1).all() and int(n) == 1


# ------------------------------------------------------------------ 2. the mask pass
def padded(a, pad, fill=float("nan")):
    """`a` on the device as a slice of a buffer `pad` elements wider in the last axis, `fill` in the pad."""
    t = torch.from_numpy(np.array(a))
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + pad,), fill, dtype=t.dtype, device="cuda")
    buf[..., :a.shape[-1]] = t.cuda()
    return buf[..., :a.shape[-1]]


@functools.lru_cache(maxsize=None)
def mask_cube(p, dtype):
    """(9, 11, p): background exactly 0; two thirds of the foreground with values in [1, 2], the rest in
    [0.01, 0.02] (every foreground mean ≥ 0.01); one NaN pixel."""
    rng = np.random.default_rng(p)
    cube = np.zeros((9, 11, p), dtype=dtype)
    fg = rng.random((9, 11)) < 0.6
    high = rng.random((9, 11)) < 0.66
    vals = rng.uniform(1.0, 2.0, size=(9, 11, p))
    vals[~high] *= 0.01
    cube[fg] = vals[fg].astype(dtype)
    cube[4, 5] = 0.0
    cube[4, 5, p // 2] = np.nan
    cube.setflags(write=False)
    return cube


@pytest.mark.parametrize("pad", [0, 3, 1])  # ldx = p + 1: 16-byte loads and a scalar tail at p = 7
@pytest.mark.parametrize("p", [1, 7, 256, 2050])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_foreground_mask(dtype, p, pad):
    """The mask equals NumPy's ~(mean < thr).  The reference averages in the cube's dtype (float32
    here) and the kernel in fp64, so the thresholds are kept away from rounding: every mean is 0,
    in [0.01, 0.02] or in [1, 2] against thresholds 1e-6 and 0.5.  mean_out against the float64
    mean within p·2⁻⁵³·Σ|x|/p: the error bound of a float64 sum of p terms in any order, over p."""
    from ocm import image

    cube = mask_cube(p, dtype)
    Xd = padded(cube, pad)
    assert Xd.stride(1) == p + pad
    with np.errstate(invalid="ignore"):
        mean_np = cube.mean(axis=2)
        mean64 = cube.astype(np.float64).mean(axis=2)
        bound = p * 2.0 ** -53 * np.abs(cube.astype(np.float64)).sum(axis=2) / p
    for thr in (1e-6, 0.5):
        with np.errstate(invalid="ignore"):
            want = ~(mean_np < thr)
        assert want[4, 5] and 0 < want.sum() < want.size
        got, mean = image.foreground_mask(Xd, thr, return_mean=True)
        assert got.dtype == torch.bool and got.shape == (9, 11) and mean.dtype == torch.float64
        assert np.array_equal(got.cpu().numpy(), want), thr
        assert torch.equal(image.foreground_mask(Xd, thr), got)
    mean = mean.cpu().numpy()
    assert np.isnan(mean[4, 5]) and np.isnan(mean64[4, 5])
    ok = ~np.isnan(mean64)
    err = np.abs(mean - mean64)[ok]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.where(bound[ok] > 0, err / bound[ok], 0.0)))
    print(f"{np.dtype(dtype).name} p={p} ldx=p+{pad}: largest |mean − ref| / bound {ratio:.4f}")
    assert (err <= bound[ok]).all()
    assert (mean[cube.astype(np.float64).sum(axis=2) == 0] == 0).all()
    host = image.foreground_mask(cube.copy())  # NumPy in, NumPy out; the default threshold
    assert isinstance(host, np.ndarray) and host.dtype == np.bool_
    with np.errstate(invalid="ignore"):
        assert np.array_equal(host, ~(mean_np < 1e-6))


# ------------------------------------------------------------------ 3. the row gather
@functools.lru_cache(maxsize=None)
def any_bits(m, p, dtype):
    """Arbitrary bit patterns (NaNs with payloads, infinities, denormals among them)."""
    rng = np.random.default_rng(m + p)
    it = np.int32 if dtype == np.float32 else np.int64
    a = rng.integers(np.iinfo(it).min, np.iinfo(it).max, size=(m, p), dtype=it).view(dtype)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("pad_src,pad_dst", [(0, 0), (3, 0), (0, 3), (4, 4), (1, 3)])
@pytest.mark.parametrize("p", [1, 3, 37, 256, 2050])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gather_rows_bit_equal(dtype, p, pad_src, pad_dst):
    from ocm import _lib, image

    m = 301
    X = any_bits(m, p, dtype)
    it = np.int32 if dtype == np.float32 else np.int64
    Xd = padded(X, pad_src, fill=0.0)
    rng = np.random.default_rng(p)
    some = np.sort(rng.choice(m, size=77, replace=False))
    cases = {"sorted": some, "reversed": some[::-1].copy(), "repeated": rng.integers(0, m, size=500),
             "all": np.arange(m), "one": np.array([m - 1]), "none": np.zeros(0, dtype=np.int64)}
    lib, ctx = _lib.load(), _lib.Context.get(0).handle
    fn = lib.ocm_gather_rows_f64 if dtype == np.float64 else lib.ocm_gather_rows_f32
    for name, idx in cases.items():
        idx = idx.astype(np.int64)
        rows = torch.from_numpy(idx).cuda()
        n = idx.size
        buf = torch.full((max(n, 1), p + pad_dst), 5.0, dtype=Xd.dtype, device="cuda")
        rc = fn(ctx, _lib.ptr(Xd), p + pad_src, _lib.ptr(rows), n, p, _lib.ptr(buf), p + pad_dst,
                _lib.stream_handle(Xd.device))
        assert rc == 0, name
        got = buf.cpu().numpy()
        assert np.array_equal(got[:n, :p].view(it), X[idx].view(it)), name
        assert (got[:, p:] == 5.0).all() and (got[n:] == 5.0).all(), name  # nothing else is written
        if pad_dst == 0:
            out = image.gather_rows(Xd, rows)
            assert out.shape == (n, p) and np.array_equal(out.cpu().numpy().view(it), X[idx].view(it)), name


# ------------------------------------------------------------------ 4. extract_objects
FIELDS = ("offsets", "pixel_index", "labels", "n_pixels", "bbox", "centroid")


def host_objects(cube, conn=8, min_pixels=1, mask=None):
    """The reference route on the host: NumPy's mask, SciPy's labels, objects_from_labels."""
    from ocm import image

    if mask is None:
        mask = ~(cube.mean(axis=2) < 1e-6)
    lab, _ = ndimage.label(mask, structure=STRUCTURE[conn])
    return image.objects_from_labels(lab, min_pixels=min_pixels)


def check_table(t, cube, ref):
    p = cube.shape[2]
    it = np.int32 if cube.dtype == np.float32 else np.int64
    get = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v
    assert np.array_equal(get(t.pixel_index), ref.order) and get(t.pixel_index).dtype == np.int64
    for name, want in zip(FIELDS, (ref.offsets, ref.order, ref.labels, ref.n_pixels, ref.bbox, ref.centroid)):
        got = get(getattr(t, name))
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    X = get(t.X)
    assert X.dtype == cube.dtype and X.shape == (ref.order.size, p)
    assert np.array_equal(X.view(it), cube.reshape(-1, p)[ref.order].view(it))
    assert t.shape == cube.shape[:2]


@functools.lru_cache(maxsize=None)
def scene_cube(H, W, p, dtype):
    from ocm import synth

    cube = synth.scene(H, W, p, blobs=9, seed=H + p, dtype=dtype)
    assert cube.shape == (H, W, p) and cube.dtype == dtype and cube.is_cuda
    return cube, cube.cpu().numpy()


@pytest.mark.parametrize("H,W,p", [(70, 90, 37), (40, 50, 256)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_extract_objects_equals_the_host_route(dtype, H, W, p):
    from ocm import image

    cube, host = scene_cube(H, W, p, dtype)
    ref = host_objects(host)
    G = ref.n_pixels.size
    assert G >= 2 and (host.reshape(-1, p)[ref.labels.ravel() == 0] == 0).all()
    t = image.extract_objects(cube)
    assert all(isinstance(getattr(t, f), torch.Tensor) and getattr(t, f).is_cuda for f in FIELDS + ("X",))
    check_table(t, host, ref)
    # two calls give the same bits
    t2 = image.extract_objects(cube)
    for f in FIELDS + ("X",):
        assert torch.equal(getattr(t, f), getattr(t2, f)), f
    # paint(pixel-wise labels) reproduces the label image; the NaN fill marks the background
    per_pixel = t.labels.view(-1)[t.pixel_index]
    assert torch.equal(t.paint(per_pixel, fill=0), t.labels)
    assert torch.equal(torch.isnan(t.paint(per_pixel)), t.labels == 0)
    # min_pixels above the smallest blob, connectivity 4, an explicit mask
    small = int(ref.n_pixels.min())
    dropped = host_objects(host, min_pixels=small + 1)
    assert dropped.n_pixels.size < G
    check_table(image.extract_objects(cube, min_pixels=small + 1), host, dropped)
    check_table(image.extract_objects(cube, connectivity=4), host, host_objects(host, conn=4))
    rng = np.random.default_rng(p)
    mask = rng.random((H, W)) < 0.45  # foreground that is zero in the cube, background that is not
    for m_in in (mask, torch.from_numpy(mask).cuda()):
        check_table(image.extract_objects(cube, mask=m_in, connectivity=4, min_pixels=3), host,
                    host_objects(host, conn=4, min_pixels=3, mask=mask))
    # NumPy in, NumPy out
    th = image.extract_objects(host)
    assert all(isinstance(getattr(th, f), np.ndarray) for f in FIELDS + ("X",))
    check_table(th, host, ref)


def test_extract_objects_on_a_band_slice_and_without_foreground():
    from ocm import image

    cube, host = scene_cube(40, 50, 256, torch.float32)
    wide = torch.full((40, 50, 259), float("nan"), device="cuda")
    wide[..., :256] = cube
    check_table(image.extract_objects(wide[..., :256]), host, host_objects(host))  # read in place, ldx = 259
    for dtype in (torch.float32, torch.float64):
        zeros = torch.zeros((13, 17, 5), dtype=dtype, device="cuda")
        t = image.extract_objects(zeros)
        assert t.X.shape == (0, 5) and t.X.dtype == dtype and t.offsets.tolist() == [0]
        assert t.pixel_index.shape == (0,) and t.n_pixels.shape == (0,) and not t.labels.any()
        assert t.centroid.shape == (0, 2) and t.bbox.shape == (0, 4) and t.shape == (13, 17)
        assert torch.isnan(t.paint_objects(torch.zeros(0))).all()
    everything = image.extract_objects(cube, min_pixels=10**6)  # every component dropped
    assert everything.X.shape == (0, 256) and not everything.labels.any()


# ------------------------------------------------------------------ 5. end to end
def test_scene_objects_through_predict_objects():
    """Discs of two spectral kinds (two sets of loadings of ocm.synth); a model of kind A fitted on
    the kind-A pixels accepts every kind-A object and rejects every kind-B object by pixel vote.
    float64 spectra, so that the fp64 oracle decides as the device model does on every pixel
    (asserted here), and the object decisions below are the oracle's too."""
    from ocm import image, synth
    from oracle import simca_oracle as O
    from utils import SIMCA

    H, W, p, k = 64, 96, 64, 20  # k: the generator's score gap; fewer components leave kind B inside Q's limit
    A = [(12, 12, 8), (12, 40, 7), (40, 14, 9), (44, 44, 6)]
    B = [(14, 76, 8), (46, 78, 9)]
    cube, kinds = synth.scene(H, W, p, [d + (0,) for d in A] + [d + (1,) for d in B], seed=5, dtype=torch.float64,
                              return_kinds=True)
    objs = image.extract_objects(cube)
    G = len(A) + len(B)
    assert objs.n_pixels.numel() == G and objs.X.dtype == torch.float64
    kind_of = kinds.view(-1)[objs.pixel_index[objs.offsets[:-1]]].cpu().numpy()  # by each object's first pixel
    assert sorted(kind_of.tolist()) == [0] * len(A) + [1] * len(B)
    pix_kind = kinds.view(-1)[objs.pixel_index].cpu().numpy()
    XA = objs.X[torch.from_numpy(pix_kind == 0).cuda()]
    est = SIMCA(n_components=k, model_class=0, verbose=False)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(XA, np.zeros(XA.shape[0], dtype=np.int64))
    res = est.predict_objects(objs.X, offsets=objs.offsets, rule="vote")
    pred = res.pred[:, 0].cpu().numpy()
    assert np.array_equal(pred, (kind_of == 0).astype(np.float64))
    # the fp64 oracle on every pixel, and the votes it implies
    Xh = objs.X.cpu().numpy()
    orc = O.OracleSIMCA(n_components=k, model_class=0).fit(XA.cpu().numpy(), np.zeros(XA.shape[0], dtype=np.int64))
    pix_ref = orc.predict(Xh)[:, 0]
    pix_dev = est.predict(objs.X)[:, 0].cpu().numpy()
    assert np.array_equal(pix_dev, pix_ref)
    off = objs.offsets.cpu().numpy()
    frac_ref = np.add.reduceat(pix_ref, off[:-1]) / np.diff(off)
    print("accepted share per object (oracle):", np.round(frac_ref, 3).tolist(), "kinds:", kind_of.tolist())
    assert np.array_equal(frac_ref >= 0.5, kind_of == 0)
    assert np.array_equal(res.fraction[:, 0].cpu().numpy(), frac_ref)
    # every decision lands on exactly its object's pixels
    painted = objs.paint_objects(res.pred[:, 0])
    lab = objs.labels.cpu().numpy()
    got = painted.cpu().numpy()
    assert np.array_equal(np.isnan(got), lab == 0)
    for g in range(G):
        assert (got[lab == g + 1] == pred[g]).all()
    assert np.array_equal(got == 1.0, np.isin(kinds.cpu().numpy(), [0]))
