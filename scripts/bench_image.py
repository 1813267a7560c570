#!/usr/bin/env python3
"""Time the image-to-objects kernels (ocm_fgmask_f32, ocm_label_u8,
ocm_gather_rows_f32; ocm.image) on a 2048 × 512 scene (1M pixels) at p = 2048
and p = 256 in ONE process, each beside the established pass it is measured
against:

  rowstats   ocm_prep_rowstats_f32 over the cube      the yardstick of fgmask
  fgmask     ocm_fgmask_f32 over the cube             bar: no slower than rowstats beyond the spread
  snv        ocm_snv_savgol_f32, SNV only, on n_fg rows: one read, one write
  gather     ocm_gather_rows_f32 of all n_fg foreground rows   bar: ≤ 1.25 × snv
  label_20 / label_60   ocm_label_u8 on disc masks of foreground density 0.2 / 0.6
                        bar: each ≤ the p = 256 fgmask of the same image
  extract    ocm.image.extract_objects end to end (device tensors in and out)
  host       the route without it: cube to the host, NumPy mask, ndimage.label,
             stable argsort, fancy index, spectra back to the device (--host-reps)

Every device variant is warmed up, then timed `--reps` times with device events
around one call, the variants alternating inside each repeat; median, min and
max per variant.  The host route is wall-clock between device synchronisations.
Writes profiles/image_ab.json (or --out) and prints the same JSON line.

    python scripts/bench_image.py [--H 2048] [--W 512] [--p 2048,256] [--reps 9]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)


def discs(H, W, density, seed):
    """Random discs (radius 6..20) until they cover `density` of the image; the list and the mask."""
    import numpy as np

    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    mask = np.zeros((H, W), dtype=bool)
    out = []
    while mask.mean() < density:
        for _ in range(50):
            r, c, rad = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(6, 21))
            out.append((r, c, rad))
            y0, y1, x0, x1 = max(r - rad, 0), min(r + rad + 1, H), max(c - rad, 0), min(c + rad + 1, W)
            mask[y0:y1, x0:x1] |= (yy[y0:y1, x0:x1] - r) ** 2 + (xx[y0:y1, x0:x1] - c) ** 2 <= rad * rad
    return out, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2048)
    ap.add_argument("--W", type=int, default=512)
    ap.add_argument("--p", default="2048,256")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "image_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy import ndimage

    from ocm import _lib, image, synth
    from ocm._lib import Context, check, ptr, stream_handle

    assert torch.cuda.is_available(), "bench_image.py needs a HIP device"
    dev = torch.device("cuda", 0)
    H, W = args.H, args.W
    HW = H * W
    lib, ctx = _lib.load(), Context.get(0).handle
    sh = lambda: stream_handle(dev)
    blobs20, mask20 = discs(H, W, 0.2, 1)
    _, mask60 = discs(H, W, 0.6, 2)
    m8 = {"label_20": torch.from_numpy(mask20).to(dev).to(torch.uint8).view(-1),
          "label_60": torch.from_numpy(mask60).to(dev).to(torch.uint8).view(-1)}
    labels = torch.empty(HW, dtype=torch.int32, device=dev)
    ncomp = torch.empty(1, dtype=torch.int32, device=dev)
    res = {"H": H, "W": W, "reps": args.reps, "host_reps": args.host_reps,
           "timing": "device events per call, variants alternating; host route wall-clock",
           "density": {"label_20": round(float(mask20.mean()), 4), "label_60": round(float(mask60.mean()), 4)},
           "components": {}, "p": {}}

    def v_label(name):
        def run():
            check(lib.ocm_label_u8(ctx, ptr(m8[name]), H, W, 8, ptr(labels), ptr(ncomp), sh()), "label")
        return run

    for p in (int(v) for v in args.p.split(",")):
        cube = synth.scene(H, W, p, blobs20, seed=3)
        X = cube.view(HW, p)
        n_fg = int(mask20.sum())
        rs = torch.empty((HW, 2), dtype=torch.float32, device=dev)
        mk = torch.empty(HW, dtype=torch.uint8, device=dev)
        rows = torch.from_numpy(np.flatnonzero(mask20)).to(dev)
        dst = torch.empty((n_fg, p), dtype=torch.float32, device=dev)

        def v_rowstats():
            check(lib.ocm_prep_rowstats_f32(ctx, ptr(X), p, HW, p, ptr(rs), sh()), "rowstats")

        def v_fgmask():
            check(lib.ocm_fgmask_f32(ctx, ptr(X), p, HW, p, 1e-6, ptr(mk), None, sh()), "fgmask")

        def v_snv():
            check(lib.ocm_snv_savgol_f32(ctx, ptr(X), p, n_fg, p, 1, 0, None, ptr(dst), p, sh()), "snv")

        def v_gather():
            check(lib.ocm_gather_rows_f32(ctx, ptr(X), p, ptr(rows), n_fg, p, ptr(dst), p, sh()), "gather")

        def v_extract():
            return image.extract_objects(cube)

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = cube.cpu().numpy()
            lab, n = ndimage.label(~(c.mean(axis=2) < 1e-6), structure=np.ones((3, 3)))
            flat = lab.ravel()
            idx = np.flatnonzero(flat)
            order = idx[np.argsort(flat[idx], kind="stable")]
            Xo = torch.from_numpy(c.reshape(HW, p)[order]).to(dev)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, Xo, n

        variants = {"rowstats": v_rowstats, "fgmask": v_fgmask, "snv": v_snv, "gather": v_gather,
                    "label_20": v_label("label_20"), "label_60": v_label("label_60"), "extract": v_extract}
        for name, fn in variants.items():  # warm-up: code objects, workspace growth, allocator
            r = fn()
            if name.startswith("label"):
                res["components"][name] = int(ncomp.item())
            if name == "fgmask":
                assert torch.equal(mk, m8["label_20"]), "fgmask differs from the scene's discs"
            if name == "extract":
                objs = r
            del r
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        st = torch.cuda.current_stream()
        for _ in range(args.reps):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                r = fn()
                e1.record(st)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
                del r
        host = []
        for _ in range(args.host_reps):
            ms, Xo, n = host_route()
            host.append(ms)
        assert n == objs.n_pixels.numel() and torch.equal(Xo, objs.X), "extract_objects differs from the host route"
        if host:
            times["host"] = host
        med = {name: statistics.median(t) for name, t in times.items()}
        out = {"n_fg": n_fg, "objects": int(objs.n_pixels.numel()),
               "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4),
                             "max": round(max(t), 4)} for name, t in times.items()},
               "read_TBps": {name: round(HW * p * 4 / med[name] / 1e9, 3) for name in ("rowstats", "fgmask")},
               "moved_TBps": {name: round(2 * n_fg * p * 4 / med[name] / 1e9, 3) for name in ("snv", "gather")},
               "fgmask_over_rowstats": round(med["fgmask"] / med["rowstats"], 3),
               "gather_over_snv": round(med["gather"] / med["snv"], 3)}
        if host:
            out["host_over_extract"] = round(med["host"] / med["extract"], 2)
        res["p"][str(p)] = out
        del cube, X, rs, mk, rows, dst, objs, Xo
        torch.cuda.empty_cache()
    narrow = res["p"].get("256")
    if narrow:
        for name in ("label_20", "label_60"):
            res[name + "_over_fgmask_p256"] = round(narrow["ms"][name]["median"] / narrow["ms"]["fgmask"]["median"], 3)
    res["bars"] = {"fgmask": "<= rowstats beyond the run-to-run spread", "gather": "<= 1.25 x snv (medians)",
                   "label": "<= the p = 256 fgmask of the same image (medians)"}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
