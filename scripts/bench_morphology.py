#!/usr/bin/env python3
"""Time the mask-morphology kernel (ocm_edt_u8; ocm.image) on 2048 × 2048 masks
in ONE process, each input beside ocm_label_u8 on the same mask (the sibling
kernel and the yardstick) and beside SciPy on this host's CPU:

  discs_20 / discs_60   the disc scenes of scripts/bench_image.py at foreground
                        density 0.2 / 0.6
  corner                all foreground but one corner pixel, border "ignore":
                        the adversarial input of a pruned outward scan without
                        the segment minima (every column but one holds no
                        background at all)
  full_border           all foreground, border "background": the deepest object
                        the image can hold (R = 1024), every column with a
                        finite vertical distance, so no segment is skipped

per input:
  d2        one call, d2_out only              SciPy: distance_transform_edt
  erode     one call, mask_out only, radius 2  SciPy: binary_erosion(disk(2))
  opening   two calls (erode, dilate)          SciPy: binary_opening(disk(2))
  label     ocm_label_u8, connectivity 8

Every device variant is warmed up (and its result compared with SciPy's), then
timed `--reps` times with device events around `--inner` back-to-back runs of
it (one sample = their mean), the variants alternating inside each repeat;
median, min and max per variant.  SciPy is
wall-clock, `--host-reps` times.  Writes profiles/morphology_ab.json (or
--out) and prints the same JSON line.

    python scripts/bench_morphology.py [--H 2048] [--W 2048] [--reps 21] [--inner 10] [--host-reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=2048)
    ap.add_argument("--W", type=int, default=2048)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "morphology_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy import ndimage

    from bench_image import discs
    from ocm import _lib, image
    from ocm._lib import Context, check, ptr, stream_handle

    assert torch.cuda.is_available(), "bench_morphology.py needs a HIP device"
    dev = torch.device("cuda", 0)
    H, W = args.H, args.W
    HW = H * W
    lib, ctx = _lib.load(), Context.get(0).handle
    sh = lambda: stream_handle(dev)
    r2 = int(np.floor(args.radius ** 2))
    disc = image.disk(args.radius)
    corner = np.ones((H, W), dtype=bool)
    corner[0, 0] = False
    # (mask, border flag of the d2 / erode calls)
    inputs = {"discs_20": (discs(H, W, 0.2, 1)[1], image.EDT_BORDER_BG),
              "discs_60": (discs(H, W, 0.6, 2)[1], image.EDT_BORDER_BG),
              "corner": (corner, 0),
              "full_border": (np.ones((H, W), dtype=bool), image.EDT_BORDER_BG)}
    m8 = {k: torch.from_numpy(v[0]).to(dev).to(torch.uint8).view(-1) for k, v in inputs.items()}
    d2 = torch.empty(HW, dtype=torch.int32, device=dev)
    tmp = torch.empty(HW, dtype=torch.uint8, device=dev)
    out = torch.empty(HW, dtype=torch.uint8, device=dev)
    labels = torch.empty(HW, dtype=torch.int32, device=dev)
    ncomp = torch.empty(1, dtype=torch.int32, device=dev)
    dil = image.EDT_INVERT_IN | image.EDT_INVERT_OUT

    def edt(src, flags, d2_out, mask_out):
        check(lib.ocm_edt_u8(ctx, ptr(src), H, W, flags, r2, ptr(d2_out), ptr(mask_out), sh()), "ocm_edt_u8")

    def variants_of(name):
        src, border = m8[name], inputs[name][1]

        def v_d2():
            edt(src, border, d2, None)

        def v_erode():
            edt(src, border, None, out)

        def v_opening():
            edt(src, image.EDT_BORDER_BG, None, tmp)
            edt(tmp, dil, None, out)

        def v_label():
            check(lib.ocm_label_u8(ctx, ptr(src), H, W, 8, ptr(labels), ptr(ncomp), sh()), "label")

        return {"d2": v_d2, "erode": v_erode, "opening": v_opening, "label": v_label}

    def host_of(name):
        mask, border = inputs[name]
        bv = 0 if border else 1
        padded = (lambda m: np.pad(m, 1)) if border else (lambda m: m)
        crop = (lambda d: d[1:-1, 1:-1]) if border else (lambda d: d)
        return {"d2": lambda: crop(ndimage.distance_transform_edt(padded(mask))),
                "erode": lambda: ndimage.binary_erosion(mask, disc, border_value=bv),
                "opening": lambda: ndimage.binary_opening(mask, disc)}

    res = {"H": H, "W": W, "radius": args.radius, "reps": args.reps, "inner": args.inner, "host_reps": args.host_reps,
           "timing": "device events around `inner` runs of a variant (their mean), variants alternating; SciPy wall-clock on the host CPU",
           "density": {k: round(float(v[0].mean()), 4) for k, v in inputs.items()}, "inputs": {}}
    variants = {(name, v): fn for name in inputs for v, fn in variants_of(name).items()}
    host_ms = {}
    for (name, v), fn in variants.items():  # warm-up (code objects, workspace growth) and the check against SciPy
        fn()
        torch.cuda.synchronize()
        if v == "label":
            continue
        t = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = host_of(name)[v]()
            t.append((time.perf_counter() - t0) * 1e3)
        host_ms[(name, v)] = t
        if v == "d2":
            got = d2.view(H, W).cpu().numpy()
            assert np.array_equal(got, np.rint(want * want).astype(np.int64)), (name, v)
        else:
            assert np.array_equal(out.view(H, W).cpu().numpy() != 0, want), (name, v)
    times = {k: [] for k in variants}
    st = torch.cuda.current_stream()
    for _ in range(args.reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(args.inner):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.inner)
    summ = lambda t: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    for name in inputs:
        entry = {"ms": {v: summ(times[(name, v)]) for v in ("d2", "erode", "opening", "label")},
                 "scipy_ms": {v: summ(host_ms[(name, v)]) for v in ("d2", "erode", "opening")}}
        lab = entry["ms"]["label"]["median"]
        entry["over_label"] = {v: round(entry["ms"][v]["median"] / lab, 3) for v in ("d2", "erode", "opening")}
        entry["scipy_over_device"] = {v: round(entry["scipy_ms"][v]["median"] / entry["ms"][v]["median"], 1)
                                      for v in ("d2", "erode", "opening")}
        res["inputs"][name] = entry
    scene = max(res["inputs"][k]["ms"]["d2"]["median"] for k in ("discs_20", "discs_60"))
    res["d2_over_scene"] = {k: round(res["inputs"][k]["ms"]["d2"]["median"] / scene, 2)
                            for k in ("corner", "full_border")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
