#!/usr/bin/env python3
"""Time robust calibration (csrc/ocm_robust.hip, ocm.robust) in ONE process, beside
the project's established one-read fp64 column-sum pass over the same matrix:

  one_segment     ocm_segsum_f32 with a single segment of all rows (the yardstick)
  weiszfeld_step  one step of ocm_l1median_f32 (k_l1_part + k_l1_group + k_l1_update),
                  as (3 steps − 1 step)/2 of calls that cannot converge (tol = 0): a
                  call also carries the distance pass at the returned centre
  l1_call_1step   the whole call with max_iter = 1 (one step + the distance pass)
  sphere_rows     ocm_sphere_rows_f32 (one read, one write)
  l1_median       ocm.robust.l1_median to tol = 1e-9 from the column mean
  screen          ocm.robust.outlier_screen(X, k)
  mahalanobis     ocm.preprocess.mahalanobis_outlier_mask(X, k), the classical screen

No target is fixed: weiszfeld_step / one_segment says whether the step is the
one-read pass it claims to be.  A step reads X once where 16 rows fit in 128 KiB of
LDS (p ≤ 2048 float32) and twice, the second time out of L2, where they do not; a
`make exp EXP_FLAGS=-DOCM_L1_FORCE_TWICE` library (OCM_LIB=…, OCM_ALLOW_EXP_LIB=1)
times the read-twice form at a p where both exist.

Every variant is warmed up, then timed `--reps` times with device events (the host
side of a call is inside the interval), the variants alternating inside each
repeat; median, min and max per variant.  Writes profiles/robust_ab.json (or
--out) and prints the same JSON line.

    python scripts/bench_robust.py [--rows 1000000] [--p 2048] [--k 10] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=2048)
    ap.add_argument("--k", type=int, default=10, help="components of the two screens")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernels-only", action="store_true", help="skip l1_median, screen and mahalanobis")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import synth_device
    from ocm import _lib, engine, preprocess, robust

    assert torch.cuda.is_available(), "bench_robust.py needs a HIP device"
    dev = torch.device("cuda", 0)
    n, p, k = args.rows, args.p, args.k
    X = synth_device(n, p, 20, 7, dev)
    off = torch.from_numpy(np.array([0, n], dtype=np.int64)).to(dev)
    start = engine.colmean(X, None, n)

    def v_step(iters):
        return lambda: engine.l1_median(X, None, start, 0.0, iters, want_dist=False)

    variants = {"one_segment": lambda: engine.segment_sums(X, off, checked=True),
                "l1_call_1step": v_step(1), "l1_call_3steps": v_step(3),
                "sphere_rows": lambda: engine.sphere_rows(X, None, start)}
    info = {}
    if not args.kernels_only:
        def v_median():
            r = robust.l1_median(X)
            info["l1_median_iters"] = r.n_iter
            return r

        def v_screen():
            s = robust.outlier_screen(X, k)
            info["screen_kept"] = int(s.keep.sum().item())
            info["screen_median_iters"] = s.pca.median.n_iter
            return s

        def v_maha():
            keep, _ = preprocess.mahalanobis_outlier_mask(X, k)
            info["mahalanobis_kept"] = int(keep.sum().item())
            return keep

        variants.update({"l1_median": v_median, "screen": v_screen, "mahalanobis": v_maha})
    for fn in variants.values():  # warm-up: code objects, workspace growth
        r = fn()
        del r
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
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
    med = {name: statistics.median(t) for name, t in times.items()}
    step = (med["l1_call_3steps"] - med["l1_call_1step"]) / 2.0
    res = {"rows": n, "p": p, "k": k, "reps": args.reps, "lib": os.path.basename(_lib.LIB_PATH),
           "timing": "device events per call, variants alternating",
           "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for name, t in times.items()},
           "weiszfeld_step_ms": round(step, 4),
           "weiszfeld_step_over_one_segment": round(step / med["one_segment"], 3),
           "read_TBps": {"one_segment": round(n * p * 4 / med["one_segment"] / 1e9, 3),
                         "weiszfeld_step": round(n * p * 4 / step / 1e9, 3)},
           "info": info}
    if "screen" in med:
        res["screen_over_mahalanobis"] = round(med["screen"] / med["mahalanobis"], 2)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
