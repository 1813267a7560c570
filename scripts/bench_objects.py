#!/usr/bin/env python3
"""Time the segment-sum kernels (ocm_segsum_f32) on the bench workload
(1M×2048 fp32 in HBM) in ONE process, beside the project's established
one-read pass over the same matrix and beside what a user writes without them:

  rowstats        ocm_prep_rowstats_f32: the SNV's read-only pass (the yardstick)
  objects_500     2000 objects of 500 rows
  one_segment     one segment of all rows (a column sum)
  objects_64      15 625 objects of 64 rows (its 256 MB of output is part of its cost)
  torch_index_add torch.zeros(G, p, f64).index_add_(0, ids, X.double()) for the 2000 objects

Bar: objects_500 and one_segment each ≤ 1.25 × rowstats by medians (the margin
the scatter-correction kernels were given beside the same yardstick: it allows
for the fp64 accumulation and the second pass); the other two are recorded.

Every variant is warmed up, then timed `--reps` times with device events, the
variants alternating inside each repeat; median, min and max per variant.
Writes profiles/objects_ab.json (or --out) and prints the same JSON line.

    python scripts/bench_objects.py [--rows 1000000] [--p 2048] [--reps 9]"""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-torch", action="store_true", help="skip the index_add_ variant (it needs 2× the matrix)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "objects_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import synth_device
    from ocm import _lib
    from ocm._lib import Context, check, ptr, stream_handle
    from ocm.objects import check_offsets

    assert torch.cuda.is_available(), "bench_objects.py needs a HIP device"
    dev = torch.device("cuda", 0)
    n, p = args.rows, args.p
    X = synth_device(n, p, 20, 7, dev)
    lib, ctx = _lib.load(), Context.get(0).handle
    rs = torch.empty((n, 2), dtype=torch.float32, device=dev)

    def offsets(length):
        off = np.arange(0, n + length, length, dtype=np.int64)
        off[-1] = n
        return torch.from_numpy(check_offsets(off, n)).to(dev)

    layouts = {"objects_500": offsets(500), "one_segment": offsets(n), "objects_64": offsets(64)}
    outs = {name: torch.empty((off.numel() - 1, p), dtype=torch.float64, device=dev) for name, off in layouts.items()}

    def v_rowstats():
        check(lib.ocm_prep_rowstats_f32(ctx, ptr(X), p, n, p, ptr(rs), stream_handle(dev)), "rowstats")

    def v_segsum(name):
        off, out = layouts[name], outs[name]

        def run():
            check(lib.ocm_segsum_f32(ctx, ptr(X), p, n, p, ptr(off), off.numel() - 1, ptr(out), p,
                                     stream_handle(dev)), "segsum")
        return run

    G500 = layouts["objects_500"].numel() - 1
    ids = torch.repeat_interleave(torch.arange(G500, device=dev), torch.diff(layouts["objects_500"]))

    def v_torch():
        return torch.zeros((G500, p), dtype=torch.float64, device=dev).index_add_(0, ids, X.double())

    variants = {"rowstats": v_rowstats, **{name: v_segsum(name) for name in layouts}}
    if not args.no_torch:
        variants["torch_index_add"] = v_torch
    agree = {}
    for name, fn in variants.items():  # warm-up: code objects, workspace growth
        r = fn()
        if name == "torch_index_add":
            d = (outs["objects_500"] - r).abs().max() / r.abs().max()
            agree["objects_500_maxrel_vs_torch_f64"] = float(d)
        del r
    agree["one_segment_maxrel_vs_sum_of_objects_500"] = float(
        ((outs["one_segment"][0] - outs["objects_500"].sum(0)).abs() / outs["one_segment"][0].abs()).max())
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
    res = {"rows": n, "p": p, "reps": args.reps, "timing": "device events per call, variants alternating",
           "segments": {name: int(off.numel() - 1) for name, off in layouts.items()},
           "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for name, t in times.items()},
           "read_TBps": {name: round(n * p * 4 / med[name] / 1e9, 3) for name in ("rowstats", *layouts)},
           "over_rowstats": {name: round(med[name] / med["rowstats"], 3) for name in layouts},
           "bar": "objects_500 and one_segment <= 1.25 x rowstats (medians)",
           "bar_met": bool(med["objects_500"] <= 1.25 * med["rowstats"] and
                           med["one_segment"] <= 1.25 * med["rowstats"]),
           "agreement": agree}
    if "torch_index_add" in med:
        res["torch_index_add_over_objects_500"] = round(med["torch_index_add"] / med["objects_500"], 2)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
