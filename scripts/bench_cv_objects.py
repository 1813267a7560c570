#!/usr/bin/env python3
"""Time ocm_cv_objects (votes and decision sums) beside ocm_cv_counts
(accept_out NULL), the kernel that does the same per-row arithmetic, on the
same scores in ONE process:

  counts           ocm_cv_counts, confusion counts only (the yardstick)
  objects_200      ocm_cv_objects, objects of --length rows (default 200)
  objects_200_v    the same, votes only
  one_object       ocm_cv_objects, one object of all rows

Every variant is warmed up, then timed `--reps` times with device events, the
variants alternating inside each repeat; median, min and max per variant, and
the ratio of the medians to `counts`.  Not gated: nobody had measured either
kernel at this shape.  Writes profiles/cv_objects_ab.json (or --out) and prints
the same JSON line.

    python scripts/bench_cv_objects.py [--rows 1000000] [--k 10] [--ncfg 135] [--length 200] [--reps 9]"""
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ncfg", type=int, default=135)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cv_objects_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from ocm import engine

    assert torch.cuda.is_available(), "bench_cv_objects.py needs a HIP device"
    dev = torch.device("cuda", 0)
    m, k = args.rows, args.k
    g = torch.Generator(device=dev).manual_seed(1)
    T = torch.randn((m, k), generator=g, device=dev) * torch.linspace(3, 0.5, k, device=dev)
    Q = torch.rand(m, generator=g, device=dev) * 4
    inv = 1.0 / torch.linspace(9, 0.3, k, dtype=torch.float64, device=dev)
    pos = (torch.rand(m, generator=g, device=dev) < 0.7).to(torch.uint8)
    types = ("alt", "sim", "ci", "dd")
    cfgs = [(1 + c % k, types[c % 4], 1.0 / (2.0 * (1 + c % k)), 0.2, 1.0 + 0.01 * c) for c in range(args.ncfg)]

    def offsets(length):
        off = np.arange(0, m + length, length, dtype=np.int64)
        off[-1] = m
        return torch.from_numpy(np.unique(off)).to(dev)

    off_l, off_1 = offsets(args.length), offsets(m)
    variants = {
        "counts": lambda: engine.cv_counts(T, Q, inv, pos, m // 2, cfgs),
        f"objects_{args.length}": lambda: engine.cv_objects(T, Q, inv, off_l, cfgs, checked=True),
        f"objects_{args.length}_v": lambda: engine.cv_objects(T, Q, inv, off_l, cfgs, want_dsum=False, checked=True),
        "one_object": lambda: engine.cv_objects(T, Q, inv, off_1, cfgs, checked=True),
    }
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    res = {"rows": m, "k": k, "ncfg": args.ncfg, "length": args.length, "reps": args.reps, "ms": {}}
    for name, t in times.items():
        res["ms"][name] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    base = res["ms"]["counts"]["median"]
    res["ratio_to_counts"] = {name: v["median"] / base for name, v in res["ms"].items()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
