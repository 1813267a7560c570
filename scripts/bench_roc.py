#!/usr/bin/env python3
"""Time the exact AUC (ocm_auc) in ONE process against the only device route
there was before it, torch.sort + torch.searchsorted on the same tensors, on
decision-value-like float64 scores: an (m, C) matrix as SIMCA.decision_function
returns it, 30 % positives, for C = 1 and C = 20 columns.

  ocm      ocm.roc._call_auc: ocm_auc on the matrix in place, u2 / P / N / NaN
           counts read back
  torch    gather the smaller class, torch.sort it along the rows, transpose,
           two torch.searchsorted of the other class, integer sums, read back

Both end in a host read of the C integers.  Every variant is warmed up, then
timed `--reps` times with a host clock around the call and a device
synchronise, the variants alternating inside each repeat; median, min and max
per variant, the ratio torch / ocm of the medians, and the radix passes ocm_auc
executed (of 8).  The two routes must give the same integers, or the script fails
and writes nothing.  Writes
profiles/roc_bench.json (or --out) and prints the same JSON line.

    python scripts/bench_roc.py [--rows 1000000] [--reps 15] [--cols 1,20]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)


def scores(m, C, pos, dev):
    """D_limit − dred for an 'alt' decision: dred = √(t² + q²) of two scaled χ²-like
    distances, the negatives about twice as far out; column c has its own limit."""
    import torch

    g = torch.Generator(device=dev).manual_seed(20 + C)
    t = torch.empty((m, C), dtype=torch.float64, device=dev).normal_(generator=g).square_()
    q = torch.empty((m, C), dtype=torch.float64, device=dev).normal_(generator=g).square_()
    far = 1.0 + (~pos).to(torch.float64)[:, None]
    dlim = torch.linspace(1.2, 2.4, C, dtype=torch.float64, device=dev)
    return dlim - torch.sqrt(t * t + q * q) * far


def torch_u2(S, pos):
    """u2 of every column by torch.sort + torch.searchsorted, sorting the smaller class."""
    import torch

    P = int(pos.sum())
    N = pos.numel() - P
    small_is_pos = P <= N
    small = S[pos if small_is_pos else ~pos]
    other = S[~pos if small_is_pos else pos]
    srt = torch.sort(small, dim=0).values.t().contiguous()
    oth = other.t().contiguous()
    lt = torch.searchsorted(srt, oth, right=False)
    le = torch.searchsorted(srt, oth, right=True)
    u2 = (2 * (P - le) + (le - lt)).sum(1) if small_is_pos else (2 * lt + (le - lt)).sum(1)
    return u2.cpu().numpy(), P, N


def bench_cols(m, C, reps, dev):
    import numpy as np
    import torch

    from ocm import roc

    g = torch.Generator(device=dev).manual_seed(7)
    pos = torch.rand(m, device=dev, generator=g) < 0.3
    S = scores(m, C, pos, dev)
    pos8 = pos.to(torch.uint8)
    mm, ncol, cs, rs = roc._layout(S.shape, S.stride(), 0)

    def v_ocm():
        return roc._call_auc(S, mm, ncol, cs, rs, pos8)

    def v_torch():
        return torch_u2(S, pos)

    variants = {"ocm": v_ocm, "torch": v_torch}
    warm = {name: fn() for name, fn in variants.items()}  # code objects, workspace growth, the allocator's blocks
    warm = {name: fn() for name, fn in variants.items()}
    torch.cuda.synchronize()
    passes = roc.last_passes()
    same = bool(np.array_equal(warm["ocm"][0], warm["torch"][0])) and warm["ocm"][1:3] == warm["torch"][1:3]
    if not same:
        raise SystemExit(f"bench_roc: ocm_auc and the torch route disagree at {C} columns: "
                         f"{warm['ocm'][0][:4]} vs {warm['torch'][0][:4]}; no timing written")
    P, N = warm["ocm"][1], warm["ocm"][2]
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: statistics.median(t) for name, t in times.items()}
    return {"rows": m, "cols": C, "P": P, "N": N, "auc_first": int(warm["ocm"][0][0]) / (2 * P * N),
            "same_integers": same, "passes_executed": passes, "passes_of": 8,
            "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                   for name, t in times.items()},
            "torch_over_ocm": round(med["torch"] / med["ocm"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cols", default="1,20")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "roc_bench.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_roc.py needs a HIP device"
    dev = torch.device("cuda", 0)
    res = {"reps": args.reps, "dtype": "float64", "positives": 0.3,
           "timing": "host clock around the call and a device synchronise, variants alternating",
           "cases": [bench_cols(args.rows, int(c), args.reps, dev) for c in args.cols.split(",")]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
