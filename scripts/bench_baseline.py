#!/usr/bin/env python3
"""Time the baseline kernels on the bench workload (1M×2048 fp32 in HBM) in
ONE process, beside the machine's streaming yardstick of the same shape:

  snv_sg5        ocm_snv_savgol_f32, SNV + SG(5, 2, 1): one read, one write
  whittaker      ocm_whittaker_f32, w = 1, d = 2, λ = --lam (shared factor)
  whittaker_rows ocm_whittaker_f32 with (m, p) weights uniform in [0.01, 1]
  asls           ocm_asls_f32, d = 2, λ = --lam, asym = --asym, 10 iterations

Each kernel's bytes are counted from what it moves per element (DESIGN.md,
baseline correction): matrix reads and writes plus the workgroup slabs; for
asls from the solves each 64-row block really ran (ocm_asls_f32's iters).
Prints ms and achieved bytes/s per variant, and the single-thread
scipy.linalg.solveh_banded time per row measured on this host (ten solves),
extrapolated to --rows rows: that figure is extrapolated, not measured.

Every variant is warmed up, then timed `--reps` times with device events, the
variants alternating inside each repeat; median, min and max per variant.
Writes profiles/baseline_bench.json (or --out) and prints the same JSON line.

    python scripts/bench_baseline.py [--rows 1000000] [--p 2048] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=2048)
    ap.add_argument("--lam", type=float, default=1e5)
    ap.add_argument("--asym", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-rows", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "baseline_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy.linalg import solveh_banded

    from bench import synth_device
    from ocm import preprocess

    assert torch.cuda.is_available(), "bench_baseline.py needs a HIP device"
    dev = torch.device("cuda", 0)
    n, p, lam, asym, d, n_iter = args.rows, args.p, args.lam, args.asym, 2, 10
    X = synth_device(n, p, 20, 7, dev)
    out = torch.empty((n, p), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    W = torch.empty((n, p), dtype=torch.float32, device=dev).uniform_(0.01, 1.0, generator=gen)

    def v_snv():
        preprocess.snv_savgol(X, 5, 2, 1, out=out)

    def v_whittaker():
        preprocess.whittaker(X, lam, d, out=out)

    def v_rows():
        preprocess.whittaker(X, lam, d, weights=W, out=out)

    def v_asls():
        preprocess.asls(X, lam, asym, n_iter, d, out=out)

    variants = {"snv_sg5": v_snv, "whittaker": v_whittaker, "whittaker_rows": v_rows, "asls": v_asls}
    for fn in variants.values():  # warm-up: code objects, workspace growth
        fn()
    torch.cuda.synchronize()
    # the solves each 64-row block ran: all rows finished after K solves → one more that writes, at most n_iter
    _, iters = preprocess.asls(X, lam, asym, n_iter, d, out=out, return_iters=True)
    pad = (-n) % 64
    blk = torch.cat([iters, iters.new_zeros(pad)]).view(-1, 64).max(dim=1).values
    solves = torch.clamp(blk + 1, max=n_iter).double()
    mean_solves = float(solves.mean())
    it_host = iters.cpu().numpy()
    slab = 8 * (d + 1)  # bytes per element of u, l1, l2
    per_elem = {"snv_sg5": 8.0,
                "whittaker": 4 + 4 + 2 * 8,  # x, out, u stored and loaded
                "whittaker_rows": 4 + 4 + 4 + 2 * slab,  # x, w, out, (u, l1, l2) stored and loaded
                # first solve under the shared factor: x twice, u twice; later solves: x twice, the slab twice,
                # the weight bits (one word per 32 columns, read forward, read and written backward); one write
                "asls": (8 + 16) + (mean_solves - 1) * (8 + 2 * slab + 12 / 32) + 4}
    times = {name: [] for name in variants}
    st = torch.cuda.current_stream()
    for _ in range(args.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {name: statistics.median(t) for name, t in times.items()}

    # the CPU's way: ten banded Cholesky solves per row, one thread, fp64
    xs = X[:args.cpu_rows].double().cpu().numpy()
    ab0 = lam * preprocess.whittaker_bands(p, d)
    t0 = time.perf_counter()
    for x in xs:
        w = np.ones(p)
        for _ in range(n_iter):
            ab = ab0.copy()
            ab[0] += w
            z = solveh_banded(ab, w * x, lower=True)
            w = np.where(x > z, asym, 1.0 - asym)
    cpu_row_us = (time.perf_counter() - t0) / len(xs) * 1e6

    res = {"rows": n, "p": p, "lam": lam, "asym": asym, "d": d, "n_iter": n_iter, "reps": args.reps,
           "timing": "device events per call, variants alternating",
           "ms": {name: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
                  for name, t in times.items()},
           "bytes_per_element": {name: round(b, 3) for name, b in per_elem.items()},
           "TBps": {name: round(n * p * per_elem[name] / med[name] / 1e9, 3) for name in variants},
           "asls_iters": {"min": int(it_host.min()), "mean": round(float(it_host.mean()), 3), "max": int(it_host.max())},
           "asls_mean_solves_per_block": round(mean_solves, 3),
           "asls_over_whittaker_byte_rate": round((per_elem["asls"] / med["asls"]) /
                                                  (per_elem["whittaker"] / med["whittaker"]), 3),
           "cpu_solveh_banded_us_per_row_10_solves": round(cpu_row_us, 1),
           "cpu_one_thread_s_extrapolated_to_rows": round(cpu_row_us * n / 1e6, 1)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
