#!/usr/bin/env python3
"""Time PLS-DA (ocm/plsda.py) on the bench workload (1M×2048 fp32 in HBM, 3
classes, A = 25) in ONE process:

  fit             PLSDA(25).fit(X, y): Gram over the class segments, moments, ocm_pls_fit_f64, LDA tables
  predict_sweep   the full-data sweep over 1..25 components with confusion counts (the whole call)
  predict_kernel  ocm_plsda_predict_f32 alone, outputs allocated beforehand (pred + counts for 25 prefixes)
  composed        the route without it: engine.score(..., want_T=True) at k = 25 (ocm_score_f32_diag, which
                  reads X twice at k > 20) plus torch for the 25 LDAs and their argmax
  cv_curve        plsda_cv_curve(X, y, 1..25, 5 folds): one Gram, one ocm_pls_fit_f64 of 6 problems, 6 sweeps

predict_kernel and composed alternate inside each repeat and are timed with
device events; the other three are host wall-clock around calls that end in a
synchronise.  Medians, min and max.  ``floor_fraction`` is the time of one read
of X at the HBM peak (8 TB/s: 8.19 GB → 1.024 ms) over the kernel's time.
Writes profiles/plsda_bench.json (or --out) and prints the same JSON line.

    python scripts/bench_plsda.py [--rows 1000000] [--p 2048] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--components", type=int, default=25)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slow-reps", type=int, default=3, help="repeats of fit, predict_sweep and cv_curve")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plsda_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import synth_device
    from ocm import engine
    from ocm.plsda import PLSDA, plsda_cv_curve

    assert torch.cuda.is_available(), "bench_plsda.py needs a HIP device"
    dev = torch.device("cuda", 0)
    n, p, C, A = args.rows, args.p, args.classes, args.components
    X = synth_device(n, p, 20, 7, dev)
    y = np.random.default_rng(11).integers(0, C, size=n)
    wl = torch.linspace(0.0, 1.0, p, device=dev)
    bands = torch.stack([torch.exp(-0.5 * ((wl - c) / 0.05) ** 2) for c in np.linspace(0.2, 0.8, C)])
    bands = (bands / bands.norm(dim=1, keepdim=True)).float()
    yd = torch.from_numpy(y).to(dev)
    for s in range(0, n, 100_000):  # class c's rows carry its band
        X[s:s + 100_000] += bands[yd[s:s + 100_000]]
    lvs = list(range(1, A + 1))
    yt = yd.to(torch.uint8)

    def wall(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
            del r
        return out

    est = PLSDA(A).fit(X, y)  # warm-up: code objects, workspace growth
    mdl = est._model
    table, lv_eff = mdl.table(lvs)
    outs = {"pred": torch.empty((n, A), dtype=torch.uint8, device=dev),
            "counts": torch.empty((A, C, C), dtype=torch.int64, device=dev)}
    coef = table[:A * C * A].view(A, C, A)
    icpt = table[A * C * A:].view(A, C)
    ones = torch.ones(A, dtype=torch.float64, device=dev)

    def v_kernel():
        return engine.plsda_predict(X, None, n, mdl.proj, mdl.mean, lv_eff, C, table, y_true=yt, outs=outs)

    def v_composed():
        T = engine.score(X, None, n, mdl.proj, mdl.mean, ones, want_T=True, want_T2=False, want_Q=False)["T"]
        pred = torch.empty((n, A), dtype=torch.uint8, device=dev)
        cnt = torch.empty((A, C, C), dtype=torch.int64, device=dev)
        for l, a in enumerate(lv_eff):
            D = T[:, :a].double() @ coef[l, :, :a].T + icpt[l]
            pr = D.argmax(1)
            pred[:, l] = pr
            cnt[l] = torch.bincount(yd * C + pr, minlength=C * C).view(C, C)
        return pred, cnt

    variants = {"predict_kernel": v_kernel, "composed": v_composed}
    v_kernel()
    pc, cc = v_composed()
    torch.cuda.synchronize()
    agree = {"pred_equal_fraction": float((pc == outs["pred"]).float().mean()),
             "counts_abs_diff": int((cc - outs["counts"]).abs().sum())}
    del pc, cc
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
    times["fit"] = wall(lambda: PLSDA(A).fit(X, y), args.slow_reps)
    times["predict_sweep"] = wall(lambda: est.predict_sweep(X, lvs, y_true=yt), args.slow_reps)
    plsda_cv_curve(X, y, lvs)  # warm-up: the six-problem fit's workspace
    curve = {}

    def v_cv():
        curve.update(plsda_cv_curve(X, y, lvs))

    times["cv_curve"] = wall(v_cv, args.slow_reps)
    med = {name: statistics.median(t) for name, t in times.items()}
    floor_ms = n * p * 4 / HBM_PEAK * 1e3
    res = {"rows": n, "p": p, "classes": C, "components": A, "reps": args.reps, "slow_reps": args.slow_reps,
           "timing": "predict_kernel / composed: device events, alternating; fit / predict_sweep / cv_curve: "
                     "host clock around calls ending in a synchronise",
           "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for name, t in times.items()},
           "hbm_floor_ms": round(floor_ms, 4),
           "floor_fraction": {"predict_kernel": round(floor_ms / med["predict_kernel"], 3)},
           "composed_over_predict_kernel": round(med["composed"] / med["predict_kernel"], 2),
           "n_components_completed": int(est.n_components_),
           "f1_cal": [round(float(v), 4) for v in curve["f1_cal"]],
           "f1_cv": [round(float(v), 4) for v in curve["f1_cv"]],
           "agreement": agree}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
