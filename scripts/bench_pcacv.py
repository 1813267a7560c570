#!/usr/bin/env python3
"""Time the PCA cross-validation (csrc/ocm_press.hip, ocm.pcacv) in ONE process,
beside the project's one-read scorer over the same rows:

  press_passes   (a) ocm_press_f32 over every fold's held-out rows against its model
                 (the fold models are fitted once, outside the interval)
  score_passes   (b) engine.score (ocm_score_f32_diag: T² and Q at K components) over
                 the same rows and models: the one-read yardstick
  torch_passes   (c) the same steps composed in torch: Y = X[rows] − μ, T = Y·Pᵀ, then a
                 loop over k of R ← R − t_k·P_k, Σ w_k·R² and Σ R² (float32, fp64 sums)
  pca_press      (d) the whole call: one Gram pass for all folds, an eigensolve per
                 fold, the PRESS passes

The only gate is (a) faster than (c); (a)/(b) says how far the PRESS pass is from a
one-read pass (it does about four lane operations per element and component on top).

Every variant is warmed up, then timed with device events (the host side of a call
is inside the interval), the variants alternating inside each repeat; median, min
and max per variant.  Writes profiles/pcacv_ab.json (or --out) and prints the same
JSON line.

    python scripts/bench_pcacv.py [--rows 1000000] [--p 2048] [--k 20] [--folds 10] [--reps 5]"""
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
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-whole", type=int, default=2, help="repeats of the whole pca_press")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pcacv_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import synth_device
    from ocm import _lib, cv, engine, pcacv

    assert torch.cuda.is_available(), "bench_pcacv.py needs a HIP device"
    dev = torch.device("cuda", 0)
    n, p, K, F = args.rows, args.p, args.k, args.folds
    X = synth_device(n, p, 20, 7, dev)
    folds = pcacv.make_folds(X, F)
    fm = cv.fold_models(X, folds, folds, n, K, 0)
    rows = [torch.from_numpy(f).to(dev) for f in folds]
    P32 = [e.to(torch.float32) for e in fm.evecs]
    mu32 = [m.to(torch.float32) for m in fm.mean]
    W32 = []
    for e in fm.evecs:
        h = torch.cat([torch.zeros((1, p), dtype=torch.float64, device=dev), torch.cumsum(e * e, dim=0)])
        d = 1.0 - h
        W32.append(torch.where(d > pcacv.DEGENERATE, 1.0 / (d * d), torch.zeros_like(d)).to(torch.float32))
    torch.cuda.synchronize()

    def v_press():
        return [engine.press(X, rows[f], int(folds[f].size), fm.evecs[f], fm.mean[f]) for f in range(F)]

    def v_score():
        return [engine.score(X, rows[f], int(folds[f].size), fm.evecs[f], fm.mean[f], fm.inv[f], want_T2=True,
                             want_Q=True) for f in range(F)]

    def v_torch():
        out = []
        for f in range(F):
            R = X.index_select(0, rows[f]) - mu32[f]
            T = R @ P32[f].T
            press = torch.empty(K + 1, dtype=torch.float64, device=dev)
            naive = torch.empty(K + 1, dtype=torch.float64, device=dev)
            for k in range(K + 1):
                if k:
                    R.addr_(T[:, k - 1], P32[f][k - 1], alpha=-1.0)
                R2 = R * R
                naive[k] = R2.sum(dtype=torch.float64)
                press[k] = (R2 * W32[f][k]).sum(dtype=torch.float64)
            out.append((press, naive))
        return out

    def v_whole():
        return pcacv.pca_press(X, K, folds=folds)

    variants = {"press_passes": v_press, "score_passes": v_score, "torch_passes": v_torch}
    got = {}
    for name, fn in list(variants.items()) + [("pca_press", v_whole)]:  # warm-up: code objects, workspace growth
        got[name] = fn()
    torch.cuda.synchronize()
    a = torch.stack([o[0] for o in got["press_passes"]]).sum(dim=0).cpu().numpy()
    c = torch.stack([o[0] for o in got["torch_passes"]]).sum(dim=0).cpu().numpy()
    agree = float(np.max(np.abs(a - c) / np.abs(a)))
    whole = got["pca_press"]
    del got
    torch.cuda.empty_cache()
    times = {name: [] for name in list(variants) + ["pca_press"]}
    st = torch.cuda.current_stream()

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        r = fn()
        e1.record(st)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
        del r

    for i in range(args.reps):
        for name, fn in variants.items():
            timed(name, fn)
        if i < args.reps_whole:
            timed("pca_press", v_whole)
    med = {name: statistics.median(t) for name, t in times.items()}
    res = {"rows": n, "p": p, "k": K, "folds": F, "reps": args.reps, "reps_whole": args.reps_whole,
           "lib": os.path.basename(_lib.LIB_PATH), "timing": "device events per call, variants alternating",
           "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for name, t in times.items()},
           "press_over_score": round(med["press_passes"] / med["score_passes"], 3),
           "torch_over_press": round(med["torch_passes"] / med["press_passes"], 2),
           "press_beats_torch": bool(med["press_passes"] < med["torch_passes"]),
           "press_read_TBps": round(n * p * 4 / med["press_passes"] / 1e9, 3),
           "press_vs_torch_max_rel_diff": agree,
           "selected": {"min": int(np.argmin(whole.press)), "naive_argmin": int(np.argmin(whole.naive))}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
