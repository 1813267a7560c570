#!/usr/bin/env python3
"""Time the scatter-correction kernels on the bench workload (1M×2048 fp32 in
HBM) in ONE process, against the existing passes of the same shape and
against what a user would write without them:

  rowstats      ocm_prep_rowstats_f32: the SNV's one read-only pass
  rowfit_q2/4/8 ocm_rowfit_f32 (coefficients + row statistics), q = 2, 4, 8
  snv           ocm_snv_savgol_f32 without a filter: one read, one write
  emsc_q2/4     ocm_emsc_apply_f32, q = 2 (MSC) and q = 4
  torch_fit_q2  C = X @ W32.T                                (float32 torch)
  torch_q2/4    C = X @ W32.T; (X − C[:, :1] − C[:, 2:] @ B32[2:]) / C[:, 1:2]

and fit + predict (k = 20, alt / Fdist / jm: the nuts setting) on a lazy
MSC + SG(5, 2, 1) view against the lazy SNV + SG(5, 2, 1) view; they should
differ by the row-statistics kernel alone.  The views read rows MSC is meant
for: the bench rows' deviations from their mean spectrum shrunk to 5 % (as
they stand, the deviations dwarf the mean's own shape, the fitted scale c1
of many rows is near 0 and the corrected rows explode), each row then
scaled by b ∈ [0.5, 2] and offset by a ∈ [−2, 2].

Every variant is warmed up, then timed `--reps` times with device events, the
variants alternating inside each repeat; median, min and max per variant.
Writes profiles/scatter_ab.json (or --out) and prints the same JSON line.

    python scripts/bench_scatter.py [--rows 1000000] [--p 2048] [--reps 7]"""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scatter_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import synth_device
    from ocm import _lib, preprocess
    from ocm._lib import Context, check, ptr, stream_handle
    from utils import SIMCA

    assert torch.cuda.is_available(), "bench_scatter.py needs a HIP device"
    dev = torch.device("cuda", 0)
    n, p, k = args.rows, args.p, args.k
    X = synth_device(n, p, 20, 7, dev)
    lib, ctx = _lib.load(), Context.get(0).handle
    ref = X[:65536].double().mean(0).cpu().numpy()
    inter = np.stack([np.cos(3.0 * np.linspace(0.0, 1.0, p)), np.sin(5.0 * np.linspace(0.0, 1.0, p)),
                      np.exp(-0.5 * ((np.linspace(0.0, 1.0, p) - 0.3) / 0.05) ** 2)])
    est = {2: preprocess.MSC(reference=ref), 4: preprocess.EMSC(degree=2, reference=ref),
           8: preprocess.EMSC(degree=3, reference=ref, interferents=inter)}
    W = {q: torch.from_numpy(e.weights_).to(dev) for q, e in est.items()}
    B = {q: torch.from_numpy(e.basis_).to(dev) for q, e in est.items()}
    W32 = {q: W[q].float() for q in W}
    B32 = {q: B[q].float() for q in B}
    out = torch.empty((n, p), dtype=torch.float32, device=dev)
    coef = torch.empty((n, 8), dtype=torch.float32, device=dev)
    rs = torch.empty((n, 2), dtype=torch.float32, device=dev)
    y = torch.zeros(n, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    ref_t = torch.from_numpy(ref).to(dev).float()
    Xv = torch.empty_like(X)
    for lo in range(0, n, 65536):  # in blocks: no second full-size temporary
        hi = min(n, lo + 65536)
        b = 0.5 + 1.5 * torch.rand((hi - lo, 1), device=dev, generator=gen)
        a = -2.0 + 4.0 * torch.rand((hi - lo, 1), device=dev, generator=gen)
        Xv[lo:hi] = a + b * (ref_t + 0.05 * (X[lo:hi] - ref_t))

    def v_rowstats():
        check(lib.ocm_prep_rowstats_f32(ctx, ptr(X), p, n, p, ptr(rs), stream_handle(dev)), "rowstats")

    def v_rowfit(q):
        def run():
            check(lib.ocm_rowfit_f32(ctx, ptr(X), p, n, p, ptr(W[q]), q, ptr(coef), ptr(rs), stream_handle(dev)),
                  "rowfit")
        return run

    def v_snv():
        check(lib.ocm_snv_savgol_f32(ctx, ptr(X), p, n, p, 1, 0, None, ptr(out), p, stream_handle(dev)), "snv")

    def v_emsc(q):
        def run():
            check(lib.ocm_emsc_apply_f32(ctx, ptr(X), p, n, p, ptr(W[q]), ptr(B[q]), q, ptr(out), p, None,
                                         stream_handle(dev)), "emsc")
        return run

    def v_torch_fit():
        return X @ W32[2].T

    def v_torch(q):
        def run():
            C = X @ W32[q].T
            return (X - C[:, :1] - C[:, 2:] @ B32[q][2:]) / C[:, 1:2]
        return run

    diag = {}

    def fit_predict(view, name):
        from ocm import engine
        from ocm.prepview import materialised_count

        c0 = materialised_count(0)
        model = SIMCA(n_components=k, model_class=0, type="alt", t2lim="Fdist", qlim="jm", verbose=False)
        model.fit(view, y)
        marks = engine.last_gram_marks(0)
        pred = model.predict(view)
        # what the data makes of the fit, beside the time: eigensolver iterations, rows the Gram's
        # outlier guard set aside, views written out on a fallback path
        diag[name] = {"eig_iters": int(model._fits[0].eig_iters), "gram_outlier_marks": int(marks),
                      "materialised_views": materialised_count(0) - c0}
        return pred

    def v_view_snv():
        return fit_predict(preprocess.snv_savgol(Xv, 5, 2, 1, 1.0, snv=True, lazy=True), "view_snv_sg5")

    def v_view_msc():
        return fit_predict(est[2].transform(Xv, 5, 2, 1, lazy=True), "view_msc_sg5")

    variants = {"rowstats": v_rowstats, "rowfit_q2": v_rowfit(2), "rowfit_q4": v_rowfit(4), "rowfit_q8": v_rowfit(8),
                "snv": v_snv, "emsc_q2": v_emsc(2), "emsc_q4": v_emsc(4), "torch_fit_q2": v_torch_fit,
                "torch_q2": v_torch(2), "torch_q4": v_torch(4), "view_snv_sg5_fit_predict": v_view_snv,
                "view_msc_sg5_fit_predict": v_view_msc}
    # warm-up (code objects, workspace growth, rocBLAS algorithm choice) and agreement with the torch composition
    agree = {}
    for name, fn in list(variants.items()):
        try:
            r = fn()
        except _lib.OcmNotConverged as exc:  # an estimator fit that does not converge on these rows: reported
            agree[f"{name}_error"] = str(exc)[:200]
            del variants[name]
            continue
        if name in ("torch_q2", "torch_q4"):
            q = int(name[-1])
            v_emsc(q)()
            d = (out[:4096] - r[:4096]).abs().max() / r[:4096].abs().max()
            agree[f"emsc_q{q}_maxrel_vs_torch_f32"] = float(d)
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
    res = {"rows": n, "p": p, "k": k, "reps": args.reps, "timing": "device events per call, variants alternating",
           "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for name, t in times.items()},
           "read_TBps": {name: round(n * p * 4 / med[name] / 1e9, 3)
                         for name in ("rowstats", "rowfit_q2", "rowfit_q4", "rowfit_q8")},
           "read_plus_write_TBps": {name: round(2 * n * p * 4 / med[name] / 1e9, 3)
                                    for name in ("snv", "emsc_q2", "emsc_q4")},
           "rowfit_q2_over_rowstats": round(med["rowfit_q2"] / med["rowstats"], 3),
           "emsc_q2_over_snv": round(med["emsc_q2"] / med["snv"], 3),
           "torch_fit_q2_over_rowfit_q2": round(med["torch_fit_q2"] / med["rowfit_q2"], 3),
           "torch_q2_over_emsc_q2": round(med["torch_q2"] / med["emsc_q2"], 3),
           "torch_q4_over_emsc_q4": round(med["torch_q4"] / med["emsc_q4"], 3),
           "agreement": agree, "view_fit_diagnostics": diag}
    if "view_msc_sg5_fit_predict" in med and "view_snv_sg5_fit_predict" in med:
        res["view_msc_minus_view_snv_ms"] = round(med["view_msc_sg5_fit_predict"] - med["view_snv_sg5_fit_predict"], 4)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
