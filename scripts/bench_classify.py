#!/usr/bin/env python3
"""Time the multi-class scoring kernel (ocm_score_multi_f32) in ONE process
against the composition of the per-class kernels it replaces, on 1M float32
rows in HBM:

  fused      engine.score_multi: one launch for all classes (pred, ratio,
             index, nearest, n_accept and the count tables)
  composed   ocm.multiclass.classify_composed: engine.score + engine.decide per
             class and the torch epilogue, the same outputs
  fused_rows / composed_rows   the same two without y_true (no count tables)
  predict    the reference's predict loop alone: engine.score with the fused
             decision per class (context: the (m, C) matrix and nothing else)

at the shapes  p = 2048, k = 20, C = 3;  p = 2048, k = 12, C = 4;  p = 1000,
k = 12, C = 4 and p = 1536, k = 12, C = 4 (the last two take the per-class
route's two-sweep kernel, which reads X twice per class; at p = 1536 the fused
kernel's row tile does not fit the LDS either).  Every variant is warmed up, then timed `--reps`
times with device events, the variants alternating inside each repeat; median,
min and max per variant.  Writes profiles/classify_ab.json (or --out) and
prints the same JSON line.

    python scripts/bench_classify.py [--rows 1000000] [--reps 7] [--shapes 2048:20:3,2048:12:4,1000:12:4,1536:12:4]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)


def models(X, p, k, C, dev):
    """C class models around the data: orthonormal loadings, means near the data mean, 1/λ over a decade,
    'alt' decisions whose limits sit at the median T² / Q of a sample (about half the rows accepted)."""
    import torch

    from ocm import engine

    g = torch.Generator(device="cpu").manual_seed(1234 + p + k + C)
    mean = X[:4096].double().mean(0)
    fits, decs = [], []
    for c in range(C):
        Pc, _ = torch.linalg.qr(torch.randn(p, k, dtype=torch.float64, generator=g).to(dev))
        fit = SimpleNamespace(k=k, P64=Pc.T.contiguous(),
                              mean64=mean + 0.01 * (c + 1) * torch.randn(p, dtype=torch.float64, generator=g).to(dev),
                              inv_diag=torch.linspace(1.0, 0.1, k, dtype=torch.float64, device=dev))
        sc = engine.score(X[:4096], None, 4096, fit.P64, fit.mean64, fit.inv_diag)
        decs.append(engine.make_decision("alt", 1.0 / float(sc["T2"].median()), 1.0 / float(sc["Q"].median()),
                                         2.0 ** 0.5))
        fits.append(fit)
    return fits, decs


def bench_shape(n, p, k, C, reps, dev):
    import torch

    from bench import synth_device
    from ocm import engine, multiclass

    X = synth_device(n, p, 20, 7, dev)
    fits, decs = models(X, p, k, C, dev)
    stack = engine.stack_models(fits)
    y = (torch.arange(n, device=dev) % (C + 1)).to(torch.uint8)
    want = tuple(w for w in engine.MULTI_WANT if w not in ("T2", "Q"))

    def v_fused():
        return engine.score_multi(X, None, n, fits, decs, want=want, y_true=y, stack=stack)

    def v_composed():
        return multiclass.classify_composed(X, fits, decs, y_index=y)

    def v_predict():
        pred = torch.zeros((n, C), dtype=torch.float64, device=dev)
        for i, (fit, dec) in enumerate(zip(fits, decs)):
            engine.score(X, None, n, fit.P64, fit.mean64, fit.inv_diag, want_T2=False, want_Q=False, decision=dec,
                         accept_out=pred[:, i:], accept_stride=C)
        return pred

    def v_fused_rows():
        return engine.score_multi(X, None, n, fits, decs, want=want, stack=stack)

    def v_composed_rows():
        return multiclass.classify_composed(X, fits, decs)

    variants = {"fused": v_fused, "composed": v_composed, "fused_rows": v_fused_rows,
                "composed_rows": v_composed_rows, "predict": v_predict}
    warm = {name: fn() for name, fn in variants.items()}  # code objects, workspace growth
    torch.cuda.synchronize()
    f, c = warm["fused"], warm["composed"]
    agree = {"ratio_maxrel": float(((f["ratio"] - c["ratio"]).abs() / c["ratio"].abs()).max()),
             "pred_differs": int((f["pred"] != c["pred"]).sum()),
             "index_differs": int((f["index"].to(torch.int64) != c["index"]).sum()),
             "accepted_share": float(c["pred"].mean())}
    del warm, f, c
    torch.cuda.empty_cache()
    times = {name: [] for name in variants}
    st = torch.cuda.current_stream()
    for _ in range(reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            out = fn()
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            del out
    med = {name: statistics.median(t) for name, t in times.items()}
    return {"rows": n, "p": p, "k": k, "C": C,
            "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                   for name, t in times.items()},
            "composed_over_fused": round(med["composed"] / med["fused"], 3),
            "composed_rows_over_fused_rows": round(med["composed_rows"] / med["fused_rows"], 3), "agreement": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="2048:20:3,2048:12:4,1000:12:4,1536:12:4", help="p:k:C, comma separated")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "classify_ab.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_classify.py needs a HIP device"
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    res = {"reps": args.reps, "timing": "device events per call, variants alternating",
           "shapes": [bench_shape(args.rows, p, k, C, args.reps, dev) for p, k, C in shapes]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
