#!/usr/bin/env python3
"""Time the contribution kernel on the bench workload (1M×2048 fp32 in HBM,
k = 20) in ONE process, against what a user would write without it:

  profile    ocm_contrib_f32 without E / C: row sums + the group profiles
  matrices   ocm_contrib_f32 writing E and C (m×p each) as well
  score      ocm_score_f32_diag on the same rows (context: the scoring pass)
  torch      Y = X − μ; T = Y·Pᵀ; E = Y − T·P; q = (E·E).sum(0);
             C = Y·((T·a)·P); c = C.sum(0)        (float32 torch expressions)

Every variant is warmed up, then timed `--reps` times with device events, the
variants alternating inside each repeat; median, min and max per variant.
Writes profiles/contrib_ab.json (or --out) and prints the same JSON line.

    python scripts/bench_contrib.py [--rows 1000000] [--p 2048] [--k 20] [--reps 7]"""
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "contrib_ab.json"))
    args = ap.parse_args()
    import torch

    from bench import synth_device
    from ocm import engine

    assert torch.cuda.is_available(), "bench_contrib.py needs a HIP device"
    dev = torch.device("cuda", 0)
    n, p, k = args.rows, args.p, args.k
    X = synth_device(n, p, 20, 7, dev)
    mean = X[:4096].double().mean(0)
    P, _ = torch.linalg.qr(torch.randn(p, k, dtype=torch.float64, device=dev))
    P = P.T.contiguous()
    inv = torch.linspace(1.0, 0.1, k, dtype=torch.float64, device=dev)
    group = (torch.arange(n, device=dev) % 2).to(torch.uint8)
    P32, mu32, a32 = P.float(), mean.float(), inv.float()

    def v_profile():
        return engine.contributions(X, None, n, P, mean, inv, group=group, ngroups=2)

    def v_matrices():
        return engine.contributions(X, None, n, P, mean, inv, group=group, ngroups=2, want_E=True, want_C=True)

    def v_score():
        return engine.score(X, None, n, P, mean, inv)

    def v_torch():
        Y = X - mu32
        T = Y @ P32.T
        E = Y - T @ P32
        q = (E * E).sum(0)
        C = Y * ((T * a32) @ P32)
        c = C.sum(0)
        return q, c

    variants = {"profile": v_profile, "matrices": v_matrices, "score": v_score, "torch": v_torch}
    # warm-up (code objects, workspace growth, rocBLAS algorithm choice) and agreement of the profiles
    warm = {name: fn() for name, fn in variants.items()}
    torch.cuda.synchronize()
    q_t, c_t = warm["torch"]
    prof = warm["profile"]["profiles"].sum(0)
    agree = {"q_profile_maxrel_vs_torch": float(((prof[0] - q_t.double()).abs() / q_t.double().abs()).max()),
             "t2_profile_maxrel_vs_torch": float(((prof[1] - c_t.double()).abs() / c_t.double().abs().max()).max()),
             "profile_equals_matrices_run": bool(torch.equal(warm["profile"]["profiles"],
                                                             warm["matrices"]["profiles"]))}
    del warm, q_t, c_t, prof
    torch.cuda.empty_cache()
    times = {name: [] for name in variants}
    st = torch.cuda.current_stream()
    for _ in range(args.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            out = fn()
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            del out
    res = {"rows": n, "p": p, "k": k, "reps": args.reps, "timing": "device events per call, variants alternating",
           "ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for name, t in times.items()}}
    med = {name: statistics.median(t) for name, t in times.items()}
    res["torch_over_profile"] = round(med["torch"] / med["profile"], 3)
    res["torch_over_matrices"] = round(med["torch"] / med["matrices"], 3)
    res["profile_over_score"] = round(med["profile"] / med["score"], 3)
    res["agreement"] = agree
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
