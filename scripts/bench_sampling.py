#!/usr/bin/env python3
"""Time Kennard–Stone selection (csrc/ocm_kstone.hip) in ONE process, each figure
beside the same work written with torch ops:

  pair      ocm_ks_pair_f32, the farthest pair of n rows (q = 20) at n = 20k, 100k,
            beside torch's cdist-free form at a size where its n × n matrix fits
            (row blocks of 2048: subtract, square-sum, max per block)
  per pick  ocm_ks_select_f32, K picks after one explicit start, on the small
            (one workgroup, LDS) and the wide (one launch per pick) path over a
            range of n, beside the torch loop: per step subtract, square-sum,
            minimum, argmax (fp64, Z converted once outside the timed window; the
            pick stays on the device, so the loop never waits for the host)

The selection is host-launch bound, so a time is the host clock around the call
ending in a device synchronise; every variant is warmed up, then timed --reps
times, the variants alternating inside each repeat; medians.  The small / wide
crossover is read from the rows where both paths ran.  Writes
profiles/sampling_bench.json and .md (or --out) and prints the JSON line.

    python scripts/bench_sampling.py [--picks 200] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ocm-vae-simca_amd"))
sys.path.insert(0, REPO)

LDS_DYN = 160 * 1024 - 2048  # csrc/ocm_kstone.hip KS_LDS_DYN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--picks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pair-n", type=int, nargs="*", default=[20_000, 100_000])
    ap.add_argument("--n", type=int, nargs="*",
                    default=[500, 1000, 1800, 4000, 8000, 16000, 40_000, 100_000, 1_000_000])
    ap.add_argument("--q", type=int, nargs="*", default=[4, 20])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sampling_bench"))
    args = ap.parse_args()
    import torch

    from ocm import engine

    assert torch.cuda.is_available(), "bench_sampling.py needs a HIP device"
    dev = torch.device("cuda", 0)
    K = args.picks

    def data(n, q):
        g = torch.Generator(device=dev).manual_seed(1000 + q)
        return torch.randn((n, q), generator=g, device=dev, dtype=torch.float32)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def timed(variants):
        """{name: (median ms, min, max, last output)} of callables, warmed up, alternating."""
        outs = {}
        for name, fn in variants.items():
            _, outs[name] = wall(fn)
        ts = {name: [] for name in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                t, outs[name] = wall(fn)
                ts[name].append(t)
        return {name: (statistics.median(t), min(t), max(t), outs[name]) for name, t in ts.items()}

    def torch_pair(Z64, block=2048):
        n = Z64.shape[0]
        best = torch.full((), -1.0, dtype=torch.float64, device=dev)
        for i0 in range(0, n, block):
            t = Z64[i0:i0 + block, None, :] - Z64[None, :, :]
            d = (t * t).sum(dim=2)
            d = torch.triu(d, diagonal=i0 + 1)
            best = torch.maximum(best, d.max())
        return best

    def torch_loop(Z64, start, picks):
        n = Z64.shape[0]
        order = torch.empty(picks, dtype=torch.int64, device=dev)
        t = Z64 - Z64[start]
        m = (t * t).sum(dim=1)
        m[start] = -1.0
        for k in range(picks):
            p = torch.argmax(m)
            order[k] = p
            t = Z64 - Z64[p]
            m = torch.minimum(m, (t * t).sum(dim=1))
            m[p] = -1.0  # earlier picks stay at −1 under the minimum
        return order

    pair_rows = []
    for n in args.pair_n:
        Z = data(n, 20)
        variants = {"ocm": lambda: engine.ks_pair(Z)}
        torch_n = n if n <= 20_000 else None  # the n × q × block temporary: 20k rows need 6.5 GB per block
        if torch_n:
            Z64 = Z.double()
            variants["torch"] = lambda: torch_pair(Z64)
        r = timed(variants)
        row = {"n": n, "q": 20, "ocm_ms": round(r["ocm"][0], 3), "ocm_min": round(r["ocm"][1], 3),
               "ocm_max": round(r["ocm"][2], 3),
               "pairs_per_s": round(n * (n - 1) / 2 / r["ocm"][0] * 1e3, 0),
               "gfma_per_s": round(n * (n - 1) / 2 * 20 / r["ocm"][0] / 1e6, 1)}
        if torch_n:
            row["torch_ms"] = round(r["torch"][0], 3)
            row["same_d2"] = bool(abs(float(r["torch"][3]) - float(r["ocm"][3][1])) <= 1e-12 * float(r["torch"][3]))
        else:
            row["torch_ms"] = None  # not measured: the blocked n × n form does not fit a sensible temporary
        pair_rows.append(row)
        print(json.dumps({"pair": row}), flush=True)

    pick_rows = []
    for q in args.q:
        for n in args.n:
            picks = min(K, n - 1)
            Z = data(n, q)
            Z64 = Z.double()
            st = torch.zeros(1, dtype=torch.int64, device=dev)
            m_fit = n * 8 <= LDS_DYN
            z_fit = m_fit and n * q * 4 <= LDS_DYN - n * 8
            variants = {"wide": lambda: engine.ks_select(Z, st, picks + 1, path=2)["order_a"],
                        "torch": lambda: torch_loop(Z64, 0, picks)}
            if m_fit:
                variants["small"] = lambda: engine.ks_select(Z, st, picks + 1, path=1)["order_a"]
            r = timed(variants)
            ref = r["wide"][3][1:]
            row = {"n": n, "q": q, "picks": picks, "z_in_lds": bool(z_fit),
                   "wide_us_per_pick": round(r["wide"][0] / picks * 1e3, 2),
                   "small_us_per_pick": round(r["small"][0] / picks * 1e3, 2) if m_fit else None,
                   "torch_us_per_pick": round(r["torch"][0] / picks * 1e3, 2),
                   "wide_spread_us": [round(r["wide"][1] / picks * 1e3, 2), round(r["wide"][2] / picks * 1e3, 2)],
                   "torch_same_order": bool(torch.equal(r["torch"][3], ref)),
                   "small_same_order": bool(torch.equal(r["small"][3][1:], ref)) if m_fit else None}
            pick_rows.append(row)
            print(json.dumps({"pick": row}), flush=True)

    both = [r for r in pick_rows if r["small_us_per_pick"] is not None]
    res = {"picks": K, "reps": args.reps, "dtype": "float32 rows, fp64 distances",
           "timing": "host clock around the call + synchronise, variants alternating, median",
           "pair": pair_rows, "per_pick": pick_rows,
           "small_faster_at": [[r["n"], r["q"]] for r in both if r["small_us_per_pick"] <= r["wide_us_per_pick"]],
           "wide_faster_at": [[r["n"], r["q"]] for r in both if r["small_us_per_pick"] > r["wide_us_per_pick"]]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as fh:
        fh.write(line + "\n")
    with open(args.out + ".md", "w") as fh:
        fh.write("# Kennard–Stone selection on one MI355X (scripts/bench_sampling.py)\n\n")
        fh.write(f"{K} picks per run, {args.reps} repeats, medians; host clock around the call + synchronise.\n\n")
        fh.write("## Farthest pair (q = 20)\n\n| n | ocm_ks_pair ms | torch blocks ms | GFMA/s |\n|---|---|---|---|\n")
        for r in pair_rows:
            fh.write(f"| {r['n']} | {r['ocm_ms']} | {r['torch_ms'] if r['torch_ms'] is not None else 'not measured'} "
                     f"| {r['gfma_per_s']} |\n")
        fh.write("\n## Time per pick, µs\n\n| n | q | Z in LDS | small | wide | torch loop |\n|---|---|---|---|---|---|\n")
        for r in pick_rows:
            fh.write(f"| {r['n']} | {r['q']} | {'yes' if r['z_in_lds'] else 'no'} | "
                     f"{r['small_us_per_pick'] if r['small_us_per_pick'] is not None else '—'} | "
                     f"{r['wide_us_per_pick']} | {r['torch_us_per_pick']} |\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
