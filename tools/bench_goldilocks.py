"""Goldilocks forward transforms on one GPU: the 8-byte engine against the routes a caller had before it.

  (a) field 3, one limb: the Eng64G plan (8-byte elements);
  (b) the same modulus zero-padded to 4 limbs through ntt_plan_create_custom (32-byte elements, the
      nine-limb 256-bit engine): the only route before the engine existed;
  (c) the P469762049 plan (8-byte `long long` elements, 4-byte scratch): context only, another field.

Sizes 2^20 and 2^24.  The three plans of a size are timed in ONE process, interleaved round by round
(a, b, c, a, b, c, ...), each round a window of `--steps` transforms ended by a device synchronise;
the figure of a configuration is the median of its rounds, and the spread (min, max) is kept.  Per
launch times come from the plan's own events (ntt_plan_last_launch_ms) in a separate pass afterwards.
"Roofline fraction" is the algorithm's least traffic, one read and one write of the vector, over the
time, as a fraction of 8 TB/s; a p-pass schedule moves p times that.

The driver runs each GPU step as a child under its own `timeout -k 10` and stops at the first step
that fails: first a check that (a) and (b) compute the same transform, then the timing.

    python tools/bench_goldilocks.py [--out profiles/goldilocks/bench.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 0xFFFFFFFF00000001
PEAK_BYTES_PER_S = 8e12
SIZES = (20, 24)


def make_plans(log_n):
    from ntt_amd.ntt import NTTPlan
    return {"a_goldilocks_1limb": NTTPlan(3, log_n, 1),
            "b_goldilocks_4limb_custom": NTTPlan(log_n=log_n, limbs64=4, modulus=P, generator=7),
            "c_p469762049_1limb": NTTPlan(0, log_n, 1)}


def step_check():
    """(a) and (b) agree on a seeded input at 2^20 (limb 0 equal, limbs 1..3 zero)."""
    import torch
    plans = make_plans(20)
    a, b = plans["a_goldilocks_1limb"], plans["b_goldilocks_4limb_custom"]
    x = a.fill(a.empty(), "random", seed=7)
    y = torch.zeros((1 << 20, 4), dtype=torch.int64, device=x.device)
    y[:, 0] = x
    a.forward(x)
    b.forward(y)
    torch.cuda.synchronize()
    if not (torch.equal(y[:, 0], x) and not bool(y[:, 1:].any())):
        raise SystemExit("check: the 1-limb and the 4-limb plans disagree at 2^20")
    print("check ok", flush=True)


def step_time(out, steps, rounds, warmup):
    import torch
    rows = []
    for log_n in SIZES:
        plans = make_plans(log_n)
        data = {k: pl.fill(pl.empty(), "random", seed=1) for k, pl in plans.items()}
        for k, pl in plans.items():
            for _ in range(warmup):
                pl.forward(data[k])
        torch.cuda.synchronize()
        samples = {k: [] for k in plans}
        for _ in range(rounds):
            for k, pl in plans.items():
                t = data[k]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    pl.forward(t)
                torch.cuda.synchronize()
                samples[k].append((time.perf_counter() - t0) / steps)
        for k, pl in plans.items():
            pl.set_profiling(True)
            per = []
            for _ in range(9):
                pl.forward(data[k])
                torch.cuda.synchronize()
                per.append(pl.last_launch_ms())
            labels = pl.last_launch_labels()
            pl.set_profiling(False)
            launch_ms = [statistics.median(p[i] for p in per) for i in range(min(len(p) for p in per))]
            s = statistics.median(samples[k])
            n = 1 << log_n
            rows.append({"config": k, "log_n": log_n, "elem_bytes": pl.elem_bytes, "passes": pl.passes,
                         "ms": s * 1e3, "ms_min": min(samples[k]) * 1e3, "ms_max": max(samples[k]) * 1e3,
                         "rounds": rounds, "steps": steps, "elements_per_s": n / s,
                         "algorithmic_bytes": 2 * n * pl.elem_bytes,
                         "roofline_fraction": 2 * n * pl.elem_bytes / s / PEAK_BYTES_PER_S,
                         "launch_labels": labels, "launch_ms": launch_ms})
            print(json.dumps(rows[-1]), flush=True)
        del plans, data
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    by = {(r["config"][0], r["log_n"]): r["ms"] for r in rows}
    for log_n in SIZES:
        print(f"2^{log_n}: (a)/(b) = {by[('a', log_n)] / by[('b', log_n)]:.3f}, "
              f"(a)/(c) = {by[('a', log_n)] / by[('c', log_n)]:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goldilocks", "bench.jsonl"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step", choices=("check", "time"), help="run one GPU step in this process (the driver's children)")
    args = ap.parse_args()
    if args.step == "check":
        return step_check()
    if args.step == "time":
        return step_time(args.out, args.steps, args.rounds, args.warmup)
    me = [sys.executable, os.path.abspath(__file__), "--out", args.out, "--steps", str(args.steps), "--rounds",
          str(args.rounds), "--warmup", str(args.warmup)]
    for name, limit in (("check", 120), ("time", 420)):
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + me + ["--step", name], cwd=ROOT).returncode
        if rc != 0:
            raise SystemExit(f"step {name} failed (exit status {rc}); nothing further is run")


if __name__ == "__main__":
    main()
