"""BabyBear forward transforms on one GPU: the 4-byte engine against the routes a caller had before it.

  (a) field 4, one limb: the Eng31 plan (4-byte elements);
  (b) the same modulus zero-padded to 4 limbs through ntt_plan_create_custom (32-byte elements, the
      nine-limb 256-bit engine): the only route before the engine existed;
  (c) the P469762049 plan (8-byte `long long` elements, 4-byte scratch): context only, another field.

Single transforms at 2^20 and 2^24, and a batched line: 64 transforms of 2^16 through
ntt_forward_batch, (a) against (b).  The plans of a size are timed in ONE process, interleaved round
by round (a, b, c, a, b, c, ...), each round a window of `--steps` calls ended by a device
synchronise; the figure of a configuration is the median of its rounds, and the spread (min, max) is
kept.  Per launch times come from the plan's own events (ntt_plan_last_launch_ms) in a separate pass
afterwards.  "Roofline fraction" is the algorithm's least traffic, one read and one write of the
vector, over the time, as a fraction of 8 TB/s; a p-pass schedule moves p times that.

--configs a times (a) alone: the A/B runs of a library variant (NTT_LIB_PATH) or of an environment
switch (NTT_PASS1_FULL), written to another --out.

The driver runs each GPU step as a child under its own `timeout -k 10` and stops at the first step
that fails: first a check that (a) and (b) compute the same transform, then the timing.

    python tools/bench_field31.py [--out profiles/field31/bench.jsonl]
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

P, G = 2013265921, 31
PEAK_BYTES_PER_S = 8e12
CASES = ((20, 1), (24, 1), (16, 64))  # (log_n, batch)


def make_plans(log_n, batch, configs):
    from ntt_amd.ntt import NTTPlan
    plans = {}
    if "a" in configs:
        plans["a_babybear_4byte"] = NTTPlan(4, log_n, 1)
    if "b" in configs:
        plans["b_babybear_4limb_custom"] = NTTPlan(log_n=log_n, limbs64=4, modulus=P, generator=G)
    if "c" in configs and batch == 1:
        plans["c_p469762049_1limb"] = NTTPlan(0, log_n, 1)
    return plans


def step_check():
    """(a) and (b) agree on a seeded input at 2^20 (limb 0 equal, limbs 1..3 zero)."""
    import torch
    plans = make_plans(20, 1, "ab")
    a, b = plans["a_babybear_4byte"], plans["b_babybear_4limb_custom"]
    x = a.fill(a.empty(), "random", seed=7)
    y = torch.zeros((1 << 20, 4), dtype=torch.int64, device=x.device)
    y[:, 0] = x.to(torch.int64) & 0xFFFFFFFF
    a.forward(x)
    b.forward(y)
    torch.cuda.synchronize()
    if not (torch.equal(y[:, 0], x.to(torch.int64) & 0xFFFFFFFF) and not bool(y[:, 1:].any())):
        raise SystemExit("check: the 4-byte and the 4-limb plans disagree at 2^20")
    print("check ok", flush=True)


def step_time(out, steps, rounds, warmup, configs):
    import torch
    rows = []
    for log_n, batch in CASES:
        plans = make_plans(log_n, batch, configs)
        run = {k: ((lambda t, pl=pl: pl.forward(t)) if batch == 1 else (lambda t, pl=pl: pl.forward_batch(t, batch)))
               for k, pl in plans.items()}
        data = {}
        for k, pl in plans.items():
            data[k] = pl.empty(batch)
            one = pl.fill(pl.empty(), "random", seed=1)
            for b in range(batch):
                data[k][b * one.shape[0]:(b + 1) * one.shape[0]] = one
        for k in plans:
            for _ in range(warmup):
                run[k](data[k])
        torch.cuda.synchronize()
        samples = {k: [] for k in plans}
        for _ in range(rounds):
            for k in plans:
                t = data[k]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    run[k](t)
                torch.cuda.synchronize()
                samples[k].append((time.perf_counter() - t0) / steps)
        for k, pl in plans.items():
            pl.set_profiling(True)
            per = []
            for _ in range(9):
                run[k](data[k])
                torch.cuda.synchronize()
                per.append(pl.last_launch_ms())
            labels = pl.last_launch_labels()
            pl.set_profiling(False)
            launch_ms = [statistics.median(p[i] for p in per) for i in range(min(len(p) for p in per))]
            s = statistics.median(samples[k])
            n = batch << log_n
            rows.append({"config": k, "log_n": log_n, "batch": batch, "elem_bytes": pl.elem_bytes, "passes": pl.passes,
                         "ms": s * 1e3, "ms_min": min(samples[k]) * 1e3, "ms_max": max(samples[k]) * 1e3,
                         "rounds": rounds, "steps": steps, "elements_per_s": n / s,
                         "algorithmic_bytes": 2 * n * pl.elem_bytes,
                         "roofline_fraction": 2 * n * pl.elem_bytes / s / PEAK_BYTES_PER_S,
                         "launch_labels": labels, "launch_ms": launch_ms,
                         "lib": os.path.basename(os.environ.get("NTT_LIB_PATH", "libntt.so")),
                         "pass1_full_env": os.environ.get("NTT_PASS1_FULL", "")})
            print(json.dumps(rows[-1]), flush=True)
        del plans, data, run
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    by = {(r["config"][0], r["log_n"], r["batch"]): r["ms"] for r in rows}
    for log_n, batch in CASES:
        a, b, c = (by.get((k, log_n, batch)) for k in "abc")
        line = f"{batch} x 2^{log_n}:"
        if a and b:
            line += f" (a)/(b) = {a / b:.3f}"
        if a and c:
            line += f" (a)/(c) = {a / c:.3f}"
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field31", "bench.jsonl"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="abc", help="which of a, b, c to time (default all)")
    ap.add_argument("--step", choices=("check", "time"), help="run one GPU step in this process (the driver's children)")
    args = ap.parse_args()
    if args.step == "check":
        return step_check()
    if args.step == "time":
        return step_time(args.out, args.steps, args.rounds, args.warmup, args.configs)
    me = [sys.executable, os.path.abspath(__file__), "--out", args.out, "--steps", str(args.steps), "--rounds",
          str(args.rounds), "--warmup", str(args.warmup), "--configs", args.configs]
    todo = (("check", 120), ("time", 420)) if "b" in args.configs else (("time", 420),)
    for name, limit in todo:
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + me + ["--step", name], cwd=ROOT).returncode
        if rc != 0:
            raise SystemExit(f"step {name} failed (exit status {rc}); nothing further is run")


if __name__ == "__main__":
    main()
