"""Low-degree extension on one GPU: ntt_lde_batch against the composed route a caller had before it.

  lde:      one ntt_lde_batch call (the first pass loads the n coefficients of each polynomial, takes
            the padding from registers and applies the shift at load);
  composed: zero-fill of the batch x N output, a strided copy of the coefficients into the head of
            each vector, then ntt_forward_coset per vector, which is every call the library had.

Shapes: BabyBear, Goldilocks and BN254 at N = 2^20, blowup 2 and 8 (log_blowup 1, 3), batch 1 and 16,
shift = the field's generator.  The two routes of a shape are timed in ONE process, alternating
round by round (lde, composed, lde, ...).  A round is a window of as many calls as fill about
`--window-ms` (calibrated per route), ended by a device synchronise, and is timed twice over: by the
host clock around the window (`*_ms`: what a caller waits for, enqueue cost included) and by a pair of
device events around the same calls (`*_dev_ms`: the stream's own time, which leaves out what the host
spends before the first launch but still contains any gap in which the device waits for the host).
The figure of a route is the median of its rounds; min and max are kept.  `*_launches` counts the
kernel launches and device copies / fills one call of the route enqueues.  Before the timing the two
routes' outputs are compared bit for bit on a seeded input.

Every field runs as a child process under its own `timeout -k 10`; the driver stops at the first
field that fails.

    python tools/bench_lde.py [--out profiles/lde/bench.jsonl]
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

FIELDS = (("babybear", 4, 1), ("goldilocks", 3, 1), ("bn254", 1, 4))  # name, field id, 64-bit limbs
LOG_N = 20
SHAPES = [(lb, batch) for lb in (1, 3) for batch in (1, 16)]


def child(name, fid, limbs, log_blowup, batch, window_ms, rounds, warmup):
    import torch

    from ntt_amd.fields import field_params
    from ntt_amd.ntt import NTTPlan
    p, g = field_params(fid)
    pl = NTTPlan(fid, LOG_N, limbs)
    N, n_in = pl.n, pl.n >> log_blowup
    # seeded canonical coefficients: the plan's own fill, cut to n_in per polynomial
    full = pl.fill(pl.empty(), "random", seed=11)
    coeffs = torch.cat([full[:n_in]] * batch).contiguous()
    out_a, out_b = pl.empty(batch), pl.empty(batch)

    def lde():
        pl.lde_batch(coeffs, out_a, log_blowup, g, batch)

    def composed():
        out_b.zero_()
        vb = out_b.view((batch, N) if limbs == 1 else (batch, N, limbs))
        vc = coeffs.view((batch, n_in) if limbs == 1 else (batch, n_in, limbs))
        vb[:, :n_in] = vc
        for v in range(batch):
            pl.forward_coset(vb[v], g)

    lde()
    composed()
    torch.cuda.synchronize()
    if not torch.equal(out_a, out_b):
        raise SystemExit(f"check: the two routes disagree ({name}, log_blowup {log_blowup}, batch {batch})")
    routes = {"lde": lde, "composed": composed}
    for f in routes.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    steps = {}
    for k, f in routes.items():  # calls per window, from a short timed run
        t0 = time.perf_counter()
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) * 1e3 / 20
        steps[k] = max(20, min(50000, int(window_ms / per) + 1))
    ms = {k: [] for k in routes}
    dev = {k: [] for k in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, f in routes.items():
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps[k]):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k])
            dev[k].append(e0.elapsed_time(e1) / steps[k])
    pl.set_profiling(True)
    lde()
    torch.cuda.synchronize()
    launches = dict(zip(pl.last_launch_labels(), [round(v, 4) for v in pl.last_launch_ms()]))
    pl.set_profiling(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    meddev = {k: statistics.median(v) for k, v in dev.items()}
    row = {"field": name, "log_n": LOG_N, "log_blowup": log_blowup, "batch": batch, "passes": pl.passes,
           "steps": steps, "rounds": rounds, "window_ms": window_ms,
           "lde_launches": len(launches), # composed: fill, strided copy, then per vector the plan's passes (+ k_scale_pow where the shift
           # is not fused into pass 1: the one-limb engines)
           "composed_launches": 2 + batch * (len(pl.passes) + (0 if limbs == 4 else 1)),
           "lde_dev_ms": round(meddev["lde"], 5), "composed_dev_ms": round(meddev["composed"], 5),
           "composed_over_lde_dev": round(meddev["composed"] / meddev["lde"], 3),
           "lde_ms": round(med["lde"], 5), "lde_min_ms": round(min(ms["lde"]), 5), "lde_max_ms": round(max(ms["lde"]), 5),
           "composed_ms": round(med["composed"], 5), "composed_min_ms": round(min(ms["composed"]), 5),
           "composed_max_ms": round(max(ms["composed"]), 5),
           "composed_over_lde": round(med["composed"] / med["lde"], 3), "lde_launch_ms": launches}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lde", "bench.jsonl"))
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        name, fid, limbs = a.child
        for lb, batch in SHAPES:
            child(name, int(fid), int(limbs), lb, batch, a.window_ms, a.rounds, a.warmup)
        return
    rows = []
    for name, fid, limbs in FIELDS:
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--window-ms", str(a.window_ms),
               "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--child", name, str(fid), str(limbs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-3000:], sep="\n")
            raise SystemExit(f"{name}: exit status {r.returncode}; stopping")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
