"""The FRI fold (NTTPlan.fri_fold) on one GPU: its two load forms against a device-to-device copy that moves
the same bytes.

A fold of arity 2^k reads the N d elements of its input once and writes N d / 2^k: (1 + 2^-k) N d elem_bytes
bytes of traffic.  The yardstick is a copy whose read plus write are that many bytes (a copy of half of them),
the rate a streaming pass can reach; `<form>_over_copy` is the fold's median time over the copy's (1.0 = the
fold is free beside its own traffic).

  direct: NTT_FOLD_STAGED=0, every thread loads its own fibre of 2^k d elements;
  staged: NTT_FOLD_STAGED=1, lane l of a workgroup loads 16 B at base + 16 l and the fibres reach their
          threads through LDS.

Cases: BabyBear with its quartic extension (d = 4) and Goldilocks with its quadratic one (d = 2), N = 2^22,
arity 2, 4 and 16, the field's generator as the shift.  The three routes of a case are timed in ONE process,
interleaved step by step (direct, staged, copy, direct, ...), each step one call between two device events;
the figure is the median of `--steps` steps (at least 20) after `--warmup` untimed ones.  Before the timing
the two forms' outputs are compared bit for bit.

Every case runs as a child process under its own `timeout -k 10`; the driver stops at the first that fails.

    python tools/bench_fold.py [--out profiles/fold/bench.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_N = 22
CASES = [(name, fid, k) for name, fid in (("babybear", 4), ("goldilocks", 3)) for k in (1, 2, 4)]


def child(name, fid, k, steps, warmup):
    import torch

    from ntt_amd.fields import EXTENSIONS, field_params
    from ntt_amd.ntt import NTTPlan
    p, g = field_params(fid)
    d, w = EXTENSIONS[fid]
    pl = NTTPlan(fid, LOG_N, 1)
    N, eb = pl.n, pl.elem_bytes
    # seeded canonical elements: the plan's own fill, one rotation per coordinate, row-major [N][d]
    base = pl.fill(pl.empty(), "random", seed=11)
    x = torch.stack([torch.roll(base, b) for b in range(d)]).t().contiguous().view(-1)
    outs = {f: torch.empty((N >> k) * d, dtype=pl.dtype, device="cuda:0") for f in ("direct", "staged")}
    beta = [(0x9E3779B97F4A7C15 * (j + 1)) % p for j in range(d)]
    traffic = (N + (N >> k)) * d * eb
    c_src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda:0")
    c_dst = torch.empty_like(c_src)

    def fold(form):
        os.environ["NTT_FOLD_STAGED"] = "1" if form == "staged" else "0"
        pl.fri_fold(x, outs[form], k, beta, ext_degree=d, ext_w=w, shift=g)

    routes = {"direct": lambda: fold("direct"), "staged": lambda: fold("staged"), "copy": lambda: c_dst.copy_(c_src)}
    fold("direct")
    fold("staged")
    torch.cuda.synchronize()
    if not torch.equal(outs["direct"], outs["staged"]):
        raise SystemExit(f"check: the two load forms disagree ({name}, arity 2^{k})")
    for _ in range(warmup):
        for f in routes.values():
            f()
    torch.cuda.synchronize()
    ms = {r: [] for r in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(steps):
        for r, f in routes.items():
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[r].append(e0.elapsed_time(e1))
    med = {r: statistics.median(v) for r, v in ms.items()}
    row = {"field": name, "log_rows": LOG_N, "ext_degree": d, "log_arity": k, "fibre_bytes": (d * eb) << k,
           "traffic_bytes": traffic, "steps": steps, "warmup": warmup}
    for r in routes:
        row[r + "_ms"] = round(med[r], 5)
        row[r + "_min_ms"] = round(min(ms[r]), 5)
        row[r + "_max_ms"] = round(max(ms[r]), 5)
    for r in ("direct", "staged"):
        row[r + "_over_copy"] = round(med[r] / med["copy"], 3)
        row[r + "_gbs"] = round(traffic / (med[r] * 1e-3) / 1e9, 1)
    row["copy_gbs"] = round(traffic / (med["copy"] * 1e-3) / 1e9, 1)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold", "bench.jsonl"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: the median is taken over at least 20 steps")
    if a.child:
        name, fid, k = a.child
        child(name, int(fid), int(k), a.steps, a.warmup)
        return
    rows = []
    for name, fid, k in CASES:
        cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--child", name, str(fid), str(k)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-3000:], sep="\n")
            raise SystemExit(f"{name} arity 2^{k}: exit status {r.returncode}; stopping")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
