"""The DEEP calls (NTTPlan.deep_points / open_matrix / deep_quotient) on one GPU, each against a
device-to-device copy that moves the same bytes: the fold's yardstick (tools/bench_fold.py).

Traffic counted per call, with N rows, W columns, d the extension degree and e the element bytes:
  points    writes N d e;
  open      reads the matrix N W e and the inverses N d e (once: the strips of one row chunk re-read them from
            cache), writes W d e;
  quotient  reads N W e + N d e + W d e, writes N d e.
The yardstick is a copy whose read plus write are that many bytes (a copy of half of them);
`<call>_over_copy` is the call's median time over that copy's.

Cases: 2^20 rows x widths 16, 64 and 256; BabyBear with its quartic extension (d = 4) and Goldilocks with its
quadratic one (d = 2); rows bit-reversed, the field's generator as the shift.  The routes of a case are timed in
ONE process, interleaved step by step, each step one call between two device events; the figure is the
median of `--steps` steps (at least 20) after `--warmup` untimed ones.  Before the timing column 0, the
evaluations of the constant 7, must open to 7, and a second open must give the same bits.

Every case runs as a child process under its own `timeout -k 10`; the driver stops at the first that fails.

    python tools/bench_deep.py [--out profiles/deep/bench.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_ROWS = 20
CASES = [(name, fid, w) for name, fid in (("babybear", 4), ("goldilocks", 3)) for w in (16, 64, 256)]


def child(name, fid, width, steps, warmup):
    import torch

    from ntt_amd.fields import EXTENSIONS, field_params
    from ntt_amd.ntt import NTTPlan
    p, g = field_params(fid)
    d, w = EXTENSIONS[fid]
    pl = NTTPlan(fid, LOG_ROWS, 1)
    N, eb = pl.n, pl.elem_bytes
    dev = "cuda:0"
    # seeded canonical elements: the plan's own fill, one rotation per column, row-major [N][width]
    base = pl.fill(pl.empty(), "random", seed=11)
    mat = torch.empty(N * width, dtype=pl.dtype, device=dev).view(N, width)
    for b in range(width):
        mat[:, b] = torch.roll(base, 17 * b)
    mat[:, 0] = 7  # the constant polynomial 7
    mat = mat.view(-1)
    inv = torch.empty(N * d, dtype=pl.dtype, device=dev)
    val = torch.empty(width * d, dtype=pl.dtype, device=dev)
    out = torch.empty(N * d, dtype=pl.dtype, device=dev)
    z = [(0x9E3779B97F4A7C15 * (j + 1)) % p for j in range(d)]
    alpha = [(0xD1B54A32D192ED03 * (j + 1)) % p for j in range(d)]
    kw = dict(ext_degree=d, ext_w=w, log_rows=LOG_ROWS)
    traffic = {"points": N * d * eb, "open": (N * width + N * d + width * d) * eb,
               "quotient": (N * width + 2 * N * d + width * d) * eb}
    copies = {}
    for r, t in traffic.items():
        src = torch.empty(t // 2, dtype=torch.uint8, device=dev)
        copies[r] = (src, torch.empty_like(src))

    routes = {
        "points": lambda: pl.deep_points(inv, z, shift=g, bitrev=True, **kw),
        "open": lambda: pl.open_matrix(mat, width, inv, val, z, shift=g, bitrev=True, **kw),
        "quotient": lambda: pl.deep_quotient(mat, width, inv, val, out, alpha, **kw),
    }
    for r in list(routes):
        s, t = copies[r]
        routes[r + "_copy"] = (lambda s=s, t=t: t.copy_(s))
    for r in ("points", "open", "quotient"):
        routes[r]()
    torch.cuda.synchronize()
    first = val.clone()
    if [int(v) for v in first[:d].cpu()] != [7] + [0] * (d - 1):
        raise SystemExit(f"check: the constant column does not open to 7 ({name}, width {width}): {first[:d].cpu()}")
    routes["open"]()
    torch.cuda.synchronize()
    if not torch.equal(first, val):
        raise SystemExit(f"check: two opens differ ({name}, width {width})")
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
    chunks, lanes = pl.deep_info(width, log_rows=LOG_ROWS, ext_degree=d)
    row = {"field": name, "log_rows": LOG_ROWS, "width": width, "ext_degree": d, "open_row_chunks": chunks,
           "quotient_lanes_per_row": lanes, "steps": steps, "warmup": warmup}
    for r in ("points", "open", "quotient"):
        row[r + "_bytes"] = traffic[r]
        row[r + "_ms"] = round(med[r], 5)
        row[r + "_min_ms"] = round(min(ms[r]), 5)
        row[r + "_max_ms"] = round(max(ms[r]), 5)
        row[r + "_copy_ms"] = round(med[r + "_copy"], 5)
        row[r + "_over_copy"] = round(med[r] / med[r + "_copy"], 3)
        row[r + "_gbs"] = round(traffic[r] / (med[r] * 1e-3) / 1e9, 1)
        row[r + "_copy_gbs"] = round(traffic[r] / (med[r + "_copy"] * 1e-3) / 1e9, 1)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep", "bench.jsonl"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # one case in this process (also what a profiler is pointed at, with few steps)
        name, fid, width = a.child
        child(name, int(fid), int(width), a.steps, a.warmup)
        return
    if a.steps < 20:
        raise SystemExit("--steps: the median is taken over at least 20 steps")
    rows = []
    for name, fid, width in CASES:
        cmd = ["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--child", name, str(fid), str(width)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-3000:], sep="\n")
            raise SystemExit(f"{name} width {width}: exit status {r.returncode}; stopping")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
