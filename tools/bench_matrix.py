"""Row-major matrix transforms on one GPU: the ntt_*_matrix calls against the route a caller had before
them on the same library, and against the batched-layout call of the same total size.

  matrix:   one call on the row-major [n][W] matrix (forward_matrix; lde_matrix with blow-up 2 and the
            field's generator as the shift);
  composed: what the library offered before: tensor.t().contiguous() into the batched layout [W][n],
            forward_batch / lde_batch with batch = W, and the transpose back to row-major -- three trips
            over the data;
  batched:  forward_batch / lde_batch alone on data already in the batched layout: what the row-major
            addressing costs (`matrix_over_batched` = batched time / matrix time, 1.0 = free).

Cases: BabyBear N = 2^20 at W = 16, 37, 256 and Goldilocks at W = 37, forward and extension.  The three
routes of a case are timed in ONE process, interleaved step by step (matrix, composed, batched,
matrix, ...), each step one call between two device events; the figure is the median of `--steps` steps
(at least 20) after `--warmup` untimed ones.  Before the timing the matrix and composed routes' outputs are
compared bit for bit.  `matrix_gbs` is the bytes the matrix call must move (each pass reads and writes
the matrix once; an extension's first pass reads the n coefficient rows only) over its time, and
`matrix_hbm_frac` that rate over the 6.3 TB/s a streaming copy reaches on this device (8 TB/s spec).

After the two plain rows of a case comes one `variants` row: the coset forward, the bit-reversed forward,
the coset inverse and the bit-reversed extension (forward_matrix(shift=g), forward_matrix(bitrev_out=True),
inverse_matrix(shift=g), lde_matrix(bitrev_out=True)), each timed interleaved with the plain call of the
same shape in the same loop; `<variant>_over_plain` is the variant's median over the plain call's (1.0 =
free), and the per-launch times of the plain and the coset inverse show what the c^-j epilogue costs the
final pass.  --no-variants leaves that row out (a library without the _ex calls).

Every case runs as a child process under its own `timeout -k 10`; the driver stops at the first that fails.

    python tools/bench_matrix.py [--out profiles/matrix/bench.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_N = 20
CASES = [("babybear", 4, 16), ("babybear", 4, 37), ("babybear", 4, 256), ("goldilocks", 3, 37)]  # name, field id, W
HBM_COPY_TBS = 6.3


def variants(pl, name, width, g, x_rows, steps, warmup):
    import torch
    N, n_in = pl.n, pl.n >> 1
    src = x_rows[:n_in].contiguous().view(-1)
    data = x_rows.contiguous().view(-1).clone()  # transformed in place over and over: the time does not depend on the values
    out = torch.empty(N * width, dtype=pl.dtype, device="cuda:0")
    routes = {
        "forward": lambda: pl.forward_matrix(data, width),
        "forward_coset": lambda: pl.forward_matrix(data, width, shift=g),
        "forward_bitrev": lambda: pl.forward_matrix(data, width, bitrev_out=True),
        "inverse": lambda: pl.inverse_matrix(data, width),
        "inverse_coset": lambda: pl.inverse_matrix(data, width, shift=g),
        "lde": lambda: pl.lde_matrix(src, out, 1, g, width),
        "lde_bitrev": lambda: pl.lde_matrix(src, out, 1, g, width, bitrev_out=True),
    }
    plain_of = {"forward_coset": "forward", "forward_bitrev": "forward", "inverse_coset": "inverse", "lde_bitrev": "lde"}
    for _ in range(warmup):
        for f in routes.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(steps):
        for k, f in routes.items():
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    launches = {}
    pl.set_profiling(True)
    for k, f in routes.items():
        f()
        torch.cuda.synchronize()
        launches[k] = dict(zip(pl.last_launch_labels(), [round(v, 4) for v in pl.last_launch_ms()]))
    pl.set_profiling(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"field": name, "log_n": LOG_N, "width": width, "op": "variants", "matrix_passes": pl.matrix_passes(width),
           "steps": steps, "warmup": warmup}
    for k in routes:
        row[k + "_ms"] = round(med[k], 5)
        row[k + "_min_ms"] = round(min(ms[k]), 5)
        row[k + "_max_ms"] = round(max(ms[k]), 5)
    for k, plain in plain_of.items():
        row[k + "_over_plain"] = round(med[k] / med[plain], 3)
    row["launch_ms"] = launches
    print("ROW " + json.dumps(row), flush=True)


def child(name, fid, width, steps, warmup, with_variants=True):
    import torch

    from ntt_amd.fields import field_params
    from ntt_amd.ntt import NTTPlan
    p, g = field_params(fid)
    pl = NTTPlan(fid, LOG_N, 1)
    N, n_in, eb = pl.n, pl.n >> 1, pl.elem_bytes
    # seeded canonical elements: the plan's own fill, repeated over the columns with a per-column rotation
    base = pl.fill(pl.empty(), "random", seed=11)
    cols = torch.stack([torch.roll(base, b) for b in range(width)])  # [W][N], the batched layout
    x_rows = cols.t().contiguous()                                   # [N][W], row-major
    for op in ("forward", "lde"):
        rows_in = N if op == "forward" else n_in
        src_rows = x_rows[:rows_in].contiguous().view(-1)
        src_cols = cols[:, :rows_in].contiguous().view(-1)
        out_m, out_c, out_b = (torch.empty(N * width, dtype=pl.dtype, device="cuda:0") for _ in range(3))

        def run_matrix():
            if op == "forward":
                pl.forward_matrix(out_m, width)  # in place on whatever it holds: the time does not depend on the values
            else:
                pl.lde_matrix(src_rows, out_m, 1, g, width)

        def composed():
            t = src_rows.view(rows_in, width).t().contiguous().view(-1)
            if op == "forward":
                pl.forward_batch(t, width)
            else:
                pl.lde_batch(t, out_b, 1, g, width)
                t = out_b
            out_c.view(N, width).copy_(t.view(width, N).t())

        work_b = src_cols.clone()

        def batched():
            if op == "forward":
                pl.forward_batch(work_b, width)
            else:
                pl.lde_batch(src_cols, out_b, 1, g, width)

        if op == "forward":
            out_m.copy_(src_rows)
        run_matrix()
        composed()
        torch.cuda.synchronize()
        if not torch.equal(out_m, out_c):
            raise SystemExit(f"check: the matrix and composed routes disagree ({name}, W {width}, {op})")
        routes = {"matrix": run_matrix, "composed": composed, "batched": batched}
        for _ in range(warmup):
            for f in routes.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in routes}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(steps):
            for k, f in routes.items():
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        pl.set_profiling(True)
        run_matrix()
        torch.cuda.synchronize()
        launches = dict(zip(pl.last_launch_labels(), [round(v, 4) for v in pl.last_launch_ms()]))
        batched()
        torch.cuda.synchronize()
        launches_b = dict(zip(pl.last_launch_labels(), [round(v, 4) for v in pl.last_launch_ms()]))
        pl.set_profiling(False)
        med = {k: statistics.median(v) for k, v in ms.items()}
        passes = pl.matrix_passes(width)
        moved = 2 * len(passes) * N * width * eb - (0 if op == "forward" else (N - n_in) * width * eb)
        gbs = moved / (med["matrix"] * 1e-3) / 1e9
        row = {"field": name, "log_n": LOG_N, "width": width, "op": op, "matrix_passes": passes,
               "batched_passes": pl.passes, "steps": steps, "warmup": warmup,
               "matrix_ms": round(med["matrix"], 5), "matrix_min_ms": round(min(ms["matrix"]), 5),
               "matrix_max_ms": round(max(ms["matrix"]), 5),
               "composed_ms": round(med["composed"], 5), "composed_min_ms": round(min(ms["composed"]), 5),
               "composed_max_ms": round(max(ms["composed"]), 5),
               "batched_ms": round(med["batched"], 5), "batched_min_ms": round(min(ms["batched"]), 5),
               "batched_max_ms": round(max(ms["batched"]), 5),
               "composed_over_matrix": round(med["composed"] / med["matrix"], 3),
               "matrix_over_batched": round(med["batched"] / med["matrix"], 3),
               "matrix_bytes": moved, "matrix_gbs": round(gbs, 1),
               "matrix_hbm_frac": round(gbs / (HBM_COPY_TBS * 1e3), 3),
               "matrix_launch_ms": launches, "batched_launch_ms": launches_b}
        print("ROW " + json.dumps(row), flush=True)
    if with_variants:
        variants(pl, name, width, g, x_rows, steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix", "bench.jsonl"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-variants", action="store_true", help="only the plain rows (a library without the _ex calls)")
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: the median is taken over at least 20 steps")
    if a.child:
        name, fid, width = a.child
        child(name, int(fid), int(width), a.steps, a.warmup, not a.no_variants)
        return
    rows = []
    for name, fid, width in CASES:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--child", name, str(fid), str(width)] + (["--no-variants"] if a.no_variants else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-3000:], sep="\n")
            raise SystemExit(f"{name} W={width}: exit status {r.returncode}; stopping")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
