"""The batch inverse and the column scans (NTTPlan.batch_inverse, matrix_scan) on one GPU against a
device-to-device copy that moves the same bytes, the yardstick of DESIGN.md section 4.2.

  inverse: reads and writes count d elements: 2 count d elem_bytes of traffic.  Its three ways of sharing an
           inversion (NTT_INV_FORM 0: a run of 16 words per thread, 1: of 32, 2: one inversion per wave behind a
           cross-lane product scan) are timed interleaved in one process and compared bit for bit first.
  scan:    three launches move the matrix three times (two reads, one write): 3 rows width d elem_bytes.

Cases: BabyBear and Goldilocks, d = 1 and the field's extension degree, 2^20 and 2^22 elements / rows, the scans
at width 1 (the narrow layout) and at a width of several strips, sum and product.  Every route of a case is timed
in ONE process, interleaved step by step with its copy, each step one call between two device events; the figure
is the median of `--steps` steps (at least 20) after `--warmup` untimed ones.

Every case runs as a child process under its own `timeout -k 10`; the driver stops at the first that fails.

    python tools/bench_scan.py [--out profiles/scan/bench.jsonl] [--quick]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = (("babybear", 4), ("goldilocks", 3))
WIDE = 40  # columns of the wide scan cases: several strips at every element size


def cases(quick):
    logs = (20,) if quick else (20, 22)
    out = []
    for name, fid in FIELDS:
        for ext in (False, True):
            for log in logs:
                out.append(("inverse", name, fid, int(ext), log, 1, "-"))
                for op in ("sum", "product"):
                    out.append(("scan", name, fid, int(ext), log, 1, op))
                    out.append(("scan", name, fid, int(ext), log - 5, WIDE, op))  # the same order of bytes
    return out


def child(kind, name, fid, ext, log, width, op, steps, warmup):
    import torch

    from ntt_amd.fields import EXTENSIONS, field_params
    from ntt_amd.ntt import NTTPlan
    p, _ = field_params(fid)
    d, w = EXTENSIONS[fid] if ext else (1, 0)
    pl = NTTPlan(fid, 10, 1)
    rows, eb = 1 << log, pl.elem_bytes
    n = rows * width * d
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    if pl.elem32:
        x = torch.randint(1, p, (n,), generator=gen, device="cuda:0", dtype=torch.int64).to(torch.int32)
    else:
        x = torch.randint(1, 1 << 62, (n,), generator=gen, device="cuda:0", dtype=torch.int64)  # canonical: below p
    passes = 2 if kind == "inverse" else 3
    traffic = passes * n * eb
    c_src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda:0")
    c_dst = torch.empty_like(c_src)
    routes = {}
    if kind == "inverse":
        outs = {f: torch.empty_like(x) for f in range(3)}

        def inv(form):
            os.environ["NTT_INV_FORM"] = str(form)
            pl.batch_inverse(x, outs[form], ext_degree=d, ext_w=w)

        for f in range(3):
            inv(f)
        torch.cuda.synchronize()
        if not (torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])):
            raise SystemExit(f"check: the inverse's forms disagree ({name}, d={d})")
        routes = {f"form{f}": (lambda f=f: inv(f)) for f in range(3)}
    else:
        out, tot = torch.empty_like(x), torch.empty(width * d, dtype=pl.dtype, device="cuda:0")
        routes = {"scan": lambda: pl.matrix_scan(x, out, width, op=op, totals=tot, ext_degree=d, ext_w=w, rows=rows)}
    routes["copy"] = lambda: c_dst.copy_(c_src)
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
    row = {"call": kind, "field": name, "ext_degree": d, "log_rows": log, "width": width, "op": op,
           "traffic_bytes": traffic, "steps": steps, "warmup": warmup}
    if kind == "scan":
        row["info"] = list(pl.scan_info(rows, width, op=op, ext_degree=d))
    for r in routes:
        row[r + "_ms"] = round(med[r], 5)
        row[r + "_min_ms"] = round(min(ms[r]), 5)
        row[r + "_max_ms"] = round(max(ms[r]), 5)
        if r != "copy":
            row[r + "_over_copy"] = round(med[r] / med["copy"], 3)
            row[r + "_gelems"] = round(n / d / (med[r] * 1e-3) / 1e9, 3)
    row["copy_gbs"] = round(traffic / (med["copy"] * 1e-3) / 1e9, 1)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan", "bench.jsonl"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="2^20 only")
    ap.add_argument("--child", nargs=7, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("--steps: the median is taken over at least 20 steps")
    if a.child:
        kind, name, fid, ext, log, width, op = a.child
        child(kind, name, int(fid), int(ext), int(log), int(width), op, a.steps, a.warmup)
        return
    rows = []
    for c in cases(a.quick):
        cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--child", *[str(v) for v in c]]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-3000:], sep="\n")
            raise SystemExit(f"{c}: exit status {r.returncode}; stopping")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
