"""The Poseidon2 Merkle commitment (NTTPlan.merkle_commit) on one GPU against the static VALU cost of its
permutation: how close the leaf kernel comes to the vector ALU's issue rate.  A copy's bandwidth is no
yardstick here: a permutation is thousands of vector instructions per 32 absorbed bytes.

Two steps.

    python tools/bench_merkle.py --static      (no GPU: needs hipcc)
compiles ntt_e31_hash.hip and ntt_eg_hash.hip to assembly and counts the vector instructions of
k_p2_permute<E, degree>: its three round loops are single basic blocks that branch to themselves (first
external half, internal rounds, second external half), so
    VALU per permutation = outside the loops + first * rounds_f / 2 + internal * rounds_p + second * rounds_f / 2.
`issue_cycles` weighs each instruction by its measured issue cost on one SIMD (2 cycles for the
VOP2 forms, 4 for v_mul_lo/hi_u32, v_mad_u64_u32, the 64-bit and the other VOP3-only forms).  The counts go to
profiles/merkle/static_valu.json.

    python tools/bench_merkle.py [--out profiles/merkle/bench.jsonl]
times, at 2^20 rows x widths 16, 64 and 256 on BabyBear and Goldilocks with seeded random parameters at the
usual round counts (fields.POSEIDON2_SHAPES): the whole commit between two device events, its launches by label
(the plan's profiling events: h the leaves, m1 a layer, m9 the tail), and a permute of 2^20 states.  From the
leaf launch: permutations per second, and the fraction of the VALU peak the static count implies,
    permutations / s * issue_cycles / (1024 SIMDs * 64 lanes * clock),
at the nominal 2.4 GHz (the clock under this load is not measured here, so the fraction is a lower bound
where the chip holds its clock down).  Every case runs in a fresh child process under its own `timeout -k 10`,
--warmup untimed commits, then the median of --steps (at least 20); the driver stops at the first that fails.
Before the timing the root must equal the root of a second commit, and the tree's first leaf the permute of the
first row's chunks done through poseidon2_permute.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_ROWS = 20
CASES = [(name, fid, w) for name, fid in (("babybear", 4), ("goldilocks", 3)) for w in (16, 64, 256)]
STATIC = os.path.join(ROOT, "profiles", "merkle", "static_valu.json")
SIMDS, LANES, CLOCK_HZ = 1024, 64, 2.4e9
FOUR_CYCLE = re.compile(r"^v_(mul_lo_u32|mul_hi_u32|mad_u64_u32|lshl_add_u64|lshlrev_b64|lshrrev_b64|add3_u32|"
                        r"add_co_u32|addc_co_u32|sub_co_u32|subb_co_u32|\w+_e64)$")


def static_counts():
    from ntt_amd import build as B
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for eng, src in (("Eng31", "ntt_e31_hash.hip"), ("Eng64G", "ntt_eg_hash.hip")):
            asm = os.path.join(tmp, src + ".s")
            cmd = [B.hipcc(), "-O3", "-std=c++17", f"--offload-arch={B.ARCH}", "--cuda-device-only", "-S",
                   os.path.join(B.CSRC, src), "-o", asm, "-I", B.CSRC, "-I", B.INCLUDE, "-Wno-pass-failed"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-3000:])
            with open(asm) as f:
                text = f.read()
            for m in re.finditer(r"^(_ZN3ntt12k_p2_permuteINS_\d+(\w+?)ELi(\d)E\w+):.*?\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
                engine, degree, body = m.group(2), int(m.group(3)), m.group(4)
                parts = re.split(r"^(\.LBB\d+_\d+):.*$", body, flags=re.M)
                labels, texts = ["entry"] + parts[1::2], [parts[0]] + parts[2::2]
                loops, outside, outside_cyc = [], 0, 0
                for label, t in zip(labels, texts):
                    ins = re.findall(r"^\s+(v_\w+)", t, re.M)
                    cyc = sum(4 if FOUR_CYCLE.match(i) else 2 for i in ins)
                    if label in re.findall(r"^\s+s_cbranch\w*\s+(\.LBB\d+_\d+)", t, re.M):
                        loops.append((len(ins), cyc))
                    else:
                        outside += len(ins)
                        outside_cyc += cyc
                if len(loops) != 3:
                    raise SystemExit(f"{engine} degree {degree}: {len(loops)} self-loops, expected the three round loops")
                out[f"{engine}/{degree}"] = {"outside": [outside, outside_cyc], "external_first": list(loops[0]),
                                             "internal": list(loops[1]), "external_second": list(loops[2])}
    return out


def per_permutation(counts, engine, degree, rounds_f, rounds_p):
    c = counts[f"{engine}/{degree}"]
    return tuple(c["outside"][k] + (c["external_first"][k] + c["external_second"][k]) * (rounds_f // 2) +
                 c["internal"][k] * rounds_p for k in (0, 1))


def child(name, fid, width, steps, warmup):
    import random

    import torch

    from ntt_amd.fields import POSEIDON2_SHAPES, field_params
    from ntt_amd.ntt import NTTPlan
    p, _ = field_params(fid)
    t, alpha, rf, rp = POSEIDON2_SHAPES[fid]
    d = t // 2
    rng = random.Random(1234 + fid)
    pl = NTTPlan(fid, LOG_ROWS, 1)
    pl.set_poseidon2(alpha, rf, rp, [[rng.randrange(p) for _ in range(t)] for _ in range(rf)],
                     [rng.randrange(p) for _ in range(rp)], [rng.randrange(p) for _ in range(t)])
    N, dev = pl.n, "cuda:0"
    base = pl.fill(pl.empty(), "random", seed=11)
    mat = torch.empty(N * width, dtype=pl.dtype, device=dev).view(N, width)
    for b in range(width):
        mat[:, b] = torch.roll(base, 17 * b)
    mat = mat.view(-1)
    tree = torch.empty((2 * N - 1) * d, dtype=pl.dtype, device=dev)
    states = pl.fill(pl.empty(), "random", seed=12).repeat(t)[:N * t].contiguous()
    pl.merkle_commit(mat, width, tree)
    torch.cuda.synchronize()
    first = tree.clone()
    pl.merkle_commit(mat, width, tree)
    torch.cuda.synchronize()
    if not torch.equal(first, tree):
        raise SystemExit(f"check: two commits differ ({name}, width {width})")
    s = torch.zeros(t, dtype=pl.dtype, device=dev)
    for c in range(0, width, d):
        s[:d] = mat[c:c + d]
        pl.poseidon2_permute(s)
    if not torch.equal(s[:d], tree[:d]):
        raise SystemExit(f"check: leaf 0 is not the sponge of row 0 ({name}, width {width})")

    for _ in range(warmup):
        pl.merkle_commit(mat, width, tree)
        pl.poseidon2_permute(states)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    commit_ms, permute_ms = [], []
    for _ in range(steps):
        e0.record()
        pl.merkle_commit(mat, width, tree)
        e1.record()
        torch.cuda.synchronize()
        commit_ms.append(e0.elapsed_time(e1))
        e0.record()
        pl.poseidon2_permute(states)
        e1.record()
        torch.cuda.synchronize()
        permute_ms.append(e0.elapsed_time(e1))
    pl.set_profiling(True)
    for _ in range(steps):
        pl.merkle_commit(mat, width, tree)
    by_label = {}
    for lab, ms in zip(pl.last_launch_labels(), pl.last_launch_ms()):  # averaged over the recorded commits
        by_label[lab] = round(by_label.get(lab, 0.0) + ms, 5)
    pl.set_profiling(False)

    dg, elems, launches, tail = pl.merkle_info(width)
    leaf_perms = N * ((width + d - 1) // d)
    row = {"field": name, "log_rows": LOG_ROWS, "width": width, "t": t, "sbox_degree": alpha, "rounds_f": rf, "rounds_p": rp,
           "launches": launches, "tail_log": tail, "steps": steps, "warmup": warmup,
           "commit_ms": round(statistics.median(commit_ms), 5), "commit_min_ms": round(min(commit_ms), 5),
           "commit_max_ms": round(max(commit_ms), 5), "ms_by_label": by_label,
           "permutations": leaf_perms + N - 1, "leaf_permutations": leaf_perms,
           "permute_states": N, "permute_ms": round(statistics.median(permute_ms), 5)}
    row["permute_per_s"] = round(N / (row["permute_ms"] * 1e-3))
    if by_label.get("h"):
        row["leaf_permutations_per_s"] = round(leaf_perms / (by_label["h"] * 1e-3))
    if os.path.exists(STATIC):
        with open(STATIC) as f:
            valu, cyc = per_permutation(json.load(f), "Eng31" if pl.elem32 else "Eng64G", alpha, rf, rp)
        peak = SIMDS * LANES * CLOCK_HZ / cyc  # permutations per second at the issue rate
        row.update(static_valu_per_permutation=valu, static_issue_cycles_per_permutation=cyc,
                   peak_permutations_per_s=round(peak), permute_fraction_of_valu_peak=round(row["permute_per_s"] / peak, 3))
        if "leaf_permutations_per_s" in row:
            row["leaf_fraction_of_valu_peak"] = round(row["leaf_permutations_per_s"] / peak, 3)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "bench.jsonl"))
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--static", action="store_true", help="count the permutation's vector instructions (no GPU)")
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.static:
        counts = static_counts()
        os.makedirs(os.path.dirname(STATIC), exist_ok=True)
        with open(STATIC, "w") as f:
            f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(counts[k], sort_keys=True)}' for k in sorted(counts)) + "\n}")
            f.write("\n")
        for key in sorted(counts):
            print(key, counts[key])
        print(f"wrote {STATIC}")
        return
    if a.child:
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
