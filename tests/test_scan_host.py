"""The scan calls' host side without a device: the integer oracle (tests/scan_ref.py) against itertools.accumulate
on small cases, and ntt_amd/csrc/scan_shape.hpp -- the shape decisions the launcher, the kernels and ntt_scan_info
share -- swept by tests/c/scan_shape_check.cpp, a stand-alone program built with -fsanitize=address,undefined."""
import itertools
import os
import random
import subprocess

import numpy as np

from tests import scan_ref as R
from tests.test_gpu_fold import _ext_mul
from tests.test_poseidon2_host import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BABYBEAR, GOLDILOCKS = 2013265921, (1 << 64) - (1 << 32) + 1


def test_the_oracles_scans_are_itertools_accumulate():
    rng = random.Random(5)
    for p, d, w in ((BABYBEAR, 1, None), (BABYBEAR, 4, 11), (GOLDILOCKS, 2, 7)):
        for rows, width in ((1, 1), (2, 3), (7, 2), (19, 5)):
            mat = np.array([[rng.randrange(p) for _ in range(width * d)] for _ in range(rows)], dtype=np.uint64)
            mat[rows // 2, :d] = 0  # a zero element in column 0
            for op in ("sum", "product"):
                inc, exc, tot = R.scan(mat, width, d, w, p, op)
                for j in range(width):
                    col = [[int(v) for v in mat[r, j * d:(j + 1) * d]] for r in range(rows)]
                    one = [1 if op == "product" and k == 0 else 0 for k in range(d)]
                    f = (lambda a, b: [(x + y) % p for x, y in zip(a, b)]) if op == "sum" else (lambda a, b: _ext_mul(a, b, w, p))
                    want = list(itertools.accumulate(col, f))
                    assert [[int(v) for v in inc[r, j * d:(j + 1) * d]] for r in range(rows)] == want, (p, d, op, rows, width, j)
                    assert [[int(v) for v in exc[r, j * d:(j + 1) * d]] for r in range(rows)] == [one] + want[:-1]
                    assert [int(v) for v in tot[j * d:(j + 1) * d]] == want[-1]
                if d == 1 and width == 1:
                    i1, e1, t1 = R.scan_one_column([int(v) for v in mat[:, 0]], p, op)
                    assert i1 == [int(v) for v in inc[:, 0]] and e1 == [int(v) for v in exc[:, 0]] and t1 == int(tot[0])


def test_the_oracles_inverse():
    rng = random.Random(6)
    for p, d, w in ((BABYBEAR, 1, None), (BABYBEAR, 4, 11), (GOLDILOCKS, 2, 7)):
        xs = [[rng.randrange(p) for _ in range(d)] for _ in range(6)] + [[0] * d, [1] + [0] * (d - 1), [p - 1] * d]
        ys = [R.ext_inverse(x, w, p) for x in xs]
        for x, y in zip(xs, ys):
            assert (y == [0] * d) if not any(x) else (_ext_mul(x, y, w, p) == [1] + [0] * (d - 1)), (p, d, x)
        assert R.is_inverse(np.array(xs, dtype=np.uint64), np.array(ys, dtype=np.uint64), d, w, p)
        ys[0][0] ^= 1
        assert not R.is_inverse(np.array(xs, dtype=np.uint64), np.array(ys, dtype=np.uint64), d, w, p)


def test_shape_header_keeps_its_invariants(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler found (g++, c++, clang++)"
    exe = str(tmp_path / "scan_shape_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "ntt_amd", "csrc"), os.path.join(ROOT, "tests", "c", "scan_shape_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "scan_shape_check: ok" in r.stdout
