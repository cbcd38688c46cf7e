"""The pure helpers the plan's parts share (ntt_amd/csrc/plan_schedule.hpp: mid_digits, overlaps, and the
prover-stage calls' degree_ok, fits32, aligned16), checked on the host: tests/c/plan_pure_check.cpp prints the
final pass's middle digits for every schedule of three or more passes in tests/golden/schedule_table.txt, then
overlaps() on edge values (touching ranges, one shared byte, containment, empty ranges), then the three
predicates on theirs (degrees 0, 1, 2, 3, 4, 8; width 0, log_rows 31 and 32, width << log_rows at 2^32 - 1
and 2^32; a pointer at offset 8 among aligned ones).  The output must equal
tests/golden/plan_pure_table.txt, whose middle-digit lines were printed once by the two loops as they
stood in ntt_plan.cpp (pass_args and the matrix transforms) before they became one function, and whose
overlaps lines are the comparison a0 < b1 && b0 < a1 that the three call sites spelled out; the predicates'
lines were written down by hand and are recomputed below from the predicates' definitions.  The same
program built with -fsanitize=address,undefined prints the same table (its own main: nothing is
preloaded).  The host-words -> canonical-element helper (HostField::canonical) needs the kernels'
headers and is covered by the GPU tests of the coset, matrix and fold calls' argument checks."""
import os
import subprocess

import pytest

from test_schedule_host import SAN, _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "plan_pure_check.cpp")
SCHEDULES = os.path.join(ROOT, "tests", "golden", "schedule_table.txt")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_pure_table.txt")


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_plan_pure_table_unchanged(variant, tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler found (g++, c++, clang++)")
    exe = str(tmp_path / f"plan_pure_check_{variant}")
    cmd = [cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ntt_amd", "csrc"), SRC, "-o", exe]
    if variant == "sanitized":
        probe = str(tmp_path / "probe")
        r = subprocess.run([cxx, *SAN, "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
        if r.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
            pytest.skip(f"{cxx} cannot link -fsanitize=address,undefined: {r.stderr.strip()[-300:]}")
        cmd[1:1] = SAN
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, SCHEDULES], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    with open(GOLDEN) as f:
        exp = f.read()
    got = r.stdout
    if got != exp:
        g, e = got.splitlines(), exp.splitlines()
        diff = [(i + 1, a, b) for i, (a, b) in enumerate(zip(g, e)) if a != b][:10]
        pytest.fail(f"table differs from {GOLDEN}: {len(g)} lines against {len(e)}; first differences: {diff}")
    # every middle-digit line: the widths are the schedule's middle radices, most significant pass last,
    # the offsets their running sum from pass 2 on, and nothing is written past them
    mids = [l.split() for l in got.splitlines() if " bits " in l]
    assert len(mids) > 500
    for w in mids:
        bits = [int(x) for x in w[w.index("bits") + 1:w.index("off")]]
        off = [int(x) for x in w[w.index("off") + 1:w.index("rest")]]
        assert w[w.index("rest") + 1:] == ["0", "0"], w
        mid = bits[::-1]  # r_2 .. r_{p-1}
        assert off[::-1] == [sum(mid[:i]) for i in range(len(mid))], w
    # the predicates, from their definitions: an element has degree 1, 2 or 4; a [2^log_rows][width] matrix is
    # not empty and holds fewer than 2^32 elements; every pointer given (-1: none) is a multiple of 16
    rows = {k: [[int(x) for x in l.split()[1:]] for l in got.splitlines() if l.startswith(k + " ")]
            for k in ("degree_ok", "fits32", "aligned16")}
    assert [r[0] for r in rows["degree_ok"]] == [0, 1, 2, 3, 4, 8]
    for d, ok in rows["degree_ok"]:
        assert ok == (d in (1, 2, 4)), (d, ok)
    shapes = {(w, lr) for w, lr, _ in rows["fits32"]}
    assert {(0, 0), (1, 31), (1, 32), (2**32 - 1, 0), (2**31, 1), (2**16, 16)} <= shapes
    for w, lr, ok in rows["fits32"]:
        assert ok == (w >= 1 and (w << lr) < 2**32), (w, lr, ok)
    assert [8, 16, 32, 0] in rows["aligned16"] and [0, 16, 8, 0] in rows["aligned16"]
    for *offs, ok in rows["aligned16"]:
        assert ok == all(o % 16 == 0 for o in offs if o >= 0), (offs, ok)
