"""The radix scheduler of ntt_amd/csrc/plan_schedule.hpp (the text the plans run) checked on the host:
tests/c/schedule_check.cpp prints the pass radices of every size 2^0 .. 2^40 for each engine's parameters,
and the palindromic schedule of the in-place plans; the output must equal tests/golden/schedule_table.txt,
which was printed once by the scheduler functions as they stood in ntt_plan.cpp before they moved into
the header.  Three runs: NTT_SCHEDULE unset, set to a sequence every engine accepts (6,8,8 at 2^22), and
set to one every engine rejects (3,9,3: radix 9 is out of range on the 1024-element tiles, r_1 + r_p = 6
is below every tile elsewhere; a set NTT_SCHEDULE still switches Eng31's preferred column width off).
Every emitted sequence must sum to log_n and satisfy schedule_ok; palindrome rows must read the same
both ways.  The same program built with -fsanitize=address,undefined prints the same table (its own
main: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "schedule_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "schedule_table.txt")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
# (TILE_LOG, MIN_COLS_LOG, preferred columns log2, NARROW_FIRST, in-place plans exist) per engine:
# engines.hpp with its NTT_* default macros (NTT_TILE_LOG_256 10, NTT_TILE_LOG_P 13, NTT_MIN_COLS_LOG_P 4,
# NTT_P_NARROW_FIRST 1, NTT_TILE_LOG_G 12, NTT_TILE_LOG_31 13, NTT_MIN_COLS_LOG_31 4, NTT_PREF_COLS_LOG_31 5)
ENGINES = [
    ("Eng256", 10, 2, 2, 0, 1),    # Eng29<9, 8>
    ("Eng384", 10, 2, 2, 0, 1),    # Eng29<14, 12>
    ("Eng256w", 10, 2, 2, 0, 0),   # Eng29<9, 12>; its in-place plans are Eng256wI's
    ("Eng256wI", 10, 2, 2, 0, 1),  # Eng29<9, 12, 12>
    ("Eng256T", 12, 0, 0, 0, 1),   # Eng29<9, 8, 0, 12>: 4096-element tiles, one column per tile allowed
    ("EngP", 13, 4, 4, 1, 0),      # Eng32<1, 2>; its in-place plans are EngPI's
    ("EngPI", 13, 4, 4, 1, 1),     # Eng32<1, 2, 2>
    ("Eng64G", 12, 4, 4, 1, 0),    # Goldilocks: no in-place plans
    ("Eng31", 13, 4, 5, 1, 0),     # prefers 32-column groups; no in-place plans
]
FORCED = [None, "6,8,8", "3,9,3"]  # unset, accepted, rejected


def _host_compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and (shutil.which(cand) or os.path.exists(cand)):
            return cand
    return None


_exe = {}


def _build(variant, tmp_path_factory):
    """The check program, plain or sanitized; (path, None) or (None, reason it could not be linked)."""
    if variant not in _exe:
        cxx = _host_compiler()
        if cxx is None:
            pytest.fail("no host C++ compiler found (g++, c++, clang++)")
        exe = str(tmp_path_factory.mktemp("sched") / f"schedule_check_{variant}")
        cmd = [cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ntt_amd", "csrc"), SRC, "-o", exe]
        if variant == "sanitized":
            probe = str(tmp_path_factory.mktemp("schedp") / "probe")
            r = subprocess.run([cxx, *SAN, "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                               capture_output=True, text=True)
            if r.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
                _exe[variant] = (None, f"{cxx} cannot link -fsanitize=address,undefined: {r.stderr.strip()[-300:]}")
                return _exe[variant]
            cmd[1:1] = SAN
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _exe[variant] = (exe, None)
    return _exe[variant]


def _table(exe):
    out = []
    for forced in FORCED:
        env = {k: v for k, v in os.environ.items() if k != "NTT_SCHEDULE"}
        env.update(ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        if forced is not None:
            env["NTT_SCHEDULE"] = forced
        r = subprocess.run([exe] + [":".join(map(str, e)) for e in ENGINES], capture_output=True, text=True,
                           timeout=120, env=env)
        assert r.returncode == 0 and not r.stderr.strip(), (forced, r.returncode, r.stderr[-3000:])
        out.append(r.stdout)
    return "".join(out)


def _schedule_ok(r, tile_log):
    """schedule_ok of plan_schedule.hpp: r_1 + r_p >= tile_log and every column pass's block spans a tile."""
    if len(r) < 2:
        return True
    return r[0] + r[-1] >= tile_log and all(sum(r[i:]) >= tile_log for i in range(len(r) - 1))


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_schedule_table_unchanged(variant, tmp_path_factory):
    exe, why = _build(variant, tmp_path_factory)
    if exe is None:
        pytest.skip(why)
    got = _table(exe)
    with open(GOLDEN) as f:
        exp = f.read()
    if got != exp:
        g, e = got.splitlines(), exp.splitlines()
        diff = [(i + 1, a, b) for i, (a, b) in enumerate(zip(g, e)) if a != b][:10]
        pytest.fail(f"schedule table differs from {GOLDEN}: {len(g)} lines against {len(e)}; first differences "
                    f"(line, got, expected): {diff}")
    # the properties of every emitted sequence
    params = {e[0]: e for e in ENGINES}
    seen = {name: 0 for name in params}
    engines_listed, forced_seen = [], []
    for line in got.splitlines():
        w = line.split()
        if w[0] == "#":
            forced_seen.append(w[1].split("=", 1)[1] or None)
            continue
        if w[0] == "engine":
            assert tuple(w[1:2] + [int(x) for x in w[2:]]) == params[w[1]], line
            engines_listed.append(w[1])
            continue
        name, kind, log_n = w[0], w[1], int(w[2])
        _, tile_log, min_cols, pref_cols, _, pal = params[name]
        assert w[3:] not in (["FAIL"], ["NONE"]) or kind == "pal", line  # every size has a schedule
        if w[3:] == ["NONE"]:
            continue
        r = [int(x) for x in w[3:]]
        seen[name] += 1
        if kind == "sched":
            if log_n <= 2:
                assert r == [], line  # the naive kernel
            elif log_n <= tile_log:
                assert r == [log_n], line
            else:
                rmax = tile_log - min_cols
                assert len(r) >= 2 and sum(r) == log_n and all(3 <= x <= rmax for x in r), line
        else:
            assert kind == "pal" and pal and len(r) >= 2 and sum(r) == log_n, line
            assert all(r[i] == r[len(r) - 1 - i] for i in range(len(r))), line
            assert all(3 <= x <= tile_log - min_cols for x in r), line
        assert _schedule_ok(r, tile_log), line
    assert forced_seen == FORCED
    assert engines_listed == [e[0] for e in ENGINES] * len(FORCED)
    assert all(c >= 41 * len(FORCED) for c in seen.values()), seen
    # the forced sequence is taken where accepted (2^22) and nowhere in the rejected run
    assert f"# NTT_SCHEDULE=6,8,8\n" in got and got.count(" sched 22 6 8 8\n") == len(ENGINES)
    assert " 3 9 3\n" not in got
