"""The single-launch schedules' host arithmetic (ntt_amd/csrc/plan_fused.hpp, the text the plans run) checked
on the host: tests/c/fused_layout_check.cpp prints the geometry of every radix triple the fused kernels are
instantiated for (7 out of place, 3 in place) at its natural size, in modes 0 and 1, with room for fewer and
for more workgroups than tiles, and the sync-word layout of the forms with 1 .. 4 grid barriers.  The output
must equal tests/golden/fused_layout_table.txt, which was printed once by the formulas as they stood in
ntt_plan.cpp before they moved into the header.  The offsets the kernels and the plan once spelled as
literals are asserted outright.  The same program built with -fsanitize=address,undefined prints the same
table (its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

from test_schedule_host import SAN, _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "fused_layout_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_layout_table.txt")
TILE_LOG = 10  # Eng256
TRIPLES = [(6, 6, 6), (7, 6, 6), (7, 7, 6), (7, 7, 7), (8, 7, 7), (8, 8, 7), (8, 8, 8)]  # k_fused3, k_fused3b
TRIPLES_IP = [(6, 6, 6), (6, 7, 6), (7, 6, 7)]  # k_fused3bi

_exe = {}


def _build(variant, tmp_path_factory):
    """The check program, plain or sanitized; (path, None) or (None, reason it could not be linked)."""
    if variant not in _exe:
        cxx = _host_compiler()
        if cxx is None:
            pytest.fail("no host C++ compiler found (g++, c++, clang++)")
        exe = str(tmp_path_factory.mktemp("flayout") / f"fused_layout_check_{variant}")
        cmd = [cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ntt_amd", "csrc"), SRC, "-o", exe]
        if variant == "sanitized":
            probe = str(tmp_path_factory.mktemp("flayoutp") / "probe")
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


def _fields(line):
    """'name k v k v ...: k v v k v ...' -> {k: [v, ...]} (go has several values; words before the first
    key are dropped)."""
    out, key = {}, None
    for w in line.replace(":", " ").split()[1:]:
        if w.isdigit():
            if key is not None:
                out[key].append(int(w))
        else:
            key = w
            out[key] = []
    return out


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_fused_layout_table_unchanged(variant, tmp_path_factory):
    exe, why = _build(variant, tmp_path_factory)
    if exe is None:
        pytest.skip(why)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    args = [str(TILE_LOG)] + [":".join(map(str, t)) for t in TRIPLES + TRIPLES_IP]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    got = r.stdout
    with open(GOLDEN) as f:
        exp = f.read()
    if got != exp:
        g, e = got.splitlines(), exp.splitlines()
        diff = [(i + 1, a, b) for i, (a, b) in enumerate(zip(g, e)) if a != b][:10]
        pytest.fail(f"fused layout table differs from {GOLDEN}: {len(g)} lines against {len(e)}; first differences "
                    f"(line, got, expected): {diff}")
    lines = got.splitlines()
    geom = [ln for ln in lines if ln.startswith("geom ")]
    assert len(geom) == (len(TRIPLES) + len(TRIPLES_IP)) * 4 and not any("REFUSED" in ln for ln in geom)
    for ln in geom:
        r1, r2, r3 = (int(x) for x in ln.split()[1:4])
        f = {k: v[0] for k, v in _fields(ln).items()}
        assert f["tiles"] == 1 << (r1 + r2 + r3 - TILE_LOG) and f["nwg"] == min(f["tiles"], f["cap"]), ln
        # every pass-1 tile is counted in exactly once, and every pass-2 tile
        assert f["n12"] * f["need12"] == f["tiles"] and f["n23"] * f["need23"] == f["tiles"], ln
        # the counters fit below the ready lines; abort and shard lines follow the last ready line
        assert f["rbase"] % 32 == 0 and 4 + f["n12"] + f["n23"] <= f["rbase"], ln
        assert f["abort"] == f["rbase"] + 32 * (f["n12"] + f["n23"]) and f["shards"] == f["abort"] + 32, ln
        assert f["total"] == f["shards"] + 32 * 8, ln
    # the literals of the barrier forms: total / abort / shards, and the final barrier's go word
    bar = {int(ln.split()[1].rstrip(":")): _fields(ln) for ln in lines if ln.startswith("barriers ")}
    assert sorted(bar) == [1, 2, 3, 4]
    three, four = bar[3], bar[4]
    assert (three["total"], three["abort"], three["shards"]) == ([416], [128], [160])
    assert (four["total"], four["abort"], four["shards"]) == ([448], [160], [192])
    assert three["rbase"] == four["rbase"] == [32]
    assert three["go"][-1] == three["rbase"][0] + 64 and four["go"][-1] == four["rbase"][0] + 96
    for k, f in bar.items():
        assert f["go"] == [32 * (1 + i) for i in range(k)], (k, f)
