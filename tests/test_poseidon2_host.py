"""ntt_amd/csrc/poseidon2.hpp on the host: tests/c/poseidon2_check.cpp, a stand-alone program built with
-fsanitize=address,undefined, runs the header's permutation, sponge and compression -- the text the Merkle
kernels run -- against tests/golden/poseidon2_vectors.json (canonical and Montgomery-form data), and checks the
two algebraic pins (M_E is circ(2 M4, M4, ..); two degree-3 rounds written out).  The golden file is the integer
oracle's (tests/poseidon2_ref.py): it is regenerated here and compared, and the oracle's numpy path, which the
GPU tests use at their shapes, is held to its integer path."""
import json
import os
import random
import shutil
import subprocess

import numpy as np

from tests import poseidon2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "poseidon2_vectors.json")


def _host_compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and (shutil.which(cand) or os.path.exists(cand)):
            return cand
    return None


def _tokens(golden) -> str:
    out = [len(golden)]
    for case in golden.values():
        P = R.Params.from_dict(case["params"])
        out += [P.p, P.t, P.alpha, P.rounds_f, P.rounds_p] + P.flat_ext() + P.int_rc + P.int_diag
        out.append(len(case["states"]))
        for s in case["states"]:
            out += s["in"] + s["out"]
        out.append(len(case["rows"]))
        for r in case["rows"]:
            out += [len(r["row"])] + r["row"] + r["digest"]
        leaves = case["tree"]["rows"]
        out += [len(leaves), len(leaves[0])] + [v for r in leaves for v in r] + [v for n in case["tree"]["nodes"] for v in n]
    return " ".join(str(v) for v in out) + "\n"


def test_golden_vectors_are_the_oracles():
    with open(GOLDEN) as f:
        assert json.load(f) == R.golden()


def test_header_matches_the_golden_vectors_and_the_pins(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler found (g++, c++, clang++)"
    with open(GOLDEN) as f:
        golden = json.load(f)
    tokens = tmp_path / "tokens.txt"
    tokens.write_text(_tokens(golden))
    exe = str(tmp_path / "poseidon2_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "ntt_amd", "csrc"), os.path.join(ROOT, "tests", "c", "poseidon2_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(tokens)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert f"poseidon2_check: ok ({len(golden)} cases)" in r.stdout


def test_the_oracles_numpy_path_is_its_integer_path():
    for name, p, t, alpha, rf, rp, seed in R.GOLDEN_FIELDS:
        P = R.seeded_params(p, t, alpha, rf, rp, seed)
        rng = random.Random(seed + 7)
        states = [[0] * t, [p - 1] * t] + [[rng.randrange(p) for _ in range(t)] for _ in range(12)]
        got = R.permute_many(np.array(states, dtype=np.uint64), P)
        assert [[int(v) for v in r] for r in got] == [R.permute(s, P) for s in states], name
        for w in (1, P.d + 1, 2 * P.d + 3):
            mat = [[rng.randrange(p) for _ in range(w)] for _ in range(8)]
            got = R.tree_many(np.array(mat, dtype=np.uint64), P)
            assert [[int(v) for v in r] for r in got] == R.tree(mat, P), (name, w)


def test_m_ext_is_the_circulant():
    rng = random.Random(3)
    for p, t in ((0x78000001, 16), (R._GL, 8)):
        s = [rng.randrange(p) for _ in range(t)]
        M = R.m_ext_matrix(t)
        assert R.m_ext(s, p) == [sum(M[i][j] * s[j] for j in range(t)) % p for i in range(t)]
