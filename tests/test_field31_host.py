"""The one-word arithmetic of ntt_amd/csrc/field31.hpp (the text the Eng31 kernels run) checked on the
host: tests/c/field31_check.cpp compares add, sub, the twiddle product with its precomputed companion,
the variable product and canonicalisation with uint64_t arithmetic mod p, and asserts every documented
intermediate bound, for BabyBear, KoalaBear, the 30-bit 1004535809 and 3: the edge set's cross product
and 10^6 seeded random pairs each."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and (shutil.which(cand) or os.path.exists(cand)):
            return cand
    return None


def test_field31_matches_uint64_arithmetic(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler found (g++, c++, clang++)")
    exe = str(tmp_path / "field31_check")
    cmd = [cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ntt_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "field31_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "field31_check: ok" in r.stdout
