"""The binomial-extension arithmetic of ntt_amd/csrc/fieldext.hpp (the text the FRI fold kernel runs) checked
on the host: tests/c/fieldext_check.cpp compares the product in F_p[X]/(X^D - W) in each of its forms, the
products by a base-field scalar and add / sub with schoolbook arithmetic in unsigned __int128, and asserts
every documented bound, for (BabyBear, 4, 11), (BabyBear, 2, 11), (KoalaBear, 4, 3), (Goldilocks, 2, 7) and
(1004535809, 2, 3): the cross product of the edge coordinates in every position and 10^5 seeded random pairs
each."""
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


def test_fieldext_matches_schoolbook_arithmetic(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler found (g++, c++, clang++)")
    exe = str(tmp_path / "fieldext_check")
    cmd = [cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ntt_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "fieldext_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "fieldext_check: ok" in r.stdout
