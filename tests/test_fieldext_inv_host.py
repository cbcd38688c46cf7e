"""The extension-field inverse of ntt_amd/csrc/fieldext.hpp (f31x::inv, gl64x::inv and the xf interface the
DEEP calls run on the host and in their kernels) checked on the host: tests/c/fieldext_inv_check.cpp asserts
a a^-1 = 1 with the product taken by schoolbook arithmetic in unsigned __int128 on BabyBear (d = 2, 4),
KoalaBear (d = 4), Goldilocks (d = 2, 4) and a prime above 2^30 (d = 2), each also at d = 1: random elements,
base-field elements, a = X and the edge coordinates; the inverse of 0 is 0 and returns; xf::pow agrees with
repeated products."""
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


def test_fieldext_inverse_times_the_element_is_one(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler found (g++, c++, clang++)")
    exe = str(tmp_path / "fieldext_inv_check")
    cmd = [cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ntt_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "fieldext_inv_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "fieldext_inv_check: ok" in r.stdout
