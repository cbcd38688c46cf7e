"""The row-major matrix calls (ntt_forward_matrix, ntt_inverse_matrix, ntt_lde_matrix,
ntt_plan_matrix_info) at the C ABI and the argument checks of NTTPlan.forward_matrix / inverse_matrix /
lde_matrix / matrix_passes and lde_matrix_from_evals, without a device: the symbols are exported by both
builds, declared in the header and in lib.PROTOTYPES, a null plan is NTT_ERR_ARG, and the Python layer
refuses bad arguments before the library is reached."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BABYBEAR = 2013265921
SYMBOLS = ("ntt_forward_matrix", "ntt_inverse_matrix", "ntt_lde_matrix", "ntt_plan_matrix_info")


def test_symbols_are_exported_by_both_builds():
    for name in ("libntt.so", "libntt_debug.so"):
        so = C.CDLL(os.path.join(ROOT, "ntt_amd", name))
        for sym in SYMBOLS:
            assert hasattr(so, sym), (name, sym)


def test_prototypes_are_declared():
    from ntt_amd import lib as L
    for sym, nargs in zip(SYMBOLS, (4, 4, 7, 4)):
        res, args = L.PROTOTYPES[sym]
        assert res is C.c_int and len(args) == nargs, sym
    with open(os.path.join(ROOT, "include", "ntt.h")) as f:
        text = f.read()
    for decl in ("int ntt_forward_matrix(ntt_plan* plan, void* d_data, unsigned width, void* hip_stream);",
                 "int ntt_inverse_matrix(ntt_plan* plan, void* d_data, unsigned width, void* hip_stream);",
                 "int ntt_lde_matrix(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup",
                 "int ntt_plan_matrix_info(const ntt_plan* plan, unsigned width, unsigned* npasses, "
                 "unsigned radix_log[8]);"):
        assert decl in text, decl


def test_null_plan_is_an_argument_error():
    from ntt_amd import lib as L
    so = L.load()
    buf = (C.c_uint64 * 8)()
    npass = C.c_uint()
    radix = (C.c_uint * 8)()
    assert so.ntt_forward_matrix(None, buf, 1, None) == L.NTT_ERR_ARG
    assert so.ntt_last_error() == L.NTT_ERR_ARG
    assert so.ntt_inverse_matrix(None, buf, 1, None) == L.NTT_ERR_ARG
    assert so.ntt_lde_matrix(None, buf, buf, 1, None, 1, None) == L.NTT_ERR_ARG
    assert so.ntt_plan_matrix_info(None, 1, C.byref(npass), radix) == L.NTT_ERR_ARG


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _plan_without_device(log_n=6):
    """An NTTPlan object with the attributes of a BabyBear plan and no library handle behind it."""
    from ntt_amd.ntt import NTTPlan
    pl = NTTPlan.__new__(NTTPlan)
    pl._lib, pl._h = _NoLibrary(), None
    pl.log_n, pl.n, pl.limbs64, pl.device = log_n, 1 << log_n, 1, 0
    pl.p, pl.g = BABYBEAR, 31
    pl.elem_bytes, pl.elem32, pl.dtype, pl.montgomery_io = 4, True, torch.int32, False
    return pl


def _mat(rows, width, dtype=torch.int32):
    return torch.zeros(rows * width, dtype=dtype)


@pytest.mark.parametrize("call", ["forward_matrix", "inverse_matrix"])
def test_transforms_refuse_bad_arguments_before_the_library(call):
    pl = _plan_without_device()
    f = getattr(pl, call)
    with pytest.raises(ValueError, match="width"):
        f(_mat(64, 3), 0)
    with pytest.raises(ValueError, match="width"):
        f(_mat(64, 3), -3)
    with pytest.raises(ValueError, match="width"):
        f(_mat(64, 3), 3.0)
    with pytest.raises(ValueError, match="2\\^32"):
        f(_mat(64, 3), 1 << 26)
    with pytest.raises(ValueError, match="expected 64 rows of 3"):
        f(_mat(64, 4), 3)  # a matrix of another width
    with pytest.raises(ValueError, match="expected 64 rows of 3"):
        f(_mat(32, 3), 3)  # too few rows
    with pytest.raises(ValueError, match="contiguous"):
        f(torch.zeros(64, 6, dtype=torch.int32)[:, :3], 3)  # a row pitch other than width
    with pytest.raises(ValueError, match="contiguous"):
        f(_mat(64, 3, torch.int64), 3)  # another element type
    with pytest.raises(ValueError, match="device"):
        f(_mat(64, 3), 3)  # everything right but a host tensor


def test_lde_matrix_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    good_in, good_out = _mat(16, 3), _mat(64, 3)
    for kw in (dict(log_blowup=7), dict(log_blowup=-1), dict(log_blowup=1.0), dict(shift=0), dict(shift=BABYBEAR),
               dict(shift=-1), dict(width=0), dict(width=-1)):
        args = dict(log_blowup=2, shift=31, width=3)
        args.update(kw)
        with pytest.raises(ValueError):
            pl.lde_matrix(good_in, good_out, args["log_blowup"], args["shift"], args["width"])
    with pytest.raises(ValueError, match="coeffs: expected 16 rows of 3"):
        pl.lde_matrix(_mat(64, 3), good_out, 2, 31, 3)
    with pytest.raises(ValueError, match="out: expected 64 rows of 3"):
        pl.lde_matrix(good_in, _mat(16, 3), 2, 31, 3)
    with pytest.raises(ValueError, match="coeffs must be a contiguous"):
        pl.lde_matrix(torch.zeros(16, 6, dtype=torch.int32)[:, :3], good_out, 2, 31, 3)
    with pytest.raises(ValueError, match="out must be a contiguous"):
        pl.lde_matrix(good_in, torch.zeros(64, 6, dtype=torch.int32)[:, :3], 2, 31, 3)
    both = _mat(80, 3)
    with pytest.raises(ValueError, match="overlap"):
        pl.lde_matrix(both[:48], both[:192], 2, 31, 3)  # coeffs inside out
    with pytest.raises(ValueError, match="overlap"):
        pl.lde_matrix(both[180:228], both[:192], 2, 31, 3)  # the last elements of out
    with pytest.raises(ValueError, match="device"):
        pl.lde_matrix(good_in, good_out, 2, 31, 3)
    with pytest.raises(ValueError, match="device"):
        pl.lde_matrix(both[192:240], both[:192], 2, 31, 3)  # adjacent, not overlapping: only the device is wrong


def test_matrix_passes_refuses_a_bad_width_before_the_library():
    pl = _plan_without_device()
    for w in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="width"):
            pl.matrix_passes(w)


def test_lde_matrix_from_evals_refuses_bad_arguments_before_the_library():
    from ntt_amd.ntt import lde_matrix_from_evals
    small, big = _plan_without_device(4), _plan_without_device(6)
    evals, out = _mat(16, 3), _mat(64, 3)
    with pytest.raises(ValueError, match="at least as large"):
        lde_matrix_from_evals(big, small, evals, out, 31, 3)  # the large plan first
    with pytest.raises(ValueError, match="expected 16 rows of 3"):
        lde_matrix_from_evals(small, big, _mat(16, 2), out, 31, 3)
    with pytest.raises(ValueError, match="width"):
        lde_matrix_from_evals(small, big, evals, out, 31, 0)
    big.p = 2130706433
    with pytest.raises(ValueError, match="share field"):
        lde_matrix_from_evals(small, big, evals, out, 31, 3)
