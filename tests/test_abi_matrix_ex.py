"""The coset / bit-reversed-order matrix calls (ntt_forward_matrix_ex, ntt_inverse_matrix_ex,
ntt_lde_matrix_ex) at the C ABI and the keyword options of NTTPlan.forward_matrix / inverse_matrix /
lde_matrix and lde_matrix_from_evals, without a device: the symbols are exported by both builds, declared
in the header and in lib.PROTOTYPES, a null plan is NTT_ERR_ARG, and the Python layer refuses a bad
shift, flag, width or shape before the library is reached."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BABYBEAR = 2013265921
SYMBOLS = ("ntt_forward_matrix_ex", "ntt_inverse_matrix_ex", "ntt_lde_matrix_ex")


def test_symbols_are_exported_by_both_builds():
    for name in ("libntt.so", "libntt_debug.so"):
        so = C.CDLL(os.path.join(ROOT, "ntt_amd", name))
        for sym in SYMBOLS:
            assert hasattr(so, sym), (name, sym)


def test_prototypes_are_declared():
    from ntt_amd import lib as L
    for sym, nargs in zip(SYMBOLS, (6, 6, 8)):
        res, args = L.PROTOTYPES[sym]
        assert res is C.c_int and len(args) == nargs, sym
    assert (L.NTT_MATRIX_BITREV_OUT, L.NTT_MATRIX_BITREV_IN) == (1, 2)
    with open(os.path.join(ROOT, "include", "ntt.h")) as f:
        text = " ".join(f.read().split())
    for decl in ("#define NTT_MATRIX_BITREV_OUT 1u", "#define NTT_MATRIX_BITREV_IN 2u",
                 "int ntt_forward_matrix_ex(ntt_plan* plan, void* d_data, unsigned width, const uint64_t* shift, "
                 "unsigned order, void* hip_stream);",
                 "int ntt_inverse_matrix_ex(ntt_plan* plan, void* d_data, unsigned width, const uint64_t* shift, "
                 "unsigned order, void* hip_stream);",
                 "int ntt_lde_matrix_ex(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup, "
                 "const uint64_t* shift, unsigned width, unsigned order, void* hip_stream);"):
        assert decl in text, decl


def test_null_plan_is_an_argument_error():
    from ntt_amd import lib as L
    so = L.load()
    buf = (C.c_uint64 * 8)()
    shift = (C.c_uint64 * 1)(31)
    assert so.ntt_forward_matrix_ex(None, buf, 1, shift, L.NTT_MATRIX_BITREV_OUT, None) == L.NTT_ERR_ARG
    assert so.ntt_last_error() == L.NTT_ERR_ARG
    assert so.ntt_forward_matrix_ex(None, buf, 1, None, 0, None) == L.NTT_ERR_ARG
    assert so.ntt_inverse_matrix_ex(None, buf, 1, shift, L.NTT_MATRIX_BITREV_IN, None) == L.NTT_ERR_ARG
    assert so.ntt_lde_matrix_ex(None, buf, buf, 1, shift, 1, L.NTT_MATRIX_BITREV_OUT, None) == L.NTT_ERR_ARG


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


BAD_SHIFTS = (0, BABYBEAR, BABYBEAR + 5, -1, 31.0, "31", True)
BAD_FLAGS = (1, 0, None, "yes")


@pytest.mark.parametrize("call,flag", [("forward_matrix", "bitrev_out"), ("inverse_matrix", "bitrev_in")])
def test_transforms_refuse_bad_options_before_the_library(call, flag):
    pl = _plan_without_device()
    f = getattr(pl, call)
    for shift in BAD_SHIFTS:
        with pytest.raises(ValueError, match="shift"):
            f(_mat(64, 3), 3, shift=shift)
    for v in BAD_FLAGS:
        with pytest.raises(ValueError, match=flag):
            f(_mat(64, 3), 3, **{flag: v})
    with pytest.raises(TypeError):
        f(_mat(64, 3), 3, None, 31)  # the options are keyword-only
    other = "bitrev_in" if flag == "bitrev_out" else "bitrev_out"
    with pytest.raises(TypeError):
        f(_mat(64, 3), 3, **{other: True})  # the other direction's flag
    for kw in (dict(shift=31), {flag: True}, {"shift": BABYBEAR - 1, flag: True}):
        with pytest.raises(ValueError, match="width"):
            f(_mat(64, 3), 0, **kw)
        with pytest.raises(ValueError, match="width"):
            f(_mat(64, 3), 3.0, **kw)
        with pytest.raises(ValueError, match="2\\^32"):
            f(_mat(64, 3), 1 << 26, **kw)
        with pytest.raises(ValueError, match="expected 64 rows of 3"):
            f(_mat(64, 4), 3, **kw)
        with pytest.raises(ValueError, match="expected 64 rows of 3"):
            f(_mat(32, 3), 3, **kw)
        with pytest.raises(ValueError, match="contiguous"):
            f(torch.zeros(64, 6, dtype=torch.int32)[:, :3], 3, **kw)
        with pytest.raises(ValueError, match="contiguous"):
            f(_mat(64, 3, torch.int64), 3, **kw)
        with pytest.raises(ValueError, match="device"):
            f(_mat(64, 3), 3, **kw)  # everything right but a host tensor


def test_lde_matrix_refuses_a_bad_flag_before_the_library():
    pl = _plan_without_device()
    good_in, good_out = _mat(16, 3), _mat(64, 3)
    for v in BAD_FLAGS:
        with pytest.raises(ValueError, match="bitrev_out"):
            pl.lde_matrix(good_in, good_out, 2, 31, 3, bitrev_out=v)
    with pytest.raises(TypeError):
        pl.lde_matrix(good_in, good_out, 2, 31, 3, None, True)  # keyword-only
    for shift in (0, BABYBEAR, -1):
        with pytest.raises(ValueError, match="shift"):
            pl.lde_matrix(good_in, good_out, 2, shift, 3, bitrev_out=True)
    with pytest.raises(ValueError, match="width"):
        pl.lde_matrix(good_in, good_out, 2, 31, 0, bitrev_out=True)
    with pytest.raises(ValueError, match="log_blowup"):
        pl.lde_matrix(good_in, good_out, 7, 31, 3, bitrev_out=True)
    with pytest.raises(ValueError, match="coeffs: expected 16 rows of 3"):
        pl.lde_matrix(_mat(64, 3), good_out, 2, 31, 3, bitrev_out=True)
    both = _mat(80, 3)
    with pytest.raises(ValueError, match="overlap"):
        pl.lde_matrix(both[:48], both[:192], 2, 31, 3, bitrev_out=True)
    with pytest.raises(ValueError, match="device"):
        pl.lde_matrix(good_in, good_out, 2, 31, 3, bitrev_out=True)


def test_lde_matrix_from_evals_refuses_bad_options_before_the_library():
    from ntt_amd.ntt import lde_matrix_from_evals
    small, big = _plan_without_device(4), _plan_without_device(6)
    evals, out = _mat(16, 3), _mat(64, 3)
    for shift in BAD_SHIFTS:
        with pytest.raises(ValueError, match="shift"):
            lde_matrix_from_evals(small, big, evals, out, 31, 3, in_shift=shift)
    for v in BAD_FLAGS:
        with pytest.raises(ValueError, match="bitrev_out"):
            lde_matrix_from_evals(small, big, evals, out, 31, 3, bitrev_out=v)
    with pytest.raises(ValueError, match="expected 16 rows of 3"):
        lde_matrix_from_evals(small, big, _mat(16, 2), out, 31, 3, in_shift=31, bitrev_out=True)
    with pytest.raises(ValueError, match="device"):
        lde_matrix_from_evals(small, big, evals, out, 31, 3, in_shift=31, bitrev_out=True)
