"""ntt_lde_batch at the C ABI and NTTPlan.lde_batch's argument checks, without a device: the symbol is
exported by both builds, a null plan is NTT_ERR_ARG, and the Python layer refuses bad arguments
before the library is reached."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BABYBEAR = 2013265921


def test_symbol_is_exported_by_both_builds():
    for name in ("libntt.so", "libntt_debug.so"):
        so = C.CDLL(os.path.join(ROOT, "ntt_amd", name))
        assert hasattr(so, "ntt_lde_batch"), name


def test_prototype_is_declared():
    from ntt_amd import lib as L
    res, args = L.PROTOTYPES["ntt_lde_batch"]
    assert res is C.c_int and len(args) == 7
    with open(os.path.join(ROOT, "include", "ntt.h")) as f:
        assert "int ntt_lde_batch(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup" in f.read()


def test_null_plan_is_an_argument_error():
    from ntt_amd import lib as L
    so = L.load()
    buf = (C.c_uint64 * 8)()
    assert so.ntt_lde_batch(None, buf, buf, 1, None, 1, None) == L.NTT_ERR_ARG
    assert so.ntt_last_error() == L.NTT_ERR_ARG


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _plan_without_device(log_n=10):
    """An NTTPlan object with the attributes of a BabyBear plan and no library handle behind it."""
    from ntt_amd.ntt import NTTPlan
    pl = NTTPlan.__new__(NTTPlan)
    pl._lib, pl._h = _NoLibrary(), None
    pl.log_n, pl.n, pl.limbs64, pl.device = log_n, 1 << log_n, 1, 0
    pl.p, pl.g = BABYBEAR, 31
    pl.elem_bytes, pl.elem32, pl.dtype, pl.montgomery_io = 4, True, torch.int32, False
    return pl


@pytest.mark.parametrize("kw", [dict(log_blowup=11), dict(log_blowup=-1), dict(log_blowup=1.0), dict(batch=0),
                                dict(batch=-2), dict(shift=0), dict(shift=BABYBEAR), dict(shift=-1)])
def test_lde_batch_refuses_bad_scalars_before_the_library(kw):
    pl = _plan_without_device()
    args = dict(log_blowup=2, shift=31, batch=1)
    args.update(kw)
    coeffs, out = torch.zeros(256, dtype=torch.int32), torch.zeros(1024, dtype=torch.int32)
    with pytest.raises(ValueError):
        pl.lde_batch(coeffs, out, args["log_blowup"], args["shift"], args["batch"])


def test_lde_batch_refuses_host_tensors_before_the_library():
    pl = _plan_without_device()
    coeffs, out = torch.zeros(256, dtype=torch.int32), torch.zeros(1024, dtype=torch.int32)
    with pytest.raises(ValueError, match="device"):
        pl.lde_batch(coeffs, out, 2, 31, 1)


def test_lde_from_evals_refuses_mismatched_plans_before_the_library():
    from ntt_amd.ntt import lde_from_evals
    small, big = _plan_without_device(8), _plan_without_device(10)
    evals, out = torch.zeros(256, dtype=torch.int32), torch.zeros(1024, dtype=torch.int32)
    with pytest.raises(ValueError):
        lde_from_evals(big, small, evals, out)  # the large plan first
    big.p = 2130706433
    with pytest.raises(ValueError):
        lde_from_evals(small, big, evals, out)
