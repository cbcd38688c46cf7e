"""The FRI fold (ntt_fri_fold) at the C ABI and NTTPlan.fri_fold's argument checks, without a device: the
symbol is exported by both builds, declared in the header and in lib.PROTOTYPES, a null plan is NTT_ERR_ARG,
the Python layer refuses every bad argument before the library is reached, and fields.EXTENSIONS names the
three usual extensions."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BABYBEAR = 2013265921


def test_symbol_is_exported_by_both_builds():
    for name in ("libntt.so", "libntt_debug.so"):
        so = C.CDLL(os.path.join(ROOT, "ntt_amd", name))
        assert hasattr(so, "ntt_fri_fold"), name


def test_prototype_is_declared():
    from ntt_amd import lib as L
    res, args = L.PROTOTYPES["ntt_fri_fold"]
    assert res is C.c_int and len(args) == 10
    assert args[6] is C.c_uint64  # ext_w travels by value
    with open(os.path.join(ROOT, "include", "ntt.h")) as f:
        text = " ".join(f.read().split())
    assert ("int ntt_fri_fold(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_rows, unsigned log_arity, "
            "unsigned ext_degree, uint64_t ext_w, const uint64_t* beta, const uint64_t* shift, void* hip_stream);") in text
    assert "x FRI fold" in text  # the launch label's letter, in ntt_plan_last_launch_labels' comment


def test_null_plan_is_an_argument_error():
    from ntt_amd import lib as L
    so = L.load()
    buf, out = (C.c_uint32 * 64)(), (C.c_uint32 * 32)()
    beta = (C.c_uint64 * 4)(1, 2, 3, 4)
    shift = (C.c_uint64 * 1)(31)
    assert so.ntt_fri_fold(None, buf, out, 4, 1, 4, 11, beta, shift, None) == L.NTT_ERR_ARG
    assert so.ntt_last_error() == L.NTT_ERR_ARG
    assert so.ntt_fri_fold(None, buf, out, 4, 1, 1, 0, beta, None, None) == L.NTT_ERR_ARG


def test_extensions_table():
    from ntt_amd import fields as F
    assert F.EXTENSIONS == {3: (2, 7), 4: (4, 11), 5: (4, 3)}
    for fid, (d, w) in F.EXTENSIONS.items():
        p, _ = F.field_params(fid)
        assert pow(w, (p - 1) // 2, p) == p - 1, (fid, "W is a square")  # a non-residue
        if d == 4:
            assert p % 4 == 1  # with that, X^4 - W is irreducible


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


def test_fri_fold_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    d, w, beta = 4, 11, [1, 2, 3, 4]
    ev, out = _mat(64, d), _mat(32, d)
    ok = dict(ext_degree=d, ext_w=w)
    for k in (0, 5, -1, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="log_arity"):
            pl.fri_fold(ev, out, k, beta, **ok)
    with pytest.raises(ValueError, match="log_rows"):
        pl.fri_fold(_mat(2, d), _mat(1, d), 2, beta, log_rows=1, **ok)  # log_arity above log_rows
    for lr in (7, 2.0, "6", True):
        with pytest.raises(ValueError, match="log_rows"):
            pl.fri_fold(ev, out, 1, beta, log_rows=lr, **ok)
    for bad in (0, 3, 5, 8, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="ext_degree"):
            pl.fri_fold(ev, out, 1, beta, ext_degree=bad, ext_w=w)
    for bad in (0, BABYBEAR, BABYBEAR + 3, -1, 11.0, "11", True, None):
        with pytest.raises(ValueError, match="ext_w"):
            pl.fri_fold(ev, out, 1, beta, ext_degree=d, ext_w=bad)
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5], [], 7, None, [1, 2, 3, BABYBEAR], [1, 2, 3, -1], [1, 2, 3, 4.0],
                [1, 2, True, 4], "1234"):
        with pytest.raises(ValueError, match="beta"):
            pl.fri_fold(ev, out, 1, bad, **ok)
    with pytest.raises(ValueError, match="beta"):
        pl.fri_fold(_mat(64, 1), _mat(32, 1), 1, [BABYBEAR])  # the base field: one word, canonical
    for bad in (0, BABYBEAR, BABYBEAR + 5, -1, 31.0, "31", True):
        with pytest.raises(ValueError, match="shift"):
            pl.fri_fold(ev, out, 1, beta, shift=bad, **ok)
    with pytest.raises(TypeError):
        pl.fri_fold(ev, out, 1, beta, d, w)  # the options are keyword-only
    # tensors: shape, layout, overlap, device (checked last: everything else is right by then)
    with pytest.raises(ValueError, match="evals: expected 64 rows of 4"):
        pl.fri_fold(_mat(32, d), out, 1, beta, **ok)
    with pytest.raises(ValueError, match="out: expected 32 rows of 4"):
        pl.fri_fold(ev, _mat(64, d), 1, beta, **ok)
    with pytest.raises(ValueError, match="out: expected 4 rows of 4"):
        pl.fri_fold(ev, out, 4, beta, **ok)
    with pytest.raises(ValueError, match="evals: expected 16 rows of 4"):
        pl.fri_fold(ev, _mat(8, d), 1, beta, log_rows=4, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        pl.fri_fold(torch.zeros(64, 8, dtype=torch.int32)[:, :4], out, 1, beta, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        pl.fri_fold(_mat(64, d, torch.int64), out, 1, beta, **ok)
    both = _mat(96, d)
    with pytest.raises(ValueError, match="overlap"):
        pl.fri_fold(both[:256], both[128:256], 1, beta, **ok)
    with pytest.raises(ValueError, match="overlap"):
        pl.fri_fold(both[64:320], both[:128], 1, beta, **ok)  # out ends inside evals
    with pytest.raises(ValueError, match="device"):
        pl.fri_fold(ev, out, 1, beta, **ok)  # everything right but host tensors
    with pytest.raises(ValueError, match="device"):
        pl.fri_fold(_mat(64, 1), _mat(32, 1), 1, [5], shift=31)
