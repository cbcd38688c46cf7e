"""The DEEP calls (ntt_deep_points, ntt_matrix_open, ntt_deep_quotient, ntt_deep_info) at the C ABI and the
argument checks of NTTPlan.deep_points / open_matrix / deep_quotient / deep_info, without a device: the symbols
are exported by both builds, declared in the header and in lib.PROTOTYPES, a null plan is NTT_ERR_ARG, and the
Python layer refuses every bad argument before the library is reached."""
import ctypes as C
import os

import pytest
import torch

from tests.test_abi_fold import BABYBEAR, _mat, _plan_without_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ntt_deep_points", "ntt_matrix_open", "ntt_deep_quotient", "ntt_deep_info")


def test_symbols_are_exported_by_both_builds():
    for lib in ("libntt.so", "libntt_debug.so"):
        so = C.CDLL(os.path.join(ROOT, "ntt_amd", lib))
        for name in NAMES:
            assert hasattr(so, name), (lib, name)


def test_prototypes_are_declared():
    from ntt_amd import lib as L
    assert [len(L.PROTOTYPES[n][1]) for n in NAMES] == [9, 12, 13, 6]
    for n in NAMES:
        assert L.PROTOTYPES[n][0] is C.c_int
    assert L.PROTOTYPES["ntt_deep_points"][1][4] is C.c_uint64  # ext_w travels by value
    assert L.PROTOTYPES["ntt_matrix_open"][1][6] is C.c_uint64
    assert L.PROTOTYPES["ntt_deep_quotient"][1][7] is C.c_uint64
    assert L.NTT_DEEP_ACCUMULATE == 1
    with open(os.path.join(ROOT, "include", "ntt.h")) as f:
        text = " ".join(f.read().split())
    for proto in (
            "int ntt_deep_points(ntt_plan* plan, void* d_inv, unsigned log_rows, unsigned ext_degree, uint64_t ext_w, "
            "const uint64_t* z, const uint64_t* shift, unsigned order, void* hip_stream);",
            "int ntt_matrix_open(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, const void* d_inv, "
            "unsigned ext_degree, uint64_t ext_w, const uint64_t* z, const uint64_t* shift, unsigned order, "
            "void* d_values, void* hip_stream);",
            "int ntt_deep_quotient(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, "
            "const void* d_inv, const void* d_values, unsigned ext_degree, uint64_t ext_w, const uint64_t* alpha, "
            "const uint64_t* scale, unsigned flags, void* d_out, void* hip_stream);",
            "int ntt_deep_info(const ntt_plan* plan, unsigned width, unsigned log_rows, unsigned ext_degree, "
            "unsigned* open_row_chunks, unsigned* quotient_lanes_per_row);",
            "#define NTT_DEEP_ACCUMULATE 1u"):
        assert proto in text, proto
    assert "z DEEP points" in text and "q quotient" in text  # the launch labels' letters


def test_null_plan_is_an_argument_error():
    from ntt_amd import lib as L
    so = L.load()
    a, b, c, d = ((C.c_uint32 * 64)() for _ in range(4))
    z = (C.c_uint64 * 4)(1, 2, 3, 4)
    sh = (C.c_uint64 * 1)(31)
    chunks, lanes = C.c_uint(7), C.c_uint(7)
    assert so.ntt_deep_points(None, a, 4, 4, 11, z, sh, 1, None) == L.NTT_ERR_ARG
    assert so.ntt_last_error() == L.NTT_ERR_ARG
    assert so.ntt_matrix_open(None, a, 1, 4, b, 4, 11, z, None, 0, c, None) == L.NTT_ERR_ARG
    assert so.ntt_deep_quotient(None, a, 1, 4, b, c, 4, 11, z, None, 0, d, None) == L.NTT_ERR_ARG
    assert so.ntt_deep_info(None, 1, 4, 4, C.byref(chunks), C.byref(lanes)) == L.NTT_ERR_ARG
    assert (chunks.value, lanes.value) == (7, 7)


BAD_WORDS = ([1, 2, 3], [1, 2, 3, 4, 5], [], 7, None, [1, 2, 3, BABYBEAR], [1, 2, 3, -1], [1, 2, 3, 4.0],
             [1, 2, True, 4], "1234")


def test_deep_points_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    d, w, z = 4, 11, [1, 2, 3, 4]
    out = _mat(64, d)
    ok = dict(ext_degree=d, ext_w=w)
    for lr in (7, -1, 2.0, "6", True):
        with pytest.raises(ValueError, match="log_rows"):
            pl.deep_points(out, z, log_rows=lr, **ok)
    for bad in (0, 3, 5, 8, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="ext_degree"):
            pl.deep_points(out, z, ext_degree=bad, ext_w=w)
    for bad in (0, BABYBEAR, -1, 11.0, "11", True, None):
        with pytest.raises(ValueError, match="ext_w"):
            pl.deep_points(out, z, ext_degree=d, ext_w=bad)
    for bad in BAD_WORDS:
        with pytest.raises(ValueError, match="z must be"):
            pl.deep_points(out, bad, **ok)
    for bad in (0, BABYBEAR, -1, 31.0, "31", True):
        with pytest.raises(ValueError, match="shift"):
            pl.deep_points(out, z, shift=bad, **ok)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="bitrev"):
            pl.deep_points(out, z, bitrev=bad, **ok)
    with pytest.raises(TypeError):
        pl.deep_points(out, z, d, w)  # the options are keyword-only
    # a base-field z on the coset: 31^64 = (31 w)^64 for any 64th root of unity w; 1 is on <w_N> itself
    on = pow(31, (BABYBEAR - 1) // 64, BABYBEAR) * 5 % BABYBEAR
    for zz, kw in (([on * 1 % BABYBEAR, 0, 0, 0], dict(shift=5, **ok)), ([1, 0, 0, 0], ok), ([1], {})):
        with pytest.raises(ValueError, match="domain"):
            pl.deep_points(_mat(64, len(zz)), zz, **kw)
    with pytest.raises(ValueError, match="out: expected 64 rows of 4"):
        pl.deep_points(_mat(32, d), z, **ok)
    with pytest.raises(ValueError, match="out: expected 16 rows of 4"):
        pl.deep_points(out, z, log_rows=4, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        pl.deep_points(_mat(64, d, torch.int64), z, **ok)
    with pytest.raises(ValueError, match="device"):
        pl.deep_points(out, z, **ok)  # everything right but a host tensor
    with pytest.raises(ValueError, match="device"):
        pl.deep_points(_mat(1, 1), [5], log_rows=0, shift=31)


def test_open_matrix_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    d, w, z, width = 4, 11, [1, 2, 3, 4], 5
    mat, inv, val = _mat(64, width), _mat(64, d), _mat(width, d)
    ok = dict(ext_degree=d, ext_w=w)
    for bad in (0, -1, 5.0, "5", True, None):
        with pytest.raises(ValueError, match="width"):
            pl.open_matrix(mat, bad, inv, val, z, **ok)
    with pytest.raises(ValueError, match="below 2\\^32"):
        pl.open_matrix(mat, 1 << 26, inv, val, z, **ok)
    for lr in (7, 2.0, True):
        with pytest.raises(ValueError, match="log_rows"):
            pl.open_matrix(mat, width, inv, val, z, log_rows=lr, **ok)
    with pytest.raises(ValueError, match="ext_degree"):
        pl.open_matrix(mat, width, inv, val, z, ext_degree=3, ext_w=w)
    with pytest.raises(ValueError, match="ext_w"):
        pl.open_matrix(mat, width, inv, val, z, ext_degree=d, ext_w=0)
    for bad in BAD_WORDS:
        with pytest.raises(ValueError, match="z must be"):
            pl.open_matrix(mat, width, inv, val, bad, **ok)
    with pytest.raises(ValueError, match="shift"):
        pl.open_matrix(mat, width, inv, val, z, shift=0, **ok)
    with pytest.raises(ValueError, match="bitrev"):
        pl.open_matrix(mat, width, inv, val, z, bitrev=1, **ok)
    with pytest.raises(ValueError, match="domain"):
        pl.open_matrix(mat, width, inv, val, [1, 0, 0, 0], **ok)
    with pytest.raises(ValueError, match="mat: expected 64 rows of 5"):
        pl.open_matrix(_mat(64, 4), width, inv, val, z, **ok)
    with pytest.raises(ValueError, match="inv: expected 64 rows of 4"):
        pl.open_matrix(mat, width, _mat(32, d), val, z, **ok)
    with pytest.raises(ValueError, match="values: expected 5 rows of 4"):
        pl.open_matrix(mat, width, inv, _mat(4, d), z, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        pl.open_matrix(_mat(64, width, torch.int64), width, inv, val, z, **ok)
    both = _mat(64 + width, d)
    with pytest.raises(ValueError, match="inv and values overlap"):
        pl.open_matrix(mat, width, both[:256], both[236:256], z, **ok)
    big = _mat(64, width)
    with pytest.raises(ValueError, match="mat and values overlap"):
        pl.open_matrix(big, width, inv, big[300:320], z, **ok)
    with pytest.raises(ValueError, match="device"):
        pl.open_matrix(mat, width, inv, val, z, **ok)


def test_deep_quotient_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    d, w, al, width = 4, 11, [1, 2, 3, 4], 5
    mat, inv, val, out = _mat(64, width), _mat(64, d), _mat(width, d), _mat(64, d)
    ok = dict(ext_degree=d, ext_w=w)
    for bad in (0, -1, 5.0, True):
        with pytest.raises(ValueError, match="width"):
            pl.deep_quotient(mat, bad, inv, val, out, al, **ok)
    for bad in BAD_WORDS:
        with pytest.raises(ValueError, match="alpha must be"):
            pl.deep_quotient(mat, width, inv, val, out, bad, **ok)
    for bad in BAD_WORDS:
        if bad is None:
            continue  # None is scale = 1
        with pytest.raises(ValueError, match="scale must be"):
            pl.deep_quotient(mat, width, inv, val, out, al, scale=bad, **ok)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="accumulate"):
            pl.deep_quotient(mat, width, inv, val, out, al, accumulate=bad, **ok)
    with pytest.raises(ValueError, match="log_rows"):
        pl.deep_quotient(mat, width, inv, val, out, al, log_rows=7, **ok)
    with pytest.raises(ValueError, match="ext_degree"):
        pl.deep_quotient(mat, width, inv, val, out, al, ext_degree=8, ext_w=w)
    with pytest.raises(ValueError, match="ext_w"):
        pl.deep_quotient(mat, width, inv, val, out, al, ext_degree=d, ext_w=BABYBEAR)
    with pytest.raises(TypeError):
        pl.deep_quotient(mat, width, inv, val, out, al, al)  # the options are keyword-only
    with pytest.raises(ValueError, match="out: expected 64 rows of 4"):
        pl.deep_quotient(mat, width, inv, val, _mat(32, d), al, **ok)
    with pytest.raises(ValueError, match="values: expected 5 rows of 4"):
        pl.deep_quotient(mat, width, inv, _mat(6, d), out, al, **ok)
    both = _mat(128, d)
    with pytest.raises(ValueError, match="inv and out overlap"):
        pl.deep_quotient(mat, width, both[:256], val, both[252:508], al, **ok)
    with pytest.raises(ValueError, match="values and out overlap"):
        pl.deep_quotient(mat, width, inv, both[250:270], both[:256], al, **ok)
    with pytest.raises(ValueError, match="mat and out overlap"):
        pl.deep_quotient(both[:320], width, inv, val, both[256:512], al, **ok)
    with pytest.raises(ValueError, match="device"):
        pl.deep_quotient(mat, width, inv, val, out, al, scale=[5, 0, 0, 0], accumulate=True, **ok)


def test_deep_info_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    for bad in (0, -3, 2.0, True, None):
        with pytest.raises(ValueError, match="width"):
            pl.deep_info(bad)
    with pytest.raises(ValueError, match="log_rows"):
        pl.deep_info(4, log_rows=7)
    with pytest.raises(ValueError, match="ext_degree"):
        pl.deep_info(4, ext_degree=3)
    with pytest.raises(ValueError, match="below 2\\^32"):
        pl.deep_info(1 << 26)
    with pytest.raises(AssertionError, match="library was reached"):
        pl.deep_info(4, log_rows=3, ext_degree=2)
