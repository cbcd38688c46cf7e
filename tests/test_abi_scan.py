"""ntt_batch_inverse, ntt_matrix_scan and ntt_scan_info at the C ABI and the argument checks of
NTTPlan.batch_inverse / matrix_scan / scan_info, without a device: the symbols are exported by both builds, declared
in the header and in lib.PROTOTYPES, a null plan is NTT_ERR_ARG with the info outputs untouched, and the Python
layer refuses every bad argument before the library is reached."""
import ctypes as C
import os

import pytest
import torch

from tests.test_abi_fold import BABYBEAR, _mat, _plan_without_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ntt_batch_inverse", "ntt_matrix_scan", "ntt_scan_info")


def test_symbols_are_exported_by_both_builds():
    for lib in ("libntt.so", "libntt_debug.so"):
        so = C.CDLL(os.path.join(ROOT, "ntt_amd", lib))
        for name in NAMES:
            assert hasattr(so, name), (lib, name)


def test_prototypes_are_declared():
    from ntt_amd import lib as L
    assert [len(L.PROTOTYPES[n][1]) for n in NAMES] == [7, 11, 10]
    for n in NAMES:
        assert L.PROTOTYPES[n][0] is C.c_int
    assert L.PROTOTYPES["ntt_batch_inverse"][1][3] is C.c_uint64 and L.PROTOTYPES["ntt_batch_inverse"][1][5] is C.c_uint64
    assert L.PROTOTYPES["ntt_matrix_scan"][1][3] is C.c_uint64 and L.PROTOTYPES["ntt_matrix_scan"][1][6] is C.c_uint64
    assert L.PROTOTYPES["ntt_scan_info"][1][1] is C.c_uint64
    assert (L.NTT_SCAN_SUM, L.NTT_SCAN_PRODUCT, L.NTT_SCAN_EXCLUSIVE) == (0, 1, 1)
    with open(os.path.join(ROOT, "include", "ntt.h")) as f:
        text = " ".join(f.read().split())
    for proto in (
            "int ntt_batch_inverse(ntt_plan* plan, const void* d_in, void* d_out, uint64_t count, unsigned ext_degree, "
            "uint64_t ext_w, void* hip_stream);",
            "int ntt_matrix_scan(ntt_plan* plan, const void* d_in, void* d_out, uint64_t rows, unsigned width, "
            "unsigned ext_degree, uint64_t ext_w, unsigned op, unsigned flags, void* d_totals, void* hip_stream);",
            "int ntt_scan_info(const ntt_plan* plan, uint64_t rows, unsigned width, unsigned ext_degree, unsigned op, "
            "unsigned* strip_cols, unsigned* run_rows, unsigned* chunk_rows, unsigned* chunks, unsigned* launches);",
            "#define NTT_SCAN_SUM 0u", "#define NTT_SCAN_PRODUCT 1u", "#define NTT_SCAN_EXCLUSIVE 1u"):
        assert proto in text, proto
    for label in ("v batch inverse", "t chunk totals", "k the scan", "y the chunk scan"):  # the comment wraps inside "of the totals"
        assert label in text, label
    assert "g open (gather); p permute." in text  # the label comment's earlier wording stays


def test_null_plan_is_an_argument_error():
    from ntt_amd import lib as L
    so = L.load()
    a, b, c = ((C.c_uint32 * 64)() for _ in range(3))
    assert so.ntt_batch_inverse(None, a, b, 16, 4, 11, None) == L.NTT_ERR_ARG
    assert so.ntt_last_error() == L.NTT_ERR_ARG
    assert so.ntt_matrix_scan(None, a, b, 16, 1, 4, 11, 1, 0, c, None) == L.NTT_ERR_ARG
    v = [C.c_uint(7) for _ in range(5)]
    assert so.ntt_scan_info(None, 16, 1, 4, 0, *(C.byref(x) for x in v)) == L.NTT_ERR_ARG
    assert [x.value for x in v] == [7] * 5


def test_batch_inverse_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    t = _mat(16, 4)
    for bad in (0, 3, 5, 8, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="ext_degree"):
            pl.batch_inverse(t, ext_degree=bad, ext_w=11)
    for bad in (0, BABYBEAR, BABYBEAR + 3, -1, 11.0, "11", True, None):
        with pytest.raises(ValueError, match="ext_w"):
            pl.batch_inverse(t, ext_degree=4, ext_w=bad)
    for bad in (_mat(16, 4, torch.int64), _mat(32, 4)[::2], [0] * 64, None):
        with pytest.raises(ValueError, match="contiguous"):
            pl.batch_inverse(bad, ext_degree=4, ext_w=11)
    with pytest.raises(ValueError, match="contiguous"):
        pl.batch_inverse(t, _mat(16, 4, torch.int64), ext_degree=4, ext_w=11)
    for bad in (_mat(0, 4), _mat(3, 1), _mat(5, 2)):
        with pytest.raises(ValueError, match="multiple of 4"):
            pl.batch_inverse(bad, ext_degree=4, ext_w=11)
    with pytest.raises(ValueError, match="out: expected 64 elements"):
        pl.batch_inverse(t, _mat(15, 4), ext_degree=4, ext_w=11)
    both = _mat(100, 1)
    with pytest.raises(ValueError, match="t and out overlap"):
        pl.batch_inverse(both[:64], both[4:68], ext_degree=4, ext_w=11)
    with pytest.raises(ValueError, match="device"):
        pl.batch_inverse(t, _mat(16, 4), ext_degree=4, ext_w=11)  # everything right but host tensors
    with pytest.raises(ValueError, match="device"):
        pl.batch_inverse(t)  # in place, ext_degree 1: ext_w is not read
    wide = _plan_without_device()
    wide.elem32, wide.elem_bytes, wide.limbs64, wide.dtype = False, 32, 4, torch.int64
    with pytest.raises(ValueError, match="Goldilocks plan or a plan of 4-byte elements"):
        wide.batch_inverse(_mat(16, 4, torch.int64))


def test_matrix_scan_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    mat, out, tot = _mat(100, 3 * 4), _mat(100, 3 * 4), _mat(3, 4)
    ok = dict(op="product", ext_degree=4, ext_w=11)
    for bad in ("max", 0, 1, None, "SUM"):
        with pytest.raises(ValueError, match="op must be"):
            pl.matrix_scan(mat, out, 3, op=bad, ext_degree=4, ext_w=11)
    for bad in (0, 3, 8, 4.0, "4", True, None):
        with pytest.raises(ValueError, match="ext_degree"):
            pl.matrix_scan(mat, out, 3, op="product", ext_degree=bad, ext_w=11, rows=100)
    for bad in (0, BABYBEAR, -1, 11.0, "11", True, None):
        with pytest.raises(ValueError, match="ext_w"):
            pl.matrix_scan(mat, out, 3, op="product", ext_degree=4, ext_w=bad)
    for bad in (0, -1, 3.0, "3", True, None):
        with pytest.raises(ValueError, match="width"):
            pl.matrix_scan(mat, out, bad, rows=100, **ok)
    for bad in (0, -1, 100.0, "100", True):
        with pytest.raises(ValueError, match="rows"):
            pl.matrix_scan(mat, out, 3, rows=bad, **ok)
    with pytest.raises(ValueError, match="below 2\\^32"):
        pl.matrix_scan(mat, out, 1 << 20, rows=1 << 10, **ok)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="exclusive"):
            pl.matrix_scan(mat, out, 3, exclusive=bad, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        pl.matrix_scan(_mat(100, 12, torch.int64), out, 3, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        pl.matrix_scan(mat, _mat(200, 12)[::2], 3, **ok)
    with pytest.raises(ValueError, match="mat: expected 99 rows of 12"):
        pl.matrix_scan(mat, out, 3, rows=99, **ok)
    with pytest.raises(ValueError, match="out: expected 100 rows of 12"):
        pl.matrix_scan(mat, _mat(101, 12), 3, **ok)
    with pytest.raises(ValueError, match="totals: expected 3 rows of 4"):
        pl.matrix_scan(mat, out, 3, totals=_mat(3, 3), **ok)
    with pytest.raises(ValueError, match="contiguous"):
        pl.matrix_scan(mat, out, 3, totals=_mat(3, 4, torch.int64), **ok)
    both = _mat(100 * 12 + 40, 1)
    with pytest.raises(ValueError, match="mat and out overlap"):
        pl.matrix_scan(both[:1200], both[12:1212], 3, **ok)
    with pytest.raises(ValueError, match="mat and totals overlap"):
        pl.matrix_scan(both[:1200], out, 3, totals=both[1190:1202], **ok)
    with pytest.raises(ValueError, match="out and totals overlap"):
        pl.matrix_scan(mat, both[:1200], 3, totals=both[0:12], **ok)
    with pytest.raises(ValueError, match="device"):
        pl.matrix_scan(mat, out, 3, totals=tot, **ok)  # everything right but host tensors
    with pytest.raises(ValueError, match="device"):
        pl.matrix_scan(mat, mat, 3, op="sum", ext_degree=4, ext_w=0)  # in place; the sum does not read ext_w


def test_scan_info_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    for bad in (0, -1, 7.0, "7", True, None):
        with pytest.raises(ValueError, match="rows"):
            pl.scan_info(bad, 3)
        with pytest.raises(ValueError, match="width"):
            pl.scan_info(7, bad)
    for bad in (0, 3, "1", True, None):
        with pytest.raises(ValueError, match="ext_degree"):
            pl.scan_info(7, 3, ext_degree=bad)
    with pytest.raises(ValueError, match="op must be"):
        pl.scan_info(7, 3, op="min")
    with pytest.raises(ValueError, match="below 2\\^32"):
        pl.scan_info(1 << 30, 1, ext_degree=4)
