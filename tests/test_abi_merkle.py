"""The Poseidon2 Merkle calls (ntt_plan_set_poseidon2, ntt_poseidon2_permute, ntt_merkle_commit, ntt_merkle_open,
ntt_merkle_info) at the C ABI and the argument checks of NTTPlan.set_poseidon2 / poseidon2_permute / merkle_commit /
merkle_open / merkle_info, without a device: the symbols are exported by both builds, declared in the header and
in lib.PROTOTYPES, a null plan is NTT_ERR_ARG, and the Python layer refuses every bad argument before the library
is reached."""
import ctypes as C
import os

import pytest
import torch

from tests.test_abi_fold import BABYBEAR, _mat, _plan_without_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ntt_plan_set_poseidon2", "ntt_poseidon2_permute", "ntt_merkle_commit", "ntt_merkle_open", "ntt_merkle_info")
T, D = 16, 8


def test_symbols_are_exported_by_both_builds():
    for lib in ("libntt.so", "libntt_debug.so"):
        so = C.CDLL(os.path.join(ROOT, "ntt_amd", lib))
        for name in NAMES:
            assert hasattr(so, name), (lib, name)


def test_prototypes_are_declared():
    from ntt_amd import lib as L
    assert [len(L.PROTOTYPES[n][1]) for n in NAMES] == [8, 4, 6, 10, 7]
    for n in NAMES:
        assert L.PROTOTYPES[n][0] is C.c_int
    assert L.PROTOTYPES["ntt_poseidon2_permute"][1][2] is C.c_uint64  # count
    assert L.PROTOTYPES["ntt_merkle_info"][1][4] == C.POINTER(C.c_uint64)  # tree_elems
    with open(os.path.join(ROOT, "include", "ntt.h")) as f:
        text = " ".join(f.read().split())
    for proto in (
            "int ntt_plan_set_poseidon2(ntt_plan* plan, unsigned width, unsigned sbox_degree, unsigned rounds_f, "
            "unsigned rounds_p, const uint64_t* ext_rc, const uint64_t* int_rc, const uint64_t* int_diag);",
            "int ntt_poseidon2_permute(ntt_plan* plan, void* d_states, uint64_t count, void* hip_stream);",
            "int ntt_merkle_commit(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, void* d_tree, "
            "void* hip_stream);",
            "int ntt_merkle_open(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, "
            "const void* d_tree, const uint32_t* d_index, unsigned nq, void* d_rows, void* d_paths, void* hip_stream);",
            "int ntt_merkle_info(const ntt_plan* plan, unsigned width, unsigned log_rows, unsigned* digest_elems, "
            "uint64_t* tree_elems, unsigned* launches, unsigned* tail_log);"):
        assert proto in text, proto
    for label in ("h leaf hash", "m tree layers", "g open", "p permute"):  # the launch labels' letters
        assert label in text, label
    assert "q quotient: the rows), \"\" * when unlabelled." in text  # the label comment's earlier wording stays


def test_null_plan_is_an_argument_error():
    from ntt_amd import lib as L
    so = L.load()
    a, b, c, d = ((C.c_uint32 * 64)() for _ in range(4))
    idx = (C.c_uint32 * 4)(0, 1, 2, 3)
    ext, irc, diag = (C.c_uint64 * (8 * T))(), (C.c_uint64 * 13)(), (C.c_uint64 * T)()
    assert so.ntt_plan_set_poseidon2(None, T, 7, 8, 13, ext, irc, diag) == L.NTT_ERR_ARG
    assert so.ntt_last_error() == L.NTT_ERR_ARG
    assert so.ntt_poseidon2_permute(None, a, 1, None) == L.NTT_ERR_ARG
    assert so.ntt_merkle_commit(None, a, 1, 2, b, None) == L.NTT_ERR_ARG
    assert so.ntt_merkle_open(None, a, 1, 2, b, idx, 4, c, d, None) == L.NTT_ERR_ARG
    de, te, la, tl = C.c_uint(7), C.c_uint64(7), C.c_uint(7), C.c_uint(7)
    assert so.ntt_merkle_info(None, 1, 2, C.byref(de), C.byref(te), C.byref(la), C.byref(tl)) == L.NTT_ERR_ARG
    assert (de.value, te.value, la.value, tl.value) == (7, 7, 7, 7)


def test_shapes_are_recorded():
    from ntt_amd.fields import POSEIDON2_SHAPES
    assert POSEIDON2_SHAPES == {3: (8, 7, 8, 22), 4: (16, 7, 8, 13), 5: (16, 3, 8, 20)}


def _params(rf=8, rp=13):
    return [[1] * T for _ in range(rf)], [2] * rp, [3] * T


def _set_plan(log_n=6):
    pl = _plan_without_device(log_n)
    pl._poseidon2 = (7, 8, 13)  # as after set_poseidon2
    return pl


def test_set_poseidon2_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()
    ext, irc, diag = _params()
    assert pl.poseidon2_width == T
    for bad in (8, 24, 0, 16.0, "16", True):
        with pytest.raises(ValueError, match="width"):
            pl.set_poseidon2(7, 8, 13, ext, irc, diag, width=bad)
    for bad in (0, 1, 2, 4, 9, 7.0, "7", True, None):
        with pytest.raises(ValueError, match="sbox_degree"):
            pl.set_poseidon2(bad, 8, 13, ext, irc, diag)
    for bad in (3, 5):  # p - 1 = 2^27 * 15
        with pytest.raises(ValueError, match="divides p - 1"):
            pl.set_poseidon2(bad, 8, 13, ext, irc, diag)
    for bad in (0, 1, 7, 18, -2, 8.0, "8", True, None):
        with pytest.raises(ValueError, match="rounds_f"):
            pl.set_poseidon2(7, bad, 13, ext, irc, diag)
    for bad in (-1, 65, 13.0, "13", True, None):
        with pytest.raises(ValueError, match="rounds_p"):
            pl.set_poseidon2(7, 8, bad, ext, irc, diag)
    for bad in (ext[:7], ext + [[1] * T], 5, None, "x" * 8):
        with pytest.raises(ValueError, match="ext_rc"):
            pl.set_poseidon2(7, 8, 13, bad, irc, diag)
    for row in ([1] * 15, [1] * 17, [1] * 15 + [BABYBEAR], [1] * 15 + [-1], [1] * 15 + [1.0], [1] * 15 + [True], 7, "1" * T):
        with pytest.raises(ValueError, match=r"ext_rc\[3\]"):
            pl.set_poseidon2(7, 8, 13, ext[:3] + [row] + ext[4:], irc, diag)
    for bad in ([2] * 12, [2] * 14, [2] * 12 + [BABYBEAR], [2] * 12 + [-1], [2] * 12 + [2.0], 7, None):
        with pytest.raises(ValueError, match="int_rc"):
            pl.set_poseidon2(7, 8, 13, ext, bad, diag)
    for bad in ([3] * 15, [3] * 17, [3] * 15 + [BABYBEAR], [3] * 15 + [True], None):
        with pytest.raises(ValueError, match="int_diag"):
            pl.set_poseidon2(7, 8, 13, ext, irc, bad)
    wide = _plan_without_device()
    wide.elem32, wide.elem_bytes, wide.limbs64, wide.dtype = False, 32, 4, torch.int64
    with pytest.raises(ValueError, match="Goldilocks plan or a plan of 4-byte elements"):
        wide.set_poseidon2(7, 8, 13, ext, irc, diag)


def test_calls_before_the_parameters_are_refused():
    pl = _plan_without_device()
    with pytest.raises(ValueError, match="set_poseidon2 must be called first"):
        pl.poseidon2_permute(_mat(1, T))
    with pytest.raises(ValueError, match="set_poseidon2 must be called first"):
        pl.merkle_commit(_mat(64, 3), 3, _mat(127, D))
    with pytest.raises(ValueError, match="set_poseidon2 must be called first"):
        pl.merkle_open(_mat(64, 3), 3, _mat(127, D), torch.zeros(2, dtype=torch.int32), _mat(2, 3), _mat(12, D))


def test_poseidon2_permute_refuses_bad_arguments_before_the_library():
    pl = _set_plan()
    for bad in (_mat(1, T, torch.int64), _mat(2, T)[::2], [0] * T, None):
        with pytest.raises(ValueError, match="contiguous"):
            pl.poseidon2_permute(bad)
    for bad in (_mat(0, T), _mat(1, T - 1), _mat(1, T + 1)):
        with pytest.raises(ValueError, match="multiple of 16"):
            pl.poseidon2_permute(bad)
    with pytest.raises(ValueError, match="device"):
        pl.poseidon2_permute(_mat(3, T))  # everything right but a host tensor


def test_merkle_commit_refuses_bad_arguments_before_the_library():
    pl = _set_plan()
    mat, tree = _mat(64, 5), _mat(127, D)
    for bad in (0, -1, 5.0, "5", True, None):
        with pytest.raises(ValueError, match="width"):
            pl.merkle_commit(mat, bad, tree)
    with pytest.raises(ValueError, match="below 2\\^32"):
        pl.merkle_commit(mat, 1 << 26, tree)
    for lr in (7, -1, 2.0, "6", True):
        with pytest.raises(ValueError, match="log_rows"):
            pl.merkle_commit(mat, 5, tree, log_rows=lr)
    with pytest.raises(ValueError, match="mat: expected 64 rows of 5"):
        pl.merkle_commit(_mat(64, 4), 5, tree)
    with pytest.raises(ValueError, match="mat: expected 16 rows of 5"):
        pl.merkle_commit(mat, 5, _mat(31, D), log_rows=4)
    with pytest.raises(ValueError, match="tree: expected 127 rows of 8"):
        pl.merkle_commit(mat, 5, _mat(128, D))
    with pytest.raises(ValueError, match="tree: expected 1 rows of 8"):
        pl.merkle_commit(_mat(1, 5), 5, _mat(2, D), log_rows=0)
    with pytest.raises(ValueError, match="contiguous"):
        pl.merkle_commit(_mat(64, 5, torch.int64), 5, tree)
    with pytest.raises(ValueError, match="contiguous"):
        pl.merkle_commit(mat, 5, _mat(127, D, torch.int64))
    both = _mat(64 * 5 + 127 * D, 1)
    with pytest.raises(ValueError, match="mat and tree overlap"):
        pl.merkle_commit(both[:320], 5, both[312:312 + 127 * D])
    with pytest.raises(ValueError, match="device"):
        pl.merkle_commit(mat, 5, tree)  # everything right but host tensors


def test_merkle_open_refuses_bad_arguments_before_the_library():
    pl = _set_plan()
    mat, tree, idx = _mat(64, 5), _mat(127, D), torch.zeros(3, dtype=torch.int32)
    rows, paths = _mat(3, 5), _mat(3 * 6, D)
    for bad in (0, -1, 5.0, "5", True, None):
        with pytest.raises(ValueError, match="width"):
            pl.merkle_open(mat, bad, tree, idx, rows, paths)
    for lr in (7, -1, 2.0, "6", True):
        with pytest.raises(ValueError, match="log_rows"):
            pl.merkle_open(mat, 5, tree, idx, rows, paths, log_rows=lr)
    with pytest.raises(ValueError, match="both"):
        pl.merkle_open(mat, 5, tree, idx, None, paths)
    with pytest.raises(ValueError, match="both"):
        pl.merkle_open(None, 5, tree, idx, rows, paths)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)[::2],
                [0, 1, 2], None):
        with pytest.raises(ValueError, match="index"):
            pl.merkle_open(mat, 5, tree, bad, rows, paths)
    with pytest.raises(ValueError, match="tree: expected 127 rows of 8"):
        pl.merkle_open(mat, 5, _mat(126, D), idx, rows, paths)
    with pytest.raises(ValueError, match="paths: expected 18 rows of 8"):
        pl.merkle_open(mat, 5, tree, idx, rows, _mat(17, D))
    with pytest.raises(ValueError, match="rows_out: expected 3 rows of 5"):
        pl.merkle_open(mat, 5, tree, idx, _mat(4, 5), paths)
    with pytest.raises(ValueError, match="mat: expected 64 rows of 5"):
        pl.merkle_open(_mat(63, 5), 5, tree, idx, rows, paths)
    with pytest.raises(ValueError, match="tree and paths overlap"):
        pl.merkle_open(None, 5, tree, idx, None, tree[:3 * 6 * D])
    with pytest.raises(ValueError, match="mat and rows_out overlap"):
        pl.merkle_open(mat, 5, tree, idx, mat[:15], paths)
    with pytest.raises(ValueError, match="device"):
        pl.merkle_open(mat, 5, tree, idx, rows, paths)  # everything right but host tensors
    with pytest.raises(ValueError, match="device"):
        pl.merkle_open(None, 5, tree, idx, None, paths)


def test_merkle_info_refuses_bad_arguments_before_the_library():
    pl = _plan_without_device()  # the shape alone: no parameters needed
    for bad in (0, -1, 5.0, "5", True, None):
        with pytest.raises(ValueError, match="width"):
            pl.merkle_info(bad)
    for lr in (7, -1, 2.0, "6", True):
        with pytest.raises(ValueError, match="log_rows"):
            pl.merkle_info(5, log_rows=lr)
    with pytest.raises(ValueError, match="below 2\\^32"):
        pl.merkle_info(1 << 26)
