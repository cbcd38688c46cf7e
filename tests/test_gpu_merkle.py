"""The Poseidon2 Merkle calls on the GPU (NTTPlan.set_poseidon2 / poseidon2_permute / merkle_commit / merkle_open),
bit for bit against tests/poseidon2_ref.py, the restatement of include/ntt.h's definitions (its numpy path at these
shapes; tests/test_poseidon2_host.py holds that path to the integer one), on BabyBear (degree 7), KoalaBear (3),
Goldilocks (7) and the custom 4-byte prime of tests/test_gpu_matrix.py (5), with seeded random canonical
parameters at the usual round counts and one degenerate set (rounds_f = 2, rounds_p = 1).

Every commit case first runs an unrelated matrix transform on the plan, writes into a poisoned tree with 64
poisoned elements on each side, and compares the matrix with a copy afterwards; the whole tree is compared."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import poseidon2_ref as R
from tests import test_gpu_matrix as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

LOG_N = 12
FIELDS = [4, 5, 3, "p31"]
SHAPES = {4: (16, 7, 8, 13), 5: (16, 3, 8, 20), 3: (8, 7, 8, 22), "p31": (16, 5, 8, 13)}  # t, degree, rounds_f, rounds_p
PAD = 64
_PARAMS, _TREES = {}, {}


def _p2(fid, degenerate=False):
    key = (fid, degenerate)
    if key not in _PARAMS:
        t, a, rf, rp = SHAPES[fid]
        if degenerate:
            rf, rp = 2, 1
        _PARAMS[key] = R.seeded_params(T._params(fid)[0], t, a, rf, rp, 900 + 2 * FIELDS.index(fid) + degenerate)
    return _PARAMS[key]


def _plan(fid, degenerate=False, **kw):
    """The plan with the parameter set installed (set_poseidon2 replaces the previous one)."""
    pl = T._plan(fid, LOG_N, **kw)
    P = _p2(fid, degenerate)
    pl.set_poseidon2(P.alpha, P.rounds_f, P.rounds_p, P.ext_rc, P.int_rc, P.int_diag)
    return pl, P


def _padded(pl, count):
    """A poisoned buffer of count elements with PAD poisoned elements on each side: (whole, the middle)."""
    whole = torch.full((count + 2 * PAD,), T.POISON32 if pl.elem32 else T.POISON64, dtype=pl.dtype, device="cuda:0")
    return whole, whole[PAD:PAD + count]


def _pads_intact(pl, whole, count):
    poison = T.POISON32 if pl.elem32 else T.POISON64
    return bool((whole[:PAD] == poison).all()) and bool((whole[PAD + count:] == poison).all())


def _scratch_noise(pl, seed):
    """An unrelated matrix transform on the plan: its scratch and tables hold another call's data."""
    x = T._dev(T._rand(pl.p, pl.n, 3, seed), pl)
    pl.forward_matrix(x, 3)


def _commit(pl, P, mat_host, log_rows, width):
    rows, d = 1 << log_rows, P.d
    _scratch_noise(pl, 50 + log_rows)
    mat = T._dev(mat_host, pl)
    keep = mat.clone()
    whole, tree = _padded(pl, (2 * rows - 1) * d)
    assert pl.merkle_commit(mat, width, tree, log_rows=log_rows) is tree
    torch.cuda.synchronize()
    assert torch.equal(mat, keep), "the matrix was modified"
    assert _pads_intact(pl, whole, (2 * rows - 1) * d), "a store outside the tree"
    return T._host(tree, 2 * rows - 1, d), tree, mat


def _want_tree(fid, degenerate, mat_host):
    return R.tree_many(mat_host, _p2(fid, degenerate))


# ------------------------------------------------------------------------------------------------ permute
@pytest.mark.parametrize("degenerate", [False, True])
@pytest.mark.parametrize("fid", FIELDS)
def test_permute_matches_the_oracle(fid, degenerate):
    pl, P = _plan(fid, degenerate)
    for count in (1, 63, 64, 65, 1000):
        host = T._rand(pl.p, count, P.t, 10 + count)
        whole, st = _padded(pl, count * P.t)
        st.copy_(T._dev(host, pl))
        assert pl.poseidon2_permute(st) is st
        torch.cuda.synchronize()
        assert _pads_intact(pl, whole, count * P.t)
        assert np.array_equal(T._host(st, count, P.t), R.permute_many(host, P)), (fid, count)


# ------------------------------------------------------------------------------------------------ commit
def _commit_shapes(fid):
    d = SHAPES[fid][0] // 2
    tail = T._plan(fid, LOG_N).merkle_info(5)[3]
    assert 2 <= tail <= LOG_N - 2, tail
    shapes = [(0, 1), (1, 3), (3, d), (4, d + 1), (5, 2 * d), (6, 2 * d + 1), (7, 37), (2, 600), (10, 113), (6, 64)]
    shapes += [(tail + k, 5) for k in (-1, 0, 1, 2)]  # across the hand-over from the per-layer launches to the LDS tail
    return shapes


@pytest.mark.parametrize("fid", FIELDS)
def test_commit_matches_the_oracle_tree(fid):
    pl, P = _plan(fid)
    full_tail = pl.merkle_info(5)[3]
    for log_rows, width in _commit_shapes(fid):
        host = T._rand(pl.p, 1 << log_rows, width, 20 + log_rows)
        got, _, _ = _commit(pl, P, host, log_rows, width)
        want = _want_tree(fid, False, host)
        assert got.shape == want.shape
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (fid, log_rows, width, "first wrong nodes", bad[:8])
        d, elems, launches, tail = pl.merkle_info(width, log_rows=log_rows)
        assert (d, elems) == (P.d, ((2 << log_rows) - 1) * P.d)
        assert tail == min(log_rows, full_tail)
        assert launches == 1 + (log_rows - tail) + (1 if log_rows else 0)


@pytest.mark.parametrize("fid", [4, 3])
def test_commit_with_the_degenerate_rounds(fid):
    pl, P = _plan(fid, degenerate=True)
    for log_rows, width in ((4, P.d + 1), (10, 5)):
        host = T._rand(pl.p, 1 << log_rows, width, 31 + log_rows)
        got, _, _ = _commit(pl, P, host, log_rows, width)
        assert np.array_equal(got, _want_tree(fid, True, host)), (fid, log_rows, width)


def test_commit_at_an_unaligned_address():
    """Element-aligned pointers: the matrix and the tree 4 bytes off a 16-byte boundary take the element accesses."""
    pl, P = _plan(4)
    log_rows, width = 6, 12
    host = T._rand(pl.p, 1 << log_rows, width, 77)
    mat = torch.zeros(host.size + 1, dtype=pl.dtype, device="cuda:0")[1:]
    mat.copy_(T._dev(host, pl))
    tree = torch.zeros(127 * P.d + 3, dtype=pl.dtype, device="cuda:0")[3:]
    assert mat.data_ptr() % 16 and tree.data_ptr() % 16
    pl.merkle_commit(mat, width, tree, log_rows=log_rows)
    assert np.array_equal(T._host(tree, 127, P.d), _want_tree(4, False, host))


def test_launch_labels():
    pl, P = _plan(4)
    tail = pl.merkle_info(5)[3]
    host = T._rand(pl.p, 1 << (tail + 2), 5, 5)
    mat = T._dev(host, pl)
    tree = torch.zeros(((2 << (tail + 2)) - 1) * P.d, dtype=pl.dtype, device="cuda:0")
    idx = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    calls = (lambda: pl.merkle_commit(mat, 5, tree, log_rows=tail + 2),
             lambda: pl.merkle_open(mat, 5, tree, idx, torch.zeros(15, dtype=pl.dtype, device="cuda:0"),
                                    torch.zeros(3 * (tail + 2) * P.d, dtype=pl.dtype, device="cuda:0"), log_rows=tail + 2),
             lambda: pl.poseidon2_permute(torch.zeros(4 * P.t, dtype=pl.dtype, device="cuda:0")))
    got = []
    for call in calls:
        pl.set_profiling(True)
        call()
        got.append(pl.last_launch_labels())
        pl.set_profiling(False)
    assert got == [["h", "m1", "m1", f"m{tail}"], ["g"], ["p"]], got


# ------------------------------------------------------------------------------------------------ Montgomery plans
@pytest.mark.parametrize("fid", [4, "p31"])
def test_montgomery_tree_is_the_canonical_tree_times_r(fid):
    pl, P = _plan(fid, montgomery_io=True)
    p, r = pl.p, (1 << 32) % pl.p
    for log_rows, width in ((5, 2 * P.d + 1), (10, 5)):
        host = T._rand(p, 1 << log_rows, width, 41 + log_rows)
        mont = (host * np.uint64(r)) % np.uint64(p)
        got, _, _ = _commit(pl, P, mont, log_rows, width)
        want = (_want_tree(fid, False, host) * np.uint64(r)) % np.uint64(p)
        assert np.array_equal(got, want), (fid, log_rows, width)
    host = T._rand(p, 65, P.t, 43)
    st = T._dev((host * np.uint64(r)) % np.uint64(p), pl)
    pl.poseidon2_permute(st)
    assert np.array_equal(T._host(st, 65, P.t), (R.permute_many(host, P) * np.uint64(r)) % np.uint64(p))


# ------------------------------------------------------------------------------------------------ open
@pytest.mark.parametrize("fid", FIELDS)
def test_open_rows_and_paths(fid):
    pl, P = _plan(fid)
    log_rows, width = 7, 11
    rows, d = 1 << log_rows, P.d
    host = T._rand(pl.p, rows, width, 61)
    tree_host, tree, mat = _commit(pl, P, host, log_rows, width)
    root = [int(v) for v in tree_host[-1]]
    assert root == [int(v) for v in _want_tree(fid, False, host)[-1]]
    for nq in (1, 7, 300):
        rng = np.random.default_rng(70 + nq)
        index = rng.integers(0, rows, size=nq, dtype=np.int64)
        fixed = [0, rows - 1, 5, 5, rows + 9, 0x7FFFFFFF, 0xFFFFFFFF][:nq]  # the ends, a duplicate, three >= N
        index[:len(fixed)] = fixed
        idx = torch.from_numpy(index.astype(np.uint32).view(np.int32)).to("cuda:0")
        wr, rows_out = _padded(pl, nq * width)
        wp, paths = _padded(pl, nq * log_rows * d)
        keep_tree = tree.clone()
        pl.merkle_open(mat, width, tree, idx, rows_out, paths, log_rows=log_rows)
        torch.cuda.synchronize()
        assert _pads_intact(pl, wr, nq * width) and _pads_intact(pl, wp, nq * log_rows * d)
        assert torch.equal(tree, keep_tree)
        eff = index & (rows - 1)
        assert np.array_equal(T._host(rows_out, nq, width), host[eff])
        got_paths = T._host(paths, nq * log_rows, d).reshape(nq, log_rows, d)
        for q in range(nq):
            for l in range(log_rows):
                node = R.layer_start(log_rows, l) + ((int(eff[q]) >> l) ^ 1)
                assert np.array_equal(got_paths[q, l], tree_host[node]), (fid, nq, q, l)
        for q in range(min(nq, 7)):  # the oracle's leaf hash and compress reach the root
            path = [[int(v) for v in got_paths[q, l]] for l in range(log_rows)]
            row = [int(v) for v in T._host(rows_out, nq, width)[q]]
            assert R.root_from_path(row, int(eff[q]), path, P) == root, (fid, nq, q)
        wp2, paths2 = _padded(pl, nq * log_rows * d)  # the paths alone
        pl.merkle_open(None, width, tree, idx, None, paths2, log_rows=log_rows)
        assert torch.equal(paths2, paths) and _pads_intact(pl, wp2, nq * log_rows * d)


def test_open_of_a_single_row_tree():
    pl, P = _plan(4)
    host = T._rand(pl.p, 1, 9, 3)
    _, tree, mat = _commit(pl, P, host, 0, 9)
    idx = torch.tensor([0, 5], dtype=torch.int32, device="cuda:0")
    rows_out = torch.zeros(18, dtype=pl.dtype, device="cuda:0")
    pl.merkle_open(mat, 9, tree, idx, rows_out, torch.zeros(0, dtype=pl.dtype, device="cuda:0"), log_rows=0)
    assert np.array_equal(T._host(rows_out, 2, 9), np.concatenate([host, host]))


# ------------------------------------------------------------------------------------------------ library refusals
def test_the_library_refuses_what_the_python_layer_would():
    import ctypes as C
    from ntt_amd import lib as L
    from ntt_amd.ntt import NTTPlan, _u64_array
    pl, P = _plan(4)
    so, h = pl._lib, pl._h
    mat = T._dev(T._rand(pl.p, 16, 5, 1), pl)
    whole, tree = _padded(pl, 31 * P.d)
    vp = lambda t: C.c_void_p(t.data_ptr())
    idx = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    rows_out, paths = torch.zeros(10, dtype=pl.dtype, device="cuda:0"), torch.zeros(2 * 4 * P.d, dtype=pl.dtype, device="cuda:0")
    E = L.NTT_ERR_ARG
    assert so.ntt_merkle_commit(h, None, 5, 4, vp(tree), None) == E
    assert so.ntt_merkle_commit(h, vp(mat), 5, 4, None, None) == E
    assert so.ntt_merkle_commit(h, vp(mat), 0, 4, vp(tree), None) == E
    assert so.ntt_merkle_commit(h, vp(mat), 5, LOG_N + 1, vp(tree), None) == E
    assert so.ntt_merkle_commit(h, vp(mat), 1 << 20, 12, vp(tree), None) == E
    assert so.ntt_merkle_commit(h, vp(mat), 5, 4, vp(mat), None) == E  # the tree over the matrix
    assert so.ntt_poseidon2_permute(h, None, 1, None) == E
    assert so.ntt_poseidon2_permute(h, vp(tree), 0, None) == E
    assert so.ntt_merkle_open(h, vp(mat), 5, 4, vp(tree), vp(idx), 0, vp(rows_out), vp(paths), None) == E
    assert so.ntt_merkle_open(h, vp(mat), 5, 4, vp(tree), vp(idx), 2, None, vp(paths), None) == E
    assert so.ntt_merkle_open(h, None, 5, 4, vp(tree), vp(idx), 2, vp(rows_out), vp(paths), None) == E
    assert so.ntt_merkle_open(h, vp(mat), 5, 4, vp(tree), None, 2, vp(rows_out), vp(paths), None) == E
    assert so.ntt_merkle_open(h, vp(mat), 5, 4, None, vp(idx), 2, vp(rows_out), vp(paths), None) == E
    assert so.ntt_merkle_open(h, vp(mat), 5, 4, vp(tree), vp(idx), 2, vp(rows_out), None, None) == E
    assert so.ntt_merkle_open(h, vp(mat), 5, 4, vp(tree), vp(idx), 2, vp(rows_out), vp(tree), None) == E
    ext, irc, diag = _u64_array(P.flat_ext()), _u64_array(P.int_rc), _u64_array(P.int_diag)
    for width, a, rf, rp in ((8, 7, 8, 13), (16, 3, 8, 13), (16, 5, 8, 13), (16, 4, 8, 13), (16, 7, 7, 13), (16, 7, 0, 13),
                             (16, 7, 18, 13), (16, 7, 8, 65)):
        assert so.ntt_plan_set_poseidon2(h, width, a, rf, rp, ext, irc, diag) == E, (width, a, rf, rp)
    bad = P.flat_ext()
    bad[17] = pl.p
    assert so.ntt_plan_set_poseidon2(h, 16, P.alpha, P.rounds_f, P.rounds_p, _u64_array(bad), irc, diag) == E
    assert so.ntt_plan_set_poseidon2(h, 16, P.alpha, P.rounds_f, P.rounds_p, None, irc, diag) == E
    torch.cuda.synchronize()
    assert _pads_intact(pl, whole, 31 * P.d) and bool((tree == T.POISON32).all()), "a refused call wrote"
    # the refused sets left the installed one in place
    host = T._rand(pl.p, 16, 5, 1)
    assert np.array_equal(_commit(pl, P, host, 4, 5)[0], _want_tree(4, False, host))
    # before the parameters, on engines without the calls, on twiddle-only plans
    fresh = NTTPlan(4, 5, 1)
    assert so.ntt_merkle_commit(fresh._h, vp(mat), 5, 4, vp(tree), None) == E
    assert so.ntt_poseidon2_permute(fresh._h, vp(tree), 1, None) == E
    bn = NTTPlan(1, 5, 4)
    assert so.ntt_plan_set_poseidon2(bn._h, 16, 7, 8, 13, ext, irc, diag) == E
    tw = NTTPlan(4, 5, 1, twiddle_only=True)
    assert so.ntt_plan_set_poseidon2(tw._h, 16, P.alpha, P.rounds_f, P.rounds_p, ext, irc, diag) == E


# ------------------------------------------------------------------------------------------------ the pipeline
def test_29_bit_engines_refuse_the_calls():
    """A plan of another engine answers NTT_ERR_ARG to every hashing call, writes no byte of any buffer and leaves
    the info call's outputs as they were."""
    import ctypes as C
    from ntt_amd import lib as Lb
    from ntt_amd.ntt import NTTPlan
    so = Lb.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    u64 = lambda vals: (C.c_uint64 * len(vals))(*vals)
    width, rows, nq, t, rf, rp = 5, 64, 3, 16, 8, 13  # well-formed arguments for the 4-byte fields' width 16
    ext_rc, int_rc, int_diag = u64(range(1, rf * t + 1)), u64(range(1, rp + 1)), u64(range(2, t + 2))
    for pl, words in ((NTTPlan(1, 10, 4), 4), (NTTPlan(0, 10, 1), 1)):  # BN254, P469762049
        assert so.ntt_plan_set_poseidon2(pl._h, t, 7, rf, rp, ext_rc, int_rc, int_diag) == Lb.NTT_ERR_ARG
        sizes = {"states": 4 * t, "mat": rows * width, "tree": (2 * rows - 1) * (t // 2), "rows": nq * width,
                 "paths": nq * 6 * (t // 2)}
        buf = {k: torch.full((n * words,), 1 + i, dtype=torch.int64, device="cuda:0") for i, (k, n) in enumerate(sizes.items())}
        index = torch.tensor([0, 5, 63], dtype=torch.int32, device="cuda:0")
        keep = {k: x.clone() for k, x in buf.items()}
        ptr = {k: C.c_void_p(x.data_ptr()) for k, x in buf.items()}
        assert so.ntt_poseidon2_permute(pl._h, ptr["states"], 4, st) == Lb.NTT_ERR_ARG
        assert so.ntt_merkle_commit(pl._h, ptr["mat"], width, 6, ptr["tree"], st) == Lb.NTT_ERR_ARG
        assert so.ntt_merkle_open(pl._h, ptr["mat"], width, 6, ptr["tree"], C.c_void_p(index.data_ptr()), nq, ptr["rows"],
                                  ptr["paths"], st) == Lb.NTT_ERR_ARG
        d, te, la, tl = C.c_uint(77), C.c_uint64(78), C.c_uint(79), C.c_uint(80)
        assert so.ntt_merkle_info(pl._h, width, 6, C.byref(d), C.byref(te), C.byref(la), C.byref(tl)) == Lb.NTT_ERR_ARG
        assert (d.value, te.value, la.value, tl.value) == (77, 78, 79, 80)
        torch.cuda.synchronize()
        for k, x in buf.items():
            assert torch.equal(x, keep[k]), k
        assert index.tolist() == [0, 5, 63]


@pytest.mark.parametrize("fid,d,w", [(4, 4, 11), (3, 2, 7)])
def test_pipeline_extension_commit_fold_commit(fid, d, w):
    """lde_matrix(bitrev_out) -> commit; fri_fold -> commit of the [M >> k][d << k] view: both roots against the
    oracle on the buffers the library produced."""
    pl, P = _plan(fid)
    L, blow, k = 10, 1, 2
    p, g = T._params(fid)
    coeffs = T._dev(T._rand(p, 1 << (L - blow), d, 81), T._plan(fid, L))
    big = T._plan(fid, L)
    ev = torch.zeros((1 << L) * d, dtype=pl.dtype, device="cuda:0")
    big.lde_matrix(coeffs, ev, blow, shift=g, width=d, bitrev_out=True)
    tree = torch.zeros(((2 << L) - 1) * P.d, dtype=pl.dtype, device="cuda:0")
    pl.merkle_commit(ev, d, tree, log_rows=L)
    assert np.array_equal(T._host(tree, (2 << L) - 1, P.d)[-1], R.tree_many(T._host(ev, 1 << L, d), P)[-1])
    M = 1 << (L - 1)
    folded = torch.zeros(M * d, dtype=pl.dtype, device="cuda:0")
    beta = [int(v) for v in T._rand(p, 1, d, 82)[0]]
    big.fri_fold(ev, folded, 1, beta, ext_degree=d, ext_w=w, shift=g)
    lr, width = L - 1 - k, d << k  # the layer as the next fold of arity 2^k reads it: a fibre per row
    tree2 = torch.zeros(((2 << lr) - 1) * P.d, dtype=pl.dtype, device="cuda:0")
    pl.merkle_commit(folded, width, tree2, log_rows=lr)
    assert np.array_equal(T._host(tree2, (2 << lr) - 1, P.d)[-1], R.tree_many(T._host(folded, 1 << lr, width), P)[-1])


# ------------------------------------------------------------------------------------------------ the caller's stream
def _stream_cases(eng):
    from tests import test_gpu_streams as S
    fid = S.ENGINES[eng][0]
    pl, P = _plan(fid)
    log_rows, width, nq = 11, 37, 9
    rows, d, tag = 1 << log_rows, P.d, f"{eng} merkle 2^{log_rows}x{width}"
    spec = lambda count: S._spec(pl, count)
    mat = lambda seed: S._rand(pl, rows * width, seed)

    def tree_of(seed):  # the tree of that seed's matrix, computed on the default stream
        key = (eng, "tree", seed)
        if key not in _TREES:
            t = torch.zeros((2 * rows - 1) * d, dtype=pl.dtype, device="cuda:0")
            pl.merkle_commit(mat(seed), width, t, log_rows=log_rows)
            torch.cuda.synchronize()
            _TREES[key] = t
        return _TREES[key]

    def index(seed):
        key = (eng, "idx", seed)
        if key not in _TREES:
            _TREES[key] = torch.from_numpy(np.random.default_rng(seed).integers(0, rows, size=nq).astype(np.int32)).to("cuda:0")
        return _TREES[key]

    def chain(i, o, s):
        pl.merkle_commit(i[0], width, o[0], log_rows=log_rows, stream=s)
        pl.merkle_open(i[0], width, o[0], i[1], o[1], o[2], log_rows=log_rows, stream=s)

    return [
        S.Case(f"{tag} commit", lambda seed: [mat(seed)], [spec((2 * rows - 1) * d)],
               lambda i, o, s: pl.merkle_commit(i[0], width, o[0], log_rows=log_rows, stream=s), const=(0,)),
        S.Case(f"{tag} open", lambda seed: [mat(seed), tree_of(seed), index(seed)], [spec(nq * width), spec(nq * log_rows * d)],
               lambda i, o, s: pl.merkle_open(i[0], width, i[1], i[2], o[0], o[1], log_rows=log_rows, stream=s),
               const=(0, 1, 2)),
        S.Case(f"{tag} permute", lambda seed: [S._rand(pl, 1000 * P.t, seed)], [],
               lambda i, o, s: pl.poseidon2_permute(i[0], stream=s)),
        S.Case(f"{tag} commit and open chained", lambda seed: [mat(seed), index(seed)],
               [spec((2 * rows - 1) * d), spec(nq * width), spec(nq * log_rows * d)], chain, const=(0, 1)),
    ]


@pytest.mark.parametrize("eng", ["goldilocks", "babybear", "p31"])
def test_merkle_calls_run_on_the_callers_stream(eng):
    from tests import test_gpu_streams as S
    S._need_sleep()
    S._run_all(_stream_cases(eng))


def test_stream_want_is_the_oracles():
    from tests import test_gpu_streams as S
    S._need_sleep()
    case = _stream_cases("babybear")[0]
    bad, rec = S._problems(case)
    assert not bad, bad
    pl, P = _plan(4)
    host = T._host(case.make(S.REAL)[0], 1 << 11, 37)
    assert np.array_equal(T._host(rec.want[0], (2 << 11) - 1, P.d), R.tree_many(host, P))


# ------------------------------------------------------------------------------------------------ the checked build
CHILD = r'''
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ntt_amd import lib as L
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
from tests import poseidon2_ref as R
from tests import test_gpu_matrix as T
from tests import test_gpu_merkle as M
for fid in (4, 3):
    pl, P = M._plan(fid)
    for log_rows, width in ((4, P.d + 1), (11, 37)):
        host = T._rand(pl.p, 1 << log_rows, width, 5)
        got, tree, mat = M._commit(pl, P, host, log_rows, width)
        assert np.array_equal(got, R.tree_many(host, P)), (fid, log_rows)
        idx = torch.tensor([0, 3, (1 << log_rows) - 1, 1 << 30], dtype=torch.int32, device="cuda:0")
        rows = torch.zeros(4 * width, dtype=pl.dtype, device="cuda:0")
        paths = torch.zeros(4 * log_rows * P.d, dtype=pl.dtype, device="cuda:0")
        pl.merkle_open(mat, width, tree, idx, rows, paths, log_rows=log_rows)
        st = T._dev(T._rand(pl.p, 65, P.t, 6), pl)
        pl.poseidon2_permute(st)
        s = pl.device_status()
        assert s == 0, (fid, log_rows, hex(s))
    bad = host.copy()
    bad[37, width - 1] = pl.p  # one non-canonical matrix element
    M._commit(pl, P, bad, log_rows, width)
    s = pl.device_status()
    assert s == 0x200, (fid, "commit: non-canonical input", hex(s))
    assert pl.device_status() == 0
print("MERKLE-DEBUG-OK")
'''


def test_checked_build_reports_clean_status():
    """Commits, an open and a permute on both engines through the checked build in a fresh process: right trees and
    no bounds / canonical report; a matrix with one element equal to p reports 0x200."""
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "MERKLE-DEBUG-OK" in r.stdout
