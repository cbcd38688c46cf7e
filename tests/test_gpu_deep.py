"""The DEEP calls on the GPU (NTTPlan.deep_points / open_matrix / deep_quotient), bit-exact against the
coefficient-domain definition and never against the kernels' own barycentric form: the columns are random
coefficient vectors, the matrix is the oracle's coset evaluations of each column (tests/test_gpu_matrix.py's
_expected), row-permuted as the fold tests build theirs; an opening is Horner's evaluation of the coefficients
at z in Python integers over F_p[X]/(X^d - W); a quotient is the synthetic division of
P = scale sum_j alpha^j p_j by X - z (by linearity the same polynomial as scale sum_j alpha^j q_j with
q_j = (p_j - p_j(z)) / (X - z)), evaluated by the oracle on the same coset in the same row order.  Fields and
extensions as the fold's EXTS, both row orders, shift None and non-trivial, plans of log_n 12 with log_rows
from 0 up to it.  Every case first runs an unrelated matrix transform on the plan, writes into a poisoned
buffer with 64 poisoned elements on each side, and compares every input with a clone afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_gpu_fold as F
from tests import test_gpu_matrix as T
from tests import test_gpu_matrix_ex as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

LOG_N = 12
PAD = 64
EXTS = F.EXTS
# (log_rows, width): one row; two rows narrower than anything; one strip of one workgroup step; several strips
# with a masked last one and a table longer than its LDS part at (4, 600); the plan's own size at a width
# below and above a wave, with a masked strip
SHAPES = [(0, 1), (1, 3), (5, 16), (6, 300), (12, 37), (12, 113), (4, 600)]

_MAT, _COEF, _HORNER = {}, {}, {}


def _configs(i, L, g):
    """(shift, bitrev) pairs of shape number i: all four combinations over the shapes; one at the plan's size."""
    both = [(None, True), (g, False)] if i % 2 == 0 else [(g, True), (None, False)]
    return both[:1] if L == LOG_N else both


def _coef(fid, L, W):
    key = (fid, L, W)
    if key not in _COEF:
        p, _ = T._params(fid)
        _COEF[key] = T._rand(p, 1 << L, W, 9000 + 100 * L + W)
    return _COEF[key]


def _rows(L, bitrev):
    return X._perm(L) if bitrev else np.arange(1 << L)


def _matrix(fid, L, W, c, bitrev):
    key = (fid, L, W, c, bitrev)
    if key not in _MAT:
        p, g = T._params(fid)
        _MAT[key] = np.ascontiguousarray(T._expected(_coef(fid, L, W), p, g, c, L)[_rows(L, bitrev)])
    return _MAT[key]


def _z(fid, d, L, c, seed):
    """A seeded point off the domain (d = 1: a base-field point with z^N != c^N)."""
    p, _ = T._params(fid)
    rng = np.random.default_rng(seed)
    while True:
        z = [int(v) for v in rng.integers(0, p, size=d, dtype=np.uint64)]
        if any(z[1:]) or pow(z[0], 1 << L, p) != pow(c, 1 << L, p):
            return z


def _vec_mul_scalar(a, z, w, p):
    """a z for a = [W][d] (object array), z one extension element."""
    d = a.shape[1]
    out = np.zeros_like(a)
    for i in range(d):
        for j in range(d):
            if z[j] == 0:
                continue
            t = a[:, i] * z[j]
            if i + j < d:
                out[:, i + j] += t
            else:
                out[:, i + j - d] += t * w
    return out % p


def _horner(fid, d, w, L, W, z):
    """p_j(z) for every column j: Horner over the rows of the coefficients, vectorised over the columns."""
    key = (fid, d, L, W, tuple(z))
    if key not in _HORNER:
        p, _ = T._params(fid)
        a = _coef(fid, L, W).astype(object)
        acc = np.zeros((W, d), dtype=object)
        for k in range((1 << L) - 1, -1, -1):
            acc = _vec_mul_scalar(acc, z, w, p)
            acc[:, 0] = (acc[:, 0] + a[k]) % p
        _HORNER[key] = acc
    return _HORNER[key]


def _ext_pows(alpha, count, w, p, scale):
    out, cur = [], list(scale)
    for _ in range(count):
        out.append(cur)
        cur = F._ext_mul(cur, alpha, w, p)
    return np.array(out, dtype=object).reshape(count, len(alpha))


def _quotient_coeffs(fid, d, w, L, W, z, alpha, scale):
    """[N][d]: the coefficients of (P - P(z)) / (X - z), P = sum_j (scale alpha^j) p_j, by synthetic division."""
    p, _ = T._params(fid)
    N = 1 << L
    wts = _ext_pows(alpha, W, w, p, scale)                   # [W][d]
    P = _coef(fid, L, W).astype(object).dot(wts) % p         # [N][d]: base coefficients times extension weights
    q = np.zeros((N, d), dtype=object)
    b = [0] * d
    for k in range(N - 1, 0, -1):                            # b_k = P_k + z b_{k+1}; q_{k-1} = b_k
        b = [(x + y) % p for x, y in zip(F._ext_mul(b, z, w, p), P[k])]
        q[k - 1] = b
    return q.astype(np.uint64)


def _expected_quotient(fid, d, w, L, W, c, bitrev, z, alpha, scale):
    p, g = T._params(fid)
    q = _quotient_coeffs(fid, d, w, L, W, z, alpha, scale or ([1] + [0] * (d - 1)))
    return T._expected(q, p, g, c, L)[_rows(L, bitrev)]


def _buf(pl, count, off=0):
    """`count` elements in the middle of a poisoned allocation, `off` elements past the padding."""
    big = T._poisoned(pl, count + 2 * PAD + off)
    return big, big[PAD + off:PAD + off + count]


def _check_poison(pl, big, count, off=0):
    poison = T.POISON32 if pl.elem32 else T.POISON64
    assert bool((big[:PAD + off] == poison).all()) and bool((big[PAD + off + count:] == poison).all()), "poison around the output"


def _dev(x, pl, off=0):
    """x on the device, `off` elements into its allocation (an odd offset: not 16-byte aligned)."""
    t = T._dev(x, pl)
    if not off:
        return t
    hold = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    hold[off:].copy_(t)
    return hold[off:]


def _to_io(x, pl):
    """Canonical values -> the plan's I/O form."""
    if not pl.montgomery_io:
        return x
    return (x.astype(object) * ((1 << 32) % pl.p) % pl.p).astype(np.uint64)


def _plain_inv(inv, pl):
    """ntt_deep_points' working form -> plain values (object array)."""
    if not pl.elem32:
        return inv.astype(object)
    return inv.astype(object) * pow(1 << 32, -1, pl.p) % pl.p


def _points(pl, d, w, L, z, shift, bitrev, off=0, dirty=True):
    if dirty:
        T._dirty(pl, 3)
    big, inv = _buf(pl, (1 << L) * d, off)
    pl.deep_points(inv, z, ext_degree=d, ext_w=w or 0, shift=shift, bitrev=bitrev, log_rows=L)
    _check_poison(pl, big, (1 << L) * d, off)
    return inv


def _open(pl, mat, W, inv, d, w, L, z, shift, bitrev, off=0):
    keep_m, keep_i = mat.clone(), inv.clone()
    T._dirty(pl, 3)
    big, val = _buf(pl, W * d, off)
    pl.open_matrix(mat, W, inv, val, z, ext_degree=d, ext_w=w or 0, shift=shift, bitrev=bitrev, log_rows=L)
    _check_poison(pl, big, W * d, off)
    assert torch.equal(mat, keep_m) and torch.equal(inv, keep_i), "an input was modified"
    return val


def _quot(pl, mat, W, inv, val, d, w, L, alpha, scale, off=0, into=None):
    keep = [t.clone() for t in (mat, inv, val)]
    T._dirty(pl, 3)
    if into is None:
        big, out = _buf(pl, (1 << L) * d, off)
    else:
        big, out = into
    pl.deep_quotient(mat, W, inv, val, out, alpha, scale=scale, accumulate=into is not None, ext_degree=d, ext_w=w or 0,
                     log_rows=L)
    _check_poison(pl, big, (1 << L) * d, off)
    for t, k in zip((mat, inv, val), keep):
        assert torch.equal(t, k), "an input was modified"
    return big, out


def _alphas(p, d, seed):
    rng = np.random.default_rng(seed)
    return [[int(v) for v in rng.integers(0, p, size=d, dtype=np.uint64)], [0] * d, [1] + [0] * (d - 1), [p - 1] * d]


@pytest.mark.parametrize("fid,d,w", EXTS)
def test_points_are_the_inverses_of_z_minus_x(fid, d, w):
    """(z - x_i) inv_i = 1 for every row, one Python extension product per row after undoing the working form:
    one row, two, less than a thread's run on a larger plan, several workgroups' worth and the plan's own size
    (both table levels); both orders, every shift; an odd element offset; a base-field z off the coset."""
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    wN = {L: pow(g, (p - 1) >> L, p) for L in (0, 1, 5, 9, 12)}
    for li, L in enumerate((0, 1, 5, 9, 12)):
        for shift, bitrev in _configs(li, -1, g) + [(p - 1, True)][:L == 5]:
            c = X._one(shift)
            zs = [_z(fid, d, L, c, 11 * L + d)]
            if d > 1 and L in (1, 5):
                zs.append(_z(fid, 1, L, c, 5 + L) + [0] * (d - 1))  # a base-field z off the coset
            for z in zs:
                off = 1 if L == 5 else 0
                inv = _points(pl, d, w, L, z, shift, bitrev, off)
                if off:
                    assert inv.data_ptr() % 16 != 0
                got = _plain_inv(T._host(inv, 1 << L, d), pl)
                x, xs = c, []
                for _ in range(1 << L):
                    xs.append(x)
                    x = x * wN[L] % p
                for i, r in enumerate(_rows(L, bitrev)):
                    dif = [(z[0] - xs[r]) % p] + z[1:]
                    assert F._ext_mul(dif, [int(v) for v in got[i]], w, p) == [1] + [0] * (d - 1), (fid, d, L, shift, bitrev, i)


@pytest.mark.parametrize("fid,d,w", [(4, 4, 11), (3, 1, None), ("p31", 2, T.G31)])
def test_a_base_field_point_of_the_coset_is_refused(fid, d, w):
    from ntt_amd import lib as Lb
    import ctypes as C
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    L = 5
    so = Lb.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x7 = g * pow(g, 7 * ((p - 1) >> L), p) % p  # g w_N^7
    big, inv = _buf(pl, (1 << L) * d)
    keep = big.clone()
    z = (C.c_uint64 * 4)(x7, 0, 0, 0)
    sh = (C.c_uint64 * 1)(g)
    for order in (0, 1):
        assert so.ntt_deep_points(pl._h, C.c_void_p(inv.data_ptr()), L, d, w or 0, z, sh, order, st) == Lb.NTT_ERR_ARG
    z1 = (C.c_uint64 * 4)(pow(g, 3 * ((p - 1) >> L), p), 0, 0, 0)  # on <w_N> itself
    assert so.ntt_deep_points(pl._h, C.c_void_p(inv.data_ptr()), L, d, w or 0, z1, None, 1, st) == Lb.NTT_ERR_ARG
    mat = T._dev(_matrix(fid, L, 16, g, True), pl)
    vb, val = _buf(pl, 16 * d)
    keepv = vb.clone()
    assert so.ntt_matrix_open(pl._h, C.c_void_p(mat.data_ptr()), 16, L, C.c_void_p(inv.data_ptr()), d, w or 0, z, sh, 1,
                              C.c_void_p(val.data_ptr()), st) == Lb.NTT_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(big, keep) and torch.equal(vb, keepv)
    with pytest.raises(ValueError, match="domain"):
        pl.deep_points(inv, [x7] + [0] * (d - 1), ext_degree=d, ext_w=w or 0, shift=g, log_rows=L)
    # the same point on another coset is fine
    pl.deep_points(inv, [x7] + [0] * (d - 1), ext_degree=d, ext_w=w or 0, shift=None, log_rows=L)
    torch.cuda.synchronize()


def test_shape_decisions_cover_both_sides():
    """deep_info at the shapes below: an open of one chunk and of several; at least two lane counts per engine."""
    for fid in (3, 4):
        pl = T._plan(fid, LOG_N)
        info = {s: pl.deep_info(s[1], log_rows=s[0], ext_degree=2) for s in SHAPES}
        assert info[(5, 16)][0] == 1 and info[(0, 1)][0] == 1
        assert info[(12, 37)][0] > 1 and info[(12, 113)][0] > 1 and info[(6, 300)][0] > 1
        least = 16 if pl.elem32 else 8  # 64 B of lanes
        assert info[(1, 3)][1] == 1 and info[(0, 1)][1] == 1 and info[(5, 16)][1] == least and info[(12, 37)][1] == least
        assert info[(12, 113)][1] == 16 and info[(6, 300)][1] == 64 and info[(4, 600)][1] == 64
        assert len({v[1] for v in info.values()}) >= 3


@pytest.mark.parametrize("si", range(len(SHAPES)))
@pytest.mark.parametrize("fid,d,w", EXTS)
def test_open_is_horner_evaluation_and_quotient_is_synthetic_division(fid, d, w, si):
    """values[j] = p_j(z) by Horner; two consecutive opens give the same bits; the quotient equals the oracle's
    evaluations of the synthetic division, with a random alpha and scale (and an odd element offset at one
    shape); at the smaller shapes also alpha in {0, 1, all p - 1} with scale None."""
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    L, W = SHAPES[si]
    for ci, (shift, bitrev) in enumerate(_configs(si, L, g)):
        c = X._one(shift)
        z = _z(fid, d, L, c, 100 * L + W + d)
        off = 1 if (L, W) == (5, 16) and ci == 0 else 0
        mat = _dev(_matrix(fid, L, W, c, bitrev), pl, off)
        inv = _points(pl, d, w, L, z, shift, bitrev, off)
        val = _open(pl, mat, W, inv, d, w, L, z, shift, bitrev, off)
        want = _horner(fid, d, w, L, W, z).astype(np.uint64)
        assert np.array_equal(T._host(val, W, d), want), (fid, d, L, W, shift, bitrev)
        again = _open(pl, mat, W, inv, d, w, L, z, shift, bitrev, off)
        assert torch.equal(val, again), "two opens differ"
        alphas = _alphas(p, d, 7 * L + W)
        cases = [(alphas[0], _alphas(p, d, 3 * L + W + 1)[0])]
        if L <= 6:
            cases += [(a, None) for a in alphas]
        for alpha, scale in cases:
            _, out = _quot(pl, mat, W, inv, val, d, w, L, alpha, scale, off)
            exp = _expected_quotient(fid, d, w, L, W, c, bitrev, z, alpha, scale)
            assert np.array_equal(T._host(out, 1 << L, d), exp), (fid, d, L, W, shift, bitrev, alpha, scale)


@pytest.mark.parametrize("fid,d,w", [(4, 4, 11), (3, 2, 7)])
def test_accumulate_sums_two_opening_points(fid, d, w):
    """Two calls into one buffer, the second with NTT_DEEP_ACCUMULATE, scale alpha^W and another z, equal the
    Python sum of the two quotients."""
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    L, W, shift, bitrev = 6, 300, g, True
    mat = T._dev(_matrix(fid, L, W, g, bitrev), pl)
    alpha = _alphas(p, d, 77)[0]
    scale2 = [int(v) for v in _ext_pows(alpha, W + 1, w, p, [1] + [0] * (d - 1))[W]]
    total, into = np.zeros(((1 << L), d), dtype=object), None
    for zi, scale in ((0, None), (1, scale2)):
        z = _z(fid, d, L, g, 500 + zi)
        inv = _points(pl, d, w, L, z, shift, bitrev)
        val = _open(pl, mat, W, inv, d, w, L, z, shift, bitrev)
        into = _quot(pl, mat, W, inv, val, d, w, L, alpha, scale, into=into)
        total = (total + _expected_quotient(fid, d, w, L, W, g, bitrev, z, alpha, scale).astype(object)) % p
    assert np.array_equal(T._host(into[1], 1 << L, d), total.astype(np.uint64))


def test_montgomery_io_keeps_the_data_form():
    """BabyBear with NTT_PLAN_MONTGOMERY_IO: a Montgomery-form matrix with canonical z, alpha, scale and shift
    gives the same inverses (the working form does not depend on the plan kind) and the Montgomery form of the
    expected values and quotient."""
    fid, d, w = 4, 4, 11
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N, montgomery_io=True)
    plain = T._plan(fid, LOG_N)
    for L, W in ((5, 16), (12, 37)):
        shift, bitrev = g, True
        z = _z(fid, d, L, g, 900 + L)
        mat = T._dev(_to_io(_matrix(fid, L, W, g, bitrev), pl), pl)
        inv = _points(pl, d, w, L, z, shift, bitrev)
        assert torch.equal(inv, _points(plain, d, w, L, z, shift, bitrev))
        val = _open(pl, mat, W, inv, d, w, L, z, shift, bitrev)
        assert np.array_equal(T._host(val, W, d), _to_io(_horner(fid, d, w, L, W, z).astype(np.uint64), pl))
        alpha, scale = _alphas(p, d, 901)[0], _alphas(p, d, 902)[0]
        _, out = _quot(pl, mat, W, inv, val, d, w, L, alpha, scale)
        assert np.array_equal(T._host(out, 1 << L, d), _to_io(_expected_quotient(fid, d, w, L, W, g, bitrev, z, alpha, scale), pl))


@pytest.mark.parametrize("fid,d,w", [(4, 4, 11), (3, 2, 7)])
def test_pipeline_from_the_extension_to_the_fold(fid, d, w):
    """lde_matrix (width 5, n = 2^6 coefficients to N = 2^9, bit-reversed rows) -> deep_points -> open_matrix ->
    deep_quotient -> fri_fold chained to total arity 2^6: Q has degree < n - 1, so the 8 remaining rows are
    equal; with one word of `values` off by one Q is no polynomial of that degree and the rows differ."""
    p, g = T._params(fid)
    L, Ls, W = 9, 6, 5
    pl = T._plan(fid, L)
    a = T._rand(p, 1 << Ls, W, 4242 + d)
    ev = T._poisoned(pl, (1 << L) * W)
    pl.lde_matrix(T._dev(a, pl), ev, L - Ls, g, W, bitrev_out=True)
    z = _z(fid, d, L, g, 4243)
    inv = _points(pl, d, w, L, z, g, True, dirty=False)
    val = _open(pl, ev, W, inv, d, w, L, z, g, True)
    alpha = _alphas(p, d, 4244)[0]
    betas = _alphas(p, d, 4245)

    def folded(values):
        _, q = _quot(pl, ev, W, inv, values, d, w, L, alpha, None)
        cur, rows, c = q, L, g
        for k, beta in ((4, betas[0]), (2, betas[3])):
            nxt = T._poisoned(pl, (1 << (rows - k)) * d)
            pl.fri_fold(cur, nxt, k, beta, ext_degree=d, ext_w=w, shift=c, log_rows=rows)
            cur, rows, c = nxt, rows - k, pow(c, 1 << k, p)
        return T._host(cur, 1 << rows, d)

    good = folded(val)
    assert good.shape[0] == 8 and bool((good == good[0]).all()), good
    bad_val = val.clone()
    bad_val[2] ^= 1  # one word off by one (seeded data: the word is not p - 1, so it stays canonical)
    assert pl.count_noncanonical(bad_val) == 0
    bad = folded(bad_val)
    assert not bool((bad == bad[0]).all())


def test_argument_errors_leave_the_buffers_untouched():
    import ctypes as C
    from ntt_amd import lib as Lb
    so = Lb.load()
    p, g = T._params(4)
    log_n, d, w, W = 10, 4, 11, 8
    pl = T._plan(4, log_n)
    tw = T._plan(4, log_n, twiddle_only=True)
    n = pl.n
    mat = T._dev(T._rand(p, n, W, 1), pl)
    inv = T._dev(T._rand(p, n, d, 2), pl)
    val = T._dev(T._rand(p, W, d, 3), pl)
    out = T._poisoned(pl, n * d)
    keeps = [t.clone() for t in (mat, inv, val, out)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    z, sh = u64(1, 2, 3, 4), u64(g)
    pts, opn, quo = so.ntt_deep_points, so.ntt_matrix_open, so.ntt_deep_quotient
    cases = [
        # points: null pointers, log_rows, ext_degree, ext_w, z, shift, order, twiddle-only
        pts(pl._h, None, log_n, d, w, z, sh, 0, st), pts(pl._h, P(out), log_n, d, w, None, sh, 0, st),
        pts(pl._h, P(out), log_n + 1, d, w, z, sh, 0, st), pts(pl._h, P(out), log_n, 3, w, z, sh, 0, st),
        pts(pl._h, P(out), log_n, 0, w, z, sh, 0, st), pts(pl._h, P(out), log_n, d, 0, z, sh, 0, st),
        pts(pl._h, P(out), log_n, d, p, z, sh, 0, st), pts(pl._h, P(out), log_n, d, w, u64(1, 2, 3, p), sh, 0, st),
        pts(pl._h, P(out), log_n, d, w, z, u64(0), 0, st), pts(pl._h, P(out), log_n, d, w, z, u64(p), 0, st),
        pts(pl._h, P(out), log_n, d, w, z, sh, 2, st), pts(pl._h, P(out), log_n, d, w, z, sh, 4, st),
        pts(tw._h, P(out), log_n, d, w, z, sh, 0, st),
        # open: null pointers, width 0, N width >= 2^32, the scalars, overlap of values with mat and with inv
        opn(pl._h, None, W, log_n, P(inv), d, w, z, sh, 0, P(out), st), opn(pl._h, P(mat), W, log_n, None, d, w, z, sh, 0, P(out), st),
        opn(pl._h, P(mat), W, log_n, P(inv), d, w, None, sh, 0, P(out), st), opn(pl._h, P(mat), W, log_n, P(inv), d, w, z, sh, 0, None, st),
        opn(pl._h, P(mat), 0, log_n, P(inv), d, w, z, sh, 0, P(out), st),
        opn(pl._h, P(mat), 1 << 22, log_n, P(inv), d, w, z, sh, 0, P(out), st),
        opn(pl._h, P(mat), W, log_n + 1, P(inv), d, w, z, sh, 0, P(out), st), opn(pl._h, P(mat), W, log_n, P(inv), 5, w, z, sh, 0, P(out), st),
        opn(pl._h, P(mat), W, log_n, P(inv), d, p + 1, z, sh, 0, P(out), st),
        opn(pl._h, P(mat), W, log_n, P(inv), d, w, u64(p, 0, 0, 0), sh, 0, P(out), st),
        opn(pl._h, P(mat), W, log_n, P(inv), d, w, z, u64(1 << 40), 0, P(out), st), opn(pl._h, P(mat), W, log_n, P(inv), d, w, z, sh, 2, P(out), st),
        opn(pl._h, P(mat), W, log_n, P(inv), d, w, z, sh, 0, P(mat, 4 * (n * W - 1)), st),
        opn(pl._h, P(mat), W, log_n, P(inv), d, w, z, sh, 0, P(inv, 4 * (n * d - 1)), st),
        opn(tw._h, P(mat), W, log_n, P(inv), d, w, z, sh, 0, P(out), st),
        # quotient: null pointers (scale may be null), flags, the scalars, overlap of out with each input
        quo(pl._h, None, W, log_n, P(inv), P(val), d, w, z, None, 0, P(out), st), quo(pl._h, P(mat), W, log_n, None, P(val), d, w, z, None, 0, P(out), st),
        quo(pl._h, P(mat), W, log_n, P(inv), None, d, w, z, None, 0, P(out), st), quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, None, None, 0, P(out), st),
        quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, z, None, 0, None, st), quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, z, None, 2, P(out), st),
        quo(pl._h, P(mat), 0, log_n, P(inv), P(val), d, w, z, None, 0, P(out), st),
        quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, u64(1, p, 0, 0), None, 0, P(out), st),
        quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, z, u64(0, 0, 0, p + 7), 1, P(out), st),
        quo(pl._h, P(mat), W, log_n, P(inv), P(val), 2, 0, z, None, 0, P(out), st),
        quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, z, None, 0, P(mat, 4 * (n * W - 1)), st),
        quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, z, None, 0, P(inv), st),
        quo(pl._h, P(mat), W, log_n, P(inv), P(val), d, w, z, None, 0, P(val, 4 * (W * d - 1)), st),
        quo(tw._h, P(mat), W, log_n, P(inv), P(val), d, w, z, None, 0, P(out), st),
    ]
    assert cases == [Lb.NTT_ERR_ARG] * len(cases), cases
    chunks, lanes = C.c_uint(9), C.c_uint(9)
    info = so.ntt_deep_info
    bad = [info(pl._h, 0, log_n, d, C.byref(chunks), C.byref(lanes)), info(pl._h, W, log_n + 1, d, C.byref(chunks), C.byref(lanes)),
           info(pl._h, W, log_n, 3, C.byref(chunks), C.byref(lanes)), info(pl._h, 1 << 22, log_n, d, C.byref(chunks), C.byref(lanes)),
           info(pl._h, W, log_n, d, None, C.byref(lanes)), info(pl._h, W, log_n, d, C.byref(chunks), None)]
    assert bad == [Lb.NTT_ERR_ARG] * len(bad) and (chunks.value, lanes.value) == (9, 9)
    torch.cuda.synchronize()
    for t, k in zip((mat, inv, val, out), keeps):
        assert torch.equal(t, k)


def test_29_bit_engines_refuse_the_deep_calls():
    import ctypes as C
    from ntt_amd import lib as Lb
    from ntt_amd.ntt import NTTPlan
    so = Lb.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = (C.c_uint64 * 4)(5, 0, 0, 0)
    for pl, words in ((NTTPlan(1, 10, 4), 4), (NTTPlan(0, 10, 1), 1)):  # BN254, P469762049
        t = [torch.full((pl.n * words,), 1 + i, dtype=torch.int64, device="cuda:0") for i in range(4)]
        keep = [x.clone() for x in t]
        a, b, c, o = (C.c_void_p(x.data_ptr()) for x in t)
        chunks, lanes = C.c_uint(), C.c_uint()
        assert so.ntt_deep_points(pl._h, o, 10, 1, 0, z, None, 0, st) == Lb.NTT_ERR_ARG
        assert so.ntt_matrix_open(pl._h, a, 1, 10, b, 1, 0, z, None, 0, o, st) == Lb.NTT_ERR_ARG
        assert so.ntt_deep_quotient(pl._h, a, 1, 10, b, c, 1, 0, z, None, 0, o, st) == Lb.NTT_ERR_ARG
        assert so.ntt_deep_info(pl._h, 1, 10, 1, C.byref(chunks), C.byref(lanes)) == Lb.NTT_ERR_ARG
        torch.cuda.synchronize()
        for x, k in zip(t, keep):
            assert torch.equal(x, k)


def test_profiling_labels_the_launches():
    fid, d, w, L, W = 4, 4, 11, 9, 16
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    z = _z(fid, d, L, g, 31)
    mat = T._dev(T._rand(p, 1 << L, W, 5), pl)
    inv, val, out = (T._poisoned(pl, k * d) for k in (1 << L, W, 1 << L))
    got = []
    for call in (lambda: pl.deep_points(inv, z, ext_degree=d, ext_w=w, shift=g, bitrev=True, log_rows=L),
                 lambda: pl.open_matrix(mat, W, inv, val, z, ext_degree=d, ext_w=w, shift=g, bitrev=True, log_rows=L),
                 lambda: pl.deep_quotient(mat, W, inv, val, out, z, ext_degree=d, ext_w=w, log_rows=L)):
        pl.set_profiling(True)
        call()
        got.append(pl.last_launch_labels())
        pl.set_profiling(False)
    assert got == [["z"], ["o", "e"], ["a", "q"]], got


CHILD = r'''
import sys
sys.path.insert(0, ROOT)
import numpy as np
from ntt_amd import lib as L
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
from tests import test_gpu_matrix as T
from tests import test_gpu_deep as D
for fid, d, w in ((3, 2, 7), (4, 4, 11)):
    p, g = T._params(fid)
    pl = T._plan(fid, D.LOG_N)
    for Lr, W in ((5, 16), (12, 37)):
        z = D._z(fid, d, Lr, g, 77)
        m = D._matrix(fid, Lr, W, g, True)
        mat = T._dev(m, pl)
        inv = D._points(pl, d, w, Lr, z, g, True)
        val = D._open(pl, mat, W, inv, d, w, Lr, z, g, True)
        assert np.array_equal(T._host(val, W, d), D._horner(fid, d, w, Lr, W, z).astype(np.uint64)), (fid, Lr)
        alpha = D._alphas(p, d, 78)[0]
        _, out = D._quot(pl, mat, W, inv, val, d, w, Lr, alpha, None)
        assert np.array_equal(T._host(out, 1 << Lr, d), D._expected_quotient(fid, d, w, Lr, W, g, True, z, alpha, None)), (fid, Lr)
        st = pl.device_status()
        assert st == 0, (fid, Lr, hex(st))
    bad = m.copy()
    bad[37, W - 1] = p  # one non-canonical matrix element
    D._open(pl, T._dev(bad, pl), W, inv, d, w, Lr, z, g, True)
    st = pl.device_status()
    assert st == 0x200, (fid, "open: non-canonical input", hex(st))
    D._quot(pl, T._dev(bad, pl), W, inv, val, d, w, Lr, alpha, None)
    st = pl.device_status()
    assert st & 0x200 and not st & 0x100, (fid, "quotient: non-canonical input", hex(st))
    assert pl.device_status() == 0
print("DEEP-DEBUG-OK")
'''


def test_checked_build_reports_clean_status():
    """An open and a quotient on both engines through the checked build in a fresh process: right results and no
    bounds / canonical report; a matrix with one element equal to p reports 0x200."""
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "DEEP-DEBUG-OK" in r.stdout
