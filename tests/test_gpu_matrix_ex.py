"""The matrix calls on a coset and in bit-reversed row order on the GPU (NTTPlan.forward_matrix(shift=,
bitrev_out=), inverse_matrix(shift=, bitrev_in=), lde_matrix(bitrev_out=), lde_matrix_from_evals(in_shift=,
bitrev_out=); ntt_*_matrix_ex): bit-exact against the oracle's transform of each column taken out on the
host -- oracle/ntt_ref.py coset_ntt / coset_intt up to 2^5, oracle_c.ntt_mp with mul_mp by host powers of
c / c^-1 above -- with the rows permuted on the host.

Fields, sizes and helpers are those of tests/test_gpu_matrix.py: Goldilocks, BabyBear, KoalaBear and a
custom 4-byte-element prime; log_n 0, 1, 2 (no pass kernel), 3, 5, the largest size of one pass and the
smallest of two (and of three, at width 3), from the schedule the calls report.  Every case first runs an
unrelated matrix transform on the plan, and an extension writes into a poisoned `out`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_gpu_matrix as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

FIELDS = T.FIELDS
WIDTHS = (1, 3, 16, 17, 37)  # narrower than a strip, one strip, one over, a masked remainder

_EXP = {}


def _perm(log_n):
    """perm[i] = the log_n-bit reversal of i: stored = natural[perm] both ways (an involution)."""
    i = np.arange(1 << log_n, dtype=np.uint64)
    r = np.zeros_like(i)
    for b in range(log_n):
        r |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(log_n - 1 - b)
    return r.astype(np.int64)


def _x(p, log_n, width):
    return T._rand(p, 1 << log_n, width, 100 * log_n + width)


def _forward(fid, log_n, width, c):
    """The oracle's evaluations of the columns of _x on c <w_n> in natural order (c = 1: the plain forward)."""
    key = (fid, log_n, width, c, "f")
    if key not in _EXP:
        p, g = T._params(fid)
        _EXP[key] = T._expected(_x(p, log_n, width), p, g, c, log_n)
    return _EXP[key]


def _expected_inverse(X, p, g, c, log_n):
    """out[j][b] = c^-j INTT(column b of X)_j, X in natural order."""
    from oracle import ntt_ref as R
    from oracle import oracle_c as OC
    N, width = X.shape
    if c == 1:
        return T._expected(X, p, g, 1, log_n, inverse=True)
    if log_n <= 5:
        out = np.zeros_like(X)
        for b in range(width):
            out[:, b] = np.array(R.coset_intt([int(v) for v in X[:, b]], p, g, c), dtype=np.uint64)
        return out
    base = T._expected(X, p, g, 1, log_n, inverse=True)
    pw = np.repeat(T._powers(pow(c, p - 2, p), N, p), width)
    return OC.mul_mp(base.reshape(-1, 1), pw.reshape(-1, 1), p).reshape(N, width)


def _inverse(fid, log_n, width, c):
    key = (fid, log_n, width, c, "i")
    if key not in _EXP:
        p, g = T._params(fid)
        _EXP[key] = _expected_inverse(_x(p, log_n, width), p, g, c, log_n)
    return _EXP[key]


def _shifts(fid):
    p, g = T._params(fid)
    return (None, g, p - 1)


def _one(c):
    return 1 if c is None else c


@pytest.mark.parametrize("which", range(7))
@pytest.mark.parametrize("fid", FIELDS)
def test_forward_and_inverse_on_cosets_and_in_bit_reversed_order(fid, which):
    """shift in {None, g, p - 1} x order in {0, the call's flag}, forward and inverse; the call without
    options equals the plain call."""
    sizes = T._log_ns(fid)
    if which >= len(sizes):
        return  # fewer distinct sizes than slots: nothing left to check
    log_n = sizes[which]
    p, g = T._params(fid)
    pl = T._plan(fid, log_n)
    perm = _perm(log_n)
    for width in WIDTHS:
        x = _x(p, log_n, width)
        for c in _shifts(fid):
            for rev in (False, True):
                T._dirty(pl, width)
                t = T._dev(x, pl)
                pl.forward_matrix(t, width, shift=c, bitrev_out=rev)
                exp = _forward(fid, log_n, width, _one(c))
                assert np.array_equal(T._host(t, pl.n, width), exp[perm] if rev else exp), (fid, log_n, width, c, rev,
                                                                                            "forward")
                T._dirty(pl, width)
                t = T._dev(x[perm] if rev else x, pl)
                pl.inverse_matrix(t, width, shift=c, bitrev_in=rev)
                assert np.array_equal(T._host(t, pl.n, width), _inverse(fid, log_n, width, _one(c))), (
                    fid, log_n, width, c, rev, "inverse")
        a, b = T._dev(x, pl), T._dev(x, pl)
        assert torch.equal(pl.forward_matrix(a, width, shift=None, bitrev_out=False), pl.forward_matrix(b, width))
        a, b = T._dev(x, pl), T._dev(x, pl)
        assert torch.equal(pl.inverse_matrix(a, width, shift=None, bitrev_in=False), pl.inverse_matrix(b, width))


def _ex_raw(so, name, pl, t, width, shift, order):
    """The _ex symbol itself (shift None and order 0 included, which the Python layer routes to the plain call)."""
    sh = None if shift is None else (C.c_uint64 * 1)(shift)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return getattr(so, name)(pl._h, C.c_void_p(t.data_ptr()), width, sh, order, st)


@pytest.mark.parametrize("fid", FIELDS)
def test_ex_symbols_without_options_are_the_plain_calls(fid):
    from ntt_amd import lib as L
    so = L.load()
    p, g = T._params(fid)
    width = 37
    for log_n in (2, T._size(fid, width, 1, largest=True), T._size(fid, width, 2)):
        pl = T._plan(fid, log_n)
        x = _x(p, log_n, width)
        for name, plain in (("ntt_forward_matrix_ex", pl.forward_matrix), ("ntt_inverse_matrix_ex", pl.inverse_matrix)):
            a, b = T._dev(x, pl), T._dev(x, pl)
            assert _ex_raw(so, name, pl, a, width, None, 0) == L.NTT_OK
            assert torch.equal(a, plain(b, width)), (fid, log_n, name)
        lb = 1
        src = T._dev(x[:pl.n >> lb], pl)
        a, b = T._poisoned(pl, pl.n * width), T._poisoned(pl, pl.n * width)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert so.ntt_lde_matrix_ex(pl._h, C.c_void_p(src.data_ptr()), C.c_void_p(a.data_ptr()), lb, (C.c_uint64 * 1)(g),
                                    width, 0, st) == L.NTT_OK
        assert torch.equal(a, pl.lde_matrix(src, b, lb, g, width)), (fid, log_n, "lde")


@pytest.mark.parametrize("fid", [3, 4])
def test_smallest_three_pass_size(fid):
    """A middle pass between the permuted load and the permuted store."""
    width = 3
    log_n = T._size(fid, width, 3)
    p, g = T._params(fid)
    pl = T._plan(fid, log_n)
    assert len(pl.matrix_passes(width)) == 3
    perm = _perm(log_n)
    x = _x(p, log_n, width)
    T._dirty(pl, width)
    t = T._dev(x, pl)
    pl.forward_matrix(t, width, shift=g, bitrev_out=True)
    assert np.array_equal(T._host(t, pl.n, width), _forward(fid, log_n, width, g)[perm])
    T._dirty(pl, width)
    t = T._dev(x[perm], pl)
    pl.inverse_matrix(t, width, shift=g, bitrev_in=True)
    assert np.array_equal(T._host(t, pl.n, width), _inverse(fid, log_n, width, g))


@pytest.mark.parametrize("fid", FIELDS)
def test_round_trip(fid):
    """inverse_ex(forward_ex(x, c, BITREV_OUT), c, BITREV_IN) == x"""
    p, g = T._params(fid)
    for log_n in T._log_ns(fid):
        pl = T._plan(fid, log_n)
        for width in (3, 37):
            x = _x(p, log_n, width)
            for c in (g, p - 1):
                T._dirty(pl, width)
                t = T._dev(x, pl)
                pl.forward_matrix(t, width, shift=c, bitrev_out=True)
                pl.inverse_matrix(t, width, shift=c, bitrev_in=True)
                assert np.array_equal(T._host(t, pl.n, width), x), (fid, log_n, width, c)


def _lde_rev(pl, x, log_blowup, shift, width):
    """One bit-reversed extension on dirtied scratch into a poisoned `out`; checks that d_in is unchanged."""
    t_in = T._dev(x, pl)
    keep = t_in.clone()
    T._dirty(pl, width)
    out = T._poisoned(pl, pl.n * width)
    pl.lde_matrix(t_in, out, log_blowup, shift, width, bitrev_out=True)
    assert torch.equal(t_in, keep), "d_in was modified"
    return T._host(out, pl.n, width)


@pytest.mark.parametrize("width", [3, 16, 37])
@pytest.mark.parametrize("fid", FIELDS)
def test_lde_in_bit_reversed_order(fid, width):
    """Against the permuted oracle, and the prefix property: the first n = N >> log_blowup rows are the small
    plan's coset forward in its own bit-reversed order (bitrev_N(i) = bitrev_n(i) << log_blowup for i < n)."""
    p, g = T._params(fid)
    for log_n in (2, 5, T._size(fid, width, 1, largest=True), T._size(fid, width, 2)):
        pl = T._plan(fid, log_n)
        perm = _perm(log_n)
        passes = pl.matrix_passes(width)
        r1 = passes[0] if passes else log_n
        x = T._rand(p, pl.n, width, 1000 * log_n + width)
        for lb in sorted({b for b in (0, 1, 3, r1 + 1, log_n) if b <= log_n}):
            small = T._plan(fid, log_n - lb)
            for shift in (None, g, p - 1):
                coeffs = x[:pl.n >> lb]
                got = _lde_rev(pl, coeffs, lb, shift, width)
                exp = T._expected(coeffs, p, g, _one(shift), log_n)
                assert np.array_equal(got, exp[perm]), (fid, log_n, width, lb, shift)
                t = T._dev(coeffs, small)
                small.forward_matrix(t, width, shift=shift, bitrev_out=True)
                assert np.array_equal(got[:small.n], T._host(t, small.n, width)), (fid, log_n, width, lb, shift, "prefix")


@pytest.mark.parametrize("fid", FIELDS)
def test_lde_matrix_from_evals_on_a_coset(fid):
    from ntt_amd.ntt import lde_matrix_from_evals
    p, g = T._params(fid)
    width, big_log = 37, T._size(fid, 37, 2)
    small, big = T._plan(fid, big_log - 3), T._plan(fid, big_log)
    c_in = p - 1
    evals = T._rand(p, small.n, width, 5)
    coeffs = _expected_inverse(evals, p, g, c_in, small.log_n)
    t, out = T._dev(evals, small), T._poisoned(big, big.n * width)
    T._dirty(big, width)
    lde_matrix_from_evals(small, big, t, out, g, width, in_shift=c_in, bitrev_out=True)
    assert np.array_equal(T._host(t, small.n, width), coeffs)
    assert np.array_equal(T._host(out, big.n, width), T._expected(coeffs, p, g, g, big_log)[_perm(big_log)])


@pytest.mark.parametrize("fid", [3, 4])
def test_no_extra_launch(fid):
    """The labels of a shifted, bit-reversed inverse and forward are matrix_passes' labels: n, s<r> or c.. f.."""
    p, g = T._params(fid)
    width = 37
    for log_n in (2, T._size(fid, width, 1, largest=True), T._size(fid, width, 2), T._size(fid, width, 2) + 3):
        pl = T._plan(fid, log_n)
        passes = pl.matrix_passes(width)
        if not passes:
            want = ["n"]
        elif len(passes) == 1:
            want = [f"s{passes[0]}"]
        else:
            want = [f"c{r}" for r in passes[:-1]] + [f"f{passes[-1]}"]
        t = T._dev(_x(p, log_n, width), pl)
        pl.forward_matrix(t, width, shift=g)  # the shift's tables are built: not part of the record below
        for call, kw in ((pl.inverse_matrix, dict(shift=g, bitrev_in=True)), (pl.forward_matrix, dict(shift=g, bitrev_out=True))):
            pl.set_profiling(True)
            call(t, width, **kw)
            labels = pl.last_launch_labels()
            ms = pl.last_launch_ms()
            pl.set_profiling(False)
            assert labels == want, (fid, log_n, labels, want)
            assert len(ms) == len(labels)


@pytest.mark.parametrize("fid", FIELDS)
def test_shift_cache_is_shared_and_replaced(fid):
    """One plan, the shifts alternating between the matrix calls and the vector coset call."""
    p, g = T._params(fid)
    width, log_n = 17, T._size(fid, 17, 2)
    pl = T._plan(fid, log_n)
    x = _x(p, log_n, width)
    t = T._dev(x, pl)
    pl.forward_matrix(t, width, shift=g)
    assert np.array_equal(T._host(t, pl.n, width), _forward(fid, log_n, width, g)), "forward g"
    t = T._dev(x, pl)
    pl.inverse_matrix(t, width, shift=p - 1)
    assert np.array_equal(T._host(t, pl.n, width), _inverse(fid, log_n, width, p - 1)), "inverse p - 1"
    got = T._lde(pl, x[:pl.n >> 1], 1, g, width)
    assert np.array_equal(got, T._expected(x[:pl.n >> 1], p, g, g, log_n)), "lde g"
    v = T._dev(x[:, :1], pl)
    pl.forward_coset(v, p - 1)
    assert np.array_equal(T._host(v, pl.n, 1), T._expected(x[:, :1], p, g, p - 1, log_n)), "vector forward_coset p - 1"
    t = T._dev(x, pl)
    pl.inverse_matrix(t, width, shift=g)
    assert np.array_equal(T._host(t, pl.n, width), _inverse(fid, log_n, width, g)), "inverse g"


@pytest.mark.parametrize("fid", [3, 4])
def test_permuted_rows_and_masked_strips_touch_nothing_outside_the_matrix(fid):
    """The matrix sits inside a larger poisoned allocation: the elements before and after it keep the poison
    through all three calls with shift and flag."""
    p, g = T._params(fid)
    width, pad = 37, 256
    for log_n in (T._size(fid, width, 1, largest=True), T._size(fid, width, 2)):
        pl = T._plan(fid, log_n)
        perm = _perm(log_n)
        count = pl.n * width
        poison = T.POISON32 if pl.elem32 else T.POISON64
        x = _x(p, log_n, width)
        big = T._poisoned(pl, count + 2 * pad)
        t = big[pad:pad + count]
        t.copy_(T._dev(x, pl))
        pl.forward_matrix(t, width, shift=g, bitrev_out=True)
        assert np.array_equal(T._host(t, pl.n, width), _forward(fid, log_n, width, g)[perm])
        pl.inverse_matrix(t, width, shift=g, bitrev_in=True)
        assert np.array_equal(T._host(t, pl.n, width), x)
        big2 = T._poisoned(pl, count + 2 * pad)
        lb = 2
        pl.lde_matrix(T._dev(x[:pl.n >> lb], pl), big2[pad:pad + count], lb, g, width, bitrev_out=True)
        assert np.array_equal(T._host(big2[pad:pad + count], pl.n, width),
                              T._expected(x[:pl.n >> lb], p, g, g, log_n)[perm])
        for buf in (big, big2):
            assert bool((buf[:pad] == poison).all()) and bool((buf[pad + count:] == poison).all()), (fid, log_n)


def test_montgomery_io_keeps_the_form():
    """BabyBear with NTT_PLAN_MONTGOMERY_IO (R = 2^32), the shift canonical: forward_ex(x R, c) =
    forward_ex(x, c) R, and the coset inverse too."""
    p, g = T._params(4)
    width, log_n = 17, T._size(4, 17, 2)
    pl = T._plan(4, log_n, montgomery_io=True)
    R = np.uint64((1 << 32) % p)
    x = _x(p, log_n, width)
    xr = x * R % np.uint64(p)
    t = T._dev(xr, pl)
    pl.forward_matrix(t, width, shift=g)
    assert np.array_equal(T._host(t, pl.n, width), _forward(4, log_n, width, g) * R % np.uint64(p))
    t = T._dev(xr, pl)
    pl.inverse_matrix(t, width, shift=g)
    assert np.array_equal(T._host(t, pl.n, width), _inverse(4, log_n, width, g) * R % np.uint64(p))


def test_argument_errors_leave_the_buffers_untouched():
    from ntt_amd import lib as L
    so = L.load()
    p, g = T._params(4)
    log_n, width = 10, 3
    pl = T._plan(4, log_n)
    tw = T._plan(4, log_n, twiddle_only=True)
    src = T._dev(T._rand(p, pl.n >> 1, width, 1), pl)
    out = T._poisoned(pl, pl.n * width)
    keep = out.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i, o = C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr())
    shift = lambda v: (C.c_uint64 * 1)(v)
    OUT, IN = L.NTT_MATRIX_BITREV_OUT, L.NTT_MATRIX_BITREV_IN
    fwd, inv, lde = so.ntt_forward_matrix_ex, so.ntt_inverse_matrix_ex, so.ntt_lde_matrix_ex
    cases = [
        # what the plain calls refuse
        fwd(pl._h, None, width, shift(g), OUT, st), fwd(pl._h, o, 0, shift(g), OUT, st),
        fwd(pl._h, o, 1 << 22, None, OUT, st), fwd(tw._h, o, width, shift(g), 0, st),
        inv(pl._h, None, width, shift(g), IN, st), inv(pl._h, o, 0, None, IN, st),
        inv(pl._h, o, 1 << 22, shift(g), 0, st), inv(tw._h, o, width, None, IN, st),
        lde(pl._h, None, o, 1, None, width, OUT, st), lde(pl._h, i, None, 1, None, width, OUT, st),
        lde(pl._h, i, o, 1, None, 0, OUT, st), lde(pl._h, i, o, 1, None, 1 << 22, OUT, st),
        lde(pl._h, i, o, log_n + 1, None, width, OUT, st), lde(pl._h, o, o, 1, None, width, OUT, st),
        lde(pl._h, C.c_void_p(out.data_ptr() + 4 * (pl.n * width - 1)), o, 1, None, width, OUT, st),
        lde(tw._h, i, o, 1, None, width, OUT, st),
        # unknown order bits
        fwd(pl._h, o, width, None, 4, st), fwd(pl._h, o, width, shift(g), OUT | 8, st),
        inv(pl._h, o, width, None, 4, st), inv(pl._h, o, width, shift(g), IN | 1 << 31, st),
        lde(pl._h, i, o, 1, None, width, 4, st), lde(pl._h, i, o, 1, shift(g), width, OUT | 16, st),
        # the other direction's flag
        fwd(pl._h, o, width, None, IN, st), fwd(pl._h, o, width, shift(g), IN | OUT, st),
        lde(pl._h, i, o, 1, None, width, IN, st), lde(pl._h, i, o, 1, shift(g), width, IN | OUT, st),
        inv(pl._h, o, width, None, OUT, st), inv(pl._h, o, width, shift(g), IN | OUT, st),
        # a bad shift
        fwd(pl._h, o, width, shift(0), 0, st), fwd(pl._h, o, width, shift(p), OUT, st),
        fwd(pl._h, o, width, shift(1 << 40), 0, st),
        inv(pl._h, o, width, shift(0), 0, st), inv(pl._h, o, width, shift(p), IN, st),
        lde(pl._h, i, o, 1, shift(0), width, OUT, st), lde(pl._h, i, o, 1, shift(p), width, OUT, st),
    ]
    assert cases == [L.NTT_ERR_ARG] * len(cases), cases
    torch.cuda.synchronize()
    assert torch.equal(out, keep)


def test_29_bit_engines_refuse_the_ex_calls():
    from ntt_amd import lib as L
    from ntt_amd.ntt import NTTPlan
    so = L.load()
    pl = NTTPlan(1, 10, 4)  # BN254
    t = torch.full((pl.n * 4,), 1, dtype=torch.int64, device="cuda:0")
    keep = t.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = C.c_void_p(t.data_ptr())
    sh = (C.c_uint64 * 4)(5, 0, 0, 0)
    for shift in (None, sh):
        assert so.ntt_forward_matrix_ex(pl._h, d, 1, shift, L.NTT_MATRIX_BITREV_OUT, st) == L.NTT_ERR_ARG
        assert so.ntt_forward_matrix_ex(pl._h, d, 1, shift, 0, st) == L.NTT_ERR_ARG
        assert so.ntt_inverse_matrix_ex(pl._h, d, 1, shift, L.NTT_MATRIX_BITREV_IN, st) == L.NTT_ERR_ARG
        assert so.ntt_lde_matrix_ex(pl._h, d, C.c_void_p(t.data_ptr() + 8 * 4 * 512), 1, shift, 1,
                                    L.NTT_MATRIX_BITREV_OUT, st) == L.NTT_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(t, keep)


CHILD = r'''
import sys
sys.path.insert(0, ROOT)
import numpy as np
from ntt_amd import lib as L
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
from tests import test_gpu_matrix as T
from tests import test_gpu_matrix_ex as X
width = 37
for fid in (3, 4):
    p, g = T._params(fid)
    log_n = T._size(fid, width, 2)
    pl = T._plan(fid, log_n)
    perm = X._perm(log_n)
    x = X._x(p, log_n, width)
    t = T._dev(x, pl)
    pl.forward_matrix(t, width, shift=g, bitrev_out=True)
    assert np.array_equal(T._host(t, pl.n, width), X._forward(fid, log_n, width, g)[perm]), (fid, "forward")
    st = pl.device_status()
    assert st == 0, (fid, "forward", hex(st))
    t = T._dev(x[perm], pl)
    pl.inverse_matrix(t, width, shift=g, bitrev_in=True)
    assert np.array_equal(T._host(t, pl.n, width), X._inverse(fid, log_n, width, g)), (fid, "inverse")
    st = pl.device_status()
    assert st == 0, (fid, "inverse", hex(st))
    lb = pl.matrix_passes(width)[0] + 1
    got = X._lde_rev(pl, x[:pl.n >> lb], lb, g, width)
    assert np.array_equal(got, T._expected(x[:pl.n >> lb], p, g, g, log_n)[perm]), (fid, "lde")
    st = pl.device_status()
    assert st == 0, (fid, "lde", hex(st))
print("MATRIX-EX-DEBUG-OK")
'''


def test_checked_build_reports_clean_status():
    """The two-pass size at width 37 (a masked last strip), all three calls with shift and flag, through the
    checked build in a fresh process: right results and no bounds / canonical / lazy-bound report."""
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "MATRIX-EX-DEBUG-OK" in r.stdout
