"""The FRI fold on the GPU (NTTPlan.fri_fold / ntt_fri_fold), bit-exact against the coefficient-domain
definition and never against the kernel's own form: with random coefficients a = [N][d], the input is the
oracle's evaluations of every coordinate column on c<w_N> with the rows bit-reversed
(tests/test_gpu_matrix.py's _expected, test_gpu_matrix_ex's _perm), g_m = sum_t beta^t a_{m 2^k + t} is
computed in Python integers over F_p[X]/(X^d - W), and the expected output is the oracle's evaluations of g
on c^(2^k)<w_M>, bit-reversed over L - k bits.  On Goldilocks, BabyBear, KoalaBear and a custom
4-byte-element prime above 2^30; every case first runs an unrelated matrix transform on the plan, writes
into a poisoned `out` inside a longer allocation, and compares its input with a copy afterwards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_gpu_matrix as T
from tests import test_gpu_matrix_ex as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

LOG_N = 12  # the plan; log_rows runs below it
PAD = 64    # poisoned elements on each side of `out`

# (field, d, W): W None at d = 1; the custom prime's W is its generator
EXTS = [(3, 1, None), (3, 2, 7), (4, 1, None), (4, 2, 11), (4, 4, 11), (5, 4, 3), ("p31", 2, T.G31)]

_IN, _COEF = {}, {}


def _ext_mul(a, b, w, p):
    """a b in F_p[X]/(X^d - W); a, b lists of Python ints."""
    d = len(a)
    lo, hi = [0] * d, [0] * d
    for i in range(d):
        for j in range(d):
            if i + j < d:
                lo[i + j] += a[i] * b[j]
            else:
                hi[i + j - d] += a[i] * b[j]
    return [(lo[k] + (w or 0) * hi[k]) % p for k in range(d)]


def _ext_pow(b, e, w, p):
    r = [1] + [0] * (len(b) - 1)
    for _ in range(e):
        r = _ext_mul(r, b, w, p)
    return r


def _coeffs(fid, d, L):
    key = (fid, d, L)
    if key not in _COEF:
        p, _ = T._params(fid)
        _COEF[key] = T._rand(p, 1 << L, d, 7000 + 10 * L + d)
    return _COEF[key]


def _input(fid, d, L, c):
    """[N][d] uint64: row i = f(c w_N^rev_L(i)), coordinate-wise (the oracle's coset evaluations, permuted)."""
    key = (fid, d, L, c)
    if key not in _IN:
        p, g = T._params(fid)
        _IN[key] = np.ascontiguousarray(T._expected(_coeffs(fid, d, L), p, g, c, L)[X._perm(L)])
    return _IN[key]


def _fold_coeffs(a, k, beta, w, p):
    """g_m = sum_{t < 2^k} beta^t a_{m 2^k + t}: [N][d] -> [N >> k][d], Python integers (object arrays)."""
    N, d = a.shape
    A = a.astype(object).reshape(N >> k, 1 << k, d)
    out = np.zeros((N >> k, d), dtype=object)
    bt = [1] + [0] * (d - 1)
    for t in range(1 << k):
        for i in range(d):       # coordinate i of a times coordinate j of beta^t lands on X^(i+j)
            for j in range(d):
                if bt[j] == 0:
                    continue
                term = A[:, t, i] * bt[j]
                if i + j < d:
                    out[:, i + j] += term
                else:
                    out[:, i + j - d] += term * w
        out %= p
        bt = _ext_mul(bt, list(beta), w, p)
    return out.astype(np.uint64)


def _expected_fold(fid, d, w, L, k, c, beta):
    p, g = T._params(fid)
    gm = _fold_coeffs(_coeffs(fid, d, L), k, beta, w, p)
    return T._expected(gm, p, g, pow(c, 1 << k, p), L - k)[X._perm(L - k)]


def _fold(pl, x, d, w, L, k, beta, shift, dirty=True):
    """One fold of x = [N][d] on dirtied scratch into the middle of a poisoned buffer; checks the poison around
    the output and that d_in is unchanged."""
    t_in = T._dev(x, pl)
    keep = t_in.clone()
    if dirty:
        T._dirty(pl, 3)
    count = (1 << (L - k)) * d
    big = T._poisoned(pl, count + 2 * PAD)
    out = big[PAD:PAD + count]
    pl.fri_fold(t_in, out, k, beta, ext_degree=d, ext_w=w or 0, shift=shift, log_rows=L)
    poison = T.POISON32 if pl.elem32 else T.POISON64
    assert bool((big[:PAD] == poison).all()) and bool((big[PAD + count:] == poison).all()), "poison around out"
    assert torch.equal(t_in, keep), "d_in was modified"
    return T._host(out, 1 << (L - k), d)


def _betas(p, d, seed):
    rng = np.random.default_rng(seed)
    return [[int(v) for v in rng.integers(0, p, size=d, dtype=np.uint64)], [0] * d, [1] + [0] * (d - 1), [p - 1] * d]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("fid,d,w", EXTS)
def test_fold_matches_the_coefficient_domain_definition(fid, d, w, k):
    """Every shift, every log_rows (one output row, two, less than a wave of outputs on a larger plan, several
    workgroups, and the plan's own size: output rows beyond 2^lo_bits, both table levels), every beta."""
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    for L in sorted({k, k + 1, 5, 9, 12}):
        for shift in X._shifts(fid):
            c = X._one(shift)
            x = _input(fid, d, L, c)
            for bi, beta in enumerate(_betas(p, d, 31 * L + k)):
                got = _fold(pl, x, d, w, L, k, beta, shift, dirty=bi == 0)
                want = _expected_fold(fid, d, w, L, k, c, beta)
                assert np.array_equal(got, want), (fid, d, w, k, L, shift, beta)


@pytest.mark.parametrize("fid,d,w", [(3, 2, 7), (4, 4, 11), ("p31", 2, T.G31), (5, 1, None)])
def test_both_load_forms_and_unaligned_buffers_give_the_same_bits(fid, d, w, monkeypatch):
    """The knob's two load forms, and buffers that are not 16-byte aligned (the element-wise path)."""
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    L = 9
    x = _input(fid, d, L, g)
    for k in (1, 2, 3, 4):
        beta = _betas(p, d, k)[0]
        want = _expected_fold(fid, d, w, L, k, g, beta)
        for form in ("0", "1"):
            monkeypatch.setenv("NTT_FOLD_STAGED", form)
            assert np.array_equal(_fold(pl, x, d, w, L, k, beta, g), want), (fid, d, k, form)
            # one element off a 16-byte boundary, in and out
            rows_out = 1 << (L - k)
            src = torch.empty(x.size + 1, dtype=pl.dtype, device="cuda:0")
            src[1:].copy_(T._dev(x, pl))
            big = T._poisoned(pl, rows_out * d + 2 * PAD + 1)
            out = big[PAD + 1:PAD + 1 + rows_out * d]
            assert src[1:].data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0
            pl.fri_fold(src[1:], out, k, beta, ext_degree=d, ext_w=w or 0, shift=g, log_rows=L)
            assert np.array_equal(T._host(out, rows_out, d), want), (fid, d, k, form, "unaligned")
            poison = T.POISON32 if pl.elem32 else T.POISON64
            assert bool((big[:PAD + 1] == poison).all()) and bool((big[PAD + 1 + rows_out * d:] == poison).all())
        monkeypatch.delenv("NTT_FOLD_STAGED")


@pytest.mark.parametrize("fid,d,w", [(3, 2, 7), (4, 4, 11), (5, 4, 3), (4, 1, None)])
def test_one_fold_of_arity_2k_is_k_folds_of_arity_2(fid, d, w):
    """One call of arity 2^k by beta = k calls of arity 2 by beta^(2^s) with shifts c^(2^s), bit for bit, and
    both are the oracle's; the powers come from the host."""
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N)
    L = 9
    for shift in X._shifts(fid):
        c = X._one(shift)
        x = _input(fid, d, L, c)
        for k in (2, 3, 4):
            beta = _betas(p, d, 50 + k)[0]
            one = _fold(pl, x, d, w, L, k, beta, shift)
            cur = x
            for s in range(k):
                bs = _ext_pow(beta, 1 << s, w, p)
                cs = pow(c, 1 << s, p)
                cur = _fold(pl, cur, d, w, L - s, 1, bs, None if (shift is None) else cs, dirty=False)
            assert np.array_equal(one, cur), (fid, d, k, shift)
            assert np.array_equal(one, _expected_fold(fid, d, w, L, k, c, beta)), (fid, d, k, shift)


@pytest.mark.parametrize("fid,d,w", [(4, 4, 11), (3, 2, 7)])
def test_extension_hands_over_to_the_fold(fid, d, w):
    """lde_matrix(log_blowup=1, shift=g, width=d, bitrev_out=True) feeds fri_fold(shift=g) on the device: the
    result is the oracle's fold of the zero-padded coefficients."""
    p, g = T._params(fid)
    L = 6
    pl = T._plan(fid, L)
    a = T._rand(p, 1 << (L - 1), d, 606 + d)
    padded = np.zeros((1 << L, d), dtype=np.uint64)
    padded[:1 << (L - 1)] = a
    ev = T._poisoned(pl, (1 << L) * d)
    pl.lde_matrix(T._dev(a, pl), ev, 1, g, d, bitrev_out=True)
    for k in (1, 2, 4):
        beta = _betas(p, d, 60 + k)[0]
        out = T._poisoned(pl, (1 << (L - k)) * d)
        pl.fri_fold(ev, out, k, beta, ext_degree=d, ext_w=w, shift=g)
        gm = _fold_coeffs(padded, k, beta, w, p)
        want = T._expected(gm, p, g, pow(g, 1 << k, p), L - k)[X._perm(L - k)]
        assert np.array_equal(T._host(out, 1 << (L - k), d), want), (fid, k)


def test_montgomery_io_keeps_the_form():
    """BabyBear with NTT_PLAN_MONTGOMERY_IO (R = 2^32): Montgomery-form input with canonical beta and shift
    gives the Montgomery form of the expected output."""
    fid, d, w, L = 4, 4, 11, 9
    p, g = T._params(fid)
    pl = T._plan(fid, LOG_N, montgomery_io=True)
    R = np.uint64((1 << 32) % p)
    x = _input(fid, d, L, g)
    for k in (1, 3, 4):
        beta = _betas(p, d, 70 + k)[0]
        got = _fold(pl, x * R % np.uint64(p), d, w, L, k, beta, g, dirty=False)
        assert np.array_equal(got, _expected_fold(fid, d, w, L, k, g, beta) * R % np.uint64(p)), k


def test_argument_errors_leave_the_buffers_untouched():
    from ntt_amd import lib as L
    so = L.load()
    p, g = T._params(4)
    log_n, d, w = 10, 4, 11
    pl = T._plan(4, log_n)
    tw = T._plan(4, log_n, twiddle_only=True)
    src = T._dev(T._rand(p, pl.n, d, 1), pl)
    keep_src = src.clone()
    out = T._poisoned(pl, pl.n * d)
    keep = out.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i, o = C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr())
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    beta, sh = u64(1, 2, 3, 4), u64(g)
    f = so.ntt_fri_fold
    cases = [
        # null pointers
        f(pl._h, None, o, log_n, 1, d, w, beta, sh, st), f(pl._h, i, None, log_n, 1, d, w, beta, sh, st),
        f(pl._h, i, o, log_n, 1, d, w, None, sh, st),
        # log_arity 0, above 4, above log_rows; log_rows above the plan's
        f(pl._h, i, o, log_n, 0, d, w, beta, sh, st), f(pl._h, i, o, log_n, 5, d, w, beta, None, st),
        f(pl._h, i, o, 2, 3, d, w, beta, sh, st), f(pl._h, i, o, log_n + 1, 1, d, w, beta, sh, st),
        # ext_degree
        f(pl._h, i, o, log_n, 1, 0, w, beta, sh, st), f(pl._h, i, o, log_n, 1, 3, w, beta, sh, st),
        f(pl._h, i, o, log_n, 1, 5, w, beta, None, st), f(pl._h, i, o, log_n, 1, 8, w, beta, sh, st),
        # ext_w 0 or >= p at ext_degree > 1
        f(pl._h, i, o, log_n, 1, d, 0, beta, sh, st), f(pl._h, i, o, log_n, 1, d, p, beta, sh, st),
        f(pl._h, i, o, log_n, 1, 2, 1 << 40, beta, None, st),
        # a beta word >= p
        f(pl._h, i, o, log_n, 1, d, w, u64(1, 2, 3, p), sh, st), f(pl._h, i, o, log_n, 1, d, w, u64(p, 0, 0, 0), sh, st),
        f(pl._h, i, o, log_n, 1, 1, 0, u64(1 << 33), None, st),
        # a bad shift
        f(pl._h, i, o, log_n, 1, d, w, beta, u64(0), st), f(pl._h, i, o, log_n, 1, d, w, beta, u64(p), st),
        f(pl._h, i, o, log_n, 2, d, w, beta, u64(1 << 40), st),
        # overlap: the same buffer, and out starting on in's last element
        f(pl._h, o, o, log_n, 1, d, w, beta, sh, st),
        f(pl._h, i, C.c_void_p(src.data_ptr() + 4 * (pl.n * d - 1)), log_n, 1, d, w, beta, sh, st),
        f(pl._h, C.c_void_p(out.data_ptr() + 4 * ((pl.n >> 1) * d - 1)), o, log_n, 1, d, w, beta, sh, st),
        # a plan without transform tables
        f(tw._h, i, o, log_n, 1, d, w, beta, sh, st),
    ]
    assert cases == [L.NTT_ERR_ARG] * len(cases), cases
    torch.cuda.synchronize()
    assert torch.equal(out, keep) and torch.equal(src, keep_src)
    # ext_w is ignored at ext_degree 1
    assert f(pl._h, i, o, log_n, 1, 1, p + 5, beta, sh, st) == L.NTT_OK
    torch.cuda.synchronize()


def test_29_bit_engines_refuse_the_fold():
    from ntt_amd import lib as L
    from ntt_amd.ntt import NTTPlan
    so = L.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    beta = (C.c_uint64 * 4)(1, 0, 0, 0)
    for pl, words in ((NTTPlan(1, 10, 4), 4), (NTTPlan(0, 10, 1), 1)):  # BN254, P469762049
        t = torch.full((pl.n * words,), 1, dtype=torch.int64, device="cuda:0")
        out = torch.full((pl.n * words,), 2, dtype=torch.int64, device="cuda:0")
        keep_t, keep_o = t.clone(), out.clone()
        for shift in (None, (C.c_uint64 * 4)(5, 0, 0, 0)):
            assert so.ntt_fri_fold(pl._h, C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), 10, 1, 1, 0, beta,
                                   shift, st) == L.NTT_ERR_ARG
        torch.cuda.synchronize()
        assert torch.equal(t, keep_t) and torch.equal(out, keep_o)


def test_profiling_labels_the_one_launch():
    p, g = T._params(4)
    pl = T._plan(4, LOG_N)
    d, w, L = 4, 11, 9
    x = T._dev(_input(4, d, L, g), pl)
    for k in (1, 2, 3, 4):
        out = T._poisoned(pl, (1 << (L - k)) * d)
        pl.set_profiling(True)
        pl.fri_fold(x, out, k, [1, 2, 3, 4], ext_degree=d, ext_w=w, shift=g, log_rows=L)
        labels, ms = pl.last_launch_labels(), pl.last_launch_ms()
        pl.set_profiling(False)
        assert labels == [f"x{k}"], (k, labels)
        assert len(ms) == 1


CHILD = r'''
import sys
sys.path.insert(0, ROOT)
import numpy as np
from ntt_amd import lib as L
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
from tests import test_gpu_matrix as T
from tests import test_gpu_fold as F
for fid, d, w in ((3, 2, 7), (4, 4, 11)):
    p, g = T._params(fid)
    pl = T._plan(fid, F.LOG_N)
    Lr = 9
    x = F._input(fid, d, Lr, g)
    for k in (1, 4):
        beta = F._betas(p, d, 80 + k)[0]
        got = F._fold(pl, x, d, w, Lr, k, beta, g)
        assert np.array_equal(got, F._expected_fold(fid, d, w, Lr, k, g, beta)), (fid, k)
        st = pl.device_status()
        assert st == 0, (fid, k, hex(st))
    bad = x.copy()
    bad[37, d - 1] = p  # one non-canonical input element
    F._fold(pl, bad, d, w, Lr, 4, beta, g)
    st = pl.device_status()
    assert st == 0x200, (fid, "non-canonical input", hex(st))
    assert pl.device_status() == 0
print("FOLD-DEBUG-OK")
'''


def test_checked_build_reports_clean_status():
    """Folds of arity 2 and 16 on both engines through the checked build in a fresh process: right results and
    no bounds / canonical report; one input element equal to p reports 0x200."""
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "FOLD-DEBUG-OK" in r.stdout
