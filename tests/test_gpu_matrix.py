"""The row-major matrix calls on the GPU (NTTPlan.forward_matrix / inverse_matrix / lde_matrix,
lde_matrix_from_evals): transforms over the columns of a [n][width] matrix, bit-exact against the
oracle's transform of each column taken out on the host (oracle/ntt_ref.py at the small sizes,
oracle_c.ntt_mp on the host-scaled, zero-padded column above them, as tests/test_gpu_lde.py does), on
Goldilocks, BabyBear, KoalaBear and a custom 4-byte-element prime above 2^30.

The sizes come from the schedule the calls report (matrix_passes): the largest size of one pass, the
smallest of two and of three.  Every case first runs an unrelated matrix transform on the plan, so that
its scratch holds another call's data; an extension writes into a poisoned `out`, and its input is
compared with a copy afterwards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

P31, G31 = 1811939329, 13  # 27 * 2^26 + 1 > 2^30: a custom NTT_PLAN_ELEM32 plan
FIELDS = [3, 4, 5, "p31"]
WIDTHS = (1, 2, 3, 15, 16, 17, 37)  # narrower than a strip, one strip, one over, a masked remainder
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A

_PLANS, _SIZES, _POW = {}, {}, {}


def _params(fid):
    from ntt_amd.fields import field_params
    return (P31, G31) if fid == "p31" else field_params(fid)


def _plan(fid, log_n, **kw):
    from ntt_amd.ntt import NTTPlan
    key = (fid, log_n, tuple(sorted(kw.items())))
    if key not in _PLANS:
        if fid == "p31":
            _PLANS[key] = NTTPlan(log_n=log_n, limbs64=1, modulus=P31, generator=G31, elem32=True, **kw)
        else:
            _PLANS[key] = NTTPlan(fid, log_n, 1, **kw)
    return _PLANS[key]


def _size(fid, width, passes, largest=False):
    """The smallest (largest) log_n whose matrix schedule at this width has `passes` passes."""
    key = (fid, width, passes, largest)
    if key not in _SIZES:
        found = None
        for log_n in range(3, 25):
            k = len(_plan(fid, log_n).matrix_passes(width))
            if k == passes:
                found = log_n
                if not largest:
                    break
            elif k > passes:
                break
        assert found is not None, key
        _SIZES[key] = found
    return _SIZES[key]


def _rand(p, rows, width, seed):
    """Seeded values below p, [rows][width] uint64, with the edge values 0, 1, p - 1, p - 2 in front."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, p, size=(rows, width), dtype=np.uint64)
    edge = np.array([0, 1, p - 1, p - 2], dtype=np.uint64)
    flat = x.reshape(-1)
    flat[:min(flat.size, 4)] = edge[:min(flat.size, 4)]
    return x


def _dev(x, pl):
    flat = np.ascontiguousarray(x.reshape(-1))
    host = flat.astype(np.uint32).view(np.int32) if pl.elem32 else flat.view(np.int64)
    return torch.from_numpy(host).to("cuda:0")


def _host(t, rows, width):
    a = t.cpu().numpy()
    a = a.view(np.uint32).astype(np.uint64) if a.dtype.itemsize == 4 else a.view(np.uint64)
    return a.reshape(rows, width)


def _powers(c, count, p):
    key = (c, p)
    if key not in _POW or len(_POW[key]) < count:
        out, v = np.empty(count, dtype=np.uint64), 1
        for j in range(count):
            out[j] = v
            v = v * c % p
        _POW[key] = out
    return _POW[key][:count]


def _expected(x, p, g, c, log_n, inverse=False):
    """The oracle's transform of every column of x = [n_in][width] (n_in <= N = 2^log_n), zero-padded to
    N rows: coset evaluations on c <w_N> (c = 1: the plain forward), or the inverse (n_in = N)."""
    from oracle import ntt_ref as R
    from oracle import oracle_c as OC
    N, (n_in, width) = 1 << log_n, x.shape
    out = np.zeros((N, width), dtype=np.uint64)
    for b in range(width):
        col = np.ascontiguousarray(x[:, b])
        if log_n <= 5:
            vals = [int(v) for v in col]
            res = R.intt(vals, p, g) if inverse else R.coset_ntt(vals + [0] * (N - n_in), p, g, c)
            out[:, b] = np.array(res, dtype=np.uint64)
            continue
        host = np.zeros((N, 1), dtype=np.uint64)
        host[:n_in, 0] = col if c == 1 else OC.mul_mp(col.reshape(-1, 1), _powers(c, n_in, p).reshape(-1, 1), p)[:, 0]
        out[:, b] = OC.ntt_mp(host, p, g, inverse)[:, 0]
    return out


def _dirty(pl, width):
    """An unrelated matrix transform: the plan's scratch (multi-pass sizes) holds its data."""
    pl.forward_matrix(_dev(_rand(pl.p, pl.n, width, 99), pl), width)


def _poisoned(pl, count):
    out = torch.empty(count, dtype=pl.dtype, device="cuda:0")
    out.fill_(POISON32 if pl.elem32 else POISON64)
    return out


def _lde(pl, x, log_blowup, shift, width):
    """One extension on dirtied scratch into a poisoned `out`; checks that d_in is unchanged."""
    t_in = _dev(x, pl)
    keep = t_in.clone()
    _dirty(pl, width)
    out = _poisoned(pl, pl.n * width)
    pl.lde_matrix(t_in, out, log_blowup, shift, width)
    assert torch.equal(t_in, keep), "d_in was modified"
    return _host(out, pl.n, width)


def _log_ns(fid):
    """0, 1, 2 (no pass kernel), 3, 5, the largest single-pass and the smallest two-pass size."""
    return sorted({0, 1, 2, 3, 5, _size(fid, 37, 1, largest=True), _size(fid, 37, 2)})


@pytest.mark.parametrize("which", range(7))
@pytest.mark.parametrize("fid", FIELDS)
def test_forward_and_inverse_match_the_oracle(fid, which):
    sizes = _log_ns(fid)
    if which >= len(sizes):
        return  # fewer distinct sizes than slots: nothing left to check
    log_n = sizes[which]
    p, g = _params(fid)
    pl = _plan(fid, log_n)
    for width in WIDTHS:
        x = _rand(p, pl.n, width, 100 * log_n + width)
        _dirty(pl, width)
        t = _dev(x, pl)
        pl.forward_matrix(t, width)
        fwd = _host(t, pl.n, width)
        assert np.array_equal(fwd, _expected(x, p, g, 1, log_n)), (fid, log_n, width, "forward")
        pl.inverse_matrix(t, width)
        assert np.array_equal(_host(t, pl.n, width), x), (fid, log_n, width, "inverse(forward(x))")
        _dirty(pl, width)
        t = _dev(x, pl)
        pl.inverse_matrix(t, width)
        assert np.array_equal(_host(t, pl.n, width), _expected(x, p, g, 1, log_n, inverse=True)), (fid, log_n, width,
                                                                                                  "inverse")


@pytest.mark.parametrize("fid", [3, 4])
def test_smallest_three_pass_size(fid):
    width = 3
    log_n = _size(fid, width, 3)
    p, g = _params(fid)
    pl = _plan(fid, log_n)
    assert len(pl.matrix_passes(width)) == 3
    x = _rand(p, pl.n, width, 7)
    _dirty(pl, width)
    t = _dev(x, pl)
    pl.forward_matrix(t, width)
    assert np.array_equal(_host(t, pl.n, width), _expected(x, p, g, 1, log_n))
    got = _lde(pl, x[:pl.n >> 2], 2, g, width)
    assert np.array_equal(got, _expected(x[:pl.n >> 2], p, g, g, log_n))


@pytest.mark.parametrize("fid", FIELDS)
def test_width_one_equals_the_vector_calls(fid):
    p, g = _params(fid)
    for log_n in (2, 5, _size(fid, 1, 1, largest=True), _size(fid, 1, 2)):
        pl = _plan(fid, log_n)
        x = _dev(_rand(p, pl.n, 1, log_n), pl)
        a, b = x.clone(), x.clone()
        assert torch.equal(pl.forward_matrix(a, 1), pl.forward(b)), (fid, log_n, "forward")
        a, b = x.clone(), x.clone()
        assert torch.equal(pl.inverse_matrix(a, 1), pl.inverse(b)), (fid, log_n, "inverse")
        for lb in sorted({0, 1, log_n}):
            for shift in (None, g):
                src = x[:pl.n >> lb].clone()
                a, b = _poisoned(pl, pl.n), _poisoned(pl, pl.n)
                pl.lde_matrix(src, a, lb, shift, 1)
                pl.lde_batch(src, b, lb, shift, 1)
                assert torch.equal(a, b), (fid, log_n, lb, shift)


@pytest.mark.parametrize("width", [3, 16, 37])
@pytest.mark.parametrize("fid", FIELDS)
def test_lde_matches_the_oracle(fid, width):
    p, g = _params(fid)
    for log_n in (2, 5, _size(fid, width, 1, largest=True), _size(fid, width, 2)):
        pl = _plan(fid, log_n)
        passes = pl.matrix_passes(width)
        r1 = passes[0] if passes else log_n
        x = _rand(p, pl.n, width, 1000 * log_n + width)
        for lb in sorted({b for b in (0, 1, 3, r1 + 1, log_n) if b <= log_n}):
            for shift in (None, g, p - 1):
                got = _lde(pl, x[:pl.n >> lb], lb, shift, width)
                exp = _expected(x[:pl.n >> lb], p, g, 1 if shift is None else shift, log_n)
                assert np.array_equal(got, exp), (fid, log_n, width, lb, shift)


@pytest.mark.parametrize("fid", FIELDS)
def test_lde_matrix_from_evals(fid):
    from ntt_amd.ntt import lde_matrix_from_evals
    p, g = _params(fid)
    width, big_log = 37, _size(fid, 37, 2)
    small, big = _plan(fid, big_log - 3), _plan(fid, big_log)
    evals = _rand(p, small.n, width, 5)
    coeffs = _expected(evals, p, g, 1, small.log_n, inverse=True)
    t, out = _dev(evals, small), _poisoned(big, big.n * width)
    _dirty(big, width)
    lde_matrix_from_evals(small, big, t, out, g, width)
    assert np.array_equal(_host(t, small.n, width), coeffs)
    assert np.array_equal(_host(out, big.n, width), _expected(coeffs, p, g, g, big_log))


@pytest.mark.parametrize("fid", [3, 4])
def test_masked_strips_touch_nothing_outside_the_matrix(fid):
    """The matrix sits inside a larger poisoned allocation: the elements before it and after it (the
    columns a last strip would hold past the row's end among them) keep the poison."""
    p, g = _params(fid)
    width, pad = 37, 256
    for log_n in (_size(fid, width, 1, largest=True), _size(fid, width, 2)):
        pl = _plan(fid, log_n)
        count = pl.n * width
        poison = POISON32 if pl.elem32 else POISON64
        x = _rand(p, pl.n, width, 3)
        big = _poisoned(pl, count + 2 * pad)
        t = big[pad:pad + count]
        t.copy_(_dev(x, pl))
        pl.forward_matrix(t, width)
        assert np.array_equal(_host(t, pl.n, width), _expected(x, p, g, 1, log_n))
        pl.inverse_matrix(t, width)
        assert np.array_equal(_host(t, pl.n, width), x)
        big2 = _poisoned(pl, count + 2 * pad)
        lb = 2
        pl.lde_matrix(_dev(x[:pl.n >> lb], pl), big2[pad:pad + count], lb, g, width)
        assert np.array_equal(_host(big2[pad:pad + count], pl.n, width), _expected(x[:pl.n >> lb], p, g, g, log_n))
        for buf in (big, big2):
            assert bool((buf[:pad] == poison).all()) and bool((buf[pad + count:] == poison).all()), (fid, log_n)


def test_montgomery_io_keeps_the_form():
    """BabyBear with NTT_PLAN_MONTGOMERY_IO (R = 2^32): LDE(x R) = LDE(x) R, forward and inverse too."""
    p, g = _params(4)
    width, log_n = 17, _size(4, 17, 2)
    pl = _plan(4, log_n, montgomery_io=True)
    R = (1 << 32) % p
    x = _rand(p, pl.n, width, 11)
    xr = x * np.uint64(R) % np.uint64(p)
    got = _lde(pl, xr[:pl.n >> 1], 1, g, width)
    assert np.array_equal(got, _expected(x[:pl.n >> 1], p, g, g, log_n) * np.uint64(R) % np.uint64(p))
    t = _dev(xr, pl)
    pl.forward_matrix(t, width)
    assert np.array_equal(_host(t, pl.n, width), _expected(x, p, g, 1, log_n) * np.uint64(R) % np.uint64(p))
    pl.inverse_matrix(t, width)
    assert np.array_equal(_host(t, pl.n, width), xr)


def test_argument_errors_leave_out_untouched():
    from ntt_amd import lib as L
    so = L.load()
    p, g = _params(4)
    log_n, width = 10, 3
    pl = _plan(4, log_n)
    tw = _plan(4, log_n, twiddle_only=True)
    src = _dev(_rand(p, pl.n >> 1, width, 1), pl)
    out = _poisoned(pl, pl.n * width)
    keep = out.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i, o = C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr())
    shift = lambda v: (C.c_uint64 * 1)(v)
    lde = so.ntt_lde_matrix
    cases = [
        lde(pl._h, None, o, 1, None, width, st), lde(pl._h, i, None, 1, None, width, st),
        lde(pl._h, i, o, 1, None, 0, st), lde(pl._h, i, o, 1, None, 1 << 22, st),
        lde(pl._h, i, o, log_n + 1, None, width, st), lde(pl._h, i, o, 1, shift(0), width, st),
        lde(pl._h, i, o, 1, shift(p), width, st), lde(pl._h, o, o, 1, None, width, st),
        lde(pl._h, C.c_void_p(out.data_ptr() + 4 * (pl.n * width - 1)), o, 1, None, width, st),
        lde(tw._h, i, o, 1, None, width, st),
        so.ntt_forward_matrix(pl._h, None, width, st), so.ntt_forward_matrix(pl._h, o, 0, st),
        so.ntt_forward_matrix(pl._h, o, 1 << 22, st), so.ntt_inverse_matrix(pl._h, o, 0, st),
        so.ntt_forward_matrix(tw._h, o, width, st), so.ntt_inverse_matrix(tw._h, o, width, st),
        so.ntt_plan_matrix_info(pl._h, 0, None, None), so.ntt_plan_matrix_info(pl._h, 1 << 22, None, None),
    ]
    assert cases == [L.NTT_ERR_ARG] * len(cases), cases
    torch.cuda.synchronize()
    assert torch.equal(out, keep)


def test_29_bit_engines_refuse_the_matrix_calls():
    from ntt_amd import lib as L
    from ntt_amd.ntt import NTTPlan
    so = L.load()
    pl = NTTPlan(1, 10, 4)  # BN254
    t = torch.full((pl.n * 4,), 1, dtype=torch.int64, device="cuda:0")
    keep = t.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = C.c_void_p(t.data_ptr())
    npass, radix = C.c_uint(), (C.c_uint * 8)()
    assert so.ntt_forward_matrix(pl._h, d, 1, st) == L.NTT_ERR_ARG
    assert so.ntt_inverse_matrix(pl._h, d, 1, st) == L.NTT_ERR_ARG
    assert so.ntt_lde_matrix(pl._h, d, C.c_void_p(t.data_ptr() + 8 * 4 * 512), 1, None, 1, st) == L.NTT_ERR_ARG
    assert so.ntt_plan_matrix_info(pl._h, 1, C.byref(npass), radix) == L.NTT_ERR_ARG
    with pytest.raises(L.NTTError):
        pl.matrix_passes(1)
    torch.cuda.synchronize()
    assert torch.equal(t, keep)


@pytest.mark.parametrize("fid", [3, 4])
def test_one_launch_label_per_pass(fid):
    p, _ = _params(fid)
    width = 37
    for log_n in (2, _size(fid, width, 1, largest=True), _size(fid, width, 2), _size(fid, width, 2) + 3):
        pl = _plan(fid, log_n)
        passes = pl.matrix_passes(width)
        t = _dev(_rand(p, pl.n, width, 1), pl)
        pl.set_profiling(True)
        pl.forward_matrix(t, width)
        labels = pl.last_launch_labels()
        ms = pl.last_launch_ms()
        pl.set_profiling(False)
        if not passes:
            assert labels == ["n"], labels
        elif len(passes) == 1:
            assert labels == [f"s{passes[0]}"], labels
        else:
            assert labels == [f"c{r}" for r in passes[:-1]] + [f"f{passes[-1]}"], labels
        assert len(ms) == len(labels)


CHILD = r'''
import sys
sys.path.insert(0, ROOT)
import numpy as np
from ntt_amd import lib as L
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
sys.path.insert(0, ROOT + "/tests")
import test_gpu_matrix as T
width = 37
for fid in (3, 4):
    p, g = T._params(fid)
    log_n = T._size(fid, width, 2)
    pl = T._plan(fid, log_n)
    x = T._rand(p, pl.n, width, 5)
    t = T._dev(x, pl)
    pl.forward_matrix(t, width)
    assert np.array_equal(T._host(t, pl.n, width), T._expected(x, p, g, 1, log_n)), (fid, "forward")
    pl.inverse_matrix(t, width)
    assert np.array_equal(T._host(t, pl.n, width), x), (fid, "inverse")
    st = pl.device_status()
    assert st == 0, (fid, hex(st))
    for lb in (1, pl.matrix_passes(width)[0] + 1):
        for shift in (None, g):
            got = T._lde(pl, x[:pl.n >> lb], lb, shift, width)
            assert np.array_equal(got, T._expected(x[:pl.n >> lb], p, g, 1 if shift is None else shift, log_n)), (fid, lb)
            st = pl.device_status()
            assert st == 0, (fid, lb, shift, hex(st))
print("MATRIX-DEBUG-OK")
'''


def test_matrix_checked_build_reports_clean_status():
    """The two-pass cases at width 37 (a masked last strip), log_blowup = r_1 + 1 among them, through the
    checked build in a fresh process: right results and no bounds / canonical / lazy-bound report."""
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "MATRIX-DEBUG-OK" in r.stdout
