"""The Goldilocks engine (field 3, p = 2^64 - 2^32 + 1, 8-byte elements, Eng64G) on the GPU, bit-exact
against the CPU oracle (oracle_c.ntt_mp with one limb) and against the 4-limb engine on the zero-padded
modulus.  Host vectors are uint64 mod p; every random vector starts with the edge set (values around
eps = 2^32 - 1, 2^63 and p, where the carry, the borrow and the canonicalisation of the arithmetic
can go wrong)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

P = 0xFFFFFFFF00000001
G = 7
EPS = (1 << 32) - 1
EDGE = [0, 1, 2, EPS - 1, EPS, EPS + 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, P - EPS, P - 2,
        P - 1]
TILE_LOG = 12      # Eng64G::TILE_LOG: 2^12 is the largest single-tile transform
TWO_PASS_LOG = 15  # 7 + 8: two passes of unequal radix


def _splitmix(c):
    with np.errstate(over="ignore"):
        z = c + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _fill_random(n, seed):
    """ntt_fill kind 1 for one limb: SplitMix64(seed 2^32 + 4 j) masked to 63 bits (oracle_c.random_limbs)."""
    with np.errstate(over="ignore"):
        c = (np.uint64(seed) << np.uint64(32)) + np.uint64(4) * np.arange(n, dtype=np.uint64)
    return _splitmix(c) & np.uint64((1 << 63) - 1)


def _random(n, seed):
    """Seeded values mod p with the edge set in front."""
    with np.errstate(over="ignore"):
        v = _splitmix(np.uint64(seed * 0x1000003) + np.arange(n, dtype=np.uint64)) % np.uint64(P)
    k = min(n, len(EDGE))
    v[:k] = np.array(EDGE[:k], dtype=np.uint64)
    return v


def _dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1).copy()


def _oracle(v, inverse=False, threads=0):
    from oracle import oracle_c as OC
    x = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 1)
    if x.shape[0] == 1:
        return x.reshape(-1).copy()  # the 1-point transform is the identity
    if threads:
        return OC.ntt_mp_par(x, P, G, threads, inverse).reshape(-1)
    return OC.ntt_mp(x, P, G, inverse).reshape(-1)


_PLANS = {}


def _plan(log_n):
    from ntt_amd.ntt import NTTPlan
    if log_n not in _PLANS:
        _PLANS[log_n] = NTTPlan(3, log_n, 1)
    return _PLANS[log_n]


def test_tile_constants_match_the_library():
    assert _plan(TILE_LOG).passes == [TILE_LOG]
    assert len(_plan(TILE_LOG + 1).passes) == 2
    r = _plan(TWO_PASS_LOG).passes
    assert len(r) == 2 and r[0] != r[1], r
    assert _plan(TWO_PASS_LOG).elem_bytes == 8


# ---- 1. every single-tile radix and the first two-pass size
@pytest.mark.parametrize("log_n", range(0, TILE_LOG + 2))
def test_forward_inverse_against_the_oracle(log_n):
    n = 1 << log_n
    pl = _plan(log_n)
    inputs = {"iota": np.arange(n, dtype=np.uint64), "random": _random(n, 11 + log_n),
              "p-1": np.full(n, P - 1, dtype=np.uint64)}
    for name, x in inputs.items():
        exp = _oracle(x)
        if name == "p-1":  # X_0 = n (p - 1), every other output 0
            assert int(exp[0]) == n * (P - 1) % P and not exp[1:].any()
        t = _dev(x)
        pl.forward(t)
        assert np.array_equal(_host(t), exp), (log_n, name, "forward")
        pl.inverse(t)
        assert np.array_equal(_host(t), x), (log_n, name, "round trip")
        t = _dev(x)
        pl.inverse(t)
        assert np.array_equal(_host(t), _oracle(x, inverse=True)), (log_n, name, "inverse")


# ---- 2. two passes of unequal radix, and the smallest three-pass size
def _three_pass_log():
    for lg in range(TILE_LOG + 2, 23):
        if len(_plan(lg).passes) == 3:
            return lg
    return 22


def test_multi_pass_sizes():
    """2^15 (7 + 8) and the first size ntt_plan_info reports three passes for (2^17: 5 + 5 + 7, looked
    up from 2^14 upwards): forward against the threaded oracle, inverse as a round trip."""
    three = _three_pass_log()
    assert len(_plan(three).passes) == 3, ("no three-pass size up to 2^22", three)
    for lg in (TWO_PASS_LOG, three):
        pl = _plan(lg)
        for x in (_random(1 << lg, 5), np.full(1 << lg, P - 1, dtype=np.uint64)):
            t = _dev(x)
            pl.forward(t)
            assert np.array_equal(_host(t), _oracle(x, threads=8)), (lg, pl.passes)
            pl.inverse(t)
            assert np.array_equal(_host(t), x), (lg, pl.passes)


# ---- 3. the same transform on the 4-limb engine (zero-padded modulus)
@pytest.mark.parametrize("log_n", [12, TWO_PASS_LOG])
def test_cross_engine_with_the_four_limb_plan(log_n):
    from ntt_amd.ntt import NTTPlan
    n = 1 << log_n
    x = _random(n, 23)
    t = _dev(x)
    _plan(log_n).forward(t)
    wide = NTTPlan(log_n=log_n, limbs64=4, modulus=P, generator=G)
    x4 = np.zeros((n, 4), dtype=np.uint64)
    x4[:, 0] = x
    t4 = torch.from_numpy(x4.view(np.int64)).to("cuda:0")
    wide.forward(t4)
    got4 = t4.cpu().numpy().view(np.uint64)
    assert not got4[:, 1:].any()
    assert np.array_equal(got4[:, 0], _host(t))


# ---- 4. batches
@pytest.mark.parametrize("log_n,batch", [(5, 3), (5, 128), (6, 64), (TILE_LOG, 3), (TWO_PASS_LOG, 2)])
def test_batched_transforms(log_n, batch):
    """(5, 128) and (6, 64) fill whole tiles of short transforms: the KIND_ROWS instances."""
    n = 1 << log_n
    pl = _plan(log_n)
    x = _random(n * batch, 31).reshape(batch, n)
    x[1:, :len(EDGE)] = x[0, :len(EDGE)][::-1]  # the edge set in every transform, in another order
    nexp = min(batch, 4)  # the oracle on the first and last transforms of a long batch
    rows = list(range(nexp - 1)) + [batch - 1]
    t = _dev(x.reshape(-1))
    pl.forward_batch(t, batch)
    got = _host(t).reshape(batch, n)
    for b in rows:
        assert np.array_equal(got[b], _oracle(x[b])), (log_n, batch, b)
    if batch > 4:  # every transform against the batch-1 path
        one = _dev(x[batch // 2])
        pl.forward(one)
        assert np.array_equal(got[batch // 2], _host(one))
    pl.inverse_batch(t, batch)
    assert np.array_equal(_host(t).reshape(batch, n), x)


# ---- 5. polynomial products
def test_polymul():
    from oracle import oracle_c as OC
    lg, n = 12, 1 << 12
    pl = _plan(lg)
    a, b = _random(n, 41), _random(n, 43)[::-1].copy()
    fa, fb = _oracle(a), _oracle(b)
    exp = _oracle(OC.mul_mp(fa.reshape(-1, 1), fb.reshape(-1, 1), P).reshape(-1), inverse=True)
    ta, tb, tc = _dev(a), _dev(b), pl.empty()
    pl.polymul(ta, tb, tc)
    assert np.array_equal(_host(tc), exp)
    assert np.array_equal(_host(ta), fa) and np.array_equal(_host(tb), fb)  # a, b hold their transforms
    # pointwise product alone
    pw = pl.empty()
    pl.pointwise_mul(ta, tb, pw)
    assert np.array_equal(_host(pw), OC.mul_mp(fa.reshape(-1, 1), fb.reshape(-1, 1), P).reshape(-1))
    # squaring
    ta, tc = _dev(a), pl.empty()
    pl.polymul(ta, ta, tc)
    sq = _oracle(OC.mul_mp(fa.reshape(-1, 1), fa.reshape(-1, 1), P).reshape(-1), inverse=True)
    assert np.array_equal(_host(tc), sq)
    # c aliasing a
    ta, tb = _dev(a), _dev(b)
    pl.polymul(ta, tb, ta)
    assert np.array_equal(_host(ta), exp)
    # multiplication by x rotates by one (cyclic convolution)
    xpoly = np.zeros(n, dtype=np.uint64)
    xpoly[1] = 1
    ta, tb, tc = _dev(a), _dev(xpoly), pl.empty()
    pl.polymul(ta, tb, tc)
    assert np.array_equal(_host(tc), np.roll(a, 1))
    # the batched second half
    ta, tb = _dev(np.concatenate([fa, fb])), _dev(np.concatenate([fb, fb]))
    out = pl.empty(2)
    pl.inverse_pointwise_batch(ta, tb, out, 2)
    got = _host(out).reshape(2, n)
    assert np.array_equal(got[0], exp)
    assert np.array_equal(got[1], _oracle(OC.mul_mp(fb.reshape(-1, 1), fb.reshape(-1, 1), P).reshape(-1), inverse=True))


# ---- 6. cosets
def test_coset_forward_and_inverse():
    lg, n = 12, 1 << 12
    pl = _plan(lg)
    x = _random(n, 53)
    scaled, c = np.zeros(n, dtype=np.uint64), 1
    for j in range(n):
        scaled[j] = int(x[j]) * c % P
        c = c * 7 % P
    exp = _oracle(scaled)
    t = _dev(x)
    pl.forward_coset(t, 7)
    assert np.array_equal(_host(t), exp)
    pl.inverse_coset(t, 7)
    assert np.array_equal(_host(t), x)
    # inverse alone: c^-j INTT(X)_j
    y = _random(n, 59)
    iy, ci, c7 = _oracle(y, inverse=True), 1, pow(7, P - 2, P)
    expi = np.zeros(n, dtype=np.uint64)
    for j in range(n):
        expi[j] = int(iy[j]) * ci % P
        ci = ci * c7 % P
    t = _dev(y)
    pl.inverse_coset(t, 7)
    assert np.array_equal(_host(t), expi)
    # a shift >= 2^63 (the top bit of the one limb)
    big = P - 7
    t = _dev(x)
    pl.forward_coset(t, big)
    pl.inverse_coset(t, big)
    assert np.array_equal(_host(t), x)


# ---- 7. canonical-range check
def test_count_noncanonical():
    pl = _plan(10)
    x = _random(1 << 10, 61)
    assert pl.count_noncanonical(_dev(x)) == 0
    x[[3, 500, 1023]] = np.array([P, P + 1, (1 << 64) - 1], dtype=np.uint64)
    x[7] = P - 1
    assert pl.count_noncanonical(_dev(x)) == 3


# ---- 8. synthetic inputs
def test_fill_kinds():
    lg, n = 13, 1 << 13
    pl = _plan(lg)
    t = pl.fill(pl.empty(), "iota")
    assert np.array_equal(_host(t), np.arange(n, dtype=np.uint64))
    t = pl.fill(pl.empty(), "random", seed=9)
    exp = _fill_random(n, 9)
    assert np.array_equal(_host(t), exp)
    assert (exp >> np.uint64(32)).any() and int(exp.max()) < (1 << 63)  # 63-bit values, below p
    assert pl.count_noncanonical(t) == 0
    # the mapped fill: local i <- global row0 + (i >> 4) + ((i & 15) << 9)
    loc = torch.empty(1 << 8, dtype=torch.int64, device="cuda:0")
    pl.fill_map(loc, "random", 9, 5, 4, 9)
    i = np.arange(1 << 8)
    assert np.array_equal(_host(loc), exp[5 + (i >> 4) + ((i & 15) << 9)])


# ---- 9, 10. custom plans
def test_custom_plan_and_refusals():
    import ctypes as C
    from ntt_amd import lib as L
    from ntt_amd.ntt import NTTPlan
    x = _random(1 << 12, 67)
    t, u = _dev(x), _dev(x)
    _plan(12).forward(t)
    NTTPlan(log_n=12, limbs64=1, modulus=P, generator=G).forward(u)
    assert torch.equal(t, u)
    # another generator: another root of unity, checked against the oracle with that generator
    from oracle import oracle_c as OC
    g2 = pow(7, 7, P)  # an odd power of 7: its (p-1)/n-th power still has order n
    u = _dev(x)
    NTTPlan(log_n=12, limbs64=1, modulus=P, generator=g2).forward(u)
    assert np.array_equal(_host(u), OC.ntt_mp(x.reshape(-1, 1), P, g2).reshape(-1))
    so = L.load()
    h = C.c_void_p()
    pm = (C.c_uint64 * 1)(P)
    # 49 = 7^2 is a square: 49^((p-1)/n) has order n / 2, not a primitive n-th root
    assert so.ntt_plan_create_custom(C.byref(h), pm, (C.c_uint64 * 1)(49), 1, 12, 0) == L.NTT_ERR_FIELD
    # no root of order 2^33
    assert so.ntt_plan_create_custom(C.byref(h), pm, (C.c_uint64 * 1)(7), 1, 33, 0) == L.NTT_ERR_FIELD
    assert so.ntt_plan_create(C.byref(h), 3, 33, 1, 0) == L.NTT_ERR_FIELD
    # every other one-limb modulus >= 2^31 is still refused
    assert so.ntt_plan_create_custom(C.byref(h), (C.c_uint64 * 1)(2013265921), (C.c_uint64 * 1)(31), 1, 10,
                                     0) == L.NTT_ERR_FIELD
    assert so.ntt_plan_create_custom(C.byref(h), (C.c_uint64 * 1)(P - 2), (C.c_uint64 * 1)(7), 1, 10,
                                     0) == L.NTT_ERR_FIELD


def test_twiddle_only_plan_and_ignored_single_launch():
    from ntt_amd.ntt import NTTPlan
    tw = NTTPlan(3, 14, 1, twiddle_only=True)
    t = tw.fill(tw.empty(), "iota")
    assert np.array_equal(_host(t), np.arange(1 << 14, dtype=np.uint64))
    with pytest.raises(Exception):
        tw.forward(t)
    sl = NTTPlan(3, 17, 1, single_launch=True)  # the flag is ignored: the plain passes
    x = _random(1 << 17, 71)
    a, b = _dev(x), _dev(x)
    sl.forward(a)
    _plan(17).forward(b)
    assert torch.equal(a, b)
    sl.set_profiling(True)
    sl.forward(a)
    torch.cuda.synchronize()
    labels = sl.last_launch_labels()
    assert len(labels) == 3 and labels[0].startswith("c") and labels[-1].startswith("f"), labels
    assert len(sl.last_launch_ms()) == 3


# ---- 11. the checked build
CHILD = r'''
import sys
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import numpy as np, torch
from ntt_amd import lib as L
from ntt_amd.ntt import NTTPlan
import test_gpu_goldilocks as T
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
for lg in (3, T.TILE_LOG, T.TILE_LOG + 1):
    T.test_forward_inverse_against_the_oracle(lg)
    assert T._plan(lg).device_status() == 0, lg
T.test_polymul()
assert T._plan(12).device_status() == 0
print("CLEAN-OK")
for lg in (10, T.TILE_LOG + 1):
    pl = T._plan(lg)
    x = T._random(1 << lg, 3)
    x[5] = T.P + 3
    pl.forward(T._dev(x))
    st = pl.device_status()
    assert st == 0x200, (lg, hex(st))
    assert pl.device_status() == 0
print("INPUT-OK")
'''


def test_checked_build():
    """Tests 1 (2^3, 2^12, 2^13) and 5 through libntt_debug.so: no check fires on legal data; one
    input pattern >= p is reported as 0x200 and nothing else."""
    assert os.path.exists(DEBUG_LIB), "libntt_debug.so not built (python -m ntt_amd.build --debug)"
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "CLEAN-OK" in r.stdout and "INPUT-OK" in r.stdout


# ---- 12. four-step over virtual ranks
def _index(layout, kind):
    i = torch.arange(layout.local_n, dtype=torch.int64, device="cuda:0")
    if kind == "row":
        a, j2 = i >> layout.log_n2, i & (layout.n2 - 1)
        return layout.rank * layout.r + a + layout.n1 * j2
    k1, kc = i >> layout.log_c, i & (layout.c - 1)  # column layout [n1][c]
    return layout.rank * layout.c + kc + layout.n2 * k1


@pytest.mark.parametrize("world,log_n", [(2, 12), (4, 12), (2, 14), (4, 14)])
def test_four_step_virtual_ranks(world, log_n):
    from ntt_amd.distributed import VirtualRanks
    ref = _plan(log_n)
    x = ref.fill(ref.empty(), "random", seed=42)
    x[:len(EDGE)] = _dev(np.array(EDGE, dtype=np.uint64))
    x0 = x.clone()
    ref.forward(x)
    vr = VirtualRanks(3, log_n, 1, world)
    xs = vr.empty()
    for lay, t in zip(vr.layouts, xs):  # row-layout shares of the global vector
        t.copy_(x0[_index(lay, "row")])
    shares = [t.clone() for t in xs]
    vr.forward(xs)
    for lay, t in zip(vr.layouts, xs):
        assert torch.equal(t, x[_index(lay, "col")]), (world, log_n, lay.rank)
    vr.inverse(xs)
    for s, t in zip(shares, xs):
        assert torch.equal(s, t)
