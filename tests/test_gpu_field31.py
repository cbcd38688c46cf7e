"""The 31-bit engine (Eng31) on the GPU: BabyBear (field 4, p = 2^31 - 2^27 + 1), KoalaBear (field 5,
p = 2^31 - 2^24 + 1) and NTT_PLAN_ELEM32 custom plans on 4-byte elements, bit-exact against the CPU
oracle (oracle_c.ntt_mp with one limb), against the 4-limb engine on the zero-padded modulus and
against the 8-byte one-limb engine.  Host vectors are uint64 values mod p; the device holds uint32.
Every random vector starts with the edge set (values around 2^24, 2^27, 2^30, p / 2 and p, where the
sums, differences and the canonicalisation of the arithmetic can go wrong)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

BABYBEAR, KOALABEAR, P30 = 2013265921, 2130706433, 1004535809
FIELDS = {4: (BABYBEAR, 31), 5: (KOALABEAR, 3)}
TILE_LOG = 13  # Eng31::TILE_LOG: 2^13 is the largest single-tile transform (pinned below)


def _edge(p):
    raw = [0, 1, 2, 1 << 24, 1 << 27, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1]
    return [v % p for v in raw]


def _splitmix(c):
    with np.errstate(over="ignore"):
        z = c + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _fill_random(n, seed, p):
    """ntt_fill kind 1 on 4-byte elements: SplitMix64(seed 2^32 + 4 j) & (2^(bitlen(p) - 1) - 1), one word."""
    with np.errstate(over="ignore"):
        c = (np.uint64(seed) << np.uint64(32)) + np.uint64(4) * np.arange(n, dtype=np.uint64)
    return _splitmix(c) & np.uint64((1 << (p.bit_length() - 1)) - 1)


def _random(n, seed, p):
    """Seeded values mod p with the edge set in front."""
    with np.errstate(over="ignore"):
        v = _splitmix(np.uint64(seed * 0x1000003) + np.arange(n, dtype=np.uint64)) % np.uint64(p)
    e = _edge(p)
    k = min(n, len(e))
    v[:k] = np.array(e[:k], dtype=np.uint64)
    return v


def _dev(v):
    """uint64 host values (any 32-bit pattern) -> int32 device tensor of uint32 elements."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint64).astype(np.uint32).view(np.int32).copy()).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1).astype(np.uint64)


def _oracle(v, p, g, inverse=False, threads=0):
    from oracle import oracle_c as OC
    x = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 1)
    if x.shape[0] == 1:
        return x.reshape(-1).copy()  # the 1-point transform is the identity
    if threads:
        return OC.ntt_mp_par(x, p, g, threads, inverse).reshape(-1)
    return OC.ntt_mp(x, p, g, inverse).reshape(-1)


def _mul(a, b, p):
    from oracle import oracle_c as OC
    return OC.mul_mp(np.ascontiguousarray(a).reshape(-1, 1), np.ascontiguousarray(b).reshape(-1, 1), p).reshape(-1)


_PLANS = {}


def _plan(field_id, log_n):
    from ntt_amd.ntt import NTTPlan
    if (field_id, log_n) not in _PLANS:
        _PLANS[field_id, log_n] = NTTPlan(field_id, log_n, 1)
    return _PLANS[field_id, log_n]


def _two_pass_unequal_log():
    for lg in range(TILE_LOG + 1, 23):
        r = _plan(4, lg).passes
        if len(r) == 2 and r[0] != r[1]:
            return lg
    return None


def _three_pass_log():
    for lg in range(TILE_LOG + 2, 23):
        if len(_plan(4, lg).passes) == 3:
            return lg
    return None


def test_tile_constants_match_the_library():
    pl = _plan(4, TILE_LOG)
    assert pl.passes == [TILE_LOG]
    assert len(_plan(4, TILE_LOG + 1).passes) == 2
    assert pl.elem_bytes == 4 and pl.dtype == torch.int32
    t = pl.empty(3)
    assert t.dtype == torch.int32 and t.shape == (3 << TILE_LOG,) and t.is_contiguous()
    with pytest.raises(ValueError):
        pl.forward(torch.zeros(1 << TILE_LOG, dtype=torch.int64, device="cuda:0"))


# ---- 1. every single-tile radix and the first two-pass size, both fields
@pytest.mark.parametrize("log_n", range(0, TILE_LOG + 2))
@pytest.mark.parametrize("field_id", [4, 5])
def test_forward_inverse_against_the_oracle(field_id, log_n):
    p, g = FIELDS[field_id]
    n = 1 << log_n
    pl = _plan(field_id, log_n)
    inputs = {"iota": np.arange(n, dtype=np.uint64), "random": _random(n, 11 + log_n, p),
              "p-1": np.full(n, p - 1, dtype=np.uint64)}
    for name, x in inputs.items():
        exp = _oracle(x, p, g)
        if name == "p-1":  # X_0 = n (p - 1), every other output 0
            assert int(exp[0]) == n * (p - 1) % p and not exp[1:].any()
        t = _dev(x)
        pl.forward(t)
        assert np.array_equal(_host(t), exp), (field_id, log_n, name, "forward")
        pl.inverse(t)
        assert np.array_equal(_host(t), x), (field_id, log_n, name, "round trip")
        t = _dev(x)
        pl.inverse(t)
        assert np.array_equal(_host(t), _oracle(x, p, g, inverse=True)), (field_id, log_n, name, "inverse")


# ---- 2. two passes of unequal radix, and the smallest three-pass size
def test_multi_pass_sizes():
    """The first two-pass size of unequal radices and the first size ntt_plan_info reports three passes
    for (both looked up from 2^14 upwards, at most 2^22): forward against the threaded oracle, inverse as
    a round trip."""
    two, three = _two_pass_unequal_log(), _three_pass_log()
    assert two is not None, "no two-pass size of unequal radices up to 2^22"
    assert three is not None, "no three-pass size up to 2^22"
    p, g = FIELDS[4]
    for lg in (two, three):
        pl = _plan(4, lg)
        for x in (_random(1 << lg, 5, p), np.full(1 << lg, p - 1, dtype=np.uint64)):
            t = _dev(x)
            pl.forward(t)
            assert np.array_equal(_host(t), _oracle(x, p, g, threads=8)), (lg, pl.passes)
            pl.inverse(t)
            assert np.array_equal(_host(t), x), (lg, pl.passes)


def test_every_size_up_to_2_22_has_a_schedule():
    """A plan is made at every log_n of the provers' range (twiddle-only: tables, no scratch)."""
    from ntt_amd.ntt import NTTPlan
    for lg in range(TILE_LOG + 1, 23):
        pl = NTTPlan(4, lg, 1, twiddle_only=True)
        assert sum(pl.passes) == lg and len(pl.passes) >= 2, (lg, pl.passes)
        pl.close()


# ---- 3. the same transform on the other engines
@pytest.mark.parametrize("log_n", [10, 14])
def test_cross_engine_with_the_four_limb_plan(log_n):
    from ntt_amd.ntt import NTTPlan
    p, g = FIELDS[4]
    n = 1 << log_n
    x = _random(n, 23, p)
    t = _dev(x)
    _plan(4, log_n).forward(t)
    wide = NTTPlan(log_n=log_n, limbs64=4, modulus=p, generator=g)
    x4 = np.zeros((n, 4), dtype=np.uint64)
    x4[:, 0] = x
    t4 = torch.from_numpy(x4.view(np.int64)).to("cuda:0")
    wide.forward(t4)
    got4 = t4.cpu().numpy().view(np.uint64)
    assert not got4[:, 1:].any()
    assert np.array_equal(got4[:, 0], _host(t))


@pytest.mark.parametrize("log_n", [10, 14])
def test_cross_engine_with_the_eight_byte_one_limb_plan(log_n):
    from ntt_amd.ntt import NTTPlan
    n = 1 << log_n
    x = _random(n, 29, P30)
    narrow = NTTPlan(log_n=log_n, limbs64=1, modulus=P30, generator=3, elem32=True)
    assert narrow.elem_bytes == 4
    wide = NTTPlan(log_n=log_n, limbs64=1, modulus=P30, generator=3)
    assert wide.elem_bytes == 8
    t = _dev(x)
    t8 = torch.from_numpy(x.view(np.int64).copy()).to("cuda:0")
    narrow.forward(t)
    wide.forward(t8)
    assert np.array_equal(_host(t), t8.cpu().numpy().view(np.uint64))
    narrow.inverse(t)
    assert np.array_equal(_host(t), x)


# ---- 4. batches
@pytest.mark.parametrize("log_n,batch", [(5, 256), (6, 128), (5, 300), (3, 1024), (TILE_LOG, 3), (14, 4)])
def test_batched_transforms(log_n, batch):
    """(5, 256), (6, 128) and (3, 1024) fill whole tiles of short transforms (the KIND_ROWS instances);
    300 transforms of 2^5 leave a partial last tile; 4 x 2^14 is a batch of two-pass transforms."""
    p, g = FIELDS[4]
    n = 1 << log_n
    pl = _plan(4, log_n)
    x = _random(n * batch, 31, p).reshape(batch, n)
    e = min(n, len(_edge(p)))
    x[1:, :e] = x[0, :e][::-1]  # the edge set in every transform, in another order
    nexp = min(batch, 4)  # the oracle on the first and last transforms of a long batch
    rows = list(range(nexp - 1)) + [batch - 1]
    t = _dev(x.reshape(-1))
    pl.forward_batch(t, batch)
    got = _host(t).reshape(batch, n)
    for b in rows:
        assert np.array_equal(got[b], _oracle(x[b], p, g)), (log_n, batch, b)
    if batch > 4:  # a middle transform against the batch-1 path
        one = _dev(x[batch // 2])
        pl.forward(one)
        assert np.array_equal(got[batch // 2], _host(one))
    pl.inverse_batch(t, batch)
    assert np.array_equal(_host(t).reshape(batch, n), x)


# ---- 5. plan calls
@pytest.mark.parametrize("field_id,lg", [(4, 12), (5, 13)])
def test_polymul_and_pointwise(field_id, lg):
    p, g = FIELDS[field_id]
    n = 1 << lg
    pl = _plan(field_id, lg)
    a, b = _random(n, 41, p), _random(n, 43, p)[::-1].copy()
    fa, fb = _oracle(a, p, g), _oracle(b, p, g)
    exp = _oracle(_mul(fa, fb, p), p, g, inverse=True)
    ta, tb, tc = _dev(a), _dev(b), pl.empty()
    pl.polymul(ta, tb, tc)
    assert np.array_equal(_host(tc), exp)
    assert np.array_equal(_host(ta), fa) and np.array_equal(_host(tb), fb)  # a, b hold their transforms
    pw = pl.empty()
    pl.pointwise_mul(ta, tb, pw)
    assert np.array_equal(_host(pw), _mul(fa, fb, p))
    # squaring, and c aliasing a
    ta, tc = _dev(a), pl.empty()
    pl.polymul(ta, ta, tc)
    sq = _oracle(_mul(fa, fa, p), p, g, inverse=True)
    assert np.array_equal(_host(tc), sq)
    ta, tb = _dev(a), _dev(b)
    pl.polymul(ta, tb, ta)
    assert np.array_equal(_host(ta), exp)
    # multiplication by x rotates by one (cyclic convolution)
    xpoly = np.zeros(n, dtype=np.uint64)
    xpoly[1] = 1
    ta, tb, tc = _dev(a), _dev(xpoly), pl.empty()
    pl.polymul(ta, tb, tc)
    assert np.array_equal(_host(tc), np.roll(a, 1))
    # the batched second half, with a == b in the second transform and as the same tensor
    ta, tb = _dev(np.concatenate([fa, fb])), _dev(np.concatenate([fb, fb]))
    out = pl.empty(2)
    pl.inverse_pointwise_batch(ta, tb, out, 2)
    got = _host(out).reshape(2, n)
    assert np.array_equal(got[0], exp)
    assert np.array_equal(got[1], _oracle(_mul(fb, fb, p), p, g, inverse=True))
    pl.inverse_pointwise_batch(ta, ta, out, 2)
    got = _host(out).reshape(2, n)
    assert np.array_equal(got[0], sq)


@pytest.mark.parametrize("field_id,lg", [(4, 13), (5, 12)])
def test_coset_forward_and_inverse(field_id, lg):
    p, g = FIELDS[field_id]
    n = 1 << lg
    pl = _plan(field_id, lg)
    x = _random(n, 53, p)
    for shift in (g, p - 1):
        scaled, c = np.zeros(n, dtype=np.uint64), 1
        for j in range(n):
            scaled[j] = int(x[j]) * c % p
            c = c * shift % p
        t = _dev(x)
        pl.forward_coset(t, shift)
        assert np.array_equal(_host(t), _oracle(scaled, p, g)), shift
        pl.inverse_coset(t, shift)
        assert np.array_equal(_host(t), x), shift
        # inverse alone: shift^-j INTT(X)_j
        iy, ci, si = _oracle(x, p, g, inverse=True), 1, pow(shift, p - 2, p)
        expi = np.zeros(n, dtype=np.uint64)
        for j in range(n):
            expi[j] = int(iy[j]) * ci % p
            ci = ci * si % p
        t = _dev(x)
        pl.inverse_coset(t, shift)
        assert np.array_equal(_host(t), expi), shift
    with pytest.raises(Exception):  # a shift that is not below p
        pl.forward_coset(_dev(x), p)


@pytest.mark.parametrize("field_id", [4, 5])
def test_count_noncanonical(field_id):
    p, _ = FIELDS[field_id]
    pl = _plan(field_id, 12)
    x = _random(1 << 12, 61, p)
    assert pl.count_noncanonical(_dev(x)) == 0
    x[[3, 500, 4095]] = np.array([p, 1 << 31, (1 << 32) - 1], dtype=np.uint64)
    x[7] = p - 1
    assert pl.count_noncanonical(_dev(x)) == 3


@pytest.mark.parametrize("field_id", [4, 5])
def test_fill_kinds(field_id):
    p, _ = FIELDS[field_id]
    lg, n = 13, 1 << 13
    pl = _plan(field_id, lg)
    t = pl.fill(pl.empty(), "iota")
    assert np.array_equal(_host(t), np.arange(n, dtype=np.uint64))
    t = pl.fill(pl.empty(), "random", seed=9)
    exp = _fill_random(n, 9, p)
    assert np.array_equal(_host(t), exp)
    assert int(exp.max()) < (1 << 30) < p and (exp >> np.uint64(24)).any()  # 30-bit values, below p
    assert pl.count_noncanonical(t) == 0
    # the mapped fill: local i <- global row0 + (i >> 4) + ((i & 15) << 9)
    loc = torch.empty(1 << 8, dtype=torch.int32, device="cuda:0")
    pl.fill_map(loc, "random", 9, 5, 4, 9)
    i = np.arange(1 << 8)
    assert np.array_equal(_host(loc), exp[5 + (i >> 4) + ((i & 15) << 9)])


def test_twiddle_only_plan_and_ignored_single_launch():
    from ntt_amd.ntt import NTTPlan
    p, g = FIELDS[4]
    tw = NTTPlan(4, 13, 1, twiddle_only=True)
    t = tw.fill(tw.empty(), "iota")
    assert np.array_equal(_host(t), np.arange(1 << 13, dtype=np.uint64))
    with pytest.raises(Exception):
        tw.forward(t)
    # four-step helpers of a twiddle-only plan on 4-byte elements: transpose, and twiddle_pack against
    # w_n^((row0 + a) b) from the oracle's root
    src = _dev(_random(1 << 13, 3, p))
    dst = tw.empty()
    tw.transpose(src, dst, 5, 8)
    assert np.array_equal(_host(dst).reshape(256, 32), _host(src).reshape(32, 256).T)
    tw.twiddle_pack(src, dst, 5, 8, 8, 7)
    w = pow(g, (p - 1) >> 13, p)
    a, b = np.divmod(np.arange(1 << 13), 256)
    exps = ((7 + a) * b) % (1 << 13)
    pw = np.array([pow(w, int(e), p) for e in range(1 << 13)], dtype=np.uint64)
    assert np.array_equal(_host(dst), _mul(_host(src), pw[exps], p))
    lg = _three_pass_log()
    sl = NTTPlan(4, lg, 1, single_launch=True)  # the flag is ignored: the plain passes
    x = _random(1 << lg, 71, p)
    a, b = _dev(x), _dev(x)
    sl.forward(a)
    _plan(4, lg).forward(b)
    assert torch.equal(a, b)
    sl.set_profiling(True)
    sl.forward(a)
    torch.cuda.synchronize()
    labels = sl.last_launch_labels()
    assert len(labels) == 3 and labels[0].startswith("c") and labels[-1].startswith("f"), labels
    assert len(sl.last_launch_ms()) == 3


# ---- 6. Montgomery-form elements, R = 2^32
@pytest.mark.parametrize("field_id", [4, 5])
def test_montgomery_io(field_id):
    from ntt_amd.ntt import NTTPlan
    p, g = FIELDS[field_id]
    lg, n = 12, 1 << 12
    R = (1 << 32) % p
    rv = np.full(n, R, dtype=np.uint64)
    pl = NTTPlan(field_id, lg, 1, montgomery_io=True)
    x, y = _random(n, 73, p), _random(n, 79, p)
    xr, yr = _mul(x, rv, p), _mul(y, rv, p)
    t = _dev(xr)
    pl.forward(t)
    fx = _oracle(x, p, g)
    assert np.array_equal(_host(t), _mul(fx, rv, p))  # forward(x R) = forward(x) R
    out = pl.empty()
    pl.pointwise_mul(_dev(xr), _dev(yr), out)
    assert np.array_equal(_host(out), _mul(_mul(x, y, p), rv, p))  # (a R)(b R) R^-1 = (a b) R
    ta, tb, tc = _dev(xr), _dev(yr), pl.empty()
    pl.polymul(ta, tb, tc)
    exp = _oracle(_mul(fx, _oracle(y, p, g), p), p, g, inverse=True)
    assert np.array_equal(_host(tc), _mul(exp, rv, p))


# ---- 7. size limits: the fields' two-adicities
def test_two_adicity_limits():
    import ctypes as C
    from ntt_amd import lib as L
    from ntt_amd.ntt import NTTPlan
    pl = NTTPlan(5, 24, 1, twiddle_only=True)  # KoalaBear's largest size: the plan is made
    assert sum(pl.passes) == 24 and pl.elem_bytes == 4
    pl.close()
    so = L.load()
    h = C.c_void_p()
    assert so.ntt_plan_create_ex(C.byref(h), 5, 25, 1, 0, L.NTT_PLAN_TWIDDLE_ONLY) == L.NTT_ERR_FIELD
    assert so.ntt_plan_create(C.byref(h), 5, 25, 1, 0) == L.NTT_ERR_FIELD
    assert so.ntt_plan_create(C.byref(h), 4, 28, 1, 0) == L.NTT_ERR_FIELD
    # without the flag a one-limb custom plan of BabyBear is still refused; the multi-GPU plan refuses the fields
    assert so.ntt_plan_create_custom(C.byref(h), (C.c_uint64 * 1)(BABYBEAR), (C.c_uint64 * 1)(31), 1, 10,
                                     0) == L.NTT_ERR_FIELD
    devs = (C.c_int * 1)(0)
    for field_id in (4, 5):
        assert so.ntt_mplan_create(C.byref(h), field_id, 12, 1, 1, devs) == L.NTT_ERR_ARG


# ---- 8. the checked build
CHILD = r'''
import sys
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import numpy as np, torch
from ntt_amd import lib as L
import test_gpu_field31 as T
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
for fid in (4, 5):
    for lg in (3, T.TILE_LOG, T.TILE_LOG + 1):
        T.test_forward_inverse_against_the_oracle(fid, lg)
        assert T._plan(fid, lg).device_status() == 0, (fid, lg)
T.test_polymul_and_pointwise(4, 12)
assert T._plan(4, 12).device_status() == 0
T.test_batched_transforms(5, 256)
assert T._plan(4, 5).device_status() == 0
print("CLEAN-OK")
for fid in (4, 5):
    p = T.FIELDS[fid][0]
    for lg in (3, T.TILE_LOG, T.TILE_LOG + 1):
        pl = T._plan(fid, lg)
        x = T._random(1 << lg, 3, p)
        x[5] = p + 3
        pl.forward(T._dev(x))
        st = pl.device_status()
        assert st == 0x200, (fid, lg, hex(st))
        assert pl.device_status() == 0
print("INPUT-OK")
'''


def test_checked_build():
    """Test 1 (2^3, 2^13, 2^14), a polymul and a KIND_ROWS batch through libntt_debug.so: no check fires
    on legal data; one input word >= p is reported as 0x200 and nothing else."""
    assert os.path.exists(DEBUG_LIB), "libntt_debug.so not built (python -m ntt_amd.build --debug)"
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "CLEAN-OK" in r.stdout and "INPUT-OK" in r.stdout


# ---- 9. four-step over virtual ranks
def _index(layout, kind):
    i = torch.arange(layout.local_n, dtype=torch.int64, device="cuda:0")
    if kind == "row":
        a, j2 = i >> layout.log_n2, i & (layout.n2 - 1)
        return layout.rank * layout.r + a + layout.n1 * j2
    k1, kc = i >> layout.log_c, i & (layout.c - 1)  # column layout [n1][c]
    return layout.rank * layout.c + kc + layout.n2 * k1


def _smallest_rank_plan_log(field_id, world):
    from ntt_amd import lib as L
    from ntt_amd.distributed import VirtualRanks
    for lg in range(2, 16):
        try:
            return lg, VirtualRanks(field_id, lg, 1, world)
        except L.NTTError as e:
            assert e.status == L.NTT_ERR_ARG, (lg, e)
    raise AssertionError("no rank plan up to 2^15")


@pytest.mark.parametrize("field_id,world", [(4, 2), (4, 4), (5, 2), (5, 4)])
def test_four_step_virtual_ranks(field_id, world):
    """The smallest size the rank plan accepts for the world, then 2^14 (two-pass pieces on neither
    side, a longer exchange): forward equals the one-plan transform, inverse is a round trip."""
    from ntt_amd.distributed import VirtualRanks
    p, _ = FIELDS[field_id]
    lg0, vr0 = _smallest_rank_plan_log(field_id, world)
    for log_n, vr in ((lg0, vr0), (14, None)):
        vr = vr or VirtualRanks(field_id, log_n, 1, world)
        ref = _plan(field_id, log_n)
        x = ref.fill(ref.empty(), "random", seed=42)
        e = _edge(p)
        x[:len(e)] = _dev(np.array(e, dtype=np.uint64))
        x0 = x.clone()
        ref.forward(x)
        xs = vr.empty()
        assert all(t.dtype == torch.int32 for t in xs)
        for lay, t in zip(vr.layouts, xs):  # row-layout shares of the global vector
            t.copy_(x0[_index(lay, "row")])
        shares = [t.clone() for t in xs]
        vr.forward(xs)
        for lay, t in zip(vr.layouts, xs):
            assert torch.equal(t, x[_index(lay, "col")]), (world, log_n, lay.rank)
        vr.inverse(xs)
        for s, t in zip(shares, xs):
            assert torch.equal(s, t)
