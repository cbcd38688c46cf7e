"""Primitive-level GPU tests of the radix-2^29 engine (Eng29<9,8>, Eng29<9,12>, Eng29<14,12>): the probe
kernels of tests/c/field29_probe.hip run ONE primitive per element -- the products (the generated
inline-asm chains of field29_asm9.hpp among them), reduce_top / reduce / cond_sub_rare, the lazy
butterflies, dft_q / dft_q_fast, load / put / store -- and dump raw limbs; every output element is
checked against exact integer arithmetic (tests/f29_ref.py): congruence mod p, bit-equality between
the variants of one product, the documented value and limb bounds.  No tolerances.  The moduli include
the two ends of the quotient-estimate reduction's range (top 29-bit limb 2^18 and 2^23 - 1), which
also run whole transforms at the end of the file."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import f29_np as N
from tests import f29_ref as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "c", "libf29probe.so")
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")
ENG = {0: (9, 8), 1: (9, 12), 2: (14, 12)}
# (modulus, engine): every 9-limb modulus on Eng29<9,8>; the 48-B layout's engine differs only in its
# loads and stores, so it takes two of them; the 14-limb engine its two primes
CASES = [(m, 0) for m in ("bn254", "bls12_381", "edge_lo", "edge_hi", "below_2_250", "2_250_plus_1", "2_255_minus_19")]
CASES += [("bls12_381", 1), ("edge_hi", 1), ("p300", 2), ("p380", 2)]
PRIME_CASES = [c for c in CASES if F.moduli()[c[0]][3]]
PR_MUL, PR_MUL_U, PR_MULC, PR_MULC_CC, PR_MULC_BLK, PR_MULV, PR_MONT, PR_MONT_CHAIN = range(8)
# f29_reduce codes 100 + k: (FROM, TO, FAST, R32), the table of tests/c/field29_probe.hip
REDUCE = [(8, 4, 0, 1), (16, 4, 0, 1), (32, 4, 0, 1), (8, 4, 1, 1), (16, 4, 1, 1), (32, 4, 1, 1),
          (8, 4, 1, 0), (16, 4, 1, 0), (32, 4, 1, 0), (4, 2, 1, 1), (4, 2, 0, 1), (4, 1, 0, 1)]

_lib = None


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(LIB), "tests/c/libf29probe.so not built (python tests/field29_probe_build.py)"
        _lib = C.CDLL(LIB)
        P, I, U = C.c_void_p, C.c_int, C.c_uint32
        _lib.f29_engine_info.argtypes = [I, P]
        _lib.f29_args.argtypes = [I, P, P]
        _lib.f29_prod.argtypes = [I, I, P, P, P, P, P, U]
        _lib.f29_reduce.argtypes = [I, I, P, P, P, U]
        _lib.f29_store.argtypes = [I, I, I, P, P, P, U]
        _lib.f29_load.argtypes = [I, I, P, P, U]
        _lib.f29_dft.argtypes = [I, I, P, P, P, P, U]
        for f in ("f29_engine_info", "f29_args", "f29_prod", "f29_reduce", "f29_store", "f29_load", "f29_dft"):
            getattr(_lib, f).restype = I
    return _lib


def _hp(a):
    """Host pointer of a contiguous uint32 array (kept alive by the caller)."""
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def _pad(a):
    """Rows up to a multiple of 64 (whole waves), by repeating row 0."""
    k = -len(a) % 64
    return np.ascontiguousarray(np.concatenate([a, np.repeat(a[:1], k, axis=0)]) if k else a, dtype=np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def _run(fn, head, ins, out_words, n_real):
    """Pad the (n, k) inputs to whole waves, launch, return the first n_real rows of the output."""
    ins = [_pad(a) for a in ins]
    n = len(ins[0])
    assert all(len(a) == n for a in ins) and n <= 65536
    devs = [_dev(a) for a in ins]
    out = torch.zeros(n * out_words, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = fn(*head, *[t.data_ptr() for t in devs], out.data_ptr(), n)
    assert rc == 0, rc
    return out.cpu().numpy().view(np.uint32).reshape(n, out_words)[:n_real]


class Ctx:
    def __init__(self, name, eng):
        self.name, self.eng = name, eng
        self.p, self.g, L, self.prime = F.moduli()[name]
        self.L, self.W = ENG[eng]
        assert L == self.L
        self.C = F.Consts(self.p, L)
        self.pw = np.array(F.words(self.p, self.W), dtype=np.uint32)
        self.fast = bool(self.C.red_ok) and L == 9
        self.rng = random.Random(f"gpu-{name}-{eng}")
        self.nrg = np.random.default_rng(self.p % (1 << 32) + eng)

    def lim(self, vals):
        return N.ints_to_limbs(vals, self.L)

    def tw(self, ws):
        """(w, ws) limb rows of canonical twiddles."""
        return np.concatenate([self.lim(ws), self.lim([self.C.shoup(w) for w in ws])], axis=1)

    def w8(self):
        return np.ascontiguousarray(self.tw(F.w8_of(self.p, self.g)).reshape(-1))

    def prod(self, mode, x, tw, tu=None):
        tu = np.zeros(2 * self.L, np.uint32) if tu is None else np.ascontiguousarray(tu.reshape(-1))
        return _run(lambda *a: lib().f29_prod(self.eng, mode, _hp(self.pw), a[0], a[1], _hp(tu), a[2], a[3]),
                    (), [x, tw], self.L, len(x))

    def reduce(self, code, x):
        return _run(lambda *a: lib().f29_reduce(self.eng, code, _hp(self.pw), *a), (), [x], self.L, len(x))

    def store(self, mw, code, x):
        return _run(lambda *a: lib().f29_store(self.eng, mw, code, _hp(self.pw), *a), (), [x], mw, len(x))

    def dft(self, code, x8):
        w8 = self.w8()
        n = len(x8)
        out = _run(lambda *a: lib().f29_dft(self.eng, code, _hp(self.pw), _hp(w8), *a), (),
                   [x8.reshape(n, 8 * self.L)], 8 * self.L, n)
        return out.reshape(n, 8, self.L)


def _edges(p, limit, kmax):
    s = {0, 1, (1 << 29) - 1, 1 << 29, limit - 1}
    for k in range(kmax + 1):
        for d in range(-2, 3):
            s.add(k * p + d)
    return sorted(v for v in s if 0 <= v < limit)


def _check_products(out, xv, wv, p, what, bound=3):
    assert N.normalised(out), what
    for j, (r, x, w) in enumerate(zip(N.limb_values(out), xv, wv)):
        assert r < bound * p and (r - x * w) % p == 0, (what, j, x, w, r)


# ---------------------------------------------------------------- args
@pytest.mark.parametrize("name,eng", CASES)
def test_field29_args(name, eng):
    c = Ctx(name, eng)
    L, K = c.L, c.C
    info = np.zeros(5, np.int32)
    assert lib().f29_engine_info(eng, info.ctypes.data_as(C.c_void_p)) == 0
    assert info.tolist()[:2] == [L, c.W] and info[4] == (1 if L == 9 else 0)
    out = np.zeros(13 * L + 3, np.uint32)
    assert lib().f29_args(eng, _hp(c.pw), _hp(out)) == 0
    o = out.tolist()
    got = {"p": o[:L], "p2": o[L:2 * L], "pinv": o[2 * L], "kp": [o[2 * L + 1 + j * L:2 * L + 1 + (j + 1) * L] for j in range(5)]}
    q = 7 * L + 1
    got.update(pbar=o[q:q + L], red_inv=o[q + L], red_ok=o[q + L + 1],
               pc=[o[q + L + 2 + j * L:q + L + 2 + (j + 1) * L] for j in range(5)])
    assert got["p"] == K.M_p and got["p2"] == K.M_p2 and got["pinv"] == K.pinv and got["kp"] == K.kp
    assert got["pbar"] == K.pbar and got["red_ok"] == K.red_ok
    assert got["red_inv"] == K.red_inv, (hex(got["red_inv"]), hex(K.red_inv))
    assert got["pc"] == [[v & 0xFFFFFFFF for v in row] for row in K.pc]
    K.check_pc(got["pc"], top_nonneg=bool(K.red_ok))


# ---------------------------------------------------------------- products
@pytest.mark.parametrize("name,eng", CASES)
def test_field29_products(name, eng, tmp_path, tmp_path_factory):
    c = Ctx(name, eng)
    p, L, Bv = c.p, c.L, c.C.B
    # x: edges (normalised and with 3 units of 2^29 pushed down every limb) and random values < B with
    # limbs up to 2^31 - 1; w: edges and random, per lane
    ex = _edges(p, Bv, 64)
    ew = [0, 1, 2, p - 1, p - 2, (p - 1) // 2]
    xv = [x for x in ex for _ in ew]
    wv = [w for _ in ex for w in ew]
    lx = c.lim(xv)
    lx = np.concatenate([lx, N.push_down(lx, 3)])
    xv, wv = xv * 2, wv * 2
    nr = 8192
    rx = N.rand_below(c.rng, nr, Bv)
    lx = np.concatenate([lx, N.push_down(c.lim(rx), c.nrg.integers(0, 4, (nr, L - 1)))])
    xv, wv = xv + rx, wv + N.rand_below(c.rng, nr, p)
    assert int(lx.max()) == (1 << 31) - 1
    tw = c.tw(wv)
    outs = {m: c.prod(m, lx, tw) for m in (PR_MUL, PR_MULC, PR_MULC_CC, PR_MULC_BLK)}
    for m in (PR_MULC, PR_MULC_CC, PR_MULC_BLK):
        assert np.array_equal(outs[PR_MUL], outs[m]), (name, eng, "E::mul differs from product form", m)
    _check_products(outs[PR_MUL], xv, wv, p, (name, eng, "mul"))
    # ... and bit-equal to the host build of the same header
    from tests import test_field29_host as H
    exe, why = H._build("plain", tmp_path_factory)
    b = H.Batch(H.OP_MULC, L, 0, [lx, tw], None)
    rec, res = str(tmp_path / "rec.bin"), str(tmp_path / "res.bin")
    with open(rec, "wb") as f:
        f.write(b.header(c.C).tobytes())
        f.write(b.inp.tobytes())
    subprocess.run([exe, rec, res], check=True, capture_output=True, timeout=120)
    hostout = np.fromfile(res, dtype=np.uint32).reshape(len(lx), 3 * L)
    assert np.array_equal(hostout[:, :L], outs[PR_MUL]), (name, eng, "device product differs from the host's")

    # mul_u: the twiddle as a kernel argument (wave-uniform), one launch per twiddle
    tws = [0, 1, p - 1, 2, p - 2, (p - 1) // 2] + (F.w8_of(p, c.g) if c.prime else [3, 5, 7])
    tws += N.rand_below(c.rng, 16 - len(tws), p)
    sub = np.concatenate([lx[:len(ex) * len(ew) * 2:7], lx[-512:]])
    subv = (xv[:len(ex) * len(ew) * 2:7] + xv[-512:])
    for w in tws:
        t1 = c.tw([w])
        got = c.prod(PR_MUL_U, sub, np.zeros((len(sub), 2 * L), np.uint32), t1)
        ref = c.prod(PR_MULC, sub, np.repeat(t1, len(sub), axis=0))
        assert np.array_equal(got, ref), (name, eng, "mul_u differs from mulc29", w)
        _check_products(got, subv, [w] * len(sub), p, (name, eng, "mul_u", w))

    # the stage-3 outputs of dft_q_fast<8> (limbs up to 2^31, values up to 33p) as product inputs
    if c.fast and c.prime:
        x8 = _dft_inputs(c, 64)
        y = c.dft(22, x8).reshape(-1, L)
        yv = N.limb_values(y)
        wq = N.rand_below(c.rng, len(y), p)
        got = c.prod(PR_MUL, y, c.tw(wq))
        assert np.array_equal(got, c.prod(PR_MULC, y, c.tw(wq)))
        _check_products(got, yv, wq, p, (name, eng, "mul of dft_q_fast outputs"))

    # mulv: x < 32p, y < 4p at their maxima and random; x y / B mod p, < 3p
    ea, eb = _edges(p, 32 * p, 32)[::3] + [32 * p - 1], [0, 1, p - 1, p, 2 * p - 1, 4 * p - 2, 4 * p - 1]
    a = [u for u in ea for _ in eb] + N.rand_below(c.rng, 4096, 32 * p)
    bq = [v for _ in ea for v in eb] + N.rand_below(c.rng, 4096, 4 * p)
    ya = np.concatenate([c.lim(bq), np.zeros((len(bq), L), np.uint32)], axis=1)
    mv = {m: c.prod(m, c.lim(a), ya) for m in (PR_MULV, PR_MONT, PR_MONT_CHAIN)}
    assert np.array_equal(mv[PR_MULV], mv[PR_MONT]) and np.array_equal(mv[PR_MULV], mv[PR_MONT_CHAIN])
    assert N.normalised(mv[PR_MULV])
    for j, (r, u, v) in enumerate(zip(N.limb_values(mv[PR_MULV]), a, bq)):
        assert r < 3 * p and (r - u * v * c.C.Binv) % p == 0, (name, eng, "mulv", j, u, v, r)


# ---------------------------------------------------------------- reductions
def _reduce_inputs(c):
    """k p - d, k p + d (k = 1..33, d = 0..39) and random (k - 1) p + r: values, normalised limbs, and
    the same with up to 3 units of 2^29 pushed down from limb i + 1 into limb i (what dft_q_fast hands over)."""
    p, L = c.p, c.L
    v = [k * p - d for k in range(1, 34) for d in range(40)] + [k * p + d for k in range(1, 34) for d in range(40)]
    v += [(k - 1) * p + r for k in range(1, 34) for r in N.rand_below(c.rng, 120, p)]
    l0 = c.lim(v)
    l1 = N.push_down(l0, c.nrg.integers(0, 4, (len(v), L - 1)))
    l2 = N.push_down(l0, 3)
    return v, l0, np.concatenate([l0, l1, l2]), v * 3


def _check_reduced(out, vin, p, to, what):
    assert N.normalised(out), what
    for j, (r, x) in enumerate(zip(N.limb_values(out), vin)):
        assert r < to * p and (r - x) % p == 0, (what, j, x, r)


@pytest.mark.parametrize("name,eng", CASES)
def test_field29_reductions(name, eng):
    c = Ctx(name, eng)
    p, L = c.p, c.L
    v, l0, lall, vall = _reduce_inputs(c)
    sel = lambda vals, lim_, frm: ([x for x in vals if x < frm * p], lim_[np.array([x < frm * p for x in vals])])
    if c.fast:
        for code in (0, 1):  # bare reduce_top: [0, 2p), and the follow-up subtraction has work to do
            out = c.reduce(code, lall)
            _check_reduced(out, vall, p, 2, (name, eng, "reduce_top", code))
            share = sum(r >= p for r in N.limb_values(out)) / len(out)
            print(f"reduce_top<{'true' if code == 0 else 'false'}> {name} eng {eng}: {100 * share:.2f} % of outputs >= p")
            assert share >= 0.01, (name, eng, code, share)
    else:
        assert lib().f29_reduce(eng, 0, _hp(c.pw), 0, 0, 64) == -2  # no quotient estimate on this modulus
    for k, (frm, to, fast, r32) in enumerate(REDUCE):
        if fast and not c.fast:
            continue
        raw = fast and frm > 4  # reduce_top takes the unnormalised forms; the subtraction chains do not
        vv, ll = sel(vall, lall, frm) if raw else sel(v, l0, frm)
        _check_reduced(c.reduce(100 + k, ll), vv, p, to, (name, eng, "reduce", frm, to, fast, r32))
    # through store (-> 1, canonical) and store_lazy (-> 2), as HBM words
    for code in range(1, 11):
        fast = code % 2 == 0
        if fast and not c.fast:
            continue
        frm, to = (4, 2) if code >= 9 else (4 << ((code - 1) // 2), 1)
        raw = fast and frm > 4
        vv, ll = sel(vall, lall, frm) if raw else sel(v, l0, frm)
        got = N.words_to_ints(c.store(c.W, code, ll))
        if to == 1:
            assert got == [x % p for x in vv], (name, eng, "store", frm, fast)
        else:
            assert all(r < 2 * p and (r - x) % p == 0 for r, x in zip(got, vv)), (name, eng, "store_lazy", fast)


@pytest.mark.parametrize("name,eng", CASES)
def test_field29_cond_sub_rare_lane_patterns(name, eng):
    """Waves in which no lane, every lane, or exactly one lane (0, 31, 32, 63) needs the subtraction;
    'no lane' both with top limbs below q's (branch not taken) and equal to it (taken, nothing to do)."""
    c = Ctx(name, eng)
    for code, q in ((2, c.p), (3, 2 * c.p)):
        rb = lambda lo, hi: lo + c.rng.randrange(hi - lo)
        waves = [[rb(0, q >> 30) for _ in range(64)],                    # top limb far below q's
                 [q - 1 - i for i in range(64)],                           # just below q
                 [rb(q, 2 * q) for _ in range(62)] + [q, 2 * q - 1]]     # every lane
        for lane in (0, 31, 32, 63):
            for hi in (False, True):
                w = [rb(0, q >> 30) if not hi else q - 1 - c.rng.randrange(1 << 20) for _ in range(64)]
                w[lane] = (q, 2 * q - 1, rb(q, 2 * q))[lane % 3]
                waves.append(w)
        vals = [x for w in waves for x in w]
        out = c.reduce(code, c.lim(vals))
        assert np.array_equal(out, c.lim([x - q if x >= q else x for x in vals])), (name, eng, code)


# ---------------------------------------------------------------- butterflies and register DFTs
def _dft_inputs(c, nrand):
    """(n, 8, L) inputs < 4p, normalised: all 4p - 1, all 0, alternating 0 / 4p - 1 (both phases, and in
    pairs and fours), one slot at 4p - 1, random."""
    p, m = c.p, 4 * c.p - 1
    rows = [[m] * 8, [0] * 8, [0, m] * 4, [m, 0] * 4, [0, 0, m, m] * 2, [m, m, 0, 0] * 2, [0] * 4 + [m] * 4, [m] * 4 + [0] * 4]
    rows += [[m if s == k else 0 for s in range(8)] for k in range(8)] + [[0 if s == k else m for s in range(8)] for k in range(8)]
    rows += [[(0, 1, p - 1, p, 2 * p, m)[c.rng.randrange(6)] for _ in range(8)] for _ in range(40)]
    rows += [N.rand_below(c.rng, 8, 4 * p) for _ in range(nrand)]
    flat = [x for r in rows for x in r]
    return c.lim(flat).reshape(len(rows), 8, c.L)


@pytest.mark.parametrize("name,eng", PRIME_CASES)
def test_field29_butterflies_and_dfts(name, eng):
    c = Ctx(name, eng)
    p, L = c.p, c.L
    w8 = F.w8_of(p, c.g)
    # bfly_l<K>: a, b < K p -> (a + b, a - b + K p), exactly, normalised
    for code, K in ((0, 4), (1, 8), (2, 16)):
        e = _edges(p, K * p, K)[::2] + [K * p - 1]
        a = [u for u in e for _ in e] + N.rand_below(c.rng, 1024, K * p)
        b = [v for _ in e for v in e] + N.rand_below(c.rng, 1024, K * p)
        x8 = np.zeros((len(a), 8, L), np.uint32)
        x8[:, 0], x8[:, 1] = c.lim(a), c.lim(b)
        o = c.dft(code, x8)
        assert np.array_equal(o[:, 0], c.lim([u + v for u, v in zip(a, b)])), (name, eng, "bfly_l sum", K)
        assert np.array_equal(o[:, 1], c.lim([u - v + K * p for u, v in zip(a, b)])), (name, eng, "bfly_l diff", K)
        assert not o[:, 2:].any()
    for code, K, w in ((3, 4, w8[0]), (4, 4, w8[1]), (5, 4, w8[2]), (6, 8, w8[1])):
        a, b = N.rand_below(c.rng, 1024, K * p) + [K * p - 1, 0], N.rand_below(c.rng, 1024, K * p) + [0, K * p - 1]
        x8 = np.zeros((len(a), 8, L), np.uint32)
        x8[:, 0], x8[:, 1] = c.lim(a), c.lim(b)
        o = c.dft(code, x8)
        assert np.array_equal(o[:, 0], c.lim([u + v for u, v in zip(a, b)]))
        _check_products(o[:, 1], [u - v for u, v in zip(a, b)], [w] * len(a), p, (name, eng, "bfly_w_l", code))
    # dft_q / dft_q_fast: slot brev(k) = X_k; the documented (limb, value) bounds
    x8 = _dft_inputs(c, 1024 - 64)
    xv = np.array(N.limb_values(x8.reshape(-1, L)), dtype=object).reshape(-1, 8)
    bounds = {2: (3 << 29, 9), 4: (5 << 29, 17), 8: (1 << 31, 33)}  # 1.5 2^30, 2.5 2^30, 2^31
    for qi, Q in enumerate((2, 4, 8)):
        ref = [F.dft_direct(list(r[:Q]), Q, w8, p) for r in xv]
        slot = [F.brev(k, Q.bit_length() - 1) for k in range(Q)]
        o = c.dft(10 + qi, x8)
        assert N.normalised(o.reshape(-1, L)), (name, eng, "dft_q limbs", Q)
        ov = np.array(N.limb_values(o.reshape(-1, L)), dtype=object).reshape(-1, 8)
        for j, (r, e) in enumerate(zip(ov, ref)):
            for k in range(Q):
                assert r[slot[k]] < 4 * Q * p and (r[slot[k]] - e[k]) % p == 0, (name, eng, "dft_q", Q, j, k)
        assert np.array_equal(o[:, Q:], x8[:, Q:])
        if not c.fast:
            assert lib().f29_dft(eng, 20 + qi, _hp(c.pw), _hp(c.w8()), 0, 0, 64) == -2
            continue
        f = c.dft(20 + qi, x8)
        fv = np.array(N.limb_values(f.reshape(-1, L)), dtype=object).reshape(-1, 8)
        lb, vb = bounds[Q]
        assert int(f[:, :Q].max()) <= lb, (name, eng, "dft_q_fast limb bound", Q, int(f[:, :Q].max()), lb)
        for j, (r, r0, e) in enumerate(zip(fv, ov, ref)):
            for k in range(Q):
                s = slot[k]
                # a limb that wrapped below zero shows here: the value is off by a multiple of 2^32 2^(29 i)
                assert r[s] < vb * p and (r[s] - e[k]) % p == 0 and (r[s] - r0[s]) % p == 0, (name, eng, "dft_q_fast", Q, j, k)
        assert np.array_equal(f[:, Q:], x8[:, Q:])


# ---------------------------------------------------------------- load / put / store
@pytest.mark.parametrize("eng", [0, 1, 2])
def test_field29_load_put_store(eng):
    """The device pack29 (v_alignbit) and unpack29 against exact repacking, for MEMW, SCRW and TABW, on
    values with every limb- and word-boundary bit set; Eng29<9,12> ignores words 8..11 on load and
    writes them as zero."""
    name = "p380" if eng == 2 else "bls12_381"
    c = Ctx(name, eng)
    p, L = c.p, c.L
    info = np.zeros(5, np.int32)
    lib().f29_engine_info(eng, info.ctypes.data_as(C.c_void_p))
    assert info.tolist()[1:4] == {0: [8, 8, 8], 1: [12, 8, 8], 2: [12, 12, 12]}[eng]
    for mw in sorted(set(info.tolist()[1:4])):
        bits = 32 * mw
        live = 256 if L == 9 else bits           # the 256-bit class reads 32 B of an element
        fit = min(live, 29 * L)
        edge = [0, 1, (1 << fit) - 1] + [1 << b for b in range(fit)]
        edge += [sum(1 << b for b in range(s, fit, st)) for st in (29, 32) for s in (0, st - 1)]
        edge += [((1 << fit) - 1) ^ (1 << b) for b in range(0, fit, 29)]
        v = edge + N.rand_below(c.rng, 2048, 1 << fit)
        w = N.ints_to_words(v, mw)
        if live < bits:  # garbage above the 32 live bytes must be ignored
            w[:, 8:] = c.nrg.integers(0, 1 << 32, (len(v), mw - 8), dtype=np.uint64).astype(np.uint32)
        got = _run(lambda *a: lib().f29_load(eng, mw, *a), (), [w], L, len(v))
        assert np.array_equal(got, c.lim(v)), (eng, mw, "load")
        back = c.store(mw, 0, c.lim(v))
        assert np.array_equal(back, N.ints_to_words(v, mw)), (eng, mw, "put")  # words above the value: zero
        # store (canonical) and store_lazy (< 2p) of products (< 4p)
        x = _edges(p, 4 * p, 4) + N.rand_below(c.rng, 2048, 4 * p)
        assert N.words_to_ints(c.store(mw, 1, c.lim(x))) == [u % p for u in x], (eng, mw, "store")
        lz = N.words_to_ints(c.store(mw, 9, c.lim(x)))
        assert lz == [u - 2 * p if u >= 2 * p else u for u in x], (eng, mw, "store_lazy")


# ---------------------------------------------------------------- whole transforms at the red_ok edges
def _edge_inputs(p, n, log_n, kind):
    rng = np.random.default_rng(log_n)
    if kind == "near_p":  # the pattern of test_gpu_edges.test_adversarial_near_p_against_oracle
        pattern = rng.integers(0, 4, n)
        return [(p - 1, p - 2, 0, p - 1 - int(rng.integers(0, 1 << 20)))[int(s)] for s in pattern]
    return [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)]


def _red_ok_edge_transforms():
    from ntt_amd.ntt import NTTPlan
    from oracle import oracle_c as OC
    for name, (p, g) in F.edge_plan_primes().items():
        assert F.Consts(p, 9).red_ok == 1
        for log_n in (12, 14):
            pl = NTTPlan(log_n=log_n, limbs64=4, modulus=p, generator=g)
            assert len(pl.passes) >= 2, (name, log_n, pl.passes)
            for kind in ("near_p", "random"):
                x = OC.ints_to_limbs(_edge_inputs(p, 1 << log_n, log_n, kind), 4)
                t = torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to("cuda:0").reshape(-1, 4)
                pl.forward(t)
                got = t.cpu().numpy().view(np.uint64).reshape(-1, 4)
                assert np.array_equal(got, OC.ntt_mp(x, p, g, False)), (name, log_n, kind, "forward")
                pl.inverse(t)
                assert np.array_equal(t.cpu().numpy().view(np.uint64).reshape(-1, 4), x), (name, log_n, kind, "round trip")
                assert pl.device_status() == 0, (name, log_n, kind)
    print("RED-OK-EDGES-OK")


def test_field29_red_ok_edge_transforms():
    """4-limb custom plans on primes whose top 29-bit limb is exactly 2^18 (the smallest the FAST
    kernels accept) and 2^23 - 1 (the largest): multi-pass sizes, bit-exact against the C oracle.  The
    primes are k 2^14 + 1 (f29_ref.edge_plan_primes): 2^14 needs that two-adicity, and plan creation
    refuses the largest k 2^12 + 1 below 2^255, whose top 32-bit word is 0x7fffffff."""
    _red_ok_edge_transforms()


CHILD = """
import sys
sys.path.insert(0, ROOT)
from tests.test_gpu_field29 import _red_ok_edge_transforms
_red_ok_edge_transforms()
"""


def test_field29_red_ok_edge_transforms_checked_build():
    """The same through libntt_debug.so (in-kernel bounds / canonical / lazy-bound checks), in a child."""
    assert os.path.exists(DEBUG_LIB), "libntt_debug.so not built (python -m ntt_amd.build --debug)"
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "RED-OK-EDGES-OK" in r.stdout
