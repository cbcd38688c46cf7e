"""The radix-2^29 arithmetic of ntt_amd/csrc/field29.hpp (the text the Eng29 kernels run) checked on the
host, primitive by primitive: tests/c/field29_check.cpp runs norm_u, norm_s, cond_sub, add29,
sub29_raw, sub29, mont29 / mont29_chain, mulc29 / mulc29_cc / mulc29_blk, mullo29, neg29, shoup_ws29,
inv_mod_B29 and pack29 / unpack29 on records generated here and writes the raw result limbs; every
result is checked against exact integer arithmetic (tests/f29_ref.py): value or congruence mod p,
bit-equality between the variants of one product, and every bound the header documents.  Per op and
modulus: the edge set's cross product and 10^5 seeded random records.  The same program built with
-fsanitize=address,undefined runs the same records (its own main: nothing is preloaded)."""
import itertools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import f29_np as N
from tests import f29_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "field29_check.cpp")
NRAND = 100_000
(OP_NORM_U, OP_NORM_S, OP_COND_SUB, OP_ADD, OP_SUB_RAW, OP_SUB, OP_MONT, OP_MULC, OP_MULLO, OP_NEG, OP_SHOUP_WS,
 OP_INV_B, OP_PACK, OP_UNPACK) = range(1, 15)
MODULI = ["bn254", "bls12_381", "edge_lo", "edge_hi", "below_2_250", "p300", "p380", "2_250_plus_1", "2_255_minus_19"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def _host_compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and (shutil.which(cand) or os.path.exists(cand)):
            return cand
    return None


_exe = {}


def _build(variant, tmp_path_factory):
    """The check program, plain or sanitized; (path, None) or (None, reason it could not be linked)."""
    if variant not in _exe:
        cxx = _host_compiler()
        if cxx is None:
            pytest.fail("no host C++ compiler found (g++, c++, clang++)")
        exe = str(tmp_path_factory.mktemp("f29") / f"field29_check_{variant}")
        cmd = [cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ntt_amd", "csrc"), SRC, "-o", exe]
        if variant == "sanitized":
            # does this compiler link the sanitizer runtimes at all?
            probe = str(tmp_path_factory.mktemp("f29p") / "probe")
            r = subprocess.run([cxx, *SAN, "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                               capture_output=True, text=True)
            if r.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
                _exe[variant] = (None, f"{cxx} cannot link -fsanitize=address,undefined: {r.stderr.strip()[-300:]}")
                return _exe[variant]
            cmd[1:1] = SAN
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _exe[variant] = (exe, None)
    return _exe[variant]


# ---------------------------------------------------------------- record generation
def _edges(p, limit, kmax):
    """0, 1, limb-boundary values, k p +- d for small d, limit - 1: everything in [0, limit)."""
    s = {0, 1, 2, (1 << 29) - 1, 1 << 29, (1 << 58) - 1, limit - 1, limit - 2}
    for k in list(range(0, kmax + 1)):
        for d in range(-3, 4):
            s.add(k * p + d)
    return sorted(v for v in s if 0 <= v < limit)


def _cross(a, b):
    pa, pb = zip(*itertools.product(a, b))
    return list(pa), list(pb)


class Batch:
    def __init__(self, op, L, W, arrays, check):
        self.op, self.L, self.W, self.check = op, L, W, check
        self.inp = np.ascontiguousarray(np.concatenate(arrays, axis=1), dtype=np.uint32)

    def header(self, C):
        return np.array([self.op, self.L, self.W, len(self.inp)] + C.M_p + C.M_p2 + [C.pinv] + C.pbar, dtype=np.uint32)


def _exact(exp_ints, L):
    exp = N.ints_to_limbs(exp_ints, L)

    def check(out, what):
        bad = np.nonzero((out != exp).any(axis=1))[0]
        assert bad.size == 0, (what, "record", int(bad[0]), out[bad[0]].tolist(), exp[bad[0]].tolist())
    return check


def _batches(name):
    p, _, L, _ = F.moduli()[name]
    C = F.Consts(p, L)
    Bv = C.B
    rng = random.Random(f"field29-{name}")
    nrg = np.random.default_rng(abs(hash(p)) % (1 << 32))
    lim = lambda vals: N.ints_to_limbs(vals, L)
    out = []

    # norm_u: any non-negative limbs whose carries fit (<= 2^32 - 8)
    x = nrg.integers(0, (1 << 32) - 7, (NRAND, L), dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([x, np.full((1, L), (1 << 32) - 8, np.uint32), np.full((1, L), (1 << 29) - 1, np.uint32),
                        np.full((1, L), 1 << 29, np.uint32), np.zeros((1, L), np.uint32), lim(_edges(p, Bv, 64))])
    vin = N.limb_values(x)

    def chk_norm_u(o, what, vin=vin):
        assert N.normalised(o, L - 1), what
        assert N.limb_values(o) == vin, what
    out.append(Batch(OP_NORM_U, L, 0, [x], chk_norm_u))

    # norm_s: int32 limbs whose carries fit; negative totals (a negative top limb) included
    xs = nrg.integers(-(1 << 31) + 4, (1 << 31) - 4, (NRAND, L), dtype=np.int64)
    ed = []
    for lo_, hi_ in [(-(1 << 31) + 4, -(1 << 31) + 4), ((1 << 31) - 5, (1 << 31) - 5), (-1, -1), (-(1 << 29), -(1 << 29)),
                     (-1, 0), (0, -1), ((1 << 29) - 1, -1), (-(1 << 29) - 1, 1)]:
        ed.append([lo_] * (L - 1) + [hi_])
    xs = np.concatenate([xs, np.array(ed, dtype=np.int64)]).astype(np.int32).view(np.uint32)
    vs = N.limb_values(xs, signed=True)
    assert min(vs) < 0 < max(vs)

    def chk_norm_s(o, what, vs=vs):
        assert N.normalised(o, L - 1), what
        assert (o[:, L] == o[:, L - 1]).all(), what
        assert (o[:-8, L - 1].view(np.int32) < 0).any()
        lo = N.limb_values(np.concatenate([o[:, :L - 1], np.zeros((len(o), 1), np.uint32)], axis=1))
        top = o[:, L - 1].view(np.int32).tolist()
        assert [a + (t << (29 * (L - 1))) for a, t in zip(lo, top)] == vs, what
    out.append(Batch(OP_NORM_S, L, 0, [xs], chk_norm_s))

    # cond_sub: x < 2q normalised, q = 2^j p
    xa, qa = [], []
    for j in range(5):
        q = p << j
        e = [v for v in _edges(q, 2 * q, 2)]
        r = N.rand_below(rng, NRAND // 5, 2 * q)
        xa += e + r
        qa += [q] * (len(e) + len(r))
    out.append(Batch(OP_COND_SUB, L, 0, [lim(xa), lim(qa)], _exact([a - q if a >= q else a for a, q in zip(xa, qa)], L)))

    # add29 / sub29_raw / sub29: a, b < 2p
    e = _edges(p, 2 * p, 2)
    ea, eb = _cross(e, e)
    a = ea + N.rand_below(rng, NRAND, 2 * p)
    b = eb + N.rand_below(rng, NRAND, 2 * p)
    la, lb = lim(a), lim(b)
    out.append(Batch(OP_ADD, L, 0, [la, lb], _exact([u + v - (2 * p if u + v >= 2 * p else 0) for u, v in zip(a, b)], L)))
    out.append(Batch(OP_SUB_RAW, L, 0, [la, lb], _exact([u - v + 2 * p for u, v in zip(a, b)], L)))
    out.append(Batch(OP_SUB, L, 0, [la, lb], _exact([u - v + (2 * p if u < v else 0) for u, v in zip(a, b)], L)))

    # mont29 / mont29_chain: a < 8p, b < 2p -> < 2p (field29.hpp); x < 32p, y < 4p -> < 3p (Eng29::mulv)
    for ka, kb, kr in ((8, 2, 2), (32, 4, 3)):
        ea, eb = _cross(_edges(p, ka * p, ka), _edges(p, kb * p, kb)[::2] + [kb * p - 1])
        a = ea + N.rand_below(rng, NRAND, ka * p)
        b = eb + N.rand_below(rng, NRAND, kb * p)

        def chk_mont(o, what, a=a, b=b, kr=kr):
            assert N.normalised(o), what
            assert (o[:, :L] == o[:, L:]).all(), (what, "mont29 != mont29_chain")
            r = N.limb_values(o[:, :L])
            Binv = C.Binv
            for j, (u, v, w) in enumerate(zip(a, b, r)):
                assert w < kr * p and (w - u * v * Binv) % p == 0, (what, j, u, v, w)
        out.append(Batch(OP_MONT, L, 0, [lim(a), lim(b)], chk_mont))

    # mulc29 / mulc29_cc / mulc29_blk: any x < B with limbs < 2^31, w < p
    ex = _edges(p, Bv, 64)
    ew = sorted({0, 1, 2, p - 1, p - 2, (p - 1) // 2, p >> 1, (1 << 29) - 1})
    ea, eb = _cross(ex, ew)
    lx = lim(ea)
    lx = np.concatenate([lx, N.push_down(lx, 3), N.push_down(lx, 1)])
    xv = ea * 3 + N.rand_below(rng, NRAND, Bv)
    wv = eb * 3 + N.rand_below(rng, NRAND, p)
    rx = N.push_down(lim(xv[len(lx):]), nrg.integers(0, 4, (NRAND, L - 1)))
    lx = np.concatenate([lx, rx])
    assert int(lx.max()) == (1 << 31) - 1 and max(xv) == Bv - 1
    ws = [C.shoup(w) for w in wv]

    def chk_mulc(o, what, xv=xv, wv=wv):
        assert N.normalised(o), what
        assert (o[:, :L] == o[:, L:2 * L]).all() and (o[:, :L] == o[:, 2 * L:]).all(), (what, "variants differ")
        r = N.limb_values(o[:, :L])
        p3 = 3 * p
        for j, (u, v, w) in enumerate(zip(xv, wv, r)):
            assert w < p3 and (w - u * v) % p == 0, (what, j, u, v, w)
    out.append(Batch(OP_MULC, L, 0, [lx, lim(wv), lim(ws)], chk_mulc))

    # mullo29, neg29: normalised operands < B
    e = _edges(p, Bv, 64)[::3] + [Bv - 1]
    ea, eb = _cross(e, e)
    a = ea + N.rand_below(rng, NRAND, Bv)
    b = eb + N.rand_below(rng, NRAND, Bv)
    out.append(Batch(OP_MULLO, L, 0, [lim(a), lim(b)], _exact([u * v % Bv for u, v in zip(a, b)], L)))
    out.append(Batch(OP_NEG, L, 0, [lim(a)], _exact([(Bv - u) % Bv for u in a], L)))

    # shoup_ws29: wR = w B mod p, p^-1 mod B -> floor(w B / p)
    w = [0, 1, 2, p - 1, p - 2, (p - 1) // 2] + N.rand_below(rng, NRAND, p)
    out.append(Batch(OP_SHOUP_WS, L, 0, [lim([u * Bv % p for u in w]), lim([C.pinvB] * len(w))],
                     _exact([C.shoup(u) for u in w], L)))

    # inv_mod_B29: any odd value
    m = [p, 1, 3, Bv - 1, Bv - 3, (1 << 29) + 1] + [v | 1 for v in N.rand_below(rng, NRAND, Bv)]
    out.append(Batch(OP_INV_B, L, 0, [lim(m)], _exact([pow(v, -1, Bv) for v in m], L)))
    return C, out


def _pack_batches():
    C = F.Consts(F.moduli()["bn254"][0], 9)  # the header's modulus fields are not used by these ops
    rng = random.Random("field29-pack")
    out = []
    for L, W in F.ENGINES:
        bits_w, bits_l = 32 * W, 29 * L
        lo = min(bits_w, bits_l)
        edge = [0, 1, (1 << lo) - 1, (1 << bits_w) - 1]
        edge += [1 << b for b in range(bits_w)]                                 # every single bit
        edge += [sum(1 << b for b in range(0, bits_w, 29)), sum(1 << b for b in range(28, bits_w, 29)),
                 sum(1 << b for b in range(0, bits_w, 32)), sum(1 << b for b in range(31, bits_w, 32))]
        v = edge + N.rand_below(rng, NRAND, 1 << bits_w)
        out.append(Batch(OP_PACK, L, W, [N.ints_to_words(v, W)], _exact([u & ((1 << bits_l) - 1) for u in v], L)))
        v = [u & ((1 << lo) - 1) for u in v]
        exp = N.ints_to_words(v, W)

        def chk(o, what, exp=exp):
            assert np.array_equal(o, exp), what
        C14 = C if L == 9 else F.Consts(F.moduli()["p300"][0], 14)
        out[-1].C = C14
        out.append(Batch(OP_UNPACK, L, W, [N.ints_to_limbs(v, L)], chk))
        out[-1].C = C14
    return out


def _nout(b):
    L, W = b.L, b.W
    return {OP_NORM_S: L + 1, OP_MONT: 2 * L, OP_MULC: 3 * L, OP_UNPACK: W}.get(b.op, L)


def _run_and_check(exe, batches, consts_of, tmp_path, what):
    rec, res = str(tmp_path / "records.bin"), str(tmp_path / "results.bin")
    with open(rec, "wb") as f:
        for b in batches:
            f.write(b.header(consts_of(b)).tobytes())
            f.write(b.inp.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, rec, res], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (what, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "field29_check:" in r.stdout and not r.stderr.strip(), (what, r.stderr[-3000:])
    o = np.fromfile(res, dtype=np.uint32)
    pos = 0
    for b in batches:
        n, w = len(b.inp), _nout(b)
        b.check(o[pos:pos + n * w].reshape(n, w), (what, "op", b.op, "L", b.L, "W32", b.W))
        pos += n * w
    assert pos == o.size, what
    os.remove(rec)
    os.remove(res)


def _exe_or_skip(variant, tmp_path_factory):
    exe, why = _build(variant, tmp_path_factory)
    if exe is None:
        pytest.skip(why)
    return exe


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
@pytest.mark.parametrize("name", MODULI)
def test_field29_primitives_match_exact_arithmetic(name, variant, tmp_path, tmp_path_factory):
    exe = _exe_or_skip(variant, tmp_path_factory)
    C, batches = _batches(name)
    _run_and_check(exe, batches, lambda b: C, tmp_path, (name, variant))


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_field29_pack_unpack(variant, tmp_path, tmp_path_factory):
    exe = _exe_or_skip(variant, tmp_path_factory)
    _run_and_check(exe, _pack_batches(), lambda b: b.C, tmp_path, ("pack", variant))


def test_reference_constants_and_moduli():
    """The reference's own consistency: the edge moduli sit where the issue puts them, the padded
    offsets keep their invariants, and the butterfly network is the DFT in bit-reversed slots."""
    M = F.moduli()
    assert M["edge_lo"][0] >> 232 == 1 << 18 and M["edge_hi"][0] >> 232 == (1 << 23) - 1
    for name, (p, g, L, prime) in M.items():
        C = F.Consts(p, L)
        assert C.red_ok == (1 if name in ("bn254", "bls12_381", "edge_lo", "edge_hi", "2_250_plus_1", "2_255_minus_19") else 0)
        C.check_pc(C.pc, top_nonneg=bool(C.red_ok))
        assert F.value(C.pbar) + p == C.B and (C.pinv * p + 1) % (1 << 29) == 0
        if prime:
            w8 = F.w8_of(p, g)
            rng = random.Random(name)
            for Q in (2, 4, 8):
                x = [rng.randrange(p) for _ in range(Q)]
                net, ref = F.dft_net(x, Q, w8, p), F.dft_direct(x, Q, w8, p)
                assert [net[F.brev(k, Q.bit_length() - 1)] for k in range(Q)] == ref
    assert F.red_inv_bits(1) == 0x3EFFFFFF and F.red_inv_bits((1 << 18)) == F._f32_bits_nearest(F.Fraction(1, (1 << 18) + 1)) - 1
    assert F.pack(F.words(F.MASK << 29, 8), 9) == [0, F.MASK] + [0] * 7
