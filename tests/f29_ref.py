"""Exact reference for the radix-2^29 field engine (ntt_amd/csrc/field29.hpp, the Eng29 part of
engines.hpp, eng29_args.hpp), in plain Python ints: limb packing, the Args constants from their
definitions, Shoup companions and the register DFT network of dft_q.  Shared by the host check
(tests/test_field29_host.py) and the GPU probe (tests/test_gpu_field29.py)."""
from fractions import Fraction

MASK = (1 << 29) - 1
# (L, W32) of the three engines: Eng29<9,8>, Eng29<9,12>, Eng29<14,12>
ENGINES = [(9, 8), (9, 12), (14, 12)]
# padded-offset slots of Eng29 (engines.hpp PC_*): slot -> (K, pad)
PC = [(5, 1 << 29), (9, 1 << 30), (4, 1 << 29), (17, 1 << 29), (7, 1 << 30)]


def B(L: int) -> int:
    return 1 << (29 * L)


# ---------------------------------------------------------------- limbs and words
def limbs(v: int, L: int):
    """Normalised 29-bit limbs of 0 <= v < 2^(29 L)."""
    assert 0 <= v < B(L)
    return [(v >> (29 * i)) & MASK for i in range(L)]


def value(x, signed_top=False) -> int:
    """Value of a limb vector (any limb sizes; signed_top: limbs are int32 values)."""
    if signed_top:
        x = [l - (1 << 32) if l >= 1 << 31 else l for l in x]
    return sum(int(l) << (29 * i) for i, l in enumerate(x))


def words(v: int, W32: int):
    assert 0 <= v < 1 << (32 * W32)
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(W32)]


def from_words(w) -> int:
    return sum(int(x) << (32 * k) for k, x in enumerate(w))


def pack(w, L: int):
    """pack29<L, W32>: the low 29 L bits of the W32-word value as normalised limbs."""
    return limbs(from_words(w) & (B(L) - 1), L)


def unpack(x, W32: int):
    """unpack29<L, W32>: normalised limbs whose value fits 32 W32 bits -> words."""
    return words(value(x), W32)


# ---------------------------------------------------------------- float32, exactly
def _f32_bits_nearest(r: Fraction) -> int:
    """Bit pattern of the float32 nearest to r > 0 (ties to even; normal range)."""
    e = r.numerator.bit_length() - r.denominator.bit_length()
    if Fraction(2) ** e > r:
        e -= 1
    assert Fraction(2) ** e <= r < Fraction(2) ** (e + 1)
    m = r / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    n, rem = divmod(m.numerator, m.denominator)
    twice = 2 * rem
    if twice > m.denominator or (twice == m.denominator and n & 1):
        n += 1
    if n == 1 << 24:
        n, e = 1 << 23, e + 1
    assert -126 <= e <= 127
    return ((e + 127) << 23) | (n - (1 << 23))


def f32_from_bits(b: int) -> Fraction:
    e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
    assert 0 < e < 255
    return Fraction((1 << 23) | m) * Fraction(2) ** (e - 127 - 23)


def red_inv_bits(ptop: int) -> int:
    """float32 nextafter(1.0f / (float)(p_top + 1), 0): bit pattern."""
    d = f32_from_bits(_f32_bits_nearest(Fraction(ptop + 1)))  # (float)(p_top + 1u)
    return _f32_bits_nearest(1 / d) - 1                       # positive: one ulp toward zero


# ---------------------------------------------------------------- Args constants
class Consts:
    """The modulus-derived fields of Eng29<L, ...>::Args, from their definitions."""

    def __init__(self, p: int, L: int):
        assert p & 1 and 64 * p <= B(L)
        self.p, self.L, self.B = p, L, B(L)
        self.M_p = limbs(p, L)
        self.M_p2 = limbs(2 * p, L)
        self.kp = [limbs(p << j, L) for j in range(5)]
        self.pbar = limbs(self.B - p, L)
        self.pinv = (-pow(p, -1, 1 << 29)) % (1 << 29)
        self.ptop = p >> (29 * (L - 1))
        self.red_ok = 1 if self.ptop >= 1 << 18 else 0
        self.red_inv = red_inv_bits(self.ptop)
        self.pc = []
        for K, pad in PC:
            b = pad >> 29
            k = limbs(K * p, L)
            self.pc.append([k[0] + pad] + [k[i] + pad - b for i in range(1, L - 1)] + [k[L - 1] - b])
        self.pinvB = pow(p, -1, self.B)
        self.Binv = pow(self.B, -1, p)

    def shoup(self, w: int) -> int:
        assert 0 <= w < self.p
        return w * self.B // self.p

    def check_pc(self, pc, top_nonneg=True):
        """The invariants of the padded offsets: value exactly K p, c_0 >= pad, the other lower limbs
        >= pad - pad / 2^29 (the largest limb a subtrahend under that pad can have: 2^29 - 1 for
        normalised limbs, 2^30 - 2 for a sum of two; equality where a limb of K p is zero, as for
        p = 2^250 + small), top limb >= 0."""
        for (K, pad), c in zip(PC, pc):
            c = [int(v) for v in c]
            top = c[-1] - (1 << 32) if c[-1] >= 1 << 31 else c[-1]
            assert value(c[:-1]) + (top << (29 * (self.L - 1))) == K * self.p, (K, c)
            assert c[0] >= pad and all(v >= pad - (pad >> 29) for v in c[1:-1]), (K, pad, c)
            assert all(v < 1 << 32 for v in c)
            if top_nonneg:
                assert top >= 0, (K, c)


# ---------------------------------------------------------------- moduli
def is_prime(n: int) -> bool:
    if n < 2:
        return False
    for sp in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % sp == 0:
            return n == sp
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def non_residue(p: int) -> int:
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return g


def ntt_prime_from(start: int, two_adicity: int, step: int):
    """First prime k 2^v + 1 at or after (step = +1) / before (step = -1) `start`, and a quadratic
    non-residue g (g^((p-1)/n) is a primitive n-th root for every n | 2^v)."""
    k = (start - 1) >> two_adicity
    if step > 0 and (k << two_adicity) + 1 < start:
        k += 1
    while not is_prime((k << two_adicity) + 1):
        k += step
    p = (k << two_adicity) + 1
    return p, non_residue(p)


_cache = {}


def moduli():
    """name -> (p, g or None, L, prime).  g: a quadratic non-residue (primes only)."""
    if _cache:
        return _cache
    from oracle import ntt_ref as R
    m = {}
    m["bn254"] = (*R.FIELDS[1], 9, True)
    m["bls12_381"] = (*R.FIELDS[2], 9, True)
    lo = ntt_prime_from(1 << 250, 12, +1)      # smallest k 2^12 + 1 >= 2^250
    hi = ntt_prime_from(1 << 255, 12, -1)      # largest one below 2^255
    below = ntt_prime_from(1 << 250, 12, -1)   # just below 2^250
    assert lo[0] >= 1 << 250 and lo[0] >> 232 == 1 << 18           # red_ok = 1 at its edge
    assert hi[0] < 1 << 255 and hi[0] >> 232 == (1 << 23) - 1
    assert below[0] < 1 << 250 and below[0] >> 232 == (1 << 18) - 1  # red_ok = 0
    m["edge_lo"] = (*lo, 9, True)
    m["edge_hi"] = (*hi, 9, True)
    m["below_2_250"] = (*below, 9, True)
    for bits in (300, 380):  # the 384-bit class primes of tests/test_gpu_parity.py
        m[f"p{bits}"] = (*ntt_prime_from(1 << (bits - 1), 24, +1), 14, True)
    m["2_250_plus_1"] = ((1 << 250) + 1, None, 9, False)
    m["2_255_minus_19"] = ((1 << 255) - 19, None, 9, False)
    _cache.update(m)
    return _cache


def edge_plan_primes():
    """The red_ok edges as plan moduli: primes k 2^14 + 1 (sizes up to 2^14) whose top 29-bit limb is
    exactly 2^18 / 2^23 - 1.  The upper one lies below 2^255 - 2^224: the host arithmetic of plan
    creation takes moduli whose top 32-bit word is below 2^31 - 1, which the largest k 2^12 + 1 below
    2^255 (moduli()["edge_hi"], top word 0x7fffffff) is not."""
    lo = ntt_prime_from(1 << 250, 14, +1)
    hi = ntt_prime_from((1 << 255) - (1 << 224), 14, -1)
    assert lo[0] >> 232 == 1 << 18 and hi[0] >> 232 == (1 << 23) - 1 and hi[0] >> 224 < 0x7FFFFFFF
    return {"edge_lo": lo, "edge_hi": hi}


def w8_of(p: int, g: int):
    """[w, w^2, w^3] for a primitive 8th root of unity w (the Args::w8 constants' values)."""
    w = pow(g, (p - 1) // 8, p)
    assert pow(w, 4, p) == p - 1
    return [w, w * w % p, w * w * w % p]


# ---------------------------------------------------------------- register DFT
def brev(v: int, bits: int) -> int:
    return int(format(v, f"0{bits}b")[::-1], 2) if bits else 0


def dft_net(x, Q: int, w8, p: int):
    """dft_q's butterfly network (ntt_kernels_impl.hpp) on residues: returns the slots."""
    x = [v % p for v in x]

    def bf(i, j, w=1):
        a, b = x[i], x[j]
        x[i], x[j] = (a + b) % p, (a - b) * w % p

    if Q == 2:
        bf(0, 1)
    elif Q == 4:
        bf(0, 2); bf(1, 3, w8[1]); bf(0, 1); bf(2, 3)
    else:
        assert Q == 8
        bf(0, 4); bf(1, 5, w8[0]); bf(2, 6, w8[1]); bf(3, 7, w8[2])
        bf(0, 2); bf(1, 3, w8[1]); bf(4, 6); bf(5, 7, w8[1])
        bf(0, 1); bf(2, 3); bf(4, 5); bf(6, 7)
    return x


def dft_direct(x, Q: int, w8, p: int):
    """X_k = sum_d x_d w_Q^(d k), natural order."""
    wq = pow(w8[0], 8 // Q, p)
    return [sum(v * pow(wq, d * k, p) for d, v in enumerate(x)) % p for k in range(Q)]
