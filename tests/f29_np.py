"""Bulk transport between Python ints and uint32 limb / word arrays for the field29 tests: the
arithmetic stays in plain ints (tests/f29_ref.py); numpy only moves bits."""
import random

import numpy as np

MASK = np.uint64((1 << 29) - 1)


def _nw(bits: int) -> int:
    return (bits + 63) // 64 + 1  # one spare word: a field may straddle the last boundary


def ints_to_fields(vals, n_fields: int, width: int) -> np.ndarray:
    """Non-negative ints < 2^(n_fields * width) -> (n, n_fields) uint32 fields of `width` bits."""
    nw = _nw(n_fields * width)
    buf = b"".join([v.to_bytes(8 * nw, "little") for v in vals])
    w = np.frombuffer(buf, dtype="<u8").reshape(len(vals), nw)
    out = np.empty((len(vals), n_fields), dtype=np.uint32)
    m = np.uint64((1 << width) - 1)
    for i in range(n_fields):
        k, s = divmod(width * i, 64)
        v = w[:, k] >> np.uint64(s)
        if s + width > 64:
            v = v | (w[:, k + 1] << np.uint64(64 - s))
        out[:, i] = (v & m).astype(np.uint32)
    return out


def fields_to_ints(a: np.ndarray, width: int):
    """(n, n_fields) fields, each < 2^width -> list of ints."""
    a = np.ascontiguousarray(a).astype(np.uint64)
    n, nf = a.shape
    assert not (a >> np.uint64(width)).any(), "field wider than its slot"
    nw = _nw(nf * width)
    w = np.zeros((n, nw), dtype=np.uint64)
    for i in range(nf):
        k, s = divmod(width * i, 64)
        w[:, k] |= a[:, i] << np.uint64(s)
        if s + width > 64:
            w[:, k + 1] |= a[:, i] >> np.uint64(64 - s)
    buf, nb = memoryview(w.tobytes()), 8 * nw
    return [int.from_bytes(buf[j * nb:(j + 1) * nb], "little") for j in range(n)]


def ints_to_limbs(vals, L):
    return ints_to_fields(vals, L, 29)


def ints_to_words(vals, W32):
    return ints_to_fields(vals, W32, 32)


def words_to_ints(a):
    return fields_to_ints(a, 32)


def limb_values(a: np.ndarray, signed=False):
    """sum_i a[:, i] 2^(29 i) for any uint32 limbs (signed: read as int32)."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    L = a.shape[1]
    x = a.view(np.int32).astype(np.int64) if signed else a.astype(np.int64)
    lo = (x & np.int64((1 << 29) - 1)).astype(np.uint64)
    hi = x >> np.int64(29)  # in [-4, 7]
    if not hi.any():
        return fields_to_ints(lo, 29)
    ones4 = 4 * sum(1 << (29 * i) for i in range(L))
    vlo, vhi = fields_to_ints(lo, 29), fields_to_ints((hi + 4).astype(np.uint64), 29)
    return [u + ((v - ones4) << 29) for u, v in zip(vlo, vhi)]


def normalised(a: np.ndarray, upto=None) -> bool:
    a = a if upto is None else a[:, :upto]
    return not (a >> 29).any()


def rand_below(rng: random.Random, n: int, limit: int):
    """n seeded ints, uniform enough in [0, limit): 64 spare bits before the reduction."""
    nb = (limit.bit_length() + 64 + 7) // 8
    buf = memoryview(rng.randbytes(n * nb))
    return [int.from_bytes(buf[j * nb:(j + 1) * nb], "little") % limit for j in range(n)]


def push_down(a: np.ndarray, units) -> np.ndarray:
    """The same values with up to `units[:, i]` (0..3) units of 2^29 moved from limb i + 1 down into
    limb i: limbs grow to at most 2^31 - 1 for normalised input, the value does not change."""
    a = a.astype(np.uint32).copy()
    units = np.broadcast_to(np.asarray(units, dtype=np.uint32), (a.shape[0], a.shape[1] - 1))
    for i in range(a.shape[1] - 1):
        u = np.minimum(units[:, i], a[:, i + 1])
        a[:, i + 1] -= u
        a[:, i] += u << np.uint32(29)
    return a
