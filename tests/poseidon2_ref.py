"""The Poseidon2 sponge, compression and Merkle tree of ntt_merkle_commit, restated in plain Python integers from the
definitions in include/ntt.h (never from the kernels): the yardstick of the Merkle tests.

Width t (16 on 4-byte fields, 8 on Goldilocks), D = t / 2 the rate and the digest length.  All values are
canonical integers in [0, p).
"""
from __future__ import annotations

import random
from typing import List, Sequence

M4 = ((2, 3, 1, 1), (1, 2, 3, 1), (1, 1, 2, 3), (3, 1, 1, 2))


class Params:
    """One parameter set: the modulus, the width, the S-box degree, the round counts and the constants."""

    def __init__(self, p: int, t: int, alpha: int, rounds_f: int, rounds_p: int, ext_rc: Sequence[Sequence[int]],
                 int_rc: Sequence[int], int_diag: Sequence[int]):
        assert t % 4 == 0 and len(ext_rc) == rounds_f and all(len(r) == t for r in ext_rc)
        assert len(int_rc) == rounds_p and len(int_diag) == t
        self.p, self.t, self.d, self.alpha, self.rounds_f, self.rounds_p = p, t, t // 2, alpha, rounds_f, rounds_p
        self.ext_rc = [list(r) for r in ext_rc]
        self.int_rc = list(int_rc)
        self.int_diag = list(int_diag)

    def flat_ext(self) -> List[int]:
        return [v for r in self.ext_rc for v in r]

    def as_dict(self) -> dict:
        return {"p": self.p, "t": self.t, "alpha": self.alpha, "rounds_f": self.rounds_f, "rounds_p": self.rounds_p,
                "ext_rc": self.ext_rc, "int_rc": self.int_rc, "int_diag": self.int_diag}

    @classmethod
    def from_dict(cls, d: dict) -> "Params":
        return cls(d["p"], d["t"], d["alpha"], d["rounds_f"], d["rounds_p"], d["ext_rc"], d["int_rc"], d["int_diag"])


def seeded_params(p: int, t: int, alpha: int, rounds_f: int, rounds_p: int, seed: int) -> Params:
    """Random canonical constants: test parameters, not any prover's."""
    rng = random.Random(seed)
    ext = [[rng.randrange(p) for _ in range(t)] for _ in range(rounds_f)]
    irc = [rng.randrange(p) for _ in range(rounds_p)]
    diag = [rng.randrange(p) for _ in range(t)]
    return Params(p, t, alpha, rounds_f, rounds_p, ext, irc, diag)


def m_ext(s: List[int], p: int) -> List[int]:
    t = len(s)
    y = [0] * t
    for g in range(0, t, 4):
        for i in range(4):
            y[g + i] = sum(M4[i][j] * s[g + j] for j in range(4)) % p
    sums = [sum(y[g + j] for g in range(0, t, 4)) % p for j in range(4)]
    return [(y[i] + sums[i % 4]) % p for i in range(t)]


def m_ext_matrix(t: int) -> List[List[int]]:
    """circ(2 M4, M4, .., M4) written out."""
    m = [[0] * t for _ in range(t)]
    for bi in range(t // 4):
        for bj in range(t // 4):
            f = 2 if bi == bj else 1
            for i in range(4):
                for j in range(4):
                    m[4 * bi + i][4 * bj + j] = f * M4[i][j]
    return m


def permute(state: Sequence[int], P: Params) -> List[int]:
    p, a = P.p, P.alpha
    s = m_ext(list(state), p)

    def external(s, r):
        s = [pow((s[i] + P.ext_rc[r][i]) % p, a, p) for i in range(P.t)]
        return m_ext(s, p)

    for r in range(P.rounds_f // 2):
        s = external(s, r)
    for r in range(P.rounds_p):
        s[0] = pow((s[0] + P.int_rc[r]) % p, a, p)
        sigma = sum(s) % p
        s = [(P.int_diag[i] * s[i] + sigma) % p for i in range(P.t)]
    for r in range(P.rounds_f // 2, P.rounds_f):
        s = external(s, r)
    return s


def hash_row(row: Sequence[int], P: Params) -> List[int]:
    s = [0] * P.t
    for c in range(0, len(row), P.d):
        chunk = list(row[c:c + P.d])
        s[:len(chunk)] = chunk
        s = permute(s, P)
    return s[:P.d]


def compress(left: Sequence[int], right: Sequence[int], P: Params) -> List[int]:
    return permute(list(left) + list(right), P)[:P.d]


def tree(rows: Sequence[Sequence[int]], P: Params) -> List[List[int]]:
    """The 2N - 1 nodes: layer 0 (the leaf digests in row order) first, the root last."""
    n = len(rows)
    assert n & (n - 1) == 0 and n >= 1
    layer = [hash_row(r, P) for r in rows]
    nodes = list(layer)
    while len(layer) > 1:
        layer = [compress(layer[2 * i], layer[2 * i + 1], P) for i in range(len(layer) // 2)]
        nodes += layer
    return nodes


def layer_start(log_rows: int, layer: int) -> int:
    return (2 << log_rows) - (2 << (log_rows - layer))


def root_from_path(row: Sequence[int], index: int, path: Sequence[Sequence[int]], P: Params) -> List[int]:
    """Fold a query's path upward from the leaf hash of its row."""
    node = hash_row(row, P)
    for l, sib in enumerate(path):
        node = compress(sib, node, P) if (index >> l) & 1 else compress(node, sib, P)
    return node


# ------------------------------------------------------------------------------------------------ many rows at once
# The same definitions over numpy arrays, one state per row, for the GPU tests' shapes: uint64 arithmetic with
# `%` below 2^32 (a product stays below 2^64); on Goldilocks the 128-bit product on 32-bit halves, reduced with
# 2^64 = 2^32 - 1 and 2^96 = -1 (mod p).  tests/test_poseidon2_host.py holds this path to the integer one above.
import numpy as np

_GL = 0xFFFFFFFF00000001
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


class _Small:
    def __init__(self, p):
        assert p < 1 << 32
        self.p = np.uint64(p)

    def add(self, a, b):
        return (a + b) % self.p

    def mul(self, a, b):
        return (a * b) % self.p


class _Goldilocks:
    p = np.uint64(_GL)

    def add(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
        s = a + b
        return np.where((s < a) | (s >= self.p), s - self.p, s)

    def mul(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
        a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
        p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
        mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
        lo = (p00 & _M32) | ((mid & _M32) << _S32)
        hi = p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)
        hh, hl = hi >> _S32, hi & _M32
        t0 = lo - hh
        t0 = np.where(lo < hh, t0 - _M32, t0)
        t1 = hl * _M32
        t2 = t0 + t1
        t2 = np.where(t2 < t0, t2 + _M32, t2)
        return np.where(t2 >= self.p, t2 - self.p, t2)


def _field(p):
    return _Goldilocks() if p == _GL else _Small(p)


def _pow_many(F, x, a):
    x2 = F.mul(x, x)
    if a == 3:
        return F.mul(x2, x)
    if a == 5:
        return F.mul(F.mul(x2, x2), x)
    assert a == 7
    return F.mul(F.mul(x2, x), F.mul(x2, x2))


def _m_ext_many(F, s):
    t = s.shape[1]
    y = np.empty_like(s)
    for g in range(0, t, 4):
        for i in range(4):
            acc = None
            for j in range(4):
                term = s[:, g + j]
                for _ in range(M4[i][j] - 1):
                    term = F.add(term, s[:, g + j])
                acc = term if acc is None else F.add(acc, term)
            y[:, g + i] = acc
    out = np.empty_like(s)
    for j in range(4):
        tot = y[:, j]
        for g in range(4, t, 4):
            tot = F.add(tot, y[:, g + j])
        for g in range(0, t, 4):
            out[:, g + j] = F.add(y[:, g + j], tot)
    return out


def permute_many(states, P: Params):
    """states = [n][t] uint64 canonical -> the permuted states."""
    F = _field(P.p)
    s = _m_ext_many(F, np.array(states, dtype=np.uint64))

    def external(s, r):
        rc = np.array(P.ext_rc[r], dtype=np.uint64)[None, :]
        return _m_ext_many(F, _pow_many(F, F.add(s, rc), P.alpha))

    for r in range(P.rounds_f // 2):
        s = external(s, r)
    diag = np.array(P.int_diag, dtype=np.uint64)[None, :]
    for r in range(P.rounds_p):
        s[:, 0] = _pow_many(F, F.add(s[:, 0], np.uint64(P.int_rc[r])), P.alpha)
        sigma = s[:, 0]
        for i in range(1, P.t):
            sigma = F.add(sigma, s[:, i])
        s = F.add(F.mul(s, diag), sigma[:, None])
    for r in range(P.rounds_f // 2, P.rounds_f):
        s = external(s, r)
    return s


def hash_rows_many(mat, P: Params):
    """mat = [n][w] uint64 -> the n leaf digests [n][D]."""
    mat = np.asarray(mat, dtype=np.uint64)
    s = np.zeros((mat.shape[0], P.t), dtype=np.uint64)
    for c in range(0, mat.shape[1], P.d):
        chunk = mat[:, c:c + P.d]
        s[:, :chunk.shape[1]] = chunk
        s = permute_many(s, P)
    return s[:, :P.d].copy()


def compress_many(nodes, P: Params):
    """nodes = [2m][D] -> the m parents."""
    return permute_many(np.asarray(nodes, dtype=np.uint64).reshape(-1, P.t), P)[:, :P.d].copy()


def tree_many(mat, P: Params):
    """The [2N - 1][D] tree over the rows of mat, as `tree` lays it out."""
    layer = hash_rows_many(mat, P)
    layers = [layer]
    while layer.shape[0] > 1:
        layer = compress_many(layer, P)
        layers.append(layer)
    return np.concatenate(layers, axis=0)


# ------------------------------------------------------------------------------------------------ golden vectors
GOLDEN_FIELDS = (  # name, p, t, alpha, rounds_f, rounds_p, seed
    ("babybear", 0x78000001, 16, 7, 8, 13, 101),
    ("koalabear", 0x7F000001, 16, 3, 8, 20, 102),
    ("goldilocks", _GL, 8, 7, 8, 22, 103),
    ("p31", 1811939329, 16, 5, 8, 13, 104),
    ("babybear-degenerate", 0x78000001, 16, 7, 2, 1, 105),
    ("goldilocks-degenerate", _GL, 8, 7, 2, 1, 106),
)


def golden() -> dict:
    """tests/golden/poseidon2_vectors.json: per field the seeded parameters, a few states, rows and a 4-leaf tree."""
    out = {}
    for name, p, t, alpha, rf, rp, seed in GOLDEN_FIELDS:
        P = seeded_params(p, t, alpha, rf, rp, seed)
        rng = random.Random(seed + 1000)
        states = [[0] * t, [p - 1] * t] + [[rng.randrange(p) for _ in range(t)] for _ in range(2)]
        rows = [[rng.randrange(p) for _ in range(w)] for w in (1, P.d - 1, P.d + 1, 2 * P.d + 3)]
        leaves = [[rng.randrange(p) for _ in range(P.d + 2)] for _ in range(4)]
        out[name] = {
            "params": P.as_dict(),
            "states": [{"in": s, "out": permute(s, P)} for s in states],
            "rows": [{"row": r, "digest": hash_row(r, P)} for r in rows],
            "tree": {"rows": leaves, "nodes": tree(leaves, P)},
        }
    return out


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon2_vectors.json")
    with open(path, "w") as f:
        json.dump(golden(), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)
