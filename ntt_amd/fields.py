"""Field constants (product side).  Kept in sync with ntt_plan.cpp's kFields table."""
from __future__ import annotations

P469762049 = 469762049  # 7 * 2^26 + 1, generator 3 (reference GZKP-NTT.cu:7-8)
BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BLS12_381_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
GOLDILOCKS = 0xFFFFFFFF00000001  # 2^64 - 2^32 + 1, generator 7, two-adicity 32 (8-byte elements, 1 limb)
BABYBEAR = 0x78000001  # 2^31 - 2^27 + 1, generator 31, two-adicity 27 (4-byte elements, 1 limb)
KOALABEAR = 0x7F000001  # 2^31 - 2^24 + 1, generator 3, two-adicity 24 (4-byte elements, 1 limb)

FIELDS = {
    0: ("P469762049", P469762049, 3),
    1: ("BN254_FR", BN254_FR, 5),
    2: ("BLS12_381_FR", BLS12_381_FR, 7),
    3: ("GOLDILOCKS", GOLDILOCKS, 7),
    4: ("BABYBEAR", BABYBEAR, 31),
    5: ("KOALABEAR", KOALABEAR, 3),
}

# The usual binomial extensions F_p[X]/(X^d - W) of the fields a STARK prover folds over, field id -> (d, W):
# Goldilocks' quadratic and BabyBear's and KoalaBear's quartic extension (each W is a non-residue);
# NTTPlan.fri_fold takes them as ext_degree and ext_w.
EXTENSIONS = {3: (2, 7), 4: (4, 11), 5: (4, 3)}

# The usual Poseidon2 shapes of those fields, field id -> (t, S-box degree, rounds_f, rounds_p): plain numbers for
# NTTPlan.set_poseidon2, which takes the round constants and the diagonal from the caller (none are shipped; they
# must be the verifier's).
POSEIDON2_SHAPES = {3: (8, 7, 8, 22), 4: (16, 7, 8, 13), 5: (16, 3, 8, 20)}


def field_params(field_id: int):
    name, p, g = FIELDS[field_id]
    return p, g


def two_adicity(p: int) -> int:
    v, s = p - 1, 0
    while v % 2 == 0:
        v //= 2
        s += 1
    return s
