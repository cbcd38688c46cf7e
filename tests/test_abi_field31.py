"""BabyBear (field 4, p = 2^31 - 2^27 + 1) and KoalaBear (field 5, p = 2^31 - 2^24 + 1) on 4-byte
elements, and the NTT_PLAN_ELEM32 flag, at the C ABI and in the Python layer, without a device: which
limb counts and flags the constructors accept, the field table, and the 4-byte host helpers."""
import ctypes as C

import numpy as np
import pytest

BABYBEAR = 2013265921
KOALABEAR = 2130706433
GOLDILOCKS = 0xFFFFFFFF00000001
FIELD31 = [(4, BABYBEAR, 31, 27), (5, KOALABEAR, 3, 24)]


def _lib():
    from ntt_amd import lib as L
    return L, L.load()


def _create(so, field_id, limbs, flags=0, log_n=10):
    h = C.c_void_p()
    st = so.ntt_plan_create_ex(C.byref(h), field_id, log_n, limbs, 0, flags)
    if st == 0:
        so.ntt_plan_destroy(h)
    return st


def _create_custom(so, p, g, limbs, flags, log_n=10):
    h = C.c_void_p()
    pa = (C.c_uint64 * max(limbs, 1))(p & (2 ** 64 - 1), *([0] * (max(limbs, 1) - 1)))
    ga = (C.c_uint64 * max(limbs, 1))(g, *([0] * (max(limbs, 1) - 1)))
    st = so.ntt_plan_create_custom_ex(C.byref(h), pa, ga, limbs, log_n, 0, flags)
    if st == 0:
        so.ntt_plan_destroy(h)
    return st


def _rivals(L):
    return [L.NTT_PLAN_STOCKHAM, L.NTT_PLAN_GZKP, L.NTT_PLAN_NAIVE, L.NTT_PLAN_NO_SWAP, L.NTT_PLAN_BELLPERSON,
            L.NTT_PLAN_IMPROVED_V1, L.NTT_PLAN_IMPROVED_V2, L.NTT_PLAN_IMPROVED_V3, L.NTT_PLAN_IMPROVED_V4]


def test_constants():
    L, _ = _lib()
    assert (L.NTT_FIELD_BABYBEAR, L.NTT_FIELD_KOALABEAR, L.NTT_PLAN_ELEM32) == (4, 5, 8192)


@pytest.mark.parametrize("field_id", [4, 5])
@pytest.mark.parametrize("flags", [0, 8192])
def test_field_ids_are_accepted_with_one_limb(field_id, flags):
    """Not NTT_ERR_ARG: the plan is made (a device is present) or the call gets as far as the device
    query (NTT_ERR_NODEV / NTT_ERR_HIP without one).  NTT_PLAN_ELEM32 is accepted and implied."""
    import torch
    _, so = _lib()
    st = _create(so, field_id, 1, flags)
    if torch.cuda.is_available():
        assert st == 0
    else:
        assert st in (-5, -2)


@pytest.mark.parametrize("field_id", [4, 5])
@pytest.mark.parametrize("limbs", [0, 2, 4, 6])
def test_other_limb_counts_are_refused(field_id, limbs):
    _, so = _lib()
    assert _create(so, field_id, limbs) == -1


def test_unsupported_flags_are_refused_before_any_device_query():
    L, so = _lib()
    for flag in [L.NTT_PLAN_IN_PLACE] + _rivals(L):
        for field_id, p, g, _ in FIELD31:
            assert _create(so, field_id, 1, flag) == -1, (field_id, flag)
            assert _create(so, field_id, 1, flag | L.NTT_PLAN_ELEM32) == -1, (field_id, flag)
            # the same through the custom constructor
            assert _create_custom(so, p, g, 1, flag | L.NTT_PLAN_ELEM32) == -1, (p, flag)


@pytest.mark.parametrize("field_id,limbs", [(0, 1), (0, 4), (1, 4), (1, 6), (2, 4), (2, 6), (3, 1)])
def test_elem32_on_the_other_fields_is_refused(field_id, limbs):
    L, so = _lib()
    assert _create(so, field_id, limbs, L.NTT_PLAN_ELEM32) == -1


@pytest.mark.parametrize("limbs", [4, 6, 2, 0])
def test_elem32_with_other_limb_counts_is_refused(limbs):
    L, so = _lib()
    assert _create_custom(so, BABYBEAR, 31, limbs, L.NTT_PLAN_ELEM32) == -1


def test_elem32_with_a_modulus_of_32_bits_or_more_is_a_field_error():
    L, so = _lib()
    assert _create_custom(so, GOLDILOCKS, 7, 1, L.NTT_PLAN_ELEM32) == -4
    assert _create_custom(so, 4293918721, 19, 1, L.NTT_PLAN_ELEM32) == -4  # 32 bits
    assert _create_custom(so, 1 << 31, 3, 1, L.NTT_PLAN_ELEM32) == -4


@pytest.mark.parametrize("field_id,p,g,adicity", FIELD31)
def test_field_table(field_id, p, g, adicity):
    from ntt_amd import fields
    name, fp, fg = fields.FIELDS[field_id]
    assert (fp, fg) == (p, g) and fields.field_params(field_id) == (p, g)
    assert name == {4: "BABYBEAR", 5: "KOALABEAR"}[field_id] and getattr(fields, name) == p
    assert p == 2 ** 31 - 2 ** adicity + 1 and fields.two_adicity(p) == adicity
    # g generates the whole group: g^((p-1)/q) != 1 for every prime q | p - 1
    qs, m, q = [], p - 1, 2
    while q * q <= m:
        if m % q == 0:
            qs.append(q)
            while m % q == 0:
                m //= q
        q += 1
    if m > 1:
        qs.append(m)
    assert qs == {4: [2, 3, 5], 5: [2, 127]}[field_id]
    for q in qs:
        assert pow(g, (p - 1) // q, p) != 1


def test_four_byte_host_helpers_round_trip():
    from ntt_amd.ntt import host_array, host_ints
    for p in (BABYBEAR, KOALABEAR):
        vals = [0, 1, 2, 1 << 24, 1 << 27, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (p - 1) // 2, (p + 1) // 2, p - 2,
                p - 1, p, (1 << 31), (1 << 32) - 1]
        a = host_array(vals, 1, elem32=True)
        assert a.dtype == np.int32 and a.shape == (len(vals),)
        assert [int(v) for v in a.view(np.uint32)] == vals
        assert host_ints(a) == vals
        assert host_ints(a.view(np.uint32)) == vals
    with pytest.raises(ValueError):
        host_array([1], 4, elem32=True)


def test_eight_byte_host_helpers_are_unchanged():
    from ntt_amd.ntt import host_array, host_ints
    vals = [0, 1, BABYBEAR - 1, 1 << 63, (1 << 63) + 1, GOLDILOCKS - 1]
    a = host_array(vals, 1)
    assert a.dtype == np.int64 and a.shape == (len(vals),) and host_ints(a) == vals
    b = host_array([BABYBEAR - 1, (1 << 200) + 5], 4)
    assert b.dtype == np.int64 and b.shape == (2, 4) and host_ints(b) == [BABYBEAR - 1, (1 << 200) + 5]
