"""Goldilocks (field 3, p = 2^64 - 2^32 + 1, 8-byte elements) at the C ABI and in the Python layer,
without a device: which limb counts and flags the constructors accept, the field table, and the
one-limb host helpers on values >= 2^63."""
import ctypes as C

import numpy as np
import pytest

P = 0xFFFFFFFF00000001


def _lib():
    from ntt_amd import lib as L
    return L, L.load()


def _create(so, L, limbs, flags=0, log_n=10):
    h = C.c_void_p()
    st = so.ntt_plan_create_ex(C.byref(h), L.NTT_FIELD_GOLDILOCKS, log_n, limbs, 0, flags)
    if st == 0:
        so.ntt_plan_destroy(h)
    return st


def test_field_id_is_accepted_with_one_limb():
    """Not NTT_ERR_ARG: the plan is made (a device is present) or the call gets as far as the device
    query (NTT_ERR_NODEV / NTT_ERR_HIP without one)."""
    import torch
    L, so = _lib()
    assert L.NTT_FIELD_GOLDILOCKS == 3
    h = C.c_void_p()
    st = so.ntt_plan_create(C.byref(h), 3, 10, 1, 0)
    if torch.cuda.is_available():
        assert st == 0
        so.ntt_plan_destroy(h)
    else:
        assert st in (-5, -2)


@pytest.mark.parametrize("limbs", [4, 6, 2, 0])
def test_other_limb_counts_are_refused(limbs):
    L, so = _lib()
    assert _create(so, L, limbs) == -1


def test_unsupported_flags_are_refused_before_any_device_query():
    L, so = _lib()
    rivals = [L.NTT_PLAN_STOCKHAM, L.NTT_PLAN_GZKP, L.NTT_PLAN_NAIVE, L.NTT_PLAN_NO_SWAP, L.NTT_PLAN_BELLPERSON,
              L.NTT_PLAN_IMPROVED_V1, L.NTT_PLAN_IMPROVED_V2, L.NTT_PLAN_IMPROVED_V3, L.NTT_PLAN_IMPROVED_V4]
    for flag in [L.NTT_PLAN_IN_PLACE, L.NTT_PLAN_MONTGOMERY_IO] + rivals:
        assert _create(so, L, 1, flag) == -1, flag
    # the same through the custom constructor (the modulus selects the engine, not the field id)
    h = C.c_void_p()
    p, g = (C.c_uint64 * 1)(P), (C.c_uint64 * 1)(7)
    for flag in (L.NTT_PLAN_IN_PLACE, L.NTT_PLAN_MONTGOMERY_IO, L.NTT_PLAN_STOCKHAM):
        assert so.ntt_plan_create_custom_ex(C.byref(h), p, g, 1, 10, 0, flag) == -1, flag


def test_field_table():
    from ntt_amd import fields
    name, p, g = fields.FIELDS[3]
    assert (p, g) == (P, 7) and p == 2 ** 64 - 2 ** 32 + 1 == fields.GOLDILOCKS
    assert fields.field_params(3) == (P, 7)
    assert fields.two_adicity(p) == 32
    # 7 generates the whole group: 7^((p-1)/q) != 1 for every prime q | p - 1 = 2^32 * 3 * 5 * 17 * 257 * 65537
    for q in (2, 3, 5, 17, 257, 65537):
        assert (p - 1) % q == 0 and pow(7, (p - 1) // q, p) != 1


def test_one_limb_host_helpers_keep_values_above_2_63():
    from ntt_amd.ntt import host_array, host_ints
    vals = [0, 1, P - 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, 469762048]
    a = host_array(vals, 1)
    assert a.dtype == np.int64 and a.shape == (len(vals),)
    assert [int(v) for v in a.view(np.uint64)] == vals
    assert host_ints(a) == vals
    # the multi-limb layout is unchanged
    b = host_array([P - 1, (1 << 200) + 5], 4)
    assert b.shape == (2, 4) and host_ints(b) == [P - 1, (1 << 200) + 5]
