"""The wave-uniform sub-stage of the 256-bit passes reads its twiddles with scalar loads
(Eng29::tload_u -> mul_u).  What can go wrong there is the index arithmetic of the scalar
address, the rotation of the wave's class by the tile index, and the bounds the SGPR product accepts,
so the cases are the smallest plans that put every shape of that sub-stage through several tiles:

* single-tile transforms at 2^9 and 2^10 (the uniform sub-stage at sigma = 2 and sigma = 4);
* 2^11 (6 + 5), 2^13 (7 + 6), 2^14 (7 + 7), 2^15 (8 + 7), 2^16 (8 + 8: the flagship's first-column and
  final kernels over 64 tiles, so every rotation mod 4 occurs and every wave takes every class,
  0 included) and 2^18 (6 + 6 + 6: a middle column pass from scratch to scratch with the Shoup-pair
  outer table);
* the planner never puts radix 2^5 first (the near-equal split gives the larger radices to the first
  passes), so 2^11 also runs as 5 + 6 through NTT_SCHEDULE: the one way to a radix-2^5 column pass.

BN254 Fr and BLS12-381 Fr at 4 limbs, forward and inverse, on the SplitMix64 vector, all p - 1,
alternating 0 / p - 1 and x_j = j (also against the closed form).  Everything is bit-exact against the C
oracle.  One case per radix also runs through the checked build, whose status word must stay 0 (the
lazy-bound flag 0x400 among it).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ntt_ref as R
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

L = 4
FIELDS = [1, 2]  # BN254 Fr, BLS12-381 Fr
# (log_n, NTT_SCHEDULE or None, the radices expected)
PLANS = [(9, None, [9]), (10, None, [10]), (11, None, [6, 5]), (11, "5,6", [5, 6]), (13, None, [7, 6]),
         (14, None, [7, 7]), (15, None, [8, 7]), (16, None, [8, 8]), (18, None, [6, 6, 6])]
IDS = [f"2^{lg}" + (f"[{s}]" if s else "") for lg, s, _ in PLANS]

_inputs = {}  # (fid, log_n) -> {name: (x, forward, inverse)}, computed once and left unchanged


def _vectors(fid, log_n):
    key = (fid, log_n)
    if key not in _inputs:
        p, g = R.FIELDS[fid]
        n = 1 << log_n
        top = OC.ints_to_limbs([p - 1], L)[0]
        xs = {"splitmix": OC.random_limbs(fid, n, 11 + log_n, L), "p-1": np.tile(top, (n, 1)),
              "0/p-1": np.tile(top, (n, 1)), "iota": OC.ints_to_limbs(list(range(n)), L)}
        xs["0/p-1"][0::2] = 0
        _inputs[key] = {k: (x, OC.ntt_mp(x, p, g, False), OC.ntt_mp(x, p, g, True)) for k, x in xs.items()}
        for v in _inputs[key].values():
            for a in v:
                a.setflags(write=False)
    return _inputs[key]


def _plan(fid, log_n, sched, monkeypatch):
    from ntt_amd.ntt import NTTPlan
    if sched:
        monkeypatch.setenv("NTT_SCHEDULE", sched)
    else:
        monkeypatch.delenv("NTT_SCHEDULE", raising=False)
    return NTTPlan(field_id=fid, log_n=log_n, limbs64=L, device=0)


def _run(pl, host, inverse):
    t = torch.from_numpy(host.copy().view(np.int64)).to("cuda:0").reshape(host.shape)  # the shared input stays as it is
    (pl.inverse if inverse else pl.forward)(t)
    assert pl.device_status() == 0, hex(pl.device_status())
    return t.cpu().numpy().view(np.uint64).reshape(host.shape)


def test_the_plans_cover_every_uniform_substage_shape(monkeypatch):
    """Column passes of radix 2^5..2^8 and final passes of radix 2^5..2^8 each occur in the set, and the
    single-tile transforms are single passes."""
    col, fin = set(), set()
    for log_n, sched, want in PLANS:
        passes = list(_plan(1, log_n, sched, monkeypatch).passes)
        assert passes == want, (log_n, sched, passes)
        if len(passes) > 1:
            col.update(passes[:-1])
            fin.add(passes[-1])
    assert col == {5, 6, 7, 8} and fin == {5, 6, 7, 8}, (col, fin)


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("log_n,sched,want", PLANS, ids=IDS)
def test_forward_and_inverse_match_the_oracle(fid, log_n, sched, want, monkeypatch):
    pl = _plan(fid, log_n, sched, monkeypatch)
    assert list(pl.passes) == want
    for name, (x, fwd, inv) in _vectors(fid, log_n).items():
        assert np.array_equal(_run(pl, x, False), fwd), (fid, log_n, sched, name, "forward")
        assert np.array_equal(_run(pl, x, True), inv), (fid, log_n, sched, name, "inverse")


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("log_n,sched,want", PLANS, ids=IDS)
def test_iota_matches_the_closed_form(fid, log_n, sched, want, monkeypatch):
    """x_j = j against the closed-form KAT (no oracle involved)."""
    p, g = R.FIELDS[fid]
    n = 1 << log_n
    pl = _plan(fid, log_n, sched, monkeypatch)
    got = _run(pl, _vectors(fid, log_n)["iota"][0], False)
    ks = [0, 1, 2, 3, n // 2 - 1, n // 2, n - 2, n - 1] + [int(k) for k in np.random.default_rng(log_n).integers(0, n, 24)]
    assert OC.limbs_to_ints(got[ks]) == [R.kat_xj(n, p, g, k) for k in ks], (fid, log_n, sched)


CHILD = r'''
import os, sys
sys.path.insert(0, ROOT)
import numpy as np, torch
from ntt_amd import lib as L
from ntt_amd.ntt import NTTPlan
from oracle import ntt_ref as R
from oracle import oracle_c as OC
L.load()
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
for fid in (1, 2):
    p, g = R.FIELDS[fid]
    for lg, sched in PLANS:
        if sched:
            os.environ["NTT_SCHEDULE"] = sched
        else:
            os.environ.pop("NTT_SCHEDULE", None)
        n = 1 << lg
        pl = NTTPlan(fid, lg, 4)
        top = OC.ints_to_limbs([p - 1], 4)[0]
        alt = np.tile(top, (n, 1))
        alt[0::2] = 0
        for x in (OC.random_limbs(fid, n, 5, 4), np.tile(top, (n, 1)), alt):
            for inverse in (False, True):
                t = torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to("cuda:0").reshape(x.shape)
                (pl.inverse if inverse else pl.forward)(t)
                st = pl.device_status()
                assert st == 0, (fid, lg, sched, inverse, hex(st))
                if lg <= 14:
                    got = t.cpu().numpy().view(np.uint64).reshape(x.shape)
                    assert np.array_equal(got, OC.ntt_mp(x, p, g, inverse)), (fid, lg, sched, inverse)
print("CHECKED-OK")
'''


@pytest.mark.skipif(not os.path.exists(DEBUG_LIB), reason="libntt_debug.so not built (python -m ntt_amd.build --debug)")
def test_checked_build_raises_no_flag():
    """Every plan above through the checked build (in-kernel index, canonical and lazy-bound checks): the
    status word stays 0, so the bounds hold at the input of the SGPR product too."""
    plans = [(lg, s) for lg, s, _ in PLANS]
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    env.pop("NTT_SCHEDULE", None)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nPLANS = {plans!r}\n" + CHILD], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "CHECKED-OK" in r.stdout
