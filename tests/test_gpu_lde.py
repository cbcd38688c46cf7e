"""ntt_lde_batch (NTTPlan.lde_batch) on the GPU: `batch` polynomials of n = N >> log_blowup
coefficients to their N evaluations on the coset shift * <w_N>, bit-exact against the oracle
(oracle/ntt_ref.py coset_ntt on the zero-padded vector at the small sizes, oracle_c.ntt_mp on the
host-scaled, zero-padded limbs above them), on every engine: P469762049, BN254, BLS12-381 in 4 and 6
limbs, Goldilocks, BabyBear and KoalaBear.

Every case first runs an unrelated forward of the same batch on the plan, so that the plan's scratch
holds another call's data, and fills `out` with a nonzero pattern: a tile whose inputs are all padding
must still store its zeros.  The input is compared with a copy after every call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

# (field id, 64-bit limbs) -> log2 of the engine's tile (engines.hpp TILE_LOG; pinned by
# test_tile_constants_match_the_library): the largest single-pass size, one below the smallest two-pass one
ENGINES = {(0, 1): 13, (1, 4): 10, (2, 4): 10, (2, 6): 10, (3, 1): 12, (4, 1): 13, (5, 1): 13}
THREE_PASS = {(1, 4): 17, (3, 1): 17, (4, 1): 19}  # the smallest 3-pass sizes (schedule())
IDS = [f"f{f}L{l}" for f, l in ENGINES]

_PLANS = {}


def _params(fid):
    from ntt_amd.fields import field_params
    return field_params(fid)


def _plan(fid, L, log_n, **kw):
    from ntt_amd.ntt import NTTPlan
    key = (fid, L, log_n, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = NTTPlan(fid, log_n, L, **kw)
    return _PLANS[key]


def _custom_plan(p, g, L, log_n):
    from ntt_amd.ntt import NTTPlan
    key = ("custom", p, g, L, log_n)
    if key not in _PLANS:
        _PLANS[key] = NTTPlan(log_n=log_n, limbs64=L, modulus=p, generator=g)
    return _PLANS[key]


def _rand(p, count, seed):
    """Seeded values below p with the edge values 0, 1, p - 1, p - 2 in front."""
    rng = np.random.default_rng(seed)
    words = (p.bit_length() + 63) // 64
    raw = rng.integers(0, 1 << 63, size=(count, words), dtype=np.uint64)
    vals = [sum(int(w) << (63 * i) for i, w in enumerate(row)) % p for row in raw]
    edge = [0, 1, p - 1, p - 2]
    vals[:min(count, 4)] = edge[:min(count, 4)]
    return vals


def _dev(vals, pl):
    from ntt_amd.ntt import to_device
    return to_device(vals, pl.limbs64, "cuda:0", elem32=pl.elem32)


def _ints(t):
    from ntt_amd.ntt import from_device
    return from_device(t)


def _poisoned(pl, batch):
    out = pl.empty(batch)
    out.fill_(0x5A5A5A5A if pl.elem32 else 0x5A5A5A5A5A5A5A5A)
    return out


_JUNK = {}


def _dirty(pl, batch):
    """An unrelated forward of `batch` vectors: the plan's scratch (multi-pass sizes) holds its data.
    The junk vector is keyed on what determines its contents and layout, never on the plan object."""
    key = (pl.p, pl.n, pl.limbs64, pl.elem32)
    if key not in _JUNK:
        _JUNK[key] = _dev(_rand(pl.p, pl.n, 99), pl)
    junk = torch.cat([_JUNK[key]] * batch)
    pl.forward_batch(junk, batch)


def _expected(x, p, g, c, log_n, L):
    """Coset evaluations of the coefficients x (len <= N) on c <w_N>: the oracle on the padded vector."""
    from oracle import ntt_ref as R
    from oracle import oracle_c as OC
    N = 1 << log_n
    if log_n <= 5:
        return R.coset_ntt(list(x) + [0] * (N - len(x)), p, g, c)
    scaled, cj = [], 1
    for v in x:
        scaled.append(v * cj % p)
        cj = cj * c % p
    if L == 1:
        host = np.zeros((N, 1), dtype=np.uint64)
        host[:len(x), 0] = np.array(scaled, dtype=np.uint64)
        return [int(v) for v in OC.ntt_mp(host, p, g).reshape(-1)]
    host = np.zeros((N, L), dtype=np.uint64)
    host[:len(x)] = OC.ints_to_limbs(scaled, L)
    return OC.limbs_to_ints(OC.ntt_mp(host, p, g))


def _blowups(pl):
    r1 = pl.passes[0] if pl.passes else pl.log_n
    return sorted({b for b in (0, 1, 3, r1 + 1, pl.log_n) if b <= pl.log_n})


def _run_case(pl, coeffs, log_blowup, shift, batch):
    """One call on dirtied scratch into a poisoned `out`; returns the outputs, checks d_in is unchanged."""
    n_in = pl.n >> log_blowup
    x = []
    for v in range(batch):
        x += coeffs[v][:n_in]
    t_in = _dev(x, pl)
    keep = t_in.clone()
    _dirty(pl, batch)
    out = _poisoned(pl, batch)
    pl.lde_batch(t_in, out, log_blowup, shift, batch)
    assert torch.equal(t_in, keep), "d_in was modified"
    return _ints(out)


def _check_size(fid, L, log_n, batches=(1, 3)):
    p, g = _params(fid)
    pl = _plan(fid, L, log_n)
    N = 1 << log_n
    coeffs = [_rand(p, N, 1000 * log_n + v) for v in range(max(batches))]
    exp = {}
    for lb in _blowups(pl):
        for shift in (None, g, p - 1):
            for batch in batches:
                got = _run_case(pl, coeffs, lb, shift, batch)
                for v in range(batch):
                    if (lb, shift, v) not in exp:
                        exp[lb, shift, v] = _expected(coeffs[v][:N >> lb], p, g, 1 if shift is None else shift, log_n, L)
                    assert got[v * N:(v + 1) * N] == exp[lb, shift, v], (fid, L, log_n, lb, shift, batch, v)


def test_tile_constants_match_the_library():
    for (fid, L), tl in ENGINES.items():
        assert _plan(fid, L, tl).passes == [tl], (fid, L)
        assert len(_plan(fid, L, tl + 1).passes) == 2, (fid, L)
    for (fid, L), lg in THREE_PASS.items():
        assert len(_plan(fid, L, lg).passes) == 3 and len(_plan(fid, L, lg - 1).passes) == 2, (fid, L)


@pytest.mark.parametrize("fid,L", list(ENGINES), ids=IDS)
@pytest.mark.parametrize("log_n", [1, 2, 3])
def test_lde_tiny_sizes(fid, L, log_n):
    """2 and 4 points (the naive kernel, through the staging path) and 8 points (one radix-8 tile)."""
    _check_size(fid, L, log_n)


@pytest.mark.parametrize("fid,L", list(ENGINES), ids=IDS)
def test_lde_one_full_tile(fid, L):
    _check_size(fid, L, ENGINES[fid, L])


@pytest.mark.parametrize("fid,L", list(ENGINES), ids=IDS)
def test_lde_smallest_two_pass_size(fid, L):
    """Two passes: the first column pass loads the coefficients only; with log_blowup = r_1 + 1 whole
    column groups of it have no input at all and must still overwrite the dirty scratch with zeros."""
    _check_size(fid, L, ENGINES[fid, L] + 1)


@pytest.mark.parametrize("fid,L", list(THREE_PASS), ids=[f"f{f}L{l}" for f, l in THREE_PASS])
def test_lde_smallest_three_pass_size(fid, L):
    p, g = _params(fid)
    log_n = THREE_PASS[fid, L]
    pl = _plan(fid, L, log_n)
    coeffs = [_rand(p, pl.n >> 1, 31 + fid)]
    got = _run_case(pl, coeffs, 1, g, 1)
    assert got == _expected(coeffs[0], p, g, g, log_n, L)


@pytest.mark.parametrize("fid,L", list(ENGINES), ids=IDS)
def test_lde_batch_of_short_transforms(fid, L):
    _check_size(fid, L, 5, batches=(64,))


@pytest.mark.parametrize("fid,L", list(ENGINES), ids=IDS)
def test_lde_equals_the_composed_route(fid, L):
    """Zero-fill, strided copy and ntt_forward_coset per vector give the same bits."""
    p, g = _params(fid)
    log_n = ENGINES[fid, L] + 1
    pl = _plan(fid, L, log_n)
    N, batch = pl.n, 3
    for lb in (1, 3):
        n_in = N >> lb
        coeffs = [_rand(p, n_in, 7 * lb + v) for v in range(batch)]
        got = _run_case(pl, coeffs, lb, g, batch)
        for v in range(batch):
            t = _dev(coeffs[v] + [0] * (N - n_in), pl)
            pl.forward_coset(t, g)
            assert _ints(t) == got[v * N:(v + 1) * N], (fid, L, lb, v)


@pytest.mark.parametrize("fid,L", [(1, 4), (4, 1)], ids=["bn254", "babybear"])
def test_lde_montgomery_io(fid, L):
    """Data in Montgomery form, canonical shift: LDE(x R) = LDE(x) R."""
    p, g = _params(fid)
    log_n = ENGINES[fid, L] + 1
    pm = _plan(fid, L, log_n, montgomery_io=True)
    Rm = pow(2, 8 * pm.elem_bytes, p)
    N = pm.n
    for lb, shift in ((1, g), (3, None), (pm.passes[0] + 1, p - 1)):
        coeffs = [_rand(p, N >> lb, 50 + lb + v) for v in range(2)]
        got = _run_case(pm, [[v * Rm % p for v in c] for c in coeffs], lb, shift, 2)
        for v in range(2):
            exp = _expected(coeffs[v], p, g, 1 if shift is None else shift, log_n, L)
            assert got[v * N:(v + 1) * N] == [e * Rm % p for e in exp], (fid, lb, shift, v)


def _is_prime(n):
    if n < 2 or n % 2 == 0:
        return n == 2
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _ntt_prime(bits, two_adicity=24):
    """The smallest prime k 2^v + 1 >= 2^(bits - 1) and a quadratic non-residue as its generator."""
    k = (1 << (bits - 1 - two_adicity)) + 1
    while not _is_prime(k * (1 << two_adicity) + 1):
        k += 2
    p = k * (1 << two_adicity) + 1
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return p, g


@pytest.mark.parametrize("bits,L", [(380, 6), (300, 6), (255, 4), (200, 4)])
def test_lde_custom_moduli(bits, L):
    """Custom plans: 6-limb moduli above 2^255 run the 14-limb engine, whose first pass reads inputs
    scaled by one launch over the batch n coefficients (a staging buffer of the plan) and whose 8- and
    16-point sizes take the zero-padded staging route; 4-limb moduli run the 9-limb engine with or
    without its fast reductions."""
    p, g = _ntt_prime(bits)
    for log_n in (3, 4, 10, 11, 13):
        pl = _custom_plan(p, g, L, log_n)
        coeffs = [_rand(p, pl.n, bits + v) for v in range(2)]
        for lb in sorted({1, min(pl.passes[0] + 1, log_n)}):
            for shift in (None, g, p - 1):
                got = _run_case(pl, coeffs, lb, shift, 2)
                for v in range(2):
                    exp = _expected(coeffs[v][:pl.n >> lb], p, g, 1 if shift is None else shift, log_n, L)
                    assert got[v * pl.n:(v + 1) * pl.n] == exp, (bits, log_n, lb, shift, v)


def _raw(pl, t_in, out, lb, shift_words, batch):
    sh = None if shift_words is None else (C.c_uint64 * len(shift_words))(*shift_words)
    stream = C.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
    return pl._lib.ntt_lde_batch(pl._h, None if t_in is None else C.c_void_p(t_in.data_ptr()),
                                 None if out is None else C.c_void_p(out.data_ptr()), lb, sh, batch, stream)


@pytest.mark.parametrize("fid,L", [(1, 4), (2, 6), (3, 1), (4, 1)], ids=["bn254", "bls6", "goldilocks", "babybear"])
def test_lde_refusals(fid, L):
    """Every refusal of the contract returns NTT_ERR_ARG and launches nothing: `out` keeps its pattern."""
    from ntt_amd import lib as LL
    from ntt_amd.ntt import int_to_limbs
    p, g = _params(fid)
    log_n = 6
    pl = _plan(fid, L, log_n)
    lb, batch = 2, 2
    n_in = pl.n >> lb
    t_in = _dev(_rand(p, batch * n_in, 5), pl)
    out = _poisoned(pl, batch)
    keep = out.clone()
    ok_shift = int_to_limbs(g, L)
    ERR = LL.NTT_ERR_ARG
    assert pl._lib.ntt_lde_batch(None, C.c_void_p(t_in.data_ptr()), C.c_void_p(out.data_ptr()), lb, None, batch, None) == ERR
    assert _raw(pl, None, out, lb, ok_shift, batch) == ERR
    assert _raw(pl, t_in, None, lb, ok_shift, batch) == ERR
    assert _raw(pl, t_in, out, lb, ok_shift, 0) == ERR
    assert _raw(pl, t_in, out, log_n + 1, ok_shift, 1) == ERR
    assert _raw(pl, t_in, out, lb, int_to_limbs(0, L), batch) == ERR  # zero shift
    assert _raw(pl, t_in, out, lb, int_to_limbs(p, L), batch) == ERR  # not canonical
    if L > 1 and p.bit_length() <= 64 * (L - 1):  # 6-limb layout of a 255-bit modulus: a set high limb
        assert _raw(pl, t_in, out, lb, int_to_limbs(g, L - 1) + [1], batch) == ERR
    # overlapping byte ranges: the input inside the output, at its start, its end, and straddling its end
    flat = out.view(-1)
    per = out.numel() // (batch * pl.n)  # tensor items per element
    big = torch.cat([flat, flat.clone()])  # room behind `out`'s extent
    o = big[:flat.numel()]
    for start in (0, (batch * pl.n - batch * n_in) * per, (batch * pl.n - 1) * per):
        alias = big[start:start + batch * n_in * per]
        assert _raw(pl, alias, o, lb, ok_shift, batch) == ERR, start
    # the output starting inside the input
    src = big[:batch * n_in * per]
    assert _raw(pl, src, big[(batch * n_in - 1) * per:], lb, ok_shift, batch) == ERR
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    # plan flags (in-place plans exist for fields 0-2; P469762049's has a test of its own below)
    tw = _plan(fid, L, log_n, twiddle_only=True)
    assert _raw(tw, t_in, out, lb, ok_shift, batch) == ERR
    if fid in (1, 2):
        assert _raw(_plan(fid, L, log_n, in_place=True), t_in, out, lb, ok_shift, batch) == ERR
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    with pytest.raises(LL.NTTError):
        tw.lde_batch(t_in, out, lb, g, batch)


def test_lde_in_place_plan_is_refused_on_p469762049():
    from ntt_amd import lib as LL
    pl = _plan(0, 1, 14, in_place=True)
    t_in, out = _dev(_rand(pl.p, pl.n >> 1, 3), pl), _poisoned(pl, 1)
    assert _raw(pl, t_in, out, 1, None, 1) == LL.NTT_ERR_ARG


@pytest.mark.parametrize("flags", [{"stockham": True}, {"gzkp": True}, {"single_launch": True}, {"bealto": "v3"}],
                         ids=["stockham", "gzkp", "single_launch", "bealto_v3"])
def test_lde_on_rival_and_single_launch_plans_runs_the_default_schedule(flags):
    p, g = _params(1)
    log_n = 17 if "single_launch" in flags else 14
    pl = _plan(1, 4, log_n, **flags)
    coeffs = [_rand(p, pl.n >> 2, 77)]
    got = _run_case(pl, coeffs, 2, g, 1)
    assert got == _expected(coeffs[0], p, g, g, log_n, 4)


@pytest.mark.parametrize("fid,L", [(1, 4), (3, 1), (4, 1)], ids=["bn254", "goldilocks", "babybear"])
def test_lde_from_evals(fid, L):
    """Evaluations of a random polynomial of degree < n on <w_n> extend to its coset evaluations on N."""
    from ntt_amd.ntt import lde_from_evals
    from oracle import ntt_ref as R
    p, g = _params(fid)
    log_N = ENGINES[fid, L] + 1
    log_n = log_N - 2
    small, big = _plan(fid, L, log_n), _plan(fid, L, log_N)
    batch = 2
    coeffs = [_rand(p, small.n, 11 + v) for v in range(batch)]
    w = R.root_of_unity(p, g, small.n)
    evals = []
    for c in coeffs:
        evals += _expected(c, p, g, 1, log_n, L)  # the plain forward transform: evaluations on <w_n>
    assert evals[1] == sum(cj * pow(w, j, p) for j, cj in enumerate(coeffs[0])) % p
    t = _dev(evals, small)
    out = _poisoned(big, batch)
    lde_from_evals(small, big, t, out, shift=g, batch=batch)
    assert _ints(t) == coeffs[0] + coeffs[1]  # the inverse overwrote the evaluations
    got = _ints(out)
    for v in range(batch):
        assert got[v * big.n:(v + 1) * big.n] == _expected(coeffs[v], p, g, g, log_N, L), (fid, v)


@pytest.mark.parametrize("fid,L", list(ENGINES), ids=IDS)
def test_lde_launch_count_and_labels(fid, L):
    """One entry per pass of the plan, labelled with the existing kinds: column passes c<r>, the final
    pass f<r>, a single tile s<r>.  (The 6-limb engine above 2^255, which no built-in field runs on,
    takes one more launch: test_lde_scale_launch_of_the_14_limb_engine_is_recorded.)"""
    p, g = _params(fid)
    sizes = [ENGINES[fid, L], ENGINES[fid, L] + 1] + ([THREE_PASS[fid, L]] if (fid, L) in THREE_PASS else [])
    for log_n in sizes:
        pl = _plan(fid, L, log_n)
        pl.set_profiling(True)
        try:
            t_in, out = _dev(_rand(p, pl.n >> 1, 1), pl), _poisoned(pl, 1)
            for shift in (None, g):
                pl.lde_batch(t_in, out, 1, shift, 1)
                torch.cuda.synchronize()
                labels = pl.last_launch_labels()
                r = pl.passes
                exp = [f"s{r[0]}"] if len(r) == 1 else [f"c{x}" for x in r[:-1]] + [f"f{r[-1]}"]
                assert len(labels) == len(r), (fid, L, log_n, labels)
                assert [l.rstrip("s") if l.startswith("c") else l for l in labels] == exp, (fid, L, log_n, labels)
        finally:
            pl.set_profiling(False)


def test_lde_scale_launch_of_the_14_limb_engine_is_recorded():
    """A 6-limb modulus above 2^255 with a shift: the launch that scales the inputs is an interval of the
    call's record ahead of the passes, so last_launch_ms has one entry more than the plan has passes.
    It has no pass kind and is unlabelled, and ntt_plan_last_launch_labels leaves unlabelled intervals
    out (as for the rival schedules' rounds), so the labels are the passes'.  Without a shift there is
    no such launch."""
    p, g = _ntt_prime(380)
    for log_n in (10, 12):
        pl = _custom_plan(p, g, 6, log_n)
        r = pl.passes
        exp = [f"s{r[0]}"] if len(r) == 1 else [f"c{x}" for x in r[:-1]] + [f"f{r[-1]}"]
        assert (r[0] > 4) if len(r) == 1 else (r[0] != 3), r  # not a size on the zero-padded staging route
        pl.set_profiling(True)
        try:
            t_in, out = _dev(_rand(p, pl.n >> 1, 1), pl), _poisoned(pl, 1)
            for shift, extra in ((g, 1), (None, 0)):
                pl.lde_batch(t_in, out, 1, shift, 1)
                torch.cuda.synchronize()
                labels = [l.rstrip("s") if l.startswith("c") else l for l in pl.last_launch_labels()]
                assert labels == exp, (log_n, shift is not None, labels)
                ms = pl.last_launch_ms()
                assert len(ms) == len(r) + extra and all(v > 0 for v in ms), (log_n, shift is not None, ms)
                pl.set_profiling(False)  # a fresh record: the two calls differ in their launches
                pl.set_profiling(True)
        finally:
            pl.set_profiling(False)


CHILD = r'''
import sys
sys.path.insert(0, ROOT)
import torch
from ntt_amd import lib as L
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
sys.path.insert(0, ROOT + "/tests")
import test_gpu_lde as T
for fid, limbs in ((1, 4), (3, 1), (4, 1)):
    p, g = T._params(fid)
    log_n = T.ENGINES[fid, limbs] + 1
    pl = T._plan(fid, limbs, log_n)
    coeffs = [T._rand(p, pl.n, 5 + v) for v in range(3)]
    for lb in (1, pl.passes[0] + 1):
        for shift in (None, g):
            got = T._run_case(pl, coeffs, lb, shift, 3)
            for v in range(3):
                exp = T._expected(coeffs[v][:pl.n >> lb], p, g, 1 if shift is None else shift, log_n, limbs)
                assert got[v * pl.n:(v + 1) * pl.n] == exp, (fid, lb, shift, v)
            st = pl.device_status()
            assert st == 0, (fid, lb, shift, hex(st))
print("LDE-DEBUG-OK")
'''


def test_lde_checked_build_reports_clean_status():
    """The two-pass cases of BN254, Goldilocks and BabyBear, log_blowup = r_1 + 1 among them, through the
    checked build in a fresh process: right results and no bounds / canonical / lazy-bound report."""
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "LDE-DEBUG-OK" in r.stdout
