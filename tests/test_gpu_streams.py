"""Every launching call of include/ntt.h runs on the caller's stream, and returns before that stream has run.

The held-stream harness (_held): the plan is warmed up on the default stream with other data, so that its
scratch, its plan-owned buffers and its lazily built tables exist and hold another call's values; `want` is the
call on the real input and `stale` the call on a poison-filled input, both on the default stream, and the two
must differ.  Then a non-blocking side stream S is held by a time-bounded spin (torch.cuda._sleep); behind the
spin S gets the poison of the outputs, the copy of the real input over a poison-filled buffer, and the call
under test.  A launch or an asynchronous copy of the call that went to stream 0, or to any stream but S, runs
while S is held: it reads poison or the warm-up's scratch, or its stores are poisoned over afterwards, so the
result differs from `want`.  The control cases route the call to the default stream on purpose and require the
difference.  `busy` (S not finished right after the call returned) shows that the call did not wait for its
stream; a hold that ended before that check fails the case, it never passes it.

call                                          engines                           host side
--------------------------------------------  --------------------------------  ---------------------------------
forward / inverse / *_batch                   G B P31 BN254 P                   asynchronous (asserted)
forward_coset / inverse_coset, cached shift   G B P31 BN254 P                   asynchronous (asserted)
forward_coset / *_matrix(shift=), new shift   G B                               may block (the cached tables are
                                                                                rebuilt); not stated in ntt.h, so
                                                                                only the results are checked
pointwise_mul / polymul / inv_pointwise_batch G B P31 BN254 P                   asynchronous (asserted)
fill / fill_map / twiddle_pack / transpose    G B P31 BN254 P                   asynchronous (asserted)
in_place, no_swap (odd log n), montgomery_io  BN254 (+ P in place, B Montgomery) asynchronous (asserted)
lde_batch (fused, staged, staging launch)     G B P31, BLS12-381 on 6 limbs     asynchronous (asserted; ntt.h:245)
forward_matrix / inverse_matrix / lde_matrix  G B P31                           asynchronous (asserted; ntt.h:274)
fri_fold                                      G B P31                           asynchronous (asserted; ntt.h:346)
deep_points / open_matrix / deep_quotient     G B P31                           asynchronous (asserted; ntt.h:394)
RankPlan fill / rows / cols (+ _piece)        G BN254                           asynchronous (asserted; ntt.h:522)
set_profiling + a transform                   B                                 asynchronous (asserted; ntt.h:463)
count_noncanonical                            G BN254                           blocking (ntt.h:430)
device_status                                 BN254                             blocking (ntt.h:194)
last_launch_ms                                B                                 blocking (ntt.h:465 "waiting for
                                                                                the most recent one")
(G Goldilocks, B BabyBear, P31 the custom 4-byte prime of test_gpu_matrix.py, P = 469762049.)

Sizes come from the schedules the plans report.  Vector calls: the smallest size of 2 passes on every engine, and
the smallest of 3 passes where one exists up to 2^18: Goldilocks and BN254 (2^17).  BabyBear, P31 and P have none
up to 2^18 (asserted) and get no 3-pass vector case.  The matrix schedules reach 3 passes only at 2^19 (6 + 6 + 7
on both engines); the three-launch matrix route runs at that size, at widths 3 and 17.

Every case passes its stream through the `stream=` argument; the first case of every list also runs through the
current-stream context (the rank plan has no argument and always takes the current stream).

The hold (HOLD_MS): 20 x the host wall time of the longest enqueue sequence among the cases, measured on the
MI355X with S not held, clamped to 20..250 ms.  Measured (test_the_hold_is_twenty_times_the_longest_enqueue
repeats it and prints the figures): over all cases and three rounds the worst single time was 0.13 ms (a vector
forward behind its input copy); by the best of three rounds the longest sequence is the chained points, open,
quotient and fold at 0.08 ms.  20 x 0.13 ms = 2.6 ms, so the lower clamp holds: 20 ms
(the spin then lasts 19.6 ms by events).  torch.cuda._sleep counts device clock cycles, about 2.35e6 per ms
here; the rate is measured at the first use.

The side stream is created once and probed (_side_streams): a stream that shares a hardware queue with the
default stream would hold the default stream too, and a launch misrouted to stream 0 would then pass unnoticed.

`want` is the library's own default-stream result; one case per family (vector, lde, matrix, fold, deep) also
compares it with the oracle helpers of the other test files, so the file does not rest on self-comparison."""
import time

import numpy as np
import pytest
import torch

from tests import test_gpu_deep as D
from tests import test_gpu_fold as F
from tests import test_gpu_matrix as T

pytestmark = pytest.mark.gpu

MEASURED_MS = 0.13  # the longest enqueue sequence on the MI355X, S not held (see the module docstring)
HOLD_MS = min(250.0, max(20.0, 20 * MEASURED_MS))
OTHER, REAL = 1, 2  # seeds: the warm-up's data, the case's data

ENGINES = {"goldilocks": (3, 1), "babybear": (4, 1), "p31": ("p31", 1), "bn254": (1, 4), "p469762049": (0, 1),
           "bls381x6": (2, 6)}
VECTOR = ("goldilocks", "babybear", "p31", "bn254", "p469762049")
MATRIX = ("goldilocks", "babybear", "p31")
EXT = {"goldilocks": (2, 7), "babybear": (4, 11), "p31": (2, T.G31)}  # the DEEP cases' extension (d, W)
THREE_PASS_VECTOR = ("goldilocks", "bn254")  # the engines with a 3-pass vector size up to 2^18

PROBED = []      # (stream handle, ran beside the default stream) of every side-stream candidate
_PLANS, _SIZES, _SRC, _RATE, _SIDE = {}, {}, {}, [], []


# ------------------------------------------------------------------------------------------------ plans and data
def _new_plan(eng, log_n, **kw):
    from ntt_amd.ntt import NTTPlan
    fid, limbs = ENGINES[eng]
    if fid == "p31":
        return NTTPlan(log_n=log_n, limbs64=1, modulus=T.P31, generator=T.G31, elem32=True, **kw)
    return NTTPlan(fid, log_n, limbs, **kw)


def _plan(eng, log_n, **kw):
    key = (eng, log_n, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = _new_plan(eng, log_n, **kw)
    return _PLANS[key]


def _vector_sizes(eng):
    """[the smallest log_n of at least 2 passes, the smallest of 3 where one exists up to 2^18], as the plans
    report them."""
    if eng not in _SIZES:
        two = three = None
        for log_n in range(2, 19):
            k = len(_new_plan(eng, log_n).passes)
            if k >= 2 and two is None:
                two = log_n
            if k >= 3:
                three = log_n
                break
        assert two is not None, eng
        _SIZES[eng] = [two] + ([three] if three not in (None, two) else [])
    return _SIZES[eng]


def _matrix_size(eng, width, passes):
    """The smallest log_n whose matrix schedule at this width has `passes` passes."""
    key = (eng, width, passes)
    if key not in _SIZES:
        for log_n in range(3, 25):
            k = len(_new_plan(eng, log_n).matrix_passes(width))
            if k >= passes:
                assert k == passes, (key, log_n, k)
                _SIZES[key] = log_n
                break
    assert key in _SIZES, key
    return _SIZES[key]


def _spec(pl, count):
    return pl.dtype, ((count,) if pl.limbs64 == 1 else (count, pl.limbs64))


def _poison_t(dtype, shape):
    return torch.full(shape, T.POISON32 if dtype == torch.int32 else T.POISON64, dtype=dtype, device="cuda:0")


def _poison_like(t):
    return _poison_t(t.dtype, tuple(t.shape))


def _rand(pl, count, seed):
    """`count` seeded canonical elements on the device; cached, so never written."""
    key = (pl.p, pl.limbs64, pl.elem32, count, seed)
    if key not in _SRC:
        if pl.limbs64 == 1:
            _SRC[key] = T._dev(T._rand(pl.p, count, 1, seed), pl)
        else:
            from oracle import oracle_c as OC
            host = np.zeros((count, pl.limbs64), dtype=np.uint64)
            host[:, :4] = OC.random_limbs(pl.field_id, count, seed, 4)  # the 255-bit fields: upper limbs zero
            _SRC[key] = torch.from_numpy(np.ascontiguousarray(host).view(np.int64)).to("cuda:0")
    return _SRC[key]


# ------------------------------------------------------------------------------------------------ the harness
def _cycles_per_ms():
    """torch.cuda._sleep counts device clock cycles; their rate is measured once with events."""
    if not _RATE:
        torch.cuda._sleep(1000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 1_000_000
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        _RATE.append(cycles / max(a.elapsed_time(b), 1e-3))
    return _RATE[0]


def _hold(ms):
    """a time-bounded hold of the current stream (torch's spin kernel: one wave, bounded by its cycle count)"""
    torch.cuda._sleep(int(ms * _cycles_per_ms()))


def _need_sleep():
    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep unavailable")
    _cycles_per_ms()


def _side_streams(count=1):
    """`count` side streams, created once and reused by every case.  PyTorch creates its streams non-blocking:
    S does not wait for the legacy default stream and the default stream does not wait for S, so a misrouted
    launch is unordered, as in a prover; the harness depends on it.  It also depends on the default stream running
    while S is held, and the HIP runtime spreads its streams over a few hardware queues (4 by default): a
    stream that shares the default stream's queue holds the default stream with it, and a launch misrouted to
    stream 0 would then run in order after all.  So each candidate is probed -- held for a few milliseconds
    while one element is written on the default stream -- and taken only if the default stream finished
    first."""
    if len(_SIDE) >= count:
        return _SIDE[:count]
    probe = torch.zeros(1, device="cuda:0")
    for _ in range(32):
        if len(_SIDE) >= count:
            break
        S = torch.cuda.Stream()
        if any(S.cuda_stream == t.cuda_stream for t in _SIDE):
            continue
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            _hold(5.0)
        probe.add_(1)
        t0 = time.perf_counter()
        while not torch.cuda.default_stream().query() and time.perf_counter() - t0 < 1.0:
            pass
        independent = not S.query()
        torch.cuda.synchronize()
        PROBED.append((S.cuda_stream, independent))
        if independent:
            _SIDE.append(S)
    assert len(_SIDE) >= count, f"no side stream runs beside the default stream: {PROBED}"
    return _SIDE[:count]


class Case:
    """One call under test.  make(seed) -> the input tensors (cached, never written); outs: (dtype, shape) of the
    output buffers; call(ins, outs, stream) enqueues the call (stream None: the current stream); const: the
    inputs the call must not modify; asynchronous: the call is documented to return without waiting."""

    def __init__(self, name, make, outs, call, const=(), asynchronous=True):
        self.name, self.make, self.outs, self.call, self.const = name, make, outs, call, tuple(const)
        self.asynchronous = asynchronous


class Rec:
    pass


def _buffers(case, srcs):
    return [s.clone() for s in srcs], [_poison_t(*o) for o in case.outs]


def _written(case, ins, outs):
    return [t for i, t in enumerate(ins) if i not in case.const] + outs


def _on_default(case, srcs):
    ins, outs = _buffers(case, srcs)
    case.call(ins, outs, None)
    torch.cuda.synchronize()
    return _written(case, ins, outs)


def _held(case, hold_ms=None, misroute=False, via_arg=True):
    """The held-stream sequence of the module docstring.  hold_ms = 0 enqueues on an idle S (the measurement of
    the enqueue time); misroute issues the call on the default stream (the control cases); via_arg False leaves
    the stream to the current-stream context instead of the `stream=` argument."""
    hold_ms = HOLD_MS if hold_ms is None else hold_ms
    real = case.make(REAL)
    _on_default(case, case.make(OTHER))  # warm-up: scratch, plan-owned buffers and tables hold other data
    rec = Rec()
    rec.want = _on_default(case, real)
    poison_in = [_poison_like(s) for s in real]
    stale = _on_default(case, poison_in) if real else [_poison_like(t) for t in rec.want]
    assert not all(torch.equal(a, b) for a, b in zip(rec.want, stale)), f"{case.name}: want == stale, no power"
    ins, outs = _buffers(case, poison_in)
    torch.cuda.synchronize()
    S = _side_streams()[0]  # non-blocking, and on another hardware queue than the default stream
    with torch.cuda.stream(S):
        if hold_ms:
            _hold(hold_ms)
        t0 = time.perf_counter()
        for o in outs:
            o.fill_(T.POISON32 if o.dtype == torch.int32 else T.POISON64)
        for x, s in zip(ins, real):
            x.copy_(s)
        case.call(ins, outs, torch.cuda.default_stream() if misroute else (S if via_arg else None))
        rec.enqueue_ms = (time.perf_counter() - t0) * 1e3
        rec.busy = not S.query()
    S.synchronize()
    torch.cuda.synchronize()
    rec.got = _written(case, ins, outs)
    rec.kept = all(torch.equal(ins[i], real[i]) for i in case.const)
    return rec


def _late(rec):
    return (f"the hold ended before the check: the case proves nothing (enqueue took {rec.enqueue_ms:.2f} ms of a "
            f"{HOLD_MS:.0f} ms hold: the call waited for its stream, or the hold is too short)")


def _problems(case, via_arg=True):
    rec = _held(case, via_arg=via_arg)
    out = []
    if not all(torch.equal(a, b) for a, b in zip(rec.got, rec.want)):
        out.append("differs from the default-stream result: a launch or copy did not run on the caller's stream")
    if not rec.kept:
        out.append("an input was modified")
    if case.asynchronous and not rec.busy:
        out.append(_late(rec))
    return [f"{case.name}{'' if via_arg else ' (current-stream context)'}: {m}" for m in out], rec


def _run_all(cases):
    assert cases
    bad = []
    for case in cases:
        bad += _problems(case)[0]
    bad += _problems(cases[0], via_arg=False)[0]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ vector calls
def _vector_cases(eng, log_n, full=True):
    pl = _plan(eng, log_n)
    n, g, tag = pl.n, pl.g, f"{eng}/2^{log_n}"
    one = lambda seed: [_rand(pl, n, seed)]
    two = lambda seed: [_rand(pl, n, seed), _rand(pl, n, seed + 10)]
    three = lambda seed: [_rand(pl, 3 * n, seed)]
    cases = [
        Case(f"{tag} forward", one, [], lambda i, o, s: pl.forward(i[0], stream=s)),
        Case(f"{tag} inverse", one, [], lambda i, o, s: pl.inverse(i[0], stream=s)),
        Case(f"{tag} forward_batch", three, [], lambda i, o, s: pl.forward_batch(i[0], 3, stream=s)),
        Case(f"{tag} forward_coset", one, [], lambda i, o, s: pl.forward_coset(i[0], g, stream=s)),
        Case(f"{tag} inverse_coset", one, [], lambda i, o, s: pl.inverse_coset(i[0], g, stream=s)),
        Case(f"{tag} polymul", two, [], lambda i, o, s: pl.polymul(i[0], i[1], i[0], stream=s)),  # c aliases a
    ]
    if not full:
        return cases
    tw = _plan(eng, log_n, twiddle_only=True)
    lr, lc = 5, log_n - 5
    cases += [
        Case(f"{tag} inverse_batch", three, [], lambda i, o, s: pl.inverse_batch(i[0], 3, stream=s)),
        Case(f"{tag} pointwise_mul", two, [_spec(pl, n)], lambda i, o, s: pl.pointwise_mul(i[0], i[1], o[0], stream=s),
             const=(0, 1)),
        Case(f"{tag} inverse_pointwise_batch", lambda seed: [_rand(pl, 3 * n, seed), _rand(pl, 3 * n, seed + 10)],
             [_spec(pl, 3 * n)], lambda i, o, s: pl.inverse_pointwise_batch(i[0], i[1], o[0], 3, stream=s), const=(0, 1)),
        Case(f"{tag} fill iota", lambda seed: [], [_spec(pl, n)], lambda i, o, s: pl.fill(o[0], "iota", stream=s)),
        Case(f"{tag} fill random", lambda seed: [], [_spec(pl, n)],
             lambda i, o, s: pl.fill(o[0], "random", seed=7, stream=s)),
        Case(f"{tag} fill_map", lambda seed: [], [_spec(pl, n)],
             lambda i, o, s: tw.fill_map(o[0], "random", 9, 5, 4, log_n - 5, stream=s)),
        Case(f"{tag} twiddle_pack", one, [_spec(pl, n)],
             lambda i, o, s: tw.twiddle_pack(i[0], o[0], lr, lc, lc, 7, stream=s), const=(0,)),
        Case(f"{tag} transpose", one, [_spec(pl, n)], lambda i, o, s: tw.transpose(i[0], o[0], lr, lc, stream=s),
             const=(0,)),
    ]
    return cases


@pytest.mark.parametrize("eng", VECTOR)
def test_vector_calls_run_on_the_callers_stream(eng):
    """The smallest 2-pass size of every engine."""
    _need_sleep()
    sizes = _vector_sizes(eng)
    assert len(sizes) == (2 if eng in THREE_PASS_VECTOR else 1), (eng, sizes)  # as the module docstring says
    assert len(_plan(eng, sizes[0]).passes) == 2
    _run_all(_vector_cases(eng, sizes[0]))


@pytest.mark.parametrize("eng", THREE_PASS_VECTOR)
def test_vector_calls_of_three_passes(eng):
    """The smallest 3-pass size, on the engines that have one up to 2^18."""
    _need_sleep()
    log_n = _vector_sizes(eng)[1]
    assert len(_plan(eng, log_n).passes) == 3
    _run_all(_vector_cases(eng, log_n))


def test_bn254_at_the_benchmark_size():
    """2^20 on 4 limbs: 4096-element tiles for single transforms, 1024-element tiles for batches, and
    forward_coset's own cache."""
    _need_sleep()
    assert _plan("bn254", 20).passes == [10, 10]
    _run_all(_vector_cases("bn254", 20))


def _forward_like(pl, tag, batch=True):
    n = pl.n
    cases = [Case(f"{tag} forward", lambda seed: [_rand(pl, n, seed)], [], lambda i, o, s: pl.forward(i[0], stream=s))]
    if batch:
        cases += [
            Case(f"{tag} inverse", lambda seed: [_rand(pl, n, seed)], [], lambda i, o, s: pl.inverse(i[0], stream=s)),
            Case(f"{tag} forward_batch", lambda seed: [_rand(pl, 3 * n, seed)], [],
                 lambda i, o, s: pl.forward_batch(i[0], 3, stream=s))]
    return cases


@pytest.mark.parametrize("eng", ["bn254", "p469762049"])
def test_in_place_plans(eng):
    _need_sleep()
    _run_all(_forward_like(_plan(eng, 12, in_place=True), f"{eng}/2^12 in_place"))


def test_no_swap_rival_ends_in_a_device_copy():
    """The smallest odd size of several launches: the last round lands in the plan buffer and one device copy
    brings it back (ntt.h NTT_PLAN_NO_SWAP)."""
    _need_sleep()
    from ntt_amd import lib as L
    pl = None
    for log_n in range(3, 16, 2):
        try:
            pl = _plan("bn254", log_n, no_swap=True)
            break
        except L.NTTError:
            continue
    assert pl is not None
    _run_all(_forward_like(pl, f"bn254/2^{pl.log_n} no_swap", batch=False))


@pytest.mark.parametrize("eng", ["bn254", "babybear"])
def test_montgomery_io_plans(eng):
    _need_sleep()
    log_n = _vector_sizes(eng)[0]
    pl = _plan(eng, log_n, montgomery_io=True)
    n, tag = pl.n, f"{eng}/2^{log_n} montgomery_io"
    _run_all([
        Case(f"{tag} forward", lambda seed: [_rand(pl, n, seed)], [], lambda i, o, s: pl.forward(i[0], stream=s)),
        Case(f"{tag} pointwise_mul", lambda seed: [_rand(pl, n, seed), _rand(pl, n, seed + 10)], [_spec(pl, n)],
             lambda i, o, s: pl.pointwise_mul(i[0], i[1], o[0], stream=s), const=(0, 1))])


@pytest.mark.parametrize("eng", VECTOR)
def test_control_a_call_on_the_default_stream_is_detected(eng):
    """The same sequence with the call issued on the default stream while its input copy sits on the held S:
    the result must differ from `want` (valid memory only: wrong values, never a fault)."""
    _need_sleep()
    case = _vector_cases(eng, _vector_sizes(eng)[0], full=False)[0]
    rec = _held(case, misroute=True)
    assert rec.busy, _late(rec)
    assert not all(torch.equal(a, b) for a, b in zip(rec.got, rec.want)), f"{case.name}: a misrouted call went unnoticed"


def test_the_hold_is_twenty_times_the_longest_enqueue():
    """The rule behind HOLD_MS, repeated: the longest enqueue sequences of the families (a vector forward and a
    polymul, a 3-pass matrix forward, an extension, the chained DEEP calls and fold, a rank-plan step) are timed
    on the idle S, hold_ms = 0, the best of three rounds each; 20 x the longest, clamped to 20..250 ms, must not
    exceed the hold the cases use."""
    _need_sleep()
    gold = _vector_sizes("goldilocks")[0]
    cases = [_vector_cases("goldilocks", gold, full=False)[0], _vector_cases("bn254", 20, full=False)[-1],
             _matrix_cases("goldilocks", _matrix_size("goldilocks", 3, 3), 3)[0], _lde_cases("goldilocks", gold, "multi-pass")[0],
             _deep_cases("goldilocks", 12, 37)[-1], _deep_cases("babybear", 5, 16)[-1], _rank_cases("bn254", 1)[1]]
    times = {}
    for case in cases:
        recs = [_held(case, hold_ms=0.0) for _ in range(3)]
        assert all(torch.equal(a, b) for r in recs for a, b in zip(r.got, r.want)), case.name
        times[case.name] = min(r.enqueue_ms for r in recs)
    longest = max(times.values())
    print({k: round(v, 3) for k, v in times.items()}, "hold", HOLD_MS)
    assert min(250.0, max(20.0, 20 * longest)) <= HOLD_MS, (times, HOLD_MS)


def test_vector_want_is_the_oracles():
    from oracle import oracle_c as OC
    _need_sleep()
    eng = "goldilocks"
    log_n = _vector_sizes(eng)[0]
    pl = _plan(eng, log_n)
    case = _vector_cases(eng, log_n, full=False)[0]
    bad, rec = _problems(case)
    assert not bad, bad
    x = T._host(_rand(pl, pl.n, REAL), pl.n, 1)
    assert np.array_equal(T._host(rec.want[0], pl.n, 1), T._expected(x, pl.p, pl.g, 1, log_n))
    eng = "bn254"
    log_n = _vector_sizes(eng)[0]
    pl = _plan(eng, log_n)
    bad, rec = _problems(_vector_cases(eng, log_n, full=False)[0])
    assert not bad, bad
    x = _rand(pl, pl.n, REAL).cpu().numpy().view(np.uint64)
    assert np.array_equal(rec.want[0].cpu().numpy().view(np.uint64), OC.ntt_mp(x, pl.p, pl.g))


# ------------------------------------------------------------------------------------------------ lde_batch
def _lde_cases(eng, log_n, why):
    pl = _plan(eng, log_n)
    half = pl.n >> 1
    return [Case(f"{eng}/2^{log_n} lde_batch {why} shift={'g' if shift else None}", lambda seed: [_rand(pl, 2 * half, seed)],
                 [_spec(pl, 2 * pl.n)], lambda i, o, s, shift=shift: pl.lde_batch(i[0], o[0], 1, shift, 2, stream=s),
                 const=(0,)) for shift in (pl.g, None)]


@pytest.mark.parametrize("eng", MATRIX + ("bls381x6",))
def test_lde_batch_routes(eng):
    """batch 2, log_blowup 1: a fusable multi-pass size and 4 points (memset + 2D copy + scale + passes); on the
    6 limbs of BLS12-381 the scaled inputs go through a staging launch into the plan's buffer."""
    _need_sleep()
    if eng == "bls381x6":
        _run_all(_lde_cases(eng, _vector_sizes(eng)[0], "staging launch"))
        return
    _run_all(_lde_cases(eng, _vector_sizes(eng)[0], "multi-pass") + _lde_cases(eng, 2, "4 points"))


def test_lde_want_is_the_oracles():
    _need_sleep()
    eng = "goldilocks"
    log_n = _vector_sizes(eng)[0]
    pl = _plan(eng, log_n)
    bad, rec = _problems(_lde_cases(eng, log_n, "multi-pass")[0])
    assert not bad, bad
    x = T._host(_rand(pl, pl.n, REAL), 2, pl.n >> 1)
    for v in range(2):
        exp = T._expected(np.ascontiguousarray(x[v]).reshape(-1, 1), pl.p, pl.g, pl.g, log_n)
        assert np.array_equal(T._host(rec.want[0], 2, pl.n)[v], exp[:, 0]), v


# ------------------------------------------------------------------------------------------------ matrix calls
def _matrix_cases(eng, log_n, width):
    pl = _plan(eng, log_n)
    n, g, tag = pl.n, pl.g, f"{eng}/2^{log_n}x{width}"
    whole = lambda seed: [_rand(pl, n * width, seed)]
    half = lambda seed: [_rand(pl, (n >> 1) * width, seed)]
    out = [_spec(pl, n * width)]
    return [
        Case(f"{tag} forward_matrix", whole, [], lambda i, o, s: pl.forward_matrix(i[0], width, stream=s)),
        Case(f"{tag} inverse_matrix", whole, [], lambda i, o, s: pl.inverse_matrix(i[0], width, stream=s)),
        Case(f"{tag} lde_matrix", half, out, lambda i, o, s: pl.lde_matrix(i[0], o[0], 1, None, width, stream=s),
             const=(0,)),
        Case(f"{tag} forward_matrix shift bitrev", whole, [],
             lambda i, o, s: pl.forward_matrix(i[0], width, stream=s, shift=g, bitrev_out=True)),
        Case(f"{tag} inverse_matrix shift bitrev", whole, [],
             lambda i, o, s: pl.inverse_matrix(i[0], width, stream=s, shift=g, bitrev_in=True)),
        Case(f"{tag} lde_matrix shift bitrev", half, out,
             lambda i, o, s: pl.lde_matrix(i[0], o[0], 1, g, width, stream=s, bitrev_out=True), const=(0,)),
    ]


@pytest.mark.parametrize("passes", [0, 2, 3])
@pytest.mark.parametrize("width", [3, 17])
@pytest.mark.parametrize("eng", MATRIX)
def test_matrix_calls_run_on_the_callers_stream(eng, width, passes):
    """log n = 1 (no pass kernel: the copy / naive route), the smallest 2-pass and the smallest 3-pass size (2^19:
    the matrix schedules have no 3-pass size below it)."""
    _need_sleep()
    log_n = 1 if passes == 0 else _matrix_size(eng, width, passes)
    assert len(_plan(eng, log_n).matrix_passes(width)) == passes
    _run_all(_matrix_cases(eng, log_n, width))


def test_matrix_want_is_the_oracles():
    _need_sleep()
    eng, width = "babybear", 3
    log_n = _matrix_size(eng, width, 2)
    pl = _plan(eng, log_n)
    bad, rec = _problems(_matrix_cases(eng, log_n, width)[0])
    assert not bad, bad
    x = T._host(_rand(pl, pl.n * width, REAL), pl.n, width)
    assert np.array_equal(T._host(rec.want[0], pl.n, width), T._expected(x, pl.p, pl.g, 1, log_n))


# ------------------------------------------------------------------------------------------------ fri_fold
FOLD_L = 9


def _fold_case(fid, d, w, k, oracle_input=False):
    pl = T._plan(fid, F.LOG_N)
    beta = F._betas(pl.p, d, 40 + k)[0]

    def make(seed):
        if oracle_input and seed == REAL:
            return [T._dev(F._input(fid, d, FOLD_L, pl.g), pl)]
        return [_rand(pl, (1 << FOLD_L) * d, seed)]

    return Case(f"f{fid} fri_fold d={d} k={k}", make, [_spec(pl, (1 << (FOLD_L - k)) * d)],
                lambda i, o, s: pl.fri_fold(i[0], o[0], k, beta, ext_degree=d, ext_w=w or 0, shift=pl.g,
                                            log_rows=FOLD_L, stream=s), const=(0,)), beta


@pytest.mark.parametrize("staged", ["0", "1"])
@pytest.mark.parametrize("fid,d,w", [e for e in F.EXTS if e[0] in (3, 4, "p31")])
def test_fri_fold_runs_on_the_callers_stream(fid, d, w, staged, monkeypatch):
    """(d, k) = (1, 1), (2, 2), (4, 4) as the field has the extension; log_rows 9 on a plan of 2^12; both load
    forms."""
    _need_sleep()
    monkeypatch.setenv("NTT_FOLD_STAGED", staged)
    _run_all([_fold_case(fid, d, w, d)[0]])


def test_fold_want_is_the_oracles():
    _need_sleep()
    fid, d, w, k = 4, 4, 11, 4
    case, beta = _fold_case(fid, d, w, k, oracle_input=True)
    bad, rec = _problems(case)
    assert not bad, bad
    g = T._params(fid)[1]
    assert np.array_equal(T._host(rec.want[0], 1 << (FOLD_L - k), d), F._expected_fold(fid, d, w, FOLD_L, k, g, beta))


# ------------------------------------------------------------------------------------------------ DEEP calls
def _deep_cases(eng, L, W, oracle_input=False):
    fid = ENGINES[eng][0]
    d, w = EXT[eng]
    pl = T._plan(fid, D.LOG_N)
    g, rows, tag = pl.g, 1 << L, f"{eng} 2^{L}x{W} d={d}"
    z = D._z(fid, d, L, g, 600 + L)
    alpha, scale = D._alphas(pl.p, d, 601)[0], D._alphas(pl.p, d, 602)[0]
    kw = dict(ext_degree=d, ext_w=w, log_rows=L)

    def mat(seed):
        if oracle_input and seed == REAL:
            return T._dev(D._matrix(fid, L, W, g, True), pl)
        return _rand(pl, rows * W, seed)

    def points(out, s):
        pl.deep_points(out, z, shift=g, bitrev=True, stream=s, **kw)

    def inv(seed):  # deep_points' own output for z, computed on the default stream (the same for every seed)
        key = (eng, L, "inv")
        if key not in _SRC:
            t = _poison_t(*_spec(pl, rows * d))
            points(t, None)
            torch.cuda.synchronize()
            _SRC[key] = t
        return _SRC[key]

    def chain(i, o, s):  # the pipeline of test_pipeline_from_the_extension_to_the_fold from the points on
        points(o[0], s)
        pl.open_matrix(i[0], W, o[0], o[1], z, shift=g, bitrev=True, stream=s, **kw)
        pl.deep_quotient(i[0], W, o[0], o[1], o[2], alpha, scale=scale, stream=s, **kw)
        pl.fri_fold(o[2], o[3], 1, alpha, ext_degree=d, ext_w=w, shift=g, log_rows=L, stream=s)

    val = lambda seed: _rand(pl, W * d, seed + 20)
    return [
        Case(f"{tag} deep_points", lambda seed: [], [_spec(pl, rows * d)], lambda i, o, s: points(o[0], s)),
        Case(f"{tag} open_matrix", lambda seed: [mat(seed), inv(seed)], [_spec(pl, W * d)],
             lambda i, o, s: pl.open_matrix(i[0], W, i[1], o[0], z, shift=g, bitrev=True, stream=s, **kw), const=(0, 1)),
        Case(f"{tag} deep_quotient", lambda seed: [mat(seed), inv(seed), val(seed)], [_spec(pl, rows * d)],
             lambda i, o, s: pl.deep_quotient(i[0], W, i[1], i[2], o[0], alpha, scale=scale, stream=s, **kw),
             const=(0, 1, 2)),
        Case(f"{tag} deep_quotient accumulate",
             lambda seed: [mat(seed), inv(seed), val(seed), _rand(pl, rows * d, seed + 30)], [],
             lambda i, o, s: pl.deep_quotient(i[0], W, i[1], i[2], i[3], alpha, accumulate=True, stream=s, **kw),
             const=(0, 1, 2)),
        Case(f"{tag} points, open, quotient, fold chained", lambda seed: [mat(seed)],
             [_spec(pl, rows * d), _spec(pl, W * d), _spec(pl, rows * d), _spec(pl, (rows >> 1) * d)], chain, const=(0,)),
    ]


@pytest.mark.parametrize("L,W", [(5, 16), (12, 37)])
@pytest.mark.parametrize("eng", list(EXT))
def test_deep_calls_run_on_the_callers_stream(eng, L, W):
    _need_sleep()
    _run_all(_deep_cases(eng, L, W))


def test_deep_want_is_the_oracles():
    _need_sleep()
    eng, L, W = "babybear", 5, 16
    fid = ENGINES[eng][0]
    d, w = EXT[eng]
    case = _deep_cases(eng, L, W, oracle_input=True)[1]
    bad, rec = _problems(case)
    assert not bad, bad
    z = D._z(fid, d, L, T._params(fid)[1], 600 + L)
    assert np.array_equal(T._host(rec.want[0], W, d), D._horner(fid, d, w, L, W, z).astype(np.uint64))


# ------------------------------------------------------------------------------------------------ the rank plan
def _rank_cases(eng, rank):
    from ntt_amd import lib as Lb
    from ntt_amd.distributed import RankPlan
    fid, limbs = ENGINES[eng]
    key = ("rplan", eng, rank)
    if key not in _PLANS:
        for log_n in range(2, 17):  # the smallest size the schedule accepts at world 2
            try:
                _PLANS[key] = RankPlan(fid, log_n, limbs, 2, rank, 0)
                break
            except Lb.NTTError:
                continue
    rp = _PLANS[key]
    lay = rp.layout
    ref = _plan(eng, 4)  # element layout of the data only
    m, tag = lay.local_n, f"{eng} rplan 2^{lay.log_n} rank {rank}"
    P, Q = min(2, lay.r), min(2, lay.c)
    one = lambda seed: [_rand(ref, m, seed)]
    two = lambda seed: [_rand(ref, m, seed), _rand(ref, m, seed + 10)]
    out = [_spec(ref, m)]

    def on(s, f, *a):  # the rank plan launches on the current stream
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream()):
            f(*a)

    return [
        Case(f"{tag} fill", lambda seed: [], out, lambda i, o, s: on(s, rp.fill, o[0], "random", 5)),
        Case(f"{tag} forward_rows", one, out, lambda i, o, s: on(s, rp.forward_rows, i[0], o[0], 1, 0), const=(0,)),
        Case(f"{tag} forward_cols", one, out, lambda i, o, s: on(s, rp.forward_cols, i[0], o[0], 1, 0), const=(0,)),
        Case(f"{tag} inverse_cols with y", two, out, lambda i, o, s: on(s, rp.inverse_cols, i[0], i[1], o[0]),
             const=(0, 1)),
        Case(f"{tag} inverse_rows", one, out, lambda i, o, s: on(s, rp.inverse_rows, i[0], o[0]), const=(0,)),
        Case(f"{tag} forward_rows_piece", one, out,
             lambda i, o, s: on(s, rp.forward_rows_piece, i[0], o[0], 1, 0, P - 1, P, Q), const=(0,)),
        Case(f"{tag} forward_cols_piece", one, out,
             lambda i, o, s: on(s, rp.forward_cols_piece, i[0], o[0], 1, 0, Q - 1, P, Q), const=(0,)),
        Case(f"{tag} inverse_cols_piece with y", two, out,
             lambda i, o, s: on(s, rp.inverse_cols_piece, i[0], i[1], o[0], Q - 1, P, Q), const=(0, 1)),
        Case(f"{tag} inverse_rows_piece", one, out,
             lambda i, o, s: on(s, rp.inverse_rows_piece, i[0], o[0], P - 1, P, Q), const=(0,)),
    ]


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("eng", ["goldilocks", "bn254"])
def test_rank_plan_calls_run_on_the_callers_stream(eng, rank):
    """One rank of a world of 2 (both ranks' plans live on one device; nothing is exchanged)."""
    _need_sleep()
    _run_all(_rank_cases(eng, rank))


# ------------------------------------------------------------------------------------------------ blocking by contract
@pytest.mark.parametrize("eng", ["goldilocks", "bn254"])
def test_count_noncanonical_counts_on_the_callers_stream(eng):
    """Blocking on its stream by contract: only the result is checked.  The real input has 3 elements that are not
    below p; the poison it is copied over has none (Goldilocks) or only such (BN254)."""
    _need_sleep()
    pl = _plan(eng, _vector_sizes(eng)[0])
    src = _rand(pl, pl.n, REAL).clone()
    src.view(-1, pl.limbs64)[[1, 77, pl.n - 1]] = -1  # all bits set: >= p
    x = _poison_like(src)
    assert pl.count_noncanonical(src) == 3 and pl.count_noncanonical(x) != 3
    torch.cuda.synchronize()
    S = _side_streams()[0]  # non-blocking, as in _held
    with torch.cuda.stream(S):
        _hold(HOLD_MS)
        x.copy_(src)
        busy = not S.query()
        bad = pl.count_noncanonical(x, stream=S)
    S.synchronize()
    assert busy, "the hold ended before the check: the case proves nothing"
    assert bad == 3


def test_device_status_waits_for_the_side_stream():
    """ntt_plan_device_status synchronises the device: after it the held forward has run, and reports nothing."""
    _need_sleep()
    eng = "bn254"
    pl = _plan(eng, _vector_sizes(eng)[0])
    src = _rand(pl, pl.n, REAL)
    want = src.clone()
    pl.forward(want)
    x = _poison_like(src)
    torch.cuda.synchronize()
    S = _side_streams()[0]  # non-blocking, as in _held
    with torch.cuda.stream(S):
        _hold(HOLD_MS)
        x.copy_(src)
        pl.forward(x, stream=S)
        busy = not S.query()
        status = pl.device_status()
        done = S.query()
    S.synchronize()
    assert busy, "the hold ended before the check: the case proves nothing"
    assert status == 0 and done and torch.equal(x, want)


# ------------------------------------------------------------------------------------------------ ordering beyond routing
@pytest.mark.parametrize("kind", ["vector", "matrix"])
@pytest.mark.parametrize("eng", ["goldilocks", "babybear"])
def test_a_shift_replaced_while_a_call_is_queued(eng, kind):
    """forward_coset(x1, c1) is queued on the held S when the same call with c2 replaces the cached c^j tables
    (plan_shift.hpp ensure_tables: free, allocate, blocking copy).  The queued call must still read c1's tables:
    both results equal their default-stream values.  The second call may block the host (ntt.h allows the
    rebuild), so nothing is asserted about `busy` after it."""
    _need_sleep()
    width = 3
    log_n = _vector_sizes(eng)[0] if kind == "vector" else _matrix_size(eng, width, 2)
    pl = _plan(eng, log_n)
    c1, c2 = pl.g, pl.p - 1
    count = pl.n * (1 if kind == "vector" else width)

    def call(t, c, s=None):
        if kind == "vector":
            pl.forward_coset(t, c, stream=s)
        else:
            pl.forward_matrix(t, width, stream=s, shift=c)

    src = [_rand(pl, count, REAL), _rand(pl, count, REAL + 1)]
    want = [s.clone() for s in src]
    call(_rand(pl, count, OTHER).clone(), c2)
    call(want[1], c2)
    call(want[0], c1)  # the cached shift is c1: nothing is rebuilt before the first held call
    xs = [_poison_like(s) for s in src]
    torch.cuda.synchronize()
    S = _side_streams()[0]  # non-blocking, as in _held
    with torch.cuda.stream(S):
        _hold(HOLD_MS)
        xs[0].copy_(src[0])
        xs[1].copy_(src[1])
        call(xs[0], c1, S)
        busy = not S.query()
        call(xs[1], c2, S)
    S.synchronize()
    assert busy, "the hold ended before the check: the case proves nothing"
    assert torch.equal(xs[0], want[0]), "the queued call did not see the tables of its own shift"
    assert torch.equal(xs[1], want[1])


def test_two_plans_on_two_held_streams():
    """A Goldilocks plan on S1 and a BabyBear plan on S2, their enqueues interleaved: a matrix forward of two
    passes, a fold and a quotient on each.  Both streams are still held after the last enqueue and both plans'
    results are right."""
    _need_sleep()
    width, Lf, Lq, W = 3, 9, 5, 16
    jobs = []
    for eng in ("goldilocks", "babybear"):
        fid = ENGINES[eng][0]
        d, w = EXT[eng]
        pl = _plan(eng, _matrix_size(eng, width, 2))
        assert len(pl.matrix_passes(width)) == 2 and pl.log_n >= Lf
        z = D._z(fid, d, Lq, pl.g, 700)
        alpha = D._alphas(pl.p, d, 701)[0]
        inv = _poison_t(*_spec(pl, (1 << Lq) * d))
        pl.deep_points(inv, z, ext_degree=d, ext_w=w, shift=pl.g, bitrev=True, log_rows=Lq)
        src = [_rand(pl, pl.n * width, REAL), _rand(pl, (1 << Lf) * d, REAL + 1), _rand(pl, (1 << Lq) * W, REAL + 2),
               inv, _rand(pl, W * d, REAL + 3)]
        steps = [
            lambda b, o, s, pl=pl: pl.forward_matrix(b[0], width, stream=s),
            lambda b, o, s, pl=pl, d=d, w=w, alpha=alpha: pl.fri_fold(b[1], o[0], d, alpha, ext_degree=d, ext_w=w,
                                                                      shift=pl.g, log_rows=Lf, stream=s),
            lambda b, o, s, pl=pl, d=d, w=w, alpha=alpha: pl.deep_quotient(b[2], W, b[3], b[4], o[1], alpha, ext_degree=d,
                                                                            ext_w=w, log_rows=Lq, stream=s)]
        outs = [_spec(pl, (1 << (Lf - d)) * d), _spec(pl, (1 << Lq) * d)]

        def run(bufs, s, steps=steps, outs=outs):
            o = [_poison_t(*spec) for spec in outs]
            for step in steps:
                step(bufs, o, s)
            return o

        run([_rand(pl, t.numel() // pl.limbs64, OTHER).clone() for t in src[:3]] + src[3:], None)  # warm-up
        b = [t.clone() for t in src]
        o = run(b, None)
        torch.cuda.synchronize()
        jobs.append(dict(src=src, steps=steps, want=[b[0]] + o, bufs=[_poison_like(t) for t in src],
                         outs=[_poison_t(*spec) for spec in outs]))
    torch.cuda.synchronize()
    streams = _side_streams(2)  # non-blocking, as in _held
    for job, S in zip(jobs, streams):
        with torch.cuda.stream(S):
            _hold(HOLD_MS)
            for x, s in zip(job["bufs"], job["src"]):
                x.copy_(s)
    for k in range(3):
        for job, S in zip(jobs, streams):
            job["steps"][k](job["bufs"], job["outs"], S)
    busy = [not S.query() for S in streams]
    for S in streams:
        S.synchronize()
    assert all(busy), f"the hold ended before the check: the case proves nothing (busy {busy})"
    for job in jobs:
        got = [job["bufs"][0]] + job["outs"]
        assert all(torch.equal(a, b) for a, b in zip(got, job["want"]))
        assert all(torch.equal(job["bufs"][i], job["src"][i]) for i in (1, 2, 3, 4)), "an input was modified"


def test_profiling_on_a_side_stream():
    """set_profiling(True): the events are recorded on the held S without a wait, the labels are those of
    test_one_launch_label_per_pass and test_profiling_labels_the_launches, and last_launch_ms (which waits for
    the most recent record) returns one positive time per label."""
    _need_sleep()
    eng, width, L, W = "babybear", 37, 9, 16
    fid = ENGINES[eng][0]
    d, w = EXT[eng]
    pl = _plan(eng, _matrix_size(eng, width, 2))
    passes = pl.matrix_passes(width)
    z = D._z(fid, d, L, pl.g, 31)
    inv = _poison_t(*_spec(pl, (1 << L) * d))
    pl.deep_points(inv, z, ext_degree=d, ext_w=w, shift=pl.g, bitrev=True, log_rows=L)
    forward = Case("profiled forward_matrix", lambda seed: [_rand(pl, pl.n * width, seed)], [],
                   lambda i, o, s: pl.forward_matrix(i[0], width, stream=s))
    opening = Case("profiled open_matrix", lambda seed: [_rand(pl, (1 << L) * W, seed), inv], [_spec(pl, W * d)],
                   lambda i, o, s: pl.open_matrix(i[0], W, i[1], o[0], z, ext_degree=d, ext_w=w, shift=pl.g, bitrev=True,
                                                  log_rows=L, stream=s), const=(0, 1))
    for case, labels in ((forward, [f"c{r}" for r in passes[:-1]] + [f"f{passes[-1]}"]), (opening, ["o", "e"])):
        pl.set_profiling(True)
        try:
            bad, _ = _problems(case)
            assert not bad, bad
            assert pl.last_launch_labels() == labels
            ms = pl.last_launch_ms()
            assert len(ms) == len(labels) and all(t > 0 for t in ms), ms
        finally:
            pl.set_profiling(False)
