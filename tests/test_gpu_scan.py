"""NTTPlan.batch_inverse and matrix_scan on the GPU, bit-exact against Python integers (tests/scan_ref.py) and never
against the kernels' own order of operations.  Plans of log_n 10; fields and extensions as the fold's EXTS, BabyBear
also as a Montgomery plan.  The scan shapes come from scan_info, on both sides of each decision: a thread's run, a
chunk, the narrow and the strip layout, a masked last strip.  Outputs land in the middle of poisoned, padded buffers
(tests/test_gpu_deep.py's); out-of-place inputs are compared with a clone afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import scan_ref as R
from tests import test_gpu_deep as D
from tests import test_gpu_fold as F
from tests import test_gpu_matrix as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "ntt_amd", "libntt_debug.so")

LOG_N = 10
EXTS = F.EXTS
OPS = ("sum", "product")
_ORACLE = {}


def _data(p, rows, cols, seed):
    """Seeded canonical values with the edge values 1, p - 1, p - 2 in front; the first is not zero, so that a
    product column does not vanish at row 0 (the zeros are placed by the cases that want them)."""
    x = T._rand(p, rows, cols, seed)
    x.reshape(-1)[0] = 2
    return x


def _oracle(fid, d, w, rows, width, op, seed):
    """(mat, inclusive, exclusive, totals), canonical, computed once per case."""
    key = (fid, d, rows, width, op, seed)
    if key not in _ORACLE:
        p, _ = T._params(fid)
        mat = _data(p, rows, width * d, seed)
        if width * d == 1:
            inc, exc, tot = R.scan_one_column([int(v) for v in mat[:, 0]], p, op)
            res = tuple(np.array(x, dtype=np.uint64).reshape(-1, 1) for x in (inc, exc)) + (np.array([tot], dtype=np.uint64),)
        else:
            res = tuple(x.astype(np.uint64) for x in R.scan(mat, width, d, w, p, op))
        _ORACLE[key] = (mat,) + res
    return _ORACLE[key]


def _scan(pl, mat_io, width, d, w, op, exclusive, with_totals=True, in_place=False, off=0):
    """One scan of mat_io (the plan's I/O form) into a poisoned buffer; returns (out, totals) as host arrays."""
    rows = mat_io.shape[0]
    n = rows * width * d
    if in_place:
        big, out = D._buf(pl, n, off)
        out.copy_(T._dev(mat_io, pl))
        src = out
    else:
        src = D._dev(mat_io, pl, off)
        keep = src.clone()
        big, out = D._buf(pl, n, off)
    tb, tot = D._buf(pl, width * d, off) if with_totals else (None, None)
    if off:
        assert out.data_ptr() % 16 != 0
    pl.matrix_scan(src, out, width, op=op, exclusive=exclusive, totals=tot, ext_degree=d, ext_w=w or 0, rows=rows)
    D._check_poison(pl, big, n, off)
    if with_totals:
        D._check_poison(pl, tb, width * d, off)
    if not in_place:
        assert torch.equal(src, keep), "the input was modified"
    return T._host(out, rows, width * d), (T._host(tot, 1, width * d)[0] if with_totals else None)


def _check(pl, fid, d, w, rows, width, op, seed=1, **kw):
    mat, inc, exc, tot = _oracle(fid, d, w, rows, width, op, seed)
    for exclusive in (False, True):
        got, gt = _scan(pl, D._to_io(mat, pl), width, d, w, op, exclusive, **kw)
        want = D._to_io(exc if exclusive else inc, pl)
        assert np.array_equal(got, want), (fid, d, rows, width, op, exclusive, kw)
        if gt is not None:
            assert np.array_equal(gt, D._to_io(tot, pl)), (fid, d, rows, width, op, exclusive, "totals")


def _row_counts(pl, d, op):
    """Width 1: 1, 2, 3; around a thread's run; around a chunk and past two of them, where chunks > 1."""
    _, run, _, _, _ = pl.scan_info(1, 1, op=op, ext_degree=d)
    _, _, cr, chunks, launches = pl.scan_info(1 << 16, 1, op=op, ext_degree=d)
    assert chunks > 1 and launches == 3
    rows = sorted({1, 2, 3, run - 1, run, run + 1, cr - 1, cr, cr + 1, 2 * cr + 5} - {0})
    for r in rows:  # chunk_rows as the call itself decides it at that count
        _, _, c2, n2, l2 = pl.scan_info(r, 1, op=op, ext_degree=d)
        assert (n2 > 1) == (r > cr) and l2 == (3 if n2 > 1 else 1) and (n2 == 1 or c2 == cr), (r, c2, n2)
    return rows


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("fid,d,w", EXTS)
def test_rows_at_width_one(fid, d, w, op):
    pl = T._plan(fid, LOG_N)
    rows = _row_counts(pl, d, op)
    assert rows[-1] > pl.n  # more rows than the plan's n: no table of the plan is used
    for r in rows:
        _check(pl, fid, d, w, r, 1, op, with_totals=r % 2 == 1)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("fid,d,w", [(4, 1, None), (4, 4, 11), (3, 1, None), (5, 4, 3)])
def test_widths_on_both_sides_of_the_layouts(fid, d, w, op):
    """Width 1, the width whose row is exactly 64 B, one less and one more; 37 and 300 at d = 1: rows that give at
    least two chunks and, at the wide shapes, a masked last strip."""
    pl = T._plan(fid, LOG_N)
    w64 = 64 // (d * pl.elem_bytes)
    for width in [1, w64 - 1, w64, w64 + 1] + ([37, 300] if d == 1 else []):
        tile = pl.scan_info(1, width, op=op, ext_degree=d)[2]
        rows = 2 * tile + 3
        strip, _, cr, chunks, launches = pl.scan_info(rows, width, op=op, ext_degree=d)
        assert chunks >= 2 and launches == 3, (width, rows, chunks)
        cols = width * (d if op == "sum" else 1)
        row_bytes = width * d * pl.elem_bytes
        if row_bytes >= 64:
            assert strip * (row_bytes // cols) >= 64 and strip & (strip - 1) == 0
            if width in (w64 + 1, 37, 300):
                assert cols % strip, "a masked last strip"
        else:
            assert strip == cols
        _check(pl, fid, d, w, rows, width, op)


@pytest.mark.parametrize("fid", [4, 3])
def test_the_most_chunks_within_2_18_rows(fid):
    """One base column of 2^18 - 3 rows: the largest chunk count reachable at that size."""
    pl = T._plan(fid, LOG_N)
    rows = (1 << 18) - 3
    for op in OPS:
        _, _, cr, chunks, _ = pl.scan_info(rows, 1, op=op)
        assert chunks == -(-rows // cr) and chunks >= 32
        mat, inc, exc, tot = _oracle(fid, 1, None, rows, 1, op, 3)
        got, gt = _scan(pl, mat, 1, 1, None, op, False)
        assert np.array_equal(got, inc) and int(gt[0]) == int(tot[0]), (fid, op)


@pytest.mark.parametrize("fid,d,w", [(4, 4, 11), (3, 2, 7), (4, 1, None)])
def test_special_columns(fid, d, w):
    p, _ = T._params(fid)
    pl = T._plan(fid, LOG_N)
    rows = 2 * pl.scan_info(1, 2, op="product", ext_degree=d)[2] + 9
    # all p - 1 under the sum, beside a column of ones
    mat = np.full((rows, 2 * d), p - 1, dtype=np.uint64)
    mat[:, d:] = 0
    mat[:, d] = 1
    got, tot = _scan(pl, mat, 2, d, w, "sum", False)
    steps = np.arange(1, rows + 1, dtype=object)
    assert np.array_equal(got[:, 0].astype(object), steps * (p - 1) % p) and np.array_equal(got[:, d].astype(object), steps % p)
    assert int(tot[0]) == rows * (p - 1) % p
    # a product column with a zero in the middle, beside a column of ones
    mat = _data(p, rows, 2 * d, 11)
    mat[:, d:] = 0
    mat[:, d] = 1
    z = rows // 2
    mat[z, :d] = 0
    _, inc, exc, _ = _oracle_of(mat, 2, d, w, p, "product")
    for exclusive, want in ((False, inc), (True, exc)):
        got, tot = _scan(pl, mat, 2, d, w, "product", exclusive)
        first_zero = z + 1 if exclusive else z
        assert not got[first_zero:, :d].any() and not tot[:d].any(), "every later row and the total are exactly 0"
        assert np.array_equal(got[:first_zero], want[:first_zero]), "the rows up to the zero are unaffected"
        assert np.array_equal(got[:, d:], np.tile(np.array([1] + [0] * (d - 1), dtype=np.uint64), (rows, 1))), "ones"


def _oracle_of(mat, width, d, w, p, op):
    return (mat,) + tuple(x.astype(np.uint64) for x in R.scan(mat, width, d, w, p, op))


def test_montgomery_plan_keeps_the_form():
    """BabyBear with NTT_PLAN_MONTGOMERY_IO: Montgomery-form data in and out; the exclusive product's row 0 is
    2^32 mod p."""
    fid, d, w = 4, 4, 11
    p, _ = T._params(fid)
    pl = T._plan(fid, LOG_N, montgomery_io=True)
    for width in (1, 5):
        rows = 2 * pl.scan_info(1, width, op="product", ext_degree=d)[2] + 1
        for op in OPS:
            _check(pl, fid, d, w, rows, width, op, seed=2)
    mat, _, _, _ = _oracle(fid, d, w, 7, 1, "product", 2)
    got, _ = _scan(pl, D._to_io(mat, pl), 1, d, w, "product", True)
    assert [int(v) for v in got[0]] == [(1 << 32) % p, 0, 0, 0]
    x = _data(p, 777, d, 4)
    x[5] = 0
    t = T._dev(D._to_io(x, pl), pl)
    out = T._host(pl.batch_inverse(t.clone(), ext_degree=d, ext_w=w), 777, d)
    rinv = pow(1 << 32, -1, p)
    assert R.is_inverse(x, (out.astype(object) * rinv % p).astype(np.uint64), d, w, p)


@pytest.mark.parametrize("fid,d,w", [(4, 4, 11), (3, 1, None), (4, 1, None)])
def test_in_place_unaligned_and_repeatable(fid, d, w):
    pl = T._plan(fid, LOG_N)
    for width in (1, 64 // (d * pl.elem_bytes) + 1):
        rows = 2 * pl.scan_info(1, width, op="product", ext_degree=d)[2] + 3
        for op in OPS:
            _check(pl, fid, d, w, rows, width, op, in_place=True)
            _check(pl, fid, d, w, rows, width, op, off=1)  # one element past a 16-byte boundary
            _check(pl, fid, d, w, rows, width, op, in_place=True, off=1)
            mat = _oracle(fid, d, w, rows, width, op, 1)[0]
            a = _scan(pl, mat, width, d, w, op, True)
            b = _scan(pl, mat, width, d, w, op, True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two runs differ"


def test_profiling_labels_the_launches():
    fid, d, w = 4, 4, 11
    pl = T._plan(fid, LOG_N)
    p, _ = T._params(fid)
    got = []
    for rows in (3, 2 * pl.scan_info(1, 1, op="product", ext_degree=d)[2] + 1):
        launches = pl.scan_info(rows, 1, op="product", ext_degree=d)[4]
        mat = T._dev(_data(p, rows, d, 8), pl)
        out, tot = T._poisoned(pl, rows * d), T._poisoned(pl, d)
        pl.set_profiling(True)
        pl.matrix_scan(mat, out, 1, op="product", totals=tot, ext_degree=d, ext_w=w)
        labels = pl.last_launch_labels()
        pl.set_profiling(False)
        assert len(labels) == launches
        got.append(labels)
    pl.set_profiling(True)
    pl.batch_inverse(T._dev(_data(p, 100, d, 9), pl), ext_degree=d, ext_w=w)
    got.append(pl.last_launch_labels())
    pl.set_profiling(False)
    assert got == [["y"], ["t", "k", "y"], ["v"]], got


# ------------------------------------------------------------------------------------------------ batch inverse
def _inverse(pl, x, d, w, in_place=False, off=0):
    n = x.shape[0] * d
    if in_place:
        big, out = D._buf(pl, n, off)
        out.copy_(T._dev(x, pl))
        pl.batch_inverse(out, ext_degree=d, ext_w=w or 0)
    else:
        src = D._dev(x, pl, off)
        keep = src.clone()
        big, out = D._buf(pl, n, off)
        pl.batch_inverse(src, out, ext_degree=d, ext_w=w or 0)
        assert torch.equal(src, keep), "the input was modified"
    D._check_poison(pl, big, n, off)
    return T._host(out, x.shape[0], d)


INV_FORMS = (None, 0, 1, 2)  # NTT_INV_FORM unset (the default form, 1) and every form by name


def _set_form(monkeypatch, form):
    """NTT_INV_FORM is read at every ntt_batch_inverse call: setting it in this process is enough."""
    if form is None:
        monkeypatch.delenv("NTT_INV_FORM", raising=False)
    else:
        monkeypatch.setenv("NTT_INV_FORM", str(form))


def _inv_run(pl, d, form):
    """A thread's run of elements at this form: InvShape::run_words(form) / (words per element * d), 32 words at
    form 1 (and unset), 16 at forms 0 and 2 (scan_shape.hpp)."""
    return (32 if form in (None, 1) else 16) // (pl.elem_bytes // 4 * d)


def _inv_counts(run):
    """1, 2, around a thread's run, around one wave's span (64 runs), a workgroup's worth + 1 (a second workgroup
    that holds one element) and + 3, 2^16 + 7."""
    return sorted({1, 2, run - 1, run, run + 1, 64 * run - 1, 64 * run, 64 * run + 1, 256 * run + 1, 256 * run + 3,
                   (1 << 16) + 7} - {0})


def _inv_input(p, count, run, d):
    """Seeded values with 1 and p - 1 and, where the count allows, the zero patterns: by thread run (the first
    position of the second run, the last of the third, a whole run) and by wave of 64 runs (lane 63's last element
    in wave 0, lane 0's first in wave 1, one whole lane of the otherwise non-zero wave 2, all of wave 3 beside the
    untouched wave 4, all of wave 5 but one element); for d > 1 an element whose coordinate 0 alone is zero, beside
    a zero element.  Returns (x, the positions to check element by element)."""
    x = _data(p, count, d, 20 + count % 97)
    x[count // 3] = 1
    x[count // 3, 1:] = 0
    x[count // 2] = p - 1
    wave = 64 * run
    if count > 4 * run:
        x[run] = 0                      # the first position of the second run
        x[3 * run - 1] = 0              # the last position of the third
        x[4 * run:5 * run] = 0          # a whole run
    if count >= wave:
        x[wave - 1] = 0                 # lane 63's last element
    if count > wave:
        x[wave] = 0                     # lane 0's first element of the next wave
    if count >= 3 * wave:
        lo = 2 * wave
        x[lo:lo + wave][~x[lo:lo + wave].any(axis=1)] = 3   # wave 2: nothing zero ...
        x[lo + 17 * run:lo + 18 * run] = 0                  # ... but lane 17's whole run
    if count >= 4 * wave:
        x[3 * wave:4 * wave] = 0        # every element of wave 3
        hi = min(count, 5 * wave)
        x[4 * wave:hi][~x[4 * wave:hi].any(axis=1)] = 3     # wave 4 (what the count has of it): nothing zero
    one = None
    if count >= 6 * wave:
        one = 5 * wave + 31 * run + min(1, run - 1)
        keep = x[one].copy()
        x[5 * wave:6 * wave] = 0        # wave 5: every element but one
        x[one] = keep if keep.any() else 3
    c0 = None
    if d > 1 and count >= 2:            # zero in coordinate 0 only: invertible
        c0 = wave + 1 if count > wave + 1 else (5 * run if count > 5 * run else count - 1)  # on no zero's place
        x[c0] = 5
        x[c0, 0] = 0
    zero = ~x.any(axis=1)
    edges = np.flatnonzero(zero[1:] != zero[:-1])  # a zero beside a non-zero: both sides
    pos = {0, count - 1} | {int(e) for e in edges} | {int(e) + 1 for e in edges}
    pos |= {q for q in (7, 8, 9, count // 3, count // 2, one, c0) if q is not None and q < count}
    if c0 is not None:
        pos |= {c0 - 1} | ({c0 + 1} if c0 + 1 < count else set())
    pos |= {int(q) for q in np.linspace(0, count - 1, 16).astype(np.int64)}  # at least 16 where the count has them
    assert len(pos) >= min(count, 16)
    return x, sorted(pos)


def _from_io(y, pl):
    """The plan's I/O form -> canonical values."""
    if not pl.montgomery_io:
        return y
    return (y.astype(object) * pow(1 << 32, -1, pl.p) % pl.p).astype(np.uint64)


def _inverse_sweep(pl, fid, d, w, form):
    """Every count and zero pattern of this form's run, in the three buffer forms: in * out = 1 and 0 -> 0 on all
    elements (is_inverse), and the oracle's own inverse element by element at the chosen positions."""
    p, _ = T._params(fid)
    run = _inv_run(pl, d, form)
    for count in _inv_counts(run):
        x, pos = _inv_input(p, count, run, d)
        want = {q: R.ext_inverse([int(v) for v in x[q]], w, p) for q in pos}
        for kw in ({}, {"in_place": True}, {"off": 1}):
            got = _from_io(_inverse(pl, D._to_io(x, pl), d, w, **kw), pl)
            assert R.is_inverse(x, got, d, w, p), (fid, d, form, count, kw)
            bad = [q for q in pos if [int(v) for v in got[q]] != want[q]]
            assert not bad, (fid, d, form, count, kw, bad[:8])
    return x, got


@pytest.mark.parametrize("form", INV_FORMS)
@pytest.mark.parametrize("fid,d,w", EXTS)
def test_batch_inverse(fid, d, w, form, monkeypatch):
    """in * out = 1 through the oracle's product and 0 -> 0 exactly, at every NTT_INV_FORM (unset too), the run taken
    from the form: counts 1, 2, around a thread's run, around a wave's span, a workgroup's worth + 1 and + 3 and
    2^16 + 7; random values, 1 and p - 1, a zero at the first and last position of a run and a whole run of zeros,
    the zero patterns by wave of _inv_input; in place and one element past a 16-byte boundary.  Bit-exact against
    tests/scan_ref.py alone: nothing is compared between forms."""
    _set_form(monkeypatch, form)
    p, _ = T._params(fid)
    pl = T._plan(fid, LOG_N)
    assert _inv_run(pl, d, None) == (32 if pl.elem32 else 16) // d  # 32 words of 4-byte, 16 of 8-byte elements (ntt.h)
    x, got = _inverse_sweep(pl, fid, d, w, form)
    for k in range(3):  # against the oracle's own inverse, element by element
        a = [int(v) for v in x[k + 7]]
        assert [int(v) for v in got[k + 7]] == R.ext_inverse(a, w, p)


@pytest.mark.parametrize("form", (0, 2))
def test_inverse_forms_on_the_montgomery_plan(form, monkeypatch):
    """The same sweep at forms 0 and 2 on BabyBear with NTT_PLAN_MONTGOMERY_IO (test_montgomery_plan_keeps_the_form
    runs form 1): Montgomery-form data in and out."""
    _set_form(monkeypatch, form)
    fid, d, w = 4, 4, 11
    pl = T._plan(fid, LOG_N, montgomery_io=True)
    _inverse_sweep(pl, fid, d, w, form)
    assert pl.device_status() == 0


# ------------------------------------------------------------------------------------------------ pipeline
def test_logup_running_sum():
    """LogUp on BabyBear, d = 4, N = 2^10: values a_i drawn from a table t with multiplicities m; denominators
    alpha - a_i and alpha - t_i by torch int64 arithmetic; one batch_inverse of the [2N][4] buffer; terms
    inv_a[i] - m_i inv_t[i]; the exclusive running sum with totals.  The total is zero and out[i + 1] - out[i] is
    term i; with one a_i moved off the table the total is nonzero."""
    fid, d, w = 4, 4, 11
    p, _ = T._params(fid)
    pl = T._plan(fid, LOG_N)
    N = pl.n
    rng = np.random.default_rng(77)
    table = np.unique(rng.integers(0, p, size=4 * N))[:N].astype(np.int64)  # N distinct values
    assert table.size == N
    alpha = torch.tensor([int(v) for v in rng.integers(1, p, size=d)], dtype=torch.int64, device="cuda:0")

    def total_of(idx, moved=None):
        a = torch.from_numpy(table[idx]).to("cuda:0")
        if moved is not None:
            a[moved] = (a[moved] + 1) % p  # the multiplicities below still count the old value
        m = torch.from_numpy(np.bincount(idx, minlength=N).astype(np.int64)).to("cuda:0")
        den = alpha.repeat(2 * N, 1)
        den[:, 0] = (den[:, 0] - torch.cat([a, torch.from_numpy(table).to("cuda:0")])) % p
        inv = pl.batch_inverse(den.to(torch.int32).reshape(-1).contiguous(), ext_degree=d, ext_w=w).to(torch.int64).reshape(2 * N, d)
        assert R.is_inverse(den.cpu().numpy().astype(np.uint64), inv.cpu().numpy().astype(np.uint64), d, w, p)
        terms = (inv[:N] - m[:, None] * inv[N:] % p) % p
        tin = terms.to(torch.int32).reshape(-1).contiguous()
        out, tot = T._poisoned(pl, N * d), T._poisoned(pl, d)
        pl.matrix_scan(tin, out, 1, op="sum", exclusive=True, totals=tot, ext_degree=d, ext_w=w)
        th, oh = T._host(tin, N, d), T._host(out, N, d)
        _, exc, want_tot = (x.astype(np.uint64) for x in R.scan(th, 1, d, w, p, "sum"))
        assert np.array_equal(oh, exc) and np.array_equal(T._host(tot, 1, d)[0], want_tot)
        diff = (oh[1:].astype(object) - oh[:-1].astype(object)) % p
        assert np.array_equal(diff.astype(np.uint64), th[:-1])
        return [int(v) for v in T._host(tot, 1, d)[0]]

    idx = rng.integers(0, N, size=N)
    assert total_of(idx) == [0] * d
    assert total_of(idx, moved=5) != [0] * d


# ------------------------------------------------------------------------------------------------ errors
def test_argument_errors_leave_the_buffers_untouched():
    import ctypes as C
    from ntt_amd import lib as Lb
    so = Lb.load()
    p, _ = T._params(4)
    d, w, W, rows = 4, 11, 3, 50
    pl = T._plan(4, LOG_N)
    tw = T._plan(4, LOG_N, twiddle_only=True)
    mat = T._dev(_data(p, rows, W * d, 1), pl)
    out, tot = T._poisoned(pl, rows * W * d), T._poisoned(pl, W * d)
    keeps = [t.clone() for t in (mat, out, tot)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    inv, scan, info = so.ntt_batch_inverse, so.ntt_matrix_scan, so.ntt_scan_info
    n = rows * W
    cases = [
        inv(pl._h, None, P(out), n, d, w, st), inv(pl._h, P(mat), None, n, d, w, st), inv(pl._h, P(mat), P(out), 0, d, w, st),
        inv(pl._h, P(mat), P(out), 1 << 30, d, w, st), inv(pl._h, P(mat), P(out), 1 << 32, 1, 0, st),
        inv(pl._h, P(mat), P(out), n, 3, w, st), inv(pl._h, P(mat), P(out), n, 0, w, st), inv(pl._h, P(mat), P(out), n, d, 0, st),
        inv(pl._h, P(mat), P(out), n, d, p, st), inv(pl._h, P(mat), P(mat, 16), n, d, w, st), inv(tw._h, P(mat), P(out), n, d, w, st),
        scan(pl._h, None, P(out), rows, W, d, w, 1, 0, P(tot), st), scan(pl._h, P(mat), None, rows, W, d, w, 1, 0, P(tot), st),
        scan(pl._h, P(mat), P(out), 0, W, d, w, 1, 0, P(tot), st), scan(pl._h, P(mat), P(out), rows, 0, d, w, 1, 0, P(tot), st),
        scan(pl._h, P(mat), P(out), 1 << 28, 4, d, w, 1, 0, P(tot), st), scan(pl._h, P(mat), P(out), rows, W, 3, w, 1, 0, P(tot), st),
        scan(pl._h, P(mat), P(out), rows, W, d, 0, 1, 0, P(tot), st), scan(pl._h, P(mat), P(out), rows, W, d, p, 1, 0, P(tot), st),
        scan(pl._h, P(mat), P(out), rows, W, d, w, 2, 0, P(tot), st), scan(pl._h, P(mat), P(out), rows, W, d, w, 1, 2, P(tot), st),
        scan(pl._h, P(mat), P(mat, 4), rows, W, d, w, 1, 0, P(tot), st), scan(pl._h, P(mat), P(out), rows, W, d, w, 1, 0, P(mat, 48), st),
        scan(pl._h, P(mat), P(out), rows, W, d, w, 0, 0, P(out), st), scan(tw._h, P(mat), P(out), rows, W, d, w, 1, 0, P(tot), st),
    ]
    assert cases == [Lb.NTT_ERR_ARG] * len(cases), cases
    v = [C.c_uint(9) for _ in range(5)]
    refs = [C.byref(x) for x in v]
    bad = [info(pl._h, 0, W, d, 1, *refs), info(pl._h, rows, 0, d, 1, *refs), info(pl._h, rows, W, 3, 1, *refs),
           info(pl._h, rows, W, d, 2, *refs), info(pl._h, 1 << 30, 1, d, 0, *refs), info(pl._h, rows, W, d, 1, None, *refs[1:])]
    assert bad == [Lb.NTT_ERR_ARG] * len(bad) and [x.value for x in v] == [9] * 5
    assert scan(pl._h, P(mat), P(out), rows, W, d, 0, 0, 0, None, st) == Lb.NTT_OK  # the sum does not read ext_w
    torch.cuda.synchronize()
    assert torch.equal(mat, keeps[0]) and torch.equal(tot, keeps[2]) and not torch.equal(out, keeps[1])


def test_29_bit_engines_refuse_the_calls():
    import ctypes as C
    from ntt_amd import lib as Lb
    from ntt_amd.ntt import NTTPlan
    so = Lb.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for pl, words in ((NTTPlan(1, 10, 4), 4), (NTTPlan(0, 10, 1), 1)):  # BN254, P469762049
        t = [torch.full((pl.n * words,), 1 + i, dtype=torch.int64, device="cuda:0") for i in range(2)]
        keep = [x.clone() for x in t]
        a, o = (C.c_void_p(x.data_ptr()) for x in t)
        v = [C.c_uint() for _ in range(5)]
        assert so.ntt_batch_inverse(pl._h, a, o, 16, 1, 0, st) == Lb.NTT_ERR_ARG
        assert so.ntt_matrix_scan(pl._h, a, o, 16, 1, 1, 0, 0, 0, None, st) == Lb.NTT_ERR_ARG
        assert so.ntt_scan_info(pl._h, 16, 1, 1, 0, *(C.byref(x) for x in v)) == Lb.NTT_ERR_ARG
        torch.cuda.synchronize()
        for x, k in zip(t, keep):
            assert torch.equal(x, k)


CHILD = r'''
import os
import sys
sys.path.insert(0, ROOT)
import numpy as np
from ntt_amd import lib as L
assert L.LIB_PATH.endswith("libntt_debug.so"), L.LIB_PATH
from tests import scan_ref as R
from tests import test_gpu_matrix as T
from tests import test_gpu_scan as S
for fid, d, w in ((3, 2, 7), (4, 4, 11)):
    p, _ = T._params(fid)
    pl = T._plan(fid, S.LOG_N)
    for width in (1, 64 // (d * pl.elem_bytes) + 1):
        rows = 2 * pl.scan_info(1, width, op="product", ext_degree=d)[2] + 3
        for op in S.OPS:
            S._check(pl, fid, d, w, rows, width, op)
    x = S._data(p, 3000, d, 5)
    x[17] = 0
    assert R.is_inverse(x, S._inverse(pl, x, d, w), d, w, p)
    st = pl.device_status()
    assert st == 0, (fid, hex(st))
    for form in (0, 2):  # NTT_INV_FORM is read at every call
        os.environ["NTT_INV_FORM"] = str(form)
        S._inverse_sweep(pl, fid, d, w, form)
        st = pl.device_status()
        assert st == 0, (fid, form, hex(st))
    del os.environ["NTT_INV_FORM"]
    bad = S._data(p, 100, d, 6)
    bad[37, d - 1] = p  # one non-canonical element
    S._scan(pl, bad, 1, d, w, "product", False)
    st = pl.device_status()
    assert st & 0x200 and not st & 0x100, (fid, "scan: non-canonical input", hex(st))
    S._inverse(pl, bad, d, w)
    st = pl.device_status()
    assert st & 0x200 and not st & 0x100, (fid, "inverse: non-canonical input", hex(st))
    assert pl.device_status() == 0
print("SCAN-DEBUG-OK")
'''


def test_checked_build_reports_clean_status():
    """Scans of both layouts and an inverse on both engines through the checked build in a fresh process: right
    results and no bounds / canonical report, the inverse's sweep at forms 0 and 2 included; an input with one element
    equal to p reports 0x200."""
    env = dict(os.environ, NTT_LIB_PATH=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "SCAN-DEBUG-OK" in r.stdout
