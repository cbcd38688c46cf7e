"""ntt_matrix_scan and ntt_batch_inverse run on the caller's stream and return before it has run: the held-stream
harness of tests/test_gpu_streams.py (see its module docstring) on the three-launch scan, whose plan-owned buffer
of chunk aggregates the warm-up leaves full of another call's values, and on the inverse, on Goldilocks and
BabyBear."""
import pytest

from tests import test_gpu_matrix as T
from tests import test_gpu_streams as H

pytestmark = pytest.mark.gpu

EXT = {"goldilocks": (3, 2, 7), "babybear": (4, 4, 11)}


def _cases(eng):
    fid, d, w = EXT[eng]
    pl = T._plan(fid, 10)
    tag = f"{eng} d={d}"
    cases = []
    for width, op in ((1, "sum"), (1, "product"), (64 // (d * pl.elem_bytes) + 1, "product")):
        rows = 2 * pl.scan_info(1, width, op=op, ext_degree=d)[2] + 3
        assert pl.scan_info(rows, width, op=op, ext_degree=d)[4] == 3  # three launches
        n = rows * width * d
        cases.append(H.Case(f"{tag} matrix_scan {op} {rows}x{width}", lambda seed, n=n: [H._rand(pl, n, seed)],
                            [H._spec(pl, n), H._spec(pl, width * d)],
                            lambda i, o, s, width=width, op=op, rows=rows: pl.matrix_scan(
                                i[0], o[0], width, op=op, exclusive=True, totals=o[1], ext_degree=d, ext_w=w, rows=rows,
                                stream=s), const=(0,)))
    n = 3000 * d
    cases.append(H.Case(f"{tag} batch_inverse", lambda seed: [H._rand(pl, n, seed)], [H._spec(pl, n)],
                        lambda i, o, s: pl.batch_inverse(i[0], o[0], ext_degree=d, ext_w=w, stream=s), const=(0,)))
    cases.append(H.Case(f"{tag} batch_inverse in place", lambda seed: [H._rand(pl, n, seed)], [],
                        lambda i, o, s: pl.batch_inverse(i[0], ext_degree=d, ext_w=w, stream=s)))
    return cases


@pytest.mark.parametrize("eng", list(EXT))
def test_scan_and_inverse_run_on_the_callers_stream(eng):
    H._need_sleep()
    H._run_all(_cases(eng))
