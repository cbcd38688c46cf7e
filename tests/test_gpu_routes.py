"""The launch route of every public call form, pinned: tools/record_routes.py's table against
tests/golden/launch_routes.txt.

Every fused route has a correct fallback (a coset forward that stops fusing runs scale + forward, a
low-degree extension that loses its first pass goes through the staging route, a polymul that stops
fusing runs pointwise + inverse), so the parity tests stay green while a call gains a launch and a
round trip through HBM.  This test fails instead: it compares, per case, the launch labels exactly as
the plan reports them (the Shoup ``s`` suffix included) and the number of recorded launches.

The golden is recorded with the tool from a build of the commit before a change to the host
scheduling (never from the changed tree).  The case list is the tool's: both read ``cases()``."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_routes.txt")


def _tool():
    spec = importlib.util.spec_from_file_location("record_routes", os.path.join(ROOT, "tools", "record_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    with open(GOLDEN) as f:
        rows = [line.rstrip("\n").split("\t") for line in f if line.strip()]
    assert all(len(r) == 3 for r in rows), "name<TAB>labels<TAB>launches per line"
    return {name: f"{labels}\t{count}" for name, labels, count in rows}, [r[0] for r in rows]


def test_golden_lists_the_tools_cases():
    """Without a GPU: the golden has one line for every case of the tool, in its order, no other."""
    _, names = _golden()
    assert names == [c[0] for c in _tool().cases()]


@pytest.mark.gpu
def test_launch_routes_match_the_recorded_table():
    T = _tool()
    want, _ = _golden()
    diffs = []
    for name, eng, log_n, flags, call in T.cases():
        got = T.route(eng, log_n, flags, call)
        print(f"{name}\t{got}")
        if got != want.get(name):
            diffs.append(f"{name}: got {got!r}, recorded {want.get(name)!r}")
    assert not diffs, "\n".join(diffs)
