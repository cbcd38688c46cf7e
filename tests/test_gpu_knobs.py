"""The non-default side of every A/B knob of plan_knobs.hpp that selects kernel code or launch arguments and that no
other test names: NTT_SHOUP_OUTER, NTT_XCD_ORDER, NTT_PASS1_FULL, NTT_ROWS, NTT_IPN, NTT_DREV_DIAG (NTT_INV_FORM, read
at every call, is tests/test_gpu_scan.py's).  DESIGN §7 reports timings of both sides of these switches; a timing of a
path that computes the wrong thing is not evidence.

Six of the knobs are read once per process and NTT_IPN at a plan's first in-place transform, so every setting runs in
a fresh child (tests/knob_child.py), one child at a time, each under its own time limit.  The child compares every
output with the C oracle, full vectors, bit for bit, forward and inverse, on a seeded random vector and on x_j = j, and
reports the launch labels.  Two assertions per setting: every case matched the oracle, and the labels show that the
knob took effect: where it changes the route they differ from the default child's as the table below says, where
it does not they equal them.  The default child's labels equal tests/golden/launch_routes.txt where the case is listed.
Nothing is compared between two GPU runs but labels.

The default child of the "in_place_batch" group is also the only test of a product path: an in-place plan takes the
separate tile-swap digit reversal (k_digitrev_swap) for every batch > 1, here through a three-pass BN254 plan (the
middle digits enter the swap) and through the P engine.

A size at which the route cannot be taken is moved to the nearest one that takes it:
  * BN254 in place 2^13 (NTT_XCD_ORDER=1): the library refuses that plan (no palindromic schedule,
    tests/test_gpu_inplace.py::test_in_place_rejected); 2^14 is the nearest in-place size whose grid is a multiple of
    8 tiles (2^12 has 4 tiles).
Engines: KIND_ROWS reaches 2^7 on the 256-bit engines and 2^6 on P, Goldilocks and BabyBear (rows_max_log), so the
NTT_ROWS=0 cases of the latter three stop at 2^6.

Time: the slowest default child takes 2.9 s on the MI355X (interpreter, torch and HIP start included; the eight
default children 1.9 to 2.9 s); LIMIT is five times that.  The whole file takes 49 s there: 19 children."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "knob_child.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_routes.txt")
LIMIT = 15  # seconds: 5 x the slowest default child (module docstring)
KNOBS = ("NTT_INV_FORM", "NTT_SHOUP_OUTER", "NTT_XCD_ORDER", "NTT_DREV_DIAG", "NTT_IPN", "NTT_PASS1_FULL", "NTT_ROWS")
ABNORMAL = (124, 134, 137, 139, -6, -11)  # time limit, abort, kill, segmentation fault

GROUPS = {
    "shoup": ["bn254L4/2^11", "bn254L4/2^13", "bn254L4/2^18", "bls381L4/2^11"],
    # grids of 8 tiles and more (the remap runs), in place too, and one of 2 tiles (it must fall through)
    "xcd": ["bn254L4/2^13", "bn254L4/2^18", "p469L1/2^16", "goldilocks/2^15", "babybear/2^16", "bn254L4/2^14/in_place",
            "bn254L4/2^18/in_place", "bn254L4/2^11"],
    "xcd_one_column": ["bn254L4/2^20"],  # the 4096-element tiles, one column per tile: the largest buffer, 32 MiB
    "pass1": ["goldilocks/2^13", "goldilocks/2^15", "goldilocks/2^18"],
    "rows_256": [f"{e}/2^{k}/rows" for e in ("bn254L4", "bls381L6") for k in (3, 5, 7)],
    "rows_small": [f"{e}/2^{k}/rows" for e in ("p469L1", "goldilocks", "babybear") for k in (3, 5, 6)],
    "in_place": ["bn254L4/2^12/in_place", "bn254L4/2^18/in_place", "p469L1/2^14/in_place"],
    "in_place_batch": ["bn254L4/2^16/in_place/batch2", "bn254L4/2^18/in_place/batch2", "p469L1/three_pass/in_place/batch2"],
}

# cases that tests/golden/launch_routes.txt must list (it lists others too: every listed case's default labels are
# compared with the recorded ones)
RECORDED = [f"bn254L4/2^{k}/{d}" for k in (11, 18) for d in ("forward", "inverse")] + ["bn254L4/2^20/forward"] + \
           [f"{c}/in_place/{d}" for c in ("bn254L4/2^12", "bn254L4/2^18", "p469L1/2^14") for d in ("forward", "inverse")]


# ---- what a setting does to the default labels (lists of labels)
def _same(labels):
    return labels


def _no_shoup(labels):
    return [re.sub(r"^(c\d+)s$", r"\1", x) for x in labels]


def _no_shoup_pass1(labels):
    return _no_shoup(labels[:1]) + labels[1:]


def _rows_off(labels):
    assert len(labels) == 1 and labels[0][0] == "r", ("the default is not KIND_ROWS", labels)
    return ["s" + labels[0][1:]]


def _ipn_off(labels):
    assert labels[-1][0] == "i", ("the default is not the fused in-place final pass", labels)
    return labels[:-1] + ["f" + labels[-1][1:], "d"]


def _swap_kept(labels):
    assert labels[-1] == "d" and labels[-2][0] == "f", ("the default does not take the tile swap", labels)
    return labels


# setting -> (environment, groups, rule, the labels expected outright where they are known: DESIGN §1.1, the golden)
SETTINGS = {
    "shoup_outer_0": ({"NTT_SHOUP_OUTER": "0"}, ["shoup"], _no_shoup,
                      {"bn254L4/2^11": "c6,f5", "bls381L4/2^11": "c6,f5", "bn254L4/2^18": "c6,c6,f6"}),
    "shoup_outer_1": ({"NTT_SHOUP_OUTER": "1"}, ["shoup"], _no_shoup_pass1,
                      {"bn254L4/2^11": "c6,f5", "bls381L4/2^11": "c6,f5", "bn254L4/2^18": "c6,c6s,f6"}),
    "xcd_order_1": ({"NTT_XCD_ORDER": "1"}, ["xcd"], _same, {}),
    "xcd_order_0": ({"NTT_XCD_ORDER": "0"}, ["xcd_one_column"], _same, {"bn254L4/2^20": "c10,f10"}),
    "xcd_order_3": ({"NTT_XCD_ORDER": "3"}, ["xcd_one_column"], _same, {"bn254L4/2^20": "c10,f10"}),
    "pass1_full_1": ({"NTT_PASS1_FULL": "1"}, ["pass1"], _same, {}),
    "rows_0": ({"NTT_ROWS": "0"}, ["rows_256", "rows_small"], _rows_off, {}),
    "ipn_0": ({"NTT_IPN": "0"}, ["in_place"], _ipn_off,
              {"bn254L4/2^12/in_place": "c6s,f6,d", "bn254L4/2^18/in_place": "c6,c6s,f6,d", "p469L1/2^14/in_place": "c7,f7,d"}),
    "ipn_0_drev_diag_0": ({"NTT_IPN": "0", "NTT_DREV_DIAG": "0"}, ["in_place"], _ipn_off,
                          {"bn254L4/2^12/in_place": "c6s,f6,d", "bn254L4/2^18/in_place": "c6,c6s,f6,d",
                           "p469L1/2^14/in_place": "c7,f7,d"}),
    "drev_diag_0": ({"NTT_DREV_DIAG": "0"}, ["in_place_batch"], _swap_kept, {}),
}

_CASUALTY = None  # the first child that ended abnormally: no child is started after it
_CONTROL = {}     # group -> the default child's lines, or the reason there are none


def _run_child(what, env_extra, cases):
    """{name/direction: (log_n, labels, digest, status)} of one child; fails the test where the child did not finish."""
    global _CASUALTY
    if _CASUALTY:
        pytest.fail(f"not started: the child of {_CASUALTY} ended abnormally before this one")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    try:
        r = subprocess.run([sys.executable, CHILD, *cases], env=env, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        _CASUALTY = f"{what} (time limit of {LIMIT} s)"
        pytest.fail(f"{_CASUALTY}: {(e.stdout or b'')[-2000:]!r}")
    if r.returncode in ABNORMAL:
        _CASUALTY = f"{what} (exit status {r.returncode})"
        pytest.fail(f"{_CASUALTY}: {r.stdout[-2000:]} {r.stderr[-2000:]}")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), (what, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    print(r.stdout)
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE\t"):
            _, name, log_n, labels, digest, status, _ = line.split("\t")
            out[name] = (log_n, labels, digest, status)
    assert sorted(out) == sorted(f"{c}/{d}" for c in cases for d in ("forward", "inverse")), (what, sorted(out))
    return out


def _assert_oracle(what, lines):
    bad = {k: v[3] for k, v in lines.items() if v[3] != "ok"}
    assert not bad, (what, bad)


def _control(group):
    if group not in _CONTROL:
        _CONTROL[group] = "its default child did not finish"
        _CONTROL[group] = _run_child(f"default/{group}", {}, GROUPS[group])
    if isinstance(_CONTROL[group], str):
        pytest.fail(f"group {group}: {_CONTROL[group]}")
    return _CONTROL[group]


def _golden():
    with open(GOLDEN) as f:
        return {r[0]: r[1] for r in (line.rstrip("\n").split("\t") for line in f if line.strip())}


@pytest.mark.parametrize("group", list(GROUPS))
def test_default_child_matches_the_oracle_and_the_recorded_routes(group):
    """No knob set: every case of the group equals the oracle, and its labels are the recorded ones where
    tests/golden/launch_routes.txt lists the case.  The routes the cases were chosen for are taken: three passes at
    Goldilocks 2^18 and on the three-pass in-place plans, "f, d" at batch 2 in place."""
    lines = _control(group)
    _assert_oracle(f"default/{group}", lines)
    golden = _golden()
    listed = {k: (v[1], golden[k]) for k, v in lines.items() if k in golden}
    assert all(a == b for a, b in listed.values()), listed
    assert not [k for k in RECORDED if k in lines and k not in listed], "a case chosen for its recorded route is not listed"
    labels = {k: v[1].split(",") for k, v in lines.items()}
    if group == "pass1":
        assert all(len(labels[f"goldilocks/2^18/{d}"]) == 3 for d in ("forward", "inverse")), labels
    if group == "in_place_batch":
        for k, v in labels.items():
            _swap_kept(v)
        for k in ("bn254L4/2^18/in_place/batch2/forward", "p469L1/three_pass/in_place/batch2/forward"):
            assert len(labels[k]) == 4, ("three passes and the swap", k, labels[k])
        assert int(lines["p469L1/three_pass/in_place/batch2/forward"][0]) <= 22


@pytest.mark.parametrize("setting,group", [(s, g) for s, v in SETTINGS.items() for g in v[1]])
def test_knob_setting(setting, group):
    """One setting on one group of cases in a fresh child: every case equals the oracle, and the labels are the
    default child's changed as the setting's rule says (and the ones stated outright in SETTINGS, where there are any)."""
    env, _, rule, stated = SETTINGS[setting]
    default = _control(group)
    lines = _run_child(f"{setting}/{group}", env, GROUPS[group])
    _assert_oracle(f"{setting}/{group}", lines)
    for k, (log_n, labels, _, _) in lines.items():
        assert log_n == default[k][0], (k, log_n, default[k][0])
        want = ",".join(rule(default[k][1].split(",")))
        assert labels == want, (setting, k, "got", labels, "want", want, "default", default[k][1])
        case = k.rsplit("/", 1)[0]
        if case in stated:
            assert labels == stated[case], (setting, k, labels, stated[case])
    if rule is not _same and rule is not _swap_kept:
        changed = [k for k in lines if lines[k][1] != default[k][1]]
        assert changed, (setting, "no label differs from the default's: the knob is not read")
    if setting == "shoup_outer_0":
        assert not [k for k, v in lines.items() if re.search(r"c\d+s", v[1])], "no label carries the s suffix"
    if setting == "shoup_outer_1":
        assert all(re.match(r"c\d+s", default[f"{c}/2^11/forward"][1]) for c in ("bn254L4", "bls381L4")), \
            "the default's pass 1 at 2^11 runs on Shoup pairs"
