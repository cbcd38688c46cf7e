"""Print the launch route of every public call form: which launches a call makes, in order.

    python tools/record_routes.py [-o tests/golden/launch_routes.txt]

One line per case: the case's name, ``last_launch_labels()`` joined with commas exactly as the plan
reports them (the Shoup ``s`` suffix kept; ``-`` when there is no labelled launch), and
``len(last_launch_ms())`` (unlabelled launches, such as the low-degree extension's scaling launch,
count there).  Each case creates its own plan through ``ntt_amd.ntt.NTTPlan``, turns profiling on,
makes one call and synchronises.  No ``NTT_*`` variable is set: the table is the default routing.

``tests/test_gpu_routes.py`` compares this table with ``tests/golden/launch_routes.txt``.  A call that
stops fusing still computes the right values through its fallback (scale + forward, the staged
low-degree extension, pointwise + inverse), so the parity tests cannot see it; this table does.  The
golden is recorded with this tool from a build of the commit BEFORE a change to the host scheduling,
never from the changed tree; the tool uses the public Python API only, so it runs there unchanged.

Sizes are the smallest at which a route can differ: one tile, twice that (two passes), and one
three-pass size on the 4-limb engine.  The four-step pieces are not here (tests/test_gpu_distributed.py,
tests/test_gpu_polymul_dist.py).
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _is_prime(n: int) -> bool:
    if n < 2:
        return False
    for q in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def ntt_prime(bits: int, two_adicity: int = 24):
    """The smallest prime k 2^v + 1 >= 2^(bits - 1) and a quadratic non-residue as its generator
    (tests/test_gpu_lde.py builds its custom moduli the same way)."""
    k = (1 << (bits - 1 - two_adicity)) + 1
    while not _is_prime(k * (1 << two_adicity) + 1):
        k += 2
    p = k * (1 << two_adicity) + 1
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return p, g


# engine name -> (NTTPlan arguments without log_n, sizes, has lde, has matrix / fold)
ENGINES = {
    "bn254L4": (dict(field_id=1, limbs64=4), (10, 11, 18), True, False),      # Eng256, tile 2^10
    "bls381L6": (dict(field_id=2, limbs64=6), (11,), True, False),            # Eng256w
    "p380L6": (dict(custom_bits=380, limbs64=6), (11,), True, False),         # Eng384
    "p469L1": (dict(field_id=0, limbs64=1), (13, 14), True, False),           # EngP, tile 2^13
    "goldilocks": (dict(field_id=3, limbs64=1), (12, 13), True, True),        # Eng64G, tile 2^12
    "babybear": (dict(field_id=4, limbs64=1), (13, 14), True, True),          # Eng31, tile 2^13
}
SHIFT = 7  # canonical and nonzero in every field above

# the calls made on every engine and size ("lde" / "mat": where the engine has them)
CALLS = [
    ("forward", None), ("inverse", None), ("forward_batch3", None), ("coset_forward", None),
    ("coset_inverse", None), ("lde", "lde"), ("lde_shift", "lde"), ("polymul", None),
    ("mat_forward_w3", "mat"), ("mat_forward_w40", "mat"), ("mat_inverse_w3", "mat"), ("mat_inverse_w40", "mat"),
    ("mat_lde_w3", "mat"), ("mat_lde_w40", "mat"), ("mat_forward_shift_w3", "mat"), ("mat_inverse_shift_w3", "mat"),
    ("mat_forward_bitrev_w3", "mat"), ("mat_inverse_bitrev_w3", "mat"), ("mat_lde_bitrev_w3", "mat"),
    ("fri_fold_arity4", "mat"),
]


def cases():
    """[(name, engine, log_n, plan flags, call)] in table order."""
    out = []
    for eng, (_, sizes, has_lde, has_mat) in ENGINES.items():
        for log_n in sizes:
            for call, needs in CALLS:
                if (needs == "lde" and not has_lde) or (needs == "mat" and not has_mat):
                    continue
                out.append((f"{eng}/2^{log_n}/{call}", eng, log_n, {}, call))
    ip, sl, mont = dict(in_place=True), dict(single_launch=True), dict(montgomery_io=True)
    # (2^11 has no palindromic schedule on the 1024-element tiles: the plan is refused; 2^12 is the
    # smallest two-pass size in place)
    for eng, log_n in (("bn254L4", 11), ("bn254L4", 12), ("bn254L4", 18), ("p469L1", 14)):
        for call in ("forward", "inverse"):
            out.append((f"{eng}/2^{log_n}/in_place/{call}", eng, log_n, ip, call))
    out.append(("bn254L4/2^11/montgomery_io/polymul", "bn254L4", 11, mont, "polymul"))
    for log_n in (18, 20):  # k_fused3 / k_fused3bi, then the second plan's k_fused2b / k_fused2bi
        out.append((f"bn254L4/2^{log_n}/single_launch/forward", "bn254L4", log_n, sl, "forward"))
        out.append((f"bn254L4/2^{log_n}/single_launch+in_place/forward", "bn254L4", log_n, dict(**sl, **ip), "forward"))
    # a default 2^20 plan: one vector on the second plan (4096-element tiles), a batch on its own
    out.append(("bn254L4/2^20/forward", "bn254L4", 20, {}, "forward"))
    out.append(("bn254L4/2^20/forward_batch2", "bn254L4", 20, {}, "forward_batch2"))
    return out


_PRIMES = {}


def make_plan(eng: str, log_n: int, flags: dict):
    from ntt_amd.ntt import NTTPlan
    kw = dict(ENGINES[eng][0])
    bits = kw.pop("custom_bits", None)
    if bits is not None:
        if bits not in _PRIMES:
            _PRIMES[bits] = ntt_prime(bits)
        kw["modulus"], kw["generator"] = _PRIMES[bits]
    return NTTPlan(log_n=log_n, **kw, **flags)


def _zeros(pl, count: int):
    """`count` zero elements in the plan's layout (zero is canonical in every field; routes do not
    depend on the values)."""
    import torch
    shape = (count,) if pl.limbs64 == 1 else (count, pl.limbs64)
    return torch.zeros(shape, dtype=pl.dtype, device=f"cuda:{pl.device}")


def run_call(pl, call: str) -> None:
    n = pl.n
    if call == "forward":
        pl.forward(_zeros(pl, n))
    elif call == "inverse":
        pl.inverse(_zeros(pl, n))
    elif call.startswith("forward_batch"):
        b = int(call[len("forward_batch"):])
        pl.forward_batch(_zeros(pl, b * n), b)
    elif call == "coset_forward":
        pl.forward_coset(_zeros(pl, n), SHIFT)
    elif call == "coset_inverse":
        pl.inverse_coset(_zeros(pl, n), SHIFT)
    elif call in ("lde", "lde_shift"):
        pl.lde_batch(_zeros(pl, n >> 1), _zeros(pl, n), 1, SHIFT if call == "lde_shift" else None)
    elif call == "polymul":
        pl.polymul(_zeros(pl, n), _zeros(pl, n), _zeros(pl, n))
    elif call.startswith("mat_"):
        kind, *opts = call[4:].split("_")
        w = int(opts[-1][1:])
        shift = SHIFT if "shift" in opts else None
        rev = "bitrev" in opts
        if kind == "forward":
            pl.forward_matrix(_zeros(pl, n * w), w, shift=shift, bitrev_out=rev)
        elif kind == "inverse":
            pl.inverse_matrix(_zeros(pl, n * w), w, shift=shift, bitrev_in=rev)
        else:
            pl.lde_matrix(_zeros(pl, (n >> 1) * w), _zeros(pl, n * w), 1, shift, w, bitrev_out=rev)
    elif call == "fri_fold_arity4":
        pl.fri_fold(_zeros(pl, n), _zeros(pl, n >> 2), 2, [3])
    else:
        raise ValueError(call)


def route(eng: str, log_n: int, flags: dict, call: str) -> str:
    """'labels<TAB>launches' of one call on a fresh plan; 'refused(status)<TAB>0' where the library
    refuses to create the plan (a size without a palindromic schedule in place), which is pinned too."""
    import torch
    from ntt_amd.lib import NTTError
    try:
        pl = make_plan(eng, log_n, flags)
    except NTTError as e:
        return f"refused({e.status})\t0"
    try:
        pl.set_profiling(True)
        run_call(pl, call)
        torch.cuda.synchronize()
        labels, ms = pl.last_launch_labels(), pl.last_launch_ms()
    finally:
        pl.close()
    return f"{','.join(labels) or '-'}\t{len(ms)}"


def table():
    """The table's lines, each as soon as its case has run."""
    for name, eng, log_n, flags, call in cases():
        yield f"{name}\t{route(eng, log_n, flags, call)}\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    text = ""
    for line in table():
        sys.stdout.write(line)
        sys.stdout.flush()
        text += line
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
