"""The child process of tests/test_gpu_knobs.py: runs the cases named on its command line in whatever NTT_*
environment the parent gave it and prints one line per case and direction,

    CASE <TAB> name/direction <TAB> log_n <TAB> launch labels <TAB> digest of the outputs <TAB> status <TAB> seconds

status is ``ok`` when every output equals the C oracle's (oracle/ntt_oracle.c through oracle_c, as
tests/test_gpu_parity.py binds it): full vectors, bit for bit, forward and inverse, on a seeded random vector whose
first element is p - 1 and on x_j = j, every transform of a batch on its own.  Nothing is compared with another GPU run.
A mismatch is reported in the status and the child goes on; ``DONE`` is the last line of a child that ran every case.

A case is ``engine/2^k[/in_place][/batchB | /rows]``: ``rows`` is a batch of four tiles' worth of transforms (the
shape KIND_ROWS takes); ``engine/three_pass/in_place/batchB`` is the smallest in-place plan of three passes that
ntt_plan_info reports up to 2^22 (the smallest in-place plan there is, where there is none; the log_n field says
which).  Knobs read once per process are why this is a process of its own."""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# engine -> (field id, 64-bit limbs, log2 of the tile: the largest single-pass transform)
ENGINES = {"bn254L4": (1, 4, 10), "bls381L4": (2, 4, 10), "bls381L6": (2, 6, 10), "p469L1": (0, 1, 13),
           "goldilocks": (3, 1, 12), "babybear": (4, 1, 13)}
THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8"))))


def parse(name):
    """(engine, log_n or None for three_pass, in_place, batch or 'rows')"""
    eng, size, *opts = name.split("/")
    log_n = None if size == "three_pass" else int(size[2:])
    batch = 1
    for o in opts:
        if o.startswith("batch"):
            batch = int(o[5:])
        elif o == "rows":
            batch = "rows"
        else:
            assert o == "in_place", name
    return eng, log_n, "in_place" in opts, batch


def make_plan(eng, log_n, in_place):
    """(plan, log_n); None where the library refuses every candidate."""
    from ntt_amd.lib import NTTError
    from ntt_amd.ntt import NTTPlan
    fid, L, _ = ENGINES[eng]
    if log_n is not None:
        try:
            return NTTPlan(fid, log_n, L, in_place=in_place), log_n
        except NTTError:
            return None, log_n
    smallest = None
    for lg in range(4, 23):
        try:
            pl = NTTPlan(fid, lg, L, in_place=in_place)
        except NTTError:
            continue
        if len(pl.passes) == 3:
            return pl, lg
        if smallest is None and len(pl.passes) >= 2:
            smallest = lg
        pl.close()
    return (NTTPlan(fid, smallest, L, in_place=in_place), smallest) if smallest is not None else (None, None)


def inputs(eng, n, batch, kind, seed):
    """[batch * n][L] uint64 limbs, canonical."""
    from ntt_amd.fields import field_params
    from oracle import oracle_c as OC
    fid, L, _ = ENGINES[eng]
    p, _ = field_params(fid)
    count = n * batch
    x = np.zeros((count, L), dtype=np.uint64)
    if kind == "iota":
        x[:, 0] = np.tile(np.arange(n, dtype=np.uint64), batch)
        return x
    if fid in (1, 2):
        x[:] = OC.random_limbs(fid, count, seed, L)
    elif fid == 0:
        x[:, 0] = OC.random_limbs(0, count, seed, 1)[:, 0]
    else:
        x[:, 0] = np.random.default_rng(seed).integers(0, p, size=count, dtype=np.uint64)
    x[0] = [((p - 1) >> (64 * i)) & (2**64 - 1) for i in range(L)]
    return x


def to_dev(x, pl):
    import torch
    if pl.elem32:
        host = x[:, 0].astype(np.uint32).view(np.int32)
    elif pl.limbs64 == 1:
        host = x[:, 0].copy().view(np.int64)
    else:
        host = np.ascontiguousarray(x).view(np.int64)
    return torch.from_numpy(host).to("cuda:0")


def to_host(t, L):
    a = t.cpu().numpy()
    a = a.view(np.uint32).astype(np.uint64) if a.dtype.itemsize == 4 else a.view(np.uint64)
    return a.reshape(-1, L)


def oracle(x, p, g, inverse):
    from oracle import oracle_c as OC
    if x.shape[0] >= 1 << 14:
        return OC.ntt_mp_par(x, p, g, THREADS, inverse)
    return OC.ntt_mp(x, p, g, inverse)


def run_case(name):
    from ntt_amd.fields import field_params
    eng, log_n, in_place, batch = parse(name)
    fid, L, tile = ENGINES[eng]
    p, g = field_params(fid)
    pl, log_n = make_plan(eng, log_n, in_place)
    for inverse in (False, True):
        t0 = time.time()
        direction = "inverse" if inverse else "forward"
        if pl is None:
            print(f"CASE\t{name}/{direction}\t{log_n}\t-\t-\trefused\t0.0", flush=True)
            continue
        n = pl.n
        b = 4 << (tile - log_n) if batch == "rows" else batch
        seen, bad, h = [], [], hashlib.sha256()
        for kind in ("random", "iota"):
            x = inputs(eng, n, b, kind, 7 + log_n)
            t = to_dev(x, pl)
            pl.set_profiling(True)
            if b == 1:
                (pl.inverse if inverse else pl.forward)(t)
            else:
                (pl.inverse_batch if inverse else pl.forward_batch)(t, b)
            labels = ",".join(pl.last_launch_labels()) or "-"
            pl.set_profiling(False)
            if labels not in seen:
                seen.append(labels)
            got = to_host(t, L)
            h.update(got.tobytes())
            for v in range(b):
                if not np.array_equal(got[v * n:(v + 1) * n], oracle(x[v * n:(v + 1) * n], p, g, inverse)):
                    bad.append(f"{kind}[{v}]")
        st = pl.device_status()
        status = "ok" if not bad and st == 0 else f"MISMATCH({' '.join(bad[:4])};{len(bad)};status={st:#x})"
        print(f"CASE\t{name}/{direction}\t{log_n}\t{'|'.join(seen)}\t{h.hexdigest()[:16]}\t{status}\t{time.time() - t0:.2f}",
              flush=True)
    if pl is not None:
        pl.close()


def main(names):
    for name in names:
        run_case(name)
    print("DONE", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
