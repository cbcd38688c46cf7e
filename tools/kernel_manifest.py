"""One line per GPU kernel of libntt.so: what the compiler made of it, hashed.  No GPU needed.

    python tools/kernel_manifest.py [--src OTHER_TREE/ntt_amd/csrc] [--debug] [-o manifest.txt]

Every .hip unit of build.SOURCES is compiled with build.py's compile line, device side only, to
assembly (``--offload-device-only -S``).  For each kernel the manifest gives

    unit  mangled-name  sha256(instructions)  lds= scratch= kernarg= vgpr= sgpr= accum=

where the instructions are the text from the kernel's label to the end of the function without
comments, and the six figures come from its kernel descriptor (LDS bytes, scratch bytes, kernarg
bytes, next free VGPR, next free SGPR, accumulator offset).  Two trees whose manifests are equal
line for line run the same device code; a refactor of the headers is checked by

    python tools/kernel_manifest.py --src PARENT/ntt_amd/csrc -o a.txt
    python tools/kernel_manifest.py -o b.txt && cmp a.txt b.txt       (and again with --debug)

What is not kernel code is ignored: the per-unit ``__hip_cuid_*`` symbol (a hash of the source
path), ``.ident``, and the order in which a unit emits its kernels (the function ordinal inside
local labels such as ``.LBB12_3`` is dropped before hashing, and labels numbered through the unit
such as ``.Lpost_getpc7`` are numbered afresh in each kernel).  The tool hashes and compares; it looks
for no particular instruction.  Temporary files go to a directory of their own outside the tree.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ntt_amd import build as B  # noqa: E402

MAX_JOBS = 16
LOCAL_LABEL = re.compile(r"(\.L[A-Za-z_]+)\d+_(\d+)")  # .LBB12_3: function ordinal, then the block
UNIT_LABEL = re.compile(r"(\.L[A-Za-z_]*[A-Za-z])(\d+)\b")  # .Lpost_getpc7: a counter that runs through the unit
DESCRIPTOR = (("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"),
              ("kernarg", "kernarg_size"), ("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"),
              ("accum", "accum_offset"))


def assemble(src: str, csrc: str, include: str, out_dir: str, defines) -> str:
    """build.py's compile line for one unit, with `-c` replaced by device-only assembly output."""
    s = os.path.join(out_dir, src + ".s")
    cmd = [B.hipcc(), "-O3", "-std=c++17", f"--offload-arch={B.ARCH}", "-fPIC", "--offload-device-only", "-S",
           os.path.join(csrc, src), "-o", s, "-I", csrc, "-I", include, "-Wno-pass-failed",
           "-Wno-unused-command-line-argument", *defines]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr[-4000:]}")
    return s


def kernels(asm_path: str):
    """[(mangled name, instruction hash, {descriptor field: value})] of one assembly file."""
    lines = open(asm_path).read().splitlines()
    desc, cur = {}, None
    for line in lines:  # the descriptors first: they name the kernels (device functions have none)
        t = line.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = desc.setdefault(t.split()[1], {})
        elif t == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and t.startswith(".amdhsa_"):
            k, _, v = t[len(".amdhsa_"):].partition(" ")
            cur[k] = v.strip()
    out = []
    name, h, seen, in_desc = None, None, {}, False
    for line in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if name is None:
            if m and m.group(1) in desc:
                name, h, seen = m.group(1), hashlib.sha256(), {}
            continue
        t = line.split(";", 1)[0].strip()  # comment lines and trailing comments go
        if t.startswith(".Lfunc_end"):
            out.append((name, h.hexdigest(), desc[name]))
            name = None
            continue
        if t.startswith(".amdhsa_kernel"):
            in_desc = True
        if t == ".end_amdhsa_kernel":
            in_desc = False
            continue
        # labels and instructions count; the descriptor (reported field by field) and assembler
        # directives (.section, .p2align, ...) are no instruction text
        if not t or in_desc or (t.startswith(".") and not t.endswith(":")):
            continue
        # local labels carry the function's ordinal in the unit, or a count that runs through the unit:
        # the order in which a unit emits its kernels is no device code.  The ordinal is dropped, the
        # running labels are numbered afresh in each kernel.
        t = LOCAL_LABEL.sub(r"\1_\2", " ".join(t.split()))
        t = UNIT_LABEL.sub(lambda m: m.group(1) + str(seen.setdefault(m.group(0), len(seen))), t)
        h.update(t.encode() + b"\n")
    if name is not None or len(out) != len(desc):
        raise RuntimeError(f"{asm_path}: {len(desc)} kernel descriptors but {len(out)} kernel bodies")
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=B.CSRC, help="the csrc directory to compile (default: this tree's)")
    ap.add_argument("--debug", action="store_true", help="the checked build: -DNTT_DEBUG_CHECKS=1")
    ap.add_argument("--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 4))
    ap.add_argument("--units", nargs="*", default=None, help="only these units (default: every .hip of build.SOURCES)")
    ap.add_argument("-o", "--out", default="-")
    a = ap.parse_args()
    csrc = os.path.abspath(a.src)
    include = os.path.join(csrc, "..", "..", "include")
    include = os.path.abspath(include) if os.path.isdir(include) else B.INCLUDE
    units = a.units or [s for s in B.SOURCES if s.endswith(".hip")]
    defines = ["-DNTT_DEBUG_CHECKS=1"] if a.debug else []
    tmp = tempfile.mkdtemp(prefix="ntt_manifest_")
    try:
        with cf.ThreadPoolExecutor(max_workers=max(1, min(a.jobs, MAX_JOBS))) as ex:
            asms = list(ex.map(lambda s: assemble(s, csrc, include, tmp, defines), units))
        rows = []
        for unit, asm in zip(units, asms):
            for name, digest, d in kernels(asm):
                rows.append(" ".join([unit, name, digest] + [f"{k}={d.get(f, '?')}" for k, f in DESCRIPTOR]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = "".join(r + "\n" for r in sorted(rows))
    if a.out == "-":
        sys.stdout.write(text)
    else:
        with open(a.out, "w") as f:
            f.write(text)
    print(f"{len(rows)} kernels in {len(units)} units", file=sys.stderr)


if __name__ == "__main__":
    main()
