"""Build tests/c/libf29probe.so (tests/c/field29_probe.hip: kernels that run one primitive of the
radix-2^29 engine per element and dump raw limbs) with hipcc, for tests/test_gpu_field29.py.  Built on
the CPU beside the product (__graft_entry__.build()); the .so travels to the GPU box."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "field29_probe.hip")
CSRC = os.path.join(ROOT, "ntt_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "libf29probe.so")


def _newest_source() -> float:
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))]
    return max(os.path.getmtime(f) for f in [SRC, *hdrs])


def build() -> str:
    if os.path.exists(OUT) and os.path.getmtime(OUT) >= _newest_source():
        return OUT
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    arch = os.environ.get("NTT_OFFLOAD_ARCH", "gfx950")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", f"--offload-arch={arch}", "-shared", "-fPIC", "-I", CSRC, SRC,
                        "-o", OUT + ".tmp"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {SRC}:\n{r.stderr[-4000:]}")
    os.replace(OUT + ".tmp", OUT)
    return OUT


if __name__ == "__main__":
    print(build())
