"""Host-side mirror of the reference's NTT entry points over libntt.so.

Reference interfaces mirrored (tie-pilot-qxw/NTT):

* ``SSIP(x, omega, log_n)``                      — ``src/GZKP-NTT.cu:1452`` (forward, in place,
  natural order, ``long long`` elements, P = 469762049, ``omega`` = the generator ``root`` = 3).
* ``NTT_GZKP(data, length, prime, omega, B, G)``  — ``src/big-num.cu:260`` (256-bit elements,
  ``cgbn_mem_t<256>`` layout, modulus-generic).  ``reverse``/``B``/``G`` are tuning inputs of the
  reference's non-self-sorting schedule and are accepted but unused.
* inverse                                         — ``src/GZKP-NTT.cu:1725-1732``.

Device data are torch tensors on a HIP device (PyTorch is plumbing here: device memory and
streams); every transform runs in the HIP kernels of libntt.so.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import lib as _L
from .fields import FIELDS, field_params

__all__ = ["NTTPlan", "SSIP", "NTT_GZKP", "lde_from_evals", "lde_matrix_from_evals", "to_device", "from_device", "FIELDS"]


def _stream_ptr(stream, device) -> C.c_void_p:
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return C.c_void_p(stream.cuda_stream)


def _u64_array(values: Sequence[int]):
    arr = (C.c_uint64 * len(values))(*[int(v) & ((1 << 64) - 1) for v in values])
    return arr


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def int_to_limbs(v: int, limbs64: int) -> List[int]:
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(limbs64)]


def host_array(values: Iterable[int], limbs64: int, elem32: bool = False) -> np.ndarray:
    """Python ints -> host array in the cgbn_mem_t layout: int64 bit patterns, [n, limbs64] ([n] for
    1 limb).  One-limb values go through uint64, so elements >= 2^63 (Goldilocks) keep their bits.
    ``elem32`` (one limb only): the 4-byte layout of NTT_PLAN_ELEM32 plans, int32 bit patterns of
    uint32 elements, [n]."""
    vals = list(values)
    if elem32:
        if limbs64 != 1:
            raise ValueError("4-byte elements are one limb")
        return np.array([int(v) & 0xFFFFFFFF for v in vals], dtype=np.uint32).view(np.int32)
    if limbs64 == 1:
        return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64).view(np.int64)
    host = np.zeros((len(vals), limbs64), dtype=np.uint64)
    for j, v in enumerate(vals):
        for i in range(limbs64):
            host[j, i] = (v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF
    return host.view(np.int64)


def host_ints(host: np.ndarray) -> List[int]:
    """Host array in the cgbn_mem_t layout (host_array) -> Python ints (unsigned).  An int32 / uint32
    array is the 4-byte layout (``host_array(..., elem32=True)``)."""
    if host.dtype.itemsize == 4:
        return [int(v) for v in host.view(np.uint32)]
    if host.ndim == 1:
        return [int(v) for v in host.view(np.uint64)]
    u = host.view(np.uint64)
    out = []
    for row in u:
        v = 0
        for i in range(len(row) - 1, -1, -1):
            v = (v << 64) | int(row[i])
        out.append(v)
    return out


def to_device(values: Iterable[int], limbs64: int, device="cuda", elem32: bool = False) -> torch.Tensor:
    """Python ints -> device tensor in the cgbn_mem_t layout (int64 [n, limbs64]; [n] for 1 limb;
    ``elem32``: int32 [n], the 4-byte layout of NTT_PLAN_ELEM32 plans)."""
    return torch.from_numpy(host_array(values, limbs64, elem32)).to(device)


def from_device(t: torch.Tensor) -> List[int]:
    """Device tensor (cgbn_mem_t layout, or int32: the 4-byte layout) -> Python ints."""
    return host_ints(t.detach().cpu().numpy())


BEALTO_FLAGS = {"bellperson": _L.NTT_PLAN_BELLPERSON, "v1": _L.NTT_PLAN_IMPROVED_V1, "v2": _L.NTT_PLAN_IMPROVED_V2,
                "v3": _L.NTT_PLAN_IMPROVED_V3, "v4": _L.NTT_PLAN_IMPROVED_V4}


class NTTPlan:
    """A cached transform plan: twiddle tables and scratch live on the device.

    ``field_id`` selects a built-in field (0 P469762049, 1 BN254 Fr, 2 BLS12-381 Fr, 3 Goldilocks
    with ``limbs64=1``: int64 bit patterns of uint64 elements); or pass
    ``modulus``/``generator`` ints for any odd prime below 2^(64*limbs64 - 1) with 2^log_n | p - 1
    (big-num.cu's modulus-generic path).  Fields 4 (BabyBear) and 5 (KoalaBear) with ``limbs64=1``,
    and custom one-limb plans with ``elem32=True`` (any odd prime below 2^31), work on 4-byte
    elements: contiguous ``torch.int32`` tensors of shape ``[batch * n]`` (uint32 bit patterns).
    """

    def __init__(self, field_id: int = 1, log_n: int = 10, limbs64: int = 4, device: int = 0,
                 modulus: Optional[int] = None, generator: Optional[int] = None, twiddle_only: bool = False,
                 montgomery_io: bool = False, stockham: bool = False, gzkp: bool = False,
                 in_place: bool = False, single_launch: bool = False, naive: bool = False,
                 no_swap: bool = False, bealto: str = "", elem32: bool = False):
        if bealto and bealto not in BEALTO_FLAGS:
            raise ValueError(f"bealto must be one of {sorted(BEALTO_FLAGS)}, not {bealto!r}")
        self._lib = _L.load()
        self.log_n = int(log_n)
        self.n = 1 << self.log_n
        self.limbs64 = int(limbs64)
        self.device = int(device)
        self.field_id = field_id if modulus is None else None
        if modulus is None:
            self.p, self.g = field_params(field_id)
        else:
            self.p, self.g = int(modulus), int(generator)
        h = C.c_void_p()
        flags = (_L.NTT_PLAN_TWIDDLE_ONLY if twiddle_only else 0) | (_L.NTT_PLAN_MONTGOMERY_IO if montgomery_io else 0)
        # stockham: forward transforms on the reference's bellperson-family rival schedule (ntt.h)
        flags |= _L.NTT_PLAN_STOCKHAM if stockham else 0
        # gzkp: the reference's GZKP(B, G) rival schedule (bit reversal + in-place DIT passes)
        flags |= _L.NTT_PLAN_GZKP if gzkp else 0
        # naive: the reference's `naive` rival (bit reversal + one radix-2 round per launch)
        flags |= _L.NTT_PLAN_NAIVE if naive else 0
        # no_swap: the reference's `naive_no_swap` rival (radix-2 Stockham autosort, one round per launch)
        flags |= _L.NTT_PLAN_NO_SWAP if no_swap else 0
        # bealto: the reference's radix-2^deg group-FFT rivals -- "bellperson" (bellperson_baseline /
        # FIELD_radix_fft_revised) or "v1".."v4" (improved_NTT_v1..v4), one k_bealto launch per round
        flags |= BEALTO_FLAGS[bealto] if bealto else 0
        # in_place: no plan scratch, palindromic passes + tile-swap digit reversal (the reference's
        # self-sort-in-place property, GZKP-NTT.cu:1359-1449; ntt.h NTT_PLAN_IN_PLACE)
        flags |= _L.NTT_PLAN_IN_PLACE if in_place else 0
        # single_launch: 3-pass transforms as one persistent launch (BASELINE config 2's single kernel)
        flags |= _L.NTT_PLAN_SINGLE_LAUNCH if single_launch else 0
        # elem32: 4-byte elements (ntt.h NTT_PLAN_ELEM32; implied by the BabyBear / KoalaBear fields)
        flags |= _L.NTT_PLAN_ELEM32 if elem32 else 0
        self.montgomery_io = bool(montgomery_io)
        if modulus is None:
            st = self._lib.ntt_plan_create_ex(C.byref(h), int(field_id), self.log_n, self.limbs64, self.device, flags)
        else:
            st = self._lib.ntt_plan_create_custom_ex(C.byref(h), _u64_array(int_to_limbs(self.p, self.limbs64)),
                                                     _u64_array(int_to_limbs(self.g, self.limbs64)), self.limbs64,
                                                     self.log_n, self.device, flags)
        _L.check(st, "ntt_plan_create")
        self._h = h
        n = C.c_uint64()
        eb = C.c_uint()
        npass = C.c_uint()
        radix = (C.c_uint * 8)()
        _L.check(self._lib.ntt_plan_info(h, C.byref(n), C.byref(eb), C.byref(npass), radix), "ntt_plan_info")
        self.elem_bytes = eb.value
        self.elem32 = self.elem_bytes == 4
        self.dtype = torch.int32 if self.elem32 else torch.int64  # the tensors the plan takes
        self.passes = [radix[i] for i in range(npass.value)]

    # -------------------------------------------------------------------------------- memory
    def empty(self, batch: int = 1) -> torch.Tensor:
        shape = (batch * self.n,) if self.limbs64 == 1 else (batch * self.n, self.limbs64)
        return torch.empty(shape, dtype=self.dtype, device=f"cuda:{self.device}")

    def _check_tensor(self, t: torch.Tensor, batch: int = 1, what: str = "NTT data", count: Optional[int] = None) -> None:
        """``t`` holds ``count`` elements (default: ``batch`` vectors of the plan's size) on the plan's device."""
        count = batch * self.n if count is None else count
        if not t.is_cuda:
            raise ValueError(f"{what} must be a device (HIP) tensor")
        self._check_layout(t, what)
        if t.numel() * t.element_size() != count * self.elem_bytes:
            raise ValueError(f"{what}: expected {count} elements of {self.elem_bytes} bytes")
        if t.device.index != self.device:
            raise ValueError(f"{what} on {t.device}, plan on cuda:{self.device}")

    # -------------------------------------------------------------------------------- argument checks
    # Shared by the calls below.  Each raises ValueError; the calls check scalars first, then shapes and overlap,
    # and whether a tensor is on the plan's device last.
    def _check_layout(self, t, what: str) -> None:
        if not isinstance(t, torch.Tensor) or not t.is_contiguous() or t.dtype != self.dtype:
            raise ValueError(f"{what} must be a contiguous {'int32' if self.elem32 else 'int64'} tensor in the plan's "
                             "element layout")

    def _check_device(self, *named) -> None:
        """``named`` = (tensor or None, name) pairs: every tensor is on the plan's device."""
        for t, what in named:
            if t is None:
                continue
            if not t.is_cuda:
                raise ValueError(f"{what} must be a device (HIP) tensor")
            if t.device.index != self.device:
                raise ValueError(f"{what} on {t.device}, plan on cuda:{self.device}")

    def _check_log_rows(self, log_rows, lowest=0, lowest_name: str = "0") -> int:
        """``log_rows`` (None: the plan's log_n) is an integer in [lowest, log_n].  Returns it."""
        if log_rows is None:
            log_rows = self.log_n
        if not _is_int(log_rows) or not lowest <= log_rows <= self.log_n:
            raise ValueError(f"log_rows must be an integer in [{lowest_name}, {self.log_n}], not {log_rows!r}")
        return log_rows

    def _check_shape(self, width, log_rows: int) -> None:
        """A positive integer width with every element index of [2^log_rows][width] below 2^32."""
        if not _is_int(width) or width < 1:
            raise ValueError(f"width must be a positive integer, not {width!r}")
        if (width << log_rows) >= 1 << 32:
            raise ValueError(f"2^log_rows * width must stay below 2^32, not {1 << log_rows} * {width}")

    def _check_matrix(self, t: torch.Tensor, rows: int, width: int, what: str, log_bound: Optional[int] = None) -> None:
        """``t`` = [rows][width] in the plan's layout; the width is bounded at 2^log_bound rows (None: the plan's n)."""
        self._check_shape(width, self.log_n if log_bound is None else log_bound)
        self._check_layout(t, what)
        if t.numel() * t.element_size() != rows * width * self.elem_bytes:
            raise ValueError(f"{what}: expected {rows} rows of {width} elements of {self.elem_bytes} bytes")

    def _check_shift(self, shift) -> None:
        if shift is not None and (not _is_int(shift) or not 0 < shift < self.p):
            raise ValueError(f"shift must be None or a canonical nonzero integer (0 < shift < p), not {shift!r}")

    def _check_ext(self, ext_degree, ext_w, reads_w: bool = True) -> None:
        if not _is_int(ext_degree) or ext_degree not in (1, 2, 4):
            raise ValueError(f"ext_degree must be 1, 2 or 4, not {ext_degree!r}")
        if reads_w and ext_degree > 1 and (not _is_int(ext_w) or not 0 < ext_w < self.p):
            raise ValueError(f"ext_w must be a canonical nonzero integer (0 < ext_w < p), not {ext_w!r}")

    def _canonical_words(self, name: str, value, count: int) -> List[int]:
        """``value`` as a list: a sequence of ``count`` canonical ints."""
        try:
            vals = list(value)
        except TypeError:
            raise ValueError(f"{name} must be a sequence of {count} integers, not {value!r}") from None
        if isinstance(value, str) or len(vals) != count or not all(_is_int(v) and 0 <= v < self.p for v in vals):
            raise ValueError(f"{name} must be {count} canonical integers (0 <= {name}[j] < p), not {value!r}")
        return vals

    @staticmethod
    def _check_no_overlap(out, out_name, out_bytes, inputs, same_ok: bool = False) -> None:
        """``out`` shares no byte with any of ``inputs`` = ((tensor, name, bytes), ..); ``same_ok``: unless it is
        the same buffer."""
        b0 = out.data_ptr()
        for t, name, nbytes in inputs:
            a0 = t.data_ptr()
            if a0 < b0 + out_bytes and b0 < a0 + nbytes and not (same_ok and a0 == b0):
                raise ValueError(f"{name} and {out_name} overlap"
                                 + (" (they may be the same buffer, or apart)" if same_ok else ""))

    def _shift_arg(self, shift: Optional[int], limbs64: Optional[int] = None):
        """The ``shift`` pointer of a C call: null, or the shift as ``limbs64`` words (None: the plan's)."""
        return None if shift is None else _u64_array(int_to_limbs(int(shift), self.limbs64 if limbs64 is None else limbs64))

    # -------------------------------------------------------------------------------- transforms
    def forward(self, t: torch.Tensor, stream=None) -> torch.Tensor:
        self._check_tensor(t)
        _L.check(self._lib.ntt_forward(self._h, _ptr(t), _stream_ptr(stream, t.device)),
                 "ntt_forward")
        return t

    def inverse(self, t: torch.Tensor, stream=None) -> torch.Tensor:
        self._check_tensor(t)
        _L.check(self._lib.ntt_inverse(self._h, _ptr(t), _stream_ptr(stream, t.device)),
                 "ntt_inverse")
        return t

    def device_status(self) -> int:
        """ntt_plan_device_status: bit 0 = a watchdog gave up (single launch / fused in-place digit
        reversal; until this clears it, every call on the plan raises NTTError NTT_ERR_DEVICE); with
        the checked build (libntt_debug.so) 0x100 bounds, 0x200 non-canonical input, 0x400 lazy bound,
        0x800 non-canonical output.  Blocking (synchronises the device); clears the report."""
        v = C.c_uint()
        _L.check(self._lib.ntt_plan_device_status(self._h, C.byref(v)), "ntt_plan_device_status")
        return v.value

    def set_watchdog(self, spins: int = 1 << 21) -> None:
        """ntt_plan_set_watchdog: poll limit of the plan's inter-workgroup waits (0 = give up at once,
        a test hook for the NTT_ERR_DEVICE path)."""
        _L.check(self._lib.ntt_plan_set_watchdog(self._h, int(spins)), "ntt_plan_set_watchdog")

    def count_noncanonical(self, t: torch.Tensor, stream=None) -> int:
        """Number of elements of t that are not < p (the transforms' input contract); blocking."""
        if t.device.type != "cuda" or not t.is_contiguous() or t.dtype != self.dtype:
            raise ValueError("expected a contiguous device tensor in the plan's element layout")
        count = t.numel() if self.limbs64 == 1 else t.numel() // self.limbs64
        bad = C.c_uint64()
        _L.check(self._lib.ntt_count_noncanonical(self._h, _ptr(t), count, C.byref(bad),
                                                  _stream_ptr(stream, t.device)), "ntt_count_noncanonical")
        return bad.value

    def forward_batch(self, t: torch.Tensor, batch: int, stream=None) -> torch.Tensor:
        self._check_tensor(t, batch)
        _L.check(self._lib.ntt_forward_batch(self._h, _ptr(t), int(batch),
                                             _stream_ptr(stream, t.device)), "ntt_forward_batch")
        return t

    def inverse_batch(self, t: torch.Tensor, batch: int, stream=None) -> torch.Tensor:
        self._check_tensor(t, batch)
        _L.check(self._lib.ntt_inverse_batch(self._h, _ptr(t), int(batch),
                                             _stream_ptr(stream, t.device)), "ntt_inverse_batch")
        return t

    def forward_coset(self, t: torch.Tensor, shift: int, stream=None) -> torch.Tensor:
        """Evaluations on the coset shift*<w>: X_k = sum_j x_j (shift w^k)^j, one vector of the plan's
        size in place (no padding, no batch: ``lde_batch`` is the low-degree extension)."""
        self._check_tensor(t)
        _L.check(self._lib.ntt_forward_coset(self._h, _ptr(t),
                                             _u64_array(int_to_limbs(int(shift), self.limbs64)),
                                             _stream_ptr(stream, t.device)), "ntt_forward_coset")
        return t

    def inverse_coset(self, t: torch.Tensor, shift: int, stream=None) -> torch.Tensor:
        """Interpolation from the coset shift*<w>: x_j = shift^-j INTT(X)_j."""
        self._check_tensor(t)
        _L.check(self._lib.ntt_inverse_coset(self._h, _ptr(t),
                                             _u64_array(int_to_limbs(int(shift), self.limbs64)),
                                             _stream_ptr(stream, t.device)), "ntt_inverse_coset")
        return t

    def _check_lde(self, coeffs: torch.Tensor, out: torch.Tensor, log_blowup: int, shift: Optional[int],
                   batch: int) -> None:
        if not isinstance(log_blowup, int) or not 0 <= log_blowup <= self.log_n:
            raise ValueError(f"log_blowup must be an integer in [0, {self.log_n}], not {log_blowup!r}")
        if not isinstance(batch, int) or batch < 1:
            raise ValueError(f"batch must be a positive integer, not {batch!r}")
        if shift is not None and not 0 < int(shift) < self.p:
            raise ValueError("shift must be canonical and nonzero (0 < shift < p)")
        n_in = self.n >> log_blowup
        self._check_tensor(coeffs, what="coeffs", count=batch * n_in)
        self._check_tensor(out, what="out", count=batch * self.n)
        self._check_no_overlap(out, "out", batch * self.n * self.elem_bytes,
                               ((coeffs, "coeffs", batch * n_in * self.elem_bytes),))

    def lde_batch(self, coeffs: torch.Tensor, out: torch.Tensor, log_blowup: int, shift: Optional[int] = None,
                  batch: int = 1, stream=None) -> torch.Tensor:
        """Low-degree extension (ntt_lde_batch).  This plan has the LARGE size N = 2^log_n; ``coeffs``
        holds ``batch`` polynomials of n = N >> log_blowup coefficients back to back, ``out`` receives
        ``batch`` vectors of N evaluations: out[v][k] = sum_j coeffs[v][j] (shift w_N^k)^j (shift None: 1).
        ``coeffs`` is not modified and must not overlap ``out``."""
        self._check_lde(coeffs, out, log_blowup, shift, batch)
        _L.check(self._lib.ntt_lde_batch(self._h, _ptr(coeffs), _ptr(out), int(log_blowup), self._shift_arg(shift),
                                         int(batch), _stream_ptr(stream, out.device)), "ntt_lde_batch")
        return out

    # -------------------------------------------------------------------------------- row-major matrices
    def _check_matrix_ex(self, shift, flag, flag_name: str) -> None:
        """The keyword options of the matrix calls: a canonical nonzero integer shift (or None), a bool flag."""
        self._check_shift(shift)
        if not isinstance(flag, bool):
            raise ValueError(f"{flag_name} must be a bool, not {flag!r}")

    def forward_matrix(self, t: torch.Tensor, width: int, stream=None, *, shift: Optional[int] = None,
                       bitrev_out: bool = False) -> torch.Tensor:
        """Forward NTT of every column of the row-major matrix ``t`` = [n][width] in place
        (ntt_forward_matrix): element (j, b) at ``t.view(-1)[j * width + b]``.  ``shift`` = c evaluates on
        the coset c<w_n> instead: out[k][b] = sum_j t[j][b] (c w_n^k)^j; ``bitrev_out`` stores row k of the
        result at row bitrev(k) (ntt_forward_matrix_ex)."""
        self._check_matrix_ex(shift, bitrev_out, "bitrev_out")
        self._check_matrix(t, self.n, width, "t")
        self._check_device((t, "t"))
        if shift is None and not bitrev_out:
            _L.check(self._lib.ntt_forward_matrix(self._h, _ptr(t), int(width),
                                                  _stream_ptr(stream, t.device)), "ntt_forward_matrix")
            return t
        _L.check(self._lib.ntt_forward_matrix_ex(self._h, _ptr(t), int(width), self._shift_arg(shift),
                                                 _L.NTT_MATRIX_BITREV_OUT if bitrev_out else 0,
                                                 _stream_ptr(stream, t.device)), "ntt_forward_matrix_ex")
        return t

    def inverse_matrix(self, t: torch.Tensor, width: int, stream=None, *, shift: Optional[int] = None,
                       bitrev_in: bool = False) -> torch.Tensor:
        """Inverse NTT (1/n included) of every column of the row-major matrix ``t`` = [n][width] in place.
        ``shift`` = c interpolates from the coset c<w_n>: out[j][b] = c^-j INTT(column b)_j; ``bitrev_in``:
        row i of ``t`` holds the evaluation of natural index bitrev(i) (ntt_inverse_matrix_ex)."""
        self._check_matrix_ex(shift, bitrev_in, "bitrev_in")
        self._check_matrix(t, self.n, width, "t")
        self._check_device((t, "t"))
        if shift is None and not bitrev_in:
            _L.check(self._lib.ntt_inverse_matrix(self._h, _ptr(t), int(width),
                                                  _stream_ptr(stream, t.device)), "ntt_inverse_matrix")
            return t
        _L.check(self._lib.ntt_inverse_matrix_ex(self._h, _ptr(t), int(width), self._shift_arg(shift),
                                                 _L.NTT_MATRIX_BITREV_IN if bitrev_in else 0,
                                                 _stream_ptr(stream, t.device)), "ntt_inverse_matrix_ex")
        return t

    def _check_lde_matrix(self, coeffs: torch.Tensor, out: torch.Tensor, log_blowup: int, shift: Optional[int],
                          width: int) -> None:
        if not isinstance(log_blowup, int) or not 0 <= log_blowup <= self.log_n:
            raise ValueError(f"log_blowup must be an integer in [0, {self.log_n}], not {log_blowup!r}")
        if shift is not None and not 0 < int(shift) < self.p:
            raise ValueError("shift must be canonical and nonzero (0 < shift < p)")
        n_in = self.n >> log_blowup
        self._check_matrix(coeffs, n_in, width, "coeffs")
        self._check_matrix(out, self.n, width, "out")
        self._check_no_overlap(out, "out", self.n * width * self.elem_bytes,
                               ((coeffs, "coeffs", n_in * width * self.elem_bytes),))
        self._check_device((coeffs, "coeffs"), (out, "out"))

    def lde_matrix(self, coeffs: torch.Tensor, out: torch.Tensor, log_blowup: int, shift: Optional[int] = None,
                   width: int = 1, stream=None, *, bitrev_out: bool = False) -> torch.Tensor:
        """Low-degree extension of the columns of a row-major matrix (ntt_lde_matrix).  This plan has the
        LARGE size N = 2^log_n; ``coeffs`` = [N >> log_blowup][width] holds one polynomial per column,
        ``out`` = [N][width] receives out[k][b] = sum_j coeffs[j][b] (shift w_N^k)^j (shift None: 1).
        ``coeffs`` is not modified and must not overlap ``out``.  ``bitrev_out`` stores row k of the result
        at row bitrev(k), the reversal over this plan's log_n bits (ntt_lde_matrix_ex)."""
        if not isinstance(bitrev_out, bool):
            raise ValueError(f"bitrev_out must be a bool, not {bitrev_out!r}")
        self._check_lde_matrix(coeffs, out, log_blowup, shift, width)
        if bitrev_out:
            _L.check(self._lib.ntt_lde_matrix_ex(self._h, _ptr(coeffs), _ptr(out), int(log_blowup),
                                                 self._shift_arg(shift), int(width), _L.NTT_MATRIX_BITREV_OUT,
                                                 _stream_ptr(stream, out.device)), "ntt_lde_matrix_ex")
            return out
        _L.check(self._lib.ntt_lde_matrix(self._h, _ptr(coeffs), _ptr(out), int(log_blowup), self._shift_arg(shift),
                                          int(width), _stream_ptr(stream, out.device)), "ntt_lde_matrix")
        return out

    def fri_fold(self, evals: torch.Tensor, out: torch.Tensor, log_arity: int, beta: Sequence[int], *,
                 ext_degree: int = 1, ext_w: int = 0, shift: Optional[int] = None, log_rows: Optional[int] = None,
                 stream=None) -> torch.Tensor:
        """One FRI fold of arity 2^log_arity (ntt_fri_fold).  ``evals`` = [N = 2^log_rows][ext_degree] holds
        the evaluations of a polynomial f with coefficients in F_p[X]/(X^ext_degree - ext_w) on the coset
        shift*<w_N> with the rows in bit-reversed order, as ``lde_matrix(..., width=ext_degree,
        bitrev_out=True)`` stores them; ``out`` = [N >> log_arity][ext_degree] receives, in the same order one
        level down, the evaluations on shift^(2^log_arity)*<w_M> of g = sum_t beta^t f_t, where
        f(x) = sum_t x^t f_t(x^(2^log_arity)).  ``beta`` is ``ext_degree`` canonical ints; ``log_rows``
        defaults to the plan's log_n and may be smaller (one plan serves every later layer).  ``evals`` is not
        modified and must not overlap ``out``; ``fields.EXTENSIONS`` has the usual (ext_degree, ext_w)."""
        if not _is_int(log_arity) or not 1 <= log_arity <= 4:
            raise ValueError(f"log_arity must be an integer in [1, 4], not {log_arity!r}")
        log_rows = self._check_log_rows(log_rows, log_arity, "log_arity")
        self._check_ext(ext_degree, ext_w)
        beta = self._canonical_words("beta", beta, ext_degree)
        self._check_shift(shift)
        rows, rows_out, eb = 1 << log_rows, 1 << (log_rows - log_arity), self.elem_bytes
        self._check_matrix(evals, rows, ext_degree, "evals")
        self._check_matrix(out, rows_out, ext_degree, "out")
        self._check_no_overlap(out, "out", rows_out * ext_degree * eb, ((evals, "evals", rows * ext_degree * eb),))
        self._check_device((evals, "evals"), (out, "out"))
        _L.check(self._lib.ntt_fri_fold(self._h, _ptr(evals), _ptr(out), int(log_rows), int(log_arity), int(ext_degree),
                                        int(ext_w) if ext_degree > 1 else 0, _u64_array(beta), self._shift_arg(shift, 1),
                                        _stream_ptr(stream, out.device)), "ntt_fri_fold")
        return out

    # -------------------------------------------------------------------------------- DEEP openings and quotients
    def _check_deep(self, ext_degree, ext_w, shift, log_rows, words) -> int:
        """The scalar arguments the DEEP calls share; ``words`` = ((name, value, may_be_none), ..): sequences of
        ``ext_degree`` canonical ints.  Returns log_rows."""
        log_rows = self._check_log_rows(log_rows)
        self._check_ext(ext_degree, ext_w)
        for name, value, optional in words:
            if value is not None or not optional:
                self._canonical_words(name, value, ext_degree)
        self._check_shift(shift)
        return log_rows

    def _check_on_domain(self, z, shift, log_rows) -> None:
        if not any(z[1:]) and pow(z[0], 1 << log_rows, self.p) == pow(1 if shift is None else shift, 1 << log_rows, self.p):
            raise ValueError("z lies on the evaluation domain shift*<w_N>")

    def deep_points(self, out: torch.Tensor, z: Sequence[int], *, ext_degree: int = 1, ext_w: int = 0,
                    shift: Optional[int] = None, bitrev: bool = False, log_rows: Optional[int] = None,
                    stream=None) -> torch.Tensor:
        """``out`` = [N = 2^log_rows][ext_degree] receives (z - x_i)^-1, x_i = shift w_N^i (``bitrev``:
        w_N^bitrev(i), the row order of ``lde_matrix(..., bitrev_out=True)``), in the working form of
        ntt_deep_points: times 2^32 mod p on 4-byte elements, the plain value on Goldilocks.  ``z`` is
        ``ext_degree`` canonical ints and must not lie on the domain."""
        log_rows = self._check_deep(ext_degree, ext_w, shift, log_rows, (("z", z, False),))
        if not isinstance(bitrev, bool):
            raise ValueError(f"bitrev must be a bool, not {bitrev!r}")
        z = list(z)
        self._check_on_domain(z, shift, log_rows)
        self._check_matrix(out, 1 << log_rows, ext_degree, "out")
        self._check_device((out, "out"))
        _L.check(self._lib.ntt_deep_points(self._h, _ptr(out), int(log_rows), int(ext_degree),
                                           int(ext_w) if ext_degree > 1 else 0, _u64_array(z), self._shift_arg(shift, 1),
                                           _L.NTT_MATRIX_BITREV_OUT if bitrev else 0,
                                           _stream_ptr(stream, out.device)), "ntt_deep_points")
        return out

    def open_matrix(self, mat: torch.Tensor, width: int, inv: torch.Tensor, values: torch.Tensor, z: Sequence[int], *,
                    ext_degree: int = 1, ext_w: int = 0, shift: Optional[int] = None, bitrev: bool = False,
                    log_rows: Optional[int] = None, stream=None) -> torch.Tensor:
        """``values`` = [width][ext_degree] receives p_j(z) for every column j of ``mat`` = [N][width], the
        evaluations of p_j (degree < N) on shift*<w_N> (ntt_matrix_open); ``inv`` is ``deep_points``' output for
        the same z, shift, bitrev, log_rows and extension."""
        log_rows = self._check_deep(ext_degree, ext_w, shift, log_rows, (("z", z, False),))
        if not isinstance(bitrev, bool):
            raise ValueError(f"bitrev must be a bool, not {bitrev!r}")
        z = list(z)
        self._check_on_domain(z, shift, log_rows)
        rows = 1 << log_rows
        self._check_matrix(mat, rows, width, "mat", log_rows)
        self._check_matrix(inv, rows, ext_degree, "inv")
        self._check_matrix(values, width, ext_degree, "values")
        eb = self.elem_bytes
        self._check_no_overlap(values, "values", width * ext_degree * eb,
                               ((mat, "mat", rows * width * eb), (inv, "inv", rows * ext_degree * eb)))
        self._check_device((mat, "mat"), (inv, "inv"), (values, "values"))
        _L.check(self._lib.ntt_matrix_open(self._h, _ptr(mat), int(width), int(log_rows), _ptr(inv), int(ext_degree),
                                           int(ext_w) if ext_degree > 1 else 0, _u64_array(z), self._shift_arg(shift, 1),
                                           _L.NTT_MATRIX_BITREV_OUT if bitrev else 0, _ptr(values),
                                           _stream_ptr(stream, values.device)), "ntt_matrix_open")
        return values

    def deep_quotient(self, mat: torch.Tensor, width: int, inv: torch.Tensor, values: torch.Tensor, out: torch.Tensor,
                      alpha: Sequence[int], *, scale: Optional[Sequence[int]] = None, accumulate: bool = False,
                      ext_degree: int = 1, ext_w: int = 0, log_rows: Optional[int] = None, stream=None) -> torch.Tensor:
        """``out`` = [N][ext_degree] receives scale * inv[i] * (sum_j alpha^j values[j] - sum_j alpha^j mat[i][j])
        = scale * sum_j alpha^j (p_j(x_i) - p_j(z)) / (x_i - z) (ntt_deep_quotient), in ``inv``'s row order;
        ``accumulate`` adds into ``out``.  ``alpha`` and ``scale`` (None: 1) are ``ext_degree`` canonical ints."""
        log_rows = self._check_deep(ext_degree, ext_w, None, log_rows, (("alpha", alpha, False), ("scale", scale, True)))
        if not isinstance(accumulate, bool):
            raise ValueError(f"accumulate must be a bool, not {accumulate!r}")
        rows = 1 << log_rows
        self._check_matrix(mat, rows, width, "mat", log_rows)
        self._check_matrix(inv, rows, ext_degree, "inv")
        self._check_matrix(values, width, ext_degree, "values")
        self._check_matrix(out, rows, ext_degree, "out")
        eb = self.elem_bytes
        self._check_no_overlap(out, "out", rows * ext_degree * eb,
                               ((mat, "mat", rows * width * eb), (inv, "inv", rows * ext_degree * eb),
                                (values, "values", width * ext_degree * eb)))
        self._check_device((mat, "mat"), (inv, "inv"), (values, "values"), (out, "out"))
        _L.check(self._lib.ntt_deep_quotient(self._h, _ptr(mat), int(width), int(log_rows),
                                             _ptr(inv), _ptr(values), int(ext_degree),
                                             int(ext_w) if ext_degree > 1 else 0, _u64_array(list(alpha)),
                                             None if scale is None else _u64_array(list(scale)),
                                             _L.NTT_DEEP_ACCUMULATE if accumulate else 0, _ptr(out),
                                             _stream_ptr(stream, out.device)), "ntt_deep_quotient")
        return out

    def deep_info(self, width: int, *, log_rows: Optional[int] = None, ext_degree: int = 1):
        """(open_row_chunks, quotient_lanes_per_row) of ``open_matrix`` and ``deep_quotient`` at this shape
        (ntt_deep_info)."""
        log_rows = self._check_deep(ext_degree, 1, None, log_rows, ())
        self._check_shape(width, log_rows)
        chunks, lanes = C.c_uint(), C.c_uint()
        _L.check(self._lib.ntt_deep_info(self._h, int(width), int(log_rows), int(ext_degree), C.byref(chunks),
                                         C.byref(lanes)), "ntt_deep_info")
        return chunks.value, lanes.value

    # -------------------------------------------------------------------------------- Poseidon2 Merkle commitments
    @property
    def poseidon2_width(self) -> int:
        """The permutation's width t on this plan's engine: 16 on 4-byte elements, 8 on Goldilocks (0: no hashing)."""
        if self.elem32:
            return 16
        return 8 if (self.limbs64 == 1 and self.p == FIELDS[3][1]) else 0

    def _check_hashing(self, needs_parameters: bool = False) -> int:
        t = self.poseidon2_width
        if not t:
            raise ValueError("Poseidon2 hashing needs a Goldilocks plan or a plan of 4-byte elements")
        if needs_parameters and getattr(self, "_poseidon2", None) is None:
            raise ValueError("set_poseidon2 must be called first")
        return t

    def set_poseidon2(self, sbox_degree: int, rounds_f: int, rounds_p: int, ext_rc, int_rc: Sequence[int],
                      int_diag: Sequence[int], *, width: Optional[int] = None) -> None:
        """The Poseidon2 parameters of this plan's hashing calls (ntt_plan_set_poseidon2): S-box degree 3, 5 or 7
        coprime to p - 1, ``rounds_f`` even in [2, 16], ``rounds_p`` in [0, 64], ``ext_rc`` = rounds_f rows of t
        canonical ints, ``int_rc`` = rounds_p, ``int_diag`` = t of them.  Blocking; may be called again."""
        t = self._check_hashing()
        if width is not None and (not _is_int(width) or width != t):
            raise ValueError(f"width must be {t} on this plan, not {width!r}")
        if not _is_int(sbox_degree) or sbox_degree not in (3, 5, 7):
            raise ValueError(f"sbox_degree must be 3, 5 or 7, not {sbox_degree!r}")
        if (self.p - 1) % sbox_degree == 0:
            raise ValueError(f"sbox_degree {sbox_degree} divides p - 1: x^{sbox_degree} is no permutation of the field")
        if not _is_int(rounds_f) or not 2 <= rounds_f <= 16 or rounds_f % 2:
            raise ValueError(f"rounds_f must be an even integer in [2, 16], not {rounds_f!r}")
        if not _is_int(rounds_p) or not 0 <= rounds_p <= 64:
            raise ValueError(f"rounds_p must be an integer in [0, 64], not {rounds_p!r}")
        words = self._canonical_words
        try:
            ext_rows = list(ext_rc)
        except TypeError:
            raise ValueError(f"ext_rc must be {rounds_f} rows of {t} integers, not {ext_rc!r}") from None
        if isinstance(ext_rc, str) or len(ext_rows) != rounds_f:
            raise ValueError(f"ext_rc must be {rounds_f} rows of {t} integers")
        ext = [v for r, row in enumerate(ext_rows) for v in words(f"ext_rc[{r}]", row, t)]
        irc = words("int_rc", int_rc, rounds_p)
        diag = words("int_diag", int_diag, t)
        _L.check(self._lib.ntt_plan_set_poseidon2(self._h, t, int(sbox_degree), int(rounds_f), int(rounds_p),
                                                  _u64_array(ext), _u64_array(irc) if irc else None, _u64_array(diag)),
                 "ntt_plan_set_poseidon2")
        self._poseidon2 = (int(sbox_degree), int(rounds_f), int(rounds_p))

    def _check_hash_call(self, width, log_rows) -> int:
        """The arguments the Merkle calls share.  Returns log_rows."""
        self._check_hashing(needs_parameters=True)
        log_rows = self._check_log_rows(log_rows)
        self._check_shape(width, log_rows)
        return log_rows

    def poseidon2_permute(self, states: torch.Tensor, stream=None) -> torch.Tensor:
        """Permute ``states`` = [count][t] in place (ntt_poseidon2_permute)."""
        t = self._check_hashing(needs_parameters=True)
        self._check_layout(states, "states")
        if states.numel() == 0 or states.numel() % t:
            raise ValueError(f"states must hold a positive multiple of {t} elements, not {states.numel()}")
        self._check_device((states, "states"))
        _L.check(self._lib.ntt_poseidon2_permute(self._h, _ptr(states), states.numel() // t,
                                                 _stream_ptr(stream, states.device)), "ntt_poseidon2_permute")
        return states

    def merkle_commit(self, mat: torch.Tensor, width: int, tree: torch.Tensor, *, log_rows: Optional[int] = None,
                      stream=None) -> torch.Tensor:
        """``tree`` = [2N - 1][D] receives the Poseidon2 Merkle tree over the N = 2^log_rows rows of ``mat`` =
        [N][width] (ntt_merkle_commit): the leaf digests first, in row order, the root last."""
        log_rows = self._check_hash_call(width, log_rows)
        rows, d = 1 << log_rows, self.poseidon2_width // 2
        self._check_matrix(mat, rows, width, "mat", log_rows)
        self._check_matrix(tree, 2 * rows - 1, d, "tree")
        eb = self.elem_bytes
        self._check_no_overlap(tree, "tree", (2 * rows - 1) * d * eb, ((mat, "mat", rows * width * eb),))
        self._check_device((mat, "mat"), (tree, "tree"))
        _L.check(self._lib.ntt_merkle_commit(self._h, _ptr(mat), int(width), int(log_rows),
                                             _ptr(tree), _stream_ptr(stream, tree.device)),
                 "ntt_merkle_commit")
        return tree

    def merkle_open(self, mat: Optional[torch.Tensor], width: int, tree: torch.Tensor, index: torch.Tensor,
                    rows_out: Optional[torch.Tensor], paths: torch.Tensor, *, log_rows: Optional[int] = None,
                    stream=None):
        """For every query q of ``index`` (int32, taken & (N - 1)): ``rows_out[q]`` = that row of ``mat`` and
        ``paths[q][l]`` = the sibling at layer l (ntt_merkle_open).  ``mat`` and ``rows_out`` may both be None."""
        log_rows = self._check_hash_call(width, log_rows)
        rows, d = 1 << log_rows, self.poseidon2_width // 2
        if (mat is None) != (rows_out is None):
            raise ValueError("mat and rows_out must both be given or both be None")
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or not index.is_contiguous() or index.numel() < 1:
            raise ValueError("index must be a contiguous int32 tensor of at least one query")
        nq = index.numel()
        self._check_matrix(tree, 2 * rows - 1, d, "tree")
        if log_rows or paths is not None:
            self._check_matrix(paths, nq * log_rows, d, "paths")
        eb = self.elem_bytes
        inputs = [(tree, "tree", (2 * rows - 1) * d * eb), (index, "index", nq * 4)]
        if mat is not None:
            self._check_matrix(mat, rows, width, "mat", log_rows)
            self._check_matrix(rows_out, nq, width, "rows_out")
            inputs.append((mat, "mat", rows * width * eb))
            self._check_no_overlap(rows_out, "rows_out", nq * width * eb, inputs)
        if paths is not None and log_rows:
            self._check_no_overlap(paths, "paths", nq * log_rows * d * eb, inputs)
        self._check_device((mat, "mat"), (tree, "tree"), (index, "index"), (rows_out, "rows_out"), (paths, "paths"))
        ptr = lambda t: None if t is None or t.numel() == 0 else _ptr(t)
        _L.check(self._lib.ntt_merkle_open(self._h, ptr(mat), int(width), int(log_rows), ptr(tree), ptr(index), nq,
                                           ptr(rows_out), ptr(paths), _stream_ptr(stream, tree.device)),
                 "ntt_merkle_open")
        return rows_out, paths

    def merkle_info(self, width: int, *, log_rows: Optional[int] = None):
        """(digest_elems, tree_elems, launches, tail_log) of ``merkle_commit`` at this shape (ntt_merkle_info)."""
        self._check_hashing()
        log_rows = self._check_log_rows(log_rows)
        self._check_shape(width, log_rows)
        d, te, la, tl = C.c_uint(), C.c_uint64(), C.c_uint(), C.c_uint()
        _L.check(self._lib.ntt_merkle_info(self._h, int(width), int(log_rows), C.byref(d), C.byref(te), C.byref(la),
                                           C.byref(tl)), "ntt_merkle_info")
        return d.value, te.value, la.value, tl.value

    # -------------------------------------------------------------------------------- batch inverse and column scans
    def _check_scan_engine(self) -> None:
        if not self.poseidon2_width:  # the engines of the matrix calls
            raise ValueError("batch_inverse and matrix_scan need a Goldilocks plan or a plan of 4-byte elements")

    def batch_inverse(self, t: torch.Tensor, out: Optional[torch.Tensor] = None, *, ext_degree: int = 1, ext_w: int = 0,
                      stream=None) -> torch.Tensor:
        """``out`` = [count][ext_degree] receives the inverse of every element of ``t`` in the plan's I/O form
        (ntt_batch_inverse); a zero element gives zero.  ``out`` None: in place."""
        self._check_scan_engine()
        self._check_ext(ext_degree, ext_w)
        self._check_layout(t, "t")
        out = t if out is None else out
        self._check_layout(out, "out")
        elems = t.numel() * t.element_size() // self.elem_bytes
        if elems == 0 or elems % ext_degree:
            raise ValueError(f"t must hold a positive multiple of {ext_degree} elements, not {elems}")
        if elems >= 1 << 32:
            raise ValueError(f"count * ext_degree must stay below 2^32, not {elems}")
        if out.numel() != t.numel():
            raise ValueError(f"out: expected {t.numel()} elements like t, not {out.numel()}")
        self._check_no_overlap(out, "out", elems * self.elem_bytes, ((t, "t", elems * self.elem_bytes),), same_ok=True)
        self._check_device((t, "t"), (out, "out"))
        _L.check(self._lib.ntt_batch_inverse(self._h, _ptr(t), _ptr(out),
                                             elems // ext_degree, int(ext_degree), int(ext_w) if ext_degree > 1 else 0,
                                             _stream_ptr(stream, out.device)), "ntt_batch_inverse")
        return out

    def _check_scan_shape(self, width, ext_degree, ext_w, op, rows) -> int:
        """The arguments matrix_scan and scan_info share.  Returns the op's number."""
        self._check_scan_engine()
        if op not in ("sum", "product"):
            raise ValueError(f"op must be 'sum' or 'product', not {op!r}")
        self._check_ext(ext_degree, ext_w, reads_w=op == "product")
        if not _is_int(width) or width < 1:
            raise ValueError(f"width must be a positive integer, not {width!r}")
        if not _is_int(rows) or rows < 1:
            raise ValueError(f"rows must be a positive integer, not {rows!r}")
        if rows * width * ext_degree >= 1 << 32:
            raise ValueError(f"rows * width * ext_degree must stay below 2^32, not {rows} * {width} * {ext_degree}")
        return _L.NTT_SCAN_PRODUCT if op == "product" else _L.NTT_SCAN_SUM

    def matrix_scan(self, mat: torch.Tensor, out: torch.Tensor, width: int, *, op: str = "sum", exclusive: bool = False,
                    totals: Optional[torch.Tensor] = None, ext_degree: int = 1, ext_w: int = 0,
                    rows: Optional[int] = None, stream=None) -> torch.Tensor:
        """``out[i][j]`` = the sum (``op`` "sum") or ring product ("product") of ``mat[r][j]`` over r <= i
        (``exclusive``: r < i, row 0 the identity) for ``mat`` = [rows][width] elements of ``ext_degree`` coefficients
        (ntt_matrix_scan); ``totals`` = [width][ext_degree] receives the columns' totals.  ``out`` may be ``mat``.
        ``rows`` defaults to what ``mat`` holds."""
        self._check_layout(mat, "mat")
        if rows is None and _is_int(width) and width > 0 and _is_int(ext_degree) and ext_degree in (1, 2, 4):
            rows = mat.numel() * mat.element_size() // (self.elem_bytes * width * ext_degree)
        opn = self._check_scan_shape(width, ext_degree, ext_w, op, rows)
        if not isinstance(exclusive, bool):
            raise ValueError(f"exclusive must be a bool, not {exclusive!r}")
        self._check_layout(out, "out")
        elems = rows * width * ext_degree
        for x, what in ((mat, "mat"), (out, "out")):
            if x.numel() * x.element_size() != elems * self.elem_bytes:
                raise ValueError(f"{what}: expected {rows} rows of {width * ext_degree} elements of {self.elem_bytes} bytes")
        self._check_no_overlap(out, "out", elems * self.elem_bytes, ((mat, "mat", elems * self.elem_bytes),), same_ok=True)
        if totals is not None:
            self._check_layout(totals, "totals")
            if totals.numel() * totals.element_size() != width * ext_degree * self.elem_bytes:
                raise ValueError(f"totals: expected {width} rows of {ext_degree} elements of {self.elem_bytes} bytes")
            self._check_no_overlap(totals, "totals", width * ext_degree * self.elem_bytes,
                                   ((mat, "mat", elems * self.elem_bytes), (out, "out", elems * self.elem_bytes)))
        self._check_device((mat, "mat"), (out, "out"), (totals, "totals"))
        _L.check(self._lib.ntt_matrix_scan(self._h, _ptr(mat), _ptr(out), int(rows),
                                           int(width), int(ext_degree), int(ext_w) if ext_degree > 1 and opn else 0, opn,
                                           _L.NTT_SCAN_EXCLUSIVE if exclusive else 0,
                                           None if totals is None else _ptr(totals),
                                           _stream_ptr(stream, out.device)), "ntt_matrix_scan")
        return out

    def scan_info(self, rows: int, width: int, *, op: str = "sum", ext_degree: int = 1):
        """(strip_cols, run_rows, chunk_rows, chunks, launches) of ``matrix_scan`` at this shape (ntt_scan_info)."""
        opn = self._check_scan_shape(width, ext_degree, 1, op, rows)
        v = [C.c_uint() for _ in range(5)]
        _L.check(self._lib.ntt_scan_info(self._h, int(rows), int(width), int(ext_degree), opn, *(C.byref(x) for x in v)),
                 "ntt_scan_info")
        return tuple(x.value for x in v)

    def matrix_passes(self, width: int) -> List[int]:
        """log2 radices of the passes the matrix calls run at this width (ntt_plan_matrix_info); [] for
        sizes up to 4 rows, which one simple kernel transforms."""
        if not isinstance(width, int) or isinstance(width, bool) or width < 1:
            raise ValueError(f"width must be a positive integer, not {width!r}")
        npass = C.c_uint()
        radix = (C.c_uint * 8)()
        _L.check(self._lib.ntt_plan_matrix_info(self._h, int(width), C.byref(npass), radix), "ntt_plan_matrix_info")
        return [radix[i] for i in range(npass.value)]

    def pointwise_mul(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, stream=None) -> torch.Tensor:
        for t in (a, b, out):
            self._check_tensor(t)
        _L.check(self._lib.ntt_pointwise_mul(self._h, _ptr(a), _ptr(b),
                                             _ptr(out), _stream_ptr(stream, a.device)),
                 "ntt_pointwise_mul")
        return out

    def polymul(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, stream=None) -> torch.Tensor:
        for t in (a, b, out):
            self._check_tensor(t)
        _L.check(self._lib.ntt_polymul(self._h, _ptr(a), _ptr(b),
                                       _ptr(out), _stream_ptr(stream, a.device)), "ntt_polymul")
        return out

    def inverse_pointwise_batch(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, batch: int,
                                stream=None) -> torch.Tensor:
        """out = INTT(a * b) over `batch` transforms (a, b already forward-transformed)."""
        for t in (a, b, out):
            self._check_tensor(t, batch)
        _L.check(self._lib.ntt_inverse_pointwise_batch(self._h, _ptr(a), _ptr(b),
                                                       _ptr(out), int(batch),
                                                       _stream_ptr(stream, a.device)), "ntt_inverse_pointwise_batch")
        return out

    def fill(self, t: torch.Tensor, kind: str = "random", seed: int = 1, stream=None) -> torch.Tensor:
        """SURVEY §8d synthetic inputs on the device: 'iota' (x_j = j) or 'random' (SplitMix64)."""
        self._check_tensor(t)
        k = {"iota": 0, "random": 1}[kind]
        _L.check(self._lib.ntt_fill(self._h, _ptr(t), k, int(seed), _stream_ptr(stream, t.device)),
                 "ntt_fill")
        return t

    def fill_map(self, t: torch.Tensor, kind: str, seed: int, row0: int, log_inner: int, log_stride: int,
                 stream=None) -> torch.Tensor:
        """Local element i <- synthetic value of global j = row0 + (i >> log_inner) + ((i & m) << log_stride)."""
        count = t.numel() * t.element_size() // self.elem_bytes
        k = {"iota": 0, "random": 1}[kind]
        _L.check(self._lib.ntt_fill_map(self._h, _ptr(t), count, k, int(seed), int(row0),
                                        int(log_inner), int(log_stride), _stream_ptr(stream, t.device)),
                 "ntt_fill_map")
        return t

    def twiddle_pack(self, src: torch.Tensor, dst: torch.Tensor, log_rows: int, log_row_len: int, log_block: int,
                     row0: int, inverse: bool = False, stream=None, peer_stride: Optional[int] = None) -> torch.Tensor:
        """dst[q * peer_stride + a * bw + b % bw] = src[a][b] * w_n^(+-(row0 + a) * b), q = b >> log_block
        (four-step twiddle + pack; peer_stride defaults to the dense 2^(log_rows + log_block))."""
        ps = (1 << (log_rows + log_block)) if peer_stride is None else int(peer_stride)
        _L.check(self._lib.ntt_twiddle_pack_ex(self._h, _ptr(src), _ptr(dst),
                                               int(log_rows), int(log_row_len), int(log_block), int(row0),
                                               int(bool(inverse)), ps, _stream_ptr(stream, src.device)),
                 "ntt_twiddle_pack_ex")
        return dst

    def transpose(self, src: torch.Tensor, dst: torch.Tensor, log_rows: int, log_cols: int, stream=None,
                  log_block_rows: Optional[int] = None, block_stride: Optional[int] = None):
        """dst[c][r] = src row r, column c; source rows in blocks of 2^log_block_rows starting every
        block_stride elements (default: one dense [rows][cols] matrix)."""
        lb = log_rows if log_block_rows is None else int(log_block_rows)
        bs = (1 << (lb + log_cols)) if block_stride is None else int(block_stride)
        _L.check(self._lib.ntt_transpose_ex(self._h, _ptr(src), _ptr(dst),
                                            int(log_rows), int(log_cols), lb, bs, _stream_ptr(stream, src.device)),
                 "ntt_transpose_ex")
        return dst

    def set_profiling(self, enable: bool = True) -> None:
        _L.check(self._lib.ntt_plan_set_profiling(self._h, int(bool(enable))), "ntt_plan_set_profiling")

    def last_launch_ms(self) -> List[float]:
        """Kernel durations (ms, HIP events on the launch stream) of the most recent transform."""
        buf = (C.c_float * 16)()
        k = C.c_uint()
        _L.check(self._lib.ntt_plan_last_launch_ms(self._h, buf, 16, C.byref(k)), "ntt_plan_last_launch_ms")
        return [buf[i] for i in range(k.value)]

    def last_launch_labels(self) -> List[str]:
        """Labels of the same launches (ntt.h ntt_plan_last_launch_labels: c8, c8s, f8, ...)."""
        buf = C.create_string_buffer(256)
        _L.check(self._lib.ntt_plan_last_launch_labels(self._h, buf, 256), "ntt_plan_last_launch_labels")
        v = buf.value.decode()
        return v.split(",") if v else []

    def profile_group(self) -> None:
        """Group mode (ntt.h ntt_plan_profile_group): later transforms join one record until the next call."""
        _L.check(self._lib.ntt_plan_profile_group(self._h), "ntt_plan_profile_group")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ntt_plan_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass


def lde_from_evals(small_plan: NTTPlan, big_plan: NTTPlan, evals: torch.Tensor, out: torch.Tensor,
                   shift: Optional[int] = None, batch: int = 1, stream=None) -> torch.Tensor:
    """Evaluations of ``batch`` polynomials on <w_n> (``small_plan``'s size) -> their evaluations on the
    coset shift*<w_N> (``big_plan``'s size): ``small_plan.inverse_batch`` followed by
    ``big_plan.lde_batch``.  The inverse overwrites ``evals`` with the coefficients."""
    if big_plan.log_n < small_plan.log_n:
        raise ValueError("big_plan must be at least as large as small_plan")
    if (small_plan.p, small_plan.limbs64, small_plan.elem_bytes, small_plan.montgomery_io) != \
            (big_plan.p, big_plan.limbs64, big_plan.elem_bytes, big_plan.montgomery_io):
        raise ValueError("the two plans must share field, element layout and Montgomery-I/O mode")
    big_plan._check_lde(evals, out, big_plan.log_n - small_plan.log_n, shift, batch)
    small_plan.inverse_batch(evals, batch, stream=stream)
    return big_plan.lde_batch(evals, out, big_plan.log_n - small_plan.log_n, shift, batch, stream=stream)


def lde_matrix_from_evals(small_plan: NTTPlan, big_plan: NTTPlan, evals: torch.Tensor, out: torch.Tensor,
                          shift: Optional[int] = None, width: int = 1, stream=None, *,
                          in_shift: Optional[int] = None, bitrev_out: bool = False) -> torch.Tensor:
    """The matrix form of ``lde_from_evals``: ``evals`` = [n][width] row-major, the evaluations of one
    polynomial per column on <w_n> (``small_plan``'s size) -> ``out`` = [N][width], their evaluations on
    the coset shift*<w_N> (``big_plan``'s size): ``small_plan.inverse_matrix`` followed by
    ``big_plan.lde_matrix``.  The inverse overwrites ``evals`` with the coefficients.  ``in_shift``: the
    evaluations are given on the coset in_shift*<w_n> and interpolated with the coset inverse;
    ``bitrev_out``: ``out`` gets its rows in bit-reversed order (over ``big_plan``'s log_n bits)."""
    if big_plan.log_n < small_plan.log_n:
        raise ValueError("big_plan must be at least as large as small_plan")
    if (small_plan.p, small_plan.limbs64, small_plan.elem_bytes, small_plan.montgomery_io) != \
            (big_plan.p, big_plan.limbs64, big_plan.elem_bytes, big_plan.montgomery_io):
        raise ValueError("the two plans must share field, element layout and Montgomery-I/O mode")
    small_plan._check_matrix_ex(in_shift, bitrev_out, "bitrev_out")
    big_plan._check_lde_matrix(evals, out, big_plan.log_n - small_plan.log_n, shift, width)
    small_plan.inverse_matrix(evals, width, stream=stream, shift=in_shift)
    return big_plan.lde_matrix(evals, out, big_plan.log_n - small_plan.log_n, shift, width, stream=stream,
                               bitrev_out=bitrev_out)


# ------------------------------------------------------------------------------------ shims
def SSIP(x: torch.Tensor, omega: int = 3, log_n: Optional[int] = None) -> torch.Tensor:
    """Reference ``SSIP(long long* x, long long omega, uint log_n)`` (GZKP-NTT.cu:1452): forward NTT
    over P = 469762049 in place on a device int64 tensor; blocking like the reference."""
    lib = _L.load()
    if log_n is None:
        log_n = int(x.numel()).bit_length() - 1
    if x.dtype != torch.int64 or not x.is_cuda or x.numel() != (1 << log_n):
        raise ValueError("SSIP expects a device int64 tensor of 2^log_n elements")
    with torch.cuda.device(x.device):
        lib.SSIP(_ptr(x), int(omega), int(log_n))
    _L.check(lib.ntt_last_error(), "SSIP")
    return x


def NTT_GZKP(data: torch.Tensor, length: int, prime: int, omega: int, B: int = 5, G: int = 8) -> torch.Tensor:
    """Reference ``NTT_GZKP<8,256>(data, len, reverse, reverse_len, prime, omega, B, G)``
    (big-num.cu:260): 256-bit elements, modulus-generic, in place, blocking."""
    lib = _L.load()
    if data.dtype != torch.int64 or not data.is_cuda or data.numel() != 4 * length:
        raise ValueError("NTT_GZKP expects a device int64 tensor [len, 4] (cgbn_mem_t<256>)")
    p32 = (C.c_uint32 * 8)(*[(prime >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    g32 = (C.c_uint32 * 8)(*[(omega >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    with torch.cuda.device(data.device):
        st = lib.NTT_GZKP_256(_ptr(data), int(length), None, 0, p32, g32, int(B), int(G))
    _L.check(st, "NTT_GZKP")
    return data
