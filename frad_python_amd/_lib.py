"""ctypes binding of the C-ABI in include/frad_hip.h (libfrad_hip.so).

PyTorch is plumbing here (device memory + streams): the signatures carry raw device pointers
and sizes only.  There is no CPU fallback: if the HIP library has not been built, or no MI355X
is visible, every operator raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libfrad_hip.so")

FRAD_LITTLE_ENDIAN = 1
FRAD_RAW_BE_INTS = 2

# every symbol include/frad_hip.h declares: name -> (restype, argtypes).  STATUS is an `int` that is a frad_status: the binding
# raises FradError unless it is 0; a plain c_int (frad_abi_version, frad_has_fast_path, frad_last_hip_error) is a value.
STATUS = "frad_status"
SYMBOLS = {
    "frad_abi_version": (c_int, []),
    "frad_strerror": (c_char_p, [c_int]),
    "frad_last_hip_error": (c_int, []),
    "frad_payload_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "frad_has_fast_path": (c_int, [c_int32, c_int32, c_int32]),
    "frad_plan_prepare": (STATUS, [c_int32, c_int32]),
    "frad_plan_clear": (None, []),
    "frad_p0_analogue": (STATUS, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64, c_int32, c_uint32,
                                 c_void_p, c_int64, c_void_p, c_void_p]),
    "frad_p0_analogue_checked": (STATUS, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64, c_int32, c_uint32,
                                         c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "frad_p0_overflow_scan": (STATUS, [c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "frad_p0_digital": (STATUS, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_uint32, c_void_p, c_void_p]),
    "frad_p0_analogue_clips": (STATUS, [c_void_p, c_int32, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_uint32,
                                       c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "frad_p0_digital_clips": (STATUS, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_uint32, c_void_p, c_int64, c_void_p]),
    "frad_p4_analogue": (STATUS, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64, c_int32, c_uint32,
                                 c_void_p, c_int64, c_void_p, c_void_p]),
    "frad_p4_digital": (STATUS, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_uint32, c_void_p, c_void_p]),
    "frad_p1_analogue": (STATUS, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64, c_int32, c_int32, c_int32,
                                 c_double, c_uint32, c_void_p, c_void_p, c_void_p]),
    "frad_p1_digital": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "frad_crc32_frames": (STATUS, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "frad_p1_overlap_add": (STATUS, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "frad_p1_overlap_add_pcm": (STATUS, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int32, c_uint32, c_void_p, c_void_p, c_void_p]),
    "frad_clips_overlap_add": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int32, c_uint32, c_void_p, c_void_p, c_int64, c_void_p]),
    "frad_clips_window_add": (STATUS, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int32, c_uint32, c_void_p, c_void_p, c_int64, c_void_p]),
    "frad_clips_carry_add": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_uint32, c_void_p,
                                     c_void_p, c_int64, c_void_p]),
    "frad_clips_resample": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                    c_void_p, c_int32, c_uint32, c_void_p, c_void_p, c_int64, c_void_p]),
    "frad_clips_remix": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_uint32, c_void_p,
                                 c_void_p, c_int64, c_void_p]),
    "frad_clips_spectrum": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                    c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double, c_int32, c_void_p,
                                    c_void_p]),
    "frad_clips_frame_cut": (STATUS, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "frad_clips_carry_cut": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    "frad_p1_golomb_bound": (c_size_t, [c_int32, c_int32]),
    "frad_p1_golomb_encode": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "frad_rows_compact": (STATUS, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "frad_p1_golomb_decode": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "frad_p2_golomb_decode": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "frad_p2_synth": (STATUS, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "frad_p2_analogue": (STATUS, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64, c_int32, c_int32, c_int32, c_double, c_uint32,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "frad_p2_golomb_bound": (c_size_t, [c_int32, c_int32]),
    "frad_p2_golomb_encode": (STATUS, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "frad_from_f64": (STATUS, [c_void_p, c_int64, c_int32, c_uint32, c_void_p, c_void_p]),
    "frad_p0_digital_pcm": (STATUS, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_uint32, c_int32, c_void_p, c_void_p]),
    "frad_p4_digital_pcm": (STATUS, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_uint32, c_int32, c_void_p, c_void_p]),
    "frad_p1_digital_pcm": (STATUS, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_uint32, c_void_p, c_void_p]),
    "frad_asfh_scan": (c_int64, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "frad_rs_encode": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "frad_rs_repair": (STATUS, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    "frad_rs_encode_frames": (STATUS, [c_void_p, c_int64, c_int64, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "frad_crc16_ansi_frames": (STATUS, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "frad_inflate_raw": (STATUS, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "frad_deflate_raw": (STATUS, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "frad_deflate_stride": (c_int64, [c_int64]),
    "frad_bench_copy": (STATUS, [c_void_p, c_void_p, c_int64, c_void_p]),
}


# mirror of `frad_frame_info` (include/frad_hip.h)
def _frame_info_dtype():
    import numpy as np
    return np.dtype([("header_off", "<i8"), ("payload_off", "<i8"), ("payload_bytes", "<i8"), ("profile", "<i4"), ("ecc", "<i4"),
                     ("little_endian", "<i4"), ("depth_idx", "<i4"), ("channels", "<i4"), ("srate", "<i4"), ("fsize", "<i4"),
                     ("overlap_ratio", "<i4"), ("ecc_dsize", "<i4"), ("ecc_codesize", "<i4"), ("force_flush", "<i4"), ("crc", "<u4")])


FRAME_INFO_DTYPE = _frame_info_dtype()
assert FRAME_INFO_DTYPE.itemsize == 72


class FradError(RuntimeError):
    def __init__(self, status: int, message: str, hip_error: int = 0):
        super().__init__(f"libfrad_hip: {message} (status {status}" + (f", hipError {hip_error})" if hip_error else ")"))
        self.status = status
        self.hip_error = hip_error


class FradLib:
    """One loaded copy of the C-ABI library; methods take raw pointers (ints) and sizes.

    Every symbol of ``SYMBOLS`` is a method named like the symbol without ``frad_``, with the C parameters in the C order,
    generated in ``__init__``: a status entry point raises ``FradError`` unless it returns 0, and its trailing ``stream`` may
    be left out (NULL, the default stream); any other entry point returns its value.  The methods written out below are the
    ones whose Python signature is deliberately not the C one."""

    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: the HIP transform core has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the product path.")
        self.path = path
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and must be the one that gets loaded.  If this
        # library came first it would bind /opt/rocm's copy, torch would then bring a second runtime, and every launch here
        # would fail with hipErrorNoDevice (seen when build() and smoke() run in one process).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        self.dll = ctypes.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(self.dll, name)           # AttributeError if the library lacks a symbol
            fn.restype, fn.argtypes = (c_int if res is STATUS else res), args
            if not hasattr(FradLib, name[5:]):     # (a method written out below keeps its own signature)
                setattr(self, name[5:], self._checked(fn, len(args)) if res is STATUS else fn)

    def _checked(self, fn, n_args: int):
        """the method of a status entry point; ``stream``, its last parameter, defaults to 0"""
        def call(*args):
            rc = fn(*args) if len(args) == n_args else fn(*args, 0)
            if rc:
                self._check(rc)
        call.__name__ = fn.__name__[5:]
        return call

    def _check(self, rc: int):
        if rc != 0:
            raise FradError(rc, self.dll.frad_strerror(rc).decode(), self.dll.frad_last_hip_error())

    # casts and defaults
    def payload_bytes(self, N, C, bits):
        return int(self.dll.frad_payload_bytes(N, C, bits))

    def has_fast_path(self, N, C, f32=False):
        return bool(self.dll.frad_has_fast_path(N, C, int(f32)))

    def plan_prepare(self, N, f32=False):
        self._check(self.dll.frad_plan_prepare(N, int(f32)))

    def deflate_stride(self, max_body_bytes):
        """a negative result is a frad_status"""
        r = int(self.dll.frad_deflate_stride(max_body_bytes))
        self._check(r if r < 0 else 0)
        return r

    # `flags` sits behind the stream and defaults to FRAD_RAW_BE_INTS: these four take the reference's from_f64 as it is
    def from_f64(self, pcm, n_values, out_dtype, out, stream=0, flags=FRAD_RAW_BE_INTS):
        self._check(self.dll.frad_from_f64(pcm, n_values, out_dtype, flags, out, stream))

    def p1_digital_pcm(self, q, tq, n_frames, N, C, bits, srate, out_dtype, out, stream=0, flags=FRAD_RAW_BE_INTS):
        self._check(self.dll.frad_p1_digital_pcm(q, tq, n_frames, N, C, bits, srate, out_dtype, flags, out, stream))

    def p1_overlap_add_pcm(self, frames, n_frames, N, C, ratio, prev_tail, out_dtype, out, next_tail, stream=0, flags=FRAD_RAW_BE_INTS):
        self._check(self.dll.frad_p1_overlap_add_pcm(frames, n_frames, N, C, ratio, prev_tail, out_dtype, flags, out, next_tail, stream))

    def clips_overlap_add(self, frames, clip_frame0, n_clips, N, C, ratio, tails, tail_off, tail_rows, tail_win, out_dtype, out, out_off,
                          out_rows, stream=0, flags=FRAD_RAW_BE_INTS):
        self._check(self.dll.frad_clips_overlap_add(frames, clip_frame0, n_clips, N, C, ratio, tails, tail_off, tail_rows, tail_win,
                                                    out_dtype, flags, out, out_off, out_rows, stream))

    def asfh_scan(self, data, start: int = 0, max_frames: int = 0):
        """frad_asfh_scan over a bytes-like object -> (numpy structured table, next_pos, stop_reason)"""
        import numpy as np
        view = memoryview(data)
        n = view.nbytes
        cap = max_frames or max(16, (n - start) // 9 + 1)
        cap = min(cap, 1 << 22)
        table = np.zeros(cap, FRAME_INFO_DTYPE)
        nxt, why = ctypes.c_int64(0), ctypes.c_int32(0)
        buf = (ctypes.c_char * n).from_buffer_copy(view) if view.readonly and not isinstance(data, (bytes, bytearray)) else None
        ptr = ctypes.cast(ctypes.c_char_p(data), c_void_p) if isinstance(data, bytes) else \
            ctypes.addressof((ctypes.c_char * n).from_buffer(data)) if buf is None else ctypes.addressof(buf)
        rows = self.dll.frad_asfh_scan(ptr, n, start, table.ctypes.data, cap, ctypes.byref(nxt), ctypes.byref(why))
        if rows < 0:
            self._check(int(rows))
        return table[:rows], int(nxt.value), int(why.value)


_lib: FradLib | None = None


def load() -> FradLib:
    """The product library (HIP, gfx950).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = FradLib(LIB_PATH)
    return _lib
