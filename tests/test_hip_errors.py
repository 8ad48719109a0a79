"""A failed HIP call reaches the caller, whichever translation unit made it.

Runs on the emulator only: its hipGetLastError() can be told to fail once (frad_emu_fail_next, exported by the emulator
build alone).  One entry point per translation unit of libfrad_hip.so, plus frad_p0_analogue at the frame lengths that
take the mixed-radix, Bluestein and direct routes: each must return FRAD_E_HIP, frad_last_hip_error() must give the very
code that was injected, and the same call must succeed right after."""
import zlib

import numpy as np
import pytest

from frad_python_amd.backend.pcmformat import pcm_dtype_code
from helpers import EmuBackend

FRAD_OK, FRAD_E_HIP = 0, -3


@pytest.fixture(scope="module")
def lib():
    return EmuBackend().lib


def abuf(nbytes, dtype=np.uint8):
    """zeroed buffer whose base address is a multiple of 16"""
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + nbytes].view(dtype)


def p0_analogue_call(N):
    def make(lib):
        pcm = abuf(N * 2, np.int16); pcm[:] = (np.arange(N) * 37 % 201 - 100).astype(np.int16)
        stride = (N * 4 + 15) // 16 * 16
        pay, am = abuf(stride), abuf(8, np.float64)
        return lambda: lib.dll.frad_p0_analogue(pcm.ctypes.data, pcm_dtype_code("s16le"), 1, N, 1, N, 32, 2, pay.ctypes.data, stride,
                                                am.ctypes.data, None), (pcm, pay, am)
    return make


def p4_analogue_call(lib):
    pcm, pay, am = abuf(128, np.int16), abuf(128), abuf(8, np.float64)
    return lambda: lib.dll.frad_p4_analogue(pcm.ctypes.data, pcm_dtype_code("s16le"), 1, 64, 1, 64, 16, 2, pay.ctypes.data, 128,
                                            am.ctypes.data, None), (pcm, pay, am)


def crc32_call(lib):
    data, out = abuf(64), abuf(4, np.uint32)
    return lambda: lib.dll.frad_crc32_frames(data.ctypes.data, 64, 1, 64, out.ctypes.data, None), (data, out)


def rs_encode_frames_call(lib):
    data, out = abuf(32), abuf(48)
    return lambda: lib.dll.frad_rs_encode_frames(data.ctypes.data, 32, 1, 32, 16, 4, out.ctypes.data, 48, None), (data, out)


def rows_compact_call(lib):
    rows, nbytes, out, offs = abuf(32), abuf(16, np.int64), abuf(64), abuf(24, np.int64)
    nbytes[:] = (5, 7)
    return lambda: lib.dll.frad_rows_compact(rows.ctypes.data, 16, nbytes.ctypes.data, 2, out.ctypes.data, offs.ctypes.data, None), \
        (rows, nbytes, out, offs)


def inflate_call(lib):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(b"a failed HIP call reaches the caller") + co.flush()
    src, offs = abuf(len(body) + 16), abuf(16, np.int64)
    src[:len(body)] = np.frombuffer(body, np.uint8); offs[:] = (0, len(body))
    dst, n, st = abuf(64), abuf(8, np.int64), abuf(4, np.int32)
    return lambda: lib.dll.frad_inflate_raw(src.ctypes.data, offs.ctypes.data, 1, dst.ctypes.data, 64, n.ctypes.data, st.ctypes.data, None), \
        (src, offs, dst, n, st)


def deflate_call(lib):
    text = b"a failed HIP call reaches the caller"
    src, offs = abuf(len(text) + 16), abuf(16, np.int64)
    src[:len(text)] = np.frombuffer(text, np.uint8); offs[:] = (0, len(text))
    stride = lib.deflate_stride(len(text))
    dst, n, st = abuf(stride), abuf(8, np.int64), abuf(4, np.int32)
    return lambda: lib.dll.frad_deflate_raw(src.ctypes.data, offs.ctypes.data, 1, dst.ctypes.data, stride, n.ctypes.data, st.ctypes.data, None), \
        (src, offs, dst, n, st)


def from_f64_call(lib):
    pcm, out = abuf(64, np.float64), abuf(16, np.int16)
    return lambda: lib.dll.frad_from_f64(pcm.ctypes.data, 8, pcm_dtype_code("s16le"), 2, out.ctypes.data, None), (pcm, out)


def overlap_add_call(lib):
    frames, prev, out, nxt = abuf(64, np.float64), abuf(32, np.float64), abuf(32, np.float64), abuf(32, np.float64)
    return lambda: lib.dll.frad_p1_overlap_add(frames.ctypes.data, 1, 8, 1, 2, prev.ctypes.data, out.ctypes.data, nxt.ctypes.data, None), \
        (frames, prev, out, nxt)


CALLS = {
    "frad_hip.hip: frad_p4_analogue": p4_analogue_call,
    "frad_crc.hip: frad_crc32_frames": crc32_call,
    "frad_ecc.hip: frad_rs_encode_frames": rs_encode_frames_call,
    "frad_golomb.hip: frad_rows_compact": rows_compact_call,
    "frad_inflate.hip: frad_inflate_raw": inflate_call,
    "frad_deflate.hip: frad_deflate_raw": deflate_call,
    "frad_epilogue.hip: frad_from_f64": from_f64_call,
    "frad_p1.hip: frad_p1_overlap_add": overlap_add_call,
    "frad_mixed.hip: frad_p0_analogue N=896": p0_analogue_call(896),
    "frad_p0_blue.hip: frad_p0_analogue N=300": p0_analogue_call(300),
    "frad_hip.hip: frad_p0_analogue N=40 (direct)": p0_analogue_call(40),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_a_failed_hip_call_reaches_the_caller(lib, name):
    call, keep = CALLS[name](lib)
    code = 700 + list(CALLS).index(name)                      # a different code per call: a stale one from the call before shows
    assert call() == FRAD_OK, "the arguments themselves must be valid"
    lib.dll.frad_emu_fail_next(code)
    rc = call()
    got = lib.dll.frad_last_hip_error()
    lib.dll.frad_emu_fail_next(0)                             # (not consumed if the call never asked: do not leak into the next test)
    assert rc == FRAD_E_HIP
    assert got == code
    assert call() == FRAD_OK
    del keep
