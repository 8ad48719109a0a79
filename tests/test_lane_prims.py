"""Parity test of the toolchain seam (frad_platform.hpp): every exact lane primitive has a gfx950 definition
(frad_platform_gfx950.hpp), which ships, and an emulator definition (frad_platform_emu.hpp), which most of this suite
runs.  frad_debug_lane_prims (frad_util.hip, not part of the ABI) applies them to caller-supplied lane inputs in one block of
two waves; the expected bits below come from the plain definitions in NumPy, and the same assertions run on the emulator
library (CPU suite) and on the device (-m gpu).  One launch per case group.

Not here: the four approximate float32 instructions (p1w_sqrtf, k7_log2f, k7_exp2f, k7_rcpf).  They are about 1 ulp from
libm by design; what the kernels build on them is exact and is covered end to end by tests/test_p1_exact.py."""
import ctypes as ct
from fractions import Fraction
import math

import numpy as np
import pytest

T = 128          # threads of the debug kernels: two waves
_backends = {}


class _Emu:
    def __init__(self):
        from helpers import EmuBackend
        self.dll = EmuBackend().lib.dll

    def run(self, group, inp, out_bytes, n=0):
        src = np.zeros(len(inp) + 16, np.uint8); dst = np.zeros(out_bytes + 16, np.uint8)
        so, do = (-src.ctypes.data) % 16, (-dst.ctypes.data) % 16
        src[so:so + len(inp)] = inp
        rc = self.dll.frad_debug_lane_prims(ct.c_int(group), ct.c_void_p(src.ctypes.data + so), ct.c_void_p(dst.ctypes.data + do),
                                            ct.c_int64(n), ct.c_void_p(0))
        assert rc == 0
        return dst[do:do + out_bytes].copy()


class _Gpu:
    def __init__(self):
        import torch
        from frad_python_amd import _lib
        assert torch.cuda.is_available()
        self.t, self.dll = torch, _lib.load().dll

    def run(self, group, inp, out_bytes, n=0):
        t = self.t
        src = t.from_numpy(np.ascontiguousarray(inp)).to("cuda:0")
        dst = t.zeros(out_bytes, dtype=t.uint8, device="cuda:0")
        rc = self.dll.frad_debug_lane_prims(ct.c_int(group), ct.c_void_p(src.data_ptr()), ct.c_void_p(dst.data_ptr()), ct.c_int64(n),
                                            ct.c_void_p(int(t.cuda.current_stream().cuda_stream)))
        assert rc == 0
        t.cuda.synchronize()
        return dst.cpu().numpy()


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param not in _backends:
        _backends[request.param] = _Emu() if request.param == "emu" else _Gpu()
    return _backends[request.param]


def _bytes(*arrays):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    show = (lambda x: hex(int(x))) if got.dtype.kind in "ui" else repr
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: got {show(got.reshape(-1)[bad[0]])}, want {show(want.reshape(-1)[bad[0]])}"


# ---- reductions: the documented butterfly, rows of 16 lanes first (xor 1, 2, 4, 8), then the four rows ------------------
def _rows16(v, op):
    lane = np.arange(T)
    for off in (1, 2, 4, 8):
        v = op(v, v[lane ^ off])
    return v.reshape(2, 4, 16)[:, :, 0]                      # [wave][row]: every lane of a row holds the row's value


def _all(v, op):
    r = _rows16(v, op)
    return np.repeat(op(op(r[:, 0], r[:, 1]), op(r[:, 2], r[:, 3])), 64)


def _halves(v, op):
    r = _rows16(v, op)
    return np.repeat(op(r[:, 0], r[:, 1]), 64), np.repeat(op(r[:, 2], r[:, 3]), 64)


def test_reductions(be):
    rng = np.random.default_rng(47)
    a = rng.integers(0, 2 ** 64, T, dtype=np.uint64)
    a[32:64] >>= np.uint64(20); a[64:96] >>= np.uint64(41); a[96:] |= np.uint64(1) << np.uint64(63)      # four different halves
    # a sum that depends on association: full-width mantissas, magnitudes within 2^8 of each other, both signs
    d = rng.standard_normal(T) * np.exp2(rng.integers(-4, 5, T).astype(np.float64))
    d[32:64] *= 1e-3; d[64:] = d[64:][::-1] * 7.0
    fsum = lambda x, y: x + y
    want_sum = _all(d, fsum)
    for order in (slice(None), slice(None, None, -1)):        # lane 0 to lane 63 in order, and backwards
        seq = np.array([np.cumsum(d[:64][order])[-1], np.cumsum(d[64:][order])[-1]])
        assert (want_sum[::64] != seq).all(), "the data must tell one order of additions from another"
    out = be.run(0, _bytes(a, d), 7 * T * 8).view(np.uint64).reshape(7, T)
    _same(out[0], _all(a, np.maximum), "all-reduce max")
    _same(out[1], _all(a, np.bitwise_or), "all-reduce or")
    _same(out[2], want_sum.view(np.uint64), "all-reduce float64 sum")
    lo, hi = _halves(a, np.maximum)
    _same(out[3], lo, "half-wave max, lanes 0-31"); _same(out[4], hi, "half-wave max, lanes 32-63")
    lo, hi = _halves(d, fsum)
    _same(out[5], lo.view(np.uint64), "half-wave sum, lanes 0-31"); _same(out[6], hi.view(np.uint64), "half-wave sum, lanes 32-63")
    assert (lo != hi).all()


def test_uniform_values(be):
    rng = np.random.default_rng(42)
    v = rng.integers(-2 ** 31, 2 ** 31, T).astype(np.int32)
    src = np.array([[0, 63, 17, 32], [5, 0, 63, 40]], np.int32)
    pred = np.zeros((3, T), np.int32)
    pred[0, 63] = 1                                           # wave 0: lane 63 alone; wave 1: no lane
    pred[1, 64] = 7                                           # wave 0: no lane; wave 1: lane 0 alone
    pred[2] = rng.integers(0, 2, T)                           # many lanes in both
    out = be.run(1, _bytes(v, src, pred), 8 * T * 4).view(np.int32).reshape(8, T)
    vw = v.reshape(2, 64)
    for k in range(4):
        _same(out[k], np.repeat(vw[[0, 1], src[:, k]], 64), f"wave_read_lane, source {src[:, k]}")
    _same(out[4], np.repeat(vw[:, 0], 64), "wave_uniform_int")
    for k in range(3):
        _same(out[5 + k], np.repeat((pred[k].reshape(2, 64) != 0).any(axis=1).astype(np.int32), 64), f"wave_any, case {k}")
    assert out[5, 0] == 1 and out[5, 64] == 0 and out[6, 0] == 0 and out[6, 64] == 1


def test_bit_field_extract(be):
    rng = np.random.default_rng(43)
    word = rng.integers(0, 2 ** 32, T, dtype=np.uint32)
    word[:8] = [0, 0xffffffff, 0x80000000, 0x7fffffff, 0x00800080, 0x80008000, 0x7f7f7f7f, 0x01020304]
    out = be.run(2, _bytes(word), 16 * T * 4).view(np.int32).reshape(16, T)
    w64 = word.astype(np.int64)
    for wi, width in enumerate((8, 16)):
        for si, shift in enumerate((0, 8, 16, 24)):
            wd = min(width, 32 - shift)                       # a field that would pass bit 31 ends there
            field = (w64 >> shift) & ((1 << wd) - 1)
            _same(out[4 * wi + si], field.astype(np.uint32).view(np.int32), f"unsigned, width {width} at {shift}")
            signed = np.where(field >> (wd - 1), field - (1 << wd), field)
            _same(out[8 + 4 * wi + si], signed.astype(np.int32), f"signed, width {width} at {shift}")


def test_wave_perm(be):
    rng = np.random.default_rng(44)
    v = rng.integers(0, 2 ** 32, T, dtype=np.uint32)
    selb = np.concatenate([np.array([[4, 5, 6, 7], [5, 4, 7, 7], [7, 6, 5, 4]]), rng.integers(4, 8, (16, 4))]).astype(np.uint8)   # byte 0 first
    sel = np.ascontiguousarray(selb).view("<u4").reshape(-1)
    assert list(sel[:3]) == [0x07060504, 0x07070405, 0x04050607]        # the three the kernels use
    out = be.run(3, _bytes(v, sel), len(sel) * T * 4, n=len(sel)).view(np.uint32).reshape(len(sel), T)
    vb = v.view(np.uint8).reshape(T, 4)
    for k in range(len(sel)):
        want = np.ascontiguousarray(vb[:, selb[k] - 4]).view("<u4").reshape(-1)
        _same(out[k], want, f"selector {sel[k]:#010x}")


# ---- arithmetic -----------------------------------------------------------------------------------------------------------
_DEN_MIN, _DEN_MAX, _NORM_MIN, _MAX = 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308
_CLASSES = [0.0, -0.0, math.inf, -math.inf, math.nan, _DEN_MIN, -_DEN_MAX, _NORM_MIN, 1.0, -1.5, 1.0 + 2.0 ** -52, _MAX, -_MAX]


def _fma_exact(s, b, a):
    """fma(s, b, a) with one rounding, from exact rational arithmetic; a NaN result is math.nan"""
    if math.isnan(s) or math.isnan(b) or math.isnan(a):
        return math.nan
    if math.isinf(s) or math.isinf(b):
        if s == 0.0 or b == 0.0:
            return math.nan
        p = math.copysign(math.inf, math.copysign(1.0, s) * math.copysign(1.0, b))
        return math.nan if math.isinf(a) and a != p else p
    if math.isinf(a):
        return a
    exact = Fraction(s) * Fraction(b) + Fraction(a)
    if exact == 0:                                            # an exact zero: the common sign of the two terms, else +0
        ps = math.copysign(1.0, s) * math.copysign(1.0, b)
        both_zero = (s == 0.0 or b == 0.0) and a == 0.0
        return math.copysign(0.0, ps) if both_zero and ps == math.copysign(1.0, a) else 0.0
    try:
        return float(exact)                                   # correctly rounded, signed zero on underflow
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def test_absmax_fma_nonfinite(be):
    rng = np.random.default_rng(45)
    tri = np.array([(s, b, a) for s in _CLASSES for b in _CLASSES for a in _CLASSES])
    n = (len(tri) + 200 + T - 1) // T * T
    extra = n - len(tri)
    # where one rounding differs from two: (1 + x)(1 + y) - 1 with x y below an ulp of the product; products that overflow
    # alone but not with the addend; denormal results
    x = 1.0 + rng.integers(1, 2 ** 30, extra) * 2.0 ** -52
    more = np.stack([x, 1.0 + rng.integers(1, 2 ** 30, extra) * 2.0 ** -52, -np.ones(extra)], axis=1)
    more[::3] = np.stack([rng.uniform(1, 2, extra) * 1e154, rng.uniform(1, 2, extra) * 1e154, -rng.uniform(0.5, 1, extra) * _MAX], axis=1)[::3]
    more[1::3] = np.stack([rng.uniform(1, 2, extra) * 1e-154, rng.uniform(-2, 2, extra) * 1e-160, rng.uniform(-1, 1, extra) * 1e-310], axis=1)[1::3]
    tri = np.concatenate([tri, more])
    fm = np.resize(np.array([0.0, _DEN_MIN, 1.0, 2.5, 1e308, math.inf]), n)
    v = np.concatenate([np.repeat(np.array(_CLASSES + [-_DEN_MIN, 2.5, -2.5, 1e308, -1e-300]), 6), rng.standard_normal(n)])[:n]
    fbits = np.concatenate([np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7fa00000, 0xff800001, 1, 0x807fffff,
                                      0x00800000, 0x7f7fffff, 0xff7fffff, 0x3f800000], np.uint32), rng.integers(0, 2 ** 32, n, dtype=np.uint32)])[:n]
    inp = _bytes(fm, v, tri[:, 0].copy(), tri[:, 1].copy(), tri[:, 2].copy(), fbits)
    out = be.run(4, inp, n * 20, n=n)
    am, fma, nf = out[:8 * n].view(np.uint64), out[8 * n:16 * n].view(np.float64), out[16 * n:].view(np.uint32)
    with np.errstate(all="ignore"):
        _same(am, np.where(np.isnan(v), fm, np.maximum(fm, np.abs(v))).view(np.uint64), "absmax_acc")
    want = np.array([_fma_exact(*map(float, r)) for r in tri])
    isn = np.isnan(want)
    assert isn.sum() > 400 and (~isn).sum() > 1500
    _same(np.isnan(fma), isn, "fma_free: NaN results")          # (of a NaN, sign and payload are the implementation's)
    _same(fma[~isn].view(np.uint64), want[~isn].view(np.uint64), "fma_free")
    with np.errstate(all="ignore"):
        two = tri[:, 0] * tri[:, 1] + tri[:, 2]
    assert (two[~isn].view(np.uint64) != want[~isn].view(np.uint64)).sum() > 30, "cases that tell one rounding from two"
    _same(nf, ((fbits & 0x7f800000) == 0x7f800000).astype(np.uint32), "nonfinite_f32")


def test_lds_dma_and_nontemporal(be):
    rng = np.random.default_rng(46)
    src = rng.integers(0, 256, (2, T, 16), dtype=np.uint8)      # the DMA's source (1 KiB per wave), the nontemporal round trip's
    out = be.run(5, _bytes(src), 3 * T * 16).reshape(3, T, 16)
    _same(out[0], src[0], "LDS-DMA, own slot")
    _same(out[1], src[0].reshape(2, 64, 16)[:, ::-1].reshape(T, 16), "LDS-DMA, mirrored slot")
    _same(out[2], src[1], "nontemporal load and store")
