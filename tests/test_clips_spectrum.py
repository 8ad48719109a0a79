"""frad_clips_spectrum alone: framing, window, float64 FFT, |X|^2 or |X|, banded filterbank, logarithm, float32/float64 stores for
many ragged float64 windows in one launch (include/frad_hip.h).

Legs, raw pointers and guard bytes as in test_clips_ola.py ("emu": the CPU interpreter build of the same kernel source, "gpu": the
MI355X), whose backends are imported.  The model is ``spectral.clips_spectrum_host`` (``np.fft.rfft`` in float64).

Tolerance, derived and not tuned.  u = 2^-53, N = n_fft, E_f = sum((x w)^2) of the model's frame, W_m = sum_k |W[m][k]| (1 without
a filterbank): |got - model| <= 32 u log2(N) N E_f W_m for power = 2 and 16 u log2(N) sqrt(N E_f) W_m for power = 1 -- the
radix-FFT error bound with constant 8 per stage, doubled for the window product and the sums -- plus 2^-23 |model| for float32
output.  ``test_numpy_rfft_is_well_inside_the_bound_and_float32_is_not`` shows on the CPU that numpy's own rfft uses a small part
of that bound against a long-double DFT and that a float32 transform misses it by orders of magnitude.  With a logarithm the
test sets floor = 2^20 * (the largest linear bound of the case), so that every element, the clamped ones included, obeys
|got - model| <= s 2^-19 (+ 2^-23 |model| for float32).  No element is left out of any comparison."""
import math

import numpy as np
import pytest

from frad_python_amd._lib import FradError
from frad_python_amd.spectral import LOG_SCALE, SpecTables, bands_of, clips_spectrum_host, frame_count, make_window
from test_clips_ola import GUARD, be  # noqa: F401  (be: the fixture)

U = 2.0 ** -53
F32, F64 = 20, 22                                              # FRAD_PCM_F32LE, FRAD_PCM_F64LE
PLANS = (128, 256, 512, 1024, 2048, 4096)


def tables(n_fft, hop, *, center=False, power=2, window="hann", win_length=None, bank=None, log=None, floor=None, dtype="f64"):
    w = make_window(window, win_length or n_fft, n_fft)
    return SpecTables(n_fft, hop, center, power, w, bands_of(np.asarray(bank, np.float64)) if bank is not None else None,
                      LOG_SCALE[log] if log else 0.0, floor, np.float64 if dtype == "f64" else np.float32)


def place(be, clips):
    """the sources in one buffer with NaNs between them, so that a clip starts 8 or 16 bytes off a 16-byte boundary (as
    test_clips_remix.layout places them) -> (what has to stay alive, the pointer table)"""
    parts, at, where = [np.full(3, np.nan)], 3, []
    for x in clips:
        where.append(at)
        if x is not None and x.size:
            parts.append(np.ascontiguousarray(x, np.float64).reshape(-1))
            at += x.size
            parts.append(np.full(1 + len(where) % 2, np.nan))
            at += parts[-1].size
    d_src = be.put(np.concatenate(parts))
    ptr = np.array([be.ptr(d_src) + 8 * w if x is not None and x.size else 0 for w, x in zip(where, clips)], np.int64)
    return d_src, be.put(ptr)


status = [0]                                                   # of the last raw_call that overrode an argument


def raw_call(be, clips, tb, K, frame_off, out_frames, out, out_at=0, valid=None, over=None):
    """the raw entry point; ``out``: a uint8 host array that is uploaded, written from byte ``out_at`` on, and returned"""
    keep, d_ptr = place(be, clips)
    valid = np.array([0 if x is None else len(x) for x in clips], np.int32) if valid is None else np.asarray(valid, np.int32)
    d_valid, d_off = be.put(valid), be.put(np.ascontiguousarray(frame_off, np.int64))
    d_win = be.put(tb.window)
    has = tb.band_lo is not None
    d_b = [be.put(a if a.size else np.zeros(1, a.dtype)) for a in (tb.band_lo, tb.band_len, tb.band_off, tb.band_w)] if has else [None] * 4
    d_out = be.put(out)
    a = dict(src=be.ptr(d_ptr), valid=be.ptr(d_valid), n_clips=len(clips), K=K, off=be.ptr(d_off), out_frames=out_frames, n_fft=tb.n_fft,
             hop=tb.hop, center=int(tb.center), window=be.ptr(d_win), power=tb.power, n_bands=tb.n_bins if has else 0, lo=be.ptr(d_b[0]),
             ln=be.ptr(d_b[1]), boff=be.ptr(d_b[2]), w=be.ptr(d_b[3]), n_w=len(tb.band_w) if has else 0, s=tb.log_scale, floor=tb.floor,
             floor_log=tb.floor_log, dtype=F64 if tb.dtype == np.float64 else F32, out=be.ptr(d_out) + out_at)
    a.update(over or {})
    status[0] = 0
    try:
        be.lib.clips_spectrum(*a.values(), be.stream)
    except FradError as e:
        if not over:
            raise
        status[0] = e.status
    got = be.get(d_out)
    del keep
    return got


def run(be, clips, tb, K, pad=None, misalign=0):
    """ragged (every clip its own frame count) or, with ``pad``, dense (every clip the frames of ``pad`` rows) -> ([frames, K,
    n_bins], frame_off); the guards are checked"""
    counts = [frame_count(len(x) if x is not None else 0, tb.n_fft, tb.hop, tb.center) if pad is None else
              frame_count(pad, tb.n_fft, tb.hop, tb.center) for x in clips]
    off = np.zeros(len(clips) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    nb = int(off[-1]) * K * tb.n_bins * tb.dtype.itemsize
    raw = raw_call(be, clips, tb, K, off, int(off[-1]), np.full(misalign + nb + GUARD, 0xA5, np.uint8), misalign)
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    return np.frombuffer(raw[misalign:misalign + nb].tobytes(), tb.dtype).reshape(-1, K, tb.n_bins), off


def model(clips, tb, K, pad=None):
    pieces = [clips_spectrum_host(x if x is not None else np.zeros((0, K)), tb, rows=pad) for x in clips]
    return np.concatenate(pieces) if pieces else np.zeros((0, K, tb.n_bins), tb.dtype)


def energies(clips, tb, K, pad=None):
    """E_f = sum((x w)^2) of every frame-channel, framed here on its own -> [frames, K]"""
    out = []
    for x in clips:
        x = np.zeros((0, K)) if x is None else x
        rows = len(x) if pad is None else pad
        shift = tb.n_fft // 2 if tb.center else 0
        for f in range(frame_count(rows, tb.n_fft, tb.hop, tb.center)):
            r = f * tb.hop - shift + np.arange(tb.n_fft)
            ok = (r >= 0) & (r < len(x))
            fr = np.zeros((tb.n_fft, K))
            fr[ok] = x[r[ok]]
            out.append(((fr * tb.window[:, None]) ** 2).sum(0))
    return np.array(out).reshape(-1, K)


def linear_bound(E, tb):
    """the bound on |got - model| before the logarithm and the float32 rounding, [frames, K, n_bins]"""
    N = tb.n_fft
    bank = tb.dense_bank()
    Wm = np.abs(bank).sum(1) if bank is not None else np.ones(N // 2 + 1)
    per = 32 * U * math.log2(N) * N * E if tb.power == 2 else 16 * U * math.log2(N) * np.sqrt(N * E)
    return per[:, :, None] * Wm[None, None, :]


def check(be, clips, K, pad=None, misalign=0, **spec):
    """linear: within the bound; with ``log``: floor = 2^20 * the largest linear bound, every element within s 2^-19"""
    log = spec.pop("log", None)
    lin = tables(**spec)
    bound = linear_bound(energies(clips, lin, K, pad), lin)
    tb = lin if log is None else tables(log=log, floor=2.0 ** 20 * max(float(bound.max()), 2.0 ** -1000), **spec)
    got, off = run(be, clips, tb, K, pad, misalign)
    want = model(clips, tb, K, pad)
    assert got.shape == want.shape and got.dtype == want.dtype and not np.isnan(got).any()
    tol = bound if log is None else np.full(bound.shape, tb.log_scale * 2.0 ** -19)
    if tb.dtype == np.float32:
        tol = tol + 2.0 ** -23 * np.abs(want.astype(np.float64))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = float((err / np.maximum(tol, 5e-324)).max()) if err.size else 0.0
    print(f"n_fft={tb.n_fft} hop={tb.hop} K={K} power={tb.power} log={log} {tb.dtype}: worst |got - model| / bound = {worst:.3g}")
    assert (err <= tol).all(), worst
    return got, want, off


def noise(rows, K, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (rows, K))


def sine(rows, K, n_fft, b):
    r = np.arange(rows)[:, None]
    return 0.9 * np.sin(2 * np.pi * (b + np.arange(K)[None, :]) * r / n_fft)           # channel c sits on bin b + c exactly


# ---------------------------------------------------------------------------------------------------- 0. the bound, on the CPU
@pytest.mark.parametrize("N", [128, 512, 4096])
def test_numpy_rfft_is_well_inside_the_bound_and_float32_is_not(N):
    """numpy's float64 rfft against a long-double DFT (65 bins spread over 0 .. N/2) uses a small part of the power = 2 bound; a
    float32 transform of the same frame misses the bound by orders of magnitude: the bound tells float64 from anything less"""
    w = make_window("hann", N, N)
    ks = np.unique(np.linspace(0, N // 2, 65).astype(np.int64))
    n = np.arange(N, dtype=np.int64)
    ang = (np.outer(ks, n) % N).astype(np.longdouble) * (np.longdouble(-2) * np.arctan(np.longdouble(1)) * 4 / N)
    for name, x in (("noise", noise(N, 1, N)[:, 0]), ("sine", sine(N, 1, N, N // 8)[:, 0])):
        xw = x * w
        ref = ((np.cos(ang) * xw.astype(np.longdouble)).sum(1)) ** 2 + ((np.sin(ang) * xw.astype(np.longdouble)).sum(1)) ** 2
        bound = 32 * U * math.log2(N) * N * float((xw ** 2).sum())
        z = np.fft.rfft(xw)[ks]
        r64 = float(np.abs((z.real ** 2 + z.imag ** 2).astype(np.longdouble) - ref).max()) / bound
        # a float32 radix-2 transform of the same frame (numpy's own fft computes float32 input in float64)
        y = xw.astype(np.complex64)
        y = y[np.array([int(format(i, f"0{int(math.log2(N))}b")[::-1], 2) for i in range(N)])]
        size = 2
        while size <= N:
            tw = np.exp(-2j * np.pi * np.arange(size // 2) / size).astype(np.complex64)
            y = y.reshape(-1, size)
            a, b = y[:, :size // 2], (y[:, size // 2:] * tw).astype(np.complex64)
            y = np.concatenate([a + b, a - b], axis=1).astype(np.complex64).reshape(-1)
            size *= 2
        z32 = y[ks]
        p32 = z32.real.astype(np.float32) ** 2 + z32.imag.astype(np.float32) ** 2
        r32 = float(np.abs(p32.astype(np.longdouble) - ref).max()) / bound
        print(f"N={N} {name}: rfft/bound = {r64:.3g}, float32/bound = {r32:.3g}")
        assert r64 < 0.5 and r32 > 100.0, (name, r64, r32)


# ------------------------------------------------------------------------------------------------------------ 1. every plan
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("n_fft", PLANS)
def test_every_plan_matches_the_model(be, n_fft, K):
    for hop in (n_fft // 4, n_fft, 37):
        frames = (3, 5, 4)
        clips = [noise(n_fft + (frames[0] - 1) * hop + 5, K, n_fft + hop), sine(n_fft + (frames[1] - 1) * hop, K, n_fft, n_fft // 8 + 1),
                 noise(n_fft + (frames[2] - 1) * hop + hop - 1, K, hop)]
        got, want, off = check(be, clips, K, n_fft=n_fft, hop=hop)
        assert list(np.diff(off)) == list(frames)
        peak = got[frames[0]:frames[0] + frames[1]].argmax(2)           # the sine's bin, in every frame of clip 1
        assert (peak == n_fft // 8 + 1 + np.arange(K)[None, :]).all()
    hop = n_fft // 4
    clips = [noise(n_fft + 2 * hop, K, 5), sine(n_fft + 3 * hop + 1, K, n_fft, 3)]
    check(be, clips, K, n_fft=n_fft, hop=hop, power=1)
    check(be, clips, K, n_fft=n_fft, hop=hop, dtype="f32", window="hamming", misalign=4)
    check(be, clips, K, n_fft=n_fft, hop=hop, log="log10", center=True)
    check(be, clips, K, n_fft=n_fft, hop=hop, log="db", dtype="f32", power=1, win_length=n_fft - 27, window="rect")


# ------------------------------------------------------------------------------------------------------------ 2. clip shapes
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n_fft,hop", [(128, 32), (256, 37)])
def test_clip_lengths_around_n_fft_with_empty_clips_between(be, n_fft, hop, center):
    K = 2
    lens = (0, 1, n_fft - 1, n_fft, n_fft + 1, n_fft + hop)
    clips = []
    for j, rows in enumerate(lens):
        clips += [noise(rows, K, 40 + j) if rows else None, None if j % 2 else np.zeros((0, K))]
    for pad in (None, n_fft + hop, n_fft + 3 * hop + 1):          # ragged; dense, the longest clip fills it; dense with padding frames
        for kw in (dict(), dict(log="ln"), dict(dtype="f32", power=1)):
            got, want, off = check(be, clips, K, pad=pad, n_fft=n_fft, hop=hop, center=center, **kw)
            want_frames = [frame_count(rows if pad is None else pad, n_fft, hop, center) for rows in lens]
            assert list(np.diff(off))[::2] == want_frames and got.shape[0] == off[-1]
    # frames no real row reaches are all zero: +0.0
    got, _ = run(be, clips, tables(n_fft, hop, center=center), K, pad=4 * n_fft)
    F = frame_count(4 * n_fft, n_fft, hop, center)
    assert (got.reshape(len(clips), F, K, -1)[:, -1].view(np.uint64) == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 3. exact
@pytest.mark.parametrize("n_fft", [128, 1024, 4096])
def test_zero_frames_repeats_neighbours_and_float32(be, n_fft):
    K, hop = 2, n_fft // 2
    x = noise(n_fft + 2 * hop, K, 3)
    x[:, 1] = 0.0                                                   # one channel silent: exact zero next to a loud channel
    other = noise(n_fft + hop + 9, K, 4)
    neg = make_window("hann", n_fft, n_fft) - 0.3                   # (negative weights: -0.0 products)
    bank = np.zeros((3, n_fft // 2 + 1))
    bank[0, 2:9], bank[1, 5:7], bank[2, :] = 0.5, -1.0, 0.25
    for kw in (dict(), dict(power=1), dict(bank=bank), dict(window=neg, win_length=n_fft)):
        tb = tables(n_fft, hop, **kw)
        got, off = run(be, [x, None, other, x], tb, K)
        assert (got[:3, 1].view(np.uint64) == 0).all(), "an all-zero frame is +0.0"
        assert np.array_equal(got[:3].view(np.uint64), got[off[3]:].view(np.uint64)), "the same clip twice"
        alone, _ = run(be, [x], tb, K)
        assert np.array_equal(alone.view(np.uint64), got[:3].view(np.uint64)), "a clip alone and among others"
        late, _ = run(be, [other, other, x], tb, K, misalign=8)
        assert np.array_equal(late[-3:].view(np.uint64), alone.view(np.uint64))
        tb32 = tables(n_fft, hop, dtype="f32", **kw)
        got32, _ = run(be, [x, None, other, x], tb32, K)
        assert np.array_equal(got32.view(np.uint32), got.astype(np.float32).view(np.uint32)), "float32 is the rounding of float64"
    for log in ("ln", "log10", "db"):
        tb = tables(n_fft, hop, log=log, floor=1e-10)
        got, _ = run(be, [x], tb, K)
        want = np.float64(LOG_SCALE[log] * math.log(1e-10))
        assert (got[:, 1].view(np.uint64) == want.view(np.uint64)).all() and (got[:, 0] > want).all()
        got32, _ = run(be, [x], tables(n_fft, hop, log=log, floor=1e-10, dtype="f32"), K)
        assert np.array_equal(got32.view(np.uint32), got.astype(np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- 4. filterbank
@pytest.mark.parametrize("n_fft", [128, 512])
def test_filterbanks(be, n_fft):
    K, hop, nb = 2, n_fft // 4, n_fft // 2 + 1
    clips = [noise(n_fft + 3 * hop, K, 9), sine(n_fft + hop, K, n_fft, 7)]
    plain, _ = run(be, clips, tables(n_fft, hop), K)
    ident, _ = run(be, clips, tables(n_fft, hop, bank=np.eye(nb)), K)
    assert np.array_equal(plain.view(np.uint64), ident.view(np.uint64)), "the identity bank is the call without one"
    k = np.arange(nb)
    tri = lambda c, h: np.maximum(0.0, 1.0 - np.abs(k - c) / h)
    holed = np.zeros(nb)
    holed[[3, 4, 9]] = 0.5, -0.25, 2.0                           # a hole of zeros inside the band stays as weights
    bank = np.stack([np.eye(nb)[5], np.full(nb, 1.0 / nb), tri(10, 6), tri(13, 6), np.zeros(nb), holed])
    tb = tables(n_fft, hop, bank=bank)
    assert list(tb.band_len) == [1, nb, 11, 11, 0, 7] and np.array_equal(tb.dense_bank(), bank)
    got, want, _ = check(be, clips, K, n_fft=n_fft, hop=hop, bank=bank)
    assert np.array_equal(got[:, :, 0].view(np.uint64), plain[:, :, 5].view(np.uint64)), "a band of length 1 with weight 1"
    assert (got[:, :, 4].view(np.uint64) == 0).all(), "a row of zeros gives +0.0"
    check(be, clips, K, n_fft=n_fft, hop=hop, bank=bank, power=1, dtype="f32")
    check(be, clips, K, n_fft=n_fft, hop=hop, bank=bank[:4], log="log10", center=True)


# ----------------------------------------------------------------------------------------------------------- 5. status codes
def test_invalid_arguments_write_nothing(be):
    K, n_fft, hop = 2, 128, 32
    clips = [noise(200, K, 1)]
    tb = tables(n_fft, hop, bank=np.eye(65)[:4], log="ln", floor=1e-9)
    off = np.array([0, 3], np.int64)
    blank = np.full(3 * K * 4 * 8 + GUARD, 0xA5, np.uint8)
    assert (raw_call(be, clips, tb, K, off, 3, blank.copy()) != 0xA5).any()          # the valid call writes
    bad = [dict(n_fft=100), dict(n_fft=64), dict(n_fft=8192), dict(n_fft=400), dict(hop=0), dict(hop=-3), dict(K=0), dict(center=2),
           dict(power=0), dict(power=3), dict(dtype=18), dict(dtype=21), dict(dtype=10), dict(n_clips=-1), dict(out_frames=-1),
           dict(n_bands=-1), dict(n_w=-1), dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor_log=float("inf")),
           dict(s=float("nan")), dict(src=0), dict(valid=0), dict(off=0), dict(window=0), dict(out=0), dict(lo=0), dict(ln=0), dict(boff=0),
           dict(w=0)]
    for over in bad:
        raw = raw_call(be, clips, tb, K, off, 3, blank.copy(), over=over)
        assert status[0] == -1 and (raw == 0xA5).all(), (over, status[0])      # FRAD_E_INVALID, and nothing written
    # nothing is launched and nothing written for an empty call
    for over in (dict(n_clips=0), dict(out_frames=0)):
        assert (raw_call(be, clips, tb, K, off, 3, blank.copy(), over=over) == 0xA5).all(), over
