"""Profile 1 (K7 / K8): the quantiser's integers against the oracle EXACTLY, over the depths, PCM types, rates and loss levels below.

The rule for a kernel integer g against the oracle's unrounded value y (``aux["y"]`` for q, ``aux["v"]`` for tq):
g == round(y), unless the oracle itself cannot decide.  "Cannot decide": the kernels' DCT is not pocketfft's, the two agree to
dX = 8 eps64 log2(N) max|X| per channel (the profile-0 transform bound of DESIGN.md section 5).  With every coefficient moved
by +-dX a band's RMS moves by at most dX, so each threshold gets the interval [t(rms - dX), t(rms + dX)] widened by a relative
1e-13 (the last bits of pow and log), the ramps between thresholds (monotone in both ends) the matching interval, and each
bin the interval [quant((X - dX) / div), quant((X + dX) / div)] with div taken at the end that widens it.  Only where the two
ends round to different integers may g be either of them -- on at most max(1, 1e-5 x values) values of a case, which keeps the
interval from hiding a failure (the oracle alone is undecided on 0 of 32768 values of the signals below).  The same rule holds
for tq through the threshold interval.  f32 / f16 PCM (the reference's mixed-precision path, 2 % contract) is not covered here.
"""
import functools

import numpy as np
import pytest

from helpers import EmuBackend, GpuBackend
from frad_python_amd import synth
from oracle import frad_oracle as fo

_backends = {}
EPS64 = 2.0 ** -52
REL = 1e-13


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param not in _backends:
        _backends[request.param] = EmuBackend() if request.param == "emu" else GpuBackend()
    return _backends[request.param]


# ---------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------
def _band_thresholds(mag, dx, srate, loss, rel):
    """mask_thresholds (p1tools.py:18-33) with every band's RMS moved by ``dx`` and the result by the factor 1 + ``rel``"""
    edges = fo.band_edges(len(mag), srate)
    thres = np.zeros(fo.N_BANDS)
    for i in range(fo.N_BANDS):
        sub = mag[edges[i]:edges[i + 1]]
        if len(sub) == 0:
            break
        rms = max(np.sqrt(np.mean(sub ** 2)) + dx, 0.0)
        thres[i] = max(rms ** fo.SPREAD_ALPHA, min(fo.hearing_threshold(i), 1.0)) * loss * (1.0 + rel)
    return thres


def _allowed(got, want, lo, hi, what, unrounded):
    """-> (excused, undecided); asserts got == want except where round(lo) != round(hi), there either of the two"""
    got = np.asarray(got).astype(np.int64).reshape(-1)
    want = np.asarray(want).astype(np.int64).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} values, the oracle has {want.shape}"
    assert np.all(lo <= unrounded) and np.all(unrounded <= hi), f"{what}: the oracle's value lies outside its own interval"
    r_lo, r_hi = np.round(lo).astype(np.int64), np.round(hi).astype(np.int64)
    open_ = r_lo != r_hi
    bad = (got != want) & ~(open_ & ((got == r_lo) | (got == r_hi)))
    if bad.any():
        at = np.flatnonzero(bad)
        show = ", ".join(f"[{i}] {got[i]} for {unrounded[i]:.9g}" for i in at[:6])
        raise AssertionError(f"{what}: {at.size} of {got.size} values are not the oracle's: {show}")
    return int(np.count_nonzero(got != want)), int(np.count_nonzero(open_))


def check_exact(q, tq, wq, wt, aux, what):
    """One frame: the kernel's q [N*C] / tq [27*C] against ``fo.p1_analogue_pre``'s (wq, wt, aux).  -> (excused, undecided)."""
    freqs = aux["freqs"]
    assert freqs.dtype == np.float64, "f32 / f16 PCM keeps its own contract"
    C, dlen = freqs.shape
    scale, srate, loss = 2.0 ** (aux["bits"] - 1), aux["srate"], aux["loss"]
    y_lo, y_hi, v_lo, v_hi = (np.zeros((C, n)) for n in (dlen, dlen, fo.N_BANDS, fo.N_BANDS))
    for c in range(C):
        X = freqs[c]
        dX = 8 * EPS64 * np.log2(dlen) * np.max(np.abs(X))
        mag = np.abs(X * scale)
        assert np.array_equal(_band_thresholds(mag, 0.0, srate, loss, 0.0), aux["thres"][c]), "comparator != oracle"
        t_lo, t_hi = _band_thresholds(mag, -dX * scale, srate, loss, -REL), _band_thresholds(mag, dX * scale, srate, loss, REL)
        d_lo, d_hi = (fo.spread_thresholds(t, dlen, srate) for t in (t_lo, t_hi))
        d_lo, d_hi = np.where(d_lo == 0, np.inf, d_lo), np.where(d_hi == 0, np.inf, d_hi)
        x_lo, x_hi = (X - dX) * scale, (X + dX) * scale
        y_lo[c] = fo.quant(x_lo / np.where(x_lo > 0, d_hi, d_lo))
        y_hi[c] = fo.quant(x_hi / np.where(x_hi > 0, d_lo, d_hi))
        v_lo[c], v_hi[c] = (fo.dequant(np.log(t.clip(min=1.0)) / np.log(np.e / 2)) for t in (t_lo, t_hi))
    eq, uq = _allowed(q, wq, y_lo.T.ravel(), y_hi.T.ravel(), f"q {what}", aux["y"])
    et, ut = _allowed(tq, wt, v_lo.T.ravel(), v_hi.T.ravel(), f"tq {what}", aux["v"])
    return eq + et, uq + ut


def check_case(items, what):
    """A case: (q, tq, wq, wt, aux) per frame, the last three from ``fo.p1_analogue_pre``.  The cap on excused values holds for
    the case as a whole; the counts are printed.  -> excused"""
    excused = undecided = values = 0
    for f, (q, tq, wq, wt, aux) in enumerate(items):
        e, u = check_exact(np.asarray(q).reshape(-1), np.asarray(tq).reshape(-1), wq, wt, aux, f"{what} frame {f}")
        excused += e; undecided += u; values += wq.size + wt.size
    print(f"[p1 exact] {what}: excused {excused}, oracle undecided on {undecided} of {values} values")
    assert excused <= max(1, 1e-5 * values), f"{what}: {excused} of {values} values excused"
    return excused


def check_frames(q, tq, frames_f64, bits, srate, loss, what):
    """A case: q [F, N, C], tq [F, 27, C] against the oracle on each float64 frame -> excused"""
    return check_case([(q[f], tq[f]) + fo.p1_analogue_pre(frame, bits, srate, loss) for f, frame in enumerate(frames_f64)], what)


def frames_of(raw, fmt, F, N, C, raw_be=True, hop=None, n_valid=None):
    """the float64 frames the reference would see: to_f64 (with or without its big-endian quirk), then zero padding to N"""
    dt = fo.pcm_dtype(fmt)
    hop, nv = N if hop is None else hop, N if n_valid is None else n_valid
    flat = raw.reshape(-1, C)
    out = []
    for f in range(F):
        x = fo.to_f64(flat[f * hop:f * hop + nv], dt, be_int_quirk=raw_be)
        out.append(np.pad(x, ((0, N - nv), (0, 0))) if nv < N else x)
    return out


def run_case(be, raw, fmt, F, N, C, bits, srate, loss, what, raw_be=True, hop=None, n_valid=None, offset=0):
    q, tq = be.p1_analogue(np.ascontiguousarray(raw), fmt, F, N, C, bits, srate, loss, frame_stride=hop, n_valid=n_valid,
                           raw_be=raw_be, offset=offset)
    check_frames(q, tq, frames_of(raw, fmt, F, N, C, raw_be, hop, n_valid), bits, srate, loss, what)
    return q, tq


# ---------------------------------------------------------------------------------------------------------------------
# signals
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mix(n, C, srate):
    x = synth.harmonic_mix(n, C, srate, seed=7)
    x.setflags(write=False)
    return x


def _tonal(seeds, N, C, srate):
    """near-full-scale harmonic frames, one seed per frame: band RMS within a few dB of the PCM type's peak"""
    return np.concatenate([synth.harmonic_mix(N, C, srate, seed=s, peak=0.99) for s in seeds])


def _signal(name, F, N, C, srate=48000):
    """-> (PCM array, format)"""
    n = F * N
    rng = np.random.default_rng(11)
    if name == "lsb":
        return rng.integers(-1, 2, (n, C)).astype("<i2"), "s16le"
    if name in ("f64_1e6", "f64_1e-6"):
        return (_mix(n, C, srate) * float(name[4:])).astype("<f8"), "f64le"
    x = _mix(n, C, srate).copy()
    if name == "silence":
        x[:] = 0.0
    elif name == "silent_channel":
        x[:, C - 1] = 0.0
    elif name == "silent_frame":
        x[N:2 * N] = 0.0
    elif name == "dc":
        x[:] = 0.999
    elif name == "impulse_first":
        x[:] = 0.0; x[0, 0] = 0.9
    elif name == "impulse_last":
        x[:] = 0.0; x[n - 1, C - 1] = -0.9
    elif name == "square":
        x[:] = np.where((np.arange(n) // 32) % 2 == 0, 1.0, -1.0)[:, None]
    elif name == "noise":
        x[:] = rng.uniform(-1.0, 1.0, (n, C))
    else:
        assert name == "mix", name
    return synth.to_pcm(x, "s16le"), "s16le"


WAVE_GEOMS = [(2048, 2, 2), (2048, 1, 3), (1024, 2, 2)]          # (N, C, F): the wave kernel (mono: a half-empty last wave), one-shot
DEPTHS = [8, 12, 16, 24, 32, 48, 64, 20]                         # 20: not a profile-1 depth, treated as 16 (profile1.py:16)
FORMATS = ["u8", "s8", "u16le", "u16be", "s16be", "s32le", "s32be", "u32le", "u32be", "s64le", "s64be", "u64be", "f64le", "f64be"]
RATES = list(fo.COMPACT_SRATES) + [37800]                        # 37800: between two table entries, 44100 in the reference
LOSSES = [0.0, -2.0, 0.553, 5.065, 50.0]                         # 0: clamped to 0.125; negative: its absolute value
SIGNALS = ["silence", "silent_channel", "silent_frame", "dc", "impulse_first", "impulse_last", "square", "noise", "lsb",
           "f64_1e6", "f64_1e-6"]


def _is_be_int(fmt):
    return fmt.endswith("be") and fmt[0] in "us"


def _cases():
    out = []
    for (N, C, F) in WAVE_GEOMS:
        g = f"{N}x{C}"
        out += [(f"{g}-bits{b}", N, C, F, "mix", "s16le", b, 48000, 1.0, True) for b in DEPTHS]
        for fmt in FORMATS:
            out.append((f"{g}-{fmt}", N, C, F, "mix", fmt, 16, 48000, 1.0, True))
            if _is_be_int(fmt):
                out.append((f"{g}-{fmt}-normalised", N, C, F, "mix", fmt, 16, 48000, 1.0, False))
        # unscaled big-endian integers at deeper depths (s16be at 24 bit, loss 1: its peak is beyond the band-code table)
        out += [(f"{g}-{fmt}-bits{b}", N, C, F, "mix", fmt, b, 48000, 1.0, True) for fmt, b in (("s16be", 24), ("s16be", 32), ("s32be", 32))]
        # the same at the smallest loss level, where the band codes stay inside the table and only the size of the band RMS
        # decides which kernel may run: scaled RMS in [2^32, 2^40) puts rms^4 beyond float32, where the wave kernel's threshold
        # keeps its float32 seed (1e-6 off) and a bin within 1e-4 of a tie goes wrong.  Near-full-scale tonal frames get there;
        # the seeds are frames in which such a bin exists.  Peak 2^31 (u16be at 16 bit, s16le at 32 bit) is the last the wave
        # kernel holds exactly.
        if N == 2048:
            for fmt, b, seeds in {2: (("s16be", 24, (1229, 1259)), ("s32be", 8, (1047, 1066)), ("u32be", 8, (1047, 1066))),
                                  1: (("s16be", 24, (1044, 1045, 1046)), ("u16be", 24, (1044, 1045, 1046)), ("s32be", 8, (1044, 1045, 1046)))}[C]:
                out.append((f"{g}-{fmt}-bits{b}-loss0-tonal", N, C, len(seeds), "tonal:" + ",".join(map(str, seeds)), fmt, b, 48000, 0.0, True))
        out += [(f"{g}-{fmt}-bits{b}-loss0-tonal", N, C, F, "tonal:1035,1036,1037"[:6 + 5 * F - 1], fmt, b, 48000, 0.0, True)
                for fmt, b in (("u16be", 16), ("s16le", 32))]
        out += [(f"{g}-rate{r}", N, C, F, "mix", "s16le", 16, r, 1.0, True) for r in RATES]
        out += [(f"{g}-loss{l}", N, C, F, "mix", "s16le", 16, 48000, l, True) for l in LOSSES]
        out += [(f"{g}-{s}", N, C, 3 if s == "silent_frame" else F, s, None, 16, 48000, 1.0, True) for s in SIGNALS
                if not (s == "silent_channel" and C == 1)]
    # one-shot at 2048 (three channels), mixed radix, several frames per block (7 frames: no multiple of it), channel groups
    for (N, C, F) in [(2048, 3, 2), (640, 1, 2), (128, 2, 7), (4096, 6, 2)]:
        g = f"{N}x{C}"
        out += [(f"{g}-bits{b}", N, C, F, "mix", "s16le", b, 48000, 0.553, True) for b in (16, 64)]
        out += [(f"{g}-s32be", N, C, F, "mix", "s32be", 16, 48000, 1.0, True), (f"{g}-noise", N, C, F, "noise", None, 16, 48000, 5.065, True)]
    return [pytest.param(*c[1:], id=c[0]) for c in out]


@pytest.mark.parametrize("N,C,F,signal,fmt,bits,srate,loss,raw_be", _cases())
def test_p1_quantiser_is_exact(be, N, C, F, signal, fmt, bits, srate, loss, raw_be):
    if be.name == "emu" and N > 2048:
        pytest.skip("emulator: channel groups run on the device only, as in test_parity_p1")
    if signal.startswith("tonal:"):
        raw, sfmt = synth.to_pcm(_tonal([int(v) for v in signal[6:].split(",")], N, C, srate), fmt), fmt
    else:
        raw, sfmt = _signal(signal, F, N, C, srate)
        if fmt not in (None, sfmt):
            raw = synth.to_pcm(_mix(F * N, C, srate), fmt)
    run_case(be, raw, fmt or sfmt, F, N, C, bits, srate, loss, f"{N}x{C} {signal} {fmt or sfmt} bits {bits} {srate} Hz loss {loss}", raw_be)


@pytest.mark.parametrize("C,F", [(1, 37), (2, 23)])
def test_p1_batch_equals_its_frames_alone(be, C, F):
    """A batch longer than a block's waves, silent frames scattered in it: exact, and frame by frame what the frame gives alone."""
    N = 2048
    x = _mix(F * N, C, 48000).copy().reshape(F, N, C)
    x[[0, 5, 6, 17, F - 1]] = 0.0
    raw = synth.to_pcm(x.reshape(-1, C), "s16le")
    q, tq = run_case(be, raw, "s16le", F, N, C, 16, 48000, 1.0, f"batch of {F} x {C} ch")
    for f in range(F):
        q1, tq1 = be.p1_analogue(np.ascontiguousarray(raw[f * N:(f + 1) * N]), "s16le", 1, N, C, 16, 48000, 1.0)
        assert np.array_equal(q1[0], q[f]) and np.array_equal(tq1[0], tq[f]), f"frame {f} alone differs from the batch"


def test_p1_stride_padding_and_alignment(be):
    N, C = 2048, 2
    raw = synth.to_pcm(_mix(3 * N, C, 48000), "s16le")
    run_case(be, raw[:2 * 1920 + N], "s16le", 3, N, C, 16, 48000, 1.0, "hop 1920", hop=1920)           # the encoder's overlap read
    run_case(be, raw[:2 * N], "s16le", 2, N, C, 16, 48000, 1.0, "n_valid 1500", n_valid=1500)          # zero padding: not the wave kernel
    run_case(be, raw[:2 * N], "s16le", 2, N, C, 16, 48000, 1.0, "PCM at +2 bytes", offset=2)            # unaligned rows: not the wave kernel


# ---------------------------------------------------------------------------------------------------------------------
# K8 on what the deep depths and unscaled integers make: every frame beyond the wave kernel's tables (codes and |q| >= 256)
# ---------------------------------------------------------------------------------------------------------------------
def _decode_marked(be, raw, fmt, F, N, C, bits, srate=48000):
    frames = frames_of(raw, fmt, F, N, C)
    ints = [fo.p1_analogue_pre(x, bits, srate, 1.0)[:2] for x in frames]
    q = np.stack([a.reshape(N, C) for a, _ in ints]).astype(np.int32)
    tq = np.stack([b.reshape(27, C) for _, b in ints]).astype(np.int32)
    assert np.abs(q).max() >= 256 and tq.max() >= 256, "the case no longer leaves the tables"      # or it silently stops testing that route
    dec = be.p1_digital(q, tq, N, C, bits, srate)
    fb = fo.P1_DEPTHS.index(bits)
    for f in range(F):
        ref = fo.p1_digital_post(q[f].reshape(-1), tq[f].reshape(-1), fb, C, srate, N)
        assert np.all(np.isfinite(ref))
        assert np.max(np.abs(dec[f] - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), f"frame {f}"


@pytest.mark.parametrize("C", [2, 1])
@pytest.mark.parametrize("fmt,bits", [("s16le", 48), ("s16le", 64), ("s32be", 16)])
def test_p1_decode_of_marked_frames(be, C, fmt, bits):
    _decode_marked(be, synth.to_pcm(_mix(3 * 2048, C, 48000), fmt), fmt, 3, 2048, C, bits)


def test_p1_decode_more_marked_frames_than_the_redo_grid(be):
    """300 marked frames: the kernel behind the wave kernel has a grid of 256 blocks, which then loop over the list"""
    _decode_marked(be, synth.to_pcm(_mix(300 * 2048, 1, 48000), "s16le"), "s16le", 300, 2048, 1, 64)
