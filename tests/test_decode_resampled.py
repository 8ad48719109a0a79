"""StreamIndex.decode(..., srate=R) / decode_windows: windows of mixed-rate streams at one sample rate.

Legs.  "host": the product code over test_batch_decode.HostBridge -- helpers.OracleBridge plus the native header scan, so that the
streams are planned; it has no ``clips_resample`` (nor ``clips_window_add``), so ``window.clips_resample_host`` resamples.
"oracle": helpers.OracleBridge as it is -- no header scan either, so every stream is a fallback stream, decoded whole and
resampled as one span.  "gpu": HipBridge, one frad_clips_resample per ratio.  The streams are encoded once, with the package's
Encoder on helpers.OracleBridge: profiles 4 and 1, N = 128, six frames (profile 4: five and a tail frame of 50; profile 1:
cross-faded, ratio 16), two channels, at 44 100, 48 000 and 16 000 Hz; the target is 16 000 Hz.

Bounds.  The whole resampled stream against scipy.signal.resample_poly of decode_batch's float64 output: the bound of
test_clips_resample.py (two recursive sums of T terms, plus T * dh * max|x| for scipy's own taps).  Everything else is exact: a
window is the same terms in the same order as the whole stream, a stream already at R takes the path without ``srate``."""
import numpy as np
import pytest

from helpers import OracleBridge
from frad_python_amd import Encoder, StreamIndex, decode_batch, decode_windows, synth
from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64
from frad_python_amd.window import resample_ratio, resample_rows, resample_taps
from test_clips_resample import model_bound

R = 16000
RATES = (44100, 48000, 16000)
N, C = 128, 2
_made = {}


def _encode(profile, srate, seed):
    ratio = 16 if profile == 1 else 0
    cut = N * (ratio - 1) // ratio if ratio else N
    n = 4 * cut + N + (0 if profile == 1 else 50)
    pcm = synth.to_pcm(synth.harmonic_mix(n, C, srate, seed=seed) * 0.8, "s16le").tobytes()
    enc = Encoder(profile, srate, C, 16, N, "s16le", bridge=OracleBridge())
    enc.set_overlap_ratio(ratio)
    enc.set_loss_level(0.5)
    return enc.process(pcm).buf + enc.flush().buf


def streams():
    """profile 4 at the three rates, then profile 1 at the three rates"""
    if "streams" not in _made:
        _made["streams"] = [_encode(p, r, 40 + 3 * p + k) for p in (4, 1) for k, r in enumerate(RATES)]
    return _made["streams"]


def bridge(kind):
    if kind not in _made:
        if kind == "gpu":
            from frad_python_amd.bridge import HipBridge
            _made[kind] = HipBridge()
        elif kind == "oracle":
            _made[kind] = OracleBridge()
        else:
            from test_batch_decode import HostBridge
            _made[kind] = HostBridge()
    return _made[kind]


def index(kind):
    if ("index", kind) not in _made:
        _made["index", kind] = StreamIndex(streams(), bridge=bridge(kind))
    return _made["index", kind]


def source(kind):
    """decode_batch's float64 output of every stream, computed once"""
    if ("source", kind) not in _made:
        _made["source", kind] = [decode_batch([s], bridge=bridge(kind)).pcm[0] for s in streams()]
    return _made["source", kind]


def whole(kind, fmt=None, **kw):
    """every stream resampled whole: the yardstick of the window tests, computed once per format"""
    key = ("whole", kind, fmt, tuple(sorted(kw.items())))
    if key not in _made:
        res = index(kind).decode([(i, 0, None) for i in range(len(streams()))], srate=R, out_format=fmt, **kw)
        _made[key] = res.pcm
    return _made[key]


def windows_of(total, n_in, up, down):
    """windows of a resampled stream of ``total`` rows that can go wrong: at the start, inside the cross-fade of source frames 1 | 2
    (source rows 120 .. 127 are faded at ratio 16), at the end, past it, empty, overlapping"""
    fade = 124 * up // down
    return [(0, 10), (0, 1), (fade, 3), (fade - 2, 40), (total - 3, 3), (total - 10, 100), (total // 2, None), (total, None), (total + 5, 4),
            (7, 0), (0, total), (0, None), (total // 3, total // 3), (total // 3 + 5, total // 3)]


@pytest.fixture(params=[pytest.param("host"), pytest.param("oracle"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def kind(request):
    return request.param


def all_windows(kind):
    src = source(kind)
    wins = []
    for i, x in enumerate(src):
        up, down, _ = resample_ratio(R, RATES[i % 3])
        wins += [(i, a, n) for a, n in windows_of(resample_rows(len(x), up, down), len(x), up, down)]
    return [wins[j] for j in np.random.default_rng(4).permutation(len(wins))]


def check(res, wins, want):
    for k, (i, start, length) in enumerate(wins):
        w = want[i][start:] if length is None else want[i][start:start + length]
        got = res.pcm[k]
        assert got.dtype == w.dtype and got.shape == w.shape and got.tobytes() == np.ascontiguousarray(w).tobytes(), (k, i, start, length)
        assert res.lengths[k] == len(w)


# ---------------------------------------------------------------------------------------------------------------- lengths
def test_samples_at_comes_from_the_headers(kind):
    idx, src = index(kind), source(kind)
    assert [len(x) for x in src] == [5 * 128 + 50] * 3 + [5 * 120 + 128] * 3
    if kind == "oracle":
        assert idx.fallback == list(range(6)) and idx.samples_at(R) == [None] * 6
        return
    assert idx.fallback == [] and idx.srate == list(RATES) * 2
    want = [resample_rows(len(x), *resample_ratio(R, RATES[i % 3])[:2]) for i, x in enumerate(src)]
    assert idx.samples_at(R) == want == [len(p) for p in whole(kind)]
    assert want[0] == -(-690 * 160 // 441) == 251 and want[1] == 690 // 3 == 230 and want[2] == 690
    assert idx.samples_at(48000)[1] == 690 and idx.samples_at(48000)[2] == 3 * 690
    assert idx.frames == [6] * 6 and [p.tail_key is not None for p in idx.plans] == [True] * 3 + [False] * 3


# ------------------------------------------------------------------------------------------------------------------ scipy
def test_the_whole_stream_against_scipy(kind):
    from scipy.signal import firwin, resample_poly
    got = whole(kind)
    for i, x in enumerate(source(kind)):
        up, down, half = resample_ratio(R, RATES[i % 3])
        if up == down:
            assert got[i].tobytes() == x.tobytes()
            continue
        ref = resample_poly(x, up, down, axis=0)
        amp = np.max(np.abs(x))
        bound, T = model_bound(up, down, amp)
        dh = np.max(np.abs(resample_taps(up, down) - firwin(2 * half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up))
        assert dh <= 1e-14
        assert got[i].shape == ref.shape and got[i].dtype == np.float64
        err = np.max(np.abs(got[i] - ref))
        print(f"[scipy] stream {i} {up}/{down}: max|got - scipy| = {err:.3e} (bound {bound + T * dh * amp:.3e})")
        assert err <= bound + T * dh * amp, i


# ---------------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("fmt", (None, "s16le", "f32be", "u8"))
def test_every_window_is_the_slice_of_the_whole_resampled_stream(kind, fmt):
    wins = all_windows(kind)
    res = index(kind).decode(wins, srate=R, out_format=fmt)
    assert res.batch is None and res.fallback == (list(range(6)) if kind == "oracle" else [])
    check(res, wins, whole(kind, fmt))
    assert len({*res.lengths}) > 8 and 0 in res.lengths
    # a throw-away index
    few = wins[:9]
    check(decode_windows(streams(), few, bridge=bridge(kind), srate=R, out_format=fmt), few, whole(kind, fmt))


@pytest.mark.parametrize("fmt", (None, "s16le"))
def test_a_stream_at_the_target_rate_is_what_the_call_without_srate_gives(kind, fmt):
    idx = index(kind)
    wins = [(i, a, n) for i in (2, 5) for a, n in windows_of(len(source(kind)[i]), 0, 1, 1)]
    plain = idx.decode(wins, out_format=fmt)
    res = idx.decode(wins, out_format=fmt, srate=R)
    for k in range(len(wins)):
        assert res.pcm[k].dtype == plain.pcm[k].dtype and res.pcm[k].shape == plain.pcm[k].shape
        assert res.pcm[k].tobytes() == plain.pcm[k].tobytes(), wins[k]
    assert res.lengths == plain.lengths
    dense, pdense = idx.decode(wins[:9], out_format=fmt, srate=R, pad_to=600), idx.decode(wins[:9], out_format=fmt, pad_to=600)
    assert dense.batch.dtype == pdense.batch.dtype and dense.batch.tobytes() == pdense.batch.tobytes()


@pytest.mark.parametrize("fmt", (None, "s16le", "u8"))
def test_the_dense_batch_of_mixed_rates_has_one_shape_and_silent_padding(kind, fmt):
    T = 133
    wins = [w for w in all_windows(kind) if w[2] is not None and w[2] <= T]
    assert {w[0] for w in wins} == set(range(6))
    idx = index(kind)
    plain = idx.decode(wins, srate=R, out_format=fmt)
    res = idx.decode(wins, srate=R, out_format=fmt, pad_to=T)
    dt = np.dtype(np.float64) if fmt is None else ff_format_to_numpy_type(fmt)
    assert isinstance(res.batch, np.ndarray) and res.batch.shape == (len(wins), T, C) and res.batch.dtype == dt
    assert res.lengths == plain.lengths
    silence = from_f64(np.zeros(1), dt)[0]
    for k in range(len(wins)):
        assert res.batch[k, :res.lengths[k]].tobytes() == plain.pcm[k].tobytes(), (k, wins[k])
        assert res.batch[k, res.lengths[k]:].tobytes() == np.full((T - res.lengths[k], C), silence, dt).tobytes(), k
        assert res.pcm[k].tobytes() == plain.pcm[k].tobytes()
    check(res, wins, whole(kind, fmt))


def test_argument_errors(kind):
    idx = index(kind)
    for bad in (0, -16000):
        with pytest.raises(ValueError):
            idx.decode([(0, 0, 4)], srate=bad)
        with pytest.raises(ValueError):
            idx.samples_at(bad)
    with pytest.raises(ValueError):
        idx.decode([(0, 0, 4)], srate=16001)                     # 16001 / 44100 does not reduce: max(up, down) = 44100 > 2048
    with pytest.raises(ValueError):
        idx.decode([(1, 0, 4)], srate=2049 * 3)                  # 2049 / 16000
    assert idx.decode([(2, 0, 4)], srate=R).lengths == [4]
    assert idx.decode([(1, 0, 4)], srate=2048 * 375).lengths == [4]        # 48000 -> 768000: up = 16; the limit is on the reduced ratio
    with pytest.raises(ValueError):
        idx.decode([(0, 0, 200)], srate=R, pad_to=100)
    with pytest.raises(ValueError):
        idx.decode([(0, -1, 4)], srate=R)
    with pytest.raises(IndexError):
        idx.decode([(6, 0, 4)], srate=R)


# ------------------------------------------------------------------------------------------------------------ the device
def _garbage():
    return b"garbage-before-the-first-frame" + streams()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", (None, "s16le"))
def test_tensors_device_inflate_and_a_fallback_stream_on_the_device(fmt):
    import torch
    br = bridge("gpu")
    idx = StreamIndex(streams() + [_garbage()], bridge=br)
    assert idx.fallback == [6] and idx.samples_at(R)[6] is None and idx.samples_at(R)[:6] == index("gpu").samples_at(R)
    wins = all_windows("gpu")
    total = len(whole("gpu")[0])
    wins += [(6, a, n) for a, n in windows_of(total, 0, 160, 441)]
    want = list(whole("gpu", fmt)) + [whole("gpu", fmt)[0]]       # the fallback stream decodes to stream 0's samples
    for device_inflate in (False, True):
        host = idx.decode(wins, srate=R, out_format=fmt, device_inflate=device_inflate)
        assert host.fallback == [6]
        check(host, wins, want)
        dev = idx.decode(wins, srate=R, out_format=fmt, device_inflate=device_inflate, as_tensor=True)
        for k in range(len(wins)):
            assert isinstance(dev.pcm[k], torch.Tensor) and dev.pcm[k].is_cuda
            assert dev.pcm[k].cpu().numpy().tobytes() == host.pcm[k].tobytes(), k
    short = [w for w in wins if w[2] is not None and w[2] <= 140]
    host = idx.decode(short, srate=R, out_format=fmt, pad_to=140)
    dev = idx.decode(short, srate=R, out_format=fmt, pad_to=140, as_tensor=True)
    assert isinstance(dev.batch, torch.Tensor) and dev.batch.is_cuda and tuple(dev.batch.shape)[:2] == (len(short), 140)
    assert dev.batch.cpu().numpy().tobytes() == host.batch.tobytes() and dev.lengths == host.lengths
    check(host, short, want)
    for k in range(len(short)):
        assert dev.pcm[k].is_cuda and dev.pcm[k].cpu().numpy().tobytes() == host.pcm[k].tobytes(), k
