"""StreamIndex.decode(..., features=spec): spectrograms of the decoded, resampled and mixed windows.

Legs as in test_decode_remixed.py.  "host": the product code over test_batch_decode.HostBridge (no ``clips_spectrum``:
``spectral.clips_spectrum_host`` computes).  "oracle": helpers.OracleBridge -- no header scan, every stream a fallback stream.
"gpu": HipBridge, one frad_clips_spectrum per call.  The streams: profiles 0 and 1, N = 128, mono and stereo, 48 000, 44 100 and
16 000 Hz, and one with garbage before its first frame, which is a fallback stream on every leg.

Tolerance: test_clips_spectrum's, against ``clips_spectrum_host(X_k, spec)`` of the float64 window ``X_k`` that the same call without
``features`` gives (on the host legs the stage is that function, so the difference is zero there)."""
import numpy as np
import pytest

from frad_python_amd import StreamIndex
from frad_python_amd.spectral import Spectral, clips_spectrum_host, frame_count, hz_to_mel, mel_filterbank, mel_to_hz
from test_batch_decode import Counting
from test_clips_spectrum import energies, linear_bound
from test_decode_remixed import _encode, bridge, kind  # noqa: F401  (kind: the fixture)

R = 16000
# profile, channels, sample rate
CONFIGS = [(0, 1, 48000), (1, 2, 48000), (0, 2, 16000), (1, 1, 44100), (0, 2, 44100)]
GARBAGE = len(CONFIGS)                                         # stream 5: stream 2 behind garbage
_made = {}


def streams():
    if "streams" not in _made:
        made = [_encode(p, C, r, 170 + k) for k, (p, C, r) in enumerate(CONFIGS)]
        _made["streams"] = made + [b"garbage-before-the-first-frame" + made[2]]
    return _made["streams"]


def index(kind):
    if kind not in _made:
        _made[kind] = StreamIndex(streams(), bridge=bridge(kind))
    return _made[kind]


def windows(idx, srate):
    """a few windows per stream at ``srate``: short ones (below n_fft), long ones, one to the end, an empty one"""
    wins = []
    for i in range(len(streams())):
        profile, _, rate = CONFIGS[2 if i == GARBAGE else i]
        n = 4 * 120 + 128 if profile == 1 else 4 * 128 + 128 + 50                   # test_decode_remixed._encode's lengths
        n = -(-n * srate // rate) if srate else n
        wins += [(i, 0, None), (i, 7, 100), (i, n // 3, 128), (i, n // 2, 129), (i, 3, n // 2), (i, n, 5)]
    return wins


def within(got, x, spec, srate, rows=None):
    """got against the model of the float64 window x: the linear bound, or with a logarithm (floor = 2^20 * the largest linear
    bound, set by the caller through ``spec_for``) s * 2^-19; float32 adds 2^-23 |model|"""
    tb = spec.tables(srate)
    want = clips_spectrum_host(x, tb, rows=rows)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    tol = linear_bound(energies([x], tb, x.shape[1], rows), tb) if not tb.log_scale else np.full(want.shape, tb.log_scale * 2.0 ** -19)
    if tb.dtype == np.float32:
        tol = tol + 2.0 ** -23 * np.abs(want.astype(np.float64))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= tol).all(), float((err / np.maximum(tol, 5e-324)).max())


def floor_for(xs, rate, **kw):
    """2^20 * the largest linear bound over the windows xs of the spec without its logarithm"""
    lin = Spectral(128, 32, **kw)
    tb = lin.tables(rate)
    return 2.0 ** 20 * max(float(linear_bound(energies([x], tb, x.shape[1]), tb).max()) for x in xs if len(x) >= 128)


SPECS = [dict(dtype="f64"), dict(power=1, center=True, window="hamming"), dict(n_mels=20, mel="slaney", norm="slaney", dtype="f64")]


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("srate,channels", [(R, 1), (None, 2), (R, None)])
def test_features_are_the_model_of_the_plain_window(kind, srate, channels):
    idx = index(kind)
    use = range(len(streams())) if channels else [i for i in range(len(streams())) if i == GARBAGE or CONFIGS[i][1] == 2]
    if srate is None:                                            # (a mel bank without srate needs one rate: the 48 kHz streams)
        use = [i for i in use if i != GARBAGE and CONFIGS[i][2] == 48000]
    wins = [w for w in windows(idx, srate) if w[0] in use]
    X = idx.decode(wins, srate=srate, channels=channels)
    K = channels or 2
    rate = srate or 48000
    assert {x.shape[1] for x in X.pcm} == {K} and (kind != "oracle") == (X.fallback != sorted({w[0] for w in wins}))
    if srate:
        assert GARBAGE in X.fallback
    for kw in SPECS + [dict(log="log10", n_mels=20), dict(log="db", dtype="f64", power=1), dict(log="ln", win_length=100, window="rect")]:
        if "log" in kw:
            kw = dict(kw, floor=floor_for([np.asarray(x) for x in X.pcm], rate, **{k: v for k, v in kw.items() if k != "log"}))
        spec = Spectral(128, 32, **kw)
        if kind == "oracle" and srate is None and spec.needs_rate:
            with pytest.raises(ValueError, match="srate="):       # a fallback stream's rate is not known from its headers
                idx.decode(wins, channels=channels, features=spec)
            continue
        res = idx.decode(wins, srate=srate, channels=channels, features=spec)
        assert res.pcm is None and res.batch is None and res.feature_batch is None
        assert res.lengths == X.lengths and res.fallback == X.fallback
        assert res.frames == [frame_count(n, 128, 32, spec.center) for n in X.lengths]
        assert (0 in res.frames) == (not spec.center) and max(res.frames) > 4
        for k in range(len(wins)):
            assert isinstance(res.features[k], np.ndarray) and res.features[k].shape == (res.frames[k], K, 20 if spec.n_mels else 65)
            within(res.features[k], np.asarray(X.pcm[k]), spec, rate)


@pytest.mark.parametrize("center", [False, True])
def test_dense_batch_frames_keep_pcm_and_tensors(kind, center):
    T = 300
    idx = index(kind)
    wins = [w for w in windows(idx, R) if w[2] is not None and w[2] <= T] + [(2, 0, T)]
    spec = Spectral(128, 37, center=center, n_mels=12, log="log10", floor=1e-9, dtype="f32")
    plain = idx.decode(wins, srate=R, channels=1, pad_to=T)
    ragged = idx.decode(wins, srate=R, channels=1, features=spec, keep_pcm=True)
    res = idx.decode(wins, srate=R, channels=1, pad_to=T, features=spec, keep_pcm=True)
    F = 1 + T // 37 if center else 1 + (T - 128) // 37
    assert res.feature_batch.shape == (len(wins), F, 1, 12) and res.feature_batch.dtype == np.float32 and ragged.feature_batch is None
    want_frames = [(1 + n // 37) if center else (1 + (n - 128) // 37 if n >= 128 else 0) for n in plain.lengths]
    assert res.frames == ragged.frames == want_frames and res.lengths == plain.lengths
    assert 0 in plain.lengths and T in plain.lengths and any(0 < n < 128 for n in plain.lengths)
    silent = np.float32(np.log10(1e-9))
    for k in range(len(wins)):
        assert res.features[k].shape == ragged.features[k].shape == (res.frames[k], 1, 12)
        assert np.array_equal(res.features[k].view(np.uint32), ragged.features[k].view(np.uint32)), "ragged and pad_to: the same bits"
        assert np.shares_memory(res.features[k], res.feature_batch) or not res.frames[k]
        first_silent = -(-(plain.lengths[k] + (64 if center else 0)) // 37)        # frames that start behind the window's last row
        assert (res.feature_batch[k, first_silent:] == silent).all()
        # keep_pcm: the plain call's results
        assert np.array_equal(res.pcm[k].view(np.uint64), plain.pcm[k].view(np.uint64))
        assert np.array_equal(ragged.pcm[k].view(np.uint64), plain.pcm[k].view(np.uint64))
    assert res.batch.tobytes() == plain.batch.tobytes() and ragged.batch is None
    if kind == "gpu":
        import torch
        dev = idx.decode(wins, srate=R, channels=1, pad_to=T, features=spec, keep_pcm=True, as_tensor=True)
        assert isinstance(dev.feature_batch, torch.Tensor) and dev.feature_batch.is_cuda and dev.batch.is_cuda
        assert dev.feature_batch.cpu().numpy().tobytes() == res.feature_batch.tobytes() and dev.batch.cpu().numpy().tobytes() == res.batch.tobytes()
        assert tuple(dev.feature_batch.permute(0, 2, 3, 1).shape) == (len(wins), 1, 12, F)
        rag = idx.decode(wins, srate=R, channels=1, features=spec, as_tensor=True)
        for k in range(len(wins)):
            assert dev.features[k].cpu().numpy().tobytes() == res.features[k].tobytes()
            assert rag.features[k].is_cuda and rag.features[k].cpu().numpy().tobytes() == res.features[k].tobytes()
        assert rag.pcm is None and dev.frames == res.frames
    else:
        with pytest.raises(ValueError):
            idx.decode(wins, srate=R, channels=1, features=spec, as_tensor=True)


# ------------------------------------------------------------------------------------------------------------ the mel bank
@pytest.mark.parametrize("mel", ["htk", "slaney"])
@pytest.mark.parametrize("srate,n_fft,n_mels,fmin,fmax", [(16000, 512, 40, 0.0, None), (48000, 2048, 80, 20.0, 16000.0), (16000, 128, 10, 100.0, 7000.0)])
def test_mel_filterbank(mel, srate, n_fft, n_mels, fmin, fmax):
    bank = mel_filterbank(srate, n_fft, n_mels, fmin, fmax, mel, None)
    assert bank.shape == (n_mels, n_fft // 2 + 1) and bank.dtype == np.float64 and (bank >= 0).all()
    top = srate / 2 if fmax is None else fmax
    edges = mel_to_hz(np.linspace(hz_to_mel(fmin, mel), hz_to_mel(top, mel), n_mels + 2), mel)
    assert abs(edges[0] - fmin) < 1e-9 and abs(edges[-1] - top) < 1e-9 and (np.diff(edges) > 0).all()
    assert np.allclose(mel_to_hz(hz_to_mel(edges, mel), mel), edges, rtol=1e-13, atol=1e-10)
    f = np.arange(n_fft // 2 + 1) * srate / n_fft
    for m, row in enumerate(bank):
        nz = np.flatnonzero(row)
        if nz.size:
            assert (np.diff(nz) == 1).all(), "banded"
            assert (f[nz] > edges[m]).all() and (f[nz] < edges[m + 2]).all() and row.max() <= 1.0
    # neighbouring triangles sum to 1 between their centres
    between = (f >= edges[1]) & (f <= edges[-2])
    assert between.any() and np.abs(bank.sum(0)[between] - 1.0).max() < 1e-12
    slaney = mel_filterbank(srate, n_fft, n_mels, fmin, fmax, mel, "slaney")
    assert np.abs(slaney - bank * (2.0 / (edges[2:] - edges[:-2]))[:, None]).max() < 1e-12
    # the area of a normalised triangle is 1 as an integral: its bin sum times the bin width is, where the bins sample it well
    width = srate / n_fft
    wide = (edges[2:] - edges[:-2]) > 16 * width
    if wide.any():
        assert np.abs(slaney[wide].sum(1) * width - 1.0).max() < 0.02
    try:
        import librosa
    except ImportError:
        return                                                   # (that one comparison needs librosa)
    want = librosa.filters.mel(sr=srate, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax, htk=mel == "htk", norm=None, dtype=np.float64)
    assert np.abs(bank - want).max() < 1e-9


def test_mel_formulas():
    assert abs(hz_to_mel(1000.0, "htk") - 2595.0 * np.log10(1 + 1000 / 700)) < 1e-12
    assert hz_to_mel(1000.0, "slaney") == 15.0 and hz_to_mel(200.0, "slaney") == 3.0
    assert abs(hz_to_mel(6400.0, "slaney") - 42.0) < 1e-12


# ----------------------------------------------------------------------------------------------------------------- errors
def test_spec_errors_at_construction():
    nan, inf = float("nan"), float("inf")
    for args, kw in [((400, 160), {}), ((64, 16), {}), ((8192, 16), {}), ((129, 16), {}), ((512.0, 16), {}), ((512, 0), {}), ((512, -1), {}),
                     ((512, 1.5), {}), ((512, 160), dict(win_length=513)), ((512, 160), dict(win_length=0)), ((512, 160), dict(window="kaiser")),
                     ((512, 160), dict(window=np.ones(511))), ((512, 160), dict(window=np.full(512, nan))), ((512, 160), dict(power=3)),
                     ((512, 160), dict(power=0)), ((512, 160), dict(dtype="f16")), ((512, 160), dict(log="log2", floor=1.0)),
                     ((512, 160), dict(log="ln")), ((512, 160), dict(log="ln", floor=0.0)), ((512, 160), dict(log="db", floor=-1.0)),
                     ((512, 160), dict(log="db", floor=nan)), ((512, 160), dict(log="db", floor=inf)), ((512, 160), dict(n_mels=0)),
                     ((512, 160), dict(n_mels=40, mel="bark")), ((512, 160), dict(n_mels=40, norm="l2")), ((512, 160), dict(n_mels=40, fmin=-1.0)),
                     ((512, 160), dict(n_mels=40, fmin=4000.0, fmax=4000.0)), ((512, 160), dict(n_mels=4, filterbank=np.ones((4, 257)))),
                     ((512, 160), dict(filterbank=np.ones((4, 256)))), ((512, 160), dict(filterbank=np.ones(257))),
                     ((512, 160), dict(filterbank=np.full((2, 257), inf))), ((512, 160), dict(filterbank="mel"))]:
        with pytest.raises(ValueError):
            Spectral(*args, **kw)
            print("no ValueError for", args, kw)
    spec = Spectral(512, 160, win_length=400, filterbank=np.eye(257)[[3, 3, 200]] + np.eye(257)[[9, 3, 200]])
    tb = spec.tables()
    assert list(tb.band_lo) == [3, 3, 200] and list(tb.band_len) == [7, 1, 1] and tb.band_w[1:6].tolist() == [0.0] * 5   # the hole stays
    assert (spec.window[:56] == 0).all() and spec.window[56] == 0.0 and spec.window[57] > 0 and (spec.window[456:] == 0).all()
    with pytest.raises(ValueError):
        Spectral(512, 160, n_mels=40, fmax=9000.0).tables(16000)                     # beyond half the rate
    with pytest.raises(ValueError):
        Spectral(512, 160, n_mels=40).tables()


def test_argument_errors_are_raised_before_anything_is_decoded(kind):
    """Every bridge call is counted: what the arguments and the planned streams' headers decide is refused before the first call."""
    counts = {}
    idx = StreamIndex(streams(), bridge=Counting(bridge(kind), counts))
    spec, mels = Spectral(128, 32), Spectral(128, 32, n_mels=10)
    w = [(0, 0, 200), (1, 0, 200)]
    cases = [(w, dict(features=spec, channels=1, out_format="s16le")), (w, dict(features=spec, channels=1, pad_to=127)),
             (w, dict(features="mel", channels=1)), (w, dict(features=spec, channels=1, srate=0)), (w, dict(keep_pcm=True)),
             (w, dict(features=spec, channels=0)), (w, dict(features=Spectral(128, 32, n_mels=10, fmax=9000.0), srate=R, channels=1))]
    planned = [(w, dict(features=spec)),                         # one and two channels
               ([(0, 0, 200), (3, 0, 200)], dict(features=mels, channels=1)),          # 48 000 and 44 100 Hz under a mel bank
               ([(0, 0, 200), (GARBAGE, 0, 200)], dict(features=mels, channels=1))]    # a fallback stream's rate is not known
    for wins, kw in cases + planned:
        counts.clear()
        with pytest.raises(ValueError):
            idx.decode(wins, **kw)
            print("no ValueError for", kw)
        if kind != "oracle" or (wins, kw) in cases:
            assert counts == {}, (kw, counts)
    with pytest.raises(IndexError):
        idx.decode([(9, 0, 4)], features=spec)
    counts.clear()
    short = [(0, 0, 60), (1, 0, 64)]
    res = idx.decode(short, features=mels, channels=1, srate=R, pad_to=128)          # ... and pad_to = n_fft is one frame
    assert res.feature_batch.shape == (2, 1, 1, 10) and counts and res.frames == [0, 0]
    centred = idx.decode(short, features=Spectral(128, 32, center=True), channels=1, pad_to=64, srate=R)     # centred frames need no full frame
    assert centred.feature_batch.shape == (2, 3, 1, 65)


# ------------------------------------------------------------------------------------------------------------ the device
@pytest.mark.gpu
def test_one_spectrum_launch_per_call_and_none_for_an_empty_one(monkeypatch):
    counts = {}
    idx = StreamIndex(streams(), bridge=Counting(bridge("gpu"), counts))
    wins = [(i, 3 + i, 150 + 7 * i) for i in range(len(CONFIGS))] * 2 + [(0, 10 ** 6, 4), (2, 0, 0)]
    assert len({idx.plans[w[0]].key for w in wins}) >= 2 and {CONFIGS[w[0]][1] for w in wins} == {1, 2}
    assert len({CONFIGS[w[0]][2] for w in wins}) == 3            # two ratios and the streams already at R
    spec = Spectral(128, 32, n_mels=16, log="log10", floor=1e-10)
    for kw in (dict(), dict(pad_to=200), dict(pad_to=200, as_tensor=True), dict(as_tensor=True, keep_pcm=True)):
        counts.clear()
        res = idx.decode(wins, srate=R, channels=1, features=spec, **kw)
        assert counts["clips_spectrum"] == 1 and counts["clips_remix"] == 1 and counts["clips_resample"] > 1, (kw, counts)
        assert res.frames[-2:] == [0, 0]
    counts.clear()
    res = idx.decode([], srate=R, channels=1, features=spec, pad_to=200)
    assert counts == {} and res.features == [] and tuple(res.feature_batch.shape) == (0, 3, 1, 16)
    res = idx.decode([(0, 10 ** 6, 4)], srate=R, channels=1, features=spec)          # a window without a frame
    assert "clips_spectrum" not in counts and res.features[0].shape == (0, 1, 16)
    # the C-ABI call itself, once: every call of the loaded library is counted
    from frad_python_amd import _lib
    from frad_python_amd.bridge import HipBridge
    calls = {}
    plain_idx = StreamIndex(streams(), bridge=HipBridge())
    monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), calls))
    plain_idx.decode(wins, srate=R, channels=1, pad_to=200, features=spec)
    monkeypatch.undo()
    assert calls["clips_spectrum"] == 1, calls
