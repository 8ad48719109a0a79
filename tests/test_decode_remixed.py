"""StreamIndex.decode(..., channels=K, mix=...) / decode_windows: windows of mono, stereo and three-channel streams with one
channel count, and as one dense batch.

Legs as in test_decode_resampled.py.  "host": the product code over test_batch_decode.HostBridge (planned streams, no
``clips_remix``: ``window.clips_remix_host`` mixes).  "oracle": helpers.OracleBridge as it is -- no header scan, so every stream is
a fallback stream, decoded whole.  "gpu": HipBridge, one frad_clips_remix per call.  The streams are encoded once with the
package's Encoder on helpers.OracleBridge: profiles 4 and 1, N = 128, six frames (profile 1 cross-faded at ratio 16), s16le input:
1, 2 and 3 channels at 48 000 Hz, 1 and 2 channels at 44 100 Hz, 2 channels at 16 000 Hz once per profile.

No tolerance anywhere: the mix is defined term by term (include/frad_hip.h) and ``clips_remix_host`` is that definition, so
``res.pcm[k]`` is bit for bit ``from_f64(clips_remix_host(X_k, M), out_format)`` of the float64 window ``X_k`` that the same call
without ``channels`` and ``out_format`` gives; the mix is row-wise, so a window is also the slice of the whole stream decoded with
the same keywords."""
import numpy as np
import pytest

from helpers import OracleBridge
from frad_python_amd import Encoder, StreamIndex, decode_windows, synth
from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64
from frad_python_amd.window import clips_remix_host, resample_ratio
from test_batch_decode import Counting
from test_decode_resampled import windows_of

R = 16000
N = 128
# profile, channels, sample rate
CONFIGS = [(4, 1, 48000), (1, 2, 48000), (4, 3, 48000), (1, 1, 44100), (4, 2, 44100), (4, 2, 16000), (1, 2, 16000)]
STEREO = [i for i, c in enumerate(CONFIGS) if c[1] == 2]
MIX3 = {3: [[1, 0, 0], [0, 0.5, 0.5]]}
FORMATS = (None, "s16le", "f32be", "u8")
_made = {}


def _encode(profile, C, srate, seed):
    ratio = 16 if profile == 1 else 0
    cut = N * (ratio - 1) // ratio if ratio else N
    n = 4 * cut + N + (0 if profile == 1 else 50)
    pcm = synth.to_pcm(synth.harmonic_mix(n, C, srate, seed=seed) * 0.8, "s16le").tobytes()
    enc = Encoder(profile, srate, C, 16, N, "s16le", bridge=OracleBridge())
    enc.set_overlap_ratio(ratio)
    enc.set_loss_level(0.5)
    return enc.process(pcm).buf + enc.flush().buf


def streams():
    if "streams" not in _made:
        _made["streams"] = [_encode(p, C, r, 70 + k) for k, (p, C, r) in enumerate(CONFIGS)]
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


@pytest.fixture(params=[pytest.param("host"), pytest.param("oracle"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def kind(request):
    return request.param


def rule(c_in, K, mix=None):
    """the matrix the interface promises for a stream of c_in channels (the issue's rule, written out here on its own)"""
    if mix and c_in in mix:
        return np.array(mix[c_in], np.float64)
    if c_in == K:
        return np.eye(K)
    if K == 1:
        return np.full((1, c_in), 1.0 / c_in)
    assert c_in == 1
    return np.ones((K, 1))


def plain(kind, srate):
    """every stream whole, float64, without ``channels``: the source of every expectation, computed once -> (pcm, windows)"""
    key = ("plain", kind, srate)
    if key not in _made:
        pcm = index(kind).decode([(i, 0, None) for i in range(len(CONFIGS))], srate=srate).pcm
        wins = []
        for i, x in enumerate(pcm):
            up, down, _ = resample_ratio(srate, CONFIGS[i][2]) if srate else (1, 1, 0)
            wins += [(i, a, n) for a, n in windows_of(len(x), 0, up, down)]
        _made[key] = pcm, [wins[j] for j in np.random.default_rng(6).permutation(len(wins))]
    return _made[key]


def whole_mixed(kind, srate, K, mix, fmt):
    key = ("whole", kind, srate, K, fmt)
    if key not in _made:
        _made[key] = index(kind).decode([(i, 0, None) for i in range(len(CONFIGS))], srate=srate, channels=K, mix=mix, out_format=fmt).pcm
    return _made[key]


def same_bytes(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


# ---------------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("srate", (None, R))
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("K,mix", [(1, None), (2, MIX3)])
def test_every_window_is_the_mix_of_the_plain_window_and_the_slice_of_the_whole_stream(kind, K, mix, fmt, srate):
    idx = index(kind)
    src, wins = plain(kind, srate)
    assert [x.shape[1] for x in src] == [c[1] for c in CONFIGS]
    X = idx.decode(wins, srate=srate)
    res = idx.decode(wins, srate=srate, channels=K, mix=mix, out_format=fmt)
    assert res.batch is None and res.fallback == X.fallback == (list(range(len(CONFIGS))) if kind == "oracle" else [])
    assert res.lengths == X.lengths and len({*res.lengths}) > 8 and 0 in res.lengths
    whole = whole_mixed(kind, srate, K, mix, fmt)
    dt = np.dtype(np.float64) if fmt is None else ff_format_to_numpy_type(fmt)
    for k, (i, start, length) in enumerate(wins):
        m = rule(CONFIGS[i][1], K, mix)
        want = clips_remix_host(X.pcm[k], m) if fmt is None else from_f64(clips_remix_host(X.pcm[k], m), fmt)
        assert res.pcm[k].shape == (res.lengths[k], K) and res.pcm[k].dtype == dt
        assert same_bytes(res.pcm[k], want), (k, i, start, length)
        piece = whole[i][start:] if length is None else whole[i][start:start + length]
        assert same_bytes(res.pcm[k], piece), (k, i, start, length)
    # a throw-away index
    few = wins[:9]
    got = decode_windows(streams(), few, bridge=bridge(kind), srate=srate, channels=K, mix=mix, out_format=fmt)
    for k in range(len(few)):
        assert same_bytes(got.pcm[k], res.pcm[k])


def test_mix_alone_sets_the_channel_count_and_overrides_the_rule(kind):
    idx = index(kind)
    src, _ = plain(kind, None)
    swap = {2: [[0, 1], [1, 0]], 1: [[0.5], [-0.25]]}
    wins = [(0, 3, 40), (1, 5, 60), (3, 0, None)]
    res = idx.decode(wins, mix=swap)
    for k, (i, start, length) in enumerate(wins):
        x = src[i][start:] if length is None else src[i][start:start + length]
        assert same_bytes(res.pcm[k], clips_remix_host(x, swap[CONFIGS[i][1]])), k
    assert np.array_equal(res.pcm[1], src[1][5:65][:, ::-1])     # a permutation copies
    assert same_bytes(idx.decode(wins, mix=swap, channels=2).pcm[1], res.pcm[1])


# ------------------------------------------------------------------------------------------------------------ dense batch
@pytest.mark.parametrize("fmt", (None, "s16le", "u8"))
def test_one_dense_batch_of_mixed_rates_and_layouts(kind, fmt):
    T = 133
    idx = index(kind)
    wins = [w for w in plain(kind, R)[1] if w[2] is not None and w[2] <= T] + [(1, 0, T), (2, 5, T)]       # ... and two that fill their row
    assert {w[0] for w in wins} == set(range(len(CONFIGS)))
    with pytest.raises(ValueError, match="one channel count"):
        idx.decode(wins, srate=R, out_format=fmt, pad_to=T)      # without channels: as before
    ragged = idx.decode(wins, srate=R, channels=1, out_format=fmt)
    res = idx.decode(wins, srate=R, channels=1, out_format=fmt, pad_to=T)
    dt = np.dtype(np.float64) if fmt is None else ff_format_to_numpy_type(fmt)
    assert isinstance(res.batch, np.ndarray) and res.batch.shape == (len(wins), T, 1) and res.batch.dtype == dt
    assert res.lengths == ragged.lengths and 0 in res.lengths and T in res.lengths
    silence = from_f64(np.zeros(1), dt)[0]
    if fmt == "u8":
        assert silence == 128
    want = np.full((len(wins), T, 1), silence, dt)               # the ragged result padded on the host
    for k in range(len(wins)):
        want[k, :ragged.lengths[k]] = ragged.pcm[k]
        assert same_bytes(res.pcm[k], ragged.pcm[k]), (k, wins[k])
        assert np.shares_memory(res.pcm[k], res.batch) or not res.lengths[k]
    assert res.batch.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="longer than pad_to"):
        idx.decode(wins, srate=R, channels=1, out_format=fmt, pad_to=T - 1)
    if kind == "gpu":
        import torch
        dev = idx.decode(wins, srate=R, channels=1, out_format=fmt, pad_to=T, as_tensor=True)
        assert isinstance(dev.batch, torch.Tensor) and dev.batch.is_cuda and tuple(dev.batch.shape) == (len(wins), T, dt.itemsize if fmt else 1)
        assert dev.batch.cpu().numpy().tobytes() == res.batch.tobytes() and dev.lengths == res.lengths
        rag = idx.decode(wins, srate=R, channels=1, out_format=fmt, as_tensor=True)
        for k in range(len(wins)):
            assert dev.pcm[k].is_cuda and dev.pcm[k].cpu().numpy().tobytes() == res.pcm[k].tobytes(), k
            assert rag.pcm[k].is_cuda and rag.pcm[k].cpu().numpy().tobytes() == res.pcm[k].tobytes(), k
    else:
        with pytest.raises(ValueError):
            idx.decode(wins, srate=R, channels=1, as_tensor=True)


# ------------------------------------------------------------------------------------------------- reduction to the plain call
@pytest.mark.parametrize("srate", (None, R))
@pytest.mark.parametrize("fmt", (None, "s16le", "f32be"))
def test_streams_that_have_the_channel_count_give_the_bytes_of_the_plain_call(kind, fmt, srate):
    idx = index(kind)
    wins = [w for w in plain(kind, srate)[1] if w[0] in STEREO]
    base = idx.decode(wins, srate=srate, out_format=fmt)
    res = idx.decode(wins, srate=srate, out_format=fmt, channels=2)
    assert res.lengths == base.lengths and res.fallback == base.fallback
    for k in range(len(wins)):
        assert same_bytes(res.pcm[k], base.pcm[k]), (k, wins[k])
    T = 140
    short = [w for w in wins if w[2] is not None and w[2] <= T]
    base, res = idx.decode(short, srate=srate, out_format=fmt, pad_to=T), idx.decode(short, srate=srate, out_format=fmt, pad_to=T, channels=2)
    assert same_bytes(res.batch, base.batch) and res.lengths == base.lengths
    if kind == "gpu":
        base = idx.decode(short, srate=srate, out_format=fmt, pad_to=T, as_tensor=True)
        res = idx.decode(short, srate=srate, out_format=fmt, pad_to=T, as_tensor=True, channels=2)
        assert res.batch.dtype == base.batch.dtype and res.batch.shape == base.batch.shape
        assert res.batch.cpu().numpy().tobytes() == base.batch.cpu().numpy().tobytes()
        for k in range(len(short)):
            assert res.pcm[k].shape == base.pcm[k].shape and res.pcm[k].cpu().numpy().tobytes() == base.pcm[k].cpu().numpy().tobytes()


# ----------------------------------------------------------------------------------------------------------------- errors
def test_argument_errors_are_raised_before_anything_is_decoded(kind):
    """Every bridge call is counted.  What depends on the arguments alone is refused before the first call on every leg; what
    depends on a stream's channel count (3 -> 2 without a matrix, ``mix`` alone without an entry) likewise for planned streams --
    on the "oracle" leg every stream is a fallback stream, whose channel count is known only once it is decoded, so there the
    error is checked, not the count."""
    counts = {}
    idx = StreamIndex(streams(), bridge=Counting(bridge(kind), counts))
    w = [(0, 0, 10), (1, 0, 10), (2, 0, 10)]
    nan, inf = float("nan"), float("inf")
    on_arguments = [dict(channels=0), dict(channels=-1), dict(channels=1.5), dict(channels=1, mix=MIX3), dict(channels=2, mix={3: [[1, 0, 0]]}),
                    dict(mix={3: MIX3[3], 2: [[0.5, 0.5]]}), dict(channels=2, mix={3: [[1, 0, nan], [0, 1, 0]]}),
                    dict(channels=2, mix={3: [[1, 0, 0], [0, inf, 0]]}), dict(channels=2, mix={3: [[1, 0], [0, 1]]}),
                    dict(channels=2, mix={3: [1, 0, 0]}), dict(channels=2, mix={3: [[[1, 0, 0]], [[0, 1, 0]]]}), dict(channels=2, mix={0: [[], []]}),
                    dict(mix={}), dict(channels=2, mix={3: "stereo"}), dict(channels=2, mix={3: [[1, 0, 0], [0, 1]]})]
    on_streams = [dict(channels=2), dict(mix={1: [[1.0], [1.0]], 2: [[1, 0], [0, 1]]}), dict(channels=3, mix={1: [[1.0]] * 3})]
    for kw in on_arguments + on_streams:
        counts.clear()
        with pytest.raises(ValueError):
            idx.decode(w, **kw)
            print("no ValueError for", kw)
        if kind != "oracle" or kw in on_arguments:
            assert counts == {}, (kw, counts)
    counts.clear()
    with pytest.raises(ValueError, match="stream 2 has 3 channels"):
        idx.decode(w, channels=2)                               # the error names the stream and its channel count
    with pytest.raises(IndexError):
        idx.decode([(7, 0, 4)], channels=1)
    with pytest.raises(ValueError):
        idx.decode([(0, -1, 4)], channels=1)
    with pytest.raises(ValueError):
        idx.decode([(0, 0, 4)], channels=1, srate=0)
    if kind != "oracle":
        with pytest.raises(ValueError, match="longer than pad_to"):
            idx.decode([(0, 0, 4), (1, 600, None)], channels=1, pad_to=100)
        assert counts == {}
        assert idx.decode([(0, 0, 4), (1, 700, None), (2, 10 ** 6, 500)], channels=1, pad_to=100).lengths == [4, 28, 0]
    counts.clear()
    assert idx.decode(w[:2], channels=2).lengths == [10, 10] and counts     # ... and 3 -> 2 is no error where no 3-channel stream is used


# ------------------------------------------------------------------------------------------------------------ the device
@pytest.mark.gpu
def test_one_remix_launch_per_call_and_none_for_an_empty_one(monkeypatch):
    counts = {}
    idx = StreamIndex(streams(), bridge=Counting(bridge("gpu"), counts))
    wins = [(i, 3 + i, 20 + 7 * i) for i in range(len(CONFIGS))] * 2 + [(0, 10 ** 6, 4), (2, 0, 0)]
    assert len({idx.plans[w[0]].key for w in wins}) >= 2 and {CONFIGS[w[0]][1] for w in wins} == {1, 2, 3}
    assert len({CONFIGS[w[0]][2] for w in wins}) == 3            # two ratios and the streams already at R
    for kw in (dict(), dict(out_format="s16le"), dict(pad_to=80), dict(pad_to=80, as_tensor=True), dict(as_tensor=True, out_format="u8")):
        counts.clear()
        res = idx.decode(wins, srate=R, channels=1, **kw)
        assert counts["clips_remix"] == 1 and counts["clips_resample"] > 1 and counts["clips_window_add"] > 1, (kw, counts)
        assert res.lengths[-2:] == [0, 0]
    counts.clear()
    res = idx.decode([], srate=R, channels=2, pad_to=8)
    assert counts == {} and res.pcm == [] and tuple(res.batch.shape) == (0, 8, 2)
    assert idx.decode([], channels=2).pcm == [] and counts == {}
    # the C-ABI call itself, once: every call of the loaded library is counted
    from frad_python_amd import _lib
    from frad_python_amd.bridge import HipBridge
    calls = {}
    plain_idx = StreamIndex(streams(), bridge=HipBridge())
    monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), calls))
    plain_idx.decode(wins, srate=R, channels=1, pad_to=80)
    monkeypatch.undo()
    assert calls["clips_remix"] == 1, calls
