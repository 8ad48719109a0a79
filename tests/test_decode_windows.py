"""StreamIndex / decode_windows: a window is bit for bit the slice of decode_batch's output for its stream, and only the frames
it needs are decoded.

Legs, bridges and the ``encode`` helper are test_batch_decode.py's: "host" is the product code over ``HostBridge`` (no
``clips_window_add``: the windows are assembled by ``window.clips_window_host``), "gpu" is ``HipBridge``, where one launch of
frad_clips_window_add per geometry group writes every window.

Every comparison is array_equal, dtype and shape included (``same``): a window is the same arithmetic on the same decoded frames
as the whole stream.  Streams are four whole frames and a short tail of the smallest frame sizes (128, 160, 256)."""
import numpy as np
import pytest

from conftest import load_json, load_npz
from frad_python_amd import StreamIndex, decode_batch, decode_windows
from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64
from oracle import frad_oracle as fo
from test_batch_decode import Counting, _bridge, _clip, encode, frame_spans, kind, same  # noqa: F401  (kind: the fixture)

FORMATS = (None, "s16le", "f32be", "u8")
_made = {}

# profile, channels, bits, frame size, overlap ratio, ECC ratio, damaged, tail samples
CONFIGS = [(0, 1, 16, 128, 0, None, False, 50), (0, 2, 32, 128, 0, (96, 24), False, 50), (0, 2, 32, 128, 0, (96, 24), True, 50),
           (4, 2, 16, 128, 0, None, False, 50), (4, 1, 16, 128, 0, None, False, 31),
           (1, 2, 16, 128, 2, None, False, 50), (1, 1, 16, 128, 16, None, False, 50), (1, 2, 16, 128, 0, None, False, 50),
           (1, 2, 16, 160, 2, None, False, 20),               # a tail frame of another size (128) that is faded: L = 80
           (1, 1, 16, 256, 16, None, False, 50),              # ... and with L = 16
           (1, 2, 16, 128, 16, (96, 24), True, 50),
           (2, 2, 16, 128, 2, None, False, 50), (2, 1, 16, 128, 16, None, False, 50), (2, 2, 16, 192, 0, None, False, 50)]


def damage(kind, stream: bytes) -> bytes:
    """three payload bytes of every second frame flipped: repairable under fix_error"""
    s = bytearray(stream)
    for k, (h, end, flush, p_off) in enumerate(frame_spans(kind, stream)):
        if not flush and k % 2 == 0:
            for at in (3, (end - p_off) // 2, end - p_off - 2):
                s[p_off + at] ^= 0x5A
    return bytes(s)


def streams_of(kind):
    if kind not in _made:
        out = []
        for seed, (profile, C, bits, fsize, ratio, ecc, hurt, tail) in enumerate(CONFIGS):
            cut = fsize * (ratio - 1) // ratio if ratio else fsize
            s = encode(kind, _clip(3 * cut + fsize + tail, C, 300 + seed), profile, C, bits, fsize, ratio, ecc=ecc)
            out.append(damage(kind, s) if hurt else s)
        _made[kind] = out
    return _made[kind]


def index_of(kind):
    if ("index", kind) not in _made:
        _made[("index", kind)] = StreamIndex(streams_of(kind), fix_error=True, bridge=_bridge(kind))
    return _made[("index", kind)]


def whole(kind, out_format=None, device_inflate=False, fix_error=True):
    """the yardstick, computed once: decode_batch of every stream alone"""
    key = ("whole", kind, out_format, device_inflate, fix_error)
    if key not in _made:
        _made[key] = [decode_batch([s], fix_error=fix_error, out_format=out_format, device_inflate=device_inflate, bridge=_bridge(kind)).pcm[0]
                      for s in streams_of(kind)]
    return _made[key]


def windows_for(idx, i):
    """the windows of stream i that can go wrong, from its geometry"""
    cut, L, m, R, body, _ = idx._geometry(idx.plans[i])
    S = idx.samples[i]
    return [(i, 0, 10), (i, cut + max(L // 2, 1), 7),          # at 0; starting inside a fade (ratio 0: just behind a boundary)
            (i, 2 * cut, cut), (i, 2 * cut - 1, 2),            # on a cut boundary; across one
            (i, body - 5, 5 + max(L // 2, 1)),                 # ending inside the tail's fade / the flush fragment
            (i, body + 1, 2), (i, S - 3, 3), (i, body + L, None),   # inside the tail or the fragment; its end; behind the fade
            (i, S + 5, 4), (i, S, None), (i, 7, 0),            # past the end; at the end; of length 0
            (i, 3 * cut + 1, None), (i, 0, S), (i, 0, None),   # to the end; the whole stream, twice
            (i, S - 10, 100),                                  # clipped to the end
            (i, cut - 3, cut + 10), (i, cut + 2, 2 * cut)]     # two that overlap


def check(res, wins, want, msg=()):
    for k, (i, start, length) in enumerate(wins):
        w = want[i][start:] if length is None else want[i][start:start + length]
        assert same(res.pcm[k], w), msg + (k, i, start, length, res.pcm[k].shape, w.shape)
        assert res.lengths[k] == len(w)


# ----------------------------------------------------------------------------------------------- 1. windows == slices
def test_the_streams_have_the_shapes_the_cases_need(kind):
    idx = index_of(kind)
    assert idx.fallback == [] and idx.frames == [5] * len(CONFIGS)
    tails = [p.tail_key is not None for p in idx.plans]
    assert tails == [c[0] in (0, 4) or c[3] in (160, 256, 192) for c in CONFIGS]
    assert idx.channels == [c[1] for c in CONFIGS] and idx.srate == [48000] * len(CONFIGS)


@pytest.mark.parametrize("out_format", FORMATS)
def test_every_window_is_the_slice_of_decode_batch(kind, out_format):
    idx = index_of(kind)
    streams = streams_of(kind)
    wins = [w for i in range(len(streams)) if i != 4 for w in windows_for(idx, i)]           # stream 4 has no window
    wins = [wins[j] for j in np.random.default_rng(1).permutation(len(wins))]
    for device_inflate in (False, True) if kind == "gpu" else (False,):
        res = idx.decode(wins, out_format=out_format, device_inflate=device_inflate)
        assert res.fallback == [] and res.batch is None
        check(res, wins, whole(kind, out_format, device_inflate), (out_format, device_inflate))


def test_throw_away_index_chunks_and_unrepaired_streams(kind):
    streams, br = streams_of(kind), _bridge(kind)
    idx = index_of(kind)
    wins = [w for i in (1, 2, 5, 8, 10) for w in windows_for(idx, i)]
    res = decode_windows(streams, wins, fix_error=False, bridge=br)
    check(res, wins, whole(kind, fix_error=False))
    # chunks of whole windows: the streams' frames are 128 * 2 * 8 = 2 KiB each
    res = idx.decode(wins, max_batch_bytes=3 * 2048)
    check(res, wins, whole(kind))
    assert decode_windows([], [], bridge=br).pcm == [] and idx.decode([]).pcm == []


def test_argument_errors(kind):
    idx = index_of(kind)
    for bad in ((0, -1, 5), (0, 0, -1), (0, -3, None)):
        with pytest.raises(ValueError):
            idx.decode([(0, 0, 4), bad])
    with pytest.raises(IndexError):
        idx.decode([(len(CONFIGS), 0, 4)])
    if kind == "host":
        with pytest.raises(ValueError):
            idx.decode([(0, 0, 4)], as_tensor=True)


# ------------------------------------------------------------------------------------------------- 2. header lengths
def test_samples_come_from_the_headers(kind):
    idx = index_of(kind)
    assert idx.samples == [len(p) for p in whole(kind)]
    from test_stream import _inputs
    from test_p2_decode import streams_of as g7_streams
    from test_p2_encode import streams_of as g8_streams
    g3, arr, inputs = load_json("g3_streams.json"), load_npz("g3_p1_streams.npz"), _inputs()
    ref = [arr[f"{c['name']}_stream"].tobytes() if c["params"]["profile"] == 1 else fo.encode_stream(inputs[c["name"].split("_")[0]], **c["params"])
           for c in g3["cases"]]
    ref += [s for _, s, _ in g7_streams(load_npz("g7_p2.npz"))] + [d["stream"] for d in g8_streams(load_npz("g8_p2_enc.npz"))]
    assert len(ref) == 19
    br = _bridge(kind)
    ridx = StreamIndex(ref, bridge=br)
    got = decode_batch(ref, bridge=br)
    assert ridx.fallback == [] and ridx.samples == [len(p) for p in got.pcm]
    assert (ridx.frames, ridx.srate, ridx.channels) == (got.frames, got.srate, got.channels)
    wins = [(i, n // 3, n // 2) for i, n in enumerate(ridx.samples)]
    check(ridx.decode(wins), wins, got.pcm)


def test_streams_of_another_shape_fall_back_and_still_give_the_slice(kind):
    br = _bridge(kind)
    good = streams_of(kind)[3]                                                       # profile 4, stereo
    garbage = b"garbage-before-the-first-frame" + good
    changes = good + encode(kind, _clip(600, 2, 77), 4, 2, 16, 256)                  # the frame size changes mid-stream
    streams = [good, garbage, changes, streams_of(kind)[5]]
    idx = StreamIndex(streams, bridge=br)
    assert idx.fallback == [1, 2] and idx.samples[1] is None and idx.samples[2] is None and idx.samples[0] == 4 * 128 + 50
    want = decode_batch(streams, bridge=br)
    assert want.fallback == [1, 2]
    wins = [(0, 5, 100), (1, 100, 300), (2, 500, None), (3, 64, 200), (2, 0, 10), (1, 10 ** 6, 5)]
    for fmt in (None, "s16le"):
        want = decode_batch(streams, out_format=fmt, bridge=br)
        res = idx.decode(wins, out_format=fmt)
        assert res.fallback == [1, 2]
        check(res, wins, want.pcm, (fmt,))
        dense = idx.decode(wins, out_format=fmt, pad_to=700)
        assert dense.fallback == [1, 2]
        check(dense, wins, want.pcm, (fmt, "dense"))
        silence = from_f64(np.zeros(1), fmt or "f64le")[0]
        for k in range(len(wins)):
            assert (dense.batch[k, dense.lengths[k]:] == silence).all()
    assert idx.decode([(0, 0, 4)]).fallback == []                                    # only the streams a call uses


# ------------------------------------------------------------------------------------------ 3. only the needed frames
class Recording:
    """counts the payloads the bridge's decode methods are handed"""
    METHODS = {"lossless_decode": 1, "compact_decode": 1, "p1_decode_bodies": 0, "p2_decode_bodies": 0}

    def __init__(self, inner):
        self.__dict__["_inner"], self.__dict__["payloads"] = inner, 0

    def __getattr__(self, name):
        v = getattr(self._inner, name)
        if name not in self.METHODS:
            return v

        def call(*a, **k):
            self.__dict__["payloads"] += len(a[self.METHODS[name]])
            return v(*a, **k)
        return call


def frames_read(idx, i, a, b):
    """the frames rows [a, b) of stream i depend on, row by row: a row reads its own frame and, inside the fade, the one before"""
    cut, L, m, R, body, _ = idx._geometry(idx.plans[i])
    need = set()
    for r in range(a, min(b, idx.samples[i])):
        if r < body:
            need.add(r // cut)
            if r % cut < L and r >= cut:
                need.add(r // cut - 1)
        else:
            need.add("tail" if R else m - 1)
            if R and r - body < L and m:
                need.add(m - 1)
    return {(i, f) for f in need}


def test_only_the_frames_the_windows_need_are_decoded(kind):
    base = index_of(kind)
    rec = Recording(_bridge(kind))
    idx = StreamIndex(streams_of(kind), fix_error=True, bridge=rec)
    rng = np.random.default_rng(9)
    assert rec.payloads == 0                                    # the index decodes nothing
    for wins in ([w for i in (0, 5, 6, 8, 9, 11) for w in windows_for(base, i)[:8]],
                 [(i, int(a), int(n)) for i in range(len(CONFIGS)) for a, n in zip(rng.integers(0, 500, 3), rng.integers(1, 90, 3))],
                 [(5, 200, 1)], [(8, 3 * 80 + 70, 20), (8, 0, 1)], [(3, 520, 3), (3, 100, 1)]):
        rec.__dict__["payloads"] = 0
        res = idx.decode(wins)
        check(res, wins, whole(kind))
        want = set().union(*(frames_read(base, i, a, a + n if n is not None else 10 ** 9) for i, a, n in wins))
        assert rec.payloads == len(want), (wins, rec.payloads, len(want))
    # one frame's worth out of a 40-frame stream
    long = encode(kind, _clip(39 * 64 + 128, 2, 41), 1, 2, 16, 128, 2)
    rec.__dict__["payloads"] = 0
    lidx = StreamIndex([long], bridge=rec)
    want = decode_batch([long], bridge=_bridge(kind)).pcm[0]
    assert lidx.frames[0] >= 40 and lidx.samples == [len(want)] and rec.payloads == 0
    for start, n in ((64 * 17, 64), (64 * 17 + 5, 59), (64 * 17 + 63, 1)):       # the rows of frame 17 (ratio 2: all of them fade)
        rec.__dict__["payloads"] = 0
        assert same(lidx.decode([(0, start, n)]).pcm[0], want[start:start + n])
        assert rec.payloads == 2, (start, rec.payloads)


# -------------------------------------------------------------------------------------------------------- 4. the calls
def test_calls_are_decode_batchs_with_the_window_kernel_and_an_index_is_reused(kind, monkeypatch):
    streams = [streams_of(kind)[i] for i in (0, 5, 11)]                                # p0, p1 and p2
    counts = {}

    def counted(run):
        c = {}
        if kind == "host":
            out = run(Counting(_bridge(kind), c))
        else:
            from frad_python_amd import _lib
            from frad_python_amd.bridge import HipBridge
            monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), c))                  # every C-ABI call of the loaded library
            out = run(HipBridge())
            monkeypatch.undo()
        return out, c

    _, counts["batch"] = counted(lambda br: decode_batch(streams, bridge=br))
    wins = [(0, 0, None), (1, 0, None), (2, 0, None)]
    made = {}

    def first(br):
        made["idx"] = StreamIndex(streams, bridge=br)
        return made["idx"].decode(wins)
    res, counts["windows"] = counted(first)
    want = {("clips_window_add" if k == "clips_overlap_add" else k): v for k, v in counts["batch"].items()}
    print(f"[calls] decode_batch {dict(sorted(counts['batch'].items()))}\n[calls] windows {dict(sorted(counts['windows'].items()))}")
    assert counts["windows"] == want
    if kind == "gpu":
        assert want["clips_window_add"] == 3 and "clips_overlap_add" not in want
    assert counts["windows"]["asfh_scan"] == 1
    # a second call on the index: no scan, and many windows cost what three do
    if kind == "host":
        c = {}
        made["idx"].bridge = Counting(_bridge(kind), c)
        res2 = made["idx"].decode(wins * 5 + [(1, 70, 20), (2, 300, None)])
    else:
        from frad_python_amd import _lib
        c = {}
        monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), c))
        res2 = made["idx"].decode(wins * 5 + [(1, 70, 20), (2, 300, None)])
        monkeypatch.undo()
    assert c.get("asfh_scan", 0) == 0
    assert c == {k: v for k, v in counts["windows"].items() if k != "asfh_scan"}
    for k in range(3):
        assert same(res.pcm[k], res2.pcm[k]) and same(res.pcm[k], res2.pcm[k + 12])


# -------------------------------------------------------------------------------------------------- 5. the dense batch
STEREO = [i for i, c in enumerate(CONFIGS) if c[1] == 2]


@pytest.mark.parametrize("out_format", FORMATS)
def test_dense_batch(kind, out_format):
    idx = index_of(kind)
    T = 133
    wins = [w for i in STEREO for w in windows_for(idx, i) if w[2] is not None and w[2] <= T]
    wins = [wins[j] for j in np.random.default_rng(2).permutation(len(wins))]
    plain = idx.decode(wins, out_format=out_format)
    res = idx.decode(wins, out_format=out_format, pad_to=T)
    dt = np.dtype(np.float64) if out_format is None else ff_format_to_numpy_type(out_format)
    assert isinstance(res.batch, np.ndarray) and res.batch.shape == (len(wins), T, 2) and res.batch.dtype == dt
    assert res.lengths == plain.lengths and len({*res.lengths}) > 5 and 0 in res.lengths
    silence = from_f64(np.zeros(1), dt)[0]
    if out_format == "u8":
        assert silence == 128
    for k in range(len(wins)):
        assert same(res.pcm[k], plain.pcm[k]), (k, wins[k])
        assert np.shares_memory(res.pcm[k], res.batch) or not res.lengths[k]
        assert res.batch[k, :res.lengths[k]].tobytes() == plain.pcm[k].tobytes()
        assert res.batch[k, res.lengths[k]:].tobytes() == np.full((T - res.lengths[k], 2), silence, dt).tobytes(), k
    check(res, wins, whole(kind, out_format))


def test_dense_batch_refuses_what_does_not_fit(kind):
    idx = index_of(kind)
    with pytest.raises(ValueError):
        idx.decode([(0, 0, 10), (1, 0, 10)], pad_to=64)                                  # mono and stereo
    with pytest.raises(ValueError):
        idx.decode([(1, 0, 65)], pad_to=64)
    with pytest.raises(ValueError):
        idx.decode([(1, 0, None)], pad_to=64)
    assert idx.decode([(1, 0, 64), (1, 10 ** 6, 3)], pad_to=64).lengths == [64, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("out_format", (None, "s16le"))
def test_as_tensor_keeps_the_results_on_the_device(out_format):
    import torch
    idx = index_of("gpu")
    wins = [w for i in STEREO for w in windows_for(idx, i) if w[2] is not None and w[2] <= 140]
    host = idx.decode(wins, out_format=out_format)
    dev = idx.decode(wins, out_format=out_format, as_tensor=True)
    for k in range(len(wins)):
        assert isinstance(dev.pcm[k], torch.Tensor) and dev.pcm[k].is_cuda
        assert dev.pcm[k].cpu().numpy().tobytes() == host.pcm[k].tobytes(), k
    host = idx.decode(wins, out_format=out_format, pad_to=140)
    dev = idx.decode(wins, out_format=out_format, pad_to=140, as_tensor=True)
    assert isinstance(dev.batch, torch.Tensor) and dev.batch.is_cuda and tuple(dev.batch.shape)[:2] == (len(wins), 140)
    assert dev.batch.cpu().numpy().tobytes() == host.batch.tobytes() and dev.lengths == host.lengths
    for k in range(len(wins)):
        assert dev.pcm[k].is_cuda and dev.pcm[k].cpu().numpy().tobytes() == host.pcm[k].tobytes(), k
