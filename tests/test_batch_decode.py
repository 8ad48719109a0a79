"""decode_batch: many complete streams in one device pass == one fresh Decoder per stream, bit for bit.

Legs as in test_stream.py.  "host": the product decode_batch / Decoder with oracle arithmetic behind a local subclass of
helpers.OracleBridge (plus the interpreted HIP build for what the oracle has not: the header scan, Reed-Solomon, profile 2);
it has no ``clips_overlap_add``, so the assembly runs on the host with Decoder._overlap_host's arithmetic.  "gpu": HipBridge,
where one launch of frad_clips_overlap_add assembles every group.

The header byte cannot express ``overlap_ratio == 1`` (0 means none, b > 0 means b + 1: tools/asfh.py:120), so that case of the
batched-shape rule is checked on the classifier with a hand-made scanner row (test_fallback_is_exact)."""
import hashlib

import numpy as np
import pytest

from conftest import load_json, load_npz
from helpers import OracleBridge
from frad_python_amd import Decoder, Encoder, decode_batch, synth
from frad_python_amd import batch as fb
from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type
from oracle import frad_oracle as fo

FORMATS = (None, "s16le", "s32be", "f32be", "u8")


class HostBridge(OracleBridge):
    """OracleBridge + the native header scan, Reed-Solomon and profile 2 of the CPU interpreter build (numpy buffers).  No
    fused run methods and no clips_overlap_add: every cross-fade is the oracle's / the host's numpy arithmetic."""

    def __init__(self):
        super().__init__()
        from test_ecc import EmuEcc
        from test_p2_encode import EmuP2Enc
        self._rs, self._p2 = EmuEcc(), EmuP2Enc()
        self.scan_lib = self._rs.lib
        self.rs_repair = self._rs.rs_repair
        self.p2_decode_bodies = self._p2.p2_decode_bodies


class HostBridgeOla(HostBridge):
    """... with the group-level entry point, so that the counting test sees it called"""

    def clips_overlap_add(self, frames, clip_frame0, N, C, ratio, tails, tail_off, tail_rows, out_format=None, tail_win=None, as_tensor=False):
        return fb.clips_overlap_host(frames, clip_frame0, N, C, ratio, tails, tail_off, tail_rows, out_format)


_made = {}


def _bridge(kind, enc=False):
    key = (kind, enc and kind == "host")
    if key not in _made:
        if kind == "gpu":
            from frad_python_amd.bridge import HipBridge
            _made[key] = HipBridge()
        elif enc:
            from test_encoder_ecc import EmuEncoderBridge       # the Encoder's side on the CPU (not under test here)
            _made[key] = EmuEncoderBridge()
        else:
            _made[key] = HostBridge()
    return _made[key]


@pytest.fixture(params=[pytest.param("host"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def kind(request):
    return request.param


def encode(kind, pcm: bytes, profile, C, bits, fsize, ratio=0, ecc=None, le=False, srate=48000, fmt="s16le"):
    enc = Encoder(profile, srate, C, bits, fsize, fmt, bridge=_bridge(kind, enc=True), allow_profile2=True, allow_ecc=ecc is not None)
    enc.set_little_endian(le)
    enc.set_overlap_ratio(ratio)
    enc.set_loss_level(0.5)
    if ecc is not None:
        enc.set_ecc(True, ecc)
    return enc.process(pcm).buf + enc.flush().buf


def per_stream(bridge, stream, fix_error=False, out_format=None, device_inflate=False):
    """The contract's yardstick: a fresh Decoder driven as the reference's caller drives it (src/decoder.py:70-88)."""
    dec = Decoder(fix_error, bridge=bridge, out_format=out_format, device_inflate=device_inflate)
    r = dec.process(stream)
    pieces, frames = [r.pcm], r.frames
    while True:
        before = len(dec.buffer)
        r = dec.process(b"")
        frames += r.frames
        if not r.pcm.size and len(dec.buffer) >= before:
            break
        pieces.append(r.pcm)
    srate, ch = dec.asfh.srate, dec.asfh.channels
    pieces.append(dec.flush().pcm)
    dt = np.dtype(np.float64) if out_format is None else ff_format_to_numpy_type(out_format)
    pieces = [p.reshape(-1, ch) for p in pieces if p.size]
    pcm = np.concatenate(pieces).astype(pieces[0].dtype) if pieces else np.zeros((0, ch), dt)
    return pcm, frames, srate, ch


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def frame_spans(kind, stream):
    """[(header_off, end, is_flush)] of a clean stream, from the native scanner"""
    rows, _, why = _bridge(kind).scan_lib.asfh_scan(stream, 0)
    assert why == 0
    return [(r[0], r[1] + r[2], bool(r[13]), r[1]) for r in rows.tolist()]


# ------------------------------------------------------------------------------------------------ 1. against the reference
def test_reference_streams_in_one_call(kind):
    from test_stream import _inputs
    from test_p2_decode import streams_of as g7_streams
    from test_p2_encode import streams_of as g8_streams
    g3, arr, inputs = load_json("g3_streams.json"), load_npz("g3_p1_streams.npz"), _inputs()
    cases = []                                                  # (name, stream, check)
    for c in g3["cases"]:
        p = c["params"]
        s = arr[f"{c['name']}_stream"].tobytes() if p["profile"] == 1 else fo.encode_stream(inputs[c["name"].split("_")[0]], **p)
        cases.append((c["name"], s, c))
    for i, (ratio, s, pcm) in enumerate(g7_streams(load_npz("g7_p2.npz"))):
        cases.append((f"g7_{i}", s, pcm))
    for i, d in enumerate(g8_streams(load_npz("g8_p2_enc.npz"))):
        cases.append((f"g8_{i}", d["stream"], d["pcm"]))
    assert len(cases) == 19
    batch = cases * 3
    order = np.random.default_rng(20261016).permutation(len(batch))
    batch = [batch[i] for i in order]
    res = decode_batch([s for _, s, _ in batch], bridge=_bridge(kind))
    assert res.fallback == []
    for i, (name, s, c) in enumerate(batch):
        got = res.pcm[i]
        if isinstance(c, dict):
            want = fo.decode_stream(s)
            assert res.frames[i] == c["frames"] and list(got.shape) == c["decoded_shape"], name
            assert res.srate[i] == c["params"]["srate"] and res.channels[i] == c["params"]["channels"], name
            if kind == "host" or c["params"]["profile"] == 4:
                assert hashlib.sha256(np.ascontiguousarray(got).astype("<f8").tobytes()).hexdigest() == c["decoded_sha256"], name
                continue
        else:
            want = c
            assert got.shape == want.shape, name
            assert res.frames[i] == sum(1 for f in frame_spans(kind, s) if not f[2]), name
        err = np.max(np.abs(got - want))
        print(f"[reference] {name}: max|got - want| = {err:.3e}")
        assert err <= 1e-12 * max(1.0, np.max(np.abs(want))), (name, err)


# --------------------------------------------------------------------------- 2. against the per-stream Decoder, bit for bit
def _clip(n, C, seed):
    return synth.to_pcm(synth.harmonic_mix(n, C, 48000, seed=seed) * 0.8, "s16le").tobytes()


def _clip_set(kind):
    """>= 40 encoder-written streams, every one of the batched shape"""
    if ("clips", kind) in _made:
        return _made[("clips", kind)]
    rng = np.random.default_rng(4242)
    streams, seed = [], 0
    configs = [(0, 2, 32, 2048, 0, False), (0, 1, 16, 512, 0, True), (0, 3, 64, 640, 0, False),
               (4, 2, 16, 2048, 0, False), (4, 1, 24, 512, 0, True), (4, 3, 12, 640, 0, False),
               (1, 2, 16, 2048, 16, False), (1, 1, 16, 512, 2, False), (1, 3, 16, 640, 0, False), (1, 2, 24, 512, 16, False),
               (2, 2, 16, 512, 16, False), (2, 1, 16, 512, 2, False), (2, 3, 16, 640, 0, False), (2, 2, 20, 2048, 16, False)]
    for profile, C, bits, fsize, ratio, le in configs:
        cut = fsize * (ratio - 1) // ratio if ratio else fsize
        heavy = profile == 2 and fsize == 2048 and kind == "host"             # the interpreter: one short clip of this size
        lengths = [int(rng.integers(1, 3 * fsize + fsize // 2)) for _ in range(1 if heavy else 3)]
        if not heavy:
            lengths += [fsize // 3, 2 * cut + fsize, fsize]                  # shorter than a frame, exactly k*cut + N, one frame
        for n in lengths:
            seed += 1
            streams.append(encode(kind, _clip(n, C, seed), profile, C, bits, fsize, ratio, le=le))
    streams.append(b"")
    # Reed-Solomon protected streams with a few payload bytes flipped (repairable: 3 bytes in one 120-byte block)
    for profile, C, bits, fsize, ratio in ((0, 2, 32, 512, 0), (1, 2, 16, 512, 16), (4, 1, 16, 640, 0), (0, 2, 32, 512, 0)):
        for n in (fsize * 2 + 100, fsize + 333):
            seed += 1
            s = bytearray(encode(kind, _clip(n, C, seed), profile, C, bits, fsize, ratio, ecc=(96, 24)))
            for k, (h, end, flush, p_off) in enumerate(frame_spans(kind, bytes(s))):
                if not flush and k % 2 == 0:
                    for at in (3, 40, 77):
                        s[p_off + at] ^= 0x5A
            streams.append(bytes(s))
    # one frame whose payload zlib rejects
    s = bytearray(encode(kind, _clip(2048 * 3, 2, 999), 1, 2, 16, 2048, 16))
    h, end, flush, p_off = frame_spans(kind, bytes(s))[1]
    s[p_off:end] = b"\xff" * (end - p_off)
    streams.append(bytes(s))
    assert len(streams) >= 40
    _made[("clips", kind)] = streams
    return streams


@pytest.mark.parametrize("device_inflate", [False, True])
@pytest.mark.parametrize("out_format", FORMATS)
def test_equals_the_per_stream_decoder_bit_for_bit(kind, out_format, device_inflate):
    streams = _clip_set(kind)
    br = _bridge(kind)
    res = decode_batch(streams, fix_error=True, out_format=out_format, device_inflate=device_inflate, bridge=br)
    assert res.fallback == []
    tails = set()
    for i, s in enumerate(streams):
        want, frames, srate, ch = per_stream(br, s, True, out_format, device_inflate)
        assert same(res.pcm[i], want), (i, out_format, res.pcm[i].dtype, res.pcm[i].shape, want.dtype, want.shape)
        assert (res.frames[i], res.srate[i], res.channels[i]) == (frames, srate, ch), i
        tails.add(want.shape)
    assert len(tails) > 30                                      # the clips really differ in length


def test_unrepaired_ecc_streams_equal_too(kind):
    streams = [s for s in _clip_set(kind)][-9:]
    br = _bridge(kind)
    res = decode_batch(streams, fix_error=False, bridge=br)
    assert res.fallback == []
    for i, s in enumerate(streams):
        assert same(res.pcm[i], per_stream(br, s)[0]), i


# ------------------------------------------------------------------------------------------------------- 3. fallback is exact
def test_fallback_is_exact(kind):
    br = _bridge(kind)
    good = [encode(kind, _clip(3000, 2, 1), 4, 2, 16, 1024), encode(kind, _clip(5000, 2, 2), 1, 2, 16, 2048, 16),
            encode(kind, _clip(1500, 1, 3), 0, 1, 32, 512), b""]
    p1a = encode(kind, _clip(2 * 1024 + 2048, 2, 4), 1, 2, 16, 2048, 2)          # three whole frames of 2048, ratio 2 (L = 1024)
    p1b = encode(kind, _clip(300, 2, 5), 1, 2, 16, 512, 2)                       # one frame of 512 rows < L
    short_tail = b"".join(p1a[h:e] for h, e, fl, _ in frame_spans(kind, p1a) if not fl) + p1b
    ratio_change = bytearray(encode(kind, _clip(2048 * 4, 2, 6), 1, 2, 16, 2048, 16))
    spans = frame_spans(kind, bytes(ratio_change))
    assert len([s for s in spans if not s[2]]) >= 4
    ratio_change[spans[2][0] + 11] = 1                                            # third frame: overlap_ratio 2
    mono, stereo = encode(kind, _clip(2000, 1, 7), 4, 1, 16, 1024), encode(kind, _clip(2000, 2, 8), 4, 2, 16, 1024)
    other_rate = encode(kind, _clip(2000, 1, 9), 4, 1, 16, 1024, srate=44100)
    bad = [b"garbage-before-the-first-frame" + good[0], good[2][:-10], mono + other_rate, bytes(ratio_change), short_tail,
           good[1][:len(good[1]) - 5]]
    # A change of the channel count inside one buffer: the Decoder, like the reference (decoder.py:94-99: `info` IS `asfh` after
    # the first header, so the `crit` return never fires), ends in numpy's concatenate error.  The stream is not of the batched
    # shape, goes to the per-stream Decoder, and decode_batch ends the same way.
    rows, _, _ = br.scan_lib.asfh_scan(mono + stereo, 0)
    assert fb._plan(rows.tolist(), mono + stereo, False) is None
    try:
        want = per_stream(br, mono + stereo)
    except ValueError:
        with pytest.raises(ValueError):
            decode_batch([good[0], mono + stereo], bridge=br)
    else:
        res = decode_batch([good[0], mono + stereo], bridge=br)
        assert res.fallback == [1] and same(res.pcm[1], want[0])
    streams = [good[0], bad[0], good[1], bad[1], bad[2], good[2], bad[3], good[3], bad[4], bad[5], good[1]]
    want_fallback = [1, 3, 4, 6, 8, 9]
    for fmt in (None, "s16le"):
        res = decode_batch(streams, out_format=fmt, bridge=br)
        assert res.fallback == want_fallback
        for i, s in enumerate(streams):
            want, frames, srate, ch = per_stream(br, s, out_format=fmt)
            assert same(res.pcm[i], want), (i, fmt)
            assert (res.frames[i], res.srate[i], res.channels[i]) == (frames, srate, ch), i
    # overlap_ratio == 1 cannot be written into a header; the classifier refuses it all the same
    rows, _, _ = br.scan_lib.asfh_scan(good[1], 0)
    rows = rows.tolist()
    assert fb._plan(rows, good[1], False) is not None
    rows[0] = rows[0][:10] + (1,) + rows[0][11:]
    assert fb._plan(rows, good[1], False) is None


# ------------------------------------------------------------------------------------------------------ 4. it really batches
class Counting:
    def __init__(self, inner, counts):
        self.__dict__["_inner"], self.__dict__["_counts"] = inner, counts

    def __getattr__(self, name):
        v = getattr(self._inner, name)
        if name == "scan_lib" and v is not None:
            return Counting(v, self._counts)
        if not callable(v) or name in ("torch", "core"):
            return v

        def call(*a, **k):
            self._counts[name] = self._counts.get(name, 0) + 1
            return v(*a, **k)
        return call


def _one_key_clips(kind, n):
    tails = (700, 1300, 1900)
    return [encode(kind, _clip(2 * 1920 + tails[i % 3], 2, 100 + i), 1, 2, 16, 2048, 16) for i in range(n)]


def test_call_counts_do_not_depend_on_the_number_of_streams(kind, monkeypatch):
    counts = []
    for n in (8, 64):
        streams = _one_key_clips(kind, n)
        c = {}
        if kind == "host":
            br = Counting(HostBridgeOla(), c)
        else:
            from frad_python_amd import _lib
            from frad_python_amd.bridge import HipBridge
            monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), c))          # every C-ABI call of the loaded library
            br = HipBridge()
        res = decode_batch(streams, bridge=br)
        monkeypatch.undo()
        assert res.fallback == [] and len({p.shape for p in res.pcm}) == 3
        for i in (0, 1, 2, n - 1):
            assert same(res.pcm[i], per_stream(_bridge(kind), streams[i])[0])
        counts.append(c)
        print(f"[calls] {n} clips: {dict(sorted(c.items()))}")
    assert counts[0] == counts[1]
    assert counts[0]["clips_overlap_add"] == 1 and counts[0]["asfh_scan"] == 1


# ---------------------------------------------------------------------------------------------------- 6. at size, on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("profile", [1, 0])
def test_at_size_on_the_gpu(profile, monkeypatch):
    import torch
    from frad_python_amd import _lib
    from frad_python_amd.bridge import HipBridge
    n = 256
    base = synth.harmonic_mix(48000 + n, 2, 48000, seed=77)
    args = (1, 2, 16, 2048, 16) if profile == 1 else (0, 2, 32, 2048, 0)
    streams = [encode("gpu", synth.to_pcm(np.ascontiguousarray(base[i:i + 48000]) * (0.5 + 0.4 * (i % 7) / 7), "s16le").tobytes(), *args)
               for i in range(n)]
    br = HipBridge()
    res = decode_batch(streams, bridge=br)
    assert res.fallback == []
    want = [per_stream(br, s)[0] for s in streams]
    for i in range(n):
        assert same(res.pcm[i], want[i]), i
    for fmt in (None, "s16le"):
        host = decode_batch(streams, out_format=fmt, bridge=br)
        dev = decode_batch(streams, out_format=fmt, as_tensor=True, bridge=br)
        for i in range(n):
            assert isinstance(dev.pcm[i], torch.Tensor) and dev.pcm[i].is_cuda
            assert dev.pcm[i].cpu().numpy().tobytes() == host.pcm[i].tobytes(), (fmt, i)
            if fmt is None:
                assert same(host.pcm[i], want[i])
    c = {}
    monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), c))
    per = (res.frames[0] * 2048 if profile == 1 else 48000) * 2 * 8            # float64 bytes of one clip's decoded frames
    chunked = decode_batch(streams, max_batch_bytes=86 * per, bridge=HipBridge())   # 256 clips -> 86 + 86 + 84
    monkeypatch.undo()
    assert c["clips_overlap_add"] == 3, c
    for i in range(n):
        assert same(chunked.pcm[i], want[i]), i
