"""encode_batch: many complete clips in one device pass == one fresh Encoder per clip, byte for byte.

Legs as in test_batch_decode.py.  "host": the product encode_batch / Encoder over test_encoder_ecc.EmuEncoderBridge (oracle
arithmetic for the transforms, the interpreted HIP build for profile 2, Reed-Solomon and the checksums); it has no
``clips_frame_cut``, so the frames are cut by numpy slicing in batch.py.  "gpu": HipBridge, where one launch of
frad_clips_frame_cut cuts the whole frames of every clip.

Every input is 48 kHz, N = 128 (a legal frame size of every profile), a seeded ``synth.harmonic_mix``.

The fallback case.  The forward DCT is scaled by 1 / N, so no coefficient of a full-scale input (|x| <= 1: every integer format)
exceeds 1 at ANY frame size, and 1 fits every storage float: a full-scale impulse does not escalate at N = 128 or anywhere
else (checked below on the oracle for N = 128 and 2048).  Only a float format can hold a sample beyond full scale; the test
uses ``f64be`` and an impulse of 1e8 at N = 128, whose coefficients reach 7.8e5 > 65504, the largest 16-bit storage float."""
import numpy as np
import pytest

from test_batch_decode import Counting
from frad_python_amd import Encoder, encode_batch, synth
from frad_python_amd import batch as fb
from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type
from frad_python_amd.fourier.profiles import compact
from oracle import frad_oracle as fo

N, SRATE = 128, 48000
LENGTHS = [0, 1, 50, 127, 128, 129, 4 * 128, 4 * 128 + 50, 4 * 64 + 128]     # 4 * 64 + 128: k * cut + N at overlap ratio 2
_made = {}


def _bridge(kind):
    if kind not in _made:
        if kind == "gpu":
            from frad_python_amd.bridge import HipBridge
            _made[kind] = HipBridge()
        else:
            from test_encoder_ecc import EmuEncoderBridge
            _made[kind] = EmuEncoderBridge()
    return _made[kind]


@pytest.fixture(params=[pytest.param("host"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def kind(request):
    return request.param


def clip_set(C, fmt, seed=7, extra=5, stray=True):
    """the clip lengths of the contract and `extra` seeded random ones below 1000, shuffled; every third clip carries trailing
    bytes that do not fill a sample-frame (the Encoder drops them at flush)"""
    rng = np.random.default_rng(seed)
    lengths = LENGTHS + [int(n) for n in rng.integers(1, 1000, extra)]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    step = ff_format_to_numpy_type(fmt).itemsize * C
    clips = []
    for i, n in enumerate(lengths):
        pcm = synth.to_pcm(synth.harmonic_mix(n, C, SRATE, seed=seed * 100 + i) * 0.8, fmt).tobytes() if n else b""
        clips.append(pcm + (b"\x7f" * (1 + i % max(step - 1, 1)) if stray and step > 1 and i % 3 == 0 else b""))
    return clips


def per_clip(bridge, clip, profile, C, bits, fmt, overlap=0, le=False, ecc=None, device_deflate=False, loss=0.5, fsize=N):
    """The contract's yardstick: a fresh Encoder with the same settings on the same bridge."""
    e = Encoder(profile, SRATE, C, bits, fsize, fmt, bridge=bridge, allow_profile2=profile == 2, allow_ecc=ecc is not None,
                device_deflate=device_deflate)
    e.set_overlap_ratio(overlap)
    e.set_loss_level(loss)
    e.set_little_endian(le)
    if ecc is not None:
        e.set_ecc(True, ecc)
    a, b = e.process(clip), e.flush()
    return a.buf + b.buf, a.samples + b.samples


def batched(bridge, clips, profile, C, bits, fmt, overlap=0, le=False, ecc=None, device_deflate=False, loss=0.5, fsize=N, **kw):
    return encode_batch(clips, profile, SRATE, C, bits, fsize, fmt, overlap_ratio=overlap, loss_level=loss, little_endian=le,
                        ecc_ratio=ecc, allow_profile2=profile == 2, device_deflate=device_deflate, bridge=bridge, **kw)


def reads_back(br, stream, profile, ecc, C, samples):
    """The stream decodes without an error: with the oracle where it reads the stream (its decode_stream takes profiles 0, 1 and
    4 without ECC), else -- profile 2, Reed-Solomon -- with the product Decoder over the same host bridge."""
    if profile != 2 and ecc is None:
        pcm = fo.decode_stream(stream)
    else:
        from frad_python_amd import Decoder
        d = Decoder(bridge=br)
        pieces = [d.process(stream).pcm, d.flush().pcm]
        pcm = np.concatenate([x.reshape(-1, C) for x in pieces])
    assert pcm.shape[1] == C and pcm.shape[0] >= samples, (pcm.shape, samples)


def check(kind, profile, C, bits, fmt, fallback=(), extra=5, read_back=99, **kw):
    br = _bridge(kind)
    clips = clip_set(C, fmt, seed=profile * 10 + C, extra=extra)
    res = batched(br, clips, profile, C, bits, fmt, **kw)
    assert res.fallback == list(fallback)
    n_frames = 0
    for i, c in enumerate(clips):
        want, samples = per_clip(br, c, profile, C, bits, fmt, **kw)
        assert res.streams[i] == want, (i, len(c), len(res.streams[i]), len(want))
        assert res.samples[i] == samples, (i, len(c))
        n_frames += res.frames[i]
        if kind == "host" and res.frames[i] and read_back > 0:
            reads_back(br, want, profile, kw.get("ecc"), C, samples)
            read_back -= 1
    assert n_frames > len(clips)
    return res


# ---------------------------------------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("C,le", [(1, False), (2, False), (1, True), (2, True)])
def test_profile0(kind, C, le):
    check(kind, 0, C, 16, "s16le", le=le)


@pytest.mark.parametrize("le", [False, True])
def test_profile4(kind, le):
    check(kind, 4, 2, 16, "s16le", le=le)


@pytest.mark.parametrize("overlap", [0, 2, 16])
def test_profile1_stereo(kind, overlap):
    check(kind, 1, 2, 16, "s16le", overlap=overlap)


def test_profile2_behind_its_keyword(kind):
    # (the host leg interprets the profile-2 kernels lane by lane: two random lengths, and two streams read back)
    check(kind, 2, 2, 16, "s16le", overlap=2, extra=2, read_back=2)


@pytest.mark.parametrize("profile", [0, 1])
def test_reed_solomon(kind, profile):
    check(kind, profile, 2, 16, "s16le", overlap=2 if profile else 0, ecc=(96, 24))


@pytest.mark.gpu
def test_device_deflate():
    check("gpu", 1, 2, 16, "s16le", overlap=2, device_deflate=True)


@pytest.mark.parametrize("fmt", ["s16le", "u8", "f32be", "s32be"])
@pytest.mark.parametrize("profile", [0, 1])
def test_pcm_formats(kind, profile, fmt):
    # s32be: the reference does not scale big-endian integers (pcmformat.py:34-47), so the samples are of the order 2^31 and every
    # profile-0 frame needs a deeper storage float than 16 bits; at 64 bits none does, and the clips stay in the batch
    check(kind, profile, 2, 64 if (profile, fmt) == (0, "s32be") else 16, fmt, overlap=2 if profile else 0)


def test_unscaled_big_endian_integers_at_16_bits_all_fall_back(kind):
    clips = clip_set(2, "s32be", seed=2)
    check(kind, 0, 2, 16, "s32be", fallback=[i for i, c in enumerate(clips) if len(c) >= 8])


def test_settings_are_clamped_as_the_setters_clamp_them(kind, capsys):
    br = _bridge(kind)
    clips = clip_set(2, "s16le", seed=3, extra=1)[:6]
    res = batched(br, clips, 1, 2, 16, "s16le", overlap=1, loss=-0.01, ecc=(0, 300))     # -> ratio 2, level 0.125, ECC 96 / 24
    capsys.readouterr()
    for i, c in enumerate(clips):
        assert res.streams[i] == per_clip(br, c, 1, 2, 16, "s16le", overlap=2, loss=0.125, ecc=(96, 24))[0], i


# ---------------------------------------------------------------------------------- 2. the condition of the padded tail groups
SIGNED_AND_FLOAT = [f for f in ("s8", "s16le", "s16be", "s32le", "s32be", "s64le", "s64be", "f16le", "f16be", "f32le", "f32be",
                                "f64le", "f64be")]
UNSIGNED = ["u8", "u16le", "u16be", "u32le", "u32be", "u64le", "u64be"]


def test_which_formats_pad():
    assert all(fb.zero_bytes_are_zero(f) for f in SIGNED_AND_FLOAT) and not any(fb.zero_bytes_are_zero(f) for f in UNSIGNED)
    for f in SIGNED_AND_FLOAT:                                   # the rule itself: zero bytes convert to +0.0
        z = fo.to_f64(np.zeros(4, ff_format_to_numpy_type(f)), fo.pcm_dtype(f))
        assert not z.any() and not np.signbit(z).any(), f


class EmuPayload:
    """one frame through the interpreted kernels (frad_p{1,2}_analogue, the Exp-Golomb-Rice coder) and zlib -> its payload"""

    def __init__(self):
        from helpers import EmuBackend
        from test_p2_encode import EmuP2Enc
        self.p1, self.p2 = EmuBackend(), EmuP2Enc()

    def payload(self, profile, raw: bytes, fmt, N_t, C, hop, n_valid):
        if profile == 1:
            body = self.p1.golomb_encode(*self.p1.p1_analogue(np.frombuffer(raw, np.uint8), fmt, 1, N_t, C, 16, SRATE, 0.5, hop, n_valid))[0]
        else:
            body = self.p2.p2_encode_bodies(raw, fmt, 1, N_t, C, 16, SRATE, 0.5, hop, n_valid)[0]
        return fb.raw_deflate(body)


class GpuPayload:
    def payload(self, profile, raw: bytes, fmt, N_t, C, hop, n_valid):
        return fb.raw_deflate(getattr(_bridge("gpu"), f"p{profile}_encode_bodies")(raw, fmt, 1, N_t, C, 16, SRATE, 0.5, hop, n_valid)[0])


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def coder(request):
    if ("coder", request.param) not in _made:
        _made[("coder", request.param)] = EmuPayload() if request.param == "emu" else GpuPayload()
    return _made[("coder", request.param)]


@pytest.mark.parametrize("profile", [1, 2])
@pytest.mark.parametrize("fmt", SIGNED_AND_FLOAT)
def test_a_zero_padded_tail_equals_the_n_valid_route(coder, profile, fmt):
    """The condition of grouping compact tails by N_t.  A tail of t sample-frames, padded with zero bytes to the legal frame size
    N_t and encoded with n_valid = N_t, gives the payload bytes of the Encoder's route (the t sample-frames alone, n_valid = t).
    On the kernels themselves: the interpreted build here, the device on the gpu leg.  Result: equal for every signed and float
    format and both profiles, so no format or profile beyond the unsigned ones groups by exact length."""
    C = 2
    step = ff_format_to_numpy_type(fmt).itemsize * C
    for t in (1, 50, 127, 129, 200):
        N_t = compact.get_samples_min_ge(t)
        pcm = synth.to_pcm(synth.harmonic_mix(t, C, SRATE, seed=t) * 0.8, fmt).tobytes()
        want = coder.payload(profile, pcm, fmt, N_t, C, t, t)
        got = coder.payload(profile, pcm + bytes((N_t - t) * step), fmt, N_t, C, N_t, N_t)
        assert len(want) > 4 and got == want, (fmt, t)


def test_unsigned_tails_keep_their_exact_length(kind):
    """u8: a zero byte is -1.0, so the tails are grouped by exact length -- one encode call per distinct length"""
    c = {}
    br = Counting(_bridge(kind), c)
    clips = [synth.to_pcm(synth.harmonic_mix(n, 1, SRATE, seed=n), "u8").tobytes() for n in (130, 131, 131, 140)]
    res = batched(br, clips, 1, 1, 16, "u8")
    for i, clip in enumerate(clips):
        assert res.streams[i] == per_clip(_bridge(kind), clip, 1, 1, 16, "u8")[0]
    assert c["p1_encode_bodies"] == 1 + 3                       # the whole frames, then tails of 2, 3 and 12 sample-frames
    c.clear()
    clips = [synth.to_pcm(synth.harmonic_mix(n, 1, SRATE, seed=n), "s8").tobytes() for n in (130, 131, 131, 140)]
    batched(br, clips, 1, 1, 16, "s8")
    assert c["p1_encode_bodies"] == 1 + 1                       # ... and one group of N_t = 128 where zero bytes are silence


# -------------------------------------------------------------------------------------------------------------- 3. fallback
def _impulse_clips():
    clips = [synth.harmonic_mix(n, 2, SRATE, seed=40 + n) * 0.8 for n in (300, 128, 515, 50)]
    loud = synth.harmonic_mix(400, 2, SRATE, seed=44) * 0.8
    loud[130, 0] = 1e8                                            # in the second whole frame
    clips.insert(2, loud)
    late = synth.harmonic_mix(300, 2, SRATE, seed=45) * 0.8
    late[290, 1] = -1e8                                           # in the flush frame
    clips.append(late)
    return [c.astype(">f8").tobytes() for c in clips]


def test_a_full_scale_impulse_never_escalates():
    for n in (128, 2048):
        x = np.zeros((n, 1))
        x[3] = -1.0
        assert fo.p0_analogue(x, 12, SRATE, False)[1] == 0 and np.abs(fo.dct_channels(x)).max() <= 1.0


@pytest.mark.parametrize("ecc", [None, (96, 24)])
def test_escalating_clips_fall_back(kind, ecc):
    br = _bridge(kind)
    clips = _impulse_clips()
    want = [per_clip(br, c, 0, 2, 16, "f64be", ecc=ecc) for c in clips]
    if kind == "host":                                           # the input really escalates: two depths in the loud clip's stream
        from test_encoder_ecc import _frames
        for i in range(len(clips)):
            depths = {a.bit_depth_index for a, f in _frames(want[i][0]) if f is not None}
            assert (len(depths) > 1) == (i in (2, 5)), i
    res = batched(br, clips, 0, 2, 16, "f64be", ecc=ecc)
    assert res.fallback == [2, 5]
    for i in range(len(clips)):
        assert (res.streams[i], res.samples[i]) == want[i], i


# ------------------------------------------------------------------------------------------------- 4. inputs, chunks, refusals
@pytest.mark.gpu
@pytest.mark.parametrize("profile", [0, 1])
def test_device_tensors_give_the_same_bytes(profile, monkeypatch):
    import torch
    br = _bridge("gpu")
    clips = clip_set(2, "s16le", seed=11)
    want = batched(br, clips, profile, 2, 16, "s16le", overlap=2)
    dev = [torch.frombuffer(bytearray(c), dtype=torch.uint8).to(br.device) if c else torch.empty(0, dtype=torch.uint8, device=br.device)
           for c in clips]
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("a clip was copied to the host"))
                        if self.dtype == torch.uint8 and any(self is d for d in dev) else torch.Tensor.to(self, "cpu"))
    got = batched(br, dev, profile, 2, 16, "s16le", overlap=2)
    monkeypatch.undo()
    assert got.streams == want.streams and got.samples == want.samples and got.fallback == []
    mixed = batched(br, [d if i % 2 else c for i, (c, d) in enumerate(zip(clips, dev))], profile, 2, 16, "s16le", overlap=2)
    assert mixed.streams == want.streams


@pytest.mark.parametrize("profile", [0, 1])
def test_three_chunks_give_the_same_bytes(kind, profile):
    br = _bridge(kind)
    clips = clip_set(2, "s16le", seed=13)
    whole = batched(br, clips, profile, 2, 16, "s16le", overlap=2)
    c = {}
    total = sum(len(x) for x in clips)
    res = batched(Counting(br, c), clips, profile, 2, 16, "s16le", overlap=2, max_batch_bytes=total * (2 if profile else 1) // 3 + 2000)
    assert res.streams == whole.streams and res.samples == whole.samples
    if kind == "host":
        assert c["lossless_encode_stream" if profile == 0 else "p1_encode_bodies"] >= 3
    else:
        assert c["clips_frame_cut"] >= 3 and c["clips_join"] == 3, c


@pytest.mark.parametrize("profile,overlap", [(1, 0), (1, 2), (2, 2), (0, 0)])
def test_every_chunk_keeps_the_contract(kind, profile, overlap):
    """one clip per chunk, empty clips behind the first chunk: the marker of a clip without a frame is that of an Encoder that
    has written no header, whatever the chunks before it wrote"""
    br = _bridge(kind)
    clips = [synth.to_pcm(synth.harmonic_mix(n, 2, SRATE, seed=60 + n) * 0.8, "s16le").tobytes() if n else b"" for n in (300, 0, 128, 0, 50)]
    clips[3] = b"\x01\x02\x03"                                  # no whole sample-frame either
    c = {}
    res = batched(Counting(br, c), clips, profile, 2, 16, "s16le", overlap=overlap, max_batch_bytes=1)
    assert c["lossless_encode_stream" if profile in (0, 4) else f"p{profile}_encode_bodies"] >= 3      # really chunked
    for i, clip in enumerate(clips):
        assert (res.streams[i], res.samples[i]) == per_clip(br, clip, profile, 2, 16, "s16le", overlap=overlap), i


def test_refusals(kind):
    br = _bridge(kind)
    clip = [bytes(1024)]
    with pytest.raises(ValueError, match="Invalid profile"):
        encode_batch(clip, 2, SRATE, 2, 16, N, "s16le", bridge=br)
    with pytest.raises(ValueError, match="Invalid profile"):
        encode_batch(clip, 3, SRATE, 2, 16, N, "s16le", bridge=br)
    with pytest.raises(ValueError, match="Invalid sample rate"):
        encode_batch(clip, 1, 47999, 2, 16, N, "s16le", bridge=br)
    with pytest.raises(ValueError, match="Frame size cannot be zero"):
        encode_batch(clip, 0, SRATE, 2, 16, 0, "s16le", bridge=br)
    with pytest.raises(ValueError, match="Invalid bit depth"):
        encode_batch(clip, 0, SRATE, 2, 17, N, "s16le", bridge=br)
    with pytest.raises(ValueError, match="Channel count"):
        encode_batch(clip, 0, SRATE, 0, 16, N, "s16le", bridge=br)
    assert encode_batch([], 0, SRATE, 2, 16, N, "s16le", bridge=br).streams == []


# ------------------------------------------------------------------------------------------------------ 5. it really batches
# the C-ABI calls of one encode_batch, whatever the number of clips: every clip is 4 whole frames and a tail of 50, 90 or 127
# sample-frames (profile 1: one padded group of N_t = 128; profile 0: three groups by exact length)
PINNED = {
    "p1": {"clips_frame_cut": 2, "p1_analogue": 2, "p1_golomb_bound": 2, "p1_golomb_encode": 2, "rows_compact": 4},
    "p1_ecc": {"clips_frame_cut": 2, "crc16_ansi_frames": 1, "p1_analogue": 2, "p1_golomb_bound": 2, "p1_golomb_encode": 2,
               "rows_compact": 4, "rs_encode": 1},
    "p0": {"clips_frame_cut": 4, "crc32_frames": 4, "p0_analogue": 4, "payload_bytes": 8},
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PINNED))
def test_call_counts_do_not_depend_on_the_number_of_clips(name, monkeypatch):
    from frad_python_amd import _lib
    from frad_python_amd.bridge import HipBridge
    profile, ecc = (0 if name == "p0" else 1), ((96, 24) if name.endswith("ecc") else None)
    tails = (50, 90, 127)
    counts = []
    for n in (8, 64):
        clips = [synth.to_pcm(synth.harmonic_mix(4 * N + tails[i % 3], 2, SRATE, seed=100 + i) * 0.8, "s16le").tobytes() for i in range(n)]
        c = {}
        monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), c))
        res = batched(HipBridge(), clips, profile, 2, 16, "s16le", ecc=ecc)
        monkeypatch.undo()
        assert res.fallback == []
        for i in (0, 1, 2, n - 1):
            assert res.streams[i] == per_clip(_bridge("gpu"), clips[i], profile, 2, 16, "s16le", ecc=ecc)[0]
        counts.append(c)
        print(f"[calls] {name}, {n} clips: {dict(sorted(c.items()))}")
    assert counts[0] == counts[1] == PINNED[name]
