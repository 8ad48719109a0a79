"""EncoderPool: many live streams fed chunk by chunk == one Encoder per stream, tick for tick and byte for byte.

Legs as in test_batch_encode.py, whose bridges are imported.  "host": test_encoder_ecc.EmuEncoderBridge (oracle arithmetic for
the transforms, the interpreted HIP build for profile 2, Reed-Solomon and the checksums); it has no ``clips_carry_cut``, so the
pool cuts with ``pool.clips_carry_cut_host``.  "gpu": HipBridge, one launch of frad_clips_carry_cut per tick, the members'
remainders on the device between plain ticks.

The yardstick of every comparison is an ``Encoder`` of the stream's own on the same bridge, with the same settings through its
setters, fed the same chunks: every tick's ``buf`` and ``samples`` and the flush are compared.  A test that passes on the
per-stream fallback alone would show nothing, so every case but the fallback one asserts that ``res.fallback`` stays empty.

Everything is 48 kHz and N = 128 (a legal frame size of every profile), a seeded ``synth.harmonic_mix``.  The package has no
24-bit PCM format (``ff_format_to_numpy_type`` knows 8, 16, 32 and 64 bits, as the reference's does), so ``s24le`` is a refusal
here; its sample-frame of 3 bytes is covered by three channels of ``u8``, and by step 3 in test_clips_carry_cut.py."""
import numpy as np
import pytest

from frad_python_amd import Decoder, Encoder, EncoderPool, encode_batch, synth
from frad_python_amd import pool as fp
from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type
from test_batch_decode import Counting
from test_batch_encode import _bridge, kind  # noqa: F401  (kind: the fixture)

N, SRATE = 128, 48000
LENGTHS = (4 * N + 50, 700, 300, 515)


def cfg(profile, C=2, fmt="s16le", bits=16, overlap=0, le=False, ecc=None, device_deflate=False, fsize=N, loss=0.5):
    return dict(profile=profile, C=C, fmt=fmt, bits=bits, overlap=overlap, le=le, ecc=ecc, device_deflate=device_deflate, fsize=fsize,
                loss=loss)


def make_pool(br, c, **kw):
    return EncoderPool(c["profile"], SRATE, c["C"], c["bits"], c["fsize"], c["fmt"], overlap_ratio=c["overlap"], loss_level=c["loss"],
                       little_endian=c["le"], ecc_ratio=c["ecc"], allow_profile2=c["profile"] == 2, device_deflate=c["device_deflate"],
                       bridge=br, **kw)


def yardstick(br, c):
    e = Encoder(c["profile"], SRATE, c["C"], c["bits"], c["fsize"], c["fmt"], bridge=br, allow_profile2=c["profile"] == 2,
                allow_ecc=c["ecc"] is not None, device_deflate=c["device_deflate"])
    e.set_overlap_ratio(c["overlap"])
    e.set_loss_level(c["loss"])
    e.set_little_endian(c["le"])
    if c["ecc"] is not None:
        e.set_ecc(True, c["ecc"])
    return e


def geometry(c):
    """-> (step, n_eff, hop) as Encoder.inner computes them"""
    e = yardstick(None, c)
    compact_prof = c["profile"] in (1, 2)
    n_eff = fp.compact.get_samples_min_ge(e.fsize) if compact_prof else e.fsize
    ratio = e.asfh.overlap_ratio
    hop = n_eff * (ratio - 1) // ratio if compact_prof and ratio > 1 else n_eff
    return ff_format_to_numpy_type(c["fmt"]).itemsize * c["C"], n_eff, hop


def clip(n, C, fmt, seed, stray=0):
    return synth.to_pcm(synth.harmonic_mix(n, C, SRATE, seed=seed) * 0.8, fmt).tobytes() + b"\x7f" * stray


def chunked(pcm: bytes, how: str, c, seed=0):
    step, n_eff, hop = geometry(c)
    if how == "whole":
        ends = [len(pcm)]
    elif how == "fixed":                                        # 97 bytes: stray bytes behind every tick at every step > 1
        ends = list(range(97, len(pcm), 97)) + [len(pcm)]
    elif how == "hop":                                          # exactly one hop at a time
        ends = list(range(hop * step, len(pcm), hop * step)) + [len(pcm)]
    else:                                                       # seeded random: empty chunks, chunks far below a frame
        rng, at, ends = np.random.default_rng(seed), 0, []
        while at < len(pcm):
            at = min(len(pcm), at + int(rng.choice([0, 0, 1, step, 3 * step + 1, 40, n_eff * step // 3, 2 * n_eff * step + 5])))
            ends.append(at)
    return [pcm[a:b] for a, b in zip([0] + ends[:-1], ends)]


def drive(br, c, plans, pool=None, expect_fallback=None, to_chunk=None, before_close=None, yard_br=None, **pool_kw):
    """plans: per member (the tick it is opened at, its chunks in tick order -- None: left out of that tick).  Every member is
    closed one tick after its last chunk (``before_close()`` is called ahead of the first close).  Every tick of the pool is
    compared with an Encoder per member (on ``yard_br`` when the pool's bridge counts calls), and so is the flush.
    -> (streams, samples, the pool, [(tick, member) that fell back])"""
    pool = pool or make_pool(br, c, **pool_kw)
    handles, yards, streams, samples, fell = {}, {}, {}, {}, []
    last = max(s + len(cs) for s, cs in plans)
    for t in range(last + 1):
        tick = {}
        for i, (s, cs) in enumerate(plans):
            if t == s:
                handles[i], yards[i], streams[i], samples[i] = pool.open(), yardstick(yard_br or br, c), b"", 0
            if s <= t < s + len(cs) and cs[t - s] is not None:
                tick[i] = cs[t - s]
        if tick:
            res = pool.process({handles[i]: (to_chunk(x) if to_chunk else x) for i, x in tick.items()})
            assert list(res) == [handles[i] for i in tick]
            for i, x in tick.items():
                want, got = yards[i].process(x), res[handles[i]]
                assert got.buf == want.buf, (t, i, len(x), len(got.buf), len(want.buf))
                assert got.samples == want.samples, (t, i)
                streams[i] += got.buf
                samples[i] += got.samples
            fell += [(t, i) for i in tick if handles[i] in res.fallback]
            assert len(res.fallback) == len(set(res.fallback)) and set(res.fallback) <= set(res)
        for i, (s, cs) in enumerate(plans):
            if t == s + len(cs):
                if before_close is not None:
                    before_close, _ = None, before_close()
                got, want = pool.close(handles[i]), yards[i].flush()
                assert (got.buf, got.samples) == (want.buf, want.samples), (t, i, "flush")
                streams[i] += got.buf
                samples[i] += got.samples
                with pytest.raises(KeyError):
                    pool.process({handles[i]: b""})
    if expect_fallback is None:
        assert fell == [], fell
    return streams, samples, pool, fell


def four_members(c, seed):
    """four clips, one per chunking; the third is opened late and skips every fourth tick, the second is the first to close"""
    step = geometry(c)[0]
    clips = [clip(n, c["C"], c["fmt"], seed * 10 + i, stray=(i % 2) * (step > 1)) for i, n in enumerate(LENGTHS)]
    plans = [(0, chunked(clips[0], "random", c, seed)), (0, chunked(clips[1], "whole", c)), (2, chunked(clips[2], "fixed", c)),
             (1, chunked(clips[3], "hop", c))]
    late = []
    for k, x in enumerate(plans[2][1]):
        late += [None, x] if k % 4 == 3 else [x]
    plans[2] = (2, late)
    return clips, plans


def check(kind, c, seed=1):
    br = _bridge(kind)
    clips, plans = four_members(c, seed)
    streams, samples, pool, _ = drive(br, c, plans)
    whole = encode_batch(clips, c["profile"], SRATE, c["C"], c["bits"], c["fsize"], c["fmt"], overlap_ratio=c["overlap"], loss_level=c["loss"],
                         little_endian=c["le"], ecc_ratio=c["ecc"], allow_profile2=c["profile"] == 2, device_deflate=c["device_deflate"],
                         bridge=br)
    assert whole.fallback == []
    for i in range(len(clips)):
        assert streams[i] == whole.streams[i] and samples[i] == whole.samples[i], i
        d = Decoder(bridge=br)
        pcm = np.concatenate([np.asarray(x).reshape(-1, c["C"]) for x in (d.process(streams[i]).pcm, d.flush().pcm)])
        assert pcm.shape[0] >= samples[i] > 0, (i, pcm.shape, samples[i])
    assert pool.carry_uploads == 0 and pool.carry_downloads <= len(clips)       # a flush brings a remainder down, nothing else does
    return pool


# ---------------------------------------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("profile,C,le", [(0, 1, False), (0, 2, True), (4, 2, False), (4, 1, True)])
def test_lossless(kind, profile, C, le):
    check(kind, cfg(profile, C, le=le))


@pytest.mark.parametrize("overlap", [0, 2, 16, 256])
def test_profile1_stereo(kind, overlap):
    check(kind, cfg(1, 2, overlap=overlap))


def test_profile1_mono_and_a_ratio_of_one(kind):
    check(kind, cfg(1, 1, overlap=1))                           # (the setter makes it 2)


def test_profile2_behind_its_keyword(kind):
    br, c = _bridge(kind), cfg(2, 2, overlap=2)                 # (the host leg interprets the profile-2 kernels lane by lane: two members)
    clips = [clip(n, 2, "s16le", 70 + n) for n in (300, 2 * N + 64 + 9)]
    drive(br, c, [(0, chunked(clips[0], "random", c, 3)), (1, chunked(clips[1], "hop", c))])


@pytest.mark.parametrize("profile", [0, 1])
def test_reed_solomon(kind, profile):
    check(kind, cfg(profile, 2, overlap=2 if profile else 0, ecc=(96, 24)))


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [1, 2])
def test_device_deflate(profile):
    check("gpu", cfg(profile, 2, overlap=2, device_deflate=True))


@pytest.mark.parametrize("fmt,C", [("f64be", 2), ("u8", 1), ("u8", 3), ("s16le", 3)])
@pytest.mark.parametrize("profile", [0, 1])
def test_pcm_formats(kind, profile, fmt, C):
    check(kind, cfg(profile, C, fmt=fmt, overlap=2 if profile else 0))


@pytest.mark.parametrize("profile", [0, 4, 1])
def test_a_frame_size_of_100(kind, profile):
    """compact: padded to 128 by the Encoder's own rule; lossless: frames of 100 sample-frames, no power of two"""
    c = cfg(profile, 2, overlap=2, fsize=100)
    assert geometry(c)[1:] == ((128, 64) if profile == 1 else (100, 100))
    check(kind, c)


def test_a_lossless_ratio_byte_changes_no_hop(kind):
    check(kind, cfg(0, 2, overlap=16))


def test_a_flush_in_the_middle_and_a_handle_left_out(kind):
    """flush(h) between ticks: the stream goes on, its header writer as its own Encoder's -- the next marker carries the fsize"""
    br, c = _bridge(kind), cfg(1, 2, overlap=2)
    pcm = clip(1000, 2, "s16le", 5)
    pool, enc = make_pool(br, c), yardstick(br, c)
    h, other = pool.open(), pool.open()
    for k, x in enumerate([pcm[:700], pcm[700:1300], b"", pcm[1300:1301], pcm[1301:3000], pcm[3000:]]):
        res = pool.process({h: x})
        want = enc.process(x)
        assert (res[h].buf, res[h].samples) == (want.buf, want.samples) and res.fallback == [] and list(res) == [h], k
        if k in (0, 2, 4):
            got, want = pool.flush(h), enc.flush()
            assert (got.buf, got.samples) == (want.buf, want.samples), k
    assert pool.process({}) == {} and pool.flush(other).buf == yardstick(br, c).flush().buf


# -------------------------------------------------------------------------------------------------------------- 2. fallback
@pytest.mark.parametrize("ecc", [None, (96, 24)])
def test_an_escalating_member_falls_back_in_its_tick_only(kind, ecc):
    """test_batch_encode.py's impulse: f64be, 1e8 in a 16-bit lossless pool.  Ticks of 200 sample-frames: the loud frame
    (sample-frames 256 .. 383) is completed by tick 1, and by no other."""
    br, c = _bridge(kind), cfg(0, 2, fmt="f64be", ecc=ecc)
    quiet = [synth.harmonic_mix(n, 2, SRATE, seed=40 + n) * 0.8 for n in (700, 515)]
    loud = synth.harmonic_mix(700, 2, SRATE, seed=44) * 0.8
    loud[330, 0] = 1e8
    clips = [x.astype(">f8").tobytes() for x in (quiet[0], loud, quiet[1])]
    tick = 200 * 16
    plans = [(0, [x[a:a + tick] for a in range(0, len(x), tick)]) for x in clips]
    streams, samples, pool, fell = drive(br, c, plans, expect_fallback=True)
    assert fell == [(1, 1)], fell
    from test_encoder_ecc import _frames
    depths = [{a.bit_depth_index for a, f in _frames(s) if f is not None} for s in streams.values()]
    assert [len(d) for d in depths] == [1, 2, 1]                # the input really escalates, in the loud member alone
    # its remainder came down for that tick and went up again with the next; the flushes bring the other downloads
    assert pool.carry_uploads == 1 and pool.carry_downloads == 1 + 3


# ----------------------------------------------------------------------------------------- 3. inputs, chunks, refusals
def test_refusals(kind):
    br = _bridge(kind)
    for bad, why in (((2, SRATE, 2, 16, N, "s16le"), "Invalid profile"), ((3, SRATE, 2, 16, N, "s16le"), "Invalid profile"),
                     ((1, 47999, 2, 16, N, "s16le"), "Invalid sample rate"), ((0, SRATE, 2, 16, 0, "s16le"), "Frame size cannot be zero"),
                     ((0, SRATE, 2, 17, N, "s16le"), "Invalid bit depth"), ((0, SRATE, 0, 16, N, "s16le"), "Channel count"),
                     ((0, SRATE, 1, 16, N, "s24le"), "Invalid format")):
        with pytest.raises(ValueError, match=why):
            EncoderPool(*bad, bridge=br)
    pool = make_pool(br, cfg(0))
    h = pool.open()
    before = (pool._members[h].buffer, pool._members[h].held)
    with pytest.raises(KeyError):
        pool.process({h: bytes(4000), h + 1: b""})              # an unknown handle: before any stream has moved
    assert (pool._members[h].buffer, pool._members[h].held) == before
    assert pool.open() == h + 1 and pool.close(h).buf == b"" and pool.open() == h + 2      # handles are never reused


def test_settings_are_clamped_as_the_setters_clamp_them(kind, capsys):
    br = _bridge(kind)
    pcm = clip(600, 2, "s16le", 9)
    pool = EncoderPool(1, SRATE, 2, 16, N, "s16le", overlap_ratio=300, loss_level=-0.01, ecc_ratio=(0, 300), bridge=br)
    capsys.readouterr()
    enc = yardstick(br, cfg(1, 2, overlap=256, loss=0.125, ecc=(96, 24)))
    h = pool.open()
    got, want = pool.process({h: pcm}), enc.process(pcm)
    assert got[h].buf == want.buf and got.fallback == [] and pool.close(h).buf == enc.flush().buf


@pytest.mark.parametrize("profile", [0, 1])
def test_chunks_of_members_give_the_same_bytes(kind, profile):
    br, c = _bridge(kind), cfg(profile, 2, overlap=2)
    counts = {}
    clips = [clip(700 + 30 * i, 2, "s16le", 80 + i) for i in range(6)]
    plans = [(0, [x[:1500], x[1500:]]) for x in clips]
    ticks = {}                                                  # the calls of the two ticks: the closes behind them flush per stream
    drive(Counting(br, counts), c, plans, yard_br=br, before_close=lambda: ticks.update(counts),
          max_batch_bytes=4 * N * 4)                            # four frames of 512 bytes: at most two members a chunk
    counts = ticks
    stage = "lossless_encode_stream" if profile == 0 else "p1_encode_bodies"
    assert counts[stage] >= 2 * 3, counts                       # really chunked: three chunks of members or more in either tick
    if kind == "gpu":
        assert counts["clips_carry_cut"] == counts["clips_join"] == counts[stage], counts


# ----------------------------------------------------------------------------------------------- 4. it really batches (gpu)
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p0", "p0_ecc", "p1", "p1_ecc", "p1_device_deflate"])
def test_a_tick_costs_the_same_with_twelve_members_as_with_three(name):
    br = _bridge("gpu")
    c = cfg(0 if name.startswith("p0") else 1, 2, overlap=0 if name.startswith("p0") else 2, ecc=(96, 24) if name.endswith("ecc") else None,
            device_deflate=name.endswith("deflate"))
    seen = []
    for n in (3, 12):
        counts = {}
        clips = [clip(900 + 7 * i, 2, "s16le", 200 + i) for i in range(n)]
        plans = [(0, [x[a:a + 1100] for a in range(0, len(x), 1100)]) for x in clips]       # 275 sample-frames a tick: 2 or 3 frames
        ticks = max(len(cs) for _, cs in plans)
        assert all(len(cs) == ticks for _, cs in plans)         # so every member is closed behind the last tick
        _, _, pool, _ = drive(Counting(br, counts), c, plans, yard_br=br, before_close=lambda: seen.append(dict(counts)))
        assert seen[-1]["clips_carry_cut"] == seen[-1]["clips_join"] == ticks, seen[-1]
        assert pool.carry_uploads == 0 and pool.carry_downloads == n                        # the flushes alone
        print(f"[calls] {name}, {n} members, {ticks} ticks: {dict(sorted(seen[-1].items()))}")
    assert seen[0] == seen[1], seen


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [0, 1])
def test_device_tensor_chunks_give_the_same_bytes(profile, monkeypatch):
    import torch
    br, c = _bridge("gpu"), cfg(profile, 2, overlap=2)
    clips = [clip(n, 2, "s16le", 300 + n) for n in (700, 300, 515)]
    plans = [(0, [x[a:a + 1100] for a in range(0, len(x), 1100)]) for x in clips]
    held = []

    def up(x):
        held.append(torch.frombuffer(bytearray(x), dtype=torch.uint8).to(br.device) if x else torch.empty(0, dtype=torch.uint8, device=br.device))
        return held[-1]

    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("a chunk was copied to the host"))
                        if any(self is d for d in held) else real(self, *a, **k))
    _, _, pool, _ = drive(br, c, plans, to_chunk=up)            # (drive compares every tick with the Encoder fed the host bytes)
    monkeypatch.undo()
    assert pool.carry_uploads == 0
    pool = make_pool(br, c)
    h = pool.open()
    with pytest.raises(ValueError, match="whole sample-frames"):
        pool.process({h: torch.zeros(6, dtype=torch.uint8, device=br.device)})
    with pytest.raises(TypeError):
        pool.process({h: torch.zeros(8, dtype=torch.int16, device=br.device)})
    # host bytes that leave a stray byte, then a device chunk: the seam's sample-frame is put together from both
    enc = yardstick(br, c)
    pcm = clip(400, 2, "s16le", 6)
    for x, dev in ((pcm[:1001], False), (pcm[1001:1401], True), (pcm[1401:], False)):
        got = pool.process({h: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(br.device) if dev else x})
        want = enc.process(x)
        assert (got[h].buf, got[h].samples) == (want.buf, want.samples)
    assert pool.flush(h).buf == enc.flush().buf


# ---------------------------------------------------------------------------------------------------------- 5. transactional
class Boom(RuntimeError):
    pass


class FailingBridge:
    """test_stream.FailingBridge over any bridge: the named stage method raises once"""

    def __init__(self, inner, name):
        self.__dict__.update(_inner=inner, _name=name, fail=False)

    def __getattr__(self, name):
        v = getattr(self._inner, name)
        if name != self._name:
            return v

        def call(*a, **k):
            if self.fail:
                self.__dict__["fail"] = False
                raise Boom(name)
            return v(*a, **k)
        return call


@pytest.mark.parametrize("profile,stage", [(0, "lossless_encode_stream"), (1, "p1_encode_bodies"), (1, "rs_encode_crc16")])
def test_a_failed_tick_changes_no_member(kind, profile, stage):
    inner = _bridge(kind)
    br = FailingBridge(inner, stage)
    c = cfg(profile, 2, overlap=2, ecc=(96, 24) if stage.startswith("rs") else None)
    pool = make_pool(br, c)
    clips = [clip(n, 2, "s16le", 400 + n) for n in (700, 600, 515)]
    encs = [yardstick(inner, c) for _ in clips]
    hs = [pool.open() for _ in clips]
    state = lambda: [(m.buffer, id(m.held), m.have_carry, dict(vars(m.asfh))) for m in (pool._members[h] for h in hs)]
    for t, (a, b) in enumerate(((0, 1201), (1201, 1900), (1900, 4000))):
        tick = {h: x[a:b] for h, x in zip(hs, clips)}
        if t == 1:                                              # every member holds a remainder now, and the tick completes frames
            before, counters = state(), (pool.carry_uploads, pool.carry_downloads)
            br.__dict__["fail"] = True
            with pytest.raises(Boom):
                pool.process(tick)
            assert state() == before and (pool.carry_uploads, pool.carry_downloads) == counters
        res = pool.process(tick)
        assert res.fallback == []
        for h, e, x in zip(hs, encs, clips):
            want = e.process(x[a:b])
            assert (res[h].buf, res[h].samples) == (want.buf, want.samples), (t, h)
    for h, e in zip(hs, encs):
        assert pool.close(h).buf == e.flush().buf
