"""DecoderPool: many live streams fed chunk by chunk == one Decoder per stream, tick for tick and bit for bit.

Legs as in test_batch_decode.py, whose bridges and helpers are imported.  "host": oracle arithmetic behind HostBridge, which has
no ``clips_carry_add``, so the pool cross-fades with ``pool.clips_carry_host`` (Decoder._overlap_host's arithmetic); "gpu":
HipBridge, one launch of frad_clips_carry_add per geometry group and tick, the fragments on the device between plain ticks.

The yardstick of every comparison is a ``Decoder`` of the stream's own on the same bridge, fed the same chunks.  It is a local
subclass that only takes notes -- the runs it decoded and whether it flushed, per call -- so that the tests can tell which ticks
the pool has to batch: a test that passes on the per-stream fallback alone would show nothing."""
import numpy as np
import pytest

from frad_python_amd import Decoder, DecoderPool
from frad_python_amd import pool as fp
from test_batch_decode import Counting, HostBridge, _bridge, _clip, encode, frame_spans, kind, same  # noqa: F401  (kind: the fixture)
from test_decode_windows import damage

FORMATS = (None, "s16le", "f32be", "u8")
# (profile, channels, bits, frame size, overlap ratio, ecc): nine whole frames and a short tail each
CONFIGS = [(0, 1, 32, 128, 0, None), (0, 2, 16, 256, 0, None), (4, 2, 16, 160, 0, None), (4, 1, 24, 128, 0, None),
           (1, 2, 16, 128, 0, None), (1, 1, 16, 160, 2, None), (1, 2, 16, 256, 16, None), (2, 1, 16, 128, 2, None),
           (2, 2, 16, 256, 16, None), (1, 2, 16, 256, 16, (96, 24))]
_made = {}


def stream_of(kind, profile, C, bits, fsize, ratio, ecc=None, seed=0, frames=9, tail=37):
    cut = fsize * (ratio - 1) // ratio if ratio else fsize
    return encode(kind, _clip((frames - 1) * cut + fsize + tail, C, 500 + seed), profile, C, bits, fsize, ratio, ecc=ecc)


def clean_streams(kind):
    if kind not in _made:
        out = []
        for seed, cfg in enumerate(CONFIGS):
            s = stream_of(kind, *cfg, seed=seed)
            out.append(damage(kind, s) if cfg[5] is not None else s)
        _made[kind] = out
    return _made[kind]


def frame_starts(kind, stream):
    """the header offsets of the frames and flush markers the native scanner finds (the stream may end unfinished)"""
    return [r[0] for r in _bridge(kind).scan_lib.asfh_scan(stream, 0)[0].tolist()]


def chunkings(kind, stream, seed):
    """name -> the chunks of one stream"""
    rng = np.random.default_rng(seed)
    cuts = {"whole": [len(stream), len(stream)], "fixed": list(range(97, len(stream), 97)) + [len(stream)]}
    at, ragged = 0, []
    while at < len(stream):
        at = min(len(stream), at + int(rng.choice([0, 0, 1, 40, 300, 900, 2500])))
        ragged.append(at)
    cuts["random"] = ragged
    starts = frame_starts(kind, stream)[1:]
    picked, k = [], 0
    for n in (1, 2, 3) * len(starts):                          # one, two, three frames at a time
        k += n
        if k >= len(starts):
            break
        picked.append(starts[k])
    cuts["frames"] = picked + [len(stream)]
    cuts["each"] = starts + [len(stream)]                      # every frame, and every flush marker, a chunk of its own
    return {name: [stream[a:b] for a, b in zip([0] + ends[:-1], ends)] for name, ends in cuts.items()}


class Noting(Decoder):
    """the yardstick: a Decoder that notes, per process() call, the runs it decoded and whether it flushed"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.runs, self.flushes = [], 0

    def _decode_run(self, key, entries):
        self.runs.append((key, len(entries)))
        return super()._decode_run(key, entries)

    def flush(self):
        self.flushes += 1
        return super().flush()

    def tick(self, chunk):
        self.runs, self.flushes = [], 0
        return self.process(chunk)


def as_host(pcm):
    return pcm if isinstance(pcm, np.ndarray) else pcm.cpu().numpy()


def equal(got, want, as_tensor=False):
    if as_tensor:
        assert not isinstance(got.pcm, np.ndarray) and got.pcm.is_cuda
        ok = as_host(got.pcm).tobytes() == want.pcm.tobytes()
    else:
        ok = same(got.pcm, want.pcm)
    return ok and (got.srate, got.frames, got.crit) == (want.srate, want.frames, want.crit)


def drive(kind, streams_chunks, fix_error=False, out_format=None, device_inflate=False, as_tensor=False, opened_at=None, closed_at=None):
    """Feed every stream's chunks tick by tick to one pool and to a Decoder per stream, compare every tick and the final flush.
    -> [(stream, tick, runs the Decoder decoded, it flushed or crit, in res.fallback)]"""
    br = _bridge(kind)
    pool = DecoderPool(fix_error, out_format, device_inflate, as_tensor, bridge=br)
    n = len(streams_chunks)
    opened_at, closed_at = opened_at or {}, closed_at or {}
    refs = [Noting(fix_error, bridge=br, out_format=out_format, device_inflate=device_inflate) for _ in range(n)]
    handles, notes = {}, []
    for t in range(max(opened_at.get(i, 0) + len(c) for i, c in enumerate(streams_chunks))):
        tick = {}
        for i, chunks in enumerate(streams_chunks):
            k = t - opened_at.get(i, 0)
            if k == 0:
                handles[i] = pool.open()
            if 0 <= k < len(chunks) and i in handles:
                if closed_at.get(i) == t:
                    assert equal(pool.close(handles[i]), refs[i].flush(), as_tensor), (i, t, "close")
                    with pytest.raises(KeyError):
                        pool.is_empty(handles.pop(i))
                else:
                    tick[handles[i]] = chunks[k]
        res = pool.process(tick)
        assert set(res) == set(tick) and set(res.fallback) <= set(tick)
        for i, h in handles.items():
            if h not in tick:
                continue
            want = refs[i].tick(tick[h])
            assert equal(res[h], want, as_tensor), (i, t, out_format)
            assert pool.is_empty(h) == refs[i].is_empty(), (i, t)
            a, b = pool.get_asfh(h), refs[i].get_asfh()
            assert (a.profile, a.srate, a.channels, a.fsize, a.frmbytes) == (b.profile, b.srate, b.channels, b.fsize, b.frmbytes), (i, t)
            notes.append((i, t, list(refs[i].runs), bool(refs[i].flushes) or want.crit, h in res.fallback))
    for i, h in handles.items():
        assert equal(pool.flush(h), refs[i].flush(), as_tensor), (i, "flush")
        assert pool.is_empty(h) == refs[i].is_empty(), i
    assert len(set(handles.values())) == len(handles)
    return notes


def check_plain_ticks(notes, at_least):
    """A tick whose complete frames all share one key (the Decoder decoded exactly one run and did not flush) is never in
    ``res.fallback`` -- on streams of constant geometry -- and a tick that flushed always is.  One case is the per-stream path's by
    the plainness rule itself and is left out: the short last frame of an OVERLAPPED stream has a key of its own and meets a
    pending fragment of another length; without overlap no fragment is pending and that tick is batched like any other."""
    plain, main = 0, {}
    for i, t, runs, flushed, fell_back in notes:
        if runs:
            main.setdefault(i, runs[0][0])
        if flushed:
            assert fell_back, (i, t)
        elif len(runs) == 1 and (runs[0][0] == main[i] or not (main[i][0] in (1, 2) and main[i][6])):
            assert not fell_back, (i, t, runs)
            plain += 1
        elif not runs:
            assert not fell_back, (i, t)
    assert plain >= at_least, plain


# ------------------------------------------------------------------------------- 1. + 3. every tick equals the Decoder's
@pytest.mark.parametrize("chunking", ["whole", "fixed", "random", "frames"])
@pytest.mark.parametrize("out_format", FORMATS)
def test_every_tick_equals_the_per_stream_decoder(kind, out_format, chunking):
    streams = clean_streams(kind)
    chunks = [chunkings(kind, s, 17 + i)[chunking] for i, s in enumerate(streams)]
    notes = drive(kind, chunks, fix_error=True, out_format=out_format)
    # "whole": the nine frames are one run, the tail frame a second one: that tick is the per-stream path's by rule
    check_plain_ticks(notes, {"whole": 0, "fixed": 30, "random": 10, "frames": 30}[chunking])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["device_inflate", "as_tensor", "as_tensor_s16le", "unrepaired"])
def test_on_the_gpu_with_device_inflate_and_as_tensor(mode):
    streams = clean_streams("gpu")
    chunks = [chunkings("gpu", s, 5 + i)["random" if mode != "as_tensor" else "frames"] for i, s in enumerate(streams)]
    kw = {"device_inflate": dict(device_inflate=True, fix_error=True), "as_tensor": dict(as_tensor=True, fix_error=True),
          "as_tensor_s16le": dict(as_tensor=True, out_format="s16le", fix_error=True), "unrepaired": dict(fix_error=False)}[mode]
    check_plain_ticks(drive("gpu", chunks, **kw), 10)


def test_as_tensor_needs_a_bridge_with_tensors():
    with pytest.raises(ValueError):
        DecoderPool(as_tensor=True, bridge=HostBridge.__new__(HostBridge))


# ----------------------------------------------------------------------------------------------------- 2. hard streams
def hard_streams(kind):
    if ("hard", kind) not in _made:
        body = lambda s: b"".join(s[h:e] for h, e, fl, _ in frame_spans(kind, s) if not fl)      # the frames without the flush markers
        mono, stereo = stream_of(kind, 1, 1, 16, 128, 2, seed=31, frames=4), stream_of(kind, 1, 2, 16, 128, 2, seed=32, frames=4)
        a, b = stream_of(kind, 1, 2, 16, 256, 2, seed=33, frames=4, tail=90), stream_of(kind, 1, 2, 16, 256, 2, seed=34, frames=6)
        lossless = stream_of(kind, 4, 2, 16, 160, 0, seed=35, frames=5)
        g = stream_of(kind, 1, 2, 16, 256, 16, seed=36, frames=6)
        at = frame_starts(kind, g)[3]
        cut_in_header = stream_of(kind, 0, 2, 32, 128, 0, seed=37, frames=5)
        last = frame_starts(kind, cut_in_header)[4]
        _made[("hard", kind)] = {
            "channels change": mono + stereo,                                # each ends in its flush markers
            "tail frame, then more frames": body(a) + b,                     # the fragment changes its length and comes back
            "compact, then lossless": body(a) + lossless,                    # a pending fragment meets frames without overlap
            "garbage between two frames": g[:at] + b"\x00garbage\xff\xd0 between" + g[at:],
            "cut inside a header": cut_in_header[:last + 7],
        }
    return _made[("hard", kind)]


@pytest.mark.parametrize("chunking", ["fixed", "frames", "random", "each"])
@pytest.mark.parametrize("out_format", [None, "s16le"])
def test_hard_streams_equal_the_decoder_and_fall_back(kind, out_format, chunking):
    hard = hard_streams(kind)
    names = list(hard)
    chunks = [chunkings(kind, hard[name], 3 + i)[chunking] for i, name in enumerate(names)]
    if chunking == "random":                                   # no tick with frames of both channel counts: numpy cannot join them
        chunks[0] = chunkings(kind, hard[names[0]], 0)["fixed"]
    notes = drive(kind, chunks, out_format=out_format)
    by = {name: [n for n in notes if n[0] == i] for i, name in enumerate(names)}
    for name, rows in by.items():
        for i, t, runs, flushed, fell_back in rows:
            if flushed or len(runs) > 1:
                assert fell_back, (name, t)                    # the hard ticks
    assert sum(1 for n in by["channels change"] if n[3]) >= 2                 # both halves flushed
    for name in ("tail frame, then more frames", "compact, then lossless"):
        fell = [n[1] for n in by[name] if n[4] and not n[3]]
        assert fell, name
        if chunking == "each":
            # one run, no flush, and still the per-stream path's: the pending fragment does not fit the run ...
            assert any(len(n[2]) == 1 and not n[3] and n[4] for n in by[name]), name
        # ... and later ticks are batched again (a random chunk may hold every frame that is left: no such tick then)
        assert chunking == "random" or any(n[1] > fell[0] and len(n[2]) == 1 and not n[3] and not n[4] for n in by[name]), name
    assert any(len(n[2]) == 1 and not n[4] for n in by["garbage between two frames"])
    assert any(len(n[2]) == 1 and not n[4] for n in by["cut inside a header"])


# ------------------------------------------------------------------------------------------------------- 4. call counts
class HostBridgeCarry(HostBridge):
    """... with the group-level entry point, so that the counting test sees it called"""

    def clips_carry_add(self, frames, clip_frame0, N, C, ratio, prev, out_format=None, as_tensor=False):
        return fp.clips_carry_host(frames, clip_frame0, N, C, ratio, prev, out_format)


def test_call_counts_are_per_group_not_per_member(kind, monkeypatch):
    groups = [(1, 2, 16, 256, 16), (4, 1, 16, 160, 0), (0, 2, 32, 128, 0)]
    streams = [stream_of(kind, *g, seed=70 + 4 * k + i) for k, g in enumerate(groups) for i in range(4)]
    starts = [frame_starts(kind, s) for s in streams]
    ticks = [[s[:st[3]] for s, st in zip(streams, starts)], [s[st[3]:st[5]] for s, st in zip(streams, starts)]]
    c = {}
    if kind == "host":
        br = Counting(HostBridgeCarry(), c)
    else:
        from frad_python_amd import _lib
        from frad_python_amd.bridge import HipBridge
        monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), c))              # every C-ABI call of the loaded library
        br = HipBridge()
    pool = DecoderPool(bridge=br)
    hs = [pool.open() for _ in streams]
    got = []
    for tick in ticks:
        c.clear()
        res = pool.process(dict(zip(hs, tick)))
        got.append((res, dict(c)))
        print(f"[calls] {dict(sorted(c.items()))}")
    monkeypatch.undo()
    refs = [Decoder(bridge=_bridge(kind)) for _ in streams]
    for (res, counts), tick in zip(got, ticks):
        assert res.fallback == []
        for h, ref, chunk in zip(hs, refs, tick):
            assert equal(res[h], ref.process(chunk)), h
        assert counts["clips_carry_add"] == 3, counts
        if kind == "host":
            assert counts["p1_decode_bodies"] == 1 and counts["lossless_decode"] == 2, counts
            assert not {"overlap_add", "p1_decode_run", "lossless_decode_strided"} & set(counts), counts
        else:
            assert counts["p1_golomb_decode"] == 1 and counts["p1_digital"] == 1 and counts["p0_digital"] == 1 and counts["p4_digital"] == 1, counts
            assert not {"p1_overlap_add", "p1_overlap_add_pcm", "clips_overlap_add", "from_f64"} & set(counts), counts
    if kind == "gpu":                                          # the fragments stayed where the kernel left them
        assert pool.fragment_uploads == 0 and pool.fragment_downloads == 0
        assert all(not pool._members[h].overlap_fragment.size for h in hs)
        assert all(pool._members[h].frag_dev is not None for h in hs[:4])
    for h, ref in zip(hs, refs):
        assert equal(pool.flush(h), ref.flush())
    if kind == "gpu":
        assert pool.fragment_downloads == 4


def test_max_batch_bytes_cuts_a_group_into_chunks_of_whole_members(kind):
    streams = [stream_of(kind, 1, 2, 16, 256, 16, seed=90 + i) for i in range(5)]
    first = [s[:frame_starts(kind, s)[3]] for s in streams]
    c = {}
    pool = DecoderPool(max_batch_bytes=2 * 3 * 256 * 2 * 8, bridge=Counting(HostBridgeCarry(), c) if kind == "host" else _bridge(kind))
    hs = [pool.open() for _ in streams]
    res = pool.process(dict(zip(hs, first)))
    assert res.fallback == [] and (kind != "host" or c["clips_carry_add"] == 3)          # 2 + 2 + 1 members
    for h, chunk in zip(hs, first):
        assert equal(res[h], Decoder(bridge=_bridge(kind)).process(chunk))


# ------------------------------------------------------------------------------------------------------------ 5. handles
def test_handles_open_late_close_early_and_sit_out_a_tick(kind):
    streams = clean_streams(kind)[4:8]
    chunks = [chunkings(kind, s, 40 + i)["frames"] for i, s in enumerate(streams)]
    chunks[2] = chunks[2][:2] + [b""] + chunks[2][2:]
    notes = drive(kind, chunks, opened_at={1: 3}, closed_at={0: 5})
    assert max(n[1] for n in notes if n[0] == 0) == 4 and min(n[1] for n in notes if n[0] == 1) == 3
    pool = DecoderPool(bridge=_bridge(kind))
    h = pool.open()
    for call in (lambda: pool.process({h: b"", h + 1: b""}), lambda: pool.flush(h + 1), lambda: pool.close(7), lambda: pool.get_asfh(-1)):
        with pytest.raises(KeyError):
            call()
    assert pool.process({}) == {} and pool.process({h: b""})[h].pcm.size == 0
    pool.close(h)
    assert pool.open() == h + 1                                # never reused
