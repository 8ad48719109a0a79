"""``decode_batch`` and ``encode_batch``: many independent, complete streams (clips) decoded (encoded) in one device pass.

``Decoder`` is, like the reference's, a one-stream object: a collection of short clips costs one chain of launches per clip, and
every clip's flush frame (another ``fsize``) a chain of its own.  Here the streams are scanned together, grouped by frame
geometry, and the frames of ALL streams of a group go through each device stage in one call; one launch of
``frad_clips_overlap_add`` then cross-fades inside every clip, appends the flush fragments, converts and writes the ragged
output.  ``res.pcm[i]`` is bit for bit what a fresh ``Decoder`` returns for stream i when it is driven as the
reference's caller drives it (src/decoder.py:70-88); a stream that does not have the shape ``Encoder.process`` + ``flush``
writes is decoded by such a ``Decoder`` and listed in ``res.fallback``.

``encode_batch`` is the counterpart: ``Encoder`` is a one-stream object too, so a set of short clips costs an
upload, a chain of launches for the whole frames, a second chain for the flush frame and a download per clip.  Here the
clips are joined, one launch of ``frad_clips_frame_cut`` gathers the whole frames of ALL clips into the contiguous block the
transform kernels read, their flush frames are gathered by length, and every stage is called once per such group.
``res.streams[i]`` is byte for byte ``e.process(clip_i).buf + e.flush().buf`` of a fresh ``Encoder`` with the same settings;
a lossless clip with a frame that needs a deeper format is written by such an ``Encoder`` and listed in ``res.fallback``."""
from __future__ import annotations

import numpy as np

from .backend.pcmformat import ff_format_to_numpy_type, from_f64
from .decoder import Decoder
from .encoder import Encoder
from .fourier import BIT_DEPTHS
from .fourier.profiles import COMPACT, compact
from .frames import BUILT, DEFLATED, classify, inflate_bodies, map_zlib, raw_deflate, repair

_SCAN_END, _SCAN_TABLE_FULL = 0, 3                          # include/frad_hip.h


class BatchResult:
    """``pcm[i]`` [samples_i, channels_i], ``srate[i]`` / ``channels[i]`` (of the last header read), ``frames[i]``; ``fallback``:
    the sorted indices that a per-stream ``Decoder`` decoded."""

    def __init__(self, n: int):
        self.pcm = [None] * n
        self.srate = [0] * n
        self.channels = [0] * n
        self.frames = [0] * n
        self.fallback = []


class _Plan:
    """One stream of the batched shape: m frames of one key, at most one last frame that differs in fsize."""
    __slots__ = ("key", "main", "tail_key", "tail", "srate", "channels", "frames")


# ---------------------------------------------------------------------------------------------------------------- scanning
def _scan_together(scan, streams: list):
    """frad_asfh_scan over all streams joined: one call for a clean batch, one more per stream that is not tiled exactly by
    frames (garbage, a truncated header or payload), so that such a stream cannot swallow its neighbour's first frame.
    -> (joined bytes, rows per stream or None where the stream is not a plain sequence of whole frames)"""
    n = len(streams)
    starts = np.zeros(n + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=starts[1:])
    starts = starts.tolist()
    joined = streams[0] if n == 1 else b"".join(streams)
    rows_of, bad = [[] for _ in range(n)], [False] * n
    i, cursor, pos = 0, 0, 0

    def close_until(k):                                      # streams i .. k-1 get no more frames
        nonlocal i, cursor
        while i < k:
            bad[i] = bad[i] or cursor != starts[i + 1]
            i += 1
            cursor = starts[i]

    while i < n and pos < starts[n]:
        table, nxt, why = scan(joined, pos)
        restart = None
        for row in table.tolist():
            h_off, p_off, p_len = row[0], row[1], row[2]
            k = i
            while h_off >= starts[k + 1]:
                k += 1
            close_until(k)
            if p_off + p_len > starts[i + 1]:                # runs into the next stream: an unfinished header or payload
                bad[i], restart = True, starts[i + 1]
                break
            bad[i] = bad[i] or h_off != cursor               # bytes the reference would resynchronise over
            rows_of[i].append(row)
            cursor = p_off + p_len
        if restart is not None:
            cursor = restart                                 # (= starts[i + 1]: close_until leaves the stream marked bad)
            close_until(i + 1)
            pos = restart
        elif why == _SCAN_TABLE_FULL:
            pos = nxt
        elif why != _SCAN_END:                               # an unfinished frame at the end of everything scanned
            k = i
            while nxt >= starts[k + 1]:
                k += 1
            close_until(k)
            bad[i], cursor = True, starts[i + 1]
            close_until(i + 1)
            pos = starts[i]
        else:
            break
    close_until(n)
    return joined, [None if bad[j] else rows_of[j] for j in range(n)]


def _plan(rows: list, joined: bytes, fix_error: bool):
    """The batched shape (module docstring), checked on the scanner's rows of one stream; None: the per-stream Decoder."""
    frames, flushed = [], False
    for row in rows:
        h_off, p_off, p_len, profile, is_ecc, le, depth, ch, srate, fsize, ratio, dsize, csize, fflush, crc = row
        if fflush:
            flushed = True
            continue
        if flushed or profile not in BUILT or ch < 1 or fsize < 1 or depth >= len(BIT_DEPTHS[profile]):
            return None
        if is_ecc and not 1 <= dsize + csize <= 255:
            return None
        key, (frad, _, nb) = classify(joined, row, fix_error)
        if profile in DEFLATED:
            if ratio == 1:
                return None
            key += (None,)
        else:
            if nb == 0 or (key[1] * ch * BIT_DEPTHS[profile][depth] + 7) // 8 != nb:
                return None                                   # no whole payload
            key += (nb,)                                      # equal payload length: the Decoder's run-break rule
        frames.append((key, frad if frad is not None else joined[p_off:p_off + p_len]))
    p = _Plan()
    p.frames, p.key, p.main, p.tail_key, p.tail = len(frames), None, [], None, None
    p.srate, p.channels = (rows[-1][8], rows[-1][7]) if rows else (0, 0)
    if not frames:
        return p
    key = frames[0][0]
    if any(f[0] != key for f in frames[:-1]):
        return None
    last = frames[-1][0]
    if last != key:
        if (last[0],) + last[2:7] != (key[0],) + key[2:7]:
            return None                                       # more than the frame size differs
        ratio = key[6]
        if ratio > 1 and last[1] < key[1] - key[1] * (ratio - 1) // ratio:
            return None                                       # fewer rows than the cross-fade is long
        p.tail_key, p.tail = last, frames[-1][1]
        frames = frames[:-1]
    p.key, p.main = key, [f[1] for f in frames]
    return p


# ---------------------------------------------------------------------------------------------------------------- decoding
def _drive(dec: Decoder, stream: bytes):
    """The reference's caller (src/decoder.py:70-88) with the whole stream as the first buffer."""
    pieces, frames = [], 0
    r = dec.process(stream)
    while True:
        pieces.append(r.pcm)
        frames += r.frames
        before = len(dec.buffer)
        r = dec.process(b"")
        if not r.pcm.size and len(dec.buffer) >= before:
            frames += r.frames
            break
    srate, channels = dec.asfh.srate, dec.asfh.channels
    pieces.append(dec.flush().pcm)
    return pieces, frames, srate, channels


def _frames(bridge, key, payloads: list, device_inflate: bool):
    """The frames of a whole group through the decode stages in one call each -> float64 [n, N, C], a device tensor when the
    bridge keeps them there (HipBridge), else an ndarray (a bridge built from the per-run methods)."""
    profile, N, C, depth, endian, srate = key[:6]
    bits = BIT_DEPTHS[profile][depth]
    on_dev = getattr(bridge, "compact_decode", None)
    if profile not in DEFLATED:
        if on_dev is None:
            return bridge.lossless_decode(profile, payloads, N, C, bits, endian)
        return bridge.lossless_decode(profile, payloads, N, C, bits, endian, keep=True)
    if device_inflate and on_dev is not None:
        got = on_dev(profile, payloads, N, C, bits, srate, deflated=True, keep=True)
        if got is not None:
            return got                                        # else: a frame does not inflate there -> the host inflate, as a whole
    bodies, bad = inflate_bodies(payloads)
    if on_dev is not None:
        return on_dev(profile, bodies, N, C, bits, srate, keep=True)      # an empty body decodes to a frame of zeros
    pcm = getattr(bridge, f"p{profile}_decode_bodies")(bodies, N, C, bits, srate)
    for i in bad:
        pcm[i] = 0.0
    return pcm


def clips_overlap_host(frames, clip_frame0, N, C, ratio, tails: list, tail_off, tail_rows, out_format=None):
    """What ``frad_clips_overlap_add`` computes, with ``Decoder._overlap_host``'s arithmetic (decoder.py:28-46, 110-114), for a
    bridge without ``clips_overlap_add``.  -> (ndarray [rows, C], out_off)"""
    flat = np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in tails]) if tails else np.zeros(0)
    cut = N * (ratio - 1) // ratio if ratio else N
    L = N - cut
    w = 0.5 * (1 - np.cos(np.pi * np.arange(1, L + 1) / (L + 1)))
    pieces, out_off = [], [0]
    for j in range(len(clip_frame0) - 1):
        clip = [np.array(f) for f in frames[clip_frame0[j]:clip_frame0[j + 1]]] if clip_frame0[j + 1] > clip_frame0[j] else []
        if tail_rows[j]:
            clip.append(flat[tail_off[j]:tail_off[j] + tail_rows[j] * C].reshape(tail_rows[j], C).copy())
        fragment = None
        for k, frame in enumerate(clip):
            if fragment is not None and L:
                frame[:L] = frame[:L] * w[:, None] + fragment * w[::-1, None]
            if k == len(clip) - 1:
                pieces.append(frame)                          # its own cut-out and the flush fragment together
            else:
                pieces.append(frame[:cut])
                fragment = frame[cut:]
        out_off.append(out_off[-1] + sum(len(p) for p in pieces[len(pieces) - len(clip):]))
    out = np.concatenate(pieces) if pieces else np.zeros((0, C))
    if out_format is not None:
        out = from_f64(out, out_format)
    return out, np.asarray(out_off, np.int64)


def _decode_chunk(bridge, key, plans: list, out_format, device_inflate, as_tensor):
    """-> (out, out_off): the chunk's ragged PCM, stream j of ``plans`` at rows out_off[j]:out_off[j+1]"""
    profile, N, C = key[:3]
    ratio = key[6]
    main, clip_frame0, tails_by = [], [0], {}
    for j, p in enumerate(plans):
        main.extend(p.main)
        clip_frame0.append(len(main))
        if p.tail_key is not None:
            tails_by.setdefault(p.tail_key, []).append(j)
    order = [j for js in tails_by.values() for j in js]
    fixed = repair(bridge, main + [plans[j].tail for j in order])
    main, tail_payloads = fixed[:len(main)], fixed[len(main):]
    frames = _frames(bridge, key, main, device_inflate) if main else None
    tails, tail_off, tail_rows = [], np.zeros(len(plans), np.int64), np.zeros(len(plans), np.int32)
    off = at = 0
    for tkey, js in tails_by.items():                          # the last frames, grouped again by their size
        tails.append(_frames(bridge, tkey, tail_payloads[at:at + len(js)], device_inflate))
        at += len(js)
        for k, j in enumerate(js):
            tail_off[j], tail_rows[j] = off + k * tkey[1] * C, tkey[1]
        off += len(js) * tkey[1] * C
    on_dev = getattr(bridge, "clips_overlap_add", None)
    if on_dev is None:
        return clips_overlap_host(frames, clip_frame0, N, C, ratio, tails, tail_off, tail_rows, out_format)
    win = None
    if ratio > 1:
        L = N - N * (ratio - 1) // ratio
        win = 0.5 * (1 - np.cos(np.pi * np.arange(1, L + 1) / (L + 1)))       # Decoder._overlap_host's weights
    return on_dev(frames, clip_frame0, N, C, ratio, tails, tail_off, tail_rows, out_format, win, as_tensor)


def decode_batch(streams, *, fix_error: bool = False, out_format: str | None = None, device_inflate: bool = False,
                 as_tensor: bool = False, max_batch_bytes: int = 1 << 30, bridge=None) -> BatchResult:
    """Decode a sequence of complete streams (bytes-like, one stream each).  ``fix_error``, ``out_format`` and
    ``device_inflate`` mean what they mean for ``Decoder``.  ``as_tensor``: ``res.pcm[i]`` stays on the device (float64
    [samples, channels], or the uint8 bytes of ``out_format`` as ``core.p1_overlap_add`` returns them) and nothing is
    downloaded.  ``max_batch_bytes``: a group whose float64 frames would exceed it is cut into chunks of whole streams.  An
    empty stream, or one without a frame, gives an empty array [0, channels]."""
    if bridge is None:
        from .bridge import HipBridge
        bridge = HipBridge()
    streams = [s if isinstance(s, bytes) else bytes(s) for s in streams]
    res = BatchResult(len(streams))
    dt = np.dtype(np.float64) if out_format is None else ff_format_to_numpy_type(out_format)
    if as_tensor and getattr(bridge, "torch", None) is None:
        raise ValueError("as_tensor needs a bridge that keeps tensors on the device")

    def finish(i, pcm):
        if as_tensor and isinstance(pcm, np.ndarray):
            t = bridge.torch
            raw = np.ascontiguousarray(pcm)
            pcm = t.from_numpy(raw if out_format is None else raw.view(np.uint8).reshape(-1)).to(bridge.device)
        res.pcm[i] = pcm

    scan_lib = getattr(bridge, "scan_lib", None)
    if scan_lib is None or not streams:
        plans = [None] * len(streams)                          # no native scanner behind this bridge: every stream on its own
    else:
        joined, rows_of = _scan_together(scan_lib.asfh_scan, streams)
        plans = [_plan(rows, joined, fix_error) if rows is not None else None for rows in rows_of]
    groups = {}
    for i, p in enumerate(plans):
        if p is None:
            dec = Decoder(fix_error, bridge=bridge, out_format=out_format, device_inflate=device_inflate)
            pieces, res.frames[i], res.srate[i], res.channels[i] = _drive(dec, streams[i])
            ch = max(res.channels[i], 1)
            pieces = [x.reshape(-1, ch) for x in pieces if x.size]
            pcm = (pieces[0] if len(pieces) == 1 else np.concatenate(pieces)) if pieces else np.zeros((0, res.channels[i]), dt)
            finish(i, pcm if pcm.dtype == dt or not pieces else pcm.astype(dt))
            res.fallback.append(i)
            continue
        res.frames[i], res.srate[i], res.channels[i] = p.frames, p.srate, p.channels
        if p.key is None:
            finish(i, np.zeros((0, p.channels), dt))
        else:
            groups.setdefault(p.key, []).append(i)
    for key, members in groups.items():
        N, C = key[1], key[2]
        chunk, size = [], 0
        for i in members + [None]:
            need = 0 if i is None else (len(plans[i].main) * N + (plans[i].tail_key[1] if plans[i].tail_key else 0)) * C * 8
            if chunk and (i is None or size + need > max_batch_bytes):
                out, out_off = _decode_chunk(bridge, key, [plans[j] for j in chunk], out_format, device_inflate, as_tensor)
                step = C * dt.itemsize if as_tensor and out_format is not None else 1
                for k, j in enumerate(chunk):
                    finish(j, out[int(out_off[k]) * step:int(out_off[k + 1]) * step])
                chunk, size = [], 0
            if i is not None:
                chunk.append(i)
                size += need
    return res


# ---------------------------------------------------------------------------------------------------------------- encoding
class EncodeBatchResult:
    """``streams[i]`` (bytes), ``samples[i]`` (the sum of the two ``EncodeResult.samples``), ``frames[i]``; ``fallback``: the
    sorted indices that a per-clip ``Encoder`` wrote."""

    def __init__(self, n: int):
        self.streams = [b""] * n
        self.samples = [0] * n
        self.frames = [0] * n
        self.fallback = []


def _host_bytes(clip) -> bytes:
    return clip.cpu().numpy().tobytes() if hasattr(clip, "cpu") else bytes(clip)


def zero_bytes_are_zero(pcm_format: str) -> bool:
    """All-zero bytes convert to +0.0 (pcmformat.py:34-47): the signed integers and the floats.  A little-endian (or 8-bit)
    unsigned zero is -1.0 (the bias is subtracted), so padding a frame of such a format with zero bytes is not padding it with
    silence.  The rule goes by the kind alone: the big-endian unsigned formats, which the reference does not scale (their zero
    is 0.0 too), are kept with the other unsigned ones -- conservative, and one rule instead of two."""
    return ff_format_to_numpy_type(pcm_format).kind in "if"


class _Clips:
    """The chunk's PCM, joined: on the device behind a bridge with ``clips_join`` + ``clips_frame_cut`` (one upload, one
    launch per ``cut``), else a numpy array that ``cut`` slices."""

    def __init__(self, bridge, clips: list, nbytes: list, step: int):
        self.bridge, self.step = bridge, step
        self.on_dev = getattr(bridge, "clips_frame_cut", None) is not None and getattr(bridge, "clips_join", None) is not None
        if self.on_dev:
            self.src = bridge.clips_join(clips, nbytes)
        else:
            self.src = np.frombuffer(b"".join(_host_bytes(c)[:n] for c, n in zip(clips, nbytes)), np.uint8)

    def cut(self, row_src, row_valid, row_len: int):
        """rows of ``row_len`` sample-frames: ``row_valid[r]`` of them from sample-frame ``row_src[r]`` on, then zero bytes"""
        if self.on_dev:
            return self.bridge.clips_frame_cut(self.src, row_src, row_valid, row_len, self.step)
        out = np.zeros((len(row_src), row_len * self.step), np.uint8)
        for r, (at, n) in enumerate(zip(row_src, row_valid)):
            out[r, :n * self.step] = self.src[at * self.step:(at + n) * self.step]
        return out.tobytes()


def _lossless_rows(enc: Encoder, block, n: int, fsize: int):
    """n equally long lossless frames with their headers, as ``Encoder._encode_frames`` writes them through the bridge's
    ``lossless_encode_stream``.  -> (take(first, count) -> bytes, None), or (None, the frames that need a deeper format -- all of
    them when the payload length needs the 64-bit field)"""
    a, prof, C, bridge = enc.asfh, enc.asfh.profile, enc.channels, enc.bridge
    depths = BIT_DEPTHS[prof]
    bits = enc.bit_depth if enc.bit_depth in depths else 16
    a.bit_depth_index, a.channels, a.fsize, a.srate = depths.index(bits), C, fsize, enc.srate
    ecc_kw = {"ecc_ratio": (a.ecc_dsize, a.ecc_codesize)} if a.ecc else {}
    got = bridge.lossless_encode_stream(prof, block, enc.pcm_format_name, n, fsize, C, bits, a.endian, a.lossless_head, **ecc_kw)
    if got is not None:
        size = len(got) // n
        return (lambda first, count: got[first * size:(first + count) * size]), None
    named = getattr(bridge, "last_escalated", None)            # HipBridge: the first pass has named the frames already
    if named is None:
        deeper = [used != bits for _, used in bridge.lossless_encode(prof, block, enc.pcm_format_name, n, fsize, C, bits, a.endian)]
    else:
        deeper = [False] * n
        for i in named:
            deeper[i] = True
    return None, (deeper if any(deeper) else [True] * n)


def _compact_payloads(enc: Encoder, block, n: int, rows: int) -> list:
    """n compact frames, rows of ``rows`` sample-frames that are valid throughout (a padded tail: up to the zero bytes the cut
    wrote) -> their deflated payloads, every stage called once"""
    prof, depths = enc.asfh.profile, BIT_DEPTHS[enc.asfh.profile]
    bits = enc.bit_depth if enc.bit_depth in depths else 16
    args = (block, enc.pcm_format_name, n, compact.get_samples_min_ge(rows), enc.channels, bits, compact.get_valid_srate(enc.srate),
            enc.loss_level, rows, rows)
    if enc.device_deflate:
        return getattr(enc.bridge, f"p{prof}_encode_payloads")(*args)
    return map_zlib(raw_deflate, getattr(enc.bridge, f"p{prof}_encode_bodies")(*args))


def _encode_chunk(enc: Encoder, clips: list, have: list, k: list, t: list, n_eff: int, cut: int, pad_tails: bool, fresh: bytes):
    """The clips of one chunk -- ``have[j]`` whole sample-frames: ``k[j]`` whole frames of ``n_eff``, ``cut`` apart, and a flush
    frame of ``t[j]`` -> (streams, deeper): ``deeper`` lists the clips with a lossless frame that needs a deeper format; when
    there are any, ``streams`` is None and the caller sends the rest again.  ``fresh``: the marker of a clip without a frame, as
    a header writer that has written nothing makes it (``enc``'s has, from the first chunk on)."""
    prof, C = enc.asfh.profile, enc.channels
    is_compact = prof in COMPACT
    step = enc.pcm_format.itemsize * C
    src = _Clips(enc.bridge, clips, [h * step for h in have], step)
    clip_off = np.zeros(len(clips) + 1, np.int64)
    np.cumsum(have, out=clip_off[1:])
    first = np.zeros(len(clips) + 1, np.int64)                 # clip j's whole frames are rows first[j] : first[j + 1]
    np.cumsum(k, out=first[1:])
    M = int(first[-1])
    # ---- the tails, grouped: compact ones by the legal frame size they pad to (where zero bytes are silence), else by length
    groups = {}
    for j, tj in enumerate(t):
        if tj:
            groups.setdefault(compact.get_samples_min_ge(tj) if is_compact and pad_tails else tj, []).append(j)
    row_src = np.concatenate([clip_off[j] + cut * np.arange(k[j], dtype=np.int64) for j in range(len(clips))]) if M else None
    tail_at = lambda js: [int(clip_off[j]) + k[j] * cut for j in js]
    if not is_compact:
        main, deeper, tails = None, set(), {}
        if M:
            main, bad = _lossless_rows(enc, src.cut(row_src, np.full(M, n_eff, np.int32), n_eff), M, n_eff)
            if bad is not None:
                deeper.update(j for j in range(len(clips)) if any(bad[first[j]:first[j + 1]]))
        for length, js in groups.items():
            take, bad = _lossless_rows(enc, src.cut(tail_at(js), [length] * len(js), length), len(js), length)
            if bad is not None:
                deeper.update(j for i, j in enumerate(js) if bad[i])
            for i, j in enumerate(js):
                tails[j] = (take, i)
        if deeper:
            return None, sorted(deeper)
        return [(main(int(first[j]), k[j]) if k[j] else b"") + (tails[j][0](tails[j][1], 1) if t[j] else b"")
                for j in range(len(clips))], []
    # ---- compact: payloads of every frame, one header pass (Reed-Solomon and the checksums of ALL frames in one call)
    depths = BIT_DEPTHS[prof]
    idx = depths.index(enc.bit_depth if enc.bit_depth in depths else 16)
    pay = _compact_payloads(enc, src.cut(row_src, np.full(M, n_eff, np.int32), n_eff), M, n_eff) if M else []
    tail_pay = {}
    for rows, js in groups.items():                            # rows: N_t of a padded group, else the tails' own length
        for j, p in zip(js, _compact_payloads(enc, src.cut(tail_at(js), [t[j] for j in js], rows), len(js), rows)):
            tail_pay[j] = p
    items = []
    for j in range(len(clips)):
        items += [(p, idx, n_eff) for p in pay[first[j]:first[j + 1]]]
        if t[j]:
            items.append((tail_pay[j], idx, t[j]))
    made = enc._emit_all(items)
    marker = {}                                                # force_flush() carries the fsize of the last header written
    for fsize in {n_eff} | set(t):
        if fsize:
            marker[fsize] = enc._head(idx, fsize).force_flush()
    out, at = [], 0
    for j in range(len(clips)):
        n = k[j] + (1 if t[j] else 0)
        frames = made[at:at + n]
        at += n
        # Encoder.inner: a flush frame is followed by a marker of its own, and every flush ends with one
        out.append(b"".join(frames) + (marker[t[j]] * 2 if t[j] else marker[n_eff] if k[j] else fresh))
    return out, []


def encode_batch(clips, profile: int, srate: int, channels: int, bit_depth: int, frame_size: int, pcm_format: str, *,
                 overlap_ratio: int = 0, loss_level: float = 0.5, little_endian: bool = False, ecc_ratio=None,
                 allow_profile2: bool = False, device_deflate: bool = False, max_batch_bytes: int = 1 << 30,
                 bridge=None) -> EncodeBatchResult:
    """Encode a sequence of complete clips (bytes-like, or 1-D device uint8 tensors that are not copied to the host -- except a
    clip that falls back: the per-clip ``Encoder`` takes host bytes) of raw interleaved PCM in ``pcm_format``, one stream each.  The arguments mean what the ``Encoder`` constructor's and setters'
    mean, clamping included; ``ecc_ratio`` None: no ECC, a tuple: ``allow_ecc=True`` + ``set_ecc(True, ratio)``.  What the
    ``Encoder`` refuses (profile 2 without ``allow_profile2``, its ``verify_*`` messages) is a ``ValueError`` here.
    ``max_batch_bytes``: the clips are cut into chunks of whole clips whose gathered frames stay below it."""
    checks = (lambda: None if (profile == 2 and allow_profile2) else Encoder.verify_profile(profile),
              lambda: Encoder.verify_srate(profile, srate), lambda: Encoder.verify_channels(profile, channels),
              lambda: Encoder.verify_bit_depth(profile, bit_depth), lambda: Encoder.verify_frame_size(profile, frame_size))
    for check in checks:
        e = check()
        if e is not None:
            raise ValueError(e)
    if bridge is None:
        from .bridge import HipBridge
        bridge = HipBridge()

    def fresh() -> Encoder:
        enc = Encoder(profile, srate, channels, bit_depth, frame_size, pcm_format, bridge=bridge, allow_profile2=allow_profile2,
                      allow_ecc=ecc_ratio is not None, device_deflate=device_deflate)
        enc.set_overlap_ratio(overlap_ratio)
        enc.set_loss_level(loss_level)
        enc.set_little_endian(little_endian)
        if ecc_ratio is not None:
            enc.set_ecc(True, ecc_ratio)
        return enc

    clips = list(clips)
    res = EncodeBatchResult(len(clips))
    enc = fresh()                                              # the settings, the header writer and the bridge of the batch
    untouched = enc.asfh.force_flush()                         # the marker of a clip without a frame: no header written yet
    is_compact = profile in COMPACT
    n_eff = compact.get_samples_min_ge(enc.fsize) if is_compact else enc.fsize
    ratio = enc.asfh.overlap_ratio
    cut = n_eff * (ratio - 1) // ratio if (is_compact and ratio > 1) else n_eff
    step = enc.pcm_format.itemsize * channels
    pad_tails = zero_bytes_are_zero(pcm_format)                # unsigned formats group their tails by exact length
    for c in clips:
        if hasattr(c, "numel") and (c.dim() != 1 or c.element_size() != 1):
            raise TypeError("a device clip must be a 1-D uint8 tensor of the PCM's bytes")
    have = [(c.numel() if hasattr(c, "numel") else memoryview(c).nbytes) // step for c in clips]
    k = [(h - n_eff) // cut + 1 if h >= n_eff else 0 for h in have]
    t = [h - kj * cut for h, kj in zip(have, k)]
    carry = n_eff - cut
    need = []
    for i, (kj, tj) in enumerate(zip(k, t)):                   # Encoder.inner's bookkeeping
        res.frames[i] = kj + (1 if tj else 0)
        res.samples[i] = (kj * n_eff - (kj - 1) * carry if kj else 0) + (tj - (carry if kj else 0) if tj else 0)
        rows = compact.get_samples_min_ge(tj) if (tj and is_compact) else tj
        need.append((kj * n_eff + rows) * step)

    def alone(i):
        e = fresh()
        pcm = _host_bytes(clips[i])
        res.streams[i] = e.process(pcm).buf + e.flush().buf
        res.fallback.append(i)

    def run(chunk):
        while chunk:
            streams, deeper = _encode_chunk(enc, *([x[i] for i in chunk] for x in (clips, have, k, t)), n_eff, cut, pad_tails, untouched)
            if not deeper:
                for i, s in zip(chunk, streams):
                    res.streams[i] = s
                return
            for d in deeper:                                   # the frame-by-frame route of the Encoder decides their depths
                alone(chunk[d])
            chunk = [i for d, i in enumerate(chunk) if d not in set(deeper)]

    chunk, size = [], 0
    for i in range(len(clips)):
        if chunk and size + need[i] > max_batch_bytes:
            run(chunk)
            chunk, size = [], 0
        chunk.append(i)
        size += need[i]
    run(chunk)
    res.fallback.sort()
    return res
