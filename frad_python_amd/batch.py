"""``decode_batch``: many independent, complete streams decoded in one device pass.

``Decoder`` is, like the reference's, a one-stream object: a collection of short clips costs one chain of launches per clip, and
every clip's flush frame (another ``fsize``) a chain of its own.  Here the streams are scanned together, grouped by frame
geometry, and the frames of ALL streams of a group go through each device stage in one call; one launch of
``frad_clips_overlap_add`` then cross-fades inside every clip, appends the flush fragments, converts and writes the ragged
output.  ``res.pcm[i]`` is bit for bit what a fresh ``Decoder`` returns for stream i when it is driven as the
reference's caller drives it (src/decoder.py:70-88); a stream that does not have the shape ``Encoder.process`` + ``flush``
writes is decoded by such a ``Decoder`` and listed in ``res.fallback``."""
from __future__ import annotations

import numpy as np

from .backend.pcmformat import ff_format_to_numpy_type, from_f64
from .decoder import Decoder
from .fourier import BIT_DEPTHS
from .frames import BUILT, DEFLATED, classify, inflate_bodies, repair

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
