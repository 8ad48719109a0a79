"""``DecoderPool``: many live streams decoded chunk by chunk, one device pass per tick.

``Decoder`` is the streaming object, one stream each: a server that holds a few hundred of them pays a chain of launches per
stream on every tick, each over the two or three dozen frames a chunk completes.  ``decode_batch`` and ``StreamIndex`` run every
stage once per geometry group, but want their streams whole.  The pool is the streaming shape of the batched machinery
(DESIGN.md 4n): every member keeps a ``Decoder``'s own state and is parsed by the ``Decoder``'s own parser, the frames a tick
completes are gathered by run key across the members, go through ``frames.repair`` and ``batch._frames`` once per group, and one
launch of ``frad_clips_carry_add`` cross-fades every member's run from the fragment it carried in to the fragment it carries
out.  ``res[h]`` is, bit for bit, what a ``Decoder`` of its own returns from ``process(chunk)`` for the same chunk sequence.

A member's tick is *plain* when it completed exactly one run, did not end in a force-flush header or a change of channels /
sample rate, a compact run's overlap ratio is not 1, a lossless run's payloads are whole, and the pending fragment is empty or
has the run's shape ``(L, C)`` with nothing of it consumed.  Every other tick is decoded by the member's inherited per-stream
path, run after run, and its handle is listed in ``res.fallback``.

On a bridge that keeps tensors a member's fragment stays on the device between plain ticks: the launch reads the fragments of
one tick and writes those of the next into a block of its own, so the two never share memory.  It comes to the host only when a
fallback tick or ``flush`` needs it, and goes up again only after such a tick left a new one."""
from __future__ import annotations

import numpy as np

from .backend.pcmformat import ff_format_to_numpy_type, from_f64
from .batch import _frames
from .decoder import Decoder, DecodeResult
from .fourier import BIT_DEPTHS
from .frames import DEFLATED, Damaged, repair


def clips_carry_host(frames, clip_frame0, N, C, ratio, prev=None, out_format=None):
    """What ``frad_clips_carry_add`` computes, with ``Decoder._overlap_host``'s arithmetic (decoder.py:28-46), for a bridge
    without ``clips_carry_add``.  ``prev``: None, or per clip None or the fragment [L, C] carried in.
    -> (ndarray [rows, C], out_off, next): ``next[j]`` the fragment clip j carries out -- ``prev[j]`` for a clip without a frame,
    None where nothing is carried."""
    cut = N * (ratio - 1) // ratio if ratio else N
    L = N - cut
    w = 0.5 * (1 - np.cos(np.pi * np.arange(1, L + 1) / (L + 1)))
    pieces, out_off, nxt = [], [0], []
    for j in range(len(clip_frame0) - 1):
        fragment = prev[j] if prev is not None and L else None
        rows = 0
        for frame in frames[clip_frame0[j]:clip_frame0[j + 1]] if clip_frame0[j + 1] > clip_frame0[j] else ():
            frame = np.array(frame, np.float64)
            if fragment is not None and L:
                frame[:L] = frame[:L] * w[:, None] + np.asarray(fragment).reshape(L, C) * w[::-1, None]
            pieces.append(frame[:cut])
            fragment = frame[cut:].copy() if L else None
            rows += cut
        nxt.append(fragment)
        out_off.append(out_off[-1] + rows)
    out = np.concatenate(pieces) if pieces else np.zeros((0, C))
    if out_format is not None:
        out = from_f64(out, out_format)
    return out, np.asarray(out_off, np.int64), nxt


class PoolResult(dict):
    """One tick: ``res[h]`` is the ``DecodeResult`` (pcm, srate, frames, crit) of handle h; ``fallback``: the handles whose tick
    the per-stream path decoded, in the order of the tick's dict."""

    def __init__(self):
        super().__init__()
        self.fallback = []


class _Member(Decoder):
    """A ``Decoder`` whose runs are recorded instead of decoded: the parser, the buffer, ``info``, ``broken_frame``, the fragment
    and ``overlap_prog`` are the inherited ones.  ``recorded``: (key, [(payload, data bytes)]) per run of the tick, the payload
    bytes copied out of the parser's buffer; ``frag_dev``: the fragment while it lives on the device (``overlap_fragment`` is
    empty meanwhile); ``flushed``: the tick ended in ``flush()`` (a force-flush header, or a change of channels / rate)."""

    def __init__(self, pool, **kw):
        super().__init__(pool.fix_error, **kw)
        self.pool, self.recorded, self.frag_dev, self.flushed = pool, [], None, False

    def _decode_run(self, key, entries: list) -> list:
        data = self._data
        self.recorded.append((key, [(e[0] if e[0] is not None else data[e[1]:e[1] + e[2]], e[2]) for e in entries]))
        return []

    def fragment_to_host(self):
        if self.frag_dev is not None:
            self.overlap_fragment, self.frag_dev = self.frag_dev.cpu().numpy(), None
            self.pool.fragment_downloads += 1

    def drain(self) -> list:
        """Decode what the tick recorded by the inherited per-stream path, run after run -> the pieces"""
        runs, self.recorded = self.recorded, []
        if not runs:
            return []
        self.fragment_to_host()
        pieces = []
        for key, run in runs:
            pieces.extend(Decoder._decode_run(self, key, [(p, 0, nb) for p, nb in run]))
        return pieces

    def flush(self) -> DecodeResult:
        pieces = self.drain()
        self.fragment_to_host()
        self.flushed = True
        r = Decoder.flush(self)
        return DecodeResult(pieces + [r.pcm], r.srate, 0, False) if pieces else r


class DecoderPool:
    def __init__(self, fix_error: bool = False, out_format: str | None = None, device_inflate: bool = False, as_tensor: bool = False,
                 max_batch_bytes: int = 1 << 30, bridge=None):
        """``fix_error``, ``out_format`` and ``device_inflate`` mean what they mean for ``Decoder``.  ``as_tensor``: ``pcm``
        stays on the device as ``decode_batch(as_tensor=True)`` leaves it.  ``max_batch_bytes``: a group whose float64 frames
        would exceed it is cut into chunks of whole members."""
        if bridge is None:
            from .bridge import HipBridge
            bridge = HipBridge()
        if as_tensor and getattr(bridge, "torch", None) is None:
            raise ValueError("as_tensor needs a bridge that keeps tensors on the device")
        self.fix_error, self.out_format, self.device_inflate, self.as_tensor = fix_error, out_format, device_inflate, as_tensor
        self.max_batch_bytes, self.bridge = max_batch_bytes, bridge
        self._members, self._next = {}, 0
        self.fragment_uploads = self.fragment_downloads = 0    # host <-> device copies of carried fragments so far

    # ------------------------------------------------------------------------------------------------------------ handles
    def open(self) -> int:
        """A new stream -> its handle; handles are never reused"""
        h, self._next = self._next, self._next + 1
        self._members[h] = _Member(self, bridge=self.bridge, out_format=self.out_format, device_inflate=self.device_inflate)
        return h

    def is_empty(self, h) -> bool:
        return self._members[h].is_empty()

    def get_asfh(self, h):
        return self._members[h].get_asfh()

    def flush(self, h) -> DecodeResult:
        """The ``Decoder``'s ``flush()`` of stream h"""
        return self._finish(self._members[h].flush())

    def close(self, h) -> DecodeResult:
        """``flush(h)``, and the handle is forgotten"""
        r = self.flush(h)
        del self._members[h]
        return r

    # --------------------------------------------------------------------------------------------------------------- a tick
    def process(self, chunks: dict) -> PoolResult:
        """One tick: ``chunks[h]`` (bytes-like, may be empty) is appended to stream h; a handle that is not in the dict is not
        touched.  -> ``PoolResult``"""
        members = {h: self._members[h] for h in chunks}         # (KeyError before any stream has moved)
        res, groups = PoolResult(), {}
        for h, chunk in chunks.items():
            m = members[h]
            m.recorded, m.flushed = [], False
            r = res[h] = m.process(chunk)
            if m.flushed:                                       # its runs went through the per-stream path on the way
                res.fallback.append(h)
                self._finish(r)
            elif m.recorded:
                gkey = self._plain(m)
                if gkey is not None:
                    groups.setdefault(gkey, []).append(h)
                else:
                    res[h] = self._finish(m._narrow(DecodeResult(m.drain(), r.srate, r.frames, r.crit)))
                    res.fallback.append(h)
            else:
                self._finish(r)
        for gkey, hs in groups.items():
            N, C = gkey[1], gkey[2]
            chunk, size = [], 0
            for h in hs + [None]:
                need = 0 if h is None else len(members[h].recorded[0][1]) * N * C * 8
                if chunk and (h is None or size + need > self.max_batch_bytes):
                    self._decode_chunk(gkey, chunk, members, res)
                    chunk, size = [], 0
                if h is not None:
                    chunk.append(h)
                    size += need
        return res

    @staticmethod
    def _overlap(key) -> tuple:
        """-> (the ratio the cross-fade runs at, L): none for the lossless profiles, whatever their header's byte says"""
        profile, N, ratio = key[0], key[1], key[6]
        if profile not in DEFLATED or not ratio:
            return 0, 0
        return ratio, N - N * (ratio - 1) // ratio

    def _plain(self, m: _Member):
        """The group key of a plain tick (module docstring), None for a tick the per-stream path decodes"""
        if len(m.recorded) != 1:
            return None
        key, run = m.recorded[0]
        profile, N, C, depth, endian, srate, ratio = key
        if N < 1 or C < 1 or depth >= len(BIT_DEPTHS[profile]):
            return None
        if any(isinstance(p, Damaged) and not 1 <= p.dsize + p.codesize <= 255 for p, _ in run):
            return None
        if profile in DEFLATED:
            if ratio == 1:
                return None
            gkey = key + (None,)
        else:
            nb = run[0][1]
            if nb == 0 or (N * C * BIT_DEPTHS[profile][depth] + 7) // 8 != nb:
                return None                                     # no whole payload
            gkey = key + (nb,)                                  # equal payload length: the Decoder's run-break rule
        L = self._overlap(key)[1]
        if m.frag_dev is not None:
            return gkey if tuple(m.frag_dev.shape) == (L, C) else None
        frag = m.overlap_fragment
        return gkey if not frag.size or (frag.shape == (L, C) and m.overlap_prog == 0) else None

    def _decode_chunk(self, gkey, hs: list, members: dict, res: PoolResult):
        """The plain ticks of one group (or of a chunk of it): every stage once, one ``clips_carry_add``"""
        br, key = self.bridge, gkey[:7]
        N, C = key[1], key[2]
        ratio, L = self._overlap(key)
        on_dev = getattr(br, "torch", None) is not None         # the bridge keeps tensors: so do the fragments
        payloads, clip_frame0, prev = [], [0], []
        for h in hs:
            m = members[h]
            payloads.extend(p for p, _ in m.recorded[0][1])
            clip_frame0.append(len(payloads))
            frag = m.frag_dev
            if frag is None and m.overlap_fragment.size:
                frag = np.ascontiguousarray(m.overlap_fragment, np.float64)
                if on_dev:                                      # a fallback tick left it on the host
                    frag = br.torch.from_numpy(frag).to(br.device)
                    self.fragment_uploads += 1
            prev.append(frag)
        frames = _frames(br, key, repair(br, payloads), self.device_inflate)
        carry = getattr(br, "clips_carry_add", None)
        if carry is None:
            out, out_off, nxt = clips_carry_host(frames, clip_frame0, N, C, ratio, prev, self.out_format)
        else:
            out, out_off, nxt = carry(frames, clip_frame0, N, C, ratio, prev, self.out_format, self.as_tensor)
        step = C * ff_format_to_numpy_type(self.out_format).itemsize if self.as_tensor and self.out_format is not None else 1
        for k, h in enumerate(hs):
            m = members[h]
            m.recorded = []
            if L:
                if on_dev and not isinstance(nxt[k], np.ndarray):
                    m.frag_dev, m.overlap_fragment = nxt[k], np.array([])
                else:
                    m.frag_dev, m.overlap_fragment = None, np.asarray(nxt[k]).reshape(L, C)
            res[h].pcm = out[int(out_off[k]) * step:int(out_off[k + 1]) * step]

    def _finish(self, r: DecodeResult) -> DecodeResult:
        """as_tensor: what the per-stream path left on the host goes to the device, as ``decode_batch`` sends it"""
        if self.as_tensor and isinstance(r.pcm, np.ndarray):
            t, raw = self.bridge.torch, np.ascontiguousarray(r.pcm)
            r.pcm = t.from_numpy(raw if self.out_format is None or raw.dtype == np.float64 else raw.view(np.uint8).reshape(-1)).to(self.bridge.device)
        return r
