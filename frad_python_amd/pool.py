"""``DecoderPool`` and ``EncoderPool``: many live streams decoded (encoded) chunk by chunk, one device pass per tick.  The decode
side first; the encode side is described where it begins, further down.

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

from .backend.pcmformat import FORMAT_NAMES, ff_format_to_numpy_type, from_f64
from .batch import _compact_payloads, _frames, _host_bytes, _lossless_rows
from .decoder import Decoder, DecodeResult
from .encoder import Encoder, EncodeResult
from .fourier import BIT_DEPTHS
from .fourier.profiles import COMPACT, compact
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
    """One tick: ``res[h]`` is the ``DecodeResult`` (pcm, srate, frames, crit) of handle h -- from an ``EncoderPool`` its
    ``EncodeResult`` (buf, samples); ``fallback``: the handles whose tick the per-stream path decoded (encoded), in the order of
    the tick's dict."""

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


# ======================================================================================================================
# EncoderPool: the encode side's streaming shape.  ``Encoder`` is one stream each: per tick and stream it uploads
# its whole buffer -- the overlap carry again every time -- and runs a chain of launches over the two or three frames a chunk
# completes.  ``encode_batch`` runs every stage once, but wants its clips whole.  Here every member keeps an ``Encoder``'s own
# state, with the remainder behind its last whole frame on the device; one launch of ``frad_clips_carry_cut`` gathers the frames a
# tick completes -- each from what the member carried over and the chunk that just arrived -- and writes the next remainders,
# and the frames of all members go through ``batch._lossless_rows`` / ``_compact_payloads`` / ``Encoder._emit_all`` once.
# ``res[h]`` is, byte for byte, what an ``Encoder`` of its own returns from ``process(chunk)`` for the same chunk sequence.
def clips_carry_cut_host(carry: list, src, src_off, row_clip, row_at, row_len: int, step: int, next_at):
    """What ``HipBridge.clips_carry_cut`` computes, by numpy slicing, for a bridge without it.  ``carry``: per clip None or a
    uint8 ndarray of whole sample-frames; ``src``: the joined chunks, uint8.  -> (ndarray [n_rows, row_len * step], next):
    ``next[j]`` clip j's bytes from sample-frame ``next_at[j]`` on, an array of its own."""
    src = np.frombuffer(src, np.uint8) if not isinstance(src, np.ndarray) else src.reshape(-1)
    none = np.zeros(0, np.uint8)
    seq = [np.concatenate([none if c is None else np.asarray(c, np.uint8).reshape(-1), src[int(src_off[j]) * step:int(src_off[j + 1]) * step]])
           for j, c in enumerate(carry)]
    out = np.empty((len(row_clip), row_len * step), np.uint8)
    for r, (c, at) in enumerate(zip(row_clip, row_at)):
        row = seq[int(c)][int(at) * step:(int(at) + row_len) * step]
        if at < 0 or row.size != row_len * step:
            raise ValueError("a row does not end inside its clip")
        out[r] = row
    if any(not 0 <= int(a) * step <= seq[j].size for j, a in enumerate(next_at)):
        raise ValueError("0 <= next_at[j] <= the clip's sample-frames")
    return out, [seq[j][int(a) * step:].copy() for j, a in enumerate(next_at)]


class _EncMember(Encoder):
    """An ``Encoder`` whose buffer lives with the pool between plain ticks.  ``held``: its whole sample-frames behind the last
    frame written (a device uint8 tensor behind a bridge that cuts on the device, an ndarray otherwise; None: none), and the
    inherited ``buffer`` the bytes behind them -- fewer than a sample-frame while ``held`` is there, the ``Encoder``'s whole buffer
    after a fallback tick or a flush.  The ``Encoder``'s buffer is ``held ++ buffer`` at all times."""
    held = None

    def __init__(self, pool):
        pool._settings(self)
        self.pool = pool

    def to_host(self):
        if self.held is not None:
            self.buffer, self.held = _host_bytes(self.held) + self.buffer, None
            self.pool.carry_downloads += 1

    def flush(self) -> EncodeResult:
        self.to_host()
        return Encoder.flush(self)


class _Tick:
    """One member's part of a tick that brings whole sample-frames: ``pieces`` [(bytes-like or device tensor, bytes taken)] go up,
    ``new`` sample-frames in all; ``tail``: the bytes left behind them; ``k`` whole frames out of ``have`` sample-frames."""
    __slots__ = ("h", "m", "pieces", "new", "tail", "have", "k", "samples", "uploads")


class EncoderPool:
    def __init__(self, profile: int, srate: int, channels: int, bit_depth: int, frame_size: int, pcm_format: str, *,
                 overlap_ratio: int = 0, loss_level: float = 0.5, little_endian: bool = False, ecc_ratio=None,
                 allow_profile2: bool = False, device_deflate: bool = False, max_batch_bytes: int = 1 << 30, bridge=None):
        """The arguments mean what ``encode_batch``'s mean, clamping included, and what the ``Encoder`` refuses is a ``ValueError``;
        one pool has one setting.  ``max_batch_bytes``: a tick whose gathered frames would exceed it is cut into chunks of whole
        members."""
        checks = (lambda: None if (profile == 2 and allow_profile2) else Encoder.verify_profile(profile),
                  lambda: Encoder.verify_srate(profile, srate), lambda: Encoder.verify_channels(profile, channels),
                  lambda: Encoder.verify_bit_depth(profile, bit_depth), lambda: Encoder.verify_frame_size(profile, frame_size))
        for check in checks:
            e = check()
            if e is not None:
                raise ValueError(e)
        if str(pcm_format).lower() not in FORMAT_NAMES:         # (the Encoder leaves the process on this one)
            raise ValueError(f"Invalid format: {pcm_format}")
        if bridge is None:
            from .bridge import HipBridge
            bridge = HipBridge()
        self.bridge, self.max_batch_bytes = bridge, max_batch_bytes
        self._args = (profile, srate, channels, bit_depth, frame_size, pcm_format)
        self._kw = dict(allow_profile2=allow_profile2, allow_ecc=ecc_ratio is not None, device_deflate=device_deflate)
        self._set = (overlap_ratio, loss_level, little_endian, ecc_ratio)
        self._enc = Encoder.__new__(Encoder)                    # the settings, the header writer and the bridge of every tick
        self._settings(self._enc)
        enc = self._enc
        is_compact = profile in COMPACT
        self.n_eff = compact.get_samples_min_ge(enc.fsize) if is_compact else enc.fsize
        ratio = enc.asfh.overlap_ratio
        self.cut = self.n_eff * (ratio - 1) // ratio if (is_compact and ratio > 1) else self.n_eff      # Encoder.inner's hop
        self.step = enc.pcm_format.itemsize * channels
        depths = BIT_DEPTHS[profile]
        self._idx = depths.index(enc.bit_depth if enc.bit_depth in depths else 16)
        self._on_dev = getattr(bridge, "clips_carry_cut", None) is not None and getattr(bridge, "clips_join", None) is not None
        self._members, self._next = {}, 0
        self.carry_uploads = self.carry_downloads = 0          # host <-> device copies of members' buffers so far

    def _settings(self, enc: Encoder):
        """``enc`` becomes an ``Encoder`` with the pool's settings, through its constructor and setters"""
        overlap_ratio, loss_level, little_endian, ecc_ratio = self._set
        Encoder.__init__(enc, *self._args, bridge=self.bridge, **self._kw)
        enc.set_overlap_ratio(overlap_ratio)
        enc.set_loss_level(loss_level)
        enc.set_little_endian(little_endian)
        if ecc_ratio is not None:
            enc.set_ecc(True, ecc_ratio)

    # ------------------------------------------------------------------------------------------------------------ handles
    def open(self) -> int:
        """A new stream -> its handle; handles are never reused"""
        h, self._next = self._next, self._next + 1
        self._members[h] = _EncMember(self)
        return h

    def flush(self, h) -> EncodeResult:
        """The ``Encoder``'s ``flush()`` of stream h, by the per-stream path: its remainder comes down first"""
        return self._members[h].flush()

    def close(self, h) -> EncodeResult:
        """``flush(h)``, and the handle is forgotten"""
        r = self.flush(h)
        del self._members[h]
        return r

    # --------------------------------------------------------------------------------------------------------------- a tick
    def process(self, chunks: dict) -> PoolResult:
        """One tick: ``chunks[h]`` (bytes-like, or a 1-D device uint8 tensor of whole sample-frames; may be empty) is appended
        to stream h; a handle that is not in the dict is not touched.  -> ``PoolResult`` of ``EncodeResult``s.  No member
        changes before every launch of the tick has succeeded: after a device error the same call can be made again."""
        members = {h: self._members[h] for h in chunks}         # (KeyError before any stream has moved)
        step, n_eff, cut = self.step, self.n_eff, self.cut
        for chunk in chunks.values():
            if hasattr(chunk, "numel"):
                if chunk.dim() != 1 or chunk.element_size() != 1:
                    raise TypeError("a device chunk must be a 1-D uint8 tensor of the PCM's bytes")
                if chunk.numel() % step:
                    raise ValueError(f"a device chunk must hold whole sample-frames of {step} bytes")
        res, ticks, quiet = PoolResult(), [], {}
        for h, chunk in chunks.items():
            m, res[h] = members[h], EncodeResult(b"", 0)
            pend = m.buffer
            on_dev = hasattr(chunk, "numel")
            if not on_dev and not isinstance(chunk, bytes):
                chunk = bytes(chunk)
            n = chunk.numel() if on_dev else len(chunk)
            new = (len(pend) + n) // step
            left = len(pend) + n - new * step
            t = _Tick()
            if on_dev:
                head = min(len(pend), new * step)
                t.pieces = [(pend, head), (chunk, new * step - head)]
                t.tail = (pend + _host_bytes(chunk[max(0, n - left):]))[-left:] if left else b""     # (fewer than `step` bytes come down)
            else:
                data = pend + chunk if pend else chunk
                t.pieces, t.tail = [(data, new * step)], data[new * step:]
            if not new:                                         # no whole sample-frame arrived: nothing to cut or to carry
                quiet[h] = t.tail
                continue
            held = 0 if m.held is None else len(m.held) // step
            t.h, t.m, t.new, t.have, t.uploads = h, m, new, held + new, int(len(pend) >= step)
            t.k = (t.have - n_eff) // cut + 1 if t.have >= n_eff else 0
            t.samples = t.k * n_eff - (t.k - 1) * (n_eff - cut) - (n_eff - cut if m.have_carry else 0) if t.k else 0     # Encoder.inner
            ticks.append(t)
        done, deeper = [], []                                   # (a _Tick, its frames, its remainder); the ticks that fall back
        group, size = [], 0
        for t in ticks + [None]:
            need = 0 if t is None else t.k * n_eff * step
            if group and (t is None or size + need > self.max_batch_bytes):
                while group:
                    outs, nxt, bad = self._cut_and_encode(group)
                    if not bad:
                        done.extend(zip(group, outs, nxt))
                        break
                    deeper.extend(group[d] for d in bad)        # the frame-by-frame route of the Encoder decides their depths
                    group = [g for d, g in enumerate(group) if d not in set(bad)]
                group, size = [], 0
            if t is not None:
                group.append(t)
                size += need
        # ---- nothing has changed so far.  The fallback members first: each is transactional, and is put back if a later one fails
        keep = [(t.m, t.m.buffer, t.m.held, t.m.have_carry, vars(t.m.asfh).copy()) for t in deeper]
        counters = (self.carry_uploads, self.carry_downloads)
        try:
            for t in sorted(deeper, key=ticks.index):
                t.m.to_host()
                res[t.h] = Encoder.process(t.m, _host_bytes(chunks[t.h]))
                res.fallback.append(t.h)
        except BaseException:
            for m, buffer, held, have_carry, asfh in keep:
                m.buffer, m.held, m.have_carry = buffer, held, have_carry
                vars(m.asfh).update(asfh)
            self.carry_uploads, self.carry_downloads = counters
            raise
        for h, tail in quiet.items():
            members[h].buffer = tail
        for t, out, nxt in done:
            m = t.m
            m.buffer, m.held = t.tail, (nxt if len(nxt) else None)
            self.carry_uploads += t.uploads
            if t.k:
                m.have_carry = n_eff > cut
                m._head(self._idx, n_eff)                       # the header writer as its own Encoder leaves it
            res[t.h] = EncodeResult(out, t.samples)
        return res

    def _cut_and_encode(self, group: list):
        """The ticks of one chunk of members: one ``clips_carry_cut`` for every frame row and every remainder, then every stage
        once.  -> (frames per member, remainder per member, []), or (None, None, the members with a lossless frame that needs a
        deeper format): the caller sends the rest again."""
        br, enc, step, n_eff, cut = self.bridge, self._enc, self.step, self.n_eff, self.cut
        pieces = [p for t in group for p in t.pieces]
        src_off = np.zeros(len(group) + 1, np.int64)
        np.cumsum([t.new for t in group], out=src_off[1:])
        first = np.zeros(len(group) + 1, np.int64)              # member j's frames are rows first[j] : first[j + 1]
        np.cumsum([t.k for t in group], out=first[1:])
        M = int(first[-1])
        row_clip = np.repeat(np.arange(len(group), dtype=np.int32), [t.k for t in group])
        row_at = np.concatenate([cut * np.arange(t.k, dtype=np.int64) for t in group])
        carry, next_at = [t.m.held for t in group], [t.k * cut for t in group]
        if self._on_dev:
            src = br.clips_join([c for c, _ in pieces], [n for _, n in pieces])
            block, nxt = br.clips_carry_cut(carry, src, src_off, row_clip, row_at, n_eff, step, next_at)
        else:
            src = np.frombuffer(b"".join(_host_bytes(c)[:n] for c, n in pieces), np.uint8)
            block, nxt = clips_carry_cut_host(carry, src, src_off, row_clip, row_at, n_eff, step, next_at)
            block = block.tobytes()
        if not M:
            return [b""] * len(group), nxt, []
        if enc.asfh.profile not in COMPACT:
            take, bad = _lossless_rows(enc, block, M, n_eff)
            if bad is not None:
                return None, None, [j for j in range(len(group)) if any(bad[first[j]:first[j + 1]])]
            return [take(int(first[j]), t.k) if t.k else b"" for j, t in enumerate(group)], nxt, []
        made = enc._emit_all([(p, self._idx, n_eff) for p in _compact_payloads(enc, block, M, n_eff)])
        return [b"".join(made[first[j]:first[j + 1]]) for j in range(len(group))], nxt, []
