"""Host <-> device bridge used by the streaming Encoder / Decoder.

``HipBridge`` moves a batch of frames (host bytes / ndarrays, as the reference's streaming API hands
them over) through the HIP transform core: one H2D copy, one launch per homogeneous batch, one D2H
copy.  The Encoder / Decoder only depend on this small interface, which lets the CPU-only test-suite
drive their host logic (frame cut, overlap carry, ASFH, CRC) with a bridge of its own; the default
-- and the only one in this package -- is the HIP one: there is no CPU fallback.

The seam is duck-typed (no base class); a bridge is whatever has the methods its user calls:
  * Decoder / decode_batch: ``lossless_decode``, ``p1_decode_bodies`` / ``p2_decode_bodies`` (the profiles decoded) and
    ``overlap_add``; ``rs_repair`` for fix_error=True.  Optional, probed with ``getattr``: ``scan_lib`` (the native header
    scanner; without it the byte-wise parser runs and decode_batch goes stream by stream), ``lossless_decode_strided``,
    ``p1_decode_run`` / ``p2_decode_run`` (the fused run), ``compact_decode`` (HipBridge only: device inflate, and frames
    that stay on the device for decode_batch), ``clips_overlap_add``, ``clips_window_add`` (StreamIndex.decode; without it the
    windows are assembled in numpy), ``clips_resample`` (StreamIndex.decode(srate=); without it ``window.clips_resample_host``
    resamples in numpy), ``clips_remix`` (StreamIndex.decode(channels=); without it ``window.clips_remix_host`` mixes in
    numpy), ``clips_carry_add`` (DecoderPool; without it ``pool.clips_carry_host`` cross-fades in numpy), ``torch`` + ``device``
    (as_tensor).
  * Encoder: ``lossless_encode``, ``p1_encode_bodies`` / ``p2_encode_bodies``; ``p1_encode_payloads`` /
    ``p2_encode_payloads`` for device_deflate=True (``deflate_payloads`` and ``last_deflate_host`` behind them), ``rs_encode``
    and ``rs_encode_crc16`` for ECC.  Optional: ``lossless_encode_stream``.
  * encode_batch: the Encoder's methods, called once per group of frames (``lossless_encode_stream`` is not optional here); optional ``clips_join`` + ``clips_frame_cut`` (the
    clips stay on the device and one launch cuts every frame; without them the cut is numpy slicing in batch.py).
  * EncoderPool: encode_batch's methods; optional ``clips_join`` + ``clips_carry_cut`` (the members' remainders stay on the device
    and one launch cuts a tick's frames; without them ``pool.clips_carry_cut_host`` slices in numpy).
  * Repairer: ``scan_lib``, ``rs_repair``, ``rs_encode``.
``p1_encode`` and ``p1_decode`` move the bare integers (tests and tools)."""
from __future__ import annotations

import numpy as np

from . import ecc
from .backend.pcmformat import ff_format_to_numpy_type
from .frames import raw_deflate


class HipBridge:
    _pinned = None

    def __init__(self, device=None):
        import torch
        from . import core
        if not torch.cuda.is_available():
            raise RuntimeError("the FrAD transform core needs an MI355X (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.torch, self.core = torch, core
        self.scan_lib = core._lib.load()                      # frad_asfh_scan: the decoder's native header scanner
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._resample_taps = {}                              # (up, down) -> the taps on the device (clips_resample)
        self._spectrum_tables = {}                            # SpecTables.key -> (the tables, their upload) (clips_spectrum)

    def _up(self, data: bytes):
        """host bytes -> device uint8 tensor, straight from the caller's (read-only) buffer; a device tensor (the frame block
        of encode_batch) is taken as it is"""
        import warnings
        if isinstance(data, self.torch.Tensor):
            return data
        if not len(data):
            return self.torch.empty(0, dtype=self.torch.uint8, device=self.device)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # torch warns about non-writable memory; it is only read
            return self.torch.frombuffer(data, dtype=self.torch.uint8).to(self.device)

    def _down_bytes(self, dev) -> bytes:
        """device uint8 tensor -> bytes through a cached pinned staging buffer (no pageable bounce, no fresh
        page faults for the intermediate copy)"""
        t = self.torch
        n = dev.numel()
        pin = HipBridge._pinned                               # one staging buffer per process, grown on demand
        if pin is None or pin.numel() < n:
            pin = HipBridge._pinned = t.empty(max(n, 1 << 20), dtype=t.uint8, pin_memory=True)
        pin[:n].copy_(dev.reshape(-1))
        return pin[:n].numpy().tobytes()

    def lossless_encode(self, profile, pcm: bytes, fmt, n_frames, N, C, bits, little_endian, raw_be_ints=True):
        """-> list of (payload bytes, bits actually used) per frame."""
        enc = self.core.analogue_batch(profile, self._up(pcm), fmt, n_frames, N, C, bits, little_endian,
                                       raw_be_ints=raw_be_ints)
        host = enc.payload[:, :enc.nbytes].cpu().numpy()
        out = []
        for i in range(n_frames):
            if i in enc.escalated:
                row, b = enc.escalated[i]
                out.append((bytes(row.cpu().numpy()), b))
            else:
                out.append((host[i].tobytes(), enc.bits))
        return out

    def lossless_encode_stream(self, profile, pcm: bytes, fmt, n_frames, N, C, bits, little_endian, head_fn,
                               raw_be_ints=True, ecc_ratio=None):
        """Whole batch -> finished stream bytes, assembled on the device: the payload kernel writes every
        frame behind a 32-byte hole, ``frad_crc32_frames`` fills in the checksums, the constant part of the
        header (``head_fn(payload_bytes)`` -> 28 bytes, tools/asfh.py) is broadcast, and one D2H copy returns
        the result.  With ``ecc_ratio`` = (dsize, codesize) the payload kernel writes into scratch instead and
        ``frad_rs_encode_frames`` writes the protected payload (P bytes, the same for every frame) behind the
        holes; the checksum and ``head_fn(P)`` then cover the protected bytes.  None when a frame needs a deeper
        format or a 64-bit length: the caller then goes frame by frame through ``lossless_encode``."""
        t, core = self.torch, self.core
        if bits not in core.DEPTHS:
            bits = 16
        nb = core.payload_bytes(N, C, bits)
        plen = nb if ecc_ratio is None else core.rs_protected_bytes(nb, *ecc_ratio)
        self.last_escalated = []                              # on None: the frames that need a deeper format (encode_batch reads it)
        if n_frames == 0 or plen >= 0xFFFFFFFF:
            return None
        stream = t.empty((n_frames, 32 + plen), dtype=t.uint8, device=self.device)
        pay = stream[:, 32:]
        enc = core.analogue_batch(profile, self._up(pcm), fmt, n_frames, N, C, bits, little_endian,
                                  raw_be_ints=raw_be_ints, out=None if ecc_ratio else pay)
        if enc.escalated:
            self.last_escalated = sorted(enc.escalated)
            return None
        if ecc_ratio is not None:
            core.rs_encode_frames(enc.payload, nb, *ecc_ratio, out=pay)
        crc = core.crc32_frames(pay, plen)
        stream[:, :28] = t.frombuffer(bytearray(head_fn(plen)), dtype=t.uint8).to(self.device)
        stream[:, 28:32] = crc.view(t.uint8).view(n_frames, 4).flip(1)       # big-endian, as int.to_bytes(4, "big")
        return self._down_bytes(stream)

    def _down_array(self, dev, dtype, shape) -> np.ndarray:
        """device tensor -> numpy array backed by a pinned host block of its own (torch's caching host allocator hands
        the block out again once the array is gone): one DMA, no pageable bounce, no second host copy"""
        t = self.torch
        host = t.empty(dev.numel() * dev.element_size(), dtype=t.uint8, pin_memory=True)
        host.copy_(dev.reshape(-1).view(t.uint8), non_blocking=True)
        t.cuda.current_stream(self.device).synchronize()
        return host.numpy().view(dtype).reshape(shape)

    def _down_pcm(self, dev, out_format, shape) -> np.ndarray:
        """``_down_array`` of samples the device narrowed to ``out_format``, or of float64 ones without"""
        return self._down_array(dev, np.float64 if out_format is None else ff_format_to_numpy_type(out_format), shape)

    def lossless_decode_strided(self, profile, region, n_frames, stride, nbytes, N, C, bits, little_endian, out_format=None) -> np.ndarray:
        """Frames that sit equally spaced in the stream (``region`` = first payload byte .. last payload byte, a
        read-only buffer): one H2D copy of the region, headers and all, and the kernels step over it with
        ``payload_stride = stride``; no per-frame host copies."""
        if nbytes != self.core.payload_bytes(N, C, bits):
            return None                                       # header length and geometry disagree: frame-by-frame path decides
        # with out_format the samples are narrowed on the device: 2-4x fewer bytes over PCIe
        out = self.core.digital_batch(profile, self._up(region), n_frames, N, C, bits, little_endian, payload_stride=stride,
                                      out_format=out_format)
        return self._down_pcm(out, out_format, (n_frames, N, C))

    def lossless_decode(self, profile, payloads: list, N, C, bits, little_endian, keep=False):
        """equally long profile-0 / 4 payloads -> float64 frames [n, N, C]: one upload, one launch, one download; with
        ``keep`` they stay on the device (decode_batch)"""
        n, nb = len(payloads), len(payloads[0])
        stride = (nb + 15) // 16 * 16
        host = np.zeros((n, stride), np.uint8)
        host[:, :nb] = np.frombuffer(b"".join(payloads), np.uint8).reshape(n, nb)
        frames = self.core.digital_batch(profile, self.torch.from_numpy(host).to(self.device), n, N, C, bits, little_endian)
        return frames if keep else frames.cpu().numpy()

    def p1_encode(self, pcm: bytes, fmt, n_frames, N, C, bits, srate, loss_level, hop, n_valid, raw_be_ints=True):
        q, tq = self.core.p1_analogue_batch(self._up(pcm), fmt, n_frames, N, C, bits, srate, loss_level,
                                            frame_stride=hop, n_valid=n_valid, raw_be_ints=raw_be_ints)
        return q.cpu().numpy(), tq.cpu().numpy()

    def _compact_encode(self, profile, pcm: bytes, fmt, n_frames, N, C, bits, srate, loss_level, hop, n_valid, raw_be_ints=True):
        """The quantiser (profile 1: K7; profile 2: DCT, masking, TNS analysis) and the Exp-Golomb-Rice coder on the device
        (profile1.py:15-45, profile2.py:15-52) -> (flat, offsets): the pre-deflate body of frame i at
        ``flat[offsets[i]:offsets[i + 1]]``; the integers never leave the device."""
        core = self.core
        analogue, golomb = ((core.p1_analogue_batch, core.p1_golomb_encode_batch) if profile == 1 else
                            (core.p2_analogue_batch, core.p2_golomb_encode_batch))
        return golomb(*analogue(self._up(pcm), fmt, n_frames, N, C, bits, srate, loss_level, frame_stride=hop, n_valid=n_valid,
                                raw_be_ints=raw_be_ints))

    def _bodies_down(self, flat, offsets) -> list:
        """one D2H copy of exactly the body bytes"""
        off = offsets.cpu().numpy()
        host = self._down_bytes(flat) if flat.numel() else b""
        return [host[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    # p{1,2}_encode_bodies: the pre-deflate bodies, the host deflates; p{1,2}_encode_payloads: the deflate on the device too
    # (DESIGN.md 4g), the bodies stay there.  Arguments as _compact_encode's, without the profile.
    def p1_encode_bodies(self, *args, **kw) -> list:
        return self._bodies_down(*self._compact_encode(1, *args, **kw))

    def p2_encode_bodies(self, *args, **kw) -> list:
        return self._bodies_down(*self._compact_encode(2, *args, **kw))

    def p1_encode_payloads(self, *args, **kw) -> list:
        return self.deflate_payloads(*self._compact_encode(1, *args, **kw))

    def p2_encode_payloads(self, *args, **kw) -> list:
        return self.deflate_payloads(*self._compact_encode(2, *args, **kw))

    # ------------------------------------------------------------------ device deflate (Encoder(device_deflate=True))
    def deflate_payloads(self, flat, offsets) -> list:
        """Pre-deflate bodies on the device (``flat`` uint8, frame i at ``offsets[i]:offsets[i+1]``) -> the deflated payloads,
        ``zlib.compressobj(-1, DEFLATED, -15)`` of each body (profile1.py:50, profile2.py:54): frad_deflate_raw, the rows
        compacted with frad_rows_compact, one copy back of the payloads with their offsets and statuses.  A body the device
        leaves to the host (status 1: 65 274 bytes or more) is copied back alone and deflated by zlib."""
        t, core = self.torch, self.core
        n = offsets.numel() - 1
        if n == 0:
            return []
        rows, nbytes, status = core.deflate_batch(flat, offsets)
        pay_off = core.rows_offsets(rows, nbytes)
        total = int(pay_off[-1].item())                                   # the one host read: the size of the result
        head = (total + 7) // 8 * 8
        out = t.empty(head + 8 * (n + 1) + 4 * n, dtype=t.uint8, device=self.device)        # payloads | offsets | statuses
        if total:
            core.rows_gather(rows, nbytes, pay_off, out)
        out[head:head + 8 * (n + 1)].view(t.int64).copy_(pay_off)
        out[head + 8 * (n + 1):].view(t.int32).copy_(status)
        host = self._down_bytes(out)
        off = np.frombuffer(host, np.int64, n + 1, head)
        st = np.frombuffer(host, np.int32, n, head + 8 * (n + 1))
        pays = [host[off[i]:off[i + 1]] for i in range(n)]
        left = np.flatnonzero(st != 0)
        if left.size:                                                 # only these bodies come back
            boff = offsets.cpu().numpy()
            for i in left.tolist():
                body = self._down_bytes(flat[int(boff[i]):int(boff[i + 1])]) if boff[i + 1] > boff[i] else b""
                pays[i] = raw_deflate(body)
        self.last_deflate_host = int(left.size)
        return pays

    # ------------------------------------------------------------------ device inflate (Decoder(device_inflate=True))
    def inflate_run(self, payloads: list, profile: int, N, C):
        """The deflated payloads of a compact run -> their inflated bodies on the device, compacted: (bodies uint8 with the 8
        bytes of tail slack frad_p{1,2}_golomb_decode read, offsets int64 [n + 1]), or None when any frame does not inflate
        (status != 0): the caller then takes the whole run through the host's zlib.  One upload of the payloads, one
        download of two numbers."""
        t, core = self.torch, self.core
        off = np.zeros(len(payloads) + 1, np.int64)
        np.cumsum([len(p) for p in payloads], out=off[1:])
        src = self._up(b"".join(payloads))
        stride = core.golomb_bound(profile, N, C)                         # a multiple of 16
        rows, nbytes, status = core.inflate_batch(src, t.from_numpy(off).to(self.device), stride)
        offsets = core.rows_offsets(rows, nbytes)
        bad, total = t.stack([(status != 0).any().to(t.int64), offsets[-1]]).tolist()      # the one host read
        if bad:
            return None
        bodies = t.zeros(total + 8, dtype=t.uint8, device=self.device)   # 8 zeroed bytes of slack behind the last body
        if total:
            core.rows_gather(rows, nbytes, offsets, bodies)
        return bodies, offsets

    # ------------------------------------------------------------------ the compact decode chain: source, frames, sink
    def _bodies_up(self, bodies: list):
        """inflated bodies -> (flat uint8, offsets int64 [n + 1]) on the device: one upload of the bytes (about a byte per
        coefficient instead of the four of an int32 array) with the tail slack of ``inflate_run``'s"""
        off = np.zeros(len(bodies) + 1, np.int64)
        np.cumsum([len(b) for b in bodies], out=off[1:])
        flat = self._up(b"".join(bodies) + bytes(8))              # the decoder reads the stream as aligned 32-bit words (frad_hip.h)
        return flat, self.torch.from_numpy(off).to(self.device)

    def _frames_dev(self, profile, bodies, offsets, N, C, bits, srate):
        """inflated bodies on the device -> float64 frames [n, N, C] on the device (Golomb decode, K8 / p2 synthesis)"""
        if profile == 1:
            q, tq, _ = self.core.p1_golomb_decode_batch(bodies, offsets, N, C)
            return self.core.p1_digital_batch(q, tq, N, C, bits, srate)
        q, tq, lpc, _ = self.core.p2_golomb_decode_batch(bodies, offsets, N, C)
        return self.core.p2_digital_batch(q, tq, lpc, N, C, bits, srate)

    def _p2_integers(self, bodies: list, N, C):
        """inflated profile-2 bodies -> the coder's integers on the device, before the synthesis (tests/test_p2_decode.py)"""
        return self.core.p2_golomb_decode_batch(*self._bodies_up(bodies), N, C)

    def _crossfade(self, frames, ratio, prev_tail, out_format=None):
        """frames on the device through the Hann cross-fade against ``prev_tail`` (decoder.py:28-46) and -- with
        ``out_format`` -- the output conversion in the same pass -> (PCM, new tail float64) on the host"""
        t = self.torch
        pt = t.from_numpy(np.ascontiguousarray(prev_tail)).to(self.device) if prev_tail is not None else None
        out, nxt = self.core.p1_overlap_add(frames, ratio, pt, out_format=out_format)
        pcm = out.cpu().numpy()
        if out.dtype == t.uint8:
            pcm = np.frombuffer(pcm.tobytes(), ff_format_to_numpy_type(out_format))
        return pcm, nxt.cpu().numpy()

    def compact_decode(self, profile, items: list, N, C, bits, srate, deflated=False, run=None, keep=False):
        """Profile-1 / profile-2 frames of any number of streams, every stage in one call.  Source: the inflated bodies
        (an empty one is a frame of zeros, profile1.py:59-60), or -- ``deflated`` -- the payloads as they are, inflated on the
        device; None then when a frame does not inflate.  Golomb decode, K8 / p2 synthesis + inverse DCT.  Sink: the frames
        float64 [n, N, C], downloaded or -- ``keep`` -- left on the device; with ``run`` = (ratio, prev_tail, out_format)
        the run of overlapped frames goes on through the cross-fade -> (PCM [n * cut, C], new tail float64).  One upload,
        one chain, one download."""
        src = self.inflate_run(items, profile, N, C) if deflated else self._bodies_up(items)
        if src is None:
            return None
        frames = self._frames_dev(profile, *src, N, C, bits, srate)
        if run is not None:
            pcm, tail = self._crossfade(frames, *run)
            return pcm.reshape(-1, C), tail
        return frames if keep else frames.cpu().numpy()

    def p1_decode_bodies(self, bodies: list, N, C, bits, srate) -> np.ndarray:
        return self.compact_decode(1, bodies, N, C, bits, srate)

    def p2_decode_bodies(self, bodies: list, N, C, bits, srate) -> np.ndarray:
        return self.compact_decode(2, bodies, N, C, bits, srate)

    def p1_decode_run(self, bodies: list, N, C, bits, srate, ratio, prev_tail, out_format=None):
        return self.compact_decode(1, bodies, N, C, bits, srate, run=(ratio, prev_tail, out_format))

    def p2_decode_run(self, bodies: list, N, C, bits, srate, ratio, prev_tail, out_format=None):
        return self.compact_decode(2, bodies, N, C, bits, srate, run=(ratio, prev_tail, out_format))

    def clips_overlap_add(self, frames, clip_frame0, N, C, ratio, tails: list, tail_off, tail_rows, out_format=None, tail_win=None,
                          as_tensor=False):
        """The clips' cross-fade, concatenation and output conversion in one launch (core.clips_overlap_add).  ``frames``: a
        device tensor (``keep``) from compact_decode / lossless_decode, or an ndarray, ``tails``: the last-frame tensors, concatenated here in the order
        ``tail_off`` counts them.  -> (out, out_off): a device tensor with ``as_tensor``, else one download into an ndarray
        [rows, C] of float64 or of ``out_format``'s dtype."""
        t = self.torch
        dev = lambda a: a if isinstance(a, t.Tensor) else t.from_numpy(np.ascontiguousarray(a, np.float64)).to(self.device)
        frames = dev(frames) if frames is not None else None
        tails = [dev(x).reshape(-1) for x in tails]
        flat = None if not tails else tails[0] if len(tails) == 1 else t.cat(tails)
        out, out_off = self.core.clips_overlap_add(frames, clip_frame0, N, C, ratio, flat, tail_off, tail_rows, out_format, tail_win)
        if as_tensor:
            return out, out_off
        if not out.numel():
            return np.zeros((0, C), np.float64 if out_format is None else ff_format_to_numpy_type(out_format)), out_off
        return self._down_pcm(out, out_format, (-1, C)), out_off

    def clips_carry_add(self, frames, clip_frame0, N, C, ratio, prev, out_format=None, as_tensor=False):
        """The next run of whole frames of many live streams in one launch (core.clips_carry_add: DecoderPool).  ``frames`` as
        ``clips_overlap_add`` takes them; ``prev``: None, or per clip None or the fragment the stream carried in, a float64
        device tensor [L, C].  -> (out, out_off, next): ``out`` as ``clips_overlap_add`` returns it; ``next[j]`` is the
        fragment clip j carries out, on the device -- a view of one block that this call allocates, so it never is a buffer
        that ``prev`` names -- or ``prev[j]`` itself for a clip without a frame, and None where nothing is carried."""
        t = self.torch
        if frames is not None and not isinstance(frames, t.Tensor):
            frames = t.from_numpy(np.ascontiguousarray(frames, np.float64)).to(self.device)
        cf = np.asarray(clip_frame0, np.int64).reshape(-1)
        n = cf.size - 1
        cut = N * (ratio - 1) // ratio if ratio else N
        L = N - cut
        prev = list(prev) if prev is not None else [None] * n
        nxt = list(prev)
        if L and n > 0:
            block = t.empty((n, L, C), dtype=t.float64, device=self.device)
            for j in np.flatnonzero(np.diff(cf) > 0).tolist():
                nxt[j] = block[j]
        out, out_off = self.core.clips_carry_add(frames, cf, N, C, ratio, prev if L else None,
                                                 [x if x is not p else None for x, p in zip(nxt, prev)] if L else None, out_format)
        if not L:
            nxt = [None] * n
        if as_tensor:
            return out, out_off, nxt
        if not out.numel():
            return np.zeros((0, C), np.float64 if out_format is None else ff_format_to_numpy_type(out_format)), out_off, nxt
        return self._down_pcm(out, out_format, (-1, C)), out_off, nxt

    def clips_window_add(self, frames, clip_f0, clip_m, N, C, ratio, tails: list, tail_off, tail_rows, skip, valid, out_format=None,
                         tail_win=None, span=None, dst_row=None, out=None, as_tensor=False):
        """Sample windows of the clips in one launch (core.clips_window_add); ``frames`` and ``tails`` as ``clips_overlap_add``
        takes them.  Without ``dst_row`` -> (out, out_off) as ``clips_overlap_add`` returns them; with it the spans are written
        into ``out``, a device tensor that is returned as it is (the caller downloads the batch once)."""
        t = self.torch
        dev = lambda a: a if isinstance(a, t.Tensor) else t.from_numpy(np.ascontiguousarray(a, np.float64)).to(self.device)
        frames = dev(frames) if frames is not None else None
        tails = [dev(x).reshape(-1) for x in tails]
        flat = None if not tails else tails[0] if len(tails) == 1 else t.cat(tails)
        out, out_off = self.core.clips_window_add(frames, clip_f0, clip_m, N, C, ratio, flat, tail_off, tail_rows, skip, valid, out_format,
                                                  tail_win, span, dst_row, out)
        if as_tensor or dst_row is not None:
            return out, out_off
        if not out.numel():
            return np.zeros((0, C), np.float64 if out_format is None else ff_format_to_numpy_type(out_format)), out_off
        return self._down_pcm(out, out_format, (-1, C)), out_off

    def clips_resample(self, src, src_off, src_row0, src_rows, C, up, down, out_row0, valid, out_format=None, span=None, dst_row=None,
                       out=None, as_tensor=False):
        """Source spans resampled by ``up / down`` in one launch (core.clips_resample).  ``src``: a flat float64 device tensor or
        ndarray; the taps of a ratio are computed once and stay on the device.  Results as ``clips_window_add`` returns them."""
        t = self.torch
        cache = self._resample_taps
        if (up, down) not in cache:
            from .window import resample_taps
            cache[up, down] = t.from_numpy(resample_taps(up, down).copy()).to(self.device)   # (the cached array is read-only)
        if src is not None and not isinstance(src, t.Tensor):
            src = t.from_numpy(np.ascontiguousarray(src, np.float64).reshape(-1)).to(self.device)
        out, out_off = self.core.clips_resample(src, src_off, src_row0, src_rows, C, up, down, cache[up, down], out_row0, valid, out_format,
                                                span, dst_row, out)
        if as_tensor or dst_row is not None:
            return out, out_off
        if not out.numel():
            return np.zeros((0, C), np.float64 if out_format is None else ff_format_to_numpy_type(out_format)), out_off
        return self._down_pcm(out, out_format, (-1, C)), out_off

    def clips_remix(self, srcs: list, mats, C_out, valid=None, out_format=None, span=None, dst_row=None, out=None, as_tensor=False):
        """The clips' channel mix in one launch (core.clips_remix).  ``srcs``: float64 device tensors or ndarrays [rows, C_in],
        None for a clip without rows; ``mats``: a matrix per clip, or a dict with one per ``C_in``.  Results as
        ``clips_window_add`` returns them."""
        t = self.torch
        srcs = [x if x is None or isinstance(x, t.Tensor) else t.from_numpy(np.ascontiguousarray(x, np.float64)).to(self.device)
                for x in srcs]
        out, out_off = self.core.clips_remix(srcs, mats, C_out, valid, out_format, span, dst_row, out)
        if as_tensor or dst_row is not None:
            return out, out_off
        if not out.numel():
            return np.zeros((0, C_out), np.float64 if out_format is None else ff_format_to_numpy_type(out_format)), out_off
        return self._down_pcm(out, out_format, (-1, C_out)), out_off

    def clips_spectrum(self, srcs: list, valid, tables, K, frame_off, out=None):
        """The clips' spectrograms in one launch (core.clips_spectrum).  ``srcs``: float64 device tensors or ndarrays [rows, K],
        None for a clip without rows; ``tables``: a ``spectral.SpecTables``, checked and uploaded once per distinct ``key`` and
        kept on the device.  -> the device tensor [frame_off[-1], K, n_bins] (``out`` when given)."""
        t = self.torch
        srcs = [x if x is None or isinstance(x, t.Tensor) else t.from_numpy(np.ascontiguousarray(x, np.float64)).to(self.device)
                for x in srcs]
        cache, dev = self._spectrum_tables, None
        if tables.key is not None:
            if tables.key not in cache or cache[tables.key][0] is not tables:
                self.core.spectrum_tables_check(tables)
                if len(cache) >= 64:
                    cache.clear()
                cache[tables.key] = (tables, self.core.spectrum_tables_upload(tables, self.device))
            dev = cache[tables.key][1]
        return self.core.clips_spectrum(srcs, valid, tables, K, frame_off, out, dev)

    # ------------------------------------------------------------------ encode_batch: the clips' PCM, and their frames cut out
    def clips_join(self, clips: list, nbytes: list):
        """The first ``nbytes[j]`` bytes of every clip back to back in one device uint8 tensor: host clips (bytes-like) are
        joined and uploaded in one copy, device tensors (1-D uint8) are never copied to the host."""
        t = self.torch
        if not any(isinstance(c, t.Tensor) for c in clips):
            return self._up(b"".join(memoryview(c).cast("B")[:n] for c, n in zip(clips, nbytes)))
        parts = [c[:n].to(self.device) if isinstance(c, t.Tensor) else self._up(bytes(memoryview(c).cast("B")[:n])) for c, n in zip(clips, nbytes) if n]
        return t.cat(parts) if len(parts) > 1 else parts[0] if parts else t.empty(0, dtype=t.uint8, device=self.device)

    def clips_frame_cut(self, src, row_src, row_valid, row_len: int, step: int):
        """core.clips_frame_cut: fixed-length frame rows out of the joined clips, one launch -> device uint8 [rows, row_len * step],
        which the encode methods above take in place of host bytes"""
        return self.core.clips_frame_cut(src, row_src, row_valid, row_len, step)

    def clips_carry_cut(self, carry: list, src, src_off, row_clip, row_at, row_len: int, step: int, next_at):
        """The frame rows and the remainders of many live streams in one launch (core.clips_carry_cut: EncoderPool).  ``carry``:
        per clip None or what the stream carried in, a device uint8 tensor of whole sample-frames; ``src``: the chunks that just
        arrived, joined (``clips_join``), clip j's at sample-frames ``src_off[j]:src_off[j + 1]``.  -> (rows, next): ``rows``
        device uint8 [n_rows, row_len * step]; ``next[j]`` is clip j's sample-frames from ``next_at[j]`` on, on the device -- a
        view of one block that this call allocates, so it never is a buffer that ``carry`` names."""
        t = self.torch
        so = np.asarray(src_off, np.int64).reshape(-1)
        have = np.diff(so) + np.array([0 if c is None else c.numel() // step for c in carry], np.int64)
        off = np.zeros(len(carry) + 1, np.int64)
        np.cumsum((have - np.asarray(next_at, np.int64)) * step, out=off[1:])
        if (np.diff(off) < 0).any():
            raise ValueError("0 <= next_at[j] <= the clip's sample-frames")
        block = t.empty(int(off[-1]), dtype=t.uint8, device=self.device)
        nxt = [block[int(off[j]):int(off[j + 1])] for j in range(len(carry))]
        return self.core.clips_carry_cut(carry, src, so, row_clip, row_at, row_len, step, next_at, nxt), nxt

    def p1_decode(self, q: np.ndarray, tq: np.ndarray, N, C, bits, srate) -> np.ndarray:
        t = self.torch
        return self.core.p1_digital_batch(t.from_numpy(np.ascontiguousarray(q, np.int32)).to(self.device),
                                          t.from_numpy(np.ascontiguousarray(tq, np.int32)).to(self.device),
                                          N, C, bits, srate).cpu().numpy()

    def overlap_add(self, frames: np.ndarray, ratio: int, prev_tail):
        return self._crossfade(self.torch.from_numpy(np.ascontiguousarray(frames)).to(self.device), ratio, prev_tail)

    # ------------------------------------------------------------------ Reed-Solomon (csrc/frad_ecc.hip)
    def _rs_launch(self, payloads, dsize, codesize, repair=False, tail=0):
        """What the three methods below share up to the launch: one upload of ``ecc.pack``'s buffer (the payloads and the
        three offset arrays), the output buffer -- with ``tail`` bytes behind its 16-byte-aligned data for what the caller
        sends back in the same download -- and frad_rs_encode or, ``repair``, frad_rs_repair.
        -> (packed, head, out, out_off, the repair's counters or None)"""
        t, core = self.torch, self.core
        buf, head, n_blocks, out_off = ecc.pack(payloads, dsize, codesize, repair)
        packed = t.from_numpy(buf).to(self.device)                        # payloads + the three offset arrays: one H2D copy
        room = (int(out_off[-1]) + 15) // 16 * 16
        out = t.empty(room + tail if tail else max(room, 16), dtype=t.uint8, device=self.device)
        launch = core.rs_repair_packed if repair else core.rs_encode_packed
        return packed, head, out, out_off, launch(packed, head, len(payloads), n_blocks, dsize, codesize, out)

    def _rs_down(self, out, out_off, whole=False):
        """one download of the outputs (``whole``: of everything behind them too) -> (output i = host[out_off[i]:out_off[i + 1]], host)"""
        nout = int(out_off[-1])
        host = self._down_bytes(out if whole else out[:nout]) if whole or nout else b""
        return [host[out_off[i]:out_off[i + 1]] for i in range(len(out_off) - 1)], host

    def rs_encode(self, payloads: list, dsize: int, codesize: int, crc32: bool = False):
        """ecc.encode(p, dsize, codesize) of every payload (tools/ecc.py:6-12): one upload, one launch, one download.
        With ``crc32`` also zlib.crc32 of every protected payload, computed on the device (frad_crc32_frames over each run
        of equally long outputs): -> (outputs, crcs)."""
        t = self.torch
        n = len(payloads)
        if n == 0:
            return ([], []) if crc32 else []
        _, _, out, out_off, _ = self._rs_launch(payloads, dsize, codesize)
        crcs = None
        if crc32:
            lens = np.diff(out_off)
            crc_dev = t.zeros(n, dtype=t.int32, device=self.device)
            i = 0
            while i < n:                                                  # runs of equal length: one launch each
                j = i + 1
                while j < n and lens[j] == lens[i]:
                    j += 1
                L = int(lens[i])
                self.core.crc32_frames(out.as_strided((j - i, L), (L, 1), int(out_off[i])), L, out=crc_dev[i:j])
                i = j
            crcs = crc_dev.cpu().numpy().view(np.uint32).tolist()
        outs, _ = self._rs_down(out, out_off)
        return (outs, crcs) if crc32 else outs

    def rs_encode_crc16(self, payloads: list, dsize: int, codesize: int):
        """ecc.encode of every payload and common.crc16_ansi of every protected payload (the compact-profile ECC header's
        checksum), both on the device: one upload, ``frad_rs_encode`` and ``frad_crc16_ansi_frames``, one download of the
        protected bytes with the checksums behind them.  -> (outputs, crcs)"""
        t = self.torch
        n = len(payloads)
        if n == 0:
            return [], []
        packed, head, out, out_off, _ = self._rs_launch(payloads, dsize, codesize, tail=2 * n)    # protected bytes | uint16 checksums
        o = ecc.pack_layout(head, n)[3]
        off_dev = packed[o:o + 8 * (n + 1)].view(t.int64)                 # out_off, uploaded with the payloads
        crc = self.core.crc16_ansi_frames(out[:int(out_off[-1])], off_dev)
        out[out.numel() - 2 * n:].view(t.int16).copy_(crc)
        outs, host = self._rs_down(out, out_off, whole=True)
        return outs, np.frombuffer(host, np.uint16, n, len(host) - 2 * n).tolist()

    def rs_repair(self, payloads: list, dsize: int, codesize: int):
        """ecc.decode(p, dsize, codesize, repair=True) of every payload (tools/ecc.py:14-25) on the device.
        -> (data parts, corrected blocks per payload, failed blocks per payload)"""
        n = len(payloads)
        if n == 0:
            return [], np.zeros(0, np.int32), np.zeros(0, np.int32)
        _, _, out, out_off, counts = self._rs_launch(payloads, dsize, codesize, repair=True)
        outs, _ = self._rs_down(out, out_off)
        cnt = counts.cpu().numpy()
        return outs, cnt[:n].copy(), cnt[n:].copy()
