"""Streaming decoder with the reference's API (src/libfrad/decoder.py): ``Decoder(fix_error)``,
``process(bytes) -> DecodeResult``, ``flush()``, ``is_empty()``, ``get_asfh()``.  Frame headers are parsed
on the host exactly as the reference does; runs of consecutive frames with identical geometry are then
decoded by ONE launch of the HIP transform core (the reference decodes one frame per loop iteration,
decoder.py:55-80), and the compact profiles' Hann cross-fade runs on the device as well."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from . import common, ecc
from .fourier import profiles
from .tools.asfh import ASFH
from .backend.pcmformat import from_f64

_LOSSLESS_DEPTHS = (12, 16, 24, 32, 48, 64)
_P1_DEPTHS = (8, 12, 16, 24, 32, 48, 64)
_P2_DEPTHS = (8, 10, 12, 14, 16, 20, 24)                 # fourier/profile2.py:7
_DEFLATED = (1, 2)                                      # compact profiles: deflated Golomb bodies, cut from the stream
_BUILT = (0, 1, 2, 4)


class DecodeResult:
    def __init__(self, pcm: list, srate: int, frames: int, crit: bool):
        pcm = [p for p in pcm if p.size]
        self.pcm = (pcm[0] if len(pcm) == 1 else np.concatenate(pcm)) if pcm else np.array([])
        if pcm and self.pcm.dtype != pcm[0].dtype:             # concatenate drops a big-endian byte order (out_format)
            self.pcm = self.pcm.astype(pcm[0].dtype)
        self.srate = srate
        self.frames = frames
        self.crit = crit


def _lossless_frame_len(nbytes: int, depth_idx: int, channels: int, header_fsize: int) -> int:
    """Sample-frames a lossless payload holds.  The reference's profile0/4.digital never look at the header's fsize: they
    unpack every stored value and reshape(-1, channels) (profile0.py:46-69, profile4.py:43-63), so the payload length
    decides.  A length that is no whole number of sample-frames (the reference's reshape then raises) keeps the header
    value and fails in the launch checks."""
    bits = _LOSSLESS_DEPTHS[depth_idx] if depth_idx < len(_LOSSLESS_DEPTHS) else 0
    if not bits or channels < 1:
        return header_fsize
    values = (nbytes * 2) // 3 if bits == 12 else (nbytes * 8) // bits
    return values // channels if values and values % channels == 0 else header_fsize


def _strip_ecc(frad: bytes, dsize: int, codesize: int) -> bytes:
    """tools/ecc.py:14-25 with repair off: drop the Reed-Solomon code bytes of every block."""
    block = dsize + codesize
    return b"".join(frad[i:i + block][:max(len(frad[i:i + block]) - codesize, 0)] for i in range(0, len(frad), block))


class _Damaged:
    """An ECC payload whose checksum fails, waiting for the batched repair of its run (frad_rs_repair)."""
    __slots__ = ("frad", "dsize", "codesize")

    def __init__(self, frad: bytes, dsize: int, codesize: int):
        self.frad, self.dsize, self.codesize = frad, dsize, codesize


class Decoder:
    def __init__(self, fix_error: bool = False, *, bridge=None, out_format: str | None = None, device_inflate: bool = False):
        """``fix_error``: ECC frames whose stored checksum does not match are repaired (Reed-Solomon, on the device) before
        they are decoded; a block that cannot be corrected becomes zero bytes (decoder.py:63-68, tools/ecc.py:14-25).
        ``out_format`` (extension): a PCM format name; DecodeResult.pcm then holds ``from_f64(pcm, fmt).astype(fmt)``
        -- what the reference's caller computes right after every process() (src/decoder.py:23) -- done on the device
        for the bulk path, so that 2-8 bytes per sample cross PCIe instead of 8.
        ``device_inflate`` (extension, opt-in): a run of profile-1 / profile-2 frames is inflated on the device
        (frad_inflate_raw) and decoded there from the deflated payloads on, so the inflated bodies never visit the host; a
        run with a frame that does not inflate there is decoded by the host-inflate path as a whole."""
        self.out_format = out_format
        self.asfh = ASFH()
        self.info = ASFH()
        self.buffer = b""
        self._data, self._pos = b"", 0
        self.overlap_fragment = np.array([])          # tail of the last compact frame, [L, C]
        self.overlap_prog = 0                         # rows of the fragment already cross-faded (decoder.py:25, 36): persists across frames and calls
        self.fix_error = fix_error
        self.broken_frame = False
        self._bridge = bridge
        self.device_inflate = device_inflate

    @property
    def bridge(self):
        if self._bridge is None:
            from .bridge import HipBridge
            self._bridge = HipBridge()
        return self._bridge

    def is_empty(self) -> bool:
        return len(self.buffer) < len(common.FRM_SIGN) or self.broken_frame

    def get_asfh(self) -> ASFH:
        return self.asfh

    # ------------------------------------------------------------------ batched decode of one run of frames
    def _decode_run(self, key, entries: list) -> list:
        pieces = self._decode_run_f64(key, entries)
        if self.out_format is not None:                        # whatever did not come narrowed from the device
            pieces = [from_f64(p, self.out_format) if p.dtype == np.float64 else p for p in pieces]
        return pieces

    def _decode_run_f64(self, key, entries: list) -> list:
        """entries: (payload bytes or None, offset in self._data, length) per frame of the run"""
        profile, fsize, channels, depth_idx, endian, srate, ratio = key
        entries = self._repair(entries)
        strided = getattr(self.bridge, "lossless_decode_strided", None)
        if (profile not in _DEFLATED and strided is not None and len(entries) > 1 and all(e[0] is None for e in entries)):
            step = entries[1][1] - entries[0][1]
            if step > 0 and all(entries[i + 1][1] - entries[i][1] == step for i in range(len(entries) - 1)):
                first, nb = entries[0][1], entries[0][2]
                region = memoryview(self._data)[first:entries[-1][1] + nb]
                narrow = self.out_format if not self.overlap_fragment.size else None
                if narrow is not None:
                    pcm = strided(profile, region, len(entries), step, nb, fsize, channels, _LOSSLESS_DEPTHS[depth_idx], endian, out_format=narrow)
                else:
                    pcm = strided(profile, region, len(entries), step, nb, fsize, channels, _LOSSLESS_DEPTHS[depth_idx], endian)
                if pcm is not None:
                    if self.overlap_fragment.size:
                        return self._overlap_host(pcm, key)
                    return [pcm.reshape(-1, channels)]             # one piece: no per-frame list, no concatenate
        payloads = [e[0] if e[0] is not None else self._data[e[1]:e[1] + e[2]] for e in entries]
        if profile in _DEFLATED and self.device_inflate:
            got = self._decode_run_device_inflate(key, payloads)
            if got is not None:
                return got
        if profile in _DEFLATED:
            bits = (_P1_DEPTHS if profile == 1 else _P2_DEPTHS)[depth_idx]
            # inflate on the host (profile1.py:59, profile2.py:61); Golomb decode + dequantise (+ TNS) + IDCT behind the bridge
            # (on the device)
            def inflate(frad):
                try:
                    return zlib.decompress(frad, wbits=-15)
                except Exception:
                    return None                                      # profile1.py:59-60, profile2.py:63-64 -> a frame of zeros
            from .encoder import _map_zlib
            bodies = _map_zlib(inflate, payloads)                  # runs of frames per pool task
            bad = [i for i, b in enumerate(bodies) if b is None]
            bodies = [b if b is not None else b"" for b in bodies]
            fused = getattr(self.bridge, "p1_decode_run" if profile == 1 else "p2_decode_run", None)
            L = fsize - fsize * (ratio - 1) // ratio if ratio else 0
            if fused is not None and ratio != 0 and (not self.overlap_fragment.size or self.overlap_fragment.shape == (L, channels)):
                # the whole run on the device: Golomb decode, K8, the cross-fade and the output conversion; an undecodable frame
                # is an empty body = all-zero integers = a frame of zeros (profile1.py:59-60) before the cross-fade, as in the reference
                prev = self.overlap_fragment if self.overlap_fragment.size else None
                pcm, self.overlap_fragment = fused(bodies, fsize, channels, bits, srate, ratio, prev, self.out_format)
                return [pcm]
            pcm = (self.bridge.p1_decode_bodies if profile == 1 else self.bridge.p2_decode_bodies)(bodies, fsize, channels, bits, srate)
            for i in bad:
                pcm[i] = 0.0
        else:
            pcm = self.bridge.lossless_decode(profile, payloads, fsize, channels, _LOSSLESS_DEPTHS[depth_idx], endian)
        return self._finish_run(pcm, key)

    def _decode_run_device_inflate(self, key, payloads: list):
        """device_inflate=True: the run's deflated payloads go to the device as they are (frad_inflate_raw, then the same
        chain as the host-inflate path takes).  None when a frame does not inflate there: the caller's host path then decodes
        the whole run, which keeps a frame zlib rejects a frame of zeros (profile1.py:59-60, profile2.py:63-64)."""
        profile, fsize, channels, depth_idx, endian, srate, ratio = key
        if getattr(self.bridge, "decode_run_deflated", None) is None:
            return None                                              # a bridge without a device inflate (CPU-only tests)
        bits = (_P1_DEPTHS if profile == 1 else _P2_DEPTHS)[depth_idx]
        L = fsize - fsize * (ratio - 1) // ratio if ratio else 0
        if ratio != 0 and (not self.overlap_fragment.size or self.overlap_fragment.shape == (L, channels)):
            prev = self.overlap_fragment if self.overlap_fragment.size else None
            got = self.bridge.decode_run_deflated(profile, payloads, fsize, channels, bits, srate, ratio, prev, self.out_format)
            if got is None:
                return None
            pcm, self.overlap_fragment = got
            return [pcm]
        pcm = self.bridge.decode_bodies_deflated(profile, payloads, fsize, channels, bits, srate)
        if pcm is None:
            return None
        return self._finish_run(pcm, key)

    def _repair(self, entries: list) -> list:
        """Replace the run's damaged payloads by their repaired data parts: one frad_rs_repair batch per stored ratio."""
        groups = {}
        for i, e in enumerate(entries):
            if isinstance(e[0], _Damaged):
                groups.setdefault((e[0].dsize, e[0].codesize), []).append(i)
        if not groups:
            return entries
        entries = list(entries)
        for (dsize, csize), idx in groups.items():
            if not 1 <= dsize + csize <= 255:
                raise ValueError(f"Reed-Solomon blocks of {dsize} + {csize} bytes cannot be decoded")
            fixed, _, _ = self.bridge.rs_repair([entries[i][0].frad for i in idx], dsize, csize)
            for i, f in zip(idx, fixed):
                entries[i] = (f, entries[i][1], entries[i][2])
        return entries

    def _unprotect(self, frad: bytes, profile: int, dsize: int, csize: int, crc: int):
        """ecc.decode (decoder.py:63-68): strip the check bytes, or -- fix_error and a failing checksum -- mark the payload
        for repair.  -> (payload or _Damaged, data bytes)"""
        if self.fix_error and ecc.needs_repair(profile, frad, crc):
            return _Damaged(frad, dsize, csize), ecc.data_len(len(frad), dsize, csize)
        frad = _strip_ecc(frad, dsize, csize)
        return frad, len(frad)

    def _finish_run(self, pcm: np.ndarray, key) -> list:
        profile, fsize, channels, depth_idx, endian, srate, ratio = key
        if profile in profiles.COMPACT and ratio != 0:
            # Hann cross-fade against the previous frame's tail (decoder.py:28-46) on the device
            L = fsize - fsize * (ratio - 1) // ratio
            prev = self.overlap_fragment if self.overlap_fragment.shape == (L, channels) else None
            if prev is None and self.overlap_fragment.size:
                return self._overlap_host(pcm, key)                 # geometry changed between frames: rare, host path
            out, tail = self.bridge.overlap_add(pcm, ratio, prev)
            self.overlap_fragment = tail
            return list(out)
        if self.overlap_fragment.size:
            return self._overlap_host(pcm, key)
        return list(pcm)

    def _overlap_host(self, pcm: np.ndarray, key) -> list:
        """decoder.py:28-46 verbatim semantics for the odd cases (fragment of another length)."""
        profile, fsize, channels, depth_idx, endian, srate, ratio = key
        out = []
        for frame in pcm:
            frame = frame.copy()
            L = len(self.overlap_fragment)
            if L:
                w = 0.5 * (1 - np.cos(np.pi * np.arange(1, L + 1) / (L + 1)))
                n = min(L - self.overlap_prog, len(frame))
                i = np.arange(n) + self.overlap_prog
                frame[:n] = frame[:n] * w[i, None] + self.overlap_fragment[i] * w[L - 1 - i, None]
                self.overlap_prog += n
            if L <= self.overlap_prog:
                self.overlap_fragment, self.overlap_prog = np.array([]), 0
                if profile in profiles.COMPACT and ratio != 0:
                    cut = len(frame) * (ratio - 1) // ratio
                    self.overlap_fragment, frame = frame[cut:], frame[:cut]
            out.append(frame)
        return out

    # ------------------------------------------------------------------ stream parsing
    # The parser walks `self._data` with a cursor (`self._pos`) instead of re-slicing the byte string after
    # every header and payload: a 10-minute stream handed over in one process() call would otherwise copy
    # its remaining tail ~4 times per frame.  `self.buffer` holds the unconsumed bytes between calls.
    def _lock_on_signature(self) -> bool:
        """Position the parser on the next FRM_SIGN (decoder.py:82-90): True once a header has begun."""
        sign = common.FRM_SIGN
        if self.asfh.buffer[:len(sign)] == sign:
            return True
        at = self._data.find(sign, self._pos)
        if at < 0:
            self._pos = max(self._pos, len(self._data) - (len(sign) - 1))     # keep a possible split signature
            return False
        self.asfh.buffer = sign
        self._pos = at + len(sign)
        return True

    def _read_header(self) -> str:
        """Feed the header parser a window that always covers a whole header (<= 40 bytes)."""
        window = self._data[self._pos:self._pos + 64]
        state, rest = self.asfh.read(window)
        self._pos += len(window) - len(rest)
        return state

    def _take_frame(self, stream_was_empty: bool):
        """Cut the payload of the header just completed; None while it is still arriving."""
        need = self.asfh.frmbytes
        self.broken_frame = False
        if len(self._data) - self._pos < need:
            self.broken_frame = stream_was_empty                # process(b'') marks a truncated frame (decoder.py:58-60)
            return None
        off = self._pos
        self._pos += need
        a = self.asfh
        if a.profile not in _BUILT:
            raise NotImplementedError(f"profile {a.profile} is not built (upstream: in development)")
        # lossless payloads stay where they are in the stream (offset, length): a run of equally spaced frames goes to
        # the device as one strided buffer; everything else is cut out here
        frad, nb = None, need
        if a.profile in _DEFLATED or a.ecc:
            frad = self._data[off:off + need]
            nb = len(frad)
            if a.ecc:
                frad, nb = self._unprotect(frad, a.profile, a.ecc_dsize, a.ecc_codesize, int.from_bytes(a.crc, "big"))
        fsize = a.fsize if a.profile in _DEFLATED else _lossless_frame_len(nb, a.bit_depth_index, a.channels, a.fsize)
        key = (a.profile, fsize, a.channels, a.bit_depth_index, a.endian, a.srate, a.overlap_ratio)
        a.clear()
        return key, (frad, off, nb)

    def process(self, stream: bytes) -> DecodeResult:
        """Parse as the reference does (decoder.py:51-108) but decode runs of like frames in one launch each."""
        if not isinstance(stream, (bytes, bytearray)):
            stream = bytes(stream)                              # memoryview and friends: the parser searches with bytes.find
        self._data, self._pos = (self.buffer + stream) if self.buffer else stream, 0
        try:
            res = self._process(len(stream) == 0)
        finally:
            self.buffer, self._data, self._pos = self._data[self._pos:], b"", 0
        return self._narrow(res)

    def _narrow(self, res: DecodeResult) -> DecodeResult:
        """out_format: pieces that did not come narrowed from the device (float64) are converted here"""
        if self.out_format is not None and res.pcm.dtype == np.float64 and res.pcm.size:
            res.pcm = from_f64(res.pcm, self.out_format)
        return res

    def _process(self, stream_was_empty: bool) -> DecodeResult:
        pieces, frames = [], 0
        run_key, run = None, []

        def close_run():
            nonlocal run_key, run
            if run:
                pieces.extend(self._decode_run(run_key, run))
            run_key, run = None, []

        while True:
            if self.asfh.all_set:
                got = self._take_frame(stream_was_empty)
                if got is None:
                    break
                key, frad = got
                if key != run_key or (key[0] not in _DEFLATED and run and frad[2] != run[0][2]):
                    close_run()
                    run_key = key
                run.append(frad)
                frames += 1
                continue
            if not self.asfh.buffer and self._scan is not None:
                # steady state (no half-read header carried over): the native scanner (frad_asfh_scan) lists every
                # complete frame ahead in one pass; whatever it cannot finish is left to the byte-wise parser below
                stop = self._take_scanned(pieces, close_run, lambda k, e: self._append(k, e))
                frames += self._scanned_frames
                run_key, run = self._run_key, self._run
                if stop == "flush":
                    close_run()
                    pieces.append(self.flush().pcm)
                    break
                if stop == "crit":
                    close_run()
                    pieces.append(self.flush().pcm)
                    return DecodeResult(pieces, self._crit_srate, frames, True)
                if stop == "end":
                    break
                # "partial": fall through, the byte-wise parser takes the unfinished header / payload
            if not self._lock_on_signature():
                break
            state = self._read_header()
            if state == "Incomplete":
                break
            if state == "ForceFlush":
                close_run()
                pieces.append(self.flush().pcm)
                break
            if not self.asfh.criteq(self.info):                 # channel count or sample rate changed
                previous = (self.info.srate, self.info.channels)
                self.info = self.asfh
                if any(previous):
                    close_run()
                    pieces.append(self.flush().pcm)
                    return DecodeResult(pieces, previous[0], frames, True)
        close_run()
        return DecodeResult(pieces, self.asfh.srate, frames, False)

    # ------------------------------------------------------------------ table-driven parsing (native scanner)
    @property
    def _scan(self):
        """frad_asfh_scan of the loaded C-ABI library, or None when the bridge is not the HIP one (CPU-only tests keep the
        byte-wise parser, which is the reference's algorithm)."""
        lib = getattr(self.bridge, "scan_lib", None)
        return lib.asfh_scan if lib is not None else None

    def _append(self, key, entry):
        if key != self._run_key or (key[0] not in _DEFLATED and self._run and entry[2] != self._run[0][2]):
            if self._run:
                self._pieces.extend(self._decode_run(self._run_key, self._run))
            self._run_key, self._run = key, []
        self._run.append(entry)

    def _take_scanned(self, pieces, close_run, append) -> str:
        """Consume the frames the scanner found from self._pos on.  Returns why it stopped: 'end' (nothing more in the
        buffer), 'partial' (an unfinished header or payload follows at self._pos), 'flush' (a force-flush header was
        consumed) or 'crit' (channels / rate changed, decoder.py:93-98)."""
        self._pieces, self._scanned_frames = pieces, 0
        close_run()
        self._run_key, self._run = None, []
        table, next_pos, why = self._scan(self._data, self._pos)
        a = self.asfh
        rows = table.tolist()
        for (h_off, p_off, p_len, profile, is_ecc, le, depth, ch, srate, fsize, ratio, dsize, csize, fflush, crc) in rows:
            a.profile, a.ecc, a.endian, a.bit_depth_index = profile, bool(is_ecc), bool(le), depth
            a.channels, a.srate, a.fsize, a.frmbytes = ch, srate, fsize, p_len
            if fflush:
                self._pos = p_off
                return "flush"
            a.overlap_ratio, a.ecc_dsize, a.ecc_codesize = ratio, dsize, csize
            if not a.criteq(self.info):
                previous = (self.info.srate, self.info.channels)
                self.info = a
                if any(previous):
                    self._pos, self._crit_srate = p_off, previous[0]
                    return "crit"
            if profile not in _BUILT:
                raise NotImplementedError(f"profile {profile} is not built (upstream: in development)")
            frad, nb = None, p_len
            if profile in _DEFLATED or is_ecc:
                frad = self._data[p_off:p_off + p_len]
                nb = len(frad)
                if is_ecc:
                    frad, nb = self._unprotect(frad, profile, dsize, csize, crc)
            n_eff = fsize if profile in _DEFLATED else _lossless_frame_len(nb, depth, ch, fsize)
            key = (profile, n_eff, ch, depth, bool(le), srate, ratio)
            append(key, (frad, p_off, nb))
            self._scanned_frames += 1
            self._pos = p_off + p_len
            self.broken_frame = False
        if why == 0:                                            # FRAD_SCAN_END: keep a possibly split signature
            self._pos = max(self._pos, next_pos)
            return "end"
        return "partial"

    def flush(self) -> DecodeResult:
        ret = self.overlap_fragment
        self.overlap_fragment = np.array([])                  # (overlap_prog is left alone, as in the reference)
        self.asfh.clear()
        return self._narrow(DecodeResult([ret], self.asfh.srate, 0, False))
