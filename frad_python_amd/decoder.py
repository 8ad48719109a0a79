"""Streaming decoder with the reference's API (src/libfrad/decoder.py): ``Decoder(fix_error)``,
``process(bytes) -> DecodeResult``, ``flush()``, ``is_empty()``, ``get_asfh()``.  Frame headers are parsed
on the host exactly as the reference does; runs of consecutive frames with identical geometry are then
decoded by ONE launch of the HIP transform core (the reference decodes one frame per loop iteration,
decoder.py:55-80), and the compact profiles' Hann cross-fade runs on the device as well."""
from __future__ import annotations

import numpy as np

from . import common
from .fourier import BIT_DEPTHS, profiles
from .frames import DEFLATED, Damaged, classify, inflate_bodies, repair
from .tools.asfh import ASFH
from .backend.pcmformat import from_f64


class DecodeResult:
    def __init__(self, pcm: list, srate: int, frames: int, crit: bool):
        pcm = [p for p in pcm if p.size]
        self.pcm = (pcm[0] if len(pcm) == 1 else np.concatenate(pcm)) if pcm else np.array([])
        if pcm and self.pcm.dtype != pcm[0].dtype:             # concatenate drops a big-endian byte order (out_format)
            self.pcm = self.pcm.astype(pcm[0].dtype)
        self.srate = srate
        self.frames = frames
        self.crit = crit


class _Runs:
    """The frames of one process() call, gathered into runs: consecutive frames of one key -- and, for the lossless
    profiles, one payload length -- are decoded together when the run breaks or the call ends.  Both parsers push here."""

    def __init__(self, decode):
        self.decode, self.pieces, self.frames = decode, [], 0
        self.key, self.run = None, []

    def push(self, key, entry):
        if key != self.key or (key[0] not in DEFLATED and self.run and entry[2] != self.run[0][2]):
            self.close()
            self.key = key
        self.run.append(entry)
        self.frames += 1

    def close(self):
        if self.run:
            self.pieces.extend(self.decode(self.key, self.run))
        self.key, self.run = None, []


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
        bits = BIT_DEPTHS[profile][depth_idx]
        strided = getattr(self.bridge, "lossless_decode_strided", None)
        if (profile not in DEFLATED and strided is not None and len(entries) > 1 and all(e[0] is None for e in entries)):
            step = entries[1][1] - entries[0][1]
            if step > 0 and all(entries[i + 1][1] - entries[i][1] == step for i in range(len(entries) - 1)):
                first, nb = entries[0][1], entries[0][2]
                region = memoryview(self._data)[first:entries[-1][1] + nb]
                narrow = self.out_format if not self.overlap_fragment.size else None
                if narrow is not None:
                    pcm = strided(profile, region, len(entries), step, nb, fsize, channels, bits, endian, out_format=narrow)
                else:
                    pcm = strided(profile, region, len(entries), step, nb, fsize, channels, bits, endian)
                if pcm is not None:
                    if self.overlap_fragment.size:
                        return self._overlap_host(pcm, key)
                    return [pcm.reshape(-1, channels)]             # one piece: no per-frame list, no concatenate
        payloads = [e[0] if e[0] is not None else self._data[e[1]:e[1] + e[2]] for e in entries]
        if profile in DEFLATED:
            on_device = self.device_inflate and getattr(self.bridge, "compact_decode", None) is not None
            return self._decode_compact(key, payloads, on_device)
        pcm = self.bridge.lossless_decode(profile, payloads, fsize, channels, bits, endian)
        return self._finish_run(pcm, key)

    def _decode_compact(self, key, payloads: list, on_device: bool) -> list:
        """A run of profile-1 / profile-2 frames.  The bodies come from the host inflate (profile1.py:59, profile2.py:61), or
        -- ``on_device``: device_inflate=True on a bridge that has it -- the deflated payloads go to the device as they are
        (frad_inflate_raw).  Golomb decode, dequantiser (+ TNS) and IDCT run behind the bridge either way; the whole run stays
        there through the cross-fade and the output conversion when the pending fragment fits."""
        profile, fsize, channels, depth_idx, endian, srate, ratio = key
        br, bits = self.bridge, BIT_DEPTHS[profile][depth_idx]
        bodies, bad = (payloads, []) if on_device else inflate_bodies(payloads)
        fused = on_device or getattr(br, f"p{profile}_decode_run", None) is not None
        L = fsize - fsize * (ratio - 1) // ratio if ratio else 0
        run = None
        if fused and ratio != 0 and (not self.overlap_fragment.size or self.overlap_fragment.shape == (L, channels)):
            # an undecodable frame is an empty body = all-zero integers = a frame of zeros (profile1.py:59-60) before the
            # cross-fade, as in the reference
            run = (ratio, self.overlap_fragment if self.overlap_fragment.size else None, self.out_format)
        if on_device:
            got = br.compact_decode(profile, bodies, fsize, channels, bits, srate, deflated=True, run=run)
            if got is None:
                # a frame does not inflate there: the host inflate decodes the whole run, which keeps a frame zlib rejects a
                # frame of zeros (profile1.py:59-60, profile2.py:63-64)
                return self._decode_compact(key, payloads, False)
        elif run is not None:
            got = getattr(br, f"p{profile}_decode_run")(bodies, fsize, channels, bits, srate, *run)
        else:
            got = getattr(br, f"p{profile}_decode_bodies")(bodies, fsize, channels, bits, srate)
        if run is not None:
            pcm, self.overlap_fragment = got
            return [pcm]
        for i in bad:
            got[i] = 0.0
        return self._finish_run(got, key)

    def _repair(self, entries: list) -> list:
        """Replace the run's damaged payloads by their repaired data parts (frames.repair)."""
        if not any(isinstance(e[0], Damaged) for e in entries):
            return entries
        for p, _, _ in entries:
            if isinstance(p, Damaged) and not 1 <= p.dsize + p.codesize <= 255:
                raise ValueError(f"Reed-Solomon blocks of {p.dsize} + {p.codesize} bytes cannot be decoded")
        return [(f, e[1], e[2]) for f, e in zip(repair(self.bridge, [e[0] for e in entries]), entries)]

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
        a, off = self.asfh, self._pos
        self.broken_frame = False
        if len(self._data) - off < a.frmbytes:
            self.broken_frame = stream_was_empty                # process(b'') marks a truncated frame (decoder.py:58-60)
            return None
        self._pos += a.frmbytes
        got = classify(self._data, (0, off, a.frmbytes, a.profile, a.ecc, a.endian, a.bit_depth_index, a.channels, a.srate, a.fsize,
                                    a.overlap_ratio, a.ecc_dsize, a.ecc_codesize, False, int.from_bytes(a.crc, "big")), self.fix_error)
        a.clear()
        return got

    def _take_header(self) -> str:
        """The byte-wise parser, the reference's algorithm (decoder.py:82-98), up to the end of the next header.  Returns
        'header' (complete: its payload is next), 'end' (no signature, or the header is still arriving), 'flush' or 'crit'."""
        if not self._lock_on_signature():
            return "end"
        state = self._read_header()
        if state == "Incomplete":
            return "end"
        if state == "ForceFlush":
            return "flush"
        return "crit" if not self.asfh.criteq(self.info) and self._crit() else "header"

    def _crit(self) -> bool:
        """The header in self.asfh differs from the last one in channel count or sample rate (decoder.py:93-98): True when
        that ends the call.  ``info`` IS ``asfh`` from here on, as in the reference, so this fires for the first header only."""
        previous = (self.info.srate, self.info.channels)
        self.info, self._crit_srate = self.asfh, previous[0]
        return any(previous)

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
        runs = _Runs(self._decode_run)
        while True:
            if self.asfh.all_set:
                got = self._take_frame(stream_was_empty)
                if got is None:
                    stop = "end"
                    break
                runs.push(*got)         # joins the scanned frames behind it: both kinds of entry are offsets into self._data
            # steady state (no half-read header carried over): the native scanner (frad_asfh_scan) lists every complete
            # frame ahead in one pass; whatever it cannot finish ('partial') is left to the byte-wise parser
            stop = self._take_scanned(runs) if not self.asfh.buffer and self._scan is not None else "partial"
            if stop == "partial":
                stop = self._take_header()
            if stop != "header":
                break
        runs.close()
        if stop in ("flush", "crit"):
            runs.pieces.append(self.flush().pcm)
        if stop == "crit":
            return DecodeResult(runs.pieces, self._crit_srate, runs.frames, True)
        return DecodeResult(runs.pieces, self.asfh.srate, runs.frames, False)

    # ------------------------------------------------------------------ table-driven parsing (native scanner)
    @property
    def _scan(self):
        """frad_asfh_scan of the loaded C-ABI library, or None when the bridge is not the HIP one (CPU-only tests keep the
        byte-wise parser, which is the reference's algorithm)."""
        lib = getattr(self.bridge, "scan_lib", None)
        return lib.asfh_scan if lib is not None else None

    def _take_scanned(self, runs: _Runs) -> str:
        """Consume the frames the scanner found from self._pos on.  Returns why it stopped: 'end' (nothing more in the
        buffer), 'partial' (an unfinished header or payload follows at self._pos), 'flush' (a force-flush header was
        consumed) or 'crit' (channels / rate changed, decoder.py:93-98)."""
        table, next_pos, why = self._scan(self._data, self._pos)
        a, data, fix_error = self.asfh, self._data, self.fix_error
        for row in table.tolist():
            h_off, p_off, p_len, profile, is_ecc, le, depth, ch, srate, fsize, ratio, dsize, csize, fflush, crc = row
            a.profile, a.ecc, a.endian, a.bit_depth_index = profile, bool(is_ecc), bool(le), depth
            a.channels, a.srate, a.fsize, a.frmbytes = ch, srate, fsize, p_len
            if fflush:
                self._pos = p_off
                return "flush"
            a.overlap_ratio, a.ecc_dsize, a.ecc_codesize = ratio, dsize, csize
            if not a.criteq(self.info) and self._crit():
                self._pos = p_off
                return "crit"
            runs.push(*classify(data, row, fix_error))
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
