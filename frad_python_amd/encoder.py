"""Streaming encoder with the reference's API (src/libfrad/encoder.py): same constructor, setters,
``process(bytes) -> EncodeResult`` and ``flush()``, byte-identical streams -- but every ``process`` call
hands ALL the whole frames it holds to the HIP transform core in one batched launch instead of looping
one frame at a time through NumPy (encoder.py:60-105).  ASFH framing and CRC stay on the host."""
from __future__ import annotations

import struct
import sys

import numpy as np

from .backend.pcmformat import ff_format_to_numpy_type
from .fourier import AVAILABLE, BIT_DEPTHS, SEGMAX, profiles
from .fourier.profiles import compact
from .frames import map_zlib, raw_deflate
from .tools.asfh import ASFH


class EncodeResult:
    def __init__(self, buf: bytes, samples: int):
        self.buf = buf
        self.samples = samples


class Encoder:
    def __init__(self, profile: int, srate: int, channels: int, bit_depth: int, frame_size: int, pcm_format: str, *, bridge=None,
                 allow_profile2: bool = False, allow_ecc: bool = False, device_deflate: bool = False):
        # profile 2 (TNS) is outside the reference's AVAILABLE list; `allow_profile2=True` admits it on this instance only
        self.allow_profile2 = bool(allow_profile2)
        # `allow_ecc=True` makes set_ecc the reference's: Reed-Solomon protection of every frame, on the device
        self.allow_ecc = bool(allow_ecc)
        # `device_deflate=True` (extension, opt-in): profiles 1 and 2 deflate on the device (frad_deflate_raw), byte-identical
        # to zlib; profiles 0 and 4 ignore it
        self.device_deflate = bool(device_deflate)
        if profile not in AVAILABLE and not (profile == 2 and self.allow_profile2):
            print(f"Invalid profile! Available: {AVAILABLE}", file=sys.stderr)
            sys.exit(1)
        self.asfh = ASFH()
        self.buffer = b""
        self.bit_depth = self.channels = self.fsize = self.srate = 0
        self.pcm_format_name = pcm_format
        self.pcm_format = ff_format_to_numpy_type(pcm_format)
        self.loss_level = 0.5
        self.init = False
        self.have_carry = False          # compact profiles: the head of `buffer` is the previous frame's tail
        self._bridge = bridge
        self.set_profile(profile, srate, channels, bit_depth, frame_size)

    # ------------------------------------------------------------------ device access
    @property
    def bridge(self):
        if self._bridge is None:
            from .bridge import HipBridge
            self._bridge = HipBridge()
        return self._bridge

    # ------------------------------------------------------------------ framing helpers
    def _head(self, depth_idx: int, fsize: int) -> ASFH:
        a = self.asfh
        a.bit_depth_index, a.channels, a.fsize = depth_idx, self.channels, fsize
        a.srate = compact.get_valid_srate(self.srate) if a.profile in profiles.COMPACT else self.srate
        return a

    def _emit(self, frad: bytes, depth_idx: int, fsize: int) -> bytes:
        if self.asfh.ecc and not self.allow_ecc:
            raise NotImplementedError("Reed-Solomon ECC is off unless the Encoder is built with allow_ecc=True")
        return self._head(depth_idx, fsize).write(frad)

    def _emit_all(self, items: list) -> list:
        """(payload, depth index, fsize) of a batch's frames -> the frames.  With ECC (encoder.py:102) every payload is
        protected and its header checksum computed on the device in one batch: crc32 for the lossless profiles, crc16_ansi
        for the compact ones; the host only writes the headers."""
        if not self.asfh.ecc or not items:
            return [self._emit(*it) for it in items]
        if not self.allow_ecc:
            raise NotImplementedError("Reed-Solomon ECC is off unless the Encoder is built with allow_ecc=True")
        dsize, cs = self.asfh.ecc_dsize, self.asfh.ecc_codesize
        payloads = [it[0] for it in items]
        if self.asfh.profile in profiles.COMPACT:
            prot, crcs = self.bridge.rs_encode_crc16(payloads, dsize, cs)
        else:
            prot, crcs = self.bridge.rs_encode(payloads, dsize, cs, crc32=True)
        return [self._head(idx, fsize).write(p, crc=c) for (_, idx, fsize), p, c in zip(items, prot, crcs)]

    _deflate = staticmethod(raw_deflate)                                          # profile1.py:50 wbits=-15

    def _encode_frames(self, pcm: bytes, n_frames: int, n_eff: int, hop: int, n_valid: int) -> bytes:
        """n_frames frames of n_eff sample-frames, frame i starting i*hop sample-frames into `pcm`."""
        prof, C = self.asfh.profile, self.channels
        out = []
        depths = BIT_DEPTHS[prof]
        if prof in profiles.COMPACT:
            bits = self.bit_depth if self.bit_depth in depths else 16                        # profile1.py:16, profile2.py:16
            N = compact.get_samples_min_ge(n_eff)
            # the quantiser (profile 2: with masking and TNS analysis) and the Exp-Golomb-Rice coder behind the bridge (on the
            # device); the host only deflates (profile1.py:50, profile2.py:54) and frames
            args = (pcm, self.pcm_format_name, n_frames, N, C, bits, compact.get_valid_srate(self.srate), self.loss_level, hop, n_valid)
            if self.device_deflate:
                payloads = getattr(self.bridge, f"p{prof}_encode_payloads")(*args)   # ... and the deflate as well
            else:
                payloads = map_zlib(self._deflate, getattr(self.bridge, f"p{prof}_encode_bodies")(*args))
            out += self._emit_all([(frad, depths.index(bits), n_valid) for frad in payloads])
        else:
            bits = self.bit_depth if self.bit_depth in depths else 16
            whole = getattr(self.bridge, "lossless_encode_stream", None)
            if whole is not None and n_frames > 1 and (not self.asfh.ecc or self.allow_ecc):
                # headers, Reed-Solomon and checksums on the device, one copy back (bridge.py); falls through when a frame escalates
                a = self.asfh
                a.bit_depth_index, a.channels, a.fsize, a.srate = depths.index(bits), C, n_eff, self.srate
                ecc_kw = {"ecc_ratio": (a.ecc_dsize, a.ecc_codesize)} if a.ecc else {}
                got = whole(prof, pcm, self.pcm_format_name, n_frames, n_eff, C, bits, a.endian, a.lossless_head, **ecc_kw)
                if got is not None:
                    return got
            out += self._emit_all([(frad, depths.index(used), n_eff) for frad, used in
                                   self.bridge.lossless_encode(prof, pcm, self.pcm_format_name, n_frames, n_eff, C, bits, self.asfh.endian)])
        return b"".join(out)

    def inner(self, stream: bytes, flush: bool) -> EncodeResult:
        """Transactional: `buffer` / `have_carry` change only after every launch of this call has succeeded, so a device
        error leaves the encoder exactly as it was before the call (nothing consumed, nothing half-emitted)."""
        if not self.init:
            self.buffer += stream
            return EncodeResult(b"", 0)
        buf, have_carry = self.buffer + stream, self.have_carry
        compact_prof = self.asfh.profile in profiles.COMPACT
        n_eff = compact.get_samples_min_ge(self.fsize) if compact_prof else self.fsize
        ratio = self.asfh.overlap_ratio
        cut = n_eff * (ratio - 1) // ratio if (compact_prof and ratio > 1) else n_eff      # encoder.py:48
        step = self.pcm_format.itemsize * self.channels
        have = len(buf) // step
        ret, samples = b"", 0
        # ---- whole frames (encoder.py:72-104, batched): frame i covers sample-frames [i*cut, i*cut + n_eff)
        if have >= n_eff:
            k = (have - n_eff) // cut + 1
            ret += self._encode_frames(buf[:((k - 1) * cut + n_eff) * step], k, n_eff, cut, n_eff)
            carry = n_eff - cut
            samples += k * n_eff - (k - 1) * carry - (carry if have_carry else 0)
            buf = buf[k * cut * step:]
            have_carry = carry > 0
        if flush:
            # ---- flush (encoder.py:81, 89-91, 105): what is left (carry + remainder) becomes one short frame
            have = len(buf) // step
            if have > 0:
                carry = (n_eff - cut) if have_carry else 0
                ret += self._encode_frames(buf[:have * step], 1, have, have, have)
                samples += have - carry
                ret += self.asfh.force_flush()
            buf, have_carry = b"", False
            ret += self.asfh.force_flush()
        self.buffer, self.have_carry = buf, have_carry
        return EncodeResult(ret, samples)

    def process(self, stream: bytes) -> EncodeResult:
        return self.inner(stream, False)

    def flush(self) -> EncodeResult:
        return self.inner(b"", True) if self.init else EncodeResult(b"", 0)

    # ------------------------------------------------------------------ getters / setters (encoder.py:114-215)
    @staticmethod
    def verify_profile(profile):
        return None if profile in AVAILABLE else f"Invalid profile! Available: {AVAILABLE}"

    @staticmethod
    def verify_srate(profile, srate):
        if srate == 0:
            return "Sample rate cannot be zero"
        if profile in profiles.COMPACT and compact.get_valid_srate(srate) != srate:
            return f"Invalid sample rate! Valid rates for profile {profile}: {compact.SRATES}"
        return None

    @staticmethod
    def verify_channels(profile, channels):
        return "Channel count cannot be zero" if channels == 0 else None

    @staticmethod
    def verify_bit_depth(profile, bit_depth):
        if bit_depth == 0:
            return "Bit depth cannot be zero"
        if bit_depth not in BIT_DEPTHS[profile]:
            return f"Invalid bit depth! Valid depths for profile {profile}: {list(BIT_DEPTHS[profile])}"
        return None

    @staticmethod
    def verify_frame_size(profile, frame_size):
        if frame_size == 0:
            return "Frame size cannot be zero"
        if frame_size > SEGMAX[profile]:
            return f"Samples per frame cannot exceed {SEGMAX[profile]}"
        return None

    def get_profile(self):
        return self.asfh.profile

    def set_profile(self, profile, srate, channels, bit_depth, frame_size):
        e_prof = None if (profile == 2 and getattr(self, "allow_profile2", False)) else self.verify_profile(profile)
        for e in (e_prof, self.verify_srate(profile, srate), self.verify_channels(profile, channels),
                  self.verify_bit_depth(profile, bit_depth), self.verify_frame_size(profile, frame_size)):
            if e is not None:
                return e
        res = EncodeResult(b"", 0)
        if (self.channels != 0 and self.channels != channels) or (self.srate != 0 and self.srate != srate):
            res = self.flush()
        self.asfh.profile = profile
        self.srate, self.channels, self.bit_depth, self.fsize = srate, channels, bit_depth, frame_size
        self.init = True
        return res

    def get_channels(self):
        return self.channels

    def set_channels(self, channels):
        res = EncodeResult(b"", 0)
        if self.channels != 0 and self.channels != channels:
            res = self.flush()
        self.channels = channels
        return res

    def get_srate(self):
        return self.srate

    def set_srate(self, srate):
        if e := self.verify_srate(self.get_profile(), srate):
            return e
        res = EncodeResult(b"", 0)
        if self.srate != 0 and self.srate != srate:
            res = self.flush()
        self.srate = srate
        return res

    def get_frame_size(self):
        return self.fsize

    def set_frame_size(self, frame_size):
        if e := self.verify_frame_size(self.get_profile(), frame_size):
            return e
        self.fsize = frame_size

    def get_bit_depth(self):
        return self.bit_depth

    def set_bit_depth(self, bit_depth):
        if e := self.verify_bit_depth(self.get_profile(), bit_depth):
            return e
        self.bit_depth = bit_depth

    def set_ecc(self, ecc: bool, ecc_ratio):
        if self.allow_ecc:                                   # encoder.py:201-209
            self.asfh.ecc = bool(ecc)
            dsize_zero, exceed_255 = ecc_ratio[0] == 0, ecc_ratio[0] + ecc_ratio[1] > 255
            if dsize_zero or exceed_255:
                if dsize_zero:
                    print("ECC data size must not be zero", file=sys.stderr)
                if exceed_255:
                    print(f"ECC data size and check size must not exceed 255, given: {ecc_ratio[0]} and {ecc_ratio[1]}", file=sys.stderr)
                print("Setting ECC to default 96 24", file=sys.stderr)
                ecc_ratio = (96, 24)
            self.asfh.ecc_dsize, self.asfh.ecc_codesize = ecc_ratio
            return
        # without the opt-in, protected streams come from Repairer(ecc_ratio).process(stream), which writes the same bytes
        if ecc:
            raise NotImplementedError("Encoder-side ECC is not built: protect the stream with "
                                      "frad_python_amd.Repairer(ecc_ratio).process(stream), which writes the same bytes")
        self.asfh.ecc = False
        self.asfh.ecc_dsize, self.asfh.ecc_codesize = ecc_ratio if ecc_ratio[0] and sum(ecc_ratio) <= 255 else (96, 24)

    def set_little_endian(self, little_endian: bool):
        self.asfh.endian = little_endian

    def set_loss_level(self, loss_level: float):
        self.loss_level = max(abs(loss_level), 0.125)

    def set_overlap_ratio(self, overlap_ratio: int):
        if overlap_ratio != 0:
            overlap_ratio = max(2, min(256, overlap_ratio))
        self.asfh.overlap_ratio = overlap_ratio
