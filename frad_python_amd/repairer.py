"""Stream repairer with the reference's API (src/libfrad/repairer.py): ``Repairer(ecc_ratio)``, ``process(bytes) -> bytes``,
``flush()``, ``is_empty()``.  Every frame is repaired (ECC frames whose checksum fails) or stripped (ECC frames whose checksum
holds), then protected again with this Repairer's Reed-Solomon ratio and written with ``ecc`` set and the checksum of the
protected payload.  The reference does that frame by frame; here the native header scanner lists every complete frame of a
process() call, and the repair, the re-protection and the CRC-32s run as one batch each on the device (csrc/frad_ecc.hip,
frad_crc32_frames).  A stream written without ECC comes out as the reference encoder writes it with set_ecc(True, ecc_ratio)."""
from __future__ import annotations

from . import common, ecc
from .fourier import profiles
from .frames import repair, unprotect
from .tools.asfh import ASFH


class Repairer:
    def __init__(self, ecc_ratio: tuple = ecc.DEFAULT_RATIO, *, bridge=None):
        self.ecc_ratio = ecc.check_ratio(ecc_ratio)
        self.asfh = ASFH()
        self.buffer = b""
        self.fix_error = True
        self.broken_frame = False
        self._bridge = bridge

    @property
    def bridge(self):
        if self._bridge is None:
            from .bridge import HipBridge
            self._bridge = HipBridge()
        return self._bridge

    def is_empty(self) -> bool:
        return len(self.buffer) < len(common.FRM_SIGN) or self.broken_frame

    def process(self, stream: bytes) -> bytes:
        """repairer.py:27-71: bytes outside frames pass through, a force-flush header is written again and ends the call
        (what follows it waits for the next call), every complete frame is repaired and re-protected."""
        data = self.buffer + bytes(stream)
        table, next_pos, why = self.bridge.scan_lib.asfh_scan(data, 0)
        pieces, frames, pos = [], [], 0
        for row in table.tolist():
            h_off, p_off, p_len, profile, is_ecc, le, depth, ch, srate, fsize, ratio, dsize, csize, fflush, crc = row
            pieces.append(data[pos:h_off])
            if fflush:
                a = self._header(profile, is_ecc, le, depth, ch, srate, fsize, 0)
                pieces.append(a.force_flush())
                pos = p_off
                break
            frames.append((len(pieces), row))
            pieces.append(None)
            pos = p_off + p_len
            self.broken_frame = False
        else:
            if why == 2 and not len(stream):                    # FRAD_SCAN_PARTIAL_PAYLOAD on process(b''): truncated
                self.broken_frame = True
            elif why == 2:
                self.broken_frame = False
            pieces.append(data[pos:next_pos])
            pos = max(pos, next_pos)
        self.buffer = data[pos:]
        if frames:
            for (at, _), frame in zip(frames, self._protect(data, [r for _, r in frames])):
                pieces[at] = frame
        return b"".join(pieces)

    def flush(self) -> bytes:
        ret, self.buffer = self.buffer, b""
        return ret

    # ------------------------------------------------------------------ one batch of frames
    def _header(self, profile, is_ecc, le, depth, ch, srate, fsize, ratio) -> ASFH:
        a = ASFH()
        a.profile, a.ecc, a.endian, a.bit_depth_index = profile, bool(is_ecc), bool(le), depth
        a.channels, a.srate, a.fsize, a.overlap_ratio = ch, srate, fsize, ratio
        return a

    def _protect(self, data: bytes, rows: list) -> list:
        payloads = []
        for h_off, p_off, p_len, profile, is_ecc, le, depth, ch, srate, fsize, ratio, dsize, csize, fflush, crc in rows:
            frad = data[p_off:p_off + p_len]
            payloads.append(unprotect(frad, profile, dsize, csize, crc, True)[0] if is_ecc else frad)
        payloads = repair(self.bridge, payloads)                    # ecc.decode with repair: one batch per stored ratio
        dsize, csize = self.ecc_ratio
        prot, crcs = self.bridge.rs_encode(payloads, dsize, csize, crc32=True)
        out = []
        for row, frad, c in zip(rows, prot, crcs):
            h_off, p_off, p_len, profile, is_ecc, le, depth, ch, srate, fsize, ratio, _, _, fflush, crc = row
            a = self._header(profile, True, le, depth, ch, srate, fsize, ratio)
            a.ecc_dsize, a.ecc_codesize = dsize, csize
            if profile in profiles.COMPACT:
                out.append(a.write(frad))                            # crc16 of the protected payload (asfh.py:51-73)
            else:
                out.append(a.lossless_head(len(frad)) + c.to_bytes(4, "big") + frad)
        return out
