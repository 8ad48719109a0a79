"""What a frame is, on the host: the one place that turns a header's fields and the payload bytes into a run key and a payload
entry.  ``Decoder`` (both of its parsers), ``decode_batch`` and ``Repairer`` share it, and with it the Reed-Solomon strip /
mark / repair steps and the host inflate of the compact profiles.  No device code and no torch in here: a bridge
(bridge.py) is handed in where the device does the work."""
from __future__ import annotations

import zlib

from . import ecc
from .fourier import BIT_DEPTHS

DEFLATED = (1, 2)                                       # compact profiles: deflated Golomb bodies, cut from the stream
BUILT = (0, 1, 2, 4)


def lossless_frame_len(nbytes: int, depth_idx: int, channels: int, header_fsize: int) -> int:
    """Sample-frames a lossless payload holds.  The reference's profile0/4.digital never look at the header's fsize: they
    unpack every stored value and reshape(-1, channels) (profile0.py:46-69, profile4.py:43-63), so the payload length
    decides.  A length that is no whole number of sample-frames (the reference's reshape then raises) keeps the header
    value and fails in the launch checks."""
    depths = BIT_DEPTHS[0]                                 # profiles 0 and 4 store the same depths
    bits = depths[depth_idx] if depth_idx < len(depths) else 0
    if not bits or channels < 1:
        return header_fsize
    values = (nbytes * 2) // 3 if bits == 12 else (nbytes * 8) // bits
    return values // channels if values and values % channels == 0 else header_fsize


def strip_ecc(frad: bytes, dsize: int, codesize: int) -> bytes:
    """tools/ecc.py:14-25 with repair off: drop the Reed-Solomon code bytes of every block."""
    block = dsize + codesize
    return b"".join(frad[i:i + block][:max(len(frad[i:i + block]) - codesize, 0)] for i in range(0, len(frad), block))


class Damaged:
    """An ECC payload whose checksum fails, waiting for the batched repair of its run (frad_rs_repair)."""
    __slots__ = ("frad", "dsize", "codesize")

    def __init__(self, frad: bytes, dsize: int, codesize: int):
        self.frad, self.dsize, self.codesize = frad, dsize, codesize


def unprotect(frad: bytes, profile: int, dsize: int, csize: int, crc: int, fix_error: bool):
    """ecc.decode (decoder.py:63-68): strip the check bytes, or -- fix_error and a failing checksum -- mark the payload
    for repair.  -> (payload or Damaged, data bytes)"""
    if fix_error and ecc.needs_repair(profile, frad, crc):
        return Damaged(frad, dsize, csize), ecc.data_len(len(frad), dsize, csize)
    frad = strip_ecc(frad, dsize, csize)
    return frad, len(frad)


def repair(bridge, payloads: list) -> list:
    """The payloads with every Damaged one replaced by its repaired data part: one ``rs_repair`` batch per stored ratio."""
    groups = {}
    for i, p in enumerate(payloads):
        if isinstance(p, Damaged):
            groups.setdefault((p.dsize, p.codesize), []).append(i)
    if groups:
        payloads = list(payloads)
    for (dsize, csize), idx in groups.items():
        fixed, _, _ = bridge.rs_repair([payloads[i].frad for i in idx], dsize, csize)
        for i, f in zip(idx, fixed):
            payloads[i] = f
    return payloads


def classify(data: bytes, row, fix_error: bool):
    """One frame, from the fifteen fields of a scanner row (frad_asfh_scan; ``Decoder`` reads the same values off its ASFH)
    and the bytes the row points into.  -> (run key, (payload or None, offset, data bytes)).  Lossless payloads stay where
    they are in the stream (None, offset, length): a run of equally spaced frames goes to the device as one strided buffer;
    deflated and ECC payloads are cut out here, the latter stripped or marked for repair."""
    h_off, p_off, p_len, profile, is_ecc, le, depth, ch, srate, fsize, ratio, dsize, csize, fflush, crc = row
    if profile not in BUILT:
        raise NotImplementedError(f"profile {profile} is not built (upstream: in development)")
    frad, nb = None, p_len
    if profile in DEFLATED or is_ecc:
        frad = data[p_off:p_off + p_len]
        nb = len(frad)
        if is_ecc:
            frad, nb = unprotect(frad, profile, dsize, csize, crc, fix_error)
    if profile not in DEFLATED:
        fsize = lossless_frame_len(nb, depth, ch, fsize)
    return (profile, fsize, ch, depth, bool(le), srate, ratio), (frad, p_off, nb)


# ------------------------------------------------------------------------------------------------------- host deflate / inflate
_POOL = None


def map_zlib(fn, items: list) -> list:
    """deflate / inflate of a batch's frames on a small thread pool: zlib releases the GIL, the frames are independent and
    the results are the bytes the serial loop would give (profile1.py:50, :59).  Work is handed out in runs of frames so
    that the pool's per-task overhead (tens of microseconds) does not exceed a frame's own cost."""
    global _POOL
    n = len(items)
    if n < 32:
        return [fn(b) for b in items]
    if _POOL is None:
        import os
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4))
    workers = _POOL._max_workers
    run = max(8, -(-n // (4 * workers)))
    chunks = [items[i:i + run] for i in range(0, n, run)]
    out = []
    for part in _POOL.map(lambda ch: [fn(b) for b in ch], chunks):
        out.extend(part)
    return out


def raw_deflate(body: bytes) -> bytes:
    """the reference's zlib.compress(body, wbits=-15) (profile1.py:50, profile2.py:54): level 6, no wrapper"""
    co = zlib.compressobj(zlib.Z_DEFAULT_COMPRESSION, zlib.DEFLATED, -15)
    return co.compress(body) + co.flush()


def _inflate(frad: bytes):
    try:
        return zlib.decompress(frad, wbits=-15)
    except Exception:
        return None                                          # profile1.py:59-60, profile2.py:63-64 -> a frame of zeros


def inflate_bodies(payloads: list):
    """Inflate on the host (profile1.py:59, profile2.py:61), runs of frames per pool task.  -> (bodies, bad): a payload zlib
    rejects is an empty body -- all-zero integers on the device -- and is listed in ``bad``."""
    bodies = map_zlib(_inflate, payloads)
    bad = [i for i, b in enumerate(bodies) if b is None]
    return [b if b is not None else b"" for b in bodies], bad
