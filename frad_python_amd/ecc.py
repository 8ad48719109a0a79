"""Reed-Solomon frame protection (the reference's tools/ecc.py) -- host side of ``frad_rs_encode`` / ``frad_rs_repair``.

The arithmetic runs in HIP (csrc/frad_ecc.hip).  This module holds what the host decides: the block layout of a batch
(the three offset arrays the C-ABI takes), the ratio check of the reference's Repairer, and whether a frame's stored
checksum says it needs repair."""
from __future__ import annotations

import sys
import zlib

import numpy as np

from .common import crc16_ansi
from .fourier import profiles

DEFAULT_RATIO = (96, 24)


def check_ratio(ecc_ratio) -> tuple:
    """Repairer.__init__'s validation (repairer.py:9-17): dsize 0 or dsize + codesize > 255 -> two lines on stderr and
    the default (96, 24)."""
    ecc_ratio = tuple(ecc_ratio)
    if ecc_ratio[0] == 0:
        print("ECC data size must not be zero", file=sys.stderr)
        print("Setting ECC to default 96 24", file=sys.stderr)
        ecc_ratio = DEFAULT_RATIO
    if ecc_ratio[0] + ecc_ratio[1] > 255:
        print(f"ECC data size and check size must not exceed 255, given: {ecc_ratio[0]} and {ecc_ratio[1]}", file=sys.stderr)
        print("Setting ECC to default 96 24", file=sys.stderr)
        ecc_ratio = DEFAULT_RATIO
    return ecc_ratio


def plan(lengths, dsize: int, codesize: int, repair: bool):
    """-> (in_off, blk_off, out_off), int64 [n + 1] each, as include/frad_hip.h defines them for frad_rs_encode
    (``repair`` False: blocks of dsize bytes) and frad_rs_repair (True: blocks of dsize + codesize stored bytes)."""
    lens = np.asarray(lengths, np.int64).reshape(-1)
    n = lens.size
    bin_ = dsize + codesize if repair else dsize
    if bin_ < 1:
        raise ValueError(f"Reed-Solomon block of {bin_} bytes (dsize {dsize}, codesize {codesize})")
    blocks = (lens + bin_ - 1) // bin_
    if repair:
        tail = lens - (blocks - 1) * bin_                               # length of the last block (if any)
        outl = np.where(blocks > 0, (blocks - 1) * dsize + np.maximum(tail - codesize, 0), 0)
    else:
        outl = lens + blocks * codesize
    in_off, blk_off, out_off = (np.zeros(n + 1, np.int64) for _ in range(3))
    np.cumsum(lens, out=in_off[1:])
    np.cumsum(blocks, out=blk_off[1:])
    np.cumsum(outl, out=out_off[1:])
    return in_off, blk_off, out_off


def data_len(n: int, dsize: int, codesize: int) -> int:
    """bytes ecc.decode returns for n stored bytes (with or without repair)"""
    return int(np.diff(plan([n], dsize, codesize, True)[2])[0])


def needs_repair(profile: int, frad, crc: int) -> bool:
    """The stored checksum does not match the stored (protected) payload: zlib.crc32 for the lossless profiles, crc16_ansi
    for the compact ones (decoder.py:63-68).  The reference compares the int with the header's bytes, which never match,
    and so decodes every block of every ECC frame; a block that is a codeword decodes to its data part, the bytes
    stripping gives, so the two agree on every frame whose checksum holds."""
    if profile in profiles.LOSSLESS:
        return zlib.crc32(frad) != crc
    if profile in profiles.COMPACT:
        return crc16_ansi(frad) != crc
    return False


def pack(payloads: list, dsize: int, codesize: int, repair: bool):
    """One host buffer for one upload: the payloads back to back (padded to 16 bytes) followed by in_off, blk_off and
    out_off.  -> (buffer uint8, byte offset of in_off, n_blocks, out_off)"""
    in_off, blk_off, out_off = plan([len(p) for p in payloads], dsize, codesize, repair)
    nin = int(in_off[-1])
    head = (nin + 15) // 16 * 16
    n1 = len(payloads) + 1
    buf = np.zeros(head + 24 * n1, np.uint8)
    if nin:
        buf[:nin] = np.frombuffer(b"".join(payloads), np.uint8)
    buf[head:] = np.concatenate([in_off, blk_off, out_off]).view(np.uint8)
    return buf, head, int(blk_off[-1]), out_off


def pack_layout(head: int, n: int) -> tuple:
    """byte offsets of (payloads, in_off, blk_off, out_off) in ``pack``'s buffer of n payloads: the four pointers of
    frad_rs_encode / frad_rs_repair once the buffer's address is added"""
    return 0, head, head + 8 * (n + 1), head + 16 * (n + 1)
