#!/usr/bin/env python3
"""Golden vectors of profile 2 (TNS) ENCODING -- runs the REFERENCE itself, on a build machine that has it.

Writes tests/golden/g8_p2_enc.npz:
  * per-frame cases: PCM bytes (format, rate, depth, loss level, N, C) -> the reference's to_f64 + profile2.analogue -> its
    inflated body, the three integer arrays decoded from it (q [N, C], tq [27, C], lpc [13, C]) and profile2.digital of its
    payload (every 8th PCM row above N = 2048, as g7_p2.npz stores them).  Every profile-2 depth, 48 / 44.1 / 8 kHz, 1 to 3
    channels, sizes 128 to 28 672 (powers of two and the 160 / 192 / 224 families), integer and float64 PCM; clicks, transients
    and noise bursts, which take the TNS branch, next to tonal frames, which do not;
  * whole streams at overlap ratio 0, 2 and 16: the reference Encoder (its AVAILABLE list patched, inside this process only,
    to admit profile 2) with the input PCM, and the reference Decoder's PCM of that stream.
The reference is loaded as oracle/gen_golden.py does; nothing in it is modified.  Re-run with:  python tools/gen_golden_p2_enc.py
"""
from __future__ import annotations

import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "g8_p2_enc.npz")

from oracle.gen_golden import load_reference  # noqa: E402
from gen_golden_p2 import signal  # noqa: E402

DEPTHS = (8, 10, 12, 14, 16, 20, 24)
RATES = (48000, 44100, 8000)
FORMATS = ("s16le", "s32le", "f64le", "s8", "u16le")
KINDS = ("click", "transient", "burst", "tonal")


def to_bytes(x: np.ndarray, fmt: str) -> bytes:
    """float PCM in [-1, 1] -> bytes of `fmt` (what a caller hands to Encoder.process)"""
    if fmt == "f64le":
        return np.ascontiguousarray(x, "<f8").tobytes()
    if fmt == "s8":
        return np.round(x * 127).astype("i1").tobytes()
    if fmt == "u16le":
        return (np.round(x * 32767) + 32768).astype("<u2").tobytes()
    if fmt == "s32le":
        return np.round(x * 2147483647).astype("<i4").tobytes()
    return np.round(x * 32767).astype("<i2").tobytes()


def main():
    fourier, pcmformat, backend, asfh, encoder, decoder = load_reference()
    p2 = fourier.profile2
    p1tools = fourier.tools.p1tools
    p2.zlib = fourier.profile1.zlib                            # the same zlib.compress(wbits=) wrapper

    def ints_of(body: bytes, N: int, C: int):
        n = struct.unpack(">H", body[:2])[0]
        lpc = p1tools.exp_golomb_rice_decode(body[2:2 + n])
        rest = body[2 + n:]
        t = struct.unpack(">I", rest[:4])[0]
        tq = p1tools.exp_golomb_rice_decode(rest[4:4 + t])
        q = p1tools.exp_golomb_rice_decode(rest[4 + t:])
        pad = lambda v, m: np.pad(v, (0, max(0, m - len(v))))[:m].astype(np.int32)
        return pad(q, N * C), pad(tq, 27 * C), pad(lpc, 13 * C)

    rng = np.random.default_rng(20261016)
    sizes = (128, 160, 192, 224, 512, 1536, 2048, 2048, 3584, 4096, 7168, 28672)
    cases = [(N, 1 + (j + n) % 3, kind) for n, N in enumerate(sizes) for j, kind in enumerate(KINDS)
             if N <= 4096 or kind in ("click", "burst")]
    meta, raw, bodies, qs, tqs, lpcs, pcms = [], [], [], [], [], [], []
    for i, (N, C, kind) in enumerate(cases):
        if N == 28672:
            C = 1
        bits, srate, fmt = DEPTHS[i % len(DEPTHS)], RATES[i % len(RATES)], FORMATS[i % len(FORMATS)]
        loss = (0.5, 0.125, 2.0)[i % 3]
        x = signal(kind, N, C, srate, rng)
        b = to_bytes(x, fmt)
        dt = pcmformat.ff_format_to_numpy_type(fmt)
        frame = pcmformat.to_f64(np.frombuffer(b, dt).reshape(-1, C), dt)
        frad, fb, ch, sr = p2.analogue(frame, bits, srate, loss)
        body = zlib.decompress(frad, wbits=-15)
        q, tq, lpc = ints_of(body, N, C)
        pcm = p2.digital(frad, fb, ch, sr, N)
        step = 1 if N <= 2048 else 8
        meta.append((N, C, bits, srate, FORMATS.index(fmt), step))
        raw.append(np.frombuffer(b, np.uint8)); bodies.append(np.frombuffer(body, np.uint8))
        qs.append(q); tqs.append(tq); lpcs.append(lpc)
        pcms.append(np.ascontiguousarray(pcm[::step]).reshape(-1))
        meta[-1] = meta[-1] + (int(loss * 1000),)
    tns = np.mean([np.any(v) for v in lpcs])
    print(f"{len(meta)} frames, {tns:.0%} with non-zero LPC")
    assert 0.5 <= tns < 1.0, "the cases do not cover both TNS and plain frames"

    fourier.AVAILABLE.append(2)                                # encoder.py imported this very list
    streams, sraw, spcm, smeta = [], [], [], []
    try:
        for ratio, bits, fsize, srate, fmt in ((0, 16, 512, 48000, "s16le"), (2, 20, 600, 44100, "s32le"), (16, 10, 256, 48000, "s16le")):
            C, n = 2, 4 * fsize + fsize // 3
            x = np.concatenate([signal(k, n // 4, C, srate, rng) for k in ("click", "tonal", "transient", "burst")])
            x = np.concatenate([x, signal("tonal", n - len(x), C, srate, rng)])
            b = to_bytes(x, fmt)
            enc = encoder.Encoder(2, srate, C, bits, fsize, fmt)
            enc.set_overlap_ratio(ratio)
            enc.set_loss_level(0.5)
            out = enc.process(b).buf + enc.flush().buf
            dec = decoder.Decoder()                            # byte by byte: see tools/gen_golden_p2.py
            parts = [dec.process(out[i:i + 1]).pcm for i in range(len(out))] + [dec.flush().pcm]
            pcm = np.concatenate([p.reshape(-1, C) for p in parts])
            streams.append(np.frombuffer(out, np.uint8)); sraw.append(np.frombuffer(b, np.uint8)); spcm.append(pcm.reshape(-1))
            smeta.append((ratio, bits, fsize, srate, C, FORMATS.index(fmt), len(pcm)))
    finally:
        fourier.AVAILABLE.remove(2)

    def cat(parts, dtype):
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return np.concatenate(parts).astype(dtype), off

    out = {}
    for name, parts, dt in (("raw", raw, np.uint8), ("body", bodies, np.uint8), ("q", qs, np.int32), ("tq", tqs, np.int32),
                            ("lpc", lpcs, np.int32), ("pcm", pcms, np.float64), ("stream", streams, np.uint8),
                            ("stream_raw", sraw, np.uint8), ("stream_pcm", spcm, np.float64)):
        out[name], out[name + "_off"] = cat(parts, dt)
    np.savez_compressed(OUT, meta=np.array(meta, np.int64), stream_meta=np.array(smeta, np.int64),
                        formats=np.array(FORMATS), **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
