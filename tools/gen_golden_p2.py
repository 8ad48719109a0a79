#!/usr/bin/env python3
"""Golden vectors of profile 2 (TNS) decoding -- runs the REFERENCE itself, on a build machine that has it.

Writes tests/golden/g7_p2.npz (not listed in MANIFEST.json):
  * per-frame cases: upstream profile2.analogue of a seeded frame -> its payload, and profile2.digital of that payload
    -> float64 PCM.  Sizes 128 / 1536 / 2048 / 3584 / 28672, 1-3 channels, every profile-2 depth, 48 / 44.1 / 8 kHz, and
    signals that make the encoder use TNS (clicks, transients, noise bursts) next to tonal ones.  Frames above 2048 keep
    every 8th PCM row (meta column 4 = the row step): every coefficient reaches every output row, and the file stays small;
  * whole streams at overlap ratio 0, 2 and 16: the reference Encoder (its AVAILABLE list patched, inside this process only,
    to admit profile 2, which its decoder reads but its encoder refuses) and the reference Decoder's PCM.
The reference is loaded as oracle/gen_golden.py does (bare ``libfrad`` package, inert ``reedsolo``, a ``zlib.compress(wbits=)``
wrapper); nothing in it is modified.  Re-run with:  python tools/gen_golden_p2.py
"""
from __future__ import annotations

import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g7_p2.npz")

from oracle.gen_golden import load_reference  # noqa: E402

DEPTHS = (8, 10, 12, 14, 16, 20, 24)
RATES = (48000, 44100, 8000)


def signal(kind: str, n: int, C: int, srate: int, rng) -> np.ndarray:
    t = np.arange(n) / srate
    x = np.zeros((n, C))
    for c in range(C):
        if kind == "click":                                    # a few impulses: a spectrum the LPC predicts well
            for p in rng.integers(0, n, 1 + c):
                x[p, c] += rng.uniform(0.3, 0.9) * rng.choice([-1, 1])
        elif kind == "transient":                              # silence, then a decaying tone burst
            on = int(rng.integers(n // 8, n // 2))
            env = np.where(np.arange(n) >= on, np.exp(-(np.arange(n) - on) / (0.02 * n + 1)), 0.0)
            x[:, c] = 0.8 * env * np.sin(2 * np.pi * rng.uniform(200, srate / 5) * t)
        elif kind == "burst":                                  # a short noise burst
            on, w = int(rng.integers(0, n - n // 16)), max(n // 32, 2)
            x[on:on + w, c] = rng.normal(0, 0.3, w)
        else:                                                  # tonal: two partials and a little noise
            f0 = rng.uniform(100, srate / 6)
            x[:, c] = 0.4 * np.sin(2 * np.pi * f0 * t) + 0.2 * np.sin(2 * np.pi * 2.7 * f0 * t + 1.0) + rng.normal(0, 1e-3, n)
    return np.clip(x, -1, 1)


def main():
    fourier, pcmformat, backend, asfh, encoder, decoder = load_reference()
    p2 = fourier.profile2
    p1tools, p2tools = fourier.tools.p1tools, fourier.tools.p2tools
    p2.zlib = fourier.profile1.zlib                            # the same zlib.compress(wbits=) wrapper
    from scipy import signal as ss

    def lpc_of(payload: bytes, C: int) -> np.ndarray:
        body = zlib.decompress(payload, wbits=-15)
        n = struct.unpack(">H", body[:2])[0]
        v = p1tools.exp_golomb_rice_decode(body[2:2 + n])
        return np.pad(v, (0, max(0, 13 * C - len(v))))[:13 * C].reshape(-1, C).T

    def near_edge(payload: bytes, N: int, C: int, bits: int) -> bool:
        """a channel whose filtered maximum lies within 1e-9 of tns_synthesis's 1e6 fallback edge"""
        body = zlib.decompress(payload, wbits=-15)
        n = struct.unpack(">H", body[:2])[0]
        body = body[2 + n:]
        t = struct.unpack(">I", body[:4])[0]
        fr = p1tools.dequant(p1tools.exp_golomb_rice_decode(body[4 + t:]).astype(float)) / 2.0 ** (bits - 1)
        fr = np.pad(fr, (0, max(0, N * C - len(fr)))).reshape(-1, C).T
        lpc = lpc_of(payload, C)
        for c in range(C):
            if np.any(lpc[c]):
                y = ss.lfilter([1], p2tools.dequantise_lpc(lpc[c]), fr[c])
                if abs(np.max(np.abs(y)) - 1e6) <= 1e-9 * 1e6:
                    return True
        return False

    rng = np.random.default_rng(20261015)
    meta, pays, pcms, haslpc = [], [], [], []
    kinds = ("click", "transient", "burst", "tonal")
    cases = [(N, 1 + (j + n) % 3, kind) for n, N in enumerate((128, 1536, 2048, 3584)) for j, kind in enumerate(kinds)]
    cases += [(28672, 1, "click")]
    for i, (N, C, kind) in enumerate(cases):
        bits, srate = DEPTHS[i % len(DEPTHS)], RATES[i % len(RATES)]
        x = signal(kind, N, C, srate, rng)
        frad, fb, ch, sr = p2.analogue(x, bits, srate, 0.5)
        if near_edge(frad, N, C, bits):
            continue
        pcm = p2.digital(frad, fb, ch, sr, N)
        assert pcm.shape == (N, C)
        step = 1 if N <= 2048 else 8
        meta.append((N, C, fb, sr, step))
        pays.append(np.frombuffer(frad, np.uint8))
        pcms.append(np.ascontiguousarray(pcm[::step]).reshape(-1))
        haslpc.append(bool(np.any(lpc_of(frad, C))))
    frac = np.mean(haslpc)
    print(f"{len(meta)} frames, {frac:.0%} with non-zero LPC")
    assert frac >= 0.30 and not all(haslpc), "the cases do not cover both TNS and plain frames"

    # whole streams through the reference Encoder / Decoder
    fourier.AVAILABLE.append(2)                                # encoder.py imported this very list
    streams, spcm, smeta = [], [], []
    try:
        for ratio, bits, fsize, srate in ((0, 16, 512, 48000), (2, 20, 512, 44100), (16, 10, 256, 48000)):
            C, n = 2, 4 * fsize + fsize // 3
            x = np.concatenate([signal(k, n // 4, C, srate, rng) for k in ("click", "tonal", "transient", "burst")])
            x = np.concatenate([x, signal("tonal", n - len(x), C, srate, rng)])
            pcm_bytes = (x * 32767).astype("<i2").tobytes()
            enc = encoder.Encoder(2, srate, C, bits, fsize, "s16le")
            enc.set_overlap_ratio(ratio)
            enc.set_loss_level(0.5)
            out = enc.process(pcm_bytes).buf + enc.flush().buf
            # fed byte by byte: the reference's DecodeResult cannot concatenate a frame and a force-flush piece (an empty
            # 1-D array) that arrive in the same process() call
            dec = decoder.Decoder()
            parts = [dec.process(out[i:i + 1]).pcm for i in range(len(out))] + [dec.flush().pcm]
            pcm = np.concatenate([p.reshape(-1, C) for p in parts])
            streams.append(np.frombuffer(out, np.uint8))
            spcm.append(pcm.reshape(-1))
            smeta.append((ratio, bits, fsize, srate, C, len(pcm)))
    finally:
        fourier.AVAILABLE.remove(2)

    def cat(parts, dtype):
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return (np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)), off

    pay, pay_off = cat(pays, np.uint8)
    pcm, pcm_off = cat(pcms, np.float64)
    st, st_off = cat(streams, np.uint8)
    sp, sp_off = cat(spcm, np.float64)
    np.savez_compressed(OUT, meta=np.array(meta, np.int64), payload=pay, payload_off=pay_off, pcm=pcm, pcm_off=pcm_off,
                        has_lpc=np.array(haslpc), stream=st, stream_off=st_off, stream_pcm=sp, stream_pcm_off=sp_off,
                        stream_meta=np.array(smeta, np.int64))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
