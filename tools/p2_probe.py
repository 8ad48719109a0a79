#!/usr/bin/env python3
"""Profile-2 decode on a cfg-2-sized batch (14 999 stereo frames of 2048 at 48 kHz), one process.

The integers: q / tq from the device profile-1 encoder (K7) on seeded PCM; the LPC rows tiled from the reference's own
profile-2 frames in tests/golden/g7_p2.npz (non-zero and zero rows both).  Device time (hipEvents around the launches, median
of --reps after one warm-up) of the profile-2 Golomb decode, frad_p2_synth and the inverse DCT (frad_p0_digital) separately,
the whole device chain next to profile 1's on the same q / tq, and the host wall time of HipBridge.p2_decode_run against
p1_decode_run (upload of the inflated bodies, the chain, the cross-fade at ratio 16, one download).

    python tools/p2_probe.py [--frames 14999] [--reps 5] [--json p2_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lpc_rows(path):
    """every channel's 13 LPC integers of the g7 frames"""
    import numpy as np
    from oracle import frad_oracle as fo
    d = np.load(path)
    rows = []
    for i, (N, C) in enumerate(d["meta"][:, :2].tolist()):
        body = zlib.decompress(d["payload"][d["payload_off"][i]:d["payload_off"][i + 1]].tobytes(), wbits=-15)
        n = int.from_bytes(body[:2], "big")
        v = fo.golomb_decode(body[2:2 + n])
        v = np.pad(v, (0, max(0, 13 * C - len(v))))[:13 * C].reshape(13, C)
        rows += [v[:, c] for c in range(C)]
    return np.array(rows, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14999)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import core, synth
    from frad_python_amd.bridge import HipBridge
    from oracle import frad_oracle as fo
    F, N, C, bits, sr = args.frames, 2048, 2, 16, 48000
    dev = torch.device("cuda:0")

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts[1:]))

    def wall(fn):
        ts = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[1:]))

    x = synth.to_pcm(synth.harmonic_mix(F * N, C, sr, seed=2026), "s16le")
    q, tq = core.p1_analogue_batch(torch.from_numpy(x).to(dev), "s16le", F, N, C, bits, sr, 1.0)
    pool = lpc_rows(os.path.join(ROOT, "tests", "golden", "g7_p2.npz"))
    nz = float((pool != 0).any(1).mean())
    lpc_h = np.ascontiguousarray(pool[np.arange(F * C) % len(pool)].reshape(F, C, 13).transpose(0, 2, 1))
    lpc = torch.from_numpy(lpc_h).to(dev)
    # bodies: profile 1's from the device coder; profile 2's = '>H' len + Golomb(lpc) + the profile-1 body
    flat, offs = core.p1_golomb_encode_batch(q, tq)
    host, off = flat.cpu().numpy().tobytes(), offs.cpu().numpy()
    p1_bodies = [host[off[i]:off[i + 1]] for i in range(F)]
    p2_bodies = []
    for i in range(F):
        g = fo.golomb_encode(lpc_h[i].reshape(-1))
        p2_bodies.append(len(g).to_bytes(2, "big") + g + p1_bodies[i])

    def upload(bodies):
        o = np.zeros(F + 1, np.int64)
        np.cumsum([len(b) for b in bodies], out=o[1:])
        return torch.from_numpy(np.frombuffer(b"".join(bodies) + bytes(8), np.uint8).copy()).to(dev), torch.from_numpy(o).to(dev)
    b1, o1 = upload(p1_bodies)
    b2, o2 = upload(p2_bodies)

    q2, tq2, lpc2, st = core.p2_golomb_decode_batch(b2, o2, N, C)
    assert torch.equal(q2, q) and torch.equal(tq2, tq) and torch.equal(lpc2, lpc) and not st.any(), "profile-2 Golomb decode"
    coeffs = core.p2_synth_batch(q, tq, lpc, N, C, bits, sr)
    pay = coeffs.view(torch.uint8).reshape(F, -1)
    rows = []

    def row(what, t, **kw):
        rows.append(dict(what=what, seconds=t, **kw))

    row("p1 Golomb decode (frad_p1_golomb_decode)", timed(lambda: core.p1_golomb_decode_batch(b1, o1, N, C)))
    row("p2 Golomb decode (frad_p2_golomb_decode)", timed(lambda: core.p2_golomb_decode_batch(b2, o2, N, C)))
    row("p2 TNS synthesis + ramp (frad_p2_synth)", timed(lambda: core.p2_synth_batch(q, tq, lpc, N, C, bits, sr)),
        lpc_rows_nonzero=nz)
    row("p2 synth, all LPC zero", timed(lambda: core.p2_synth_batch(q, tq, torch.zeros_like(lpc), N, C, bits, sr)))
    row("p2 inverse DCT (frad_p0_digital, 64-bit LE)", timed(lambda: core.digital_batch(0, pay, F, N, C, 64, True)))
    row("p1 K8 (frad_p1_digital)", timed(lambda: core.p1_digital_batch(q, tq, N, C, bits, sr)))
    row("p1 device chain: Golomb + K8 + overlap-add",
        timed(lambda: core.p1_overlap_add(core.p1_digital_batch(*core.p1_golomb_decode_batch(b1, o1, N, C)[:2], N, C, bits, sr), 16)))
    row("p2 device chain: Golomb + synth + IDCT + overlap-add",
        timed(lambda: core.p1_overlap_add(core.p2_digital_batch(*core.p2_golomb_decode_batch(b2, o2, N, C)[:3], N, C, bits, sr), 16)))
    br = HipBridge()
    row("HipBridge.p1_decode_run (host wall, upload + chain + download)", wall(lambda: br.p1_decode_run(p1_bodies, N, C, bits, sr, 16, None)))
    row("HipBridge.p2_decode_run (host wall, upload + chain + download)", wall(lambda: br.p2_decode_run(p2_bodies, N, C, bits, sr, 16, None)))
    for r in rows:
        print(f"{r['what']:<66} {r['seconds'] * 1e3:9.3f} ms")
    print(f"(frames {F}, N {N}, C {C}; LPC rows non-zero: {nz:.0%})")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
