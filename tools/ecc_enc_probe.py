#!/usr/bin/env python3
"""Encoder-side Reed-Solomon on the device: HIP-event device times, median of --reps after a warm-up.

  1. frad_rs_encode_frames (fixed stride) against frad_rs_encode (ragged offsets) on the same 14 062 x 32 KiB batch, at
     (96, 24) and (223, 32), with GB/s of (bytes read + bytes written) and that as a fraction of frad_bench_copy;
  2. the lossless stream assembly of HipBridge.lossless_encode_stream on the device (payload kernel, checksums, headers),
     cfg 2 geometry (14 062 frames of 2048 x 2, s16le in, 32-bit storage), with and without ECC (96, 24);
  3. frad_crc16_ansi_frames on the deflated profile-1 bodies of the same PCM (ragged, what a compact ECC batch checksums).

    python tools/ecc_enc_probe.py [--frames 14062] [--reps 5] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14062)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import _lib, core, ecc, synth
    from frad_python_amd.bridge import HipBridge
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = int(torch.cuda.current_stream().cuda_stream)
    F, nb = args.frames, 2048 * 2 * 8
    rng = np.random.default_rng(1)

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts[1:]))

    cp = torch.empty(2 * F * nb // 16 * 16, dtype=torch.uint8, device=dev)
    half = cp.numel() // 2 // 16 * 16
    t_copy = timed(lambda: lib.bench_copy(cp.data_ptr(), cp.data_ptr() + half, half, stream))
    copy_gbs = 2 * half / t_copy / 1e9
    del cp
    rows = [{"what": "frad_bench_copy", "bytes": 2 * half, "ms": t_copy * 1e3, "GB/s": copy_gbs}]

    payload = torch.from_numpy(rng.integers(0, 256, (F, nb), dtype=np.uint8)).to(dev)
    for dsize, cs in ((96, 24), (223, 32)):
        in_off, blk_off, out_off = ecc.plan([nb] * F, dsize, cs, False)
        offs = torch.from_numpy(np.concatenate([in_off, blk_off, out_off])).to(dev)
        o, n1 = offs.data_ptr(), F + 1
        P = core.rs_protected_bytes(nb, dsize, cs)
        ragged = torch.empty(F * P + 16, dtype=torch.uint8, device=dev)
        fixed = torch.empty((F, P), dtype=torch.uint8, device=dev)
        nblk = int(blk_off[-1])
        t_r = timed(lambda: lib.rs_encode(payload.data_ptr(), o, o + 8 * n1, o + 16 * n1, F, nblk, dsize, cs, ragged.data_ptr(), stream))
        t_f = timed(lambda: core.rs_encode_frames(payload, nb, dsize, cs, out=fixed))
        same = bool(torch.equal(ragged[:F * P], fixed.reshape(-1)))
        moved = F * (nb + P)
        for what, t in (("frad_rs_encode", t_r), ("frad_rs_encode_frames", t_f)):
            rows.append({"what": f"{what} ({dsize}, {cs})", "bytes": moved, "ms": t * 1e3, "GB/s": moved / t / 1e9,
                         "of_copy": moved / t / 1e9 / copy_gbs, "identical": same})
        del ragged, fixed, offs

    # stream assembly on the device, cfg 2 geometry
    N, C, bits = 2048, 2, 32
    x = synth.to_pcm(synth.harmonic_mix(F * N, C, 48000, seed=7), "s16le")
    pcm = torch.from_numpy(x.reshape(-1).view(np.uint8)).to(dev)
    nbp = lib.payload_bytes(N, C, bits)
    head = torch.zeros(28, dtype=torch.uint8, device=dev)

    def assemble(ratio):
        P = nbp if ratio is None else core.rs_protected_bytes(nbp, *ratio)
        st = torch.empty((F, 32 + P), dtype=torch.uint8, device=dev)

        def run():
            pay = st[:, 32:]
            enc = core.analogue_batch(0, pcm, "s16le", F, N, C, bits, check_overflow=False, out=None if ratio else pay)
            if ratio is not None:
                core.rs_encode_frames(enc.payload, nbp, *ratio, out=pay)
            crc = core.crc32_frames(pay, P)
            st[:, :28] = head
            st[:, 28:32] = crc.view(torch.uint8).view(F, 4).flip(1)
        return run, P

    for ratio in (None, (96, 24)):
        run, P = assemble(ratio)
        t = timed(run)
        rows.append({"what": "lossless stream assembly" + ("" if ratio is None else f" + ECC {ratio}"), "frames": F,
                     "payload_bytes": nbp, "protected_bytes": P, "ms": t * 1e3})

    # CRC-16 of a profile-1 batch (deflated bodies, as the compact ECC path checksums them after protection)
    br = HipBridge()
    bodies = br.p1_encode_bodies(x.tobytes(), "s16le", F, N, C, 16, 48000, 0.5, N, N)
    frads = [zlib.compress(b, 6)[2:-4] for b in bodies]
    off = np.zeros(F + 1, np.int64)
    np.cumsum([len(b) for b in frads], out=off[1:])
    d = torch.from_numpy(np.frombuffer(b"".join(frads), np.uint8).copy()).to(dev)
    do = torch.from_numpy(off).to(dev)
    t = timed(lambda: lib.crc16_ansi_frames(d.data_ptr(), do.data_ptr(), F, torch.empty(F, dtype=torch.int16, device=dev).data_ptr(), stream))
    got = core.crc16_ansi_frames(d, do).cpu().numpy().view(np.uint16)
    from frad_python_amd.common import crc16_ansi
    check = all(int(got[i]) == crc16_ansi(frads[i]) for i in range(0, F, max(1, F // 64)))
    rows.append({"what": "frad_crc16_ansi_frames (profile-1 bodies)", "frames": F, "bytes": int(off[-1]), "ms": t * 1e3,
                 "GB/s": int(off[-1]) / t / 1e9, "spot_checked_against_host": check})

    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
