#!/usr/bin/env python3
"""Reed-Solomon kernels on a cfg-2-sized stream (14 062 frames, 2048 x 2 x float64 payloads = 32 KiB each, ~460 MB): device
time of frad_rs_encode and frad_rs_repair (hipEvents around the launch only, median of --reps), GB/s of (bytes read + bytes
written), and that traffic as a fraction of the copy yardstick frad_bench_copy measured in the same process.
Repair runs on a protected stream with 1 % and with 100 % of its frames damaged (one byte error in every block of a damaged
frame, so every block of such a frame takes the Berlekamp-Massey / Chien / Forney path).

    python tools/ecc_probe.py [--frames 14062] [--reps 5] [--json ecc_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

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
    from frad_python_amd import _lib, ecc
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

    # copy yardstick: the same number of bytes moved as the encode
    cp = torch.empty(2 * F * nb // 16 * 16, dtype=torch.uint8, device=dev)
    half = cp.numel() // 2 // 16 * 16
    t_copy = timed(lambda: lib.bench_copy(cp.data_ptr(), cp.data_ptr() + half, half, stream))
    copy_gbs = 2 * half / t_copy / 1e9
    rows = [{"what": "frad_bench_copy", "bytes": 2 * half, "seconds": t_copy, "GB/s": copy_gbs}]

    payload = torch.from_numpy(rng.integers(0, 256, F * nb, dtype=np.uint8)).to(dev)
    for dsize, cs in ((96, 24), (223, 32)):
        # encode
        in_off, blk_off, out_off = ecc.plan([nb] * F, dsize, cs, False)
        offs = torch.from_numpy(np.concatenate([in_off, blk_off, out_off])).to(dev)
        o = offs.data_ptr(); n1 = F + 1
        nout = int(out_off[-1])
        prot = torch.empty((nout + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        nblk = int(blk_off[-1])
        t = timed(lambda: lib.rs_encode(payload.data_ptr(), o, o + 8 * n1, o + 16 * n1, F, nblk, dsize, cs, prot.data_ptr(), stream))
        moved = F * nb + nout
        rows.append({"what": f"rs_encode ({dsize}, {cs})", "bytes": moved, "seconds": t, "GB/s": moved / t / 1e9,
                     "of_copy": moved / t / 1e9 / copy_gbs})
        # repair
        r_in, r_blk, r_out = ecc.plan([nout // F] * F, dsize, cs, True)
        roffs = torch.from_numpy(np.concatenate([r_in, r_blk, r_out])).to(dev)
        ro = roffs.data_ptr()
        rblk = int(r_blk[-1])
        out = torch.empty(F * nb + 16, dtype=torch.uint8, device=dev)
        cnt = torch.empty(2 * F + rblk + 1, dtype=torch.int32, device=dev)
        bs, per = dsize + cs, nout // F
        for frac in (0.0, 0.01, 1.0):
            bad = prot.clone()
            if frac:
                frames = rng.choice(F, max(1, int(round(frac * F))), replace=False)
                host = bad[:nout].cpu().numpy()
                for f in frames:                                          # one byte error in every block of the frame
                    starts = f * per + np.arange(0, per, bs)
                    pos = starts + rng.integers(0, np.minimum(bs, per - (starts - f * per)))
                    host[pos] ^= rng.integers(1, 256, pos.size).astype(np.uint8)
                bad[:nout] = torch.from_numpy(host).to(dev)
            t = timed(lambda: lib.rs_repair(bad.data_ptr(), ro, ro + 8 * n1, ro + 16 * n1, F, rblk, dsize, cs, out.data_ptr(),
                                            cnt.data_ptr(), cnt.data_ptr() + 4 * F, cnt.data_ptr() + 8 * F, stream))
            c = cnt[:2 * F].cpu().numpy()
            assert torch.equal(out[:F * nb], payload), "repair did not restore the payload"
            moved = nout + F * nb
            rows.append({"what": f"rs_repair ({dsize}, {cs}) {frac:.0%} frames damaged", "bytes": moved, "seconds": t,
                         "GB/s": moved / t / 1e9, "of_copy": moved / t / 1e9 / copy_gbs,
                         "corrected_blocks": int(c[:F].sum()), "failed_blocks": int(c[F:].sum())})
            del bad
    for r in rows:
        extra = f"  {r['of_copy']:.3f} of copy" if "of_copy" in r else ""
        cb = f"  corrected {r['corrected_blocks']} failed {r['failed_blocks']}" if "corrected_blocks" in r else ""
        print(f"{r['what']:<44} {r['bytes'] / 1e6:9.1f} MB  {r['seconds'] * 1e3:9.3f} ms  {r['GB/s']:8.1f} GB/s{extra}{cb}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
