#!/usr/bin/env python3
"""Profile-2 encode on a cfg-2-sized batch (14 999 stereo frames of 2048 at 48 kHz, sparse noise that mostly takes the TNS
branch), one process.  Device time (hipEvents around the launches, median of --reps after one warm-up) of:
  * stage A, the float64 DCT plane (frad_p0_analogue at 64-bit little-endian storage);
  * frad_p2_analogue as a whole (stage A + k_p2_analysis), and k_p2_analysis by difference;
  * frad_p2_golomb_encode + frad_rows_compact;
  * profile 1's chain on the same PCM (frad_p1_analogue + frad_p1_golomb_encode);
and the host wall time of HipBridge.p2_encode_bodies against p1_encode_bodies (upload, the chain, one download), with the
HBM bytes each kernel must move at the least.

    python tools/p2_enc_probe.py [--frames 14999] [--reps 5] [--json p2_enc_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14999)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import _lib, core
    from frad_python_amd.bridge import HipBridge
    F, N, C, bits, sr, loss = args.frames, 2048, 2, 16, 48000, 0.5
    dev = torch.device("cuda:0")

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts[1:]))

    rng = np.random.default_rng(5)
    x = rng.normal(0, 3000, (F * N, C)) * (rng.random((F * N, 1)) < 0.01)
    raw = np.clip(x, -32767, 32767).astype("<i2").tobytes()
    pcm = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
    lib = _lib.load()
    plane = torch.empty((F, N, C), dtype=torch.float64, device=dev)
    code = 10                                                        # FRAD_PCM_S16LE

    def stage_a():
        lib.p0_analogue(pcm.data_ptr(), code, F, N, C, N, 64, 1 | _lib.FRAD_RAW_BE_INTS, plane.data_ptr(), N * C * 8, 0,
                        torch.cuda.current_stream().cuda_stream)

    out = {}
    out["stage_a_s"] = timed(stage_a)
    q, tq, lpc = core.p2_analogue_batch(pcm, "s16le", F, N, C, bits, sr, loss)
    out["p2_analogue_s"] = timed(lambda: core.p2_analogue_batch(pcm, "s16le", F, N, C, bits, sr, loss))
    out["k_p2_analysis_s"] = out["p2_analogue_s"] - out["stage_a_s"]
    out["p2_golomb_s"] = timed(lambda: core.p2_golomb_encode_batch(q, tq, lpc))
    out["p2_chain_s"] = timed(lambda: core.p2_golomb_encode_batch(*core.p2_analogue_batch(pcm, "s16le", F, N, C, bits, sr, loss)))
    q1, tq1 = core.p1_analogue_batch(pcm, "s16le", F, N, C, bits, sr, loss)
    out["p1_analogue_s"] = timed(lambda: core.p1_analogue_batch(pcm, "s16le", F, N, C, bits, sr, loss))
    out["p1_golomb_s"] = timed(lambda: core.p1_golomb_encode_batch(q1, tq1))
    out["p1_chain_s"] = timed(lambda: core.p1_golomb_encode_batch(*core.p1_analogue_batch(pcm, "s16le", F, N, C, bits, sr, loss)))
    out["tns_channel_fraction"] = float((lpc != 0).any(dim=1).float().mean())
    br = HipBridge()

    def wall(fn):
        ts = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts[1:]))
    out["p2_encode_bodies_wall_s"] = wall(lambda: br.p2_encode_bodies(raw, "s16le", F, N, C, bits, sr, loss, N, N))
    out["p1_encode_bodies_wall_s"] = wall(lambda: br.p1_encode_bodies(raw, "s16le", F, N, C, bits, sr, loss, N, N))
    # least HBM traffic: stage A reads the PCM and writes the plane; k_p2_analysis reads the plane (at least once) and writes
    # it back once (the masked spectrum), writes q / tq / lpc
    pcm_b, plane_b, q_b = F * N * C * 2, F * N * C * 8, F * (N + 27 + 13) * C * 4
    out["stage_a_GBps"] = (pcm_b + plane_b) / out["stage_a_s"] / 1e9
    out["k_p2_analysis_GBps_min_traffic"] = (2 * plane_b + q_b) / out["k_p2_analysis_s"] / 1e9
    out["frames"], out["N"], out["C"] = F, N, C
    for k, v in out.items():
        print(f"{k:34s} {v:.6g}" if isinstance(v, float) else f"{k:34s} {v}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
