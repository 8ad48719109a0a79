#!/usr/bin/env python3
"""encode_batch against one Encoder per clip, and frad_clips_frame_cut alone.

  1. --clips (256) one-second 48 kHz stereo s16le clips at N = 2048: profile 1 (16 bits, overlap ratio 2, host deflate) and
     profile 0 (32 bits), each through ``encode_batch`` and through a loop of one fresh ``Encoder`` per clip (process + flush)
     in the same process.  Both are warmed up, the timed repetitions alternate between the two, every timing is a host clock
     around work that ends with the stream bytes on the host, and the two sets of streams are compared first.  The median and
     the spread (min, max) of --reps repetitions are reported.  With --device-deflate also profile 1 with the deflate on the
     device.
  2. frad_clips_frame_cut over the whole frames of --cut-clips such clips (hop = N, and the hop of overlap ratio 2), HIP-event
     device time, against frad_bench_copy of as many bytes as the cut writes (the copy reads and writes that many; so does
     the cut, which reads the overlapped halves of a ratio-2 hop twice).

    python tools/encode_batch_probe.py [--clips 256] [--reps 7] [--cut-clips 2048] [--jsonl out.jsonl]

One JSON line per measurement."""
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
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cut-clips", type=int, default=2048)
    ap.add_argument("--device-deflate", action="store_true")
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import Encoder, _lib, core, encode_batch, synth
    from frad_python_amd.bridge import HipBridge
    if not torch.cuda.is_available():
        raise SystemExit("the probe needs the MI355X: no timing is taken without it")
    br, lib = HipBridge(), _lib.load()
    N, C, SRATE, n = 2048, 2, 48000, args.clips
    base = synth.harmonic_mix(SRATE + n, C, SRATE, seed=77)
    clips = [synth.to_pcm(np.ascontiguousarray(base[i:i + SRATE]) * (0.5 + 0.4 * (i % 7) / 7), "s16le").tobytes() for i in range(n)]
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def loop(profile, bits, ratio, dd):
        out = []
        for c in clips:
            e = Encoder(profile, SRATE, C, bits, N, "s16le", bridge=br, device_deflate=dd)
            e.set_overlap_ratio(ratio)
            out.append(e.process(c).buf + e.flush().buf)
        return out

    def batch(profile, bits, ratio, dd):
        return encode_batch(clips, profile, SRATE, C, bits, N, "s16le", overlap_ratio=ratio, device_deflate=dd, bridge=br).streams

    configs = [("profile 1, ratio 2", 1, 16, 2, False), ("profile 0, 32 bits", 0, 32, 0, False)]
    if args.device_deflate:
        configs.append(("profile 1, ratio 2, device deflate", 1, 16, 2, True))
    for name, *cfg in configs:
        a, b = loop(*cfg), batch(*cfg)                           # warm-up of every shape, and the contract
        same = a == b
        t_loop, t_batch = [], []
        for _ in range(args.reps):
            for fn, ts in ((loop, t_loop), (batch, t_batch)):    # alternating: the host is shared
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(*cfg)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        ml, mb = float(np.median(t_loop)), float(np.median(t_batch))
        emit({"what": f"encode, {n} one-second clips, {name}", "identical_streams": same, "reps": args.reps,
              "loop_ms": ml * 1e3, "loop_ms_min_max": [min(t_loop) * 1e3, max(t_loop) * 1e3],
              "encode_batch_ms": mb * 1e3, "encode_batch_ms_min_max": [min(t_batch) * 1e3, max(t_batch) * 1e3],
              "loop_over_encode_batch": ml / mb, "stream_bytes": sum(len(s) for s in b)})

    # ---- the cut alone
    stream = int(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts[1:]))

    m, step = args.cut_clips, 2 * C
    src = torch.randint(0, 256, (m * SRATE * step,), dtype=torch.uint8, device=br.device)
    for label, hop in (("hop = N", N), ("hop = N / 2 (overlap ratio 2)", N // 2)):
        k = (SRATE - N) // hop + 1
        rs = (np.arange(m, dtype=np.int64)[:, None] * SRATE + np.arange(k, dtype=np.int64)[None, :] * hop).reshape(-1)
        rv = np.full(rs.size, N, np.int32)
        table = torch.from_numpy(np.concatenate([rs.view(np.uint8), rv.view(np.uint8)])).to(br.device)
        out = torch.empty(rs.size * N * step, dtype=torch.uint8, device=br.device)
        check = core.clips_frame_cut(src, rs[:64], rv[:64], N, step).cpu().numpy()
        host = src[:int(rs[63] + N) * step].cpu().numpy()
        ok = all(np.array_equal(check[r], host[rs[r] * step:(rs[r] + N) * step]) for r in range(64))
        t_cut = timed(lambda: lib.clips_frame_cut(src.data_ptr(), table.data_ptr(), table.data_ptr() + 8 * rs.size, rs.size, N, step,
                                                  out.data_ptr(), stream))
        cp = torch.empty(out.numel(), dtype=torch.uint8, device=br.device)
        t_copy = timed(lambda: lib.bench_copy(out.data_ptr(), cp.data_ptr(), out.numel(), stream))
        emit({"what": f"frad_clips_frame_cut, {m} clips, {label}", "rows": int(rs.size), "bytes_written": out.numel(), "spot_checked": ok,
              "cut_ms": t_cut * 1e3, "cut_GB/s_read_plus_written": 2 * out.numel() / t_cut / 1e9,
              "frad_bench_copy_same_bytes_ms": t_copy * 1e3, "copy_GB/s": 2 * out.numel() / t_copy / 1e9,
              "copy_time_over_cut_time": t_copy / t_cut})
        del out, cp, table
    if args.jsonl:
        with open(args.jsonl, "w") as f:
            f.write(json.dumps({"what": "run", "device": torch.cuda.get_device_name(0), "clips": n, "reps": args.reps}) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
