#!/usr/bin/env python3
"""Sample windows against decode_batch plus a slice on the host, and frad_clips_window_add alone.

  1. --streams (256) streams of --seconds (60) s, 48 kHz stereo, N = 2048: profile 1 (16 bits, overlap ratio 2) and profile 0 (32
     bits).  --distinct (8) different recordings are encoded and used in turn, so that the host holds 8 streams and not 256.  One
     random window of --window (1) s per stream, drawn anew for every repetition and the same for both routes:
       * ``StreamIndex.decode`` on an index built once (its build time is reported on its own);
       * ``decode_batch`` of all streams and ``pcm[i][start:start + length]`` on the host -- what the parent commit offers.
     Both are warmed up, the repetitions alternate, every timing is a host clock around work that ends with the samples on the
     host, and the two results are compared first.  Median and spread (min, max) of --reps repetitions.
  2. frad_clips_window_add alone, HIP-event device time: --streams windows of one second out of 49 decoded frames each (ratio 2),
     to float64 and to s16le, ragged and scattered into a dense batch through dst_row.

    python tools/decode_windows_probe.py [--streams 256] [--seconds 60] [--reps 5] [--jsonl profiles/decode_windows_probe.jsonl]

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
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import StreamIndex, _lib, core, decode_batch, encode_batch, synth
    from frad_python_amd.bridge import HipBridge
    if not torch.cuda.is_available():
        raise SystemExit("the probe needs the MI355X: no timing is taken without it")
    br, lib = HipBridge(), _lib.load()
    N, C, SRATE, n = 2048, 2, 48000, args.streams
    rows_in, W = int(args.seconds * SRATE), int(args.window * SRATE)
    base = synth.harmonic_mix(rows_in + 1000 * args.distinct, C, SRATE, seed=78)
    clips = [synth.to_pcm(np.ascontiguousarray(base[1000 * i:1000 * i + rows_in]) * (0.5 + 0.05 * i), "s16le").tobytes()
             for i in range(args.distinct)]
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    rng = np.random.default_rng(5)
    for name, profile, bits, ratio in (("profile 1, ratio 2", 1, 16, 2), ("profile 0, 32 bits", 0, 32, 0)):
        made = encode_batch(clips, profile, SRATE, C, bits, N, "s16le", overlap_ratio=ratio, bridge=br).streams
        streams = [made[i % len(made)] for i in range(n)]
        t_index = [wall(lambda: StreamIndex(streams, bridge=br))[0] for _ in range(3)]
        idx = StreamIndex(streams, bridge=br)
        draw = lambda: [(i, int(rng.integers(0, idx.samples[i] - W)), W) for i in range(n)]

        def windows(wins):
            return idx.decode(wins).pcm

        def whole(wins):
            pcm = decode_batch(streams, bridge=br).pcm
            return [pcm[i][a:a + w] for i, a, w in wins]

        wins = draw()
        a, b = windows(wins), whole(wins)                        # warm-up of every shape, and the contract
        same = all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
        del a, b
        t_win, t_whole = [], []
        for _ in range(args.reps):
            wins = draw()
            for fn, ts in ((windows, t_win), (whole, t_whole)):  # alternating: the host is shared
                ts.append(wall(lambda: fn(wins))[0])
        mw, mb = float(np.median(t_win)), float(np.median(t_whole))
        emit({"what": f"{n} streams of {args.seconds:g} s, one {args.window:g}-s window each, {name}", "identical": same, "reps": args.reps,
              "frames_per_stream": idx.frames[0], "stream_bytes": sum(len(s) for s in streams),
              "index_build_ms": float(np.median(t_index)) * 1e3, "index_build_ms_min_max": [min(t_index) * 1e3, max(t_index) * 1e3],
              "index_decode_ms": mw * 1e3, "index_decode_ms_min_max": [min(t_win) * 1e3, max(t_win) * 1e3],
              "decode_batch_plus_slice_ms": mb * 1e3, "decode_batch_plus_slice_ms_min_max": [min(t_whole) * 1e3, max(t_whole) * 1e3],
              "decode_batch_plus_slice_over_index_decode": mb / mw})
        del streams, made, idx

    # ---- the window kernel alone
    stream = int(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts[1:]))

    ratio, cut, per = 2, N // 2, 49                              # 49 frames of hop 1024 hold any window of 48 000 rows
    frames = torch.rand((n * per, N, C), dtype=torch.float64, device=br.device) - 0.5
    f0 = np.arange(n, dtype=np.int64) * per
    skip = rng.integers(cut, 2 * cut, n).astype(np.int64)
    m, valid = np.full(n, per, np.int32), np.full(n, W, np.int32)
    zeros64, zeros32 = np.zeros(n, np.int64), np.zeros(n, np.int32)
    off = np.arange(n + 1, dtype=np.int64) * W
    dst = rng.permutation(n).astype(np.int64) * W
    wide = [f0, zeros64, skip, dst, off]
    table = torch.from_numpy(np.concatenate([x.view(np.uint8) for x in wide + [m, zeros32, valid]])).to(br.device)
    p = [table.data_ptr() + 8 * n * i for i in range(5)] + [table.data_ptr() + 8 * (5 * n + 1) + 4 * n * i for i in range(3)]
    for fmt in ("f64le", "s16le"):
        check, _ = core.clips_window_add(frames, f0[:4], m[:4], N, C, ratio, skip=skip[:4], valid=valid[:4], out_format=None if fmt == "f64le" else fmt)
        whole, _ = core.clips_overlap_add(frames[:4 * per], np.arange(5) * per, N, C, ratio, out_format=None if fmt == "f64le" else fmt)
        rows_whole = per * cut + N - cut
        size = C * (8 if fmt == "f64le" else 2)
        ok = all(torch.equal(check.reshape(-1).view(torch.uint8)[j * W * size:(j + 1) * W * size],
                             whole.reshape(-1).view(torch.uint8)[(j * rows_whole + int(skip[j])) * size:(j * rows_whole + int(skip[j]) + W) * size])
                 for j in range(4))
        out = torch.empty(n * W * size, dtype=torch.uint8, device=br.device)
        for label, d in (("ragged", 0), ("scattered through dst_row", p[3])):
            t = timed(lambda: lib.clips_window_add(frames.data_ptr(), p[0], p[5], n, N, C, ratio, 0, p[1], p[6], 0, p[2], p[7], d,
                                                   core.pcm_dtype_code(fmt), 2, out.data_ptr(), p[4], n * W, stream))
            emit({"what": f"frad_clips_window_add, {n} windows of {W} rows, {fmt}, {label}", "spot_checked": ok, "bytes_written": out.numel(),
                  "bytes_read": n * W * C * 8 * 2, "ms": t * 1e3, "GB/s_read_plus_written": (out.numel() + n * W * C * 16) / t / 1e9})
        cp = torch.empty(out.numel(), dtype=torch.uint8, device=br.device)
        t_copy = timed(lambda: lib.bench_copy(out.data_ptr(), cp.data_ptr(), out.numel(), stream))
        emit({"what": f"frad_bench_copy of the {fmt} output's bytes", "ms": t_copy * 1e3, "GB/s": 2 * out.numel() / t_copy / 1e9})
        del out, cp
    if args.jsonl:
        with open(args.jsonl, "w") as f:
            f.write(json.dumps({"what": "run", "device": torch.cuda.get_device_name(0), "streams": n, "seconds": args.seconds,
                                "distinct": args.distinct, "reps": args.reps}) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
