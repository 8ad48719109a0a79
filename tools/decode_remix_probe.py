#!/usr/bin/env python3
"""Windows of mono and stereo streams as one mono batch against mixing on the host, and frad_clips_remix
alone.

  1. --streams (256) streams of --seconds (20) s at 44.1 kHz, profile 1 (16 bits, N = 2048, overlap ratio 2), half of them mono
     and half stereo.  --distinct (8) different recordings are encoded and used in turn.  One random window of --window (1) s
     per stream as a dense float64 batch [streams, rows, 1] at 16 kHz, drawn anew for every repetition and the same for both
     routes:
       * ``StreamIndex.decode(wins, srate=16000, channels=1, pad_to=T)``: frad_clips_remix writes the batch on the device;
       * what the parent commit offers: ``StreamIndex.decode(wins, srate=16000)`` ragged, the download, numpy's mean over the
         channels on the host and the copy into the batch.
     The results are compared first (they must be identical).  Both routes are warmed up, the repetitions alternate, every
     timing is a host clock around work that ends with the batch on the host.  Median and spread (min, max) of --reps.
  2. frad_clips_remix alone, HIP-event device time, tables already on the device: --streams windows of 16 000 float64 rows,
     stereo -> mono and mono -> stereo, to float64 and to s16le, with frad_bench_copy of the output's bytes in the same process.
  3. The kernels' registers and scratch from the code-object metadata (tools/resources.py).

    python tools/decode_remix_probe.py [--streams 256] [--seconds 20] [--reps 5] [--jsonl profiles/decode_remix_probe.jsonl]

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
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import StreamIndex, core, encode_batch, synth
    from frad_python_amd._lib import load
    from frad_python_amd.bridge import HipBridge
    from frad_python_amd.window import clips_remix_host
    if not torch.cuda.is_available():
        raise SystemExit("the probe needs the MI355X: no timing is taken without it")
    br = HipBridge()
    lib = load()
    N, SRATE, R, n = 2048, 44100, 16000, args.streams
    rows_in, W = int(args.seconds * SRATE), int(args.window * R)
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

    made = {}
    per = max(1, args.distinct // 2)
    for C in (1, 2):
        base = synth.harmonic_mix(rows_in + 1000 * per, C, SRATE, seed=80 + C)
        clips = [synth.to_pcm(np.ascontiguousarray(base[1000 * i:1000 * i + rows_in]) * (0.5 + 0.05 * i), "s16le").tobytes() for i in range(per)]
        made[C] = encode_batch(clips, 1, SRATE, C, 16, N, "s16le", overlap_ratio=2, bridge=br).streams
    streams = [made[1 + i % 2][(i // 2) % per] for i in range(n)]     # mono, stereo, mono, ...
    idx = StreamIndex(streams, bridge=br)
    total = idx.samples_at(R)
    rng = np.random.default_rng(7)
    draw = lambda: [(i, int(rng.integers(0, total[i] - W)), W) for i in range(n)]

    def device(wins):
        return idx.decode(wins, srate=R, channels=1, pad_to=W).batch

    def host(wins):
        pcm = idx.decode(wins, srate=R).pcm
        batch = np.zeros((len(wins), W, 1))
        for k, x in enumerate(pcm):
            batch[k, :len(x), 0] = x.mean(axis=1)
        return batch

    wins = draw()
    a, b = device(wins), host(wins)                              # warm-up of every shape, and the comparison
    same = bool(a.shape == b.shape and np.array_equal(a, b))
    t_dev, t_host = [], []
    for _ in range(args.reps):
        wins = draw()
        for fn, ts in ((device, t_dev), (host, t_host)):         # alternating: the host is shared
            ts.append(wall(lambda: fn(wins))[0])
    md, mh = float(np.median(t_dev)), float(np.median(t_host))
    emit({"what": f"{n} streams of {args.seconds:g} s at {SRATE} Hz, half mono and half stereo, one {args.window:g}-s window each as [{n}, {W}, 1] "
                  f"float64 at {R} Hz, profile 1, ratio 2", "reps": args.reps, "results_identical": same, "frames_per_stream": idx.frames[0],
          "decode_channels_ms": md * 1e3, "decode_channels_ms_min_max": [min(t_dev) * 1e3, max(t_dev) * 1e3],
          "decode_download_mean_ms": mh * 1e3, "decode_download_mean_ms_min_max": [min(t_host) * 1e3, max(t_host) * 1e3],
          "decode_download_mean_over_decode_channels": mh / md})

    # ---- the kernel alone
    stream = int(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.median(ts[1:]))

    rows16 = 16000
    for c_in, c_out in ((2, 1), (1, 2)):
        src = torch.rand((n, rows16 + 1, c_in), dtype=torch.float64, device=br.device) - 0.5
        srcs = [src[j, j % 2:j % 2 + rows16] for j in range(n)]  # every other window starts at an odd row: 8 bytes off for one channel
        m = np.full((1, 2), 0.5) if c_out == 1 else np.ones((2, 1))
        ptr = np.array([s.data_ptr() for s in srcs], np.int64)
        off = np.arange(n + 1, dtype=np.int64) * rows16
        wide = [ptr, np.zeros(n, np.int64), off, m.reshape(-1)]
        narrow = [np.full(n, c_in, np.int32), np.full(n, rows16, np.int32)]
        table = torch.from_numpy(np.concatenate([x.view(np.uint8) for x in wide + narrow])).to(br.device)
        p, at = [], table.data_ptr()
        for x in wide + narrow:
            p.append(at)
            at += x.nbytes
        for fmt in ("f64le", "s16le"):
            check, _ = core.clips_remix(srcs[:3], {c_in: m}, c_out, out_format=None if fmt == "f64le" else fmt)
            want = np.concatenate([clips_remix_host(s.cpu().numpy(), m, None if fmt == "f64le" else fmt) for s in srcs[:3]])
            ok = check.cpu().numpy().tobytes() == want.tobytes()
            size = c_out * (8 if fmt == "f64le" else 2)
            out = torch.empty(n * rows16 * size, dtype=torch.uint8, device=br.device)
            t = timed(lambda: lib.clips_remix(p[0], p[4], p[3], p[1], n, c_out, p[5], 0, core.pcm_dtype_code(fmt), 2, out.data_ptr(), p[2],
                                              n * rows16, stream))
            got = out[:3 * rows16 * size].cpu().numpy().tobytes() == want.tobytes()
            read = n * rows16 * c_in * 8
            cp = torch.empty(out.numel(), dtype=torch.uint8, device=br.device)
            t_copy = timed(lambda: lib.bench_copy(out.data_ptr(), cp.data_ptr(), out.numel(), stream))
            emit({"what": f"frad_clips_remix {c_in} -> {c_out}, {n} windows of {rows16} rows, {fmt}", "spot_checked": bool(ok and got),
                  "bytes_read": read, "bytes_written": out.numel(), "ms": t * 1e3, "GB/s_read_plus_written": (read + out.numel()) / t / 1e9,
                  "frad_bench_copy_of_the_output_ms": t_copy * 1e3, "frad_bench_copy_GB/s": 2 * out.numel() / t_copy / 1e9})
            del out, cp
        del src, srcs
    # ---- registers and scratch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resources
    for r in sorted(resources.kernels(), key=lambda r: r["demangled"]):
        if "k_clips_remix" in r["demangled"]:
            emit({"what": "resources", "kernel": r["demangled"], "vgpr": int(r.get("vgpr_count", -1)), "sgpr": int(r.get("sgpr_count", -1)),
                  "scratch_bytes_per_lane": int(r.get("private_segment_fixed_size", -1)), "lds_bytes": int(r.get("group_segment_fixed_size", -1))})
    if args.jsonl:
        with open(args.jsonl, "w") as f:
            f.write(json.dumps({"what": "run", "device": torch.cuda.get_device_name(0), "streams": n, "seconds": args.seconds,
                                "distinct": args.distinct, "reps": args.reps}) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
