#!/usr/bin/env python3
"""Windows at one sample rate against decoding at the streams' rate and resampling on the host.

  1. --streams (256) streams of --seconds (20) s, 44.1 kHz stereo, profile 1 (16 bits, N = 2048, overlap ratio 2).  --distinct (8)
     different recordings are encoded and used in turn.  One random window of --window (1) s per stream, as a dense batch
     (``pad_to``) at 16 kHz, drawn anew for every repetition and the same for both routes:
       * ``StreamIndex.decode(wins, srate=16000, pad_to=T)``: frad_clips_resample writes the batch on the device;
       * what the parent commit offers: ``StreamIndex.decode`` of the source rows those windows read (float64), the download,
         ``scipy.signal.resample_poly`` per window on the host and the copy into the batch.  (The host route resamples the
         rows the window reads, from a multiple of `down` on, with zeros beyond them: its rows away from the window's edges
         are compared.)
     Both are warmed up, the repetitions alternate, every timing is a host clock around work that ends with the batch on the
     host.  Median and spread (min, max) of --reps repetitions.
  2. frad_clips_resample alone, HIP-event device time: the same --streams windows from float64 rows already on the device, to
     float64 and to s16le.

    python tools/decode_resample_probe.py [--streams 256] [--seconds 20] [--reps 5] [--jsonl profiles/decode_resample_probe.jsonl]

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
    from scipy.signal import resample_poly
    from frad_python_amd import StreamIndex, encode_batch, synth
    from frad_python_amd.bridge import HipBridge
    from frad_python_amd.window import resample_needs, resample_ratio
    if not torch.cuda.is_available():
        raise SystemExit("the probe needs the MI355X: no timing is taken without it")
    br = HipBridge()
    N, C, SRATE, R, n = 2048, 2, 44100, 16000, args.streams
    up, down, half = resample_ratio(R, SRATE)
    rows_in, W = int(args.seconds * SRATE), int(args.window * R)
    base = synth.harmonic_mix(rows_in + 1000 * args.distinct, C, SRATE, seed=79)
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

    made = encode_batch(clips, 1, SRATE, C, 16, N, "s16le", overlap_ratio=2, bridge=br).streams
    streams = [made[i % len(made)] for i in range(n)]
    idx = StreamIndex(streams, bridge=br)
    total = idx.samples_at(R)
    rng = np.random.default_rng(6)
    draw = lambda: [(i, int(rng.integers(0, total[i] - W)), W) for i in range(n)]

    def device(wins):
        return idx.decode(wins, srate=R, pad_to=W).batch

    def host(wins):
        need = [resample_needs(a, a + w, up, down, idx.samples[i]) for i, a, w in wins]
        need = [(lo // down * down, hi) for lo, hi in need]      # from a multiple of `down` on: the span's output rows are the stream's
        src = idx.decode([(i, lo, hi - lo) for (i, _, _), (lo, hi) in zip(wins, need)]).pcm
        batch = np.zeros((len(wins), W, C))
        for k, ((i, a, w), (lo, hi)) in enumerate(zip(wins, need)):
            y = resample_poly(src[k], up, down, axis=0)          # the span from its own row 0: stream row a is its row a - first
            first = lo // down * up
            batch[k] = y[a - first:a - first + w]
        return batch

    wins = draw()
    a, b = device(wins), host(wins)                              # warm-up of every shape, and a comparison away from the edges
    edge = 2 * half // down + 2
    err = float(np.max(np.abs(a[:, edge:-edge] - b[:, edge:-edge])))
    t_dev, t_host = [], []
    for _ in range(args.reps):
        wins = draw()
        for fn, ts in ((device, t_dev), (host, t_host)):         # alternating: the host is shared
            ts.append(wall(lambda: fn(wins))[0])
    md, mh = float(np.median(t_dev)), float(np.median(t_host))
    emit({"what": f"{n} streams of {args.seconds:g} s at {SRATE} Hz, one {args.window:g}-s window each at {R} Hz, profile 1, ratio 2, pad_to",
          "reps": args.reps, "max_abs_difference_away_from_the_edges": err, "frames_per_stream": idx.frames[0],
          "decode_srate_ms": md * 1e3, "decode_srate_ms_min_max": [min(t_dev) * 1e3, max(t_dev) * 1e3],
          "decode_download_scipy_ms": mh * 1e3, "decode_download_scipy_ms_min_max": [min(t_host) * 1e3, max(t_host) * 1e3],
          "decode_download_scipy_over_decode_srate": mh / md})

    # ---- the kernel alone
    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.median(ts[1:]))

    starts = rng.integers(1000, 2000, n)
    need = [resample_needs(int(a), int(a) + W, up, down, 10 ** 9) for a in starts]
    per = max(hi - lo for lo, hi in need)
    src = torch.rand(n * per * C, dtype=torch.float64, device=br.device) - 0.5
    tables = dict(src_off=np.arange(n, dtype=np.int64) * per * C, src_row0=[lo for lo, _ in need], src_rows=[hi - lo for lo, hi in need],
                  out_row0=starts, valid=np.full(n, W, np.int32))
    for fmt in (None, "s16le"):
        run = lambda: br.clips_resample(src, tables["src_off"], tables["src_row0"], tables["src_rows"], C, up, down, tables["out_row0"],
                                        tables["valid"], fmt, as_tensor=True)
        out, _ = run()
        t = timed(run)                                           # (includes the upload of the tables: one small copy)
        written = out.numel() * out.element_size()
        emit({"what": f"clips_resample {up}/{down}, {n} windows of {W} rows, {fmt or 'f64le'}", "source_rows_per_window": per,
              "bytes_read": n * per * C * 8, "bytes_written": written, "ms": t * 1e3,
              "Gsamples/s_out": n * W * C / t / 1e9})
    if args.jsonl:
        with open(args.jsonl, "w") as f:
            f.write(json.dumps({"what": "run", "device": torch.cuda.get_device_name(0), "streams": n, "seconds": args.seconds,
                                "distinct": args.distinct, "reps": args.reps}) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
