#!/usr/bin/env python3
"""EncoderPool against a loop of per-stream Encoders, and frad_clips_carry_cut alone.

  1. --streams (256) live inputs of 48 kHz stereo s16le, N = 2048, 100 ms (4800 sample-frames) per tick for --ticks (20) ticks:
     profile 0 (16 bits), and profile 1 at overlap ratio 2 without and with ``device_deflate``.  --distinct (8) different
     recordings are used in turn.
       * ``EncoderPool.process`` once per tick;
       * a loop of ``Encoder.process`` over the same chunks, one Encoder per stream -- what the parent commit offers.
     Both end with the frames' bytes on the host.  A first pass over all ticks compares every result of the two routes and
     warms both up; then the passes alternate, a pass being all ticks of fresh encoders, timed by a host clock around work
     that ends with a device synchronisation.  Median and spread (min, max) of --reps passes, per tick.
  2. frad_clips_carry_cut alone, HIP-event device time: --streams clips, each a carry of 1024 sample-frames and a chunk of 4800
     (the tick above at ratio 2: four rows of 2048 and a remainder of 1728), beside frad_bench_copy of the bytes it writes; and
     the kernel's registers and scratch from the code-object metadata.

    python tools/encoder_pool_probe.py [--streams 256] [--ticks 20] [--reps 5] [--cases 0,1,2] [--jsonl profiles/encoder_pool_probe.jsonl]

One JSON line per measurement, written as it is taken; a line on stderr per timed pass (the ``device_deflate`` loop takes about
15 ms per ``Encoder.process`` call, minutes per pass at the default size: --cases 2 --ticks 5 --reps 3 keeps it short)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="0,1,2", help="which of the three pool cases to run")
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import Encoder, EncoderPool, _lib, synth
    from frad_python_amd.bridge import HipBridge
    if not torch.cuda.is_available():
        raise SystemExit("the probe needs the MI355X: no timing is taken without it")
    br, lib = HipBridge(), _lib.load()
    N, C, SRATE, n, T = 2048, 2, 48000, args.streams, args.ticks
    per_tick, step = SRATE // 10, 2 * C                          # 100 ms of s16le stereo
    rows_in = T * per_tick
    base = synth.harmonic_mix(rows_in + 1000 * args.distinct, C, SRATE, seed=83)
    clips = [synth.to_pcm(np.ascontiguousarray(base[1000 * i:1000 * i + rows_in]) * (0.5 + 0.05 * i), "s16le").tobytes()
             for i in range(args.distinct)]
    chunk = lambda i, t: clips[i % len(clips)][t * per_tick * step:(t + 1) * per_tick * step]
    cases = sorted({int(x) for x in args.cases.split(",") if x != ""})
    log = open(args.jsonl, "w") if args.jsonl else None

    def emit(row):
        print(json.dumps(row), flush=True)
        if log is not None:
            log.write(json.dumps(row) + "\n")
            log.flush()

    if log is not None:
        log.write(json.dumps({"what": "run", "device": torch.cuda.get_device_name(0), "streams": n, "ticks": T, "distinct": args.distinct,
                              "reps": args.reps, "cases": cases}) + "\n")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for case, (name, profile, ratio, deflate) in enumerate((("profile 0, 16 bits", 0, 0, False), ("profile 1, ratio 2", 1, 2, False),
                                                            ("profile 1, ratio 2, device_deflate", 1, 2, True))):
        if case not in cases:
            continue
        def pooled(keep):
            pool = EncoderPool(profile, SRATE, C, 16, N, "s16le", overlap_ratio=ratio, device_deflate=deflate, bridge=br)
            hs = [pool.open() for _ in range(n)]
            fell = 0
            for t in range(T):
                res = pool.process({h: chunk(i, t) for i, h in enumerate(hs)})
                fell += len(res.fallback)
                if keep is not None:
                    keep.append([res[h] for h in hs])
            return fell, pool.carry_uploads + pool.carry_downloads

        def looped(keep):
            encs = []
            for _ in range(n):
                e = Encoder(profile, SRATE, C, 16, N, "s16le", bridge=br, device_deflate=deflate)
                e.set_overlap_ratio(ratio)
                encs.append(e)
            for t in range(T):
                out = [e.process(chunk(i, t)) for i, e in enumerate(encs)]
                if keep is not None:
                    keep.append(out)

        a, b = [], []
        fell, copies = pooled(a)                                 # warm-up of every shape, and the contract
        looped(b)
        same = all(x.buf == y.buf and x.samples == y.samples for ta, tb in zip(a, b) for x, y in zip(ta, tb))
        nbytes = sum(len(x.buf) for ta in a for x in ta)
        samples = sum(x.samples for ta in a for x in ta)
        del a, b
        t_pool, t_loop = [], []
        for _ in range(args.reps):
            for fn, ts in ((pooled, t_pool), (looped, t_loop)):  # alternating: the host is shared
                ts.append(wall(lambda: fn(None))[0] / T)
                print(f"[pass] {name}: {fn.__name__} {ts[-1] * 1e3:.2f} ms per tick", file=sys.stderr, flush=True)
        mp, ml = float(np.median(t_pool)), float(np.median(t_loop))
        emit({"what": f"{n} live streams, {T} ticks of 100 ms, {name}", "identical": same, "reps": args.reps, "fallback_ticks": fell,
              "carry_copies": copies, "stream_bytes_out": nbytes, "sample_frames_in": samples, "chunk_bytes": per_tick * step,
              "pool_ms_per_tick": mp * 1e3, "pool_ms_per_tick_min_max": [min(t_pool) * 1e3, max(t_pool) * 1e3],
              "encoder_loop_ms_per_tick": ml * 1e3, "encoder_loop_ms_per_tick_min_max": [min(t_loop) * 1e3, max(t_loop) * 1e3],
              "encoder_loop_over_pool": ml / mp})

    # ---- the cut kernel alone
    stream = int(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts[1:]))

    hop, held, k = N // 2, N // 2, 4
    left = held + per_tick - k * hop
    carry = torch.randint(1, 256, (n, held * step), dtype=torch.uint8, device=br.device)
    src = torch.randint(1, 256, (n * per_tick * step,), dtype=torch.uint8, device=br.device)
    nxt = torch.empty((n, left * step), dtype=torch.uint8, device=br.device)
    out = torch.empty((n * k, N * step), dtype=torch.uint8, device=br.device)
    ptrs = lambda t: t.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(t.shape[1])
    parts = [ptrs(carry), np.arange(n + 1, dtype=np.int64) * per_tick, np.tile(np.arange(k, dtype=np.int64) * hop, n),
             np.full(n, k * hop, np.int64), ptrs(nxt), np.full(n, held, np.int32), np.repeat(np.arange(n, dtype=np.int32), k)]
    table = torch.from_numpy(np.concatenate([x.view(np.uint8) for x in parts])).to(br.device)
    p = [table.data_ptr() + int(o) for o in np.cumsum([0] + [x.nbytes for x in parts])[:-1]]
    go = lambda: lib.clips_carry_cut(p[0], p[5], src.data_ptr(), p[1], n, p[6], p[2], n * k, N, step, out.data_ptr(), p[3], p[4], stream)
    go()
    whole = torch.cat([carry[0], src[:per_tick * step]])
    ok = bool(all(torch.equal(out[i], whole[i * hop * step:(i * hop + N) * step]) for i in range(k)) and torch.equal(nxt[0], whole[k * hop * step:]))
    t = timed(go)
    written = out.numel() + nxt.numel()
    emit({"what": f"frad_clips_carry_cut, {n} clips: a carry of {held}, a chunk of {per_tick}, {k} rows of {N} and a remainder of {left} sample-frames",
          "spot_checked": ok, "bytes_written": written, "ms": t * 1e3, "GB/s_read_plus_written": 2 * written / t / 1e9})
    cp = torch.empty(written, dtype=torch.uint8, device=br.device)
    t_copy = timed(lambda: lib.bench_copy(out.data_ptr(), cp[:out.numel()].data_ptr(), out.numel(), stream))
    emit({"what": "frad_bench_copy of the rows' bytes", "bytes": out.numel(), "ms": t_copy * 1e3, "GB/s": 2 * out.numel() / t_copy / 1e9})
    import resources
    regs = [{key: r.get(key) for key in ("demangled", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
                                         "vgpr_spill_count", "sgpr_spill_count")}
            for r in resources.kernels(_lib.LIB_PATH) if "k_clips_carry_cut" in r["demangled"]]
    emit({"what": "k_clips_carry_cut (code-object metadata)", "kernels": regs})
    if log is not None:
        log.close()


if __name__ == "__main__":
    main()
