#!/usr/bin/env python3
"""DecoderPool against a loop of per-stream Decoders, and frad_clips_carry_add alone.

  1. --streams (256) live streams of 48 kHz stereo, N = 2048: profile 1 (16 bits, overlap ratio 2) and profile 0 (32 bits).
     --distinct (8) different recordings are encoded and used in turn.  Every stream is fed in chunks of about 100 ms of its
     bytes (its length / its seconds / 10: not frame-aligned) for --ticks (50) ticks:
       * ``DecoderPool.process`` once per tick;
       * a loop of ``Decoder.process`` over the same chunks, one Decoder per stream -- what the parent commit offers.
     Both end with the samples on the host.  A first pass over all ticks compares every result of the two routes and warms
     both up; then the passes alternate, a pass being all ticks of fresh decoders, timed by a host clock around work that ends
     with a device synchronisation.  Median and spread (min, max) of --reps passes, per tick.
  2. frad_clips_carry_add alone, HIP-event device time: --streams clips of 5 frames each (a 100 ms tick at N = 2048, ratio 2),
     every clip with a fragment in and a fragment out, to float64 and to s16le, beside frad_bench_copy of its output bytes; and
     the registers and scratch of the k_clips_carry instantiations from the code-object metadata.

    python tools/decoder_pool_probe.py [--streams 256] [--ticks 50] [--reps 5] [--jsonl profiles/decoder_pool_probe.jsonl]

One JSON line per measurement."""
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
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from frad_python_amd import Decoder, DecoderPool, _lib, core, encode_batch, synth
    from frad_python_amd.bridge import HipBridge
    if not torch.cuda.is_available():
        raise SystemExit("the probe needs the MI355X: no timing is taken without it")
    br, lib = HipBridge(), _lib.load()
    N, C, SRATE, n, T = 2048, 2, 48000, args.streams, args.ticks
    seconds = T / 10 + 0.5                                       # half a second more than the ticks consume
    rows_in = int(seconds * SRATE)
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

    for name, profile, bits, ratio in (("profile 1, ratio 2", 1, 16, 2), ("profile 0, 32 bits", 0, 32, 0)):
        made = encode_batch(clips, profile, SRATE, C, bits, N, "s16le", overlap_ratio=ratio, bridge=br).streams
        streams = [made[i % len(made)] for i in range(n)]
        step = [int(len(s) / seconds / 10) for s in streams]    # about 100 ms of the stream's bytes
        chunk = lambda i, t: streams[i][t * step[i]:(t + 1) * step[i]]

        def pooled(keep):
            pool = DecoderPool(bridge=br)
            hs = [pool.open() for _ in range(n)]
            fell = 0
            for t in range(T):
                res = pool.process({h: chunk(i, t) for i, h in enumerate(hs)})
                fell += len(res.fallback)
                if keep is not None:
                    keep.append([res[h] for h in hs])
            return fell

        def looped(keep):
            decs = [Decoder(bridge=br) for _ in range(n)]
            for t in range(T):
                out = [d.process(chunk(i, t)) for i, d in enumerate(decs)]
                if keep is not None:
                    keep.append(out)

        a, b = [], []
        fell = pooled(a)                                         # warm-up of every shape, and the contract
        looped(b)
        same = all(x.pcm.dtype == y.pcm.dtype and x.pcm.shape == y.pcm.shape and np.array_equal(x.pcm, y.pcm) and
                   (x.srate, x.frames, x.crit) == (y.srate, y.frames, y.crit) for ta, tb in zip(a, b) for x, y in zip(ta, tb))
        frames = sum(x.frames for ta in a for x in ta)
        samples = sum(len(x.pcm) for ta in a for x in ta)
        del a, b
        t_pool, t_loop = [], []
        for _ in range(args.reps):
            for fn, ts in ((pooled, t_pool), (looped, t_loop)):  # alternating: the host is shared
                ts.append(wall(lambda: fn(None))[0] / T)
        mp, ml = float(np.median(t_pool)), float(np.median(t_loop))
        emit({"what": f"{n} live streams, {T} ticks of about 100 ms, {name}", "identical": same, "reps": args.reps,
              "fallback_ticks": fell, "frames_decoded": frames, "sample_frames_out": samples, "chunk_bytes": step[0],
              "pool_ms_per_tick": mp * 1e3, "pool_ms_per_tick_min_max": [min(t_pool) * 1e3, max(t_pool) * 1e3],
              "decoder_loop_ms_per_tick": ml * 1e3, "decoder_loop_ms_per_tick_min_max": [min(t_loop) * 1e3, max(t_loop) * 1e3],
              "decoder_loop_over_pool": ml / mp})
        del streams, made

    # ---- the carry kernel alone
    stream = int(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts[1:]))

    ratio, cut, per = 2, N // 2, 5
    L = N - cut
    frames = torch.rand((n * per, N, C), dtype=torch.float64, device=br.device) - 0.5
    prev = torch.rand((n, L, C), dtype=torch.float64, device=br.device) - 0.5
    nxt = torch.empty((n, L, C), dtype=torch.float64, device=br.device)
    cf = np.arange(n + 1, dtype=np.int64) * per
    off = cf * cut
    ptrs = lambda t: t.data_ptr() + np.arange(n, dtype=np.uint64) * np.uint64(8 * L * C)
    table = torch.from_numpy(np.concatenate([x.view(np.uint8) for x in (cf, off, ptrs(prev), ptrs(nxt))])).to(br.device)
    p = table.data_ptr()
    p_cf, p_off, p_prev, p_next = p, p + 8 * (n + 1), p + 16 * (n + 1), p + 16 * (n + 1) + 8 * n
    total = int(off[-1])
    for fmt in ("f64le", "s16le"):
        size = C * (8 if fmt == "f64le" else 2)
        out = torch.empty(total * size + 16, dtype=torch.uint8, device=br.device)
        go = lambda: lib.clips_carry_add(frames.data_ptr(), p_cf, n, N, C, ratio, p_prev, p_next, core.pcm_dtype_code(fmt), 2, out.data_ptr(),
                                         p_off, total, stream)
        go()
        want, tail = core.p1_overlap_add(frames[:per], ratio, prev[0], out_format=None if fmt == "f64le" else fmt)
        ok = bool(torch.equal(out[:per * cut * size], want.reshape(-1).view(torch.uint8)[:per * cut * size]) and torch.equal(nxt[0], tail))
        t = timed(go)
        read = frames.numel() * 8 + prev.numel() * 8
        written = total * size + nxt.numel() * 8
        emit({"what": f"frad_clips_carry_add, {n} clips of {per} frames, {fmt}", "spot_checked": ok, "bytes_read": read, "bytes_written": written,
              "ms": t * 1e3, "GB/s_read_plus_written": (read + written) / t / 1e9})
        cp = torch.empty(total * size, dtype=torch.uint8, device=br.device)
        t_copy = timed(lambda: lib.bench_copy(out.data_ptr(), cp.data_ptr(), total * size, stream))
        emit({"what": f"frad_bench_copy of the {fmt} output's bytes", "ms": t_copy * 1e3, "GB/s": 2 * total * size / t_copy / 1e9})
        del out, cp
    import resources
    regs = [{k: r.get(k) for k in ("demangled", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
                                    "sgpr_spill_count")}
            for r in resources.kernels(_lib.LIB_PATH) if "k_clips_carry" in r["demangled"]]
    emit({"what": "k_clips_carry instantiations (code-object metadata)", "kernels": regs})
    if args.jsonl:
        with open(args.jsonl, "w") as f:
            f.write(json.dumps({"what": "run", "device": torch.cuda.get_device_name(0), "streams": n, "ticks": T, "distinct": args.distinct,
                                "reps": args.reps}) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
