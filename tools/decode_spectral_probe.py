#!/usr/bin/env python3
"""Log-mel and power spectrograms of decoded windows on the device against torch on the batch the parent
commit leaves on the device, and frad_clips_spectrum alone.

  1. --streams (256) streams of --seconds (20) s at 44.1 kHz, profile 1 (16 bits, N = 2048, overlap ratio 2), half of them mono
     and half stereo, as in section 4l's run.  One random window of --window (1) s per stream at 16 kHz mono, drawn anew for
     every repetition and the same for both routes; two specs: n_fft = 512, hop = 160, 80 mels, log10 (float32), and n_fft =
     2048, hop = 512, 80 mels, log10:
       * ``StreamIndex.decode(wins, srate=16000, channels=1, pad_to=T, features=spec, as_tensor=True)``: one frad_clips_spectrum
         behind the mix writes [B, F, 1, 80] on the device;
       * what the parent commit offers: ``StreamIndex.decode(wins, srate=16000, channels=1, pad_to=T, as_tensor=True)`` and then,
         in torch on the device in float64, ``torch.stft(center=False, window=...)``, ``abs() ** 2``, ``matmul`` with the dense
         filterbank, ``clamp``, ``log10``, and the conversion to float32.  If ``torch.stft`` does not run on the box the row says
         so and the model on the host (``spectral.clips_spectrum_host``) takes its place.
     The results are compared first, to the tolerance of tests/test_clips_spectrum.py (floor = 2^20 * the largest linear bound).
     Both routes are warmed up, the repetitions alternate, every timing is a host clock around work that ends with the result
     on the device, synchronised.  Median and spread (min, max) of --reps.
  2. frad_clips_spectrum alone, HIP-event device time around the C-ABI call, tables already on the device: the same [B, T, 1]
     batch, both specs, with frad_bench_copy of the input's bytes in the same process.
  3. The kernels' registers and scratch from the code-object metadata (tools/resources.py).

    python tools/decode_spectral_probe.py [--streams 256] [--seconds 20] [--reps 5] [--jsonl profiles/decode_spectral_probe.jsonl]

One JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import math
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
    from frad_python_amd.spectral import Spectral, clips_spectrum_host
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
    stream = int(torch.cuda.current_stream().cuda_stream)
    U = 2.0 ** -53

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])

    for n_fft, hop in ((512, 160), (2048, 512)):
        lin = Spectral(n_fft, hop, n_mels=80, dtype="f64").tables(R)
        bank = lin.dense_bank()
        # the test's floor: 2^20 * the largest linear bound, for samples in [-1, 1): E_f <= sum(w^2)
        floor = 2.0 ** 20 * 32 * U * math.log2(n_fft) * n_fft * float((lin.window ** 2).sum()) * float(np.abs(bank).sum(1).max())
        spec = Spectral(n_fft, hop, n_mels=80, log="log10", floor=floor, dtype="f32")
        tb = spec.tables(R)
        F = spec.frames(W)
        win_t = torch.from_numpy(tb.window.copy()).to(br.device)
        bank_t = torch.from_numpy(bank.T.copy()).to(br.device)

        def device(wins):
            return idx.decode(wins, srate=R, channels=1, pad_to=W, features=spec, as_tensor=True).feature_batch

        stft_runs = True

        def with_torch(wins):
            batch = idx.decode(wins, srate=R, channels=1, pad_to=W, as_tensor=True).batch            # [B, T, 1] float64
            z = torch.stft(batch[:, :, 0], n_fft, hop_length=hop, window=win_t, center=False, return_complex=True)   # [B, bins, F]
            p = (z.abs() ** 2).transpose(1, 2) @ bank_t                                               # [B, F, 80]
            return torch.log10(p.clamp(min=floor)).to(torch.float32).reshape(len(wins), F, 1, 80)

        def with_host(wins):
            batch = idx.decode(wins, srate=R, channels=1, pad_to=W).batch
            return torch.from_numpy(np.stack([clips_spectrum_host(x, tb) for x in batch])).to(br.device)

        wins = draw()
        a = device(wins)
        try:
            b = with_torch(wins)
            other, name = with_torch, "torch.stft, abs()**2, matmul, clamp, log10 in float64 on the device"
        except RuntimeError as e:
            stft_runs = False
            b = with_host(wins)
            other, name = with_host, f"torch.stft does not run here ({str(e).splitlines()[0][:80]}): the numpy model on the host"
        err = (a.double() - b.double()).abs()
        tol = (1.0 / math.log(10.0)) * 2.0 ** -19 + 2.0 ** -23 * b.double().abs()
        agree = bool(a.shape == b.shape and (err <= tol).all().item())
        t_dev, t_other = [], []
        for _ in range(args.reps):
            wins = draw()
            for fn, ts in ((device, t_dev), (other, t_other)):   # alternating: the host is shared
                ts.append(wall(lambda: fn(wins))[0])
        md, mo = float(np.median(t_dev)), float(np.median(t_other))
        emit({"what": f"{n} one-{args.window:g}-s windows at {R} Hz mono -> [{n}, {F}, 1, 80] float32 log10-mel, n_fft={n_fft}, hop={hop}",
              "reps": args.reps, "yardstick": name, "torch_stft_runs": stft_runs, "results_agree_within_tolerance": agree,
              "worst_error_over_tolerance": float((err / tol).max().item()), "floor": floor,
              "decode_features_ms": md * 1e3, "decode_features_ms_min_max": [min(t_dev) * 1e3, max(t_dev) * 1e3],
              "decode_then_yardstick_ms": mo * 1e3, "decode_then_yardstick_ms_min_max": [min(t_other) * 1e3, max(t_other) * 1e3],
              "yardstick_over_decode_features": mo / md})
        # ---- the spectral stage alone: the same batch on the device, the kernel against the torch recipe, then the raw entry point
        batch = idx.decode(wins, srate=R, channels=1, pad_to=W, as_tensor=True).batch
        srcs = [batch[k] for k in range(n)]
        off = np.arange(n + 1, dtype=np.int64) * F
        valid = np.full(n, W, np.int32)
        br.clips_spectrum(srcs, valid, tb, 1, off)               # (tables uploaded)
        t_stage = [wall(lambda: br.clips_spectrum(srcs, valid, tb, 1, off))[0] for _ in range(args.reps)]
        row = {"what": f"the spectral stage alone on the [{n}, {W}, 1] batch, n_fft={n_fft}, hop={hop}: HipBridge.clips_spectrum (host clock)",
               "ms": float(np.median(t_stage)) * 1e3, "ms_min_max": [min(t_stage) * 1e3, max(t_stage) * 1e3]}
        if stft_runs:
            def recipe():
                z = torch.stft(batch[:, :, 0], n_fft, hop_length=hop, window=win_t, center=False, return_complex=True)
                return torch.log10(((z.abs() ** 2).transpose(1, 2) @ bank_t).clamp(min=floor)).to(torch.float32)
            recipe()
            t_rec = [wall(recipe)[0] for _ in range(args.reps)]
            row.update({"torch_recipe_ms": float(np.median(t_rec)) * 1e3, "torch_recipe_ms_min_max": [min(t_rec) * 1e3, max(t_rec) * 1e3]})
        emit(row)
        dt = core.spectrum_tables_upload(tb, br.device)
        tab = torch.from_numpy(np.concatenate([np.array([s.data_ptr() for s in srcs], np.int64).view(np.uint8), off.view(np.uint8),
                                               valid.view(np.uint8)])).to(br.device)
        p = tab.data_ptr()
        out = torch.empty((n * F, 1, 80), dtype=torch.float32, device=br.device)
        call = lambda: lib.clips_spectrum(p, p + 8 * n + 8 * (n + 1), n, 1, p + 8 * n, n * F, n_fft, hop, 0, dt["window"], 2, dt["n_bands"],
                                          dt["band_lo"], dt["band_len"], dt["band_off"], dt["band_w"], dt["n_weights"], tb.log_scale, tb.floor,
                                          tb.floor_log, core.pcm_dtype_code("f32le"), out.data_ptr(), stream)
        t, lo, hi = timed(call)
        same = bool(torch.equal(out.reshape(n, F, 1, 80), br.clips_spectrum(srcs, valid, tb, 1, off).reshape(n, F, 1, 80)))
        nbytes = batch.numel() * 8
        cp = torch.empty(nbytes, dtype=torch.uint8, device=br.device)
        t_copy, clo, chi = timed(lambda: lib.bench_copy(batch.data_ptr(), cp.data_ptr(), nbytes, stream))
        flops = n * F * (5 * (n_fft // 2) * math.log2(n_fft // 2) + 2 * float(tb.band_len.sum()) + 10 * n_fft)
        emit({"what": f"frad_clips_spectrum alone (HIP events), {n} windows of {W} rows, n_fft={n_fft}, hop={hop}, 80 mels, log10, f32",
              "equals_the_operator": same, "frames": n * F, "input_bytes": nbytes, "bytes_written": out.numel() * 4, "ms": t * 1e3,
              "ms_min_max": [lo * 1e3, hi * 1e3], "frames_per_s": n * F / t, "approx_f64_GFLOP/s": flops / t / 1e9,
              "input_rereads_n_fft_over_hop": n_fft / hop, "frad_bench_copy_of_the_input_ms": t_copy * 1e3,
              "frad_bench_copy_ms_min_max": [clo * 1e3, chi * 1e3], "frad_bench_copy_GB/s": 2 * nbytes / t_copy / 1e9})
        del out, cp, batch, srcs
    # ---- registers and scratch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resources
    for r in sorted(resources.kernels(), key=lambda r: r["demangled"]):
        if "k_clips_spectrum" in r["demangled"]:
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
