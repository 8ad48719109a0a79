#!/usr/bin/env python3
"""Raw-DEFLATE deflate on the device: kernel time against the host's zlib pool, and the encoder end
to end.

  * frad_deflate_raw on the pre-deflate bodies of 14 999 profile-1 frames (N = 2048, stereo, 16 bit, ratio 16 -- a
    10-minute stream at 48 kHz) at loss levels 0.5 and 10: device time of the launch (events, median of --reps), and the
    encoder's host path over the same bodies (zlib on its thread pool of at most 16 workers, wall time, median of --reps);
    the kernel's rows are compared with zlib's bytes;
  * Encoder.process + flush of a 60 s and a 10 min profile-1 stream (default loss level, ratio 16): the default (host
    deflate) against device_deflate=True, alternating in one process, median of --reps, the streams compared byte for byte.
Prints one JSON line per measurement.  Needs the MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pcm_of(secs: float) -> bytes:
    from frad_python_amd import synth
    return synth.to_pcm(synth.harmonic_mix(int(secs * 48000), 2, 48000, seed=2024), "s16le").tobytes()


def encoder(device_deflate: bool, loss: float | None = None):
    from frad_python_amd.encoder import Encoder
    enc = Encoder(1, 48000, 2, 16, 2048, "s16le", device_deflate=device_deflate)
    enc.set_overlap_ratio(16)
    if loss is not None:
        enc.set_loss_level(loss)
    return enc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=14999)
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    import torch
    from frad_python_amd import core, encoder as encmod, frames
    from frad_python_amd._lib import load
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = load()
    N, C, hop = 2048, 2, 1920
    for loss in (0.5, 10.0):
        pcm = pcm_of((args.frames - 1) * hop / 48000 + N / 48000)
        q, tq = core.p1_analogue_batch(torch.frombuffer(bytearray(pcm), dtype=torch.uint8).cuda(), "s16le", args.frames, N, C, 16,
                                       48000, loss, frame_stride=hop, n_valid=N)
        flat, offs = core.p1_golomb_encode_batch(q, tq)
        off = offs.cpu().numpy()
        host = flat.cpu().numpy().tobytes()
        bodies = [host[off[i]:off[i + 1]] for i in range(args.frames)]
        host_ms = []
        for r in range(args.reps + 1):
            t0 = time.perf_counter()
            ref = frames.map_zlib(encmod.Encoder._deflate, bodies)
            if r:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        stride = lib.deflate_stride(int(np.diff(off).max()) + 4)
        dst = torch.empty(args.frames * stride, dtype=torch.uint8, device="cuda")
        nb = torch.empty(args.frames, dtype=torch.int64, device="cuda")
        st = torch.empty(args.frames, dtype=torch.int32, device="cuda")
        times = []
        for r in range(args.reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            lib.deflate_raw(flat.data_ptr(), offs.data_ptr(), args.frames, dst.data_ptr(), stride, nb.data_ptr(), st.data_ptr(),
                            core._stream_ptr())
            b.record()
            torch.cuda.synchronize()
            if r >= 2:
                times.append(a.elapsed_time(b))
        rows = dst.view(args.frames, stride).cpu().numpy()
        nbh, sth = nb.cpu().numpy(), st.cpu().numpy()
        same = bool((sth == 0).all()) and all(rows[i, :nbh[i]].tobytes() == ref[i] for i in range(args.frames))
        print(json.dumps({"what": "deflate_kernel", "loss_level": loss, "frames": args.frames, "dst_stride": stride,
                          "kernel_ms_median": round(float(np.median(times)), 3), "kernel_ms_min": round(min(times), 3),
                          "body_bytes": int(off[-1]), "deflated_bytes": int(sum(map(len, ref))),
                          "longest_body": int(np.diff(off).max()), "host_pool_ms_median": round(float(np.median(host_ms)), 2),
                          "host_pool_workers": frames._POOL._max_workers if frames._POOL else 1, "bytes_equal_zlib": same}),
              flush=True)
        assert same
    if args.skip_e2e:
        return
    for secs in (60, 600):
        pcm = pcm_of(secs)
        res = {}
        for r in range(args.reps + 1):
            for mode in (False, True):
                enc = encoder(mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = enc.process(pcm).buf + enc.flush().buf
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    res.setdefault(mode, []).append(dt)
                else:
                    res[("out", mode)] = out
        assert res[("out", False)] == res[("out", True)]
        print(json.dumps({"what": "encoder_process", "seconds": secs, "stream_bytes": len(res[("out", False)]),
                          "host_deflate_ms_median": round(float(np.median(res[False])), 2),
                          "device_deflate_ms_median": round(float(np.median(res[True])), 2),
                          "host_deflate_ms": [round(x, 2) for x in res[False]],
                          "device_deflate_ms": [round(x, 2) for x in res[True]]}), flush=True)


if __name__ == "__main__":
    main()
