"""decode_batch against a loop of per-stream Decoders over the same one-second clips.

    python tools/batch_decode_bench.py [--clips 256 4096] [--reps 7] [--json profiles/batch_decode.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/batch_decode_bench.py --trace      # k_clips_ola's time

One-second 48 kHz stereo clips (seeded synth.harmonic_mix), profile 1 (overlap ratio 16, default loss level) and profile 0 at
32 bit.  Both contestants decode the same list of streams to float64 numpy arrays and end in a device synchronise; they alternate
in one process after a warm-up, and the median of --reps rounds is reported.  ``--distinct`` clips are encoded and repeated
to fill the batch (decoding does not care, encoding 4 096 clips would only lengthen the set-up)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_streams(profile, n, distinct):
    from frad_python_amd import Encoder, synth
    base = synth.harmonic_mix(48000 + distinct, 2, 48000, seed=77)
    out = []
    for i in range(min(n, distinct)):
        pcm = synth.to_pcm(np.ascontiguousarray(base[i:i + 48000]) * (0.5 + 0.4 * (i % 7) / 7), "s16le").tobytes()
        enc = Encoder(profile, 48000, 2, 16 if profile == 1 else 32, 2048, "s16le")
        if profile == 1:
            enc.set_overlap_ratio(16)
        out.append(enc.process(pcm).buf + enc.flush().buf)
    return [out[i % len(out)] for i in range(n)]


def loop_of_decoders(streams, bridge):
    from frad_python_amd import Decoder
    res = []
    for s in streams:
        dec = Decoder(bridge=bridge)
        pieces = [dec.process(s).pcm]
        while True:
            before = len(dec.buffer)
            r = dec.process(b"")
            if not r.pcm.size and len(dec.buffer) >= before:
                break
            pieces.append(r.pcm)
        pieces.append(dec.flush().pcm)
        res.append(np.concatenate([p for p in pieces if p.size]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", action="store_true", help="two decode_batch calls of 256 profile-1 clips and nothing else")
    a = ap.parse_args()
    import torch
    from frad_python_amd import decode_batch
    from frad_python_amd.bridge import HipBridge
    bridge = HipBridge()
    sync = torch.cuda.synchronize
    if a.trace:
        streams = make_streams(1, 256, a.distinct)
        for _ in range(2):
            res = decode_batch(streams, bridge=bridge)
        sync()
        rows = sum(p.shape[0] for p in res.pcm)
        frames = sum(res.frames)
        print(json.dumps({"trace": "profile 1, 256 clips", "frames": frames, "bytes_read": frames * 2048 * 2 * 8, "bytes_written": rows * 2 * 8}))
        return
    results = []
    for profile in (1, 0):
        for n in a.clips:
            streams = make_streams(profile, n, a.distinct)
            got, want = decode_batch(streams, bridge=bridge), loop_of_decoders(streams, bridge)      # warm-up, and the same answer
            assert got.fallback == [] and all(np.array_equal(g, w) for g, w in zip(got.pcm, want))
            del got, want
            tb, tl = [], []
            for _ in range(a.reps):
                sync(); t0 = time.perf_counter(); decode_batch(streams, bridge=bridge); sync(); tb.append(time.perf_counter() - t0)
                sync(); t0 = time.perf_counter(); loop_of_decoders(streams, bridge); sync(); tl.append(time.perf_counter() - t0)
            row = {"profile": profile, "clips": n, "stream_bytes": sum(len(s) for s in streams), "reps": a.reps,
                   "batch_s": statistics.median(tb), "loop_s": statistics.median(tl),
                   "batch_s_all": [round(t, 5) for t in tb], "loop_s_all": [round(t, 5) for t in tl]}
            row["loop_over_batch"] = row["loop_s"] / row["batch_s"]
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"what": "decode_batch vs a loop of per-stream Decoders, one-second 48 kHz stereo clips, float64 numpy out, "
                               "wall seconds, median of reps, alternating in one process", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
