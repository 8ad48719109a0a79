#!/usr/bin/env python3
"""Raw-DEFLATE inflate on the device: kernel time, bytes moved, and the decoder end to end.

  * frad_inflate_raw on the deflated payloads of 14 999 profile-1 frames (N = 2048, stereo, 16 bit, ratio 16 -- a 10-minute
    stream at 48 kHz) at loss levels 0.5 and 10: device time of the launch (events, median of --reps), the payload bytes
    uploaded against the inflated bodies the host path uploads, and the host's zlib over the same payloads for scale;
  * Decoder.process of a 60 s and a 10 min profile-1 stream (default loss level) in one call + flush: the default (host inflate) against
    device_inflate=True, alternating, median of --reps, with the outputs compared bit for bit.
Prints one JSON line per measurement.  Needs the MI355X."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def payloads_of(stream: bytes) -> list:
    from frad_python_amd.tools.asfh import ASFH
    pos, out = 0, []
    while pos < len(stream):
        a = ASFH()
        state, _ = a.read(stream[pos:pos + 40])
        pos += a.header_bytes
        if state != "Complete":
            continue
        out.append(stream[pos:pos + a.frmbytes])
        pos += a.frmbytes
    return out


def encode(secs: float, loss: float | None = None) -> bytes:
    from frad_python_amd import synth
    from frad_python_amd.encoder import Encoder
    n = int(secs * 48000)
    pcm = synth.to_pcm(synth.harmonic_mix(n, 2, 48000, seed=2024), "s16le").tobytes()
    enc = Encoder(1, 48000, 2, 16, 2048, "s16le")
    enc.set_overlap_ratio(16)
    if loss is not None:
        enc.set_loss_level(loss)
    return enc.process(pcm).buf + enc.flush().buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=14999)
    args = ap.parse_args()
    import torch
    from frad_python_amd import core
    from frad_python_amd._lib import load
    from frad_python_amd.decoder import Decoder
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = load()
    stride = lib.p1_golomb_bound(2048, 2)
    for loss in (0.5, 10.0):
        pays = payloads_of(encode(args.frames * 1920 / 48000 + 0.05, loss))[:args.frames]
        off = np.zeros(len(pays) + 1, np.int64)
        np.cumsum([len(p) for p in pays], out=off[1:])
        src = torch.from_numpy(np.frombuffer(b"".join(pays), np.uint8).copy()).cuda()
        offs = torch.from_numpy(off).cuda()
        t0 = time.perf_counter()
        bodies = [zlib.decompress(p, wbits=-15) for p in pays]
        host_ms = (time.perf_counter() - t0) * 1e3
        times = []
        for r in range(args.reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            dst = torch.empty(len(pays) * stride + 16, dtype=torch.uint8, device="cuda")
            nb = torch.empty(len(pays), dtype=torch.int64, device="cuda")
            st = torch.empty(len(pays), dtype=torch.int32, device="cuda")
            a.record()
            lib.inflate_raw(src.data_ptr(), offs.data_ptr(), len(pays), dst.data_ptr(), stride, nb.data_ptr(), st.data_ptr(),
                            core._stream_ptr())
            b.record()
            torch.cuda.synchronize()
            if r >= 2:
                times.append(a.elapsed_time(b))
        rows = dst[:len(pays) * stride].view(len(pays), stride).cpu().numpy()
        nbh, sth = nb.cpu().numpy(), st.cpu().numpy()
        assert (sth == 0).all() and all(rows[i, :nbh[i]].tobytes() == bodies[i] for i in range(len(pays)))
        print(json.dumps({"what": "inflate_kernel", "loss_level": loss, "frames": len(pays), "dst_stride": stride,
                          "kernel_ms_median": round(float(np.median(times)), 3), "kernel_ms_min": round(min(times), 3),
                          "payload_bytes": int(off[-1]), "inflated_bytes": int(sum(map(len, bodies))),
                          "host_zlib_serial_ms": round(host_ms, 2)}), flush=True)
    for secs in (60, 600):
        s = encode(secs)
        res = {}
        for r in range(args.reps + 1):
            for mode in (False, True):
                dec = Decoder(device_inflate=mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = dec.process(s).pcm
                tail = dec.flush().pcm
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    res.setdefault(mode, []).append(dt)
                if r == 0:
                    res[("out", mode)] = np.concatenate([x for x in (out, tail) if x.size]).tobytes()
        assert res[("out", False)] == res[("out", True)]
        print(json.dumps({"what": "decoder_process", "seconds": secs, "bytes": len(s),
                          "host_inflate_ms_median": round(float(np.median(res[False])), 2),
                          "device_inflate_ms_median": round(float(np.median(res[True])), 2),
                          "host_inflate_ms": [round(x, 2) for x in res[False]],
                          "device_inflate_ms": [round(x, 2) for x in res[True]]}), flush=True)


if __name__ == "__main__":
    main()
