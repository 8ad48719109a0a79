#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json's configuration.

Metric   : Msamples/s encode+decode, 48 kHz stereo, frame = 2048 (sample = one PCM value).
Workload : --workload cfg2 (default) = configs[1]: 10 min of 48 kHz stereo s16le PCM, profile 0 (DCT archiving),
           32-bit big-endian storage, N = 2048: 14 062 full frames + the 1 024-sample tail frame, batched on one
           MI355X.  Synthetic "signal A" (harmonic mix + -60 dBFS noise), generated on the GPU.
           --workload cfg3 = configs[2]: 4096 x 1 s stereo clips (23 full frames + an 896-sample tail each), whole clips
           sharded over the ranks (contiguous ranges, parallel.shard_range): strong scaling, still no collective.
Step     : one pass of the hot path over the whole workload: analogue (encode) of every frame with the reference's overflow
           test in the same pass (frad_p0_analogue_checked), then digital (decode) of every payload; inputs are resident in
           HBM when the clock starts.
N > 1    : one process per GPU.  Started by the driver (torch.distributed.run sets RANK / LOCAL_RANK / WORLD_SIZE) or,
           when `--gpus N` is given without that environment, by this script: the parent starts N children BEFORE it
           touches the GPU itself and never re-executes a process that has.  cfg2: every rank owns one clip (weak
           scaling); the only collectives are the timing barrier and the max-reduce (parallel.Timer).

Prints ONE JSON line (rank 0).  `roofline` is the dominant kernel of the step: algorithmic bytes per launch (SURVEY 8d:
encode B_in + b/8 = 6 B/sample, decode b/8 + 8 = 12 B/sample) / its mean HIP-event time over the timed steps;
`roofline_cold` the same kernels with three rotating buffer sets (reuse distance > the 256 MiB Infinity Cache).
`cpu_baseline` (one core, one frame per call like the reference) and `cpu_baseline_all_cores` (batched
scipy.fft.dct(workers=all)) time the oracle -- the NumPy/SciPy restatement of the reference path -- on this host.
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SRATE, CHANNELS, FSIZE, BITS = 48000, 2, 2048, 32
SECONDS = 600
HBM_PEAK_GBS = 8000.0                     # MI355X HBM3E peak (MI355X_MICROARCH.md)
PREWARM = 120                             # untimed clock-ramp steps before the warm-up proper
METRIC = "Msamples/s encode+decode, 48 kHz stereo frame=2048; achieved HBM GB/s vs peak"


# ------------------------------------------------------------------------------------------------
# launcher: `bench.py --gpus N` without a torch.distributed environment
# ------------------------------------------------------------------------------------------------
def launch_ranks(n: int, argv: list[str]) -> int:
    """Start n copies of this script, one per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment),
    wait for them, and return the worst exit code.  The parent makes no GPU call before or after: children are
    ordinary subprocesses, nothing is exec'ed over a process that has initialised the device."""
    import socket
    with socket.socket() as s:                                # a free rendezvous port on the loopback interface
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    # wait for all of them -- but a rank that dies (no such device, out of memory) must not leave the others waiting at the
    # rendezvous for ever: the first non-zero exit ends the job
    rc = 0
    live = list(procs)
    while live:
        time.sleep(0.2)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            rc = max(rc, abs(code))
        if rc and live:
            for p in live:
                p.terminate()
            for p in live:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill()                                  # (this child's own PID)
            print(f"bench.py: a rank exited with {rc}; the others were stopped", file=sys.stderr)
            break
    return rc


def csrc_fingerprint() -> str:
    """sha256 over the kernel sources: ties a committed rocprofv3 counter file to the build it was taken from"""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "frad_python_amd", "csrc", "*.h*")) + glob.glob(os.path.join(ROOT, "frad_python_amd", "csrc", "*.inc"))):
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


# ------------------------------------------------------------------------------------------------
# CPU baselines: the oracle on this host's cores (reported next to the GPU figure; never the target)
# ------------------------------------------------------------------------------------------------
def cpu_baseline(pcm_host, n_frames: int, min_seconds: float = 10.0):
    """Oracle, one frame at a time on one core -- the reference's own cost profile (encoder.py:60,
    decoder.py:55 loop one frame per iteration through numpy/scipy)."""
    from oracle import frad_oracle as fo
    dt = fo.pcm_dtype("s16le")
    t0, done = time.perf_counter(), 0
    while time.perf_counter() - t0 < min_seconds:             # whole passes over the sample, >= min_seconds of work
        for f in range(n_frames):
            frame = fo.to_f64(pcm_host[f * FSIZE:(f + 1) * FSIZE], dt)
            frad, idx, ch, sr = fo.p0_analogue(frame, BITS, SRATE, False)
            fo.p0_digital(frad, idx, ch, False)
        done += n_frames
    dt_s = time.perf_counter() - t0
    return done * FSIZE * CHANNELS / dt_s / 1e6, dt_s, done


def cpu_baseline_all_cores(pcm_host, n_frames: int, min_seconds: float = 8.0):
    """Oracle on every host core: the clip's frames in chunks, one chunk per thread at a time, each chunk through the
    batched restatement (scipy.fft.dct / idct over all its channel rows + vectorised cast / pack / unpack -- bitwise the
    per-frame result, SURVEY 8d (ii), tests/test_oracle_golden.py).  NumPy / pocketfft release the GIL, so the chunks run
    in parallel; the casts and transposes are threaded this way too, which scipy's `workers=` alone would not do."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import frad_oracle as fo
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    chunk = 32
    spans = [(a, min(a + chunk, n_frames)) for a in range(0, n_frames, chunk)]

    def work(span):
        a, b = span
        pay = fo.p0_analogue_batch(pcm_host[a * FSIZE:b * FSIZE], b - a, FSIZE, CHANNELS, BITS)
        fo.p0_digital_batch(pay, b - a, FSIZE, CHANNELS, BITS)
        return b - a
    t0, done = time.perf_counter(), 0
    with ThreadPoolExecutor(max_workers=cores) as pool:
        while time.perf_counter() - t0 < min_seconds:
            done += sum(pool.map(work, spans))
    dt_s = time.perf_counter() - t0
    return done * FSIZE * CHANNELS / dt_s / 1e6, dt_s, done, cores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # a step is ~0.26 ms of GPU work and the card needs ~10 ms of sustained load to reach its steady clocks: the defaults
    # warm up past that ramp and time long enough for a stable figure (still < 0.2 s of GPU time)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", choices=("cfg2", "cfg3"), default="cfg2")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dry-run", action="store_true", help="launcher / rendezvous rehearsal without a GPU (tests)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (seeded sample, <= 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))       # (no GPU call has been made in this process)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and "WORLD_SIZE" in os.environ and args.gpus != 1:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)

    import numpy as np
    import torch
    from frad_python_amd.parallel import Timer, shard_range

    if args.dry_run:
        # rendezvous + timing protocol only: gloo on CPU, no device, no kernels (tests/test_parallel.py)
        if os.environ.get("FRAD_BENCH_DRYRUN_DIE") == str(rank):              # (test hook: this rank is lost before the rendezvous)
            sys.exit(3)
        dist = None
        if world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo", rank=rank, world_size=world)
        a, b = shard_range(4096, rank, world)
        timer = Timer(dist)
        elapsed = timer.measure(lambda: time.sleep(0.01 * (rank + 1)))
        if rank == 0:
            print(json.dumps({"metric": METRIC, "value": 0.0, "unit": "Msamples/s", "n_gpus": world, "steps": args.steps,
                              "warmup": args.warmup, "dry_run": True, "ms_per_step": round(elapsed * 1e3, 3),
                              "rank_ms_per_step": {"min": round(min(timer.per_rank) * 1e3, 3), "max": round(max(timer.per_rank) * 1e3, 3)},
                              "clips_rank0": b - a}), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    from frad_python_amd import core
    assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU path"
    # one process per GPU; FRAD_BENCH_BACKEND=gloo lets several ranks rehearse on fewer GPUs (ranks then share
    # devices round-robin) -- the data path has no collective either way
    backend = os.environ.get("FRAD_BENCH_BACKEND", "nccl")
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    if local >= torch.cuda.device_count():
        sys.exit(f"bench.py: rank {rank} wants GPU {local}, this node shows {torch.cuda.device_count()} "
                 "(FRAD_BENCH_BACKEND=gloo lets ranks share devices for a rehearsal)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    def signal_a(n: int, seed: int) -> "torch.Tensor":
        """ "Signal A" of SURVEY 8d as s16le, synthesised on the device: 8 partials of 110*(c+1) Hz with 0.5 Hz AM,
        peak 0.8, plus -60 dBFS white noise."""
        g = torch.Generator(device=dev).manual_seed(seed)
        t = torch.arange(n, dtype=torch.float64, device=dev) / SRATE
        out = torch.empty((n, CHANNELS), dtype=torch.float64, device=dev)
        for c in range(CHANNELS):
            ph = torch.rand(8, generator=g, device=dev, dtype=torch.float64) * 2 * np.pi
            x = torch.zeros(n, dtype=torch.float64, device=dev)
            for h in range(8):
                x += torch.sin(2 * np.pi * 110.0 * (c + 1) * (h + 1) * t + ph[h]) / (h + 1)
            x *= 0.75 + 0.25 * torch.sin(2 * np.pi * 0.5 * t + c)
            out[:, c] = x
        out *= 0.8 / out.abs().max()
        out += torch.randn((n, CHANNELS), generator=g, device=dev, dtype=torch.float64) * 1e-3
        return torch.clamp(torch.round(out * 32768.0), -32768, 32767).to(torch.int16)

    lib = core._lib.load()
    lib.plan_prepare(FSIZE, False)

    class Workload:
        """cfg2: one 10-minute clip per rank (n_clips = 1).  cfg3: this rank's share of 4096 one-second clips, resident as
        [clips, 48000, C] and consumed / produced IN PLACE (frad_p0_analogue_clips / frad_p0_digital_clips: no gathered
        copies): the 23 full frames of every clip are one batch on the main stream, the 896-sample tails (Bluestein
        kernels) another on the side stream, which never joins inside the timed region."""

        def __init__(self, seed, sets=1):
            if args.workload == "cfg2":
                self.n_clips, self.clip_len = 1, SRATE * SECONDS
            else:
                a, b = shard_range(4096, rank, world)
                self.n_clips, self.clip_len = b - a, SRATE
            self.full_per_clip = self.clip_len // FSIZE
            self.tail = self.clip_len - self.full_per_clip * FSIZE
            self.n_full = self.n_clips * self.full_per_clip
            self.n_tail = self.n_clips if self.tail else 0
            self.samples = self.n_clips * self.clip_len * CHANNELS
            self.gather = self.n_clips > 1
            if self.tail:
                lib.plan_prepare(self.tail, False)
            nb = lib.payload_bytes(FSIZE, CHANNELS, BITS)
            self.sets = []
            for s in range(sets):
                d = {}
                if args.workload == "cfg2":
                    d["clips"] = signal_a(self.clip_len, seed + 977 * s).reshape(1, self.clip_len, CHANNELS)
                else:                                         # a 5 s excerpt of signal A per 5 clips keeps the synthesis short
                    base = signal_a(self.clip_len * 8, seed + 977 * s).reshape(8, self.clip_len, CHANNELS)
                    d["clips"] = base.repeat((self.n_clips + 7) // 8, 1, 1)[:self.n_clips].contiguous()
                d["pay"] = torch.empty((self.n_full, nb), dtype=torch.uint8, device=dev)
                d["absmax_all"] = torch.empty(self.n_full + self.n_tail, dtype=torch.float64, device=dev)
                if self.gather:                               # decoded clips, whole: full frames and tails land in place
                    d["out_clips"] = torch.empty((self.n_clips, self.clip_len, CHANNELS), dtype=torch.float64, device=dev)
                else:
                    d["out"] = torch.empty((self.n_full, FSIZE, CHANNELS), dtype=torch.float64, device=dev)
                if self.tail:
                    nbt = lib.payload_bytes(self.tail, CHANNELS, BITS)
                    d["pay_t"] = torch.empty((self.n_tail, nbt), dtype=torch.uint8, device=dev)
                    if not self.gather:
                        d["out_t"] = torch.empty((self.n_tail, self.tail, CHANNELS), dtype=torch.float64, device=dev)
                self.sets.append(d)
            self.cur = self.sets[0]
            self.over = torch.zeros((), dtype=torch.int32, device=dev)
            # cfg2: the clip's last, short frame is independent of the 14 062 full ones (own input slice, own buffers): it
            # runs on a second HIP stream so that its tiny launches overlap the big batch instead of queueing behind it.
            # The two streams never wait for each other inside the timed region -- the closing synchronize covers both.
            self.side = torch.cuda.Stream(device=dev)
            self.side.wait_stream(torch.cuda.current_stream())

        def use(self, i):
            self.cur = self.sets[i % len(self.sets)]

        def _tails(self, d):
            am = d["absmax_all"][self.n_full:]
            first = self.full_per_clip * FSIZE
            if self.gather:                                   # every clip's last, short frame: read and written inside the clips
                core.analogue_clips(d["clips"], "s16le", self.tail, BITS, False, first=first, out=d["pay_t"], absmax=am, overflow_flag=self.over)
                core.digital_clips(d["pay_t"], d["out_clips"], self.tail, BITS, False, first=first)
                return
            core.analogue_batch(0, d["clips"][0, first:], "s16le", self.n_tail, self.tail, CHANNELS, BITS, False, check_overflow=False,
                                out=d["pay_t"], absmax=am, overflow_flag=self.over)
            core.digital_batch(0, d["pay_t"], self.n_tail, self.tail, CHANNELS, BITS, False, out=d["out_t"])

        def encode(self, ev=None):
            d = self.cur
            if ev: ev[0].record()
            # (the reference's per-frame overflow test, profile0.py:24-26, rides along: frad_p0_analogue_checked sets the
            #  sticky device flag; the host reads it once, after the timed region)
            if self.gather:
                core.analogue_clips(d["clips"], "s16le", FSIZE, BITS, False, out=d["pay"], absmax=d["absmax_all"][:self.n_full],
                                    overflow_flag=self.over)
            else:
                core.analogue_batch(0, d["clips"], "s16le", self.n_full, FSIZE, CHANNELS, BITS, False, check_overflow=False,
                                    out=d["pay"], absmax=d["absmax_all"][:self.n_full], overflow_flag=self.over)
            if ev: ev[1].record()
            if self.tail:
                with torch.cuda.stream(self.side):            # the tail frames fill CUs as the resident kernels' blocks retire
                    self._tails(d)

        def decode(self, ev=None):
            d = self.cur
            if ev: ev[0].record()
            if self.gather:
                core.digital_clips(d["pay"], d["out_clips"], FSIZE, BITS, False)
            else:
                core.digital_batch(0, d["pay"], self.n_full, FSIZE, CHANNELS, BITS, False, out=d["out"])
            if ev: ev[1].record()

        def step(self, ev_e=None, ev_d=None):
            self.encode(ev_e); self.decode(ev_d)

    wl = Workload(seed=1234 + rank)

    # ---- cold start: the first steps after set-up, before the clocks have ramped (reported, not the headline) ----
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        wl.step()
    torch.cuda.synchronize()
    cold_start_ms = (time.perf_counter() - t0) / 5 * 1e3

    # untimed: whatever --warmup says, run at least PREWARM steps (~35 ms) first so that the card is at its steady
    # clocks when the W warm-up steps and the K timed steps run (the ramp is ~10 ms)
    for _ in range(max(0, PREWARM - args.warmup)):
        wl.step()
    for _ in range(args.warmup):
        wl.step()
    ev_enc = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    ev_dec = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]

    def timed_steps():
        for i in range(args.steps):
            wl.step(ev_enc[i], ev_dec[i])
    # barrier + torch.cuda.synchronize() on both sides of exactly K steps, MAX over ranks (parallel.Timer)
    timer = Timer(dist, torch.cuda.synchronize)
    elapsed = timer.measure(timed_steps)
    assert int(wl.over.item()) == 0, "synthetic audio must not overflow float32 storage"
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, wl, wl.cur, rank, world)

    enc_ms = float(np.mean([a.elapsed_time(b) for a, b in ev_enc]))
    dec_ms = float(np.mean([a.elapsed_time(b) for a, b in ev_dec]))
    full = wl.n_full * FSIZE * CHANNELS                      # samples one main launch processes
    enc_bytes, dec_bytes = full * (2 + BITS // 8), full * (BITS // 8 + 8)

    def roof(name, nbytes, ms):
        gbs = nbytes / (ms * 1e-3) / 1e9
        return {"kernel": name, "bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": None, "bytes_per_launch": nbytes,
                "avg_launch_ms": round(ms, 4)}
    ENC_NAME = "k_p0_fwd_wave<s16,C=2,32> (LDS-DMA load+to_f64+DCT-II 32x32+absmax+f32 cast+BE pack)"
    DEC_NAME = "k_p0_inv_wave<C=2,32> (unpack+scrub+inverse DCT pair step+32x32 IDFT+f64 interleaved store)"
    r_enc, r_dec = roof(ENC_NAME, enc_bytes, enc_ms), roof(DEC_NAME, dec_bytes, dec_ms)
    # HBM traffic per launch from the committed rocprofv3 PMC passes (profiles/, tools/profile_round.sh: FETCH_SIZE and
    # WRITE_SIZE in separate passes, FETCH_SIZE x2 as the gfx950 guide prescribes) -- only when that file was taken from
    # THIS build of the kernels; a stale file is named and ignored
    tsrc = None
    if args.workload == "cfg2":
        try:
            cnt = json.load(open(os.path.join(ROOT, "profiles", "r03_counters.json")))
            meta = cnt.get("_meta", {})
            tsrc = {"file": "profiles/r03_counters.json", "csrc_sha": meta.get("csrc_sha"), "git": meta.get("git")}
            if meta.get("csrc_sha") == csrc_fingerprint():
                for r, key in ((r_enc, "k_p0_fwd"), (r_dec, "k_p0_inv")):
                    hit = [v for k, v in cnt.items() if key in k and isinstance(v, dict) and int(v.get("hbm_bytes_per_launch_corrected", 0)) > 1e8]
                    if hit:
                        r["traffic"] = int(hit[0]["hbm_bytes_per_launch_corrected"])
            else:
                tsrc["stale"] = True
        except Exception:
            tsrc = None
    dominant, other = (r_dec, r_enc) if dec_ms >= enc_ms else (r_enc, r_dec)

    extra = {}
    if rank == 0 and world == 1 and args.workload == "cfg2":
        # ---- cold kernels: three rotating buffer sets (2.4 GB in flight) so that neither the payload decode reads nor
        # the PCM encode reads can still sit in the 256 MiB Infinity Cache from the launch before ----
        del wl
        torch.cuda.empty_cache()
        wc = Workload(seed=4321, sets=3)
        for i in range(30):
            wc.use(i); wc.step()
        n = 45
        ce = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        cd = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for i in range(n):                                    # all encodes, then all decodes: a set's payload was written 3 launches (2.1 GB) ago
            wc.use(i); wc.encode(ce[i])
        for i in range(n):
            wc.use(i); wc.decode(cd[i])
        torch.cuda.synchronize()
        ce_ms = float(np.mean([a.elapsed_time(b) for a, b in ce[5:]]))
        cd_ms = float(np.mean([a.elapsed_time(b) for a, b in cd[5:]]))
        extra["roofline_cold"] = {"encode": roof(ENC_NAME, enc_bytes, ce_ms), "decode": roof(DEC_NAME, dec_bytes, cd_ms),
                                  "note": "3 rotating buffer sets, reuse distance > 2 GB (Infinity Cache is 256 MiB)"}
        # the HBM-honest fraction next to the pipeline one, inside the parsed roofline block: in a step the payload decode reads
        # was written a launch earlier and partly comes from the Infinity Cache; `frac_cold` has no such help
        r_enc["frac_cold"], r_dec["frac_cold"] = extra["roofline_cold"]["encode"]["frac"], extra["roofline_cold"]["decode"]["frac"]
        # ---- yardstick: the library's own 16 B/lane copy kernel over the encode-sized and decode-sized footprints ----
        src = wc.sets[0]["out"].view(torch.uint8).reshape(-1)
        dst = wc.sets[1]["out"].view(torch.uint8).reshape(-1)
        nbytes = src.numel() // 16 * 16
        stream = int(torch.cuda.current_stream().cuda_stream)
        for _ in range(10):
            lib.bench_copy(src.data_ptr(), dst.data_ptr(), nbytes, stream)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            lib.bench_copy(src.data_ptr(), dst.data_ptr(), nbytes, stream)
        b.record(); torch.cuda.synchronize()
        extra["copy_yardstick"] = {"kernel": "frad_bench_copy (16 B/lane, 4 loads in flight)", "bytes": nbytes,
                                   "GB/s_read_plus_write": round(2 * nbytes * 20 / (a.elapsed_time(b) * 1e-3) / 1e9, 1)}
        host = wc.sets[0]["clips"][0, :wc.n_full * FSIZE].cpu().numpy()
        n_full = wc.n_full
        del wc
    if rank == 0:
        total_samples = wl_samples_total(args.workload, world, SRATE, SECONDS, CHANNELS)
        value = total_samples * args.steps / elapsed / 1e6
        line = {
            "metric": METRIC,
            "value": round(value, 1), "unit": "Msamples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            # every rank's own time to its local device sync, before the closing barrier: a straggler is visible here
            "rank_ms_per_step": {"min": round(min(timer.per_rank) / args.steps * 1e3, 4), "max": round(max(timer.per_rank) / args.steps * 1e3, 4)},
            "scaling": "weak" if args.workload == "cfg2" else "strong",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": ("configs[1]: 10 min 48 kHz stereo s16le, profile 0, bits=32 BE, frame=2048, "
                                    "14062 frames + 1024-sample tail per GPU, encode + overflow test + decode")
                       if args.workload == "cfg2" else
                       ("configs[2]: 4096 x 1 s 48 kHz stereo s16le clips (23 frames of 2048 + 896-sample tail each), profile 0, "
                        "bits=32 BE, whole clips sharded over the GPUs, encode + overflow test + decode"),
                       "prewarm_steps": max(0, PREWARM - args.warmup), "samples_total": total_samples,
                       "parallelism": f"frames sharded over {world} GPU(s), no collectives"},
            "roofline": dominant, "roofline_other": other,
            "hbm_frac_enc_plus_dec": round((enc_bytes + dec_bytes) / ((enc_ms + dec_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "cold_start_ms_per_step": round(cold_start_ms, 4),
            "traffic_source": tsrc,
        }
        line.update(extra)
        if world == 1 and not args.no_cpu_baseline and args.workload == "cfg2":
            v, secs, done = cpu_baseline(host, n_full)
            line["cpu_baseline"] = {"value": round(v, 2), "unit": "Msamples/s", "cores": 1, "kind": "port",
                                    "sample": f"the clip's {n_full} full frames, {done // n_full} pass(es) = {done * FSIZE * CHANNELS} samples "
                                              f"encode+decode, one frame per call like the reference loop, {secs:.1f} s of CPU work",
                                    "host_cpus": os.cpu_count()}
            v, secs, done, cores = cpu_baseline_all_cores(host, n_full)
            line["cpu_baseline_all_cores"] = {"value": round(v, 2), "unit": "Msamples/s", "cores": cores, "kind": "port",
                                              "sample": f"the same {n_full} frames in chunks of 32 over a pool of {cores} threads "
                                                        f"(batched scipy.fft + vectorised pack per chunk), {done // n_full} pass(es), {secs:.1f} s"}
            line["vs_cpu_baseline"] = round(value / line["cpu_baseline"]["value"], 1)
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


DUMP_BYTES = 60_000_000                  # --dump-outputs: all ranks' .npy data together (< 64 MB with headers)
DUMP_SEED = 20251015


def dump_outputs(out_dir: str, wl, d: dict, rank: int, world: int) -> None:
    """--dump-outputs DIR: what the last timed step handed its caller, as .npy files a second build can be compared with.
      absmax         float64 [frames]              per-frame max |x| from the encode (full frames, then the tails)
      payload        float32 [rows, N*C]           the encoded frames, 32-bit big-endian words read as float32
      decoded        float64 [rows, N, C]          the decoded PCM of the same frames (cfg3: [clips, 48000, C], whole clips)
      payload_tail / decoded_tail                  the same for the short tail frames
      sample_index   float64 [rows]                which frames (cfg2) or clips (cfg3) the sampled arrays hold
    The full output is ~0.7 GB, so whole frames / clips are sampled: a fixed seed picks the same ones on every run.  With
    several ranks, rank r writes <name>.rank<r>.npy and the budget is split between the ranks."""
    import numpy as np
    import torch

    def words(pay):                                           # uint8 rows of BE float32 words -> float32 values
        return pay.cpu().numpy().view(">f4").astype(np.float32)

    tail_pay = d.get("pay_t")
    fixed = d["absmax_all"].numel() * 8
    if wl.gather:                                             # cfg3: whole clips, every frame of a clip in place
        n_units = wl.n_clips
        per_unit = wl.full_per_clip * d["pay"].shape[1] + (tail_pay.shape[1] if wl.tail else 0) + wl.clip_len * CHANNELS * 8
    else:                                                     # cfg2: full frames; the tail frame is always written whole
        n_units = wl.n_full
        per_unit = d["pay"].shape[1] + FSIZE * CHANNELS * 8
        if wl.tail:
            fixed += tail_pay.numel() + d["out_t"].numel() * 8
    k = int(min(n_units, (DUMP_BYTES // world - fixed) // (per_unit + 8)))
    assert k >= 1, "--dump-outputs: the fixed outputs alone exceed the budget"
    pick = np.sort(np.random.default_rng(DUMP_SEED).choice(n_units, size=k, replace=False))
    sel = torch.from_numpy(pick).to(d["pay"].device)
    out = {"absmax": d["absmax_all"].cpu().numpy(), "sample_index": pick.astype(np.float64)}
    if wl.gather:
        rows = (sel[:, None] * wl.full_per_clip + torch.arange(wl.full_per_clip, device=sel.device)).reshape(-1)
        out["payload"] = words(d["pay"].index_select(0, rows))
        out["decoded"] = d["out_clips"].index_select(0, sel).cpu().numpy()
        if wl.tail:
            out["payload_tail"] = words(tail_pay.index_select(0, sel))
    else:
        out["payload"] = words(d["pay"].index_select(0, sel))
        out["decoded"] = d["out"].index_select(0, sel).cpu().numpy()
        if wl.tail:
            out["payload_tail"] = words(tail_pay)
            out["decoded_tail"] = d["out_t"].cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    suffix = f".rank{rank}" if world > 1 else ""
    for name, a in out.items():
        assert a.dtype in (np.float32, np.float64), name
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a)
    print(f"bench.py: wrote {', '.join(out)} ({sum(a.nbytes for a in out.values()) / 2**20:.1f} MiB, {k} of {n_units} "
          f"{'clips' if wl.gather else 'frames'}) to {out_dir}", file=sys.stderr, flush=True)


def wl_samples_total(workload, world, srate, seconds, channels):
    return world * srate * seconds * channels if workload == "cfg2" else 4096 * srate * channels


if __name__ == "__main__":
    main()
