#!/usr/bin/env python3
"""What the IQ ring's element costs or saves: bench.py's workload -- 512 synthetic ensembles, 18 x 64 kbit/s DAB+, rings resident in
HBM and committed frame by frame -- quantised once to int16 and to uint8 and run with

  cf32   a cf32 ring holding the expanded int16 codes (what every engine did before dabx_create_ex: the conversion at the store),
  s16    a DABX_RING_S16 ring holding the int16 codes,
  u8     a DABX_RING_U8 ring holding the uint8 codes.

Results stay on the device (no delivery: its link traffic is the same for all three and would only dilute the difference).  Every
configuration runs in a fresh child process -- from the third engine created in a process on, an engine's HIP streams share hardware
queues with the closed ones' (docs/history/r06.md, ab12) --, the three alternate, --reps each (>= 3), every child under its own
time limit, and the chain stops at the first child that fails.  One JSON line: frames/s per configuration (min / median / max of the
repetitions) and the ring bytes allocated.

  python3 tools/bench_ring_format.py [--streams 512] [--steps 49] [--warmup 14] [--reps 3]
  python3 tools/bench_ring_format.py --child s16 --steps 14        # one configuration, one line (what rocprofv3 is given)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TF = 196608
CONFIGS = ("cf32", "s16", "u8")


def child(args):
    import numpy as np
    import torch
    from dabstar_amd import lib as dx
    from dabstar_amd import shard
    from tools import dab_synth as ds
    dev = torch.device("cuda:0")
    dx.check(dx.load().dabx_set_device(0))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    subch = ds.default_subchannels(18, 64)
    n_frames = 10
    eng = dx.Engine(n_streams=args.streams, ring_frames=n_frames, max_subch=18, out_frames=8, ring_format=args.child)
    eng.set_subchannels(subch)
    fmt, bps = eng.ring_format()
    base = [torch.from_numpy(ds.build_ensemble(n_frames, subch, seed=e, cyclic=True).iq).to(dev) for e in range(args.ensembles)]
    n = n_frames * TF
    t = torch.arange(n, device=dev, dtype=torch.float64)
    sigma = float(np.sqrt(10 ** (-args.snr / 10) / 2))
    gen = torch.Generator(device=dev)
    for s in range(args.streams):
        gen.manual_seed(s)
        toff, cfo = shard.stream_params(s, TF)
        ph = (2.0 * np.pi * cfo / 2048000.0) * t
        rot = torch.complex(torch.cos(ph), torch.sin(ph)).to(torch.complex64)
        noise = torch.complex(torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)) * sigma
        y = torch.view_as_real(((torch.roll(base[s % args.ensembles], toff) * rot + noise) * 0.25).to(torch.complex64)).reshape(-1)
        if args.child == "u8":
            ring = torch.clamp(torch.round(y * 128.0 + 127.38), 0, 255).to(torch.uint8)
        else:
            ring = torch.clamp(torch.round(y * 32768.0), -32768, 32767).to(torch.int16)
            if args.child == "cf32":                               # the conversion at the store: x / 32768, exact
                ring = ring.to(torch.float32) / 32768.0
        ring = ring.contiguous()
        ptr, cap = eng.ring_ptr(s)
        assert cap == n and ring.numel() * ring.element_size() == n * bps
        torch.cuda.synchronize()
        assert hip.hipMemcpy(ptr, ring.data_ptr(), n * bps, 3) == 0    # device to device
    torch.cuda.synchronize()
    eng.announce_write(n)

    def step(k):
        for m in ([k % 7] if k % 7 else []) + [7] * (k // 7):
            eng.commit(m * TF)
            eng.process(m, sync=False)
    import gc
    gc.collect()
    gc.disable()
    eng.commit(n - TF)
    step(40)                                                       # priming: acquisition, de-interleaver fill, super-frame sync
    eng.synchronize()
    step(args.warmup)
    eng.synchronize()
    c0 = eng.counters()
    t0 = time.perf_counter()
    step(args.steps)
    eng.synchronize()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    frames = c1["frames"] - c0["frames"]
    line = dict(config=args.child, ring_format=fmt, bytes_per_sample=bps, ring_bytes=args.streams * n * bps, streams=args.streams, steps=args.steps,
                frames=frames, seconds=dt, frames_per_s=frames / dt, streams_locked=c1["streams_locked"], sf_ok=c1["sf_ok"] - c0["sf_ok"],
                sf_fail=c1["sf_fail"] - c0["sf_fail"], fib_ok=c1["fib_ok"] - c0["fib_ok"], fib_total=c1["fib_total"] - c0["fib_total"])
    if args.ingest_leg:
        # behind the timed region, for a kernel trace: four one-frame slabs of the configuration's codes through the bulk ingest --
        # expanded to cf32 by its conversion kernel (cf32) or copied as they are (s16, u8)
        eng.ingest_open(np.uint8 if args.child == "u8" else np.int16, slabs=2, max_frames=1, copy_engine=1)
        for k in range(4):
            eng.ingest_submit(k % 2, TF)
            eng.ingest_commit(k % 2)
            eng.process(1, sync=True)
        eng.ingest_close()
    eng.close()
    print(json.dumps(line), flush=True)
    return 0 if frames == args.streams * args.steps else 3         # every stream in lock, every step a frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--ensembles", type=int, default=4)
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--steps", type=int, default=49)
    ap.add_argument("--warmup", type=int, default=14)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--ingest-leg", action="store_true", help="--child only: four one-frame bulk-ingest commits behind the timed region (kernel traces)")
    ap.add_argument("--child", choices=CONFIGS, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.reps < 3:
        ap.error("--reps: at least three repetitions per configuration")
    runs = {c: [] for c in CONFIGS}
    for rep in range(args.reps):
        for c in CONFIGS:                                         # alternated: a drift of the box goes into every configuration alike
            cmd = [sys.executable, os.path.abspath(__file__), "--child", c, "--streams", str(args.streams), "--ensembles", str(args.ensembles),
                   "--snr", str(args.snr), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                print("bench_ring_format: %s (repetition %d) ran into its time limit of %d s: stopping" % (c, rep, args.child_timeout), file=sys.stderr)
                return 124
            if p.returncode != 0:                                 # nothing more is started on the GPU behind a child that failed
                print("bench_ring_format: %s (repetition %d) exited with %d: stopping\n%s" % (c, rep, p.returncode, p.stderr[-2000:]), file=sys.stderr)
                return p.returncode if p.returncode > 0 else 1
            line = json.loads(p.stdout.strip().split("\n")[-1])
            print(json.dumps(line), file=sys.stderr, flush=True)
            runs[c].append(line)
    out = dict(workload="%d ensembles x 18 x 64 kbit/s DAB+, %d steps after %d warm-up, results left on the device" % (args.streams, args.steps, args.warmup),
               reps=args.reps)
    for c in CONFIGS:
        f = [r["frames_per_s"] for r in runs[c]]
        out[c] = dict(frames_per_s_min=min(f), frames_per_s_median=statistics.median(f), frames_per_s_max=max(f), ring_bytes=runs[c][0]["ring_bytes"],
                      bytes_per_sample=runs[c][0]["bytes_per_sample"])
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
