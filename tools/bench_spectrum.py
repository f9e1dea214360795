#!/usr/bin/env python3
"""What the RF spectrum / waterfall stage (dabx_set_spectrum_mode; k_spectrum) costs, at bench.py's layout: --streams streams x 18
sub-channels of 64 kbit/s, rings filled as bench.py fills them, primed for 40 frames.  Front-end + MSC frames/s and time per step without
a delivery, in the order --order gives:

  off        the mode off on every stream (the stage exists from the first `on` leg: nothing is launched for it)
  on1        the mode on for 1 stream          on         the mode on for all streams

One JSON line per leg; a fresh process per run.  The rings are committed a frame per step; a stream in lock shows every 201 symbols, 2.6
frames, so --chunks 4 (28 steps) gives about 10 shows per stream.  While a stream has the mode on the search runs in step: --unlocked N
leaves N streams searching silence, which is where that shows.  (bench.fill_rings announces its writes once, dabx_announce_write: no
window is given up for the trust rule here.)

  python3 tools/bench_spectrum.py --order off,on1,on,off
  python3 tools/bench_spectrum.py --streams 32
  python3 tools/bench_spectrum.py --unlocked 256        # half of the streams searching: what the search in step costs"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402
from tools import dab_synth as ds  # noqa: E402

TF = bench.TF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--order", default="off,on1,on,off")
    ap.add_argument("--unlocked", type=int, default=0, help="streams that carry silence and stay out of lock (bench.py --unlocked): with the mode on the search runs in step")
    ap.add_argument("--chunks", type=int, default=4, help="timed 7-frame calls per leg (4: 28 steps, about 10 shows per stream)")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    S = a.streams
    subch = ds.default_subchannels(18, 64)
    eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=18, out_frames=8)
    eng.set_subchannels(subch)
    args = types.SimpleNamespace(ensembles=4, snr=20.0, streams=S, unlocked=a.unlocked, unlocked_kind="silence", layout="uniform")
    ring_frames = bench.fill_rings(eng, torch, dev, args, 0, subch)

    def step(n):
        for m in bench.region_chunks(n, 7, False):
            eng.commit(m * TF)
            eng.process(m, sync=False)

    def mode(name):
        eng.set_spectrum_mode(-1, enable=False)
        if name != "off":
            eng.set_spectrum_mode(0 if name.endswith("1") else -1)

    def totals():
        st = [eng.spectrum_stats(s) for s in range(0, S, max(1, S // 8))]
        return [sum(x[k] for x in st) for k in ("shows", "untrusted", "inexact")] + [st[0]["launches"]]

    eng.commit(ring_frames * TF - TF)
    step(40)
    eng.synchronize()
    locked = sum(eng.stats(s)["state"] == 2 for s in range(S))
    for name in a.order.split(","):
        mode(name)
        step(7)
        eng.synchronize()
        f0, t0s = eng.counters()["frames"], totals()
        t0 = time.perf_counter()
        step(7 * a.chunks)
        eng.synchronize()
        dt = time.perf_counter() - t0
        t1s = totals()
        print(json.dumps({"what": name, "streams": S, "locked": locked, "steps": 7 * a.chunks, "frames_per_s": (eng.counters()["frames"] - f0) / dt,
                          "ms_per_step": 1e3 * dt / (7 * a.chunks), "records_sampled": t1s[0] - t0s[0], "untrusted_sampled": t1s[1] - t0s[1],
                          "inexact_sampled": t1s[2] - t0s[2], "stage_launch_steps": t1s[3] - t0s[3]}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
