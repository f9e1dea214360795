#!/usr/bin/env python3
"""What following the FIC on the device (dabx_set_fig_mode; k_fig) costs, at bench.py's layout: --streams streams x 18 sub-channels of 64
kbit/s, rings filled as bench.py fills them (an 18-sub-channel ensemble's own FIC), primed for 40 frames.  Three measurements, one JSON line
each; a fresh process per run.

  legs       front-end + MSC frames/s and time per step without a delivery, with the mode off and on for all streams, in the order --order
             gives (alternating: the spread between two legs of one kind is the noise the difference has to be read against)
  k_fig      the kernel's own time per launch (= per frame of all streams) between two HIP events: the first ten frames of fresh decoders
             (tables and, where the FIC has them, labels are being filed) and the steady state behind them (every key is known)
  follow     the wall time of the host loop the stage replaces -- dabx_follow_fic for every stream -- over the same 7 frames per call,
             with the mode off: two blocking copies per frame and stream and walk_fib on the host

  python3 tools/bench_fig.py
  python3 tools/bench_fig.py --streams 32 --order off,on,off,on"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402
from tools import dab_synth as ds  # noqa: E402

TF = bench.TF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--order", default="off,on,off,on,off,on")
    ap.add_argument("--chunks", type=int, default=4, help="timed 7-frame calls per leg")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    S = a.streams
    subch = ds.default_subchannels(18, 64)
    eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=18, out_frames=8)
    eng.set_subchannels(subch)
    args = types.SimpleNamespace(ensembles=4, snr=20.0, streams=S, unlocked=0, unlocked_kind="silence", layout="uniform")
    ring_frames = bench.fill_rings(eng, torch, dev, args, 0, subch)

    def step(n, sync_each=False):
        for m in bench.region_chunks(n, 7, False):
            eng.commit(m * TF)
            eng.process(m, sync=sync_each)

    eng.commit(ring_frames * TF - TF)
    step(40)
    eng.synchronize()
    locked = sum(eng.stats(s)["state"] == 2 for s in range(S))
    # ---- the legs
    for name in a.order.split(","):
        eng.set_fig_mode(-1, enable=name == "on")
        step(7)
        eng.synchronize()
        f0 = eng.counters()["frames"]
        t0 = time.perf_counter()
        step(7 * a.chunks)
        eng.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"what": "leg_" + name, "streams": S, "locked": locked, "steps": 7 * a.chunks, "frames_per_s": (eng.counters()["frames"] - f0) / dt,
                          "ms_per_step": 1e3 * dt / (7 * a.chunks), "k_fig_launches": eng.fig_stats(0)["launches"]}), flush=True)
    # ---- the kernel alone: fresh decoders, then the steady state
    eng.set_fig_mode(-1, enable=False)
    eng.set_fig_mode(-1)
    dx.fig_timing(eng, True)
    step(10)
    first = dx.fig_timing(eng, True)
    step(56)
    steady = dx.fig_timing(eng, False)
    st = eng.fig_stats(0)
    print(json.dumps({"what": "k_fig", "streams": S, "first_ten_frames_us": [round(1e3 * float(v), 1) for v in first],
                      "steady_us_median": round(1e3 * float(np.median(steady)), 1), "steady_us_min": round(1e3 * float(steady.min()), 1),
                      "steady_us_max": round(1e3 * float(steady.max()), 1), "steady_launches": int(len(steady)),
                      "stream0": {k: st[k] for k in ("fibs_good", "figs", "subch_new", "subch_known", "comp_new", "comp_known", "label_new", "events")},
                      "subchannels_found": len(eng.fig_subchannels(0))}), flush=True)
    # ---- the host loop it replaces, on the same frames
    eng.set_fig_mode(-1, enable=False)
    for s in range(S):
        eng.follow_fic(s)                      # (creates the decoders, feeds what the ring holds)
    walls = []
    for _ in range(4):
        step(7)
        eng.synchronize()
        t0 = time.perf_counter()
        for s in range(S):
            r = eng.follow_fic(s)
        walls.append(time.perf_counter() - t0)
        assert r["frames_missed"] == 0
    print(json.dumps({"what": "follow_fic_loop", "streams": S, "frames_per_call": 7, "wall_ms_per_7_frames": [round(1e3 * w, 1) for w in walls],
                      "wall_ms_per_frame_median": round(1e3 * float(np.median(walls)) / 7, 2)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
