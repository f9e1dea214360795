#!/usr/bin/env python3
"""What the CIR and correlation plot stage (dabx_set_cir_mode; k_cir, k_cir_finish, k_cir_corr) costs, at bench.py's layout: --streams streams
x 18 sub-channels of 64 kbit/s, rings filled as bench.py fills them, primed for 40 frames.  Front-end + MSC frames/s and time per step
without a delivery, in the order --order gives:

  off        the mode off on every stream (the stage exists from the first `on` leg: nothing is launched for it)
  cir1       the CIR on for 1 stream          cir        the CIR on for all streams
  both1      CIR and correlation plot, 1      both       CIR and correlation plot on for all streams

One JSON line per leg; a fresh process per run.  The rings are committed a frame per step, so a stream's 385 rows fall due in two steps out
of six (381 + 4); the streams are switched on together and their windows coincide: the all-streams legs show the spike, the mean is a
sixth of it.  (A zero-copy commit puts the write horizon at ~0: a row counts as trusted only while the receiver has not read it.)

  python3 tools/bench_cir.py --order off,cir,both,both,cir,off
  python3 tools/bench_cir.py --streams 32"""
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
    ap.add_argument("--order", default="off,cir1,cir,both1,both,both,both1,cir,cir1,off")
    ap.add_argument("--chunks", type=int, default=12, help="timed 7-frame calls per leg (12: 84 steps, 14 windows per stream)")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    S = a.streams
    subch = ds.default_subchannels(18, 64)
    eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=18, out_frames=8)
    eng.set_subchannels(subch)
    args = types.SimpleNamespace(ensembles=4, snr=20.0, streams=S, unlocked=0, unlocked_kind="silence", layout="uniform")
    ring_frames = bench.fill_rings(eng, torch, dev, args, 0, subch)

    def step(n):
        for m in bench.region_chunks(n, 7, False):
            eng.commit(m * TF)
            eng.process(m, sync=False)

    def mode(name):
        eng.set_cir_mode(-1, enable=False)
        if name != "off":
            eng.set_cir_mode(0 if name.endswith("1") else -1, cir=True, correlation=name.startswith("both"))

    def totals():
        st = [eng.cir_stats(s) for s in range(0, S, max(1, S // 8))]
        return [sum(x["shows"][k] for x in st) for k in (0, 1)] + [sum(x["rows_untrusted"] for x in st), st[0]["launches"]]

    eng.commit(ring_frames * TF - TF)
    step(40)
    eng.synchronize()
    locked = sum(eng.stats(s)["state"] == 2 for s in range(S))
    for name in a.order.split(","):
        mode(name)
        step(21)
        eng.synchronize()
        f0, t0s = eng.counters()["frames"], totals()
        t0 = time.perf_counter()
        step(7 * a.chunks)
        eng.synchronize()
        dt = time.perf_counter() - t0
        t1s = totals()
        print(json.dumps({"what": name, "streams": S, "locked": locked, "steps": 7 * a.chunks, "frames_per_s": (eng.counters()["frames"] - f0) / dt,
                          "ms_per_step": 1e3 * dt / (7 * a.chunks), "cir_records_sampled": t1s[0] - t0s[0], "corr_records_sampled": t1s[1] - t0s[1],
                          "rows_untrusted_sampled": t1s[2] - t0s[2], "stage_launch_steps": t1s[3] - t0s[3]}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
