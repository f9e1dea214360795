#!/usr/bin/env python3
"""What the IQ scope on the device (dabx_set_scope_mode, k_scope) and its section of the bulk delivery (DABX_DELIVER_SCOPE, k_deliver_records)
cost, at bench.py's layout: --streams streams x 18 sub-channels of 64 kbit/s, rings filled as bench.py fills them, primed for 40 frames.
One JSON line per figure; a fresh process per run.

  --mode rate       front-end + MSC frames/s without a delivery, with the mode off, on for 1 stream and on for all streams, in the order
                    --order gives (off,one,all,...), at --symbol (default 75: the longest replay; 0 = the reference's cadence).  Run the same
                    mode under `rocprofv3 --kernel-trace --stats` for k_scope's time per launch beside k_demap_frame6's and k_demap_fic's:
                    k_scope has no row in the profile table.
  --mode deliver    delivered frames/s with what = FIB | MSC and with what = FIB | MSC | SCOPE (mode on for --scope-streams streams), in the
                    order --order gives (fibmsc,scope,...), --chunks 7-frame chunks each, a consumer thread beside

  python3 tools/bench_scope.py --mode rate --order off,one,all,all,one,off"""
import argparse
import json
import os
import sys
import threading
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402
from tools import dab_synth as ds  # noqa: E402

TF = bench.TF


class Sink(threading.Thread):
    """Takes every chunk as it lands, counts its frames and scope records, gives the slab back."""

    def __init__(self, eng):
        super().__init__(daemon=True)
        self.eng, self.stop, self.error = eng, threading.Event(), None
        self.chunks = self.frames = self.records = self.lost = 0
        self.start()

    def run(self):
        try:
            while True:
                ch = self.eng.delivery_next(wait=True)
                if ch is None:
                    if self.stop.is_set():
                        return
                    time.sleep(0.0002)
                    continue
                if ch.scope_table is not None:
                    self.records += int(ch.scope_table["n_records"].sum())
                    self.lost += int(ch.scope_table["records_lost"].sum())
                self.frames += int(ch.streams["n_frames"].sum())
                self.lost += int(ch.streams["frames_lost"].sum())
                ch.release()
                self.chunks += 1
        except Exception as ex:
            self.error = ex

    def finish(self):
        self.stop.set()
        self.join(60)
        if self.error is not None:
            raise self.error


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--mode", choices=["rate", "deliver"], default="rate")
    ap.add_argument("--order", default=None)
    ap.add_argument("--symbol", type=int, default=75)
    ap.add_argument("--scope-streams", type=int, default=8)
    ap.add_argument("--chunks", type=int, default=14)
    a = ap.parse_args()
    order = (a.order or ("off,one,all,all,one,off" if a.mode == "rate" else "fibmsc,scope,scope,fibmsc")).split(",")
    import torch
    dev = torch.device("cuda:0")
    S = a.streams
    subch = ds.default_subchannels(18, 64)
    eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=18, out_frames=8)
    eng.set_subchannels(subch)
    args = types.SimpleNamespace(ensembles=4, snr=20.0, streams=S, unlocked=0, unlocked_kind="silence", layout="uniform")
    ring_frames = bench.fill_rings(eng, torch, dev, args, 0, subch)
    sink = None
    closed = [0]

    def step(n):
        for m in bench.region_chunks(n, 7, False):
            if sink is not None:
                k = (m + 6) // 7
                while eng.delivery_wait_free(k, timeout_ms=2000) < k:
                    if sink.error is not None or not sink.is_alive():
                        raise SystemExit("bench_scope.py: the consumer died: %r" % (sink.error,))
                closed[0] += k
            eng.commit(m * TF)
            eng.process(m, sync=False)

    def drain():
        eng.synchronize()
        while sink is not None and sink.chunks < closed[0] and sink.error is None:
            time.sleep(0.00002)

    def scope(n_on):
        eng.set_scope_mode(-1, enable=False)
        for s in ([-1] if n_on == S else [k * (S // n_on) for k in range(n_on)]):
            eng.set_scope_mode(s, iq_type=0, carrier_type=8, symbol=a.symbol)       # REL_POWER: the plot with the prefix scan

    eng.commit(ring_frames * TF - TF)
    step(40)
    eng.synchronize()
    locked = sum(eng.stats(s)["state"] == 2 for s in range(S))
    if a.mode == "rate":
        for name in order:
            scope({"off": 0, "one": 1, "all": S}[name])
            step(21)
            eng.synchronize()
            f0, l0, n0 = eng.counters()["frames"], eng.scope_stats(0)["launches"], sum(eng.scope_stats(s)["shows"] for s in range(0, S, max(1, S // 8)))
            t0 = time.perf_counter()
            step(7 * a.chunks)
            eng.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"mode": "rate", "what": name, "streams": S, "locked": locked, "symbol": a.symbol, "frames_per_s": (eng.counters()["frames"] - f0) / dt,
                              "k_scope_launches": eng.scope_stats(0)["launches"] - l0,
                              "shows_sampled": sum(eng.scope_stats(s)["shows"] for s in range(0, S, max(1, S // 8))) - n0}))
    else:
        for name in order:
            on = name == "scope"
            scope(min(a.scope_streams, S) if on else 0)
            eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_MSC | (dx.DELIVER_SCOPE if on else 0))
            slab = eng.delivery_slab_bytes()
            sink = Sink(eng)
            closed[0] = 0
            step(21)
            drain()
            f0, r0 = eng.counters()["frames"], sink.records
            t0 = time.perf_counter()
            step(7 * a.chunks)
            drain()
            dt = time.perf_counter() - t0
            frames = eng.counters()["frames"] - f0
            eng.synchronize()
            sink.finish()
            print(json.dumps({"mode": "deliver", "what": name, "streams": S, "locked": locked, "symbol": a.symbol, "scope_streams": a.scope_streams if on else 0,
                              "chunks": a.chunks, "frames_per_s": frames / dt, "slab_bytes": slab, "scope_records": sink.records - r0, "lost": sink.lost}))
            eng.delivery_close()
            sink = None
    eng.close()


if __name__ == "__main__":
    main()
