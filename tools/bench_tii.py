#!/usr/bin/env python3
"""What the TII detectors on the device (dabx_set_tii_mode, k_tii) and their section of the bulk delivery (DABX_DELIVER_TII, k_deliver_tii)
cost and deliver, at bench.py's layout: --streams streams x 18 sub-channels of 64 kbit/s, every synthetic ensemble with three TII
transmitters, rings filled as bench.py fills them, primed for 40 frames.  One JSON line per figure; a fresh process per run.

  --mode deliver    delivered frames/s with what = FIB | MSC and with what = FIB | MSC | TII (mode on for all streams, min_frames 5), in the
                    order --order gives (e.g. fibmsc,tii,fibmsc,tii,...), --chunks 7-frame chunks each, a consumer thread beside.  (Run the
                    same mode under `rocprofv3 --kernel-trace --stats` for k_tii's and k_deliver_tii's times: neither has a row in the
                    profile table.)
  --mode perstream  the path it replaces: the loop over dabx_read_tii for all streams after a 10-frame call, without a delivery
  --mode single     the single-ensemble frame rate (one stream, FIC only, the frame chain's latency) with the mode off and on, alternated

  python3 tools/bench_tii.py --mode deliver --order fibmsc,tii,tii,fibmsc,fibmsc,tii"""
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
TX = [[(3, 1, 1.0, True), (40, 17, 0.6, True), (69, 23, 0.3, True)], [(25, 9, 1.0, False), (7, 2, 0.7, True), (12, 5, 0.5, True)],
      [(10, 6, 1.0, True), (33, 6, 0.8, True), (50, 0, 0.4, True)], [(61, 15, 0.9, False), (20, 11, 0.6, True), (1, 22, 0.3, True)]]


class Sink(threading.Thread):
    """Takes every chunk as it lands, counts its frames, TII events and results, gives the slab back."""

    def __init__(self, eng):
        super().__init__(daemon=True)
        self.eng, self.stop, self.error = eng, threading.Event(), None
        self.chunks = self.frames = self.events = self.results = self.lost = 0
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
                if ch.tii_table is not None:
                    self.events += int(ch.tii_table["n_events"].sum())
                    self.lost += int(ch.tii_table["events_lost"].sum())
                    for s in range(0, len(ch.tii_table), 64):          # (a sample of the streams: the consumer is not what is measured)
                        self.results += sum(len(r) for _, r in ch.tii(s))
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
    ap.add_argument("--mode", choices=["deliver", "perstream", "single"], default="deliver")
    ap.add_argument("--order", default="fibmsc,tii,tii,fibmsc,fibmsc,tii")
    ap.add_argument("--chunks", type=int, default=14)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    single = a.mode == "single"
    S = 1 if single else a.streams
    subch = ds.default_subchannels(18, 64)
    eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=18, out_frames=8, fic_only=single)
    if not single:
        eng.set_subchannels(subch)
    args = types.SimpleNamespace(ensembles=4, snr=20.0, streams=S, unlocked=0, unlocked_kind="silence", layout="uniform")
    for e in range(args.ensembles):            # bench.fill_rings takes its clean ensembles from this cache: here they carry TII
        bench._BASE_IQ[(0, e, "uniform")] = ds.build_ensemble(10, subch, seed=e, cyclic=True, tii=TX[e]).iq
    ring_frames = bench.fill_rings(eng, torch, dev, args, 0, subch)
    sink = None
    closed = [0]

    def step(n):
        for m in bench.region_chunks(n, 7, False):
            if sink is not None:
                k = (m + 6) // 7
                while eng.delivery_wait_free(k, timeout_ms=2000) < k:
                    if sink.error is not None or not sink.is_alive():
                        raise SystemExit("bench_tii.py: the consumer died: %r" % (sink.error,))
                closed[0] += k
            eng.commit(m * TF)
            eng.process(m, sync=False)

    def drain():
        eng.synchronize()
        while sink is not None and sink.chunks < closed[0] and sink.error is None:
            time.sleep(0.00002)

    eng.commit(ring_frames * TF - TF)
    step(40)
    eng.synchronize()
    locked = sum(eng.stats(s)["state"] == 2 for s in range(S))
    if a.mode == "deliver":
        for name in a.order.split(","):
            tii = name == "tii"
            eng.set_tii_mode(-1, min_frames=5, threshold_db=8, enable=tii)
            eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_MSC | (dx.DELIVER_TII if tii else 0))
            slab = eng.delivery_slab_bytes()
            sink = Sink(eng)
            closed[0] = 0
            step(21)
            drain()
            f0, e0 = eng.counters()["frames"], sink.events
            l0 = eng.tii_stats(0)["launches"]
            t0 = time.perf_counter()
            step(7 * a.chunks)
            drain()
            dt = time.perf_counter() - t0
            frames = eng.counters()["frames"] - f0
            eng.synchronize()
            sink.finish()
            print(json.dumps({"mode": "deliver", "what": name, "streams": S, "locked": locked, "chunks": a.chunks, "frames_per_s": frames / dt,
                              "slab_bytes": slab, "tii_events": sink.events - e0, "tii_results_sampled": sink.results, "lost": sink.lost,
                              "k_tii_launches": eng.tii_stats(0)["launches"] - l0}))
            eng.delivery_close()
            sink = None
    elif a.mode == "perstream":
        for i in range(2):
            step(10)
            eng.synchronize()
            t0 = time.perf_counter()
            n = 0
            for s in range(S):
                res, k = eng.read_tii(s, min_frames=5, threshold_db=8)
                n += len(res)
            dt = time.perf_counter() - t0
            print(json.dumps({"mode": "perstream", "streams": S, "locked": locked, "call": i, "results": n, "seconds_per_10_frame_call": dt}))
    else:
        for name in a.order.split(","):
            eng.set_tii_mode(0, min_frames=5, threshold_db=8, enable=name == "tii")
            step(40)
            eng.synchronize()
            f0 = eng.counters()["frames"]
            t0 = time.perf_counter()
            step(7 * 4 * a.chunks)
            eng.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"mode": "single", "what": name, "locked": locked, "frames_per_s": (eng.counters()["frames"] - f0) / dt,
                              "tii_events": eng.tii_stats(0)["events"]}))
    eng.close()


if __name__ == "__main__":
    main()
