#!/usr/bin/env python3
"""What the ETI stage of the bulk delivery (DABX_DELIVER_ETI, k_eti) costs and delivers, at bench.py's layout: --streams streams x 18
sub-channels of 64 kbit/s, rings filled as bench.py fills them, primed for 40 frames.  One JSON line per figure; a fresh process per run.

  --mode kernel     k_eti in ms per 7-frame batch from dabx_get_profile with every kernel stand-alone (dabx_set_profiling -1), with the
                    bytes the stage moves per batch.  (Run the same mode under `rocprofv3 --kernel-trace --stats` to set k_eti_rows
                    beside k_deliver_lf, which has no marker of its own: what = ETI | MSC launches both.)
  --mode deliver    delivered frames/s with what = ETI and with what = FIB | MSC (the same information, what the library could deliver
                    before), in the order --order gives, --chunks 7-frame chunks each, a consumer thread beside
  --mode perstream  the loop over dabx_read_eti for all streams after a 7-frame call, without a delivery: seconds per chunk

  python3 tools/bench_eti.py --mode deliver --order eti,fibmsc"""
import argparse
import ctypes as C
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


def profile(eng):
    ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)(); names = (C.c_char_p * 16)()
    nk = dx.check(dx.load().dabx_get_profile(eng._h, ms, cnt, names))
    return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(nk)}


class Sink(threading.Thread):
    """Takes every chunk as it lands, adds up its ETI rows and logical frames, gives the slab back."""

    def __init__(self, eng):
        super().__init__(daemon=True)
        self.eng, self.stop, self.error = eng, threading.Event(), None
        self.chunks = self.rows = self.cifs = self.frames = self.lost = 0
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
                if ch.eti_table is not None:
                    self.rows += int(ch.eti_table["n_eti"].sum())
                    self.lost += int(ch.eti_table["cifs_lost"].sum()) + int(ch.eti_table["cifs_refused"].sum())
                self.cifs += int(ch.subch["n_cifs"].sum())
                self.frames += int(ch.streams["n_frames"].sum())
                self.lost += int(ch.streams["frames_lost"].sum()) + int(ch.subch["cifs_lost"].sum())
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
    ap.add_argument("--mode", choices=["kernel", "deliver", "perstream"], default="kernel")
    ap.add_argument("--order", default="eti,fibmsc")
    ap.add_argument("--chunks", type=int, default=14)
    a = ap.parse_args()
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
                        raise SystemExit("bench_eti.py: the consumer died: %r" % (sink.error,))
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
    whats = {"eti": dx.DELIVER_ETI, "fibmsc": dx.DELIVER_FIB | dx.DELIVER_MSC}
    if a.mode == "kernel":
        eng.delivery_open(slots=4, what=dx.DELIVER_ETI | dx.DELIVER_MSC)
        sink = Sink(eng)
        step(21)
        drain()
        dx.check(dx.load().dabx_set_profiling(eng._h, -1))
        profile(eng)
        rows0 = sink.rows
        step(7 * a.chunks)
        drain()
        p = profile(eng)
        dx.check(dx.load().dabx_set_profiling(eng._h, 0))
        rows = sink.rows - rows0
        ms = p["k_eti"][0] / a.chunks
        read_b, write_b = rows / a.chunks * (96 + 18 * 192), rows / a.chunks * 6144
        assert p["k_eti"][1] == 2 * a.chunks and rows == S * 28 * a.chunks and sink.lost == 0, (p["k_eti"], rows, sink.lost)
        print(json.dumps({"mode": "kernel", "streams": S, "locked": locked, "k_eti_ms_per_batch": ms, "launch_markers_per_batch": 2,
                          "rows_per_batch": rows // a.chunks, "payload_bytes_read_per_batch": read_b, "row_bytes_written_per_batch": write_b,
                          "GBps_read_plus_written": (read_b + write_b) / ms / 1e6,
                          "others_ms_per_batch": {k: v[0] / a.chunks for k, v in p.items() if v[1] and k != "k_eti"}}))
    elif a.mode == "deliver":
        for name in a.order.split(","):
            eng.delivery_open(slots=4, what=whats[name])
            slab = eng.delivery_slab_bytes()
            sink = Sink(eng)
            closed[0] = 0
            step(21)
            drain()
            f0, r0, c0 = eng.counters()["frames"], sink.rows, sink.cifs
            t0 = time.perf_counter()
            step(7 * a.chunks)
            drain()
            dt = time.perf_counter() - t0
            frames = eng.counters()["frames"] - f0
            eng.synchronize()
            sink.finish()
            info = eng.delivery_info()
            print(json.dumps({"mode": "deliver", "what": name, "streams": S, "locked": locked, "chunks": a.chunks, "frames_per_s": frames / dt,
                              "slab_bytes": slab, "host_GBps": slab * a.chunks / dt / 1e9, "eti_rows": sink.rows - r0, "logical_frames": sink.cifs - c0,
                              "lost": sink.lost, "link_GBps_copier": info["bytes_copied"] / info["copy_seconds"] / 1e9}))
            eng.delivery_close()
            sink = None
    else:
        for i in range(2):
            step(7)
            eng.synchronize()
            t0 = time.perf_counter()
            n = 0
            for s in range(S):
                f, lost = eng.read_eti(s, 64)
                n += len(f)
            dt = time.perf_counter() - t0
            print(json.dumps({"mode": "perstream", "streams": S, "locked": locked, "chunk": i, "eti_frames": n, "seconds_per_7_frame_chunk": dt,
                              "frames_per_s_of_this_loop_alone": S * 7 / dt}))
    eng.close()


if __name__ == "__main__":
    main()
