#!/usr/bin/env python3
"""What the AAC stream stage (dabx_set_aac_stream_mode, k_aac_stream) and its section of the bulk delivery (DABX_DELIVER_AAC) cost and
deliver: --streams streams x 18 DAB+ sub-channels of 64 kbit/s with the mode on, carrying the tests' scenarios.  k_aac_stream has no row in
the profile table (all 16 are taken), so its time comes from a `rocprofv3 --kernel-trace --stats` run of its own, as k_mp2_audio's does.
One JSON line per figure.

  (default)         starts `rocprofv3 --kernel-trace --stats -- python tools/bench_aac_stream.py --mode stage` as a fresh child process and
                    reads the kernel statistics: the time per batch of 28 CIFs of k_aac_stream beside k_dabplus and k_msc_vitT of the same
                    run -- the comparison that decides between a byte and a dword per lane (docs/history/aac_stream.md)
  --mode stage      the workload alone: noise-free coded soft bits through dabx_internal_msc_inject / _decode, five batches of 28 CIFs
                    behind the history; the last slot's records, bytes and counters are checked against the model.  Then the host walk
                    the stage replaces: one host thread builds the LOAS frames of one slot's newest super frames from
                    read_superframes + read_superframe_info through dabx_internal_aac_frame_host
  --mode deliver    delivered frames/s and the slab size with what = FIB | SF, FIB | SF | AAC and FIB | AAC, through IQ as bench.py fills its
                    rings, in the order --order gives, --chunks 7-frame chunks each, a consumer thread beside

  python3 tools/bench_aac_stream.py [--streams 512]
  python3 tools/bench_aac_stream.py --mode deliver --order sf,sf+aac,aac,sf"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import threading
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

M, WARMUP, TIMED = 18, 2, 3


def host_walk(dx, sfs, sfis, repeat=20):
    """(LOAS bytes per second, access units per second) of one host thread that builds the frames of these super frames."""
    L = dx.load()
    out = np.zeros(dx.AAC_MAX_FRAME_BYTES, np.uint8)
    jobs = []
    for sf, r in zip(sfs, sfis):
        sf = np.ascontiguousarray(sf)
        for a in range(int(r["num_aus"])):
            if (int(r["au_crc_ok"]) & ~int(r["au_len_bad"])) >> a & 1:
                st = int(r["au_start"][a])
                jobs.append((sf.ctypes.data + st, int(r["au_start"][a + 1]) - st - 2, int(r["stream_parms"]), sf))
    call, dst = L.dabx_internal_aac_frame_host, out.ctypes.data
    t0 = time.perf_counter()
    n = 0
    for _ in range(repeat):
        for p, ln, parms, _ in jobs:
            n += call(p, ln, parms, dst)
    dt = time.perf_counter() - t0
    return n / dt, repeat * len(jobs) / dt


def stage(S):
    import aac_stream_cases as ac
    import dabplus_cases as dc
    from dabstar_amd import lib as dx
    H, B = dc.HISTORY, dc.BATCH
    n = (WARMUP + TIMED) * B
    layout = dc.dabplus_layout([(64, ac.PROT, 0)] * M)
    frames = [ac.scenario(64, 50 + j, False, n)[0] for j in range(M)]
    cifs = dc.cifs_of(layout, frames, np.random.default_rng(5))
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=M, out_frames=1)
    try:
        for s in range(S):
            eng.set_subchannels(layout, stream=s)
        for s in range(S):
            for j in range(M):
                eng.set_aac_stream_mode(s, j)
        for s in range(S):
            dx.msc_inject(eng, s, cifs[:H])
        dx.msc_decode(eng, [H] * S, H)
        taken = []
        for b in range(WARMUP + TIMED):
            for s in range(S):
                dx.msc_inject(eng, s, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B] * S, B)
            k = eng.subch_stats(S - 1, M - 1)["sf_count"] - sum(len(t[1]) for t in taken)
            if k:
                eng.subch = list(layout)
                taken.append((eng.read_superframes(S - 1, M - 1, k), eng.read_superframe_info(S - 1, M - 1, k)))
        st = eng.aac_stream_stats(S - 1, M - 1)
        rec, by = eng.read_aac_frames(S - 1, M - 1, 128)
        out_bytes = sum(eng.aac_stream_stats(0, j)["frame_bytes"] for j in range(M))
    finally:
        eng.close()
    sfs, sfis = np.concatenate([t[0] for t in taken]), np.concatenate([t[1] for t in taken])
    m = ac.run_model(sfs, sfis)
    k = len(rec)
    want = m.records()[-k:].copy()
    want["byte_pos"] -= want["byte_pos"][0]
    equal = k > 0 and all(st[f] == m.counters[f] for f in ac.COUNTERS) and rec.tobytes() == want.tobytes() and np.array_equal(by, m.all_bytes()[-len(by):])
    host_bytes, host_aus = host_walk(dx, sfs, sfis)
    print(json.dumps({"mode": "stage", "streams": S, "aac_slots": M * S, "batches": WARMUP + TIMED, "launches": st["launches"], "super_frames_last_slot": len(sfs),
                      "loas_bytes_per_stream": out_bytes, "model_equal": bool(equal), "host_walk_loas_bytes_per_s": host_bytes, "host_walk_aus_per_s": host_aus}))
    assert equal and st["launches"] == WARMUP + TIMED + 1, st


def profile(S):
    """The stage workload as a child process under rocprofv3; the kernel statistics of that run."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "aac", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--mode", "stage", "--streams", str(S)]
        child = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        line = [ln for ln in child.stdout.splitlines() if ln.startswith('{"mode": "stage"')]
        if child.returncode or not line:
            sys.exit("bench_aac_stream.py: the profiled run failed (%d)\n%s\n%s" % (child.returncode, child.stdout[-2000:], child.stderr[-2000:]))
        run = json.loads(line[-1])
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                rows[r["Name"]] = r

    def of(prefix):
        hit = [r for name, r in rows.items() if name.startswith(prefix) or ("::" + prefix) in name]
        if not hit:
            sys.exit("bench_aac_stream.py: no kernel %s in the statistics (%s)" % (prefix, sorted(rows)[:40]))
        return sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
    n_a, t_a = of("k_aac_stream")
    n_d, t_d = of("k_dabplus")
    n_v, t_v = of("k_msc_vitT")
    loas = run["loas_bytes_per_stream"] * S
    print(json.dumps({"mode": "profile", "streams": S, "aac_slots": run["aac_slots"], "k_aac_stream_launches": n_a, "k_aac_stream_ms_per_batch": t_a / n_a / 1e6,
                      "k_dabplus_launches": n_d, "k_dabplus_ms_per_batch": t_d / n_d / 1e6, "k_msc_vitT_launches": n_v, "k_msc_vitT_ms_per_batch": t_v / n_v / 1e6,
                      "ratio_to_dabplus": (t_a / n_a) / (t_d / n_d), "loas_bytes": loas, "loas_bytes_per_s_of_kernel_time": loas / (t_a / 1e9),
                      "host_walk_loas_bytes_per_s": run["host_walk_loas_bytes_per_s"], "model_equal": run["model_equal"]}))


class Sink(threading.Thread):
    """Takes every chunk as it lands, counts its frames and LOAS frames, gives the slab back."""

    def __init__(self, eng):
        super().__init__(daemon=True)
        self.eng, self.stop, self.error = eng, threading.Event(), None
        self.chunks = self.frames = self.records = self.loas_bytes = self.lost = 0
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
                if ch.aac_table is not None:
                    self.records += int(ch.aac_table["n_frames"].sum())
                    self.loas_bytes += int(ch.aac_table["n_bytes"].sum())
                    self.lost += int(ch.aac_table["frames_lost"].sum())
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


def deliver(S, order, chunks):
    import bench
    import torch
    from dabstar_amd import lib as dx
    from tools import dab_synth as ds
    TF = bench.TF
    dev = torch.device("cuda:0")
    subch = [ds.SubCh(j, 48 * j, 48, 64, 2, 0) for j in range(M)]
    eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=M, out_frames=8)
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
                        raise SystemExit("bench_aac_stream.py: the consumer died: %r" % (sink.error,))
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
    masks = {"sf": dx.DELIVER_FIB | dx.DELIVER_SF, "sf+aac": dx.DELIVER_FIB | dx.DELIVER_SF | dx.DELIVER_AAC, "aac": dx.DELIVER_FIB | dx.DELIVER_AAC}
    for name in order.split(","):
        aac = "aac" in name
        for s in range(S):
            for j in range(M):
                eng.set_aac_stream_mode(s, j, on=aac)
        eng.delivery_open(slots=4, what=masks[name])
        slab = eng.delivery_slab_bytes()
        sink = Sink(eng)
        closed[0] = 0
        step(21)
        drain()
        f0, a0, b0, l0 = eng.counters()["frames"], sink.records, sink.loas_bytes, eng.aac_stream_stats(0, M - 1)["launches"]
        t0 = time.perf_counter()
        step(7 * chunks)
        drain()
        dt = time.perf_counter() - t0
        frames = eng.counters()["frames"] - f0
        eng.synchronize()
        sink.finish()
        print(json.dumps({"mode": "deliver", "what": name, "streams": S, "locked": locked, "chunks": chunks, "frames_per_s": frames / dt, "slab_bytes": slab,
                          "records_delivered": sink.records - a0, "loas_bytes_per_s": (sink.loas_bytes - b0) / dt, "lost": sink.lost,
                          "k_aac_stream_launches": eng.aac_stream_stats(0, M - 1)["launches"] - l0}))
        eng.delivery_close()
        sink = None
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--mode", choices=["profile", "stage", "deliver"], default="profile")
    ap.add_argument("--order", default="sf,sf+aac,aac,sf")
    ap.add_argument("--chunks", type=int, default=14)
    a = ap.parse_args()
    if a.mode == "stage":
        stage(a.streams)
    elif a.mode == "deliver":
        deliver(a.streams, a.order, a.chunks)
    else:
        profile(a.streams)


if __name__ == "__main__":
    main()
