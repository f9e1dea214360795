#!/usr/bin/env python3
"""What the MP2 audio stage (dabx_set_mp2_audio_mode, k_mp2_audio) and its section of the bulk delivery (DABX_DELIVER_MP2_AUDIO) cost and
deliver: --streams streams x 18 sub-channels of 64 kbit/s, slots 0-1 in packet mode, slots 2-17 DAB audio slots with the mode on and the
tests' MP2 scenarios at 64 kbit/s.  k_mp2_audio has no row in the profile table (all 16 are taken), so its time comes from a
`rocprofv3 --kernel-trace --stats` run of its own, as k_tii's does.  One JSON line per figure.

  (default)         starts `rocprofv3 --kernel-trace --stats -- python tools/bench_mp2_audio.py --mode stage` as a fresh child process and reads
                    the kernel statistics: k_mp2_audio's and k_msc_vitT's time per batch of 28 CIFs in the same run, and the stage's time
                    against the multiply-adds of the frames it decoded -- 36 sub-blocks x 2 channels x (64 x 32 matrixing + 512 window taps)
                    = 184 320 per MP2 frame -- beside the int32 multiply-add rate of the device (CUs x 64 lanes x clock)
  --mode stage      the workload alone: noise-free coded soft bits through dabx_internal_msc_inject / _decode, five batches of 28 CIFs
                    behind the history; the last slot's records, PCM and counters are checked against the model
  --mode deliver    delivered frames/s and the slab size with what = FIB | MSC and with what = FIB | MSC | MP2_AUDIO, through IQ as bench.py
                    fills its rings, in the order --order gives, --chunks 7-frame chunks each, a consumer thread beside

  python3 tools/bench_mp2_audio.py [--streams 512]
  python3 tools/bench_mp2_audio.py --mode deliver --order base,audio,audio,base"""
import argparse
import csv
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

M, N_PKT, WARMUP, TIMED = 18, 2, 2, 3
MADS_PER_FRAME = 36 * 2 * (64 * 32 + 512)


def stage(S):
    import dabplus_cases as dc
    import mp2_audio_cases as ac
    import packet_cases as pkc
    import pad_cases as pc
    from dabstar_amd import lib as dx
    H, B = dc.HISTORY, dc.BATCH
    n = (WARMUP + TIMED) * B
    layout = dc.dabplus_layout([(64, pc.PROT, 0)] * M, dab_plus=[0] * M)
    frames = [pkc.scenario(64, 40 + j, n) for j in range(N_PKT)] + [ac.scenario(64, 50 + j, 3 + j, n)[0] for j in range(N_PKT, M)]
    cifs = dc.cifs_of(layout, frames, np.random.default_rng(5))
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=M, out_frames=1)
    try:
        for s in range(S):
            eng.set_subchannels(layout, stream=s)
        for s in range(S):
            for j in range(N_PKT):
                eng.set_packet_mode(s, j, pc.PACKET_ADDRESS)
        for s in range(S):
            dx.msc_inject(eng, s, cifs[:H])
        dx.msc_decode(eng, [H] * S, H)
        for s in range(S):                     # behind the 16 CIFs of history: every launch of the stage walks a full batch
            for j in range(N_PKT, M):
                eng.set_mp2_audio_mode(s, j)
        for b in range(WARMUP + TIMED):
            for s in range(S):
                dx.msc_inject(eng, s, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B] * S, B)
        st = eng.mp2_audio_stats(S - 1, M - 1)
        rec, by = eng.read_mp2_audio(S - 1, M - 1, 64)
        out = sum(eng.mp2_audio_stats(0, j)["frames_out"] for j in range(N_PKT, M))
    finally:
        eng.close()
    m = ac.run_model(64, frames[M - 1])
    k = len(rec)
    want = m.records()[-k:].copy()
    want["byte_pos"] -= want["byte_pos"][0]
    equal = all(st[f] == m.all_stats()[f] for f in ac.STAT_FIELDS) and rec.tobytes() == want.tobytes() and np.array_equal(by, m.all_pcm()[-len(by):])
    print(json.dumps({"mode": "stage", "streams": S, "audio_slots": (M - N_PKT) * S, "batches": WARMUP + TIMED, "launches": st["launches"],
                      "frames_out_per_stream": out, "model_equal": bool(equal)}))
    assert equal and st["launches"] == WARMUP + TIMED, st


def profile(S):
    """The stage workload as a child process under rocprofv3; the kernel statistics of that run."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "mp2", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--mode", "stage", "--streams", str(S)]
        child = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        line = [ln for ln in child.stdout.splitlines() if ln.startswith('{"mode": "stage"')]
        if child.returncode or not line:
            sys.exit("bench_mp2_audio.py: the profiled run failed (%d)\n%s\n%s" % (child.returncode, child.stdout[-2000:], child.stderr[-2000:]))
        run = json.loads(line[-1])
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                rows[r["Name"]] = r
    def of(prefix):
        hit = [r for name, r in rows.items() if name.startswith(prefix) or ("::" + prefix) in name]
        if not hit:
            sys.exit("bench_mp2_audio.py: no kernel %s in the statistics (%s)" % (prefix, sorted(rows)[:40]))
        return sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
    n_a, t_a = of("k_mp2_audio")
    n_v, t_v = of("k_msc_vitT")
    import torch
    p = torch.cuda.get_device_properties(0)
    clock_hz = 2.4e9                                                   # MI355X peak engine clock
    rate = p.multi_processor_count * 64 * clock_hz                     # one int32 multiply-add per lane and clock
    frames = run["frames_out_per_stream"] * S                          # MP2 frames decoded over all launches
    print(json.dumps({"mode": "profile", "streams": S, "audio_slots": run["audio_slots"], "k_mp2_audio_launches": n_a, "k_mp2_audio_ms_per_batch": t_a / n_a / 1e6,
                      "k_msc_vitT_launches": n_v, "k_msc_vitT_ms_per_batch": t_v / n_v / 1e6, "ratio_to_vitT": (t_a / n_a) / (t_v / n_v),
                      "mp2_frames_decoded": frames, "mads_per_frame": MADS_PER_FRAME, "mads_per_s": frames * MADS_PER_FRAME / (t_a / 1e9),
                      "device_mad_rate_per_s": rate, "fraction_of_mad_rate": frames * MADS_PER_FRAME / (t_a / 1e9) / rate, "model_equal": run["model_equal"]}))


class Sink(threading.Thread):
    """Takes every chunk as it lands, counts its frames and MP2 frames, gives the slab back."""

    def __init__(self, eng):
        super().__init__(daemon=True)
        self.eng, self.stop, self.error = eng, threading.Event(), None
        self.chunks = self.frames = self.mp2_frames = self.lost = 0
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
                if ch.mp2_audio_table is not None:
                    self.mp2_frames += int(ch.mp2_audio_table["n_frames"].sum())
                    self.lost += int(ch.mp2_audio_table["frames_lost"].sum())
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
    import mp2_audio_cases as ac
    import torch
    from dabstar_amd import lib as dx
    from tools import dab_synth as ds
    TF = bench.TF
    dev = torch.device("cuda:0")
    subch = [ds.SubCh(j, 48 * j, 48, 64, 2, 0, dab_plus=0) for j in range(M)]
    eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=M, out_frames=8)
    eng.set_subchannels(subch)
    args = types.SimpleNamespace(ensembles=4, snr=20.0, streams=S, unlocked=0, unlocked_kind="silence", layout="uniform")
    for e in range(args.ensembles):            # bench.fill_rings takes its clean ensembles from this cache: here the audio slots carry MP2 frames
        pay = {j: ac.scenario(64, 100 * e + j, 3 + j, 40)[0] for j in range(N_PKT, M)}
        bench._BASE_IQ[(0, e, "uniform")] = ds.build_ensemble(10, subch, seed=e, cyclic=True, payloads=pay).iq
    ring_frames = bench.fill_rings(eng, torch, dev, args, 0, subch)
    sink = None
    closed = [0]

    def step(n):
        for m in bench.region_chunks(n, 7, False):
            if sink is not None:
                k = (m + 6) // 7
                while eng.delivery_wait_free(k, timeout_ms=2000) < k:
                    if sink.error is not None or not sink.is_alive():
                        raise SystemExit("bench_mp2_audio.py: the consumer died: %r" % (sink.error,))
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
    for s in range(S):
        for j in range(N_PKT):
            eng.set_packet_mode(s, j, 0x155)
    for name in order.split(","):
        audio = name == "audio"
        for s in range(S):
            for j in range(N_PKT, M):
                eng.set_mp2_audio_mode(s, j, on=audio)
        eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_MSC | (dx.DELIVER_MP2_AUDIO if audio else 0))
        slab = eng.delivery_slab_bytes()
        sink = Sink(eng)
        closed[0] = 0
        step(21)
        drain()
        f0, a0, l0 = eng.counters()["frames"], sink.mp2_frames, eng.mp2_audio_stats(0, M - 1)["launches"]
        t0 = time.perf_counter()
        step(7 * chunks)
        drain()
        dt = time.perf_counter() - t0
        frames = eng.counters()["frames"] - f0
        eng.synchronize()
        sink.finish()
        print(json.dumps({"mode": "deliver", "what": name, "streams": S, "locked": locked, "chunks": chunks, "frames_per_s": frames / dt, "slab_bytes": slab,
                          "mp2_frames_delivered": sink.mp2_frames - a0, "pcm_bytes_per_s": (sink.mp2_frames - a0) * 4608 / dt, "lost": sink.lost,
                          "k_mp2_audio_launches": eng.mp2_audio_stats(0, M - 1)["launches"] - l0}))
        eng.delivery_close()
        sink = None
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--mode", choices=["profile", "stage", "deliver"], default="profile")
    ap.add_argument("--order", default="base,audio,audio,base")
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
