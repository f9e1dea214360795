#!/usr/bin/env python3
"""What the MP2 PAD walk (k_pad_mp2) costs per slot and batch beside k_packet of the same run: 512 streams x 18 sub-channels of 64 kbit/s,
slots 0-1 in packet mode with the tests' 64 kbit/s packet scenario, slots 2-17 DAB audio slots with PAD decoding from their MP2 frames and
the tests' MP2 scenarios at 64 kbit/s (both frame plans, alternating).  Noise-free coded soft bits through dabx_internal_msc_inject /
_decode, two warm-up batches of 28 CIFs, then three profiled batches (dabx_set_profiling -1: every kernel stand-alone); the figures are
dabx_get_profile's entries k_packet and k_pad (the marker k_pad_mp2 runs in; there is no DAB+ PAD slot here).  Both kernels stage and
walk every logical frame of their slots, one wave per slot.  The last slot's counters and sync state are checked against the model.
One JSON line.

  python3 tools/bench_mp2_pad.py [--streams 512]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import dabplus_cases as dc  # noqa: E402
import mp2_pad_cases as mc  # noqa: E402
import packet_cases as pkc  # noqa: E402
import pad_cases as pc  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402

M, N_PKT, WARMUP, TIMED = 18, 2, 2, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    S = ap.parse_args().streams
    H, B = dc.HISTORY, dc.BATCH
    n = (WARMUP + TIMED) * B
    layout = dc.dabplus_layout([(64, pc.PROT, 0)] * M, dab_plus=[0] * M)
    frames = [pkc.scenario(64, 40 + j, n) for j in range(N_PKT)] + [mc.scenario(64, 50 + j, j % 2)[0][:n] for j in range(N_PKT, M)]
    cifs = dc.cifs_of(layout, frames, np.random.default_rng(5))
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=M, out_frames=1)
    try:
        for s in range(S):
            eng.set_subchannels(layout, stream=s)
        for s in range(S):
            for j in range(M):
                if j < N_PKT:
                    eng.set_packet_mode(s, j, pc.PACKET_ADDRESS)
                else:
                    eng.set_pad_mode(s, j, source="mp2")
        for s in range(S):
            dx.msc_inject(eng, s, cifs[:H])
        dx.msc_decode(eng, [H] * S, H)
        for b in range(WARMUP + TIMED):
            if b == WARMUP:
                dx.check(dx.load().dabx_set_profiling(eng._h, -1))
            for s in range(S):
                dx.msc_inject(eng, s, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B] * S, B)
        ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)(); names = (C.c_char_p * 16)()
        nk = dx.check(dx.load().dabx_get_profile(eng._h, ms, cnt, names))
        prof = {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(nk)}
        st, sy = eng.pad_stats(S - 1, M - 1), eng.mp2_sync_stats(S - 1, M - 1)
        m = mc.run_model(64, frames[M - 1])
        equal = all(st[k] == m.pad.counters[k] for k in pc.PAD_COUNTERS) and sy == m.sync_stats()
    finally:
        eng.close()
    assert prof["k_packet"][1] == prof["k_pad"][1] == TIMED and equal, (prof, st, sy)
    pkt, mp2 = prof["k_packet"][0] / TIMED, prof["k_pad"][0] / TIMED
    print(json.dumps({"streams": S, "k_packet_ms_per_launch": pkt, "k_pad_mp2_ms_per_launch": mp2, "packet_slots": N_PKT * S, "mp2_slots": (M - N_PKT) * S,
                      "us_per_slot_k_packet": 1e3 * pkt / (N_PKT * S), "us_per_slot_k_pad_mp2": 1e3 * mp2 / ((M - N_PKT) * S),
                      "ratio_per_slot": (mp2 / ((M - N_PKT) * S)) / (pkt / (N_PKT * S)), "model_equal": equal}))


if __name__ == "__main__":
    main()
