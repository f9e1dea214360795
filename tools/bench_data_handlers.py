#!/usr/bin/env python3
"""What the data handlers of packet-mode slots (k_data_handler) cost per batch beside k_packet of the same run: --streams streams x 12
packet-mode sub-channels of 64 kbit/s carrying the crafted and random groups of tests/data_handler_cases.py, every slot with a handler, a
third each (TDC, IP, Journaline), fed noise-free coded soft bits through dabx_internal_msc_inject / _decode.  One process, one JSON line:

  k_data_handler_ms   the kernel's own time per batch between two HIP events around its launch (dabx_internal_data_timing, as
                      tools/bench_fig_si.py times k_fig), every batch of the scenario, and their mean
  k_packet_ms         k_packet per batch of the same batches from dabx_get_profile with every instrumented kernel stand-alone
                      (dabx_set_profiling -1): the profile table's own event pairs

The last slot's items are checked against the model.  Run it in three fresh processes and read the three lines together.

  python3 tools/bench_data_handlers.py [--streams 128]"""
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
import data_handler_cases as dh  # noqa: E402
import packet_cases as pkc  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402

H, B = dc.HISTORY, dc.BATCH
M = 12


def profile(eng):
    ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)(); names = (C.c_char_p * 16)()
    nk = dx.check(dx.load().dabx_get_profile(eng._h, ms, cnt, names))
    return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(nk)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    S = ap.parse_args().streams
    kinds = [dh.HANDLERS[j % 3] for j in range(M)]
    layout = dc.dabplus_layout([(64, pkc.PROT, 0)] * M, dab_plus=[0] * M)
    frames = {k: dh.frames_of(64, dh.sequence(k) + dh.random_groups(k, 60), [11, i]) for i, k in enumerate(dh.HANDLERS)}
    cifs = dc.cifs_of(layout, [frames[k] for k in kinds], np.random.default_rng(6))
    model = dh.model_of(kinds[-1], pkc.run_model(frames[kinds[-1]], dh.ADDRESS))
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=M, out_frames=1)
    try:
        for s in range(S):
            eng.set_subchannels(layout, stream=s)
            for j in range(M):
                eng.set_packet_mode(s, j, dh.ADDRESS)
                eng.set_data_mode(s, j, kinds[j])
            dx.msc_inject(eng, s, cifs[:H])
        dx.msc_decode(eng, [H] * S, H)
        dx.check(dx.load().dabx_set_profiling(eng._h, -1))
        dx.data_timing(eng, True)
        for b in range(dh.N_BATCHES):
            for s in range(S):
                dx.msc_inject(eng, s, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B] * S, B)
        own = dx.data_timing(eng, False)
        prof = profile(eng)
        rec, by = eng.read_data_items(S - 1, M - 1, 256)
        st = eng.data_stats(S - 1, M - 1)
    finally:
        eng.close()
    want = model.records()[-len(rec):].copy()
    want["byte_pos"] -= want["byte_pos"][0] if len(want) else 0
    equal = len(rec) > 0 and rec.tobytes() == want.tobytes() and all(st[k] == model.counters[k] for k in dx.DATA_COUNTERS)
    assert equal and st["lost"] == 0 and len(own) == dh.N_BATCHES == prof["k_packet"][1], (st, len(own), prof["k_packet"])
    print(json.dumps({"streams": S, "handler_slots": S * M, "k_data_handler_ms": [round(float(v), 4) for v in own], "k_data_handler_ms_mean": float(own.mean()),
                      "k_packet_ms": prof["k_packet"][0] / prof["k_packet"][1], "ratio": float(own.mean()) / (prof["k_packet"][0] / prof["k_packet"][1]),
                      "model_equal": equal, "batches": dh.N_BATCHES}))


if __name__ == "__main__":
    main()
