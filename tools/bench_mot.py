#!/usr/bin/env python3
"""What the MOT stage (k_mot) costs per batch beside k_pad of the same run, from dabx_get_profile with every kernel stand-alone
(dabx_set_profiling -1).  Two engines, both fed noise-free coded soft bits through dabx_internal_msc_inject / _decode, every batch of 28
CIFs profiled:

  stage   the engine of tests/test_gpu_mot_stage.py: two streams of tests/mot_cases.py's layout (MOT on the 64 and the 192 kbit/s slot)
  all     --streams streams x 12 sub-channels of 64 kbit/s, every slot a PAD slot with MOT on, carrying mot_cases' placement scenario

The last slot's objects are checked against the model.  One JSON line per engine.

  python3 tools/bench_mot.py [--streams 128]"""
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
import mot_cases as mc  # noqa: E402
import pad_cases as pc  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402

H, B = dc.HISTORY, dc.BATCH


def profile(eng):
    ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)(); names = (C.c_char_p * 16)()
    nk = dx.check(dx.load().dabx_get_profile(eng._h, ms, cnt, names))
    return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(nk)}


def run(name, S, layout, cifs, mot_slots, pkt_slots, check):
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=len(layout), out_frames=1)
    try:
        for s in range(S):
            eng.set_subchannels(layout, stream=s)
            for j, size in mot_slots.items():
                eng.set_pad_mode(s, j)
                eng.set_mot_mode(s, j, max_object_bytes=size)
            for j in pkt_slots:
                eng.set_packet_mode(s, j, mc.PACKET_ADDRESS)
        for s in range(S):
            dx.msc_inject(eng, s, cifs[s % len(cifs)][:H])
        dx.msc_decode(eng, [H] * S, H)
        dx.check(dx.load().dabx_set_profiling(eng._h, -1))
        for b in range(mc.N_BATCHES):
            for s in range(S):
                dx.msc_inject(eng, s, cifs[s % len(cifs)][H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B] * S, B)
        prof = profile(eng)
        s, j, m = check
        rec, by = eng.read_mot_objects(s, j, 256, max_bytes=1 << 18)
        want = m.records()[-len(rec):].copy()
        want["byte_pos"] -= want["byte_pos"][0]
        equal = len(rec) > 0 and rec.tobytes() == want.tobytes() and all(eng.mot_stats(s, j)[k] == m.counters[k] for k in dx.MOT_COUNTERS)
    finally:
        eng.close()
    n = mc.N_BATCHES
    assert prof["k_mot"][1] == prof["k_pad"][1] == n and equal, (prof, equal)
    mot, pad = prof["k_mot"][0] / n, prof["k_pad"][0] / n
    n_mot = S * len(mot_slots)
    print(json.dumps({"engine": name, "streams": S, "mot_slots": n_mot, "k_mot_ms_per_batch": mot, "k_pad_ms_per_batch": pad,
                      "us_per_slot_k_mot": 1e3 * mot / n_mot, "k_dabplus_ms_per_batch": prof["k_dabplus"][0] / n, "model_equal": equal}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    S = ap.parse_args().streams
    cases = [mc.stream_case(s) for s in range(mc.N_STREAMS)]
    o = cases[1][3][1]
    m = mc.mot_model_of(pc.run_model(o["sf"], o["sfi"]), mc.max_bytes_of(1))
    run("stage", mc.N_STREAMS, cases[0][0], [c[2] for c in cases], {0: mc.MAX_OBJECT_BYTES[0], 1: mc.MAX_OBJECT_BYTES[1]}, [4], (1, 1, m))
    M = 12
    layout = dc.dabplus_layout([(64, pc.PROT, 0)] * M, dab_plus=[1] * M)
    frames, sfs, sfi = mc.mot_frames(0, 0)
    cifs = dc.cifs_of(layout, [frames] * M, np.random.default_rng(6))
    m = mc.mot_model_of(pc.run_model(sfs, sfi), 65536)
    run("all", S, layout, [cifs], {j: 0 for j in range(M)}, [], (S - 1, M - 1, m))


if __name__ == "__main__":
    main()
