#!/usr/bin/env python3
"""What the carousel stage (k_carousel) costs per batch beside k_packet of the same run, from dabx_get_profile with every kernel
stand-alone (dabx_set_profiling -1).  Two engines, both fed noise-free coded soft bits through dabx_internal_msc_inject / _decode, every
batch of 28 CIFs profiled:

  stage   the engine of tests/test_gpu_carousel_stage.py: two streams of tests/carousel_cases.py's layout (carousel slots at 64 and 384
          kbit/s, a packet slot without, a PAD slot with MOT, a plain slot)
  all     --streams streams x 12 sub-channels of 64 kbit/s, every slot a carousel slot carrying carousel_cases' header-mode scenario

The last slot's objects are checked against the model.  One JSON line per engine.

  python3 tools/bench_carousel.py [--streams 128]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import carousel_cases as cc  # noqa: E402
import dabplus_cases as dc  # noqa: E402
import packet_cases as pkc  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402

H, B = dc.HISTORY, dc.BATCH


def profile(eng):
    ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)(); names = (C.c_char_p * 16)()
    nk = dx.check(dx.load().dabx_get_profile(eng._h, ms, cnt, names))
    return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(nk)}


def run(name, S, layout, cifs, car_slots, pkt_slots, mot_slots, check):
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=len(layout), out_frames=1)
    try:
        for s in range(S):
            eng.set_subchannels(layout, stream=s)
            for j in list(car_slots) + list(pkt_slots):
                eng.set_packet_mode(s, j, cc.ADDRESS)
            for j, cfg in car_slots.items():
                eng.set_carousel_mode(s, j, **cfg)
            for j in mot_slots:
                eng.set_pad_mode(s, j)
                eng.set_mot_mode(s, j)
        for s in range(S):
            dx.msc_inject(eng, s, cifs[s % len(cifs)][:H])
        dx.msc_decode(eng, [H] * S, H)
        dx.check(dx.load().dabx_set_profiling(eng._h, -1))
        for b in range(cc.N_BATCHES):
            for s in range(S):
                dx.msc_inject(eng, s, cifs[s % len(cifs)][H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B] * S, B)
        prof = profile(eng)
        s, j, m = check
        rec, by = eng.read_mot_objects(s, j, 256, max_bytes=1 << 18)
        want = m.records()[-len(rec):].copy()
        want["byte_pos"] -= want["byte_pos"][0]
        equal = len(rec) > 0 and rec.tobytes() == want.tobytes() and all(eng.carousel_stats(s, j)[k] == m.counters[k] for k in dx.CAROUSEL_COUNTERS)
    finally:
        eng.close()
    n = cc.N_BATCHES
    assert prof["k_carousel"][1] == prof["k_packet"][1] == n and equal, (prof, equal)
    car, pkt = prof["k_carousel"][0] / n, prof["k_packet"][0] / n
    n_car = S * len(car_slots)
    print(json.dumps({"engine": name, "streams": S, "carousel_slots": n_car, "k_carousel_ms_per_batch": car, "k_packet_ms_per_batch": pkt,
                      "us_per_slot_k_carousel": 1e3 * car / n_car, "k_dabplus_ms_per_batch": prof["k_dabplus"][0] / n, "model_equal": equal}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    S = ap.parse_args().streams
    cases = [cc.stream_case(s) for s in range(cc.N_STREAMS)]
    cfgs = {j: cc.SCENARIOS[cc.NAME_OF[j]][2] for j, (_, kind) in enumerate(cc.STAGE_LAYOUT) if kind == "car"}
    m = cc.model_of(pkc.run_model(cases[1][1][1], cc.ADDRESS), **cfgs[1])
    run("stage", cc.N_STREAMS, cases[0][0], [c[2] for c in cases], cfgs, [2], [3], (1, 1, m))
    M = 12
    layout = dc.dabplus_layout([(64, pkc.PROT, 0)] * M, dab_plus=[0] * M)
    kbps, groups, frames, cfg = cc.scenario("header", 0)
    cifs = dc.cifs_of(layout, [frames] * M, np.random.default_rng(6))
    m = cc.model_of(pkc.run_model(frames, cc.ADDRESS), **cfg)
    run("all", S, layout, [cifs], {j: cfg for j in range(M)}, [], [], (S - 1, M - 1, m))


if __name__ == "__main__":
    main()
