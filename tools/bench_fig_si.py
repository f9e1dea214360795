#!/usr/bin/env python3
"""What following the service information on the device (dabx_fig_config.service_info; k_fig_si, k_fig_directory) costs, at bench.py's
layout: --streams streams x 18 sub-channels of 64 kbit/s, rings filled as bench.py fills them, primed for 40 frames.  One JSON line per
measurement; one process.

  legs       time per step and k_fig's own time per launch (between two HIP events) in up to three configurations, alternating in the order
             --order gives: "parent" (the library --parent names, e.g. the build of the commit before, FIG mode on: its k_fig), "off" (this
             library, FIG mode on, the switch off: k_fig) and "on" (the switch on for all streams: k_fig_si).  The spread between two legs
             of one kind is the noise a difference has to be read against.  Each library has an engine of its own, filled alike.
             The benchmark's FIC carries FIG 0/0 .. 0/2 only: "on" pays for bringing every stream's FigSiState into LDS and back, the SI
             walk itself finds nothing to do.
  directory  dabx_fig_directory(-1) -- one launch, one copy -- against what a host would do without it: the per-stream getters of every
             table for every stream (wall time of the loop) plus a join of them on the host (timed apart: it is Python here)

  python3 tools/bench_fig_si.py --parent /path/to/parent/libdabx.so
  python3 tools/bench_fig_si.py --streams 32 --order off,on,off,on"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402
from tools import dab_synth as ds  # noqa: E402

TF = bench.TF


def host_join(sub, pk, labels, gd, ua, lang, pty, fec):
    """what dabx_fig_directory joins, from the per-stream getters' answers, as far as they allow (they do not return the component table:
    a host would have to walk FIG 0/2 itself; here every sub-channel and packet component stands for its component)"""
    out = []
    for q in sub:
        g = next((x for x in gd if not x["ls"] and x["subch_id"] == q["subch_id"]), None)
        out.append((q["subch_id"], g and next((u for u in ua if u["sid"] == g["sid"] and u["scids"] == g["scids"]), None),
                    next((x for x in lang if x[0] == 0 and x[1] == q["subch_id"]), None), g and next((p for p in pty if p[0] == g["sid"]), None),
                    g and next((r for r in labels if r["id"] == g["sid"]), None)))
    for q in pk:
        g = next((x for x in gd if x["ls"] and x["sid"] == int(q["sid"])), None)
        out.append((int(q["scid"]), g, next((f for f in fec if f[0] == int(q["subch_id"])), None)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--order", default="parent,off,on,parent,off,on")
    ap.add_argument("--parent", default=None, help="a libdabx.so to compare with (legs named 'parent' are skipped without it)")
    ap.add_argument("--chunks", type=int, default=4, help="timed 7-frame calls per leg")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    S = a.streams
    subch = ds.default_subchannels(18, 64)
    libs = {"tree": dx.load()}
    if a.parent:
        dx._LIB, os.environ["DABX_LIB"] = None, a.parent
        libs["parent"] = dx.load()
        del os.environ["DABX_LIB"]
    order = [n for n in a.order.split(",") if n != "parent" or a.parent]
    args = types.SimpleNamespace(ensembles=4, snr=20.0, streams=S, unlocked=0, unlocked_kind="silence", layout="uniform")
    engines = {}
    for key, L in libs.items():                                  # one engine per library, filled and primed alike
        dx._LIB = L
        eng = dx.Engine(n_streams=S, ring_frames=10, max_subch=18, out_frames=8)
        eng.set_subchannels(subch)
        ring_frames = bench.fill_rings(eng, torch, dev, args, 0, subch)
        engines[key] = eng

    def step(eng, n):
        for m in bench.region_chunks(n, 7, False):
            eng.commit(m * TF)
            eng.process(m, sync=False)

    for key, eng in engines.items():
        dx._LIB = libs[key]
        eng.commit(ring_frames * TF - TF)
        step(eng, 40)
        eng.synchronize()
    for name in order:
        key = "parent" if name == "parent" else "tree"
        dx._LIB, eng = libs[key], engines[key]
        if key == "parent":
            eng.set_fig_mode(-1)
        else:
            eng.set_fig_mode(-1, service_info=name == "on")
        step(eng, 14)                                            # (fresh SI tables and whatever else the switch resets: out of the timed part)
        eng.synchronize()
        t0 = time.perf_counter()
        step(eng, 7 * a.chunks)
        eng.synchronize()
        dt = time.perf_counter() - t0
        dx.fig_timing(eng, True)                                 # the kernel's own time: in steps of its own, the events slow a step down
        step(eng, 28)
        us = 1e3 * dx.fig_timing(eng, False)
        print(json.dumps({"what": "leg_" + name, "streams": S, "steps": 7 * a.chunks, "ms_per_step": round(1e3 * dt / (7 * a.chunks), 4),
                          "k_fig_us_median": round(float(np.median(us)), 1), "k_fig_us_min": round(float(us.min()), 1), "k_fig_us_max": round(float(us.max()), 1),
                          "launches_timed": int(len(us))}), flush=True)
    # ---- the directory against the getters' loop
    dx._LIB, eng = libs["tree"], engines["tree"]
    eng.set_fig_mode(-1, service_info=True)
    step(eng, 14)
    eng.synchronize()
    one, loop, join = [], [], []
    for _ in range(5):
        t0 = time.perf_counter()
        rows = eng.fig_directory(-1)
        one.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got = [([dx._subch_dict(q) for q in eng.fig_subchannels(s)], eng.fig_packet_components(s), eng.fig_labels(s), eng.fig_global_defs(s), eng.fig_user_apps(s),
                eng.fig_languages(s), eng.fig_programme_types(s), eng.fig_fec_schemes(s)) for s in range(S)]
        loop.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        joined = [host_join(*g) for g in got]
        join.append(time.perf_counter() - t0)
    L = dx.load()
    out, cnt = np.zeros((S, dx.FIG_MAX_COMPONENTS), dx.FIG_SERVICE), np.zeros(S, np.int32)
    raw = []
    for _ in range(5):                                           # the C call alone, without the binding's dicts
        t0 = time.perf_counter()
        dx.check(L.dabx_fig_directory(eng._h, -1, 0, dx._p(out), dx.FIG_MAX_COMPONENTS, dx._p(cnt)))
        raw.append(time.perf_counter() - t0)
    print(json.dumps({"what": "directory", "streams": S, "components_per_stream": len(rows[0]), "records": int(cnt.sum()), "joined_rows": len(joined[0]),
                      "dabx_fig_directory_ms": [round(1e3 * v, 2) for v in raw], "with_python_dicts_ms": [round(1e3 * v, 1) for v in one],
                      "getter_loop_ms": [round(1e3 * v, 1) for v in loop], "host_join_python_ms": [round(1e3 * v, 1) for v in join]}), flush=True)
    for key, eng in engines.items():
        dx._LIB = libs[key]
        eng.close()


if __name__ == "__main__":
    main()
