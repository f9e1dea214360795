"""The data handlers of a packet-mode slot on the device -- k_data_batch on crafted groups without an engine, and k_data_handler as
dabx_process launches it behind k_packet on the MSC batch's stream -- against the models of tests/data_handler_cases.py
(tdc_datahandler.cpp:52-193, ip_datahandler.cpp:44-148, dabdgdec_impl.c:130-296 with journaline_datahandler.cpp:38-132 restated), built like
test_gpu_carousel_stage.py on stage_driver.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen byte by byte (tests/data_handler_cases.py lists it; test_data_handler_cases.py
proves on the models that the inputs reach every branch and each side of every guard).  Two streams with one slot per handler (TDC 128
kbit/s, IP 64, Journaline 128; only_new_revisions on stream 1) beside a plain packet slot, a carousel slot and a DAB+ slot.  After every
batch the new items are read; at the end items, bytes and every counter are compared EXACTLY -- records by .tobytes(), bytes by
np.array_equal, counters by == -- with the model on the packet model's groups and with the model on the device's own data groups; the data
groups and logical frames are still the packet model's and the oracle back end's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import data_handler_cases as dh
import dabplus_cases as dc
import packet_cases as pkc
from dabstar_amd import lib as dx
from stage_driver import Follower, Ring, drive, engine, kernel_launches, oracle_mismatches, packet_follower, ring_mismatches

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(__file__), "..")
H, B = dc.HISTORY, dc.BATCH
DATA_ITEMS = Ring("data_stats", ("items",), ("bytes",), "read_data_items", dx.DATA_ITEM)
KINDS = dh.STAGE_LAYOUT
COUNTERS = dx.DATA_COUNTERS
PACKET_KINDS = dh.HANDLERS + ("pkt", "car")


def _follower():
    return Follower(DATA_ITEMS, 256, max_bytes=1 << 17)              # the record ring's size: the scenarios stay below it in every batch


def _slots(*kinds):
    return [j for j, (_, kind) in enumerate(KINDS) if kind in kinds]


@pytest.mark.parametrize("only_new", [False, True])
@pytest.mark.parametrize("handler", dh.HANDLERS)
def test_the_kernel_body_equals_the_model_on_crafted_groups_without_an_engine(handler, only_new):
    """dabx_internal_data_walk_device: every crafted group, the random ones, the 16 384-byte group and the 300 frames of length 0."""
    groups = dh.sequence(handler) + dh.random_groups(handler)
    if handler == "tdc":
        groups = groups + [dh.tdc_long_group(np.random.default_rng(55)), dh.overrun_group(np.random.default_rng(1))]
    rec, by = dh.records_of(groups)
    m = dh.run_model(handler, rec, by, only_new)
    items, ob, st = dx.data_walk(handler, rec, by, only_new, device=True)
    print({k: v for k, v in st.items() if v})
    want = m.records()
    assert items.tobytes() == want.tobytes(), [(k, items[k].tolist(), want[k].tolist()) for k in range(min(len(items), len(want))) if items[k].tobytes() != want[k].tobytes()][:3]
    assert np.array_equal(ob, m.all_bytes())
    assert {k: st[k] for k in COUNTERS} == m.counters
    host = dx.data_walk(handler, rec, by, only_new)
    assert host[0].tobytes() == items.tobytes() and np.array_equal(host[1], ob) and host[2] == st


def test_the_engine_less_entry_refuses_no_group_and_the_host_entry_gives_nothing_for_it():
    none = np.zeros(0, dx.DATAGROUP_INFO)
    with pytest.raises(dx.DabxError):
        dx.data_walk("tdc", none, np.zeros(0, np.uint8), device=True)
    items, ob, st = dx.data_walk("tdc", none, np.zeros(0, np.uint8))
    assert len(items) == 0 and len(ob) == 0 and st == dict(dict.fromkeys(dx.DATA_STATS.names, 0), active=1, handler=1)
    # ... and groups of no byte at all, alone: the ring of input bytes is its smallest
    rec, by = dh.records_of([b"", b""])
    for handler in dh.HANDLERS:
        items, ob, st = dx.data_walk(handler, rec, by, device=True)
        assert len(items) == 0 and st == dx.data_walk(handler, rec, by)[2] and st["groups"] == 2, (handler, st)


def _state(eng, i):
    out = []
    for j in _slots(*PACKET_KINDS):
        it, ib = eng.read_data_items(i, j, 4)
        st = {k: v for k, v in eng.data_stats(i, j).items() if k != "launches"}      # (launches counts the engine's, whatever the stream)
        out.append((sorted(st.items()), sorted(eng.packet_stats(i, j).items()), it.tobytes(), ib.tobytes()))
    return out


def _switch_on(eng, i, data=True):
    for j, (kbps, kind) in enumerate(KINDS):
        if kind in PACKET_KINDS:
            eng.set_packet_mode(i, j, dh.ADDRESS)
        if kind == "car":
            eng.set_carousel_mode(i, j)
        if kind in dh.HANDLERS and data:
            eng.set_data_mode(i, j, kind, only_new_revisions=dh.ONLY_NEW[i])


def _drive(eng, streams, schedule, data=True):
    cases = [dh.stream_case(s) for s in streams]
    followers = {(i, j): packet_follower(KINDS[j][0]) for i in range(len(streams)) for j in _slots(*PACKET_KINDS)}
    items = {(i, j): _follower() for i in range(len(streams)) for j in _slots(*dh.HANDLERS) if data}

    def after_batch(i, n, taken):
        for (s, j), f in items.items():
            if s == i:
                f.take(eng, i, j)

    got = drive(eng, cases, schedule, lambda eng, i: _switch_on(eng, i, data), followers, _state, after_batch)
    for (i, j), g in got.items():
        g["pstats"], g["dstats"], g["cstats"] = eng.packet_stats(i, j), eng.data_stats(i, j), eng.carousel_stats(i, j)
        g["items"], g["item_bytes"] = items[(i, j)].result() if (i, j) in items else (np.zeros(0, dx.DATA_ITEM), np.zeros(0, np.uint8))
    return got, cases


def _mismatches(got, cases, streams, data=True):
    bad = []
    for (i, j), g in sorted(got.items()):
        kbps, kind = KINDS[j]
        tag = "stream %d slot %d (%d kbit/s, %s): " % (i, j, kbps, kind)
        bad += oracle_mismatches(tag, g, cases[i][3][j], cases[i][1][j])
        d = g["dstats"]
        if kind == "dab+":
            if any(g["pstats"].values()) or any(v for k, v in d.items() if k != "launches") or len(g["rec"]):
                bad.append(tag + "a DAB+ slot shows packet or handler results: %s %s" % (g["pstats"], d))
            continue
        dm = pkc.run_model(cases[i][1][j], dh.ADDRESS)
        bad += ring_mismatches(tag, g, dm, pkc.PACKET_COUNTERS, "data group")
        if g["pstats"]["dg_lost"] != 0 or g["pstats"]["active"] != 1:
            bad.append(tag + "dg_lost / active: %s" % g["pstats"])
        if kind == "car" and (g["cstats"]["active"] != 1 or g["cstats"]["groups"] != dm.counters["dg_count"]):
            bad.append(tag + "the carousel beside the handlers: %s" % g["cstats"])
        if kind not in dh.HANDLERS or not data:
            if any(v for k, v in d.items() if k != "launches") or len(g["items"]):
                bad.append(tag + "no handler and shows handler results: %s" % d)
            continue
        view = {"rec": g["items"], "bytes": g["item_bytes"], "pstats": d}
        only = dh.ONLY_NEW[streams[i]]
        bad += ring_mismatches(tag + "on the model's data groups: ", view, dh.model_of(kind, dm, only), COUNTERS, "item")
        bad += ring_mismatches(tag + "on the device's data groups: ", view, dh.run_model(kind, g["rec"], g["bytes"], only), COUNTERS, "item")
        if d["lost"] != 0 or d["active"] != 1 or d["dg_overrun"] != 0 or d["handler"] != dx.DATA_HANDLERS[kind]:
            bad.append(tag + "lost / active / dg_overrun / handler: %s" % d)
    return bad


_runs = {}


def test_every_item_equals_the_model_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  k_data_handler ran once per batch, behind k_packet."""
    streams = list(range(dh.N_STREAMS))
    eng = engine(len(streams), len(KINDS))
    try:
        dx.data_timing(eng, True)                                    # every launch between two events of its own (tools/bench_data_handlers.py)
        got, cases = _drive(eng, streams, [[B] * len(streams)] * dh.N_BATCHES)
        launches = kernel_launches(eng)
        timed = dx.data_timing(eng, False)
        assert len(dx.data_timing(eng, False)) == 0
    finally:
        eng.close()
    assert len(timed) == dh.N_BATCHES + 1 and (timed > 0).all() and (timed < 100).all(), timed
    active = [g["dstats"] for g in got.values() if g["dstats"]["active"]]
    print(launches, active)
    assert launches["k_packet"] == dh.N_BATCHES + 1 == launches["k_carousel"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
    assert all(g["dstats"]["launches"] == dh.N_BATCHES + 1 for g in got.values())
    bad = _mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    total = {k: sum(d[k] for d in active) for k in COUNTERS if k != "dg_overrun"}
    assert all(v > 0 for v in total.values()), total                # every guard and every counter was exercised on the device
    kinds = np.concatenate([g["items"]["kind"] for g in got.values()])
    assert set(kinds) == {dx.DATA_TDC_0, dx.DATA_TDC_1, dx.DATA_UDP, dx.DATA_NML}
    assert max(int(g["items"]["length"].max()) for g in got.values() if len(g["items"])) == dx.DG_MAX_BYTES - 7
    _runs["full"] = got


def test_items_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """stage_driver's boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): groups stay open across
    batch ends and across batches in which a stream receives nothing.  k_msc_frame is the only decoder here; the results are also byte for
    byte those of the full-batch run."""
    streams = list(range(dh.N_STREAMS))
    schedule = pkc.boundary_schedule(len(streams), dh.N_FRAMES)
    eng = engine(len(streams), len(KINDS), fast_min=1 << 30, class_min=0)
    try:
        got, cases = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_packet"] == len(schedule) + 1 == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, launches
    assert all(g["dstats"]["launches"] == len(schedule) + 1 for g in got.values())
    bad = _mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            f = _runs["full"][key]
            assert g["items"].tobytes() == f["items"].tobytes() and np.array_equal(g["item_bytes"], f["item_bytes"]), key
            assert {k: v for k, v in g["dstats"].items() if k != "launches"} == {k: v for k, v in f["dstats"].items() if k != "launches"}, key
            assert g["rec"].tobytes() == f["rec"].tobytes() and np.array_equal(g["bytes"], f["bytes"]), key


def test_an_engine_without_a_handler_slot_launches_nothing_and_gives_what_it_gives_with_them():
    """Stream 0 with packet mode and the carousel on and no handler: launches == 0, dabx_get_data_stats all zero, nothing to read; data
    groups, logical frames, super frames and the carousel's counters are byte for byte those of the run with the handlers on."""
    eng = engine(1, len(KINDS))
    try:
        got, cases = _drive(eng, [0], [[B]] * dh.N_BATCHES, data=False)
        launches = kernel_launches(eng)
        nothing = [eng.read_data_items(0, j, 16) for j in range(len(KINDS))]
    finally:
        eng.close()
    assert launches["k_packet"] == dh.N_BATCHES + 1 == launches["k_carousel"], launches
    assert all(not any(g["dstats"].values()) for g in got.values())
    assert all(len(r) == 0 and len(b) == 0 for r, b in nothing)
    bad = _mismatches(got, cases, [0], data=False)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for (i, j), g in got.items():
            f = _runs["full"][(i, j)]
            assert g["rec"].tobytes() == f["rec"].tobytes() and np.array_equal(g["bytes"], f["bytes"]) and g["pstats"] == f["pstats"] and g["cstats"] == f["cstats"], j
            assert np.array_equal(g["frames"], f["frames"]) and np.array_equal(g["sf"], f["sf"]) and g["sfi"].tobytes() == f["sfi"].tobytes() and g["stats"] == f["stats"], j


def _since(rec, by, first):
    """The data groups from group `first` on, byte_pos counted from the first of them."""
    r = rec[first:].copy()
    base = int(r["byte_pos"][0]) if len(r) else 0
    r["byte_pos"] -= base
    return r, by[base:]


def _single(layout, cifs, j, script, cuts=()):
    """One stream: packet mode on slot j from the start, script[b](eng) in front of batch b; after every batch the new data groups and the
    new items (while a handler is on) are taken.  Returns (data groups, their bytes, per batch take() results, group count in front of
    every batch)."""
    eng = engine(1, len(layout))
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, j, dh.ADDRESS)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        groups, taken, before = packet_follower(layout[j].kbps), [], []
        items = _follower()
        n = len(cifs) - H
        edges = sorted(set(range(0, n + 1, B)) | set(cuts) | {n})
        for b, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            if b in script and script[b](eng) == "restart":
                items = _follower()
            before.append(eng.packet_stats(0, j)["dg_count"])
            dx.msc_inject(eng, 0, cifs[H + lo:H + hi])
            dx.msc_decode(eng, [hi - lo], B)
            groups.take(eng, 0, j)
            st = eng.data_stats(0, j)
            taken.append(items.take(eng, 0, j) if st["active"] else (st, None, None, 0, 0))
        return groups.result() + (taken, before)
    finally:
        eng.close()


def test_a_handler_on_off_and_on_again_and_set_packet_mode_ends_it():
    """Stream 0's Journaline slot, with two further batch boundaries behind its second item.  The handler on for batch 0, off (NULL) for
    batch 1, on again from batch 2 -- restarted with an empty table: the items after each start are the model's on the data groups
    completed from then on, `group` counting in the slot's sequence.  In a second engine dabx_set_packet_mode in front of the second batch
    ends it: the stats are all zero but `launches`, while the packet stage goes on."""
    layout, frames, cifs, want = dh.stream_case(0)
    j = _slots("journaline")[0]
    on = lambda eng: eng.set_data_mode(0, j, "journaline")      # noqa: E731
    script = {0: on, 1: lambda eng: eng.set_data_mode(0, j, on=False), 2: lambda eng: (on(eng), "restart")[1]}
    at = dh.model_of("journaline", pkc.run_model(frames[j], dh.ADDRESS)).records()["frame"]
    c1 = int(at[1]) + 1                                               # the batch boundaries: behind the second item, and two logical frames on
    cuts = (c1, c1 + 2)
    assert 0 < c1 < c1 + 2 < B and (at > c1 + 2).sum() >= 5
    rec, by, taken, before = _single(layout, cifs, j, script, cuts)
    n_batches = len(taken)
    assert n_batches == dh.N_BATCHES + 2
    assert not any(v for k, v in taken[1][0].items() if k != "launches") and taken[1][1] is None
    assert taken[-1][0]["launches"] == n_batches - 1
    eng = engine(1, len(layout))
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, j, dh.ADDRESS)
        on(eng)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        stats = []
        for b in range(2):
            if b == 1:
                eng.set_packet_mode(0, j, dh.ADDRESS)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            stats.append(eng.data_stats(0, j))
        late, pst = eng.read_data_items(0, j, 16), eng.packet_stats(0, j)
    finally:
        eng.close()
    assert stats[0]["active"] == 1 and stats[0]["items"] > 0 and stats[0]["launches"] == 2
    assert stats[1] == dict(dict.fromkeys(dx.DATA_STATS.names, 0), launches=2) and len(late[0]) == 0 and pst["active"] == 1 and pst["dg_count"] > 0
    for batches, upto in (((0,), before[1]), (range(2, n_batches), len(rec))):
        first = before[batches[0]]
        m = dh.run_model("journaline", *_since(rec[:upto], by, first), first_group=first)
        got = [taken[b] for b in batches if taken[b][1] is not None]
        its, ib = np.concatenate([t[1] for t in got]), np.concatenate([t[2] for t in got])
        assert len(its) >= 2 and its.tobytes() == m.records().tobytes() and np.array_equal(ib, m.all_bytes()), batches
        st = taken[batches[-1]][0]
        assert all(st[k] == m.counters[k] for k in COUNTERS) and st["active"] == 1 and st["lost"] == 0, (st, m.counters)


def test_a_slot_that_moves_to_other_capacity_units_in_the_middle_of_a_group_loses_nothing_and_a_changed_one_loses_its_handler():
    """dabx_set_subchannels with the TDC slot at other capacity units while the 16 384-byte group is under assembly: the slot "keeps decoding
    without interruption", and so do the packet stage and the handler.  Then the slot's protection level changes: a changed slot starts
    anew, without packet mode and handler."""
    kbps = KINDS[0][0]
    frames = dh.slot_frames(0, 0)
    dm = pkc.run_model(frames, dh.ADDRESS)
    r = dm.records()
    long_one = int(np.flatnonzero(r["length"] == dx.DG_MAX_BYTES)[0])
    assert r["last_frame"][long_one] - r["first_frame"][long_one] > 20
    cut = int(r["first_frame"][long_one]) + 10
    old = dc.dabplus_layout([(64, pkc.PROT, 0), (kbps, pkc.PROT, 0)], dab_plus=[0, 0])
    new = dc.dabplus_layout([(64, pkc.PROT, 0), (kbps, pkc.PROT, 0)], dab_plus=[0, 0])
    new[1].cu_start = 400
    filler = pkc.scenario(64, 5, dh.N_FRAMES)
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    cifs = np.concatenate([c_old[:H + cut], c_new[H + cut:]])
    m = dh.model_of("tdc", dm)
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_packet_mode(0, 1, dh.ADDRESS)
        eng.set_data_mode(0, 1, "tdc")
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        ring = _follower()
        edges = sorted(set(range(0, dh.N_FRAMES + 1, B)) | {cut})
        for lo, hi in zip(edges[:-1], edges[1:]):
            if lo == cut:
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + lo:H + hi])
            dx.msc_decode(eng, [hi - lo], B)
            st = ring.take(eng, 0, 1)[0]
        rec, by = ring.result()
        changed = dc.dabplus_layout([(64, pkc.PROT, 0), (kbps, 2, 0)], dab_plus=[0, 0])
        eng.set_subchannels(changed, stream=0)
        after, after_pkt = eng.data_stats(0, 1), eng.packet_stats(0, 1)
    finally:
        eng.close()
    assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (len(rec), len(m.rows))
    assert all(st[k] == m.counters[k] for k in COUNTERS) and st["lost"] == 0, (st, m.counters)
    assert not any(v for k, v in after.items() if k != "launches") and not any(after_pkt.values()), (after, after_pkt)


def test_set_data_mode_refuses_what_it_must():
    layout = dh.stage_layout()
    eng = engine(1, len(KINDS) + 1)
    L = dx.load()
    try:
        eng.set_subchannels(layout, stream=0)
        for j in (0, 5, 6, -1):                                        # a slot not in packet mode, a DAB+ slot, an empty slot, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_data_mode(0, j, "ip")
        with pytest.raises(dx.DabxError):
            eng.set_data_mode(1, 0, "ip")                              # no such stream
        eng.set_data_mode(0, 0, on=False)                              # NULL on a slot without a handler: nothing to do
        eng.set_packet_mode(0, 0, dh.ADDRESS)
        for handler in (0, 4, 5, -1):
            with pytest.raises(dx.DabxError):
                eng.set_data_mode(0, 0, handler)
        bad = dx.DataConfig(size=32, handler=2)
        bad.reserved[4] = 1
        assert L.dabx_set_data_mode(eng._h, 0, 0, C.byref(bad)) == -2
        assert L.dabx_set_data_mode(eng._h, 0, 0, C.byref(dx.DataConfig(size=4, handler=2))) == -2
        assert eng.data_stats(0, 0)["active"] == 0
        short = dx.DataConfig(size=8, handler=3, only_new_revisions=1)      # only_new_revisions is read only when size covers it
        short.reserved[0] = 7
        dx.check(L.dabx_set_data_mode(eng._h, 0, 0, C.byref(short)))
        fresh = dict(dict.fromkeys(dx.DATA_STATS.names, 0), active=1, handler=3)
        assert eng.data_stats(0, 0) == fresh
        eng.set_carousel_mode(0, 0)                                    # independent of the carousel mode
        assert eng.data_stats(0, 0) == fresh and eng.carousel_stats(0, 0)["active"] == 1
        eng.set_packet_mode(0, 0, dh.ADDRESS)                          # the packet stage restarts: the handler ends
        assert eng.data_stats(0, 0)["active"] == 0 and eng.packet_stats(0, 0)["active"] == 1
        eng.set_data_mode(0, 0, "tdc")
        eng.set_packet_mode(0, 0, None)                                # ... and so it does when packet mode is switched off
        assert eng.data_stats(0, 0)["active"] == 0 and eng.packet_stats(0, 0)["active"] == 0
        eng.set_packet_mode(0, 2, dh.ADDRESS)                          # another packet slot changes the packet job table: slot 1 follows
        eng.set_packet_mode(0, 1, dh.ADDRESS)
        eng.set_data_mode(0, 1, "ip")
        eng.set_packet_mode(0, 0, dh.ADDRESS)
        assert eng.data_stats(0, 1)["active"] == 1 and eng.data_stats(0, 1)["handler"] == 2 and eng.data_stats(0, 0)["active"] == 0
        for n, info in ((0, np.zeros(1, dx.DATA_ITEM)), (1, None)):
            assert L.dabx_read_data_items(eng._h, 0, 1, n, dx._p(info) if info is not None else None, None, 0) == -2
    finally:
        eng.close()


def test_the_record_ring_overrun_on_purpose_returns_the_newest_and_counts_the_rest_once():
    """One group of 300 TDC frames of length 0 in one batch against a record ring of 256: the newest 256 items are returned, they are the
    model's newest, and the 44 older ones are counted in `lost` -- once."""
    kbps = 128
    g = dh.overrun_group(np.random.default_rng(1))
    w = pkc.Writer(kbps, np.random.default_rng(9))
    w.emit(w.cut(g, dh.ADDRESS, dense=True))
    w.pad_frame()
    assert len(w.frames) <= B
    while len(w.frames) < B:
        w.pad(w.gran)
    frames = np.frombuffer(b"".join(w.frames), np.uint8).reshape(B, 3 * kbps)
    layout = dc.dabplus_layout([(kbps, pkc.PROT, 0)], dab_plus=[0])
    cifs = dc.cifs_of(layout, [frames], np.random.default_rng(4))
    m = dh.model_of("tdc", pkc.run_model(frames, dh.ADDRESS))
    assert len(m.rows) == 300
    eng = engine(1, 1)
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, 0, dh.ADDRESS)
        eng.set_data_mode(0, 0, "tdc")
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        dx.msc_inject(eng, 0, cifs[H:])
        dx.msc_decode(eng, [B], B)
        rec, by = eng.read_data_items(0, 0, 512)
        st = eng.data_stats(0, 0)
        rec2, by2 = eng.read_data_items(0, 0, 3)
        st2 = eng.data_stats(0, 0)
    finally:
        eng.close()
    want = m.records()[-256:]
    assert len(rec) == 256 and rec.tobytes() == want.tobytes() and len(by) == 0
    assert st["items"] == 300 and st["lost"] == 44 and all(st[k] == m.counters[k] for k in COUNTERS), (st, m.counters)
    assert len(rec2) == 3 and rec2.tobytes() == want[-3:].tobytes() and st2 == st


def test_the_stage_runs_in_the_hipmodule_form():
    """the engine-less entry and the full-batch engine run again with the binding pointed at hipmodule/libdabx.so: k_data_batch and
    k_data_handler are found in the code objects"""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_data_handler_stage.py", "-k",
                        "without_an_engine or lane_per_trellis"], cwd=ROOT, env=hipmodule_env(), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "7 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
