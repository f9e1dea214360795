"""The MOT stage -- k_mot as dabx_process launches it behind k_pad / k_pad_mp2 on the MSC batch's stream -- against the model of
tests/mot_cases.py (pad_handler.cpp:539-622 and mot_object.cpp:71-323 restated), built like test_gpu_pad_stage.py on stage_driver.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen byte by byte (tests/mot_cases.py lists it; test_mot_cases.py proves on the model
that the scenarios reach every branch and each side of every guard).  Two streams; slots at 64 and 192 kbit/s with MOT on (the second with
max_object_bytes 4 096), next to them a PAD slot without MOT, a plain DAB+ slot and a packet-mode slot.  After every batch the new objects
are read; at the end objects, bytes and counters are compared EXACTLY -- records by .tobytes(), bytes by np.array_equal, counters by == --
with MotModel on the PAD model's items and with MotModel on the device's own PAD items; the PAD items, logical frames, super frames and
records of every slot are still the PAD model's and the oracle back end's."""
import ctypes as C

import numpy as np
import pytest

import dabplus_cases as dc
import mot_cases as mc
import mp2_pad_cases as m2
import packet_cases as pkc
import pad_cases as pc
from dabstar_amd import lib as dx
from stage_driver import PAD_ITEMS, Follower, Ring, drive, engine, kernel_launches, oracle_mismatches, ring_mismatches

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH
MOT_OBJECTS = Ring("mot_stats", ("objects",), ("object_bytes",), "read_mot_objects", dx.MOT_OBJECT)
KINDS = mc.STAGE_LAYOUT


def _mot_follower():
    return Follower(MOT_OBJECTS, 144, max_bytes=1 << 18)           # a group emits at most one object, a batch brings at most 144 groups


def _slots(*kinds):
    return [j for j, (_, kind) in enumerate(KINDS) if kind in kinds]


def _state(eng, i):
    out = []
    for j in _slots("mot", "pad"):
        rec, by = eng.read_pad_items(i, j, 4)
        obj, ob = eng.read_mot_objects(i, j, 4)
        out.append((sorted(eng.pad_stats(i, j).items()), rec.tobytes(), by.tobytes(), sorted(eng.mot_stats(i, j).items()), obj.tobytes(), ob.tobytes()))
    return out


def _switch_on(eng, i, mot=True):
    for j, (kbps, kind) in enumerate(KINDS):
        if kind in ("mot", "pad"):
            eng.set_pad_mode(i, j)
            if kind == "mot" and mot:
                eng.set_mot_mode(i, j, max_object_bytes=mc.MAX_OBJECT_BYTES[j])
        elif kind == "pkt":
            eng.set_packet_mode(i, j, mc.PACKET_ADDRESS)


def _drive(eng, streams, schedule, mot=True):
    """stage_driver.drive on the streams with the PAD slots followed and, behind every batch, the new objects of the MOT slots taken."""
    cases = [mc.stream_case(s) for s in streams]
    followers = {(i, j): Follower(PAD_ITEMS, 144) for i in range(len(streams)) for j in _slots("mot", "pad")}
    objects = {(i, j): _mot_follower() for i in range(len(streams)) for j in _slots("mot")}

    def after_batch(i, n, taken):
        for j in _slots("mot"):
            objects[(i, j)].take(eng, i, j)

    got = drive(eng, cases, schedule, lambda eng, i: _switch_on(eng, i, mot), followers, _state, after_batch)
    for (i, j), g in got.items():
        g["pstats"], g["mstats"] = eng.pad_stats(i, j), eng.mot_stats(i, j)
        g["objects"], g["object_bytes"] = objects[(i, j)].result() if (i, j) in objects else (np.zeros(0, dx.MOT_OBJECT), np.zeros(0, np.uint8))
    return got, cases


def _mismatches(got, cases, mot=True):
    bad = []
    for (i, j), g in sorted(got.items()):
        kbps, kind = KINDS[j]
        tag = "stream %d slot %d (%d kbit/s, %s): " % (i, j, kbps, kind)
        o = cases[i][3][j]
        bad += oracle_mismatches(tag, g, o, cases[i][1][j])
        if kind not in ("mot", "pad"):
            if any(g["pstats"].values()) or any(g["mstats"].values()) or len(g["rec"]):
                bad.append(tag + "no PAD decoding and shows PAD or MOT results: %s %s" % (g["pstats"], g["mstats"]))
            continue
        pm = pc.run_model(o["sf"], o["sfi"])
        bad += ring_mismatches(tag, g, pm, pc.PAD_COUNTERS, "item")
        if g["pstats"]["items_lost"] != 0 or g["pstats"]["active"] != 1:
            bad.append(tag + "items_lost / active: %s" % g["pstats"])
        if kind != "mot" or not mot:
            if any(g["mstats"].values()) or len(g["objects"]):
                bad.append(tag + "no MOT decoding and shows MOT results: %s" % g["mstats"])
            continue
        view = {"rec": g["objects"], "bytes": g["object_bytes"], "pstats": g["mstats"]}
        bad += ring_mismatches(tag + "on the model's PAD items: ", view, mc.mot_model_of(pm, mc.max_bytes_of(j)), dx.MOT_COUNTERS, "object")
        bad += ring_mismatches(tag + "on the device's PAD items: ", view, mc.run_model(g["rec"], g["bytes"], mc.max_bytes_of(j)), dx.MOT_COUNTERS, "object")
        if g["mstats"]["objects_lost"] != 0 or g["mstats"]["active"] != 1 or g["mstats"]["pad_overrun"] != 0:
            bad.append(tag + "objects_lost / active / pad_overrun: %s" % g["mstats"])
    return bad


_runs = {}


def test_every_object_equals_the_model_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  k_mot ran once per batch, behind k_pad."""
    streams = list(range(mc.N_STREAMS))
    eng = engine(len(streams), len(KINDS))
    try:
        got, cases = _drive(eng, streams, [[B] * len(streams)] * mc.N_BATCHES)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches, [g["mstats"] for g in got.values() if g["mstats"]["active"]])
    assert launches["k_mot"] == mc.N_BATCHES + 1 == launches["k_pad"] == launches["k_dabplus"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
    bad = _mismatches(got, cases)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    total = {k: sum(g["mstats"][k] for g in got.values()) for k in dx.MOT_COUNTERS if k != "pad_overrun"}
    assert all(v > 0 for v in total.values()), total                # every guard and every counter was exercised on the device
    _runs["full"] = got


def test_objects_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """The boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): objects stay open across batch
    ends and across batches in which a stream receives nothing.  k_msc_frame is the only decoder here; the results are also byte for byte
    those of the full-batch run."""
    streams = list(range(mc.N_STREAMS))
    schedule = pc.boundary_schedule(len(streams), mc.N_FRAMES)
    eng = engine(len(streams), len(KINDS), fast_min=1 << 30, class_min=0)
    try:
        got, cases = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_mot"] == len(schedule) + 1 == launches["k_pad"] == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, launches
    bad = _mismatches(got, cases)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            f = _runs["full"][key]
            assert g["objects"].tobytes() == f["objects"].tobytes() and np.array_equal(g["object_bytes"], f["object_bytes"]) and g["mstats"] == f["mstats"], key
            assert g["rec"].tobytes() == f["rec"].tobytes() and np.array_equal(g["bytes"], f["bytes"]), key


def test_an_engine_that_never_enables_mot_launches_nothing_and_gives_what_it_gives_with_it():
    """Stream 0 with PAD and packet mode on and MOT never: zero k_mot launches, dabx_get_mot_stats all zero, nothing to read; PAD items,
    logical frames, super frames and records are the models' and the oracle's -- and byte for byte those of the run with MOT on."""
    eng = engine(1, len(KINDS))
    try:
        got, cases = _drive(eng, [0], [[B]] * mc.N_BATCHES, mot=False)
        launches = kernel_launches(eng)
        nothing = [eng.read_mot_objects(0, j, 16) for j in range(len(KINDS))]
    finally:
        eng.close()
    assert launches["k_mot"] == 0 and launches["k_pad"] == mc.N_BATCHES + 1, launches
    assert all(len(r) == 0 and len(b) == 0 for r, b in nothing)
    bad = _mismatches(got, cases, mot=False)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for (i, j), g in got.items():
            f = _runs["full"][(i, j)]
            assert g["rec"].tobytes() == f["rec"].tobytes() and np.array_equal(g["bytes"], f["bytes"]) and g["pstats"] == f["pstats"], j
            assert np.array_equal(g["frames"], f["frames"]) and np.array_equal(g["sf"], f["sf"]) and g["sfi"].tobytes() == f["sfi"].tobytes(), j


def _single(layout, cifs, j, script, follow_items=True):
    """One stream: PAD on slot j from the start, script[b](eng) in front of batch b; after every batch the new PAD items and the new
    objects (while MOT is on) are taken.  Returns (PAD items, their bytes, per batch (mot stats, new objects or None, bytes, first, first byte),
    pad item count in front of every batch, kernel launches)."""
    eng = engine(1, len(layout))
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_pad_mode(0, j)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        items, taken, before = Follower(PAD_ITEMS, 144), [], []
        objects = _mot_follower()
        for b in range((len(cifs) - H) // B):
            if b in script:
                if script[b](eng) == "restart":
                    objects = _mot_follower()
            st = eng.pad_stats(0, j)
            before.append(st["labels"] + st["groups"])
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            if follow_items:
                items.take(eng, 0, j)
            taken.append(objects.take(eng, 0, j) if eng.mot_stats(0, j)["active"] else (eng.mot_stats(0, j), None, None, 0, 0))
        return items.result() + (taken, before, kernel_launches(eng))
    finally:
        eng.close()


def _since(rec, by, first):
    """The PAD items from item `first` on, byte_pos counted from the first of them."""
    r = rec[first:].copy()
    base = int(r["byte_pos"][0]) if len(r) else 0
    r["byte_pos"] -= base
    return r, by[base:]


def test_mot_on_off_and_on_again_and_set_pad_mode_ends_it():
    """Stream 0's 64 kbit/s slot.  MOT on for batch 0, off (NULL) for batch 1, on again from batch 2: the objects after each start are the
    model's on the PAD items emitted from then on (a slot that is switched on starts with an empty object, in the middle of whatever is on
    air).  dabx_set_pad_mode in front of batch 6 ends MOT decoding: the stats are all zero and nothing more is read, while PAD decoding goes
    on."""
    layout, frames, cifs, want = mc.stream_case(0)
    j = 0
    script = {0: lambda eng: eng.set_mot_mode(0, j), 1: lambda eng: eng.set_mot_mode(0, j, on=False),
              2: lambda eng: (eng.set_mot_mode(0, j), "restart")[1]}
    rec, by, taken, before, launches = _single(layout, cifs, j, script)
    assert launches["k_mot"] == 1 + (mc.N_BATCHES - 2) and launches["k_pad"] == mc.N_BATCHES + 1, launches
    assert not any(taken[1][0].values()) and taken[1][1] is None
    pm = pc.run_model(want[j]["sf"], want[j]["sfi"])
    assert rec.tobytes() == pm.records().tobytes() and np.array_equal(by, pm.all_bytes())
    for batches, upto in (((0,), before[1]), (range(2, mc.N_BATCHES), len(rec))):
        m = mc.run_model(*_since(rec[:upto], by, before[batches[0]]))
        got = [taken[b] for b in batches if taken[b][1] is not None]
        objs, ob = np.concatenate([t[1] for t in got]), np.concatenate([t[2] for t in got])
        assert len(objs) > 3 and objs.tobytes() == m.records().tobytes() and np.array_equal(ob, m.all_bytes()), batches
        st = taken[batches[-1]][0]
        assert all(st[k] == m.counters[k] for k in dx.MOT_COUNTERS) and st["active"] == 1 and st["objects_lost"] == 0, (st, m.counters)

    def pad_again(eng):
        eng.set_mot_mode(0, j)
        eng.set_pad_mode(0, j)
    rec, by, taken, before, launches = _single(layout, cifs, j, {0: lambda eng: eng.set_mot_mode(0, j), 6: pad_again}, follow_items=False)
    assert launches["k_mot"] == 6 and launches["k_pad"] == mc.N_BATCHES + 1, launches
    assert all(t[0]["active"] == 1 for t in taken[:6]) and all(not any(t[0].values()) and t[1] is None for t in taken[6:])


def test_a_slot_that_moves_to_other_capacity_units_in_the_middle_of_an_object_loses_nothing_and_a_changed_one_loses_its_state():
    """dabx_set_subchannels with the MOT slot at other capacity units while the 3 000-byte object is under assembly: the slot "keeps
    decoding without interruption", and so do the PAD and the MOT state -- every object equals the model's on the whole scenario.  Then the
    slot's protection level changes: a changed slot starts anew, without PAD and MOT decoding."""
    kbps = 64
    frames, sfs, sfi = mc.mot_frames(0, 0)
    old = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, pc.PROT, 0)], dab_plus=[0, 1])
    new = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, pc.PROT, 0)], dab_plus=[0, 1])
    new[1].cu_start = 400
    filler = pkc.scenario(64, 5, mc.N_FRAMES)
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    m = mc.mot_model_of(pc.run_model(sfs, sfi), 65536)
    r = m.records()
    done = int(r["frame"][r["body_len"] == 3000][0])
    b_move = (done - 30) // B
    assert done - 80 < b_move * B < done - 5, (done, b_move)          # the object takes some 90 logical frames: the move falls inside it
    move = H + b_move * B
    cifs = np.concatenate([c_old[:move], c_new[move:]])
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_pad_mode(0, 1)
        eng.set_mot_mode(0, 1)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        ring = _mot_follower()
        for b in range(mc.N_BATCHES):
            if b == b_move:
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            st = ring.take(eng, 0, 1)[0]
        rec, by = ring.result()
        changed = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, 2, 0)], dab_plus=[0, 1])
        eng.set_subchannels(changed, stream=0)
        after, after_pad = eng.mot_stats(0, 1), eng.pad_stats(0, 1)
    finally:
        eng.close()
    assert rec.tobytes() == r.tobytes() and np.array_equal(by, m.all_bytes()), (len(rec), len(r))
    assert all(st[k] == m.counters[k] for k in dx.MOT_COUNTERS) and st["objects_lost"] == 0, (st, m.counters)
    assert not any(after.values()) and not any(after_pad.values()), (after, after_pad)


def test_set_mot_mode_refuses_a_slot_without_pad_decoding_and_sizes_out_of_range():
    layout = mc.stage_layout()
    eng = engine(1, len(KINDS) + 1)
    L = dx.load()
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, 4, mc.PACKET_ADDRESS)
        for j in (0, 3, 4, 5, 6, -1):                                  # DAB+ slots without PAD decoding, a packet-mode slot, an empty slot, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_mot_mode(0, j)
        with pytest.raises(dx.DabxError):
            eng.set_mot_mode(1, 0)                                     # no such stream
        eng.set_mot_mode(0, 0, on=False)                               # NULL on a slot without MOT decoding: nothing to do
        eng.set_pad_mode(0, 0)
        for size in (1, 255, (4 << 20) + 1, 0xFFFFFFFF):
            with pytest.raises(dx.DabxError):
                eng.set_mot_mode(0, 0, max_object_bytes=size)
        assert eng.mot_stats(0, 0)["active"] == 0
        for size in (256, 4 << 20, 0):
            eng.set_mot_mode(0, 0, max_object_bytes=size)
            assert eng.mot_stats(0, 0) == dict(dict.fromkeys(dx.MOT_STATS.names[:-1], 0), transport_id=-1, active=1)
        short = dx.MotConfig(size=4, max_object_bytes=1)               # max_object_bytes is read only when size >= 8
        dx.check(L.dabx_set_mot_mode(eng._h, 0, 0, C.byref(short)))
        eng.set_pad_mode(0, 0)                                         # PAD restarts: MOT decoding ends
        assert eng.mot_stats(0, 0)["active"] == 0 and eng.pad_stats(0, 0)["active"] == 1
        eng.set_mot_mode(0, 0)
        eng.set_pad_mode(0, 0, on=False)                               # ... and so it does when PAD is switched off
        assert eng.mot_stats(0, 0)["active"] == 0 and eng.pad_stats(0, 0)["active"] == 0
        with pytest.raises(dx.DabxError):
            eng.set_mot_mode(0, 0)
        eng.set_pad_mode(0, 2)                                         # another PAD slot changes the PAD job table: slot 0 follows
        eng.set_pad_mode(0, 1)
        eng.set_mot_mode(0, 1)
        eng.set_pad_mode(0, 0)
        assert eng.mot_stats(0, 1)["active"] == 1 and eng.mot_stats(0, 0)["active"] == 0 and eng.mot_stats(0, 2)["active"] == 0
    finally:
        eng.close()


def test_object_rings_overrun_on_purpose_count_exactly_what_is_lost():
    """max_object_bytes 256: a byte ring of 32 KiB.  One object of 250 bytes and 400 repeated headers, each of which emits it again, two
    per access unit at 192 kbit/s, and nobody reads: at the end the newest 131 objects are intact (131 * 250 <= 32 768 < 132 * 250), they
    are the model's newest, and every older one is counted in objects_lost -- once."""
    kbps, repeats = 192, 400
    groups = mc.overrun_groups(9, repeats)
    frames, sfs, sfi = mc.build_frames(kbps, mc.units_of(groups, 9, size=24, per_unit=2), 9, n_frames=7 * B)
    layout = dc.dabplus_layout([(kbps, pc.PROT, 0)], dab_plus=[1])
    cifs = dc.cifs_of(layout, [frames], np.random.default_rng(4))
    m = mc.mot_model_of(pc.run_model(sfs, sfi), 256)
    assert len(m.rows) == repeats + 1 and all(len(p) == 250 for p in m.payloads)
    eng = engine(1, 1)
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_pad_mode(0, 0)
        eng.set_mot_mode(0, 0, max_object_bytes=256)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        for b in range(7):
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
        rec, by = eng.read_mot_objects(0, 0, 256, max_bytes=1 << 16)
        st = eng.mot_stats(0, 0)
        rec2, by2 = eng.read_mot_objects(0, 0, 3, max_bytes=1 << 16)
        st2 = eng.mot_stats(0, 0)
    finally:
        eng.close()
    keep = 32768 // 250
    want = m.records()[-keep:].copy()
    want["byte_pos"] -= want["byte_pos"][0]
    assert len(rec) == keep == 131 and rec.tobytes() == want.tobytes() and np.array_equal(by, m.all_bytes()[-keep * 250:])
    assert st["objects"] == repeats + 1 and st["objects_lost"] == repeats + 1 - keep and all(st[k] == m.counters[k] for k in dx.MOT_COUNTERS), (st, m.counters)
    assert rec["repeat"].max() == 255 and rec["repeat"].min() == 255
    want3 = want[-3:].copy()
    want3["byte_pos"] -= want3["byte_pos"][0]
    assert len(rec2) == 3 and rec2.tobytes() == want3.tobytes() and np.array_equal(by2, by[-750:]) and st2 == st


def test_mp2_source_slots_with_mot_on_equal_the_model_on_their_items():
    """Streams 0 and 1 of tests/mp2_pad_cases.py (both layouts) with MOT on for every MP2 source slot: k_mot behind k_pad_mp2.  Their PAD
    scenarios carry random groups with good CRCs, so the group-header walk and the guards run on bytes nobody crafted.  Objects, bytes and
    counters equal MotModel on the MP2 model's items; the PAD items themselves are unchanged."""
    streams = [0, 1]
    cases = [m2.stream_case(s) for s in streams]
    mp2 = [(i, j) for i, s in enumerate(streams) for j, (_, kind) in enumerate(m2.kinds(s)) if kind == "mp2"]
    followers = {k: Follower(PAD_ITEMS, 112) for k in mp2}
    objects = {k: _mot_follower() for k in mp2}

    def switch_on(eng, i):
        for j, (kbps, kind) in enumerate(m2.kinds(streams[i])):
            if kind == "mp2":
                eng.set_pad_mode(i, j, source="mp2")
                eng.set_mot_mode(i, j)

    def state(eng, i):
        return [(sorted(eng.mot_stats(i, j).items()), sorted(eng.pad_stats(i, j).items())) for (s, j) in mp2 if s == i]

    def after_batch(i, n, taken):
        for (s, j) in mp2:
            if s == i:
                objects[(s, j)].take(eng, s, j)

    eng = engine(len(streams), 5)
    try:
        got = drive(eng, cases, [[B] * len(streams)] * m2.N_BATCHES, switch_on, followers, state, after_batch)
        stats = {k: eng.mot_stats(*k) for k in mp2}
        launches = kernel_launches(eng)
    finally:
        eng.close()
    assert launches["k_mot"] == launches["k_pad"] == m2.N_BATCHES + 1, launches
    bad, groups = [], 0
    for (i, j) in mp2:
        tag = "stream %d slot %d (%d kbit/s, mp2): " % (i, j, m2.kinds(streams[i])[j][0])
        pm = m2.slot_model(streams[i], j).pad
        g = got[(i, j)]
        bad += ring_mismatches(tag, g, pm, (), "item")
        rec, by = objects[(i, j)].result()
        m = mc.mot_model_of(pm, 65536)
        bad += ring_mismatches(tag, {"rec": rec, "bytes": by, "pstats": stats[(i, j)]}, m, dx.MOT_COUNTERS, "object")
        if stats[(i, j)]["objects_lost"] or stats[(i, j)]["pad_overrun"] or not stats[(i, j)]["active"]:
            bad.append(tag + "objects_lost / pad_overrun / active: %s" % stats[(i, j)])
        groups += m.counters["groups"]
    print({k: sum(s[k] for s in stats.values()) for k in dx.MOT_COUNTERS})
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    assert groups > 100
