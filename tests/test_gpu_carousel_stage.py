"""The carousel stage -- k_carousel as dabx_process launches it behind k_packet on the MSC batch's stream -- against the model of
tests/carousel_cases.py (mot_handler.cpp:69-259 and mot_dir.cpp:28-156 restated), built like test_gpu_mot_stage.py on stage_driver.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen byte by byte (tests/carousel_cases.py lists it; test_carousel_cases.py proves on
the model that the scenarios reach every branch and each side of every guard).  Two streams; carousel slots at 64 kbit/s (header mode,
max_object_bytes 4 096) and 384 kbit/s (directory mode, max_dir_objects 8), next to them a packet-mode slot without carousel decoding, a
DAB+ slot with PAD and MOT decoding and a plain slot.  After every batch the new objects are read; at the end objects, bytes and counters
are compared EXACTLY -- records by .tobytes(), bytes by np.array_equal, counters by == -- with MotHandlerModel on the packet model's groups
and with MotHandlerModel on the device's own data groups; the data groups, logical frames and the MOT slot's results are still the
models' and the oracle back end's."""
import ctypes as C

import numpy as np
import pytest

import carousel_cases as cc
import dabplus_cases as dc
import mot_cases as mc
import packet_cases as pkc
import pad_cases as pc
from dabstar_amd import lib as dx
from stage_driver import PAD_ITEMS, Follower, Ring, drive, engine, kernel_launches, oracle_mismatches, packet_follower, ring_mismatches

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH
CAR_OBJECTS = Ring("carousel_stats", ("objects",), ("object_bytes",), "read_mot_objects", dx.MOT_OBJECT)
MOT_OBJECTS = Ring("mot_stats", ("objects",), ("object_bytes",), "read_mot_objects", dx.MOT_OBJECT)
KINDS = cc.STAGE_LAYOUT
COUNTERS = dx.CAROUSEL_COUNTERS
NEVER = ("dg_overrun",)                            # the packet rings hold two batches: the stage is never overrun


def _follower(ring=CAR_OBJECTS):
    return Follower(ring, 256, max_bytes=1 << 18)                   # the record ring's size: the scenarios stay below it in every batch


def _slots(*kinds):
    return [j for j, (_, kind) in enumerate(KINDS) if kind in kinds]


def _cfg(j):
    return cc.SCENARIOS[cc.NAME_OF[j]][2]


def _state(eng, i):
    out = []
    for j in _slots("car", "pkt", "mot"):
        obj, ob = eng.read_mot_objects(i, j, 4)
        out.append((sorted(eng.carousel_stats(i, j).items()), sorted(eng.mot_stats(i, j).items()), sorted(eng.packet_stats(i, j).items()), obj.tobytes(), ob.tobytes()))
    return out


def _switch_on(eng, i, carousel=True):
    for j, (kbps, kind) in enumerate(KINDS):
        if kind in ("car", "pkt"):
            eng.set_packet_mode(i, j, cc.ADDRESS)
            if kind == "car" and carousel:
                eng.set_carousel_mode(i, j, **_cfg(j))
        elif kind == "mot":
            eng.set_pad_mode(i, j)
            eng.set_mot_mode(i, j)


def _drive(eng, streams, schedule, carousel=True):
    """stage_driver.drive on the streams with the packet and PAD slots followed and, behind every batch, the new objects taken."""
    cases = [cc.stream_case(s) for s in streams]
    followers = {(i, j): packet_follower(KINDS[j][0]) for i in range(len(streams)) for j in _slots("car", "pkt")}
    followers.update({(i, j): Follower(PAD_ITEMS, 144) for i in range(len(streams)) for j in _slots("mot")})
    objects = {(i, j): _follower() for i in range(len(streams)) for j in _slots("car") if carousel}
    objects.update({(i, j): _follower(MOT_OBJECTS) for i in range(len(streams)) for j in _slots("mot")})

    def after_batch(i, n, taken):
        for (s, j), f in objects.items():
            if s == i:
                f.take(eng, i, j)

    got = drive(eng, cases, schedule, lambda eng, i: _switch_on(eng, i, carousel), followers, _state, after_batch)
    for (i, j), g in got.items():
        g["pstats"], g["cstats"], g["mstats"] = eng.packet_stats(i, j), eng.carousel_stats(i, j), eng.mot_stats(i, j)
        g["padstats"] = eng.pad_stats(i, j)
        g["objects"], g["object_bytes"] = objects[(i, j)].result() if (i, j) in objects else (np.zeros(0, dx.MOT_OBJECT), np.zeros(0, np.uint8))
    return got, cases


def _mismatches(got, cases, streams, carousel=True):
    bad = []
    for (i, j), g in sorted(got.items()):
        kbps, kind = KINDS[j]
        tag = "stream %d slot %d (%d kbit/s, %s): " % (i, j, kbps, kind)
        o = cases[i][3][j]
        bad += oracle_mismatches(tag, g, o, cases[i][1][j])
        view = {"rec": g["objects"], "bytes": g["object_bytes"], "pstats": g["cstats"]}
        if kind == "mot":                                              # the X-PAD's MOT decoding beside the carousel: unchanged
            pm = pc.run_model(o["sf"], o["sfi"])
            bad += ring_mismatches(tag, dict(g, pstats=g["padstats"]), pm, pc.PAD_COUNTERS, "item")
            bad += ring_mismatches(tag, dict(view, pstats=g["mstats"]), mc.mot_model_of(pm, 65536), dx.MOT_COUNTERS, "object")
            if any(g["cstats"].values()) or g["mstats"]["objects_lost"]:
                bad.append(tag + "a PAD slot shows carousel results or lost objects: %s %s" % (g["cstats"], g["mstats"]))
            continue
        if any(g["mstats"].values()) or any(g["padstats"].values()):
            bad.append(tag + "no PAD decoding and shows PAD or MOT results: %s %s" % (g["padstats"], g["mstats"]))
        if kind == "plain":
            if any(g["pstats"].values()) or any(g["cstats"].values()) or len(g["rec"]):
                bad.append(tag + "a plain slot shows packet or carousel results: %s %s" % (g["pstats"], g["cstats"]))
            continue
        dm = pkc.run_model(cases[i][1][j], cc.ADDRESS)
        bad += ring_mismatches(tag, g, dm, pkc.PACKET_COUNTERS, "data group")
        if g["pstats"]["dg_lost"] != 0 or g["pstats"]["active"] != 1:
            bad.append(tag + "dg_lost / active: %s" % g["pstats"])
        if kind != "car" or not carousel:
            if any(g["cstats"].values()) or len(g["objects"]):
                bad.append(tag + "no carousel decoding and shows carousel results: %s" % g["cstats"])
            continue
        bad += ring_mismatches(tag + "on the model's data groups: ", view, cc.model_of(dm, **_cfg(j)), COUNTERS, "object")
        bad += ring_mismatches(tag + "on the device's data groups: ", view, cc.run_model(g["rec"], g["bytes"], **_cfg(j)), COUNTERS, "object")
        if g["cstats"]["objects_lost"] != 0 or g["cstats"]["active"] != 1 or g["cstats"]["dg_overrun"] != 0:
            bad.append(tag + "objects_lost / active / dg_overrun: %s" % g["cstats"])
    return bad


_runs = {}


def test_every_object_equals_the_model_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  k_carousel ran once per batch, behind k_packet."""
    streams = list(range(cc.N_STREAMS))
    eng = engine(len(streams), len(KINDS))
    try:
        got, cases = _drive(eng, streams, [[B] * len(streams)] * cc.N_BATCHES)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches, [g["cstats"] for g in got.values() if g["cstats"]["active"]])
    assert launches["k_carousel"] == cc.N_BATCHES + 1 == launches["k_packet"] == launches["k_mot"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
    bad = _mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    total = {k: sum(g["cstats"][k] for g in got.values()) for k in COUNTERS if k not in NEVER}
    assert all(v > 0 for v in total.values()), total                # every guard and every counter was exercised on the device
    flags = np.concatenate([g["objects"]["au"] for (i, j), g in got.items() if KINDS[j][1] == "car"])
    assert set(flags) == {0, dx.MOT_FLAG_DIR_ELEMENT}
    _runs["full"] = got


def test_objects_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """The boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): objects and directories stay open
    across batch ends and across batches in which a stream receives nothing.  k_msc_frame is the only decoder here; the results are also
    byte for byte those of the full-batch run."""
    streams = list(range(cc.N_STREAMS))
    schedule = pkc.boundary_schedule(len(streams), cc.N_FRAMES)
    eng = engine(len(streams), len(KINDS), fast_min=1 << 30, class_min=0)
    try:
        got, cases = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_carousel"] == len(schedule) + 1 == launches["k_packet"] == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, launches
    bad = _mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            f = _runs["full"][key]
            assert g["objects"].tobytes() == f["objects"].tobytes() and np.array_equal(g["object_bytes"], f["object_bytes"]) and g["cstats"] == f["cstats"], key
            assert g["rec"].tobytes() == f["rec"].tobytes() and np.array_equal(g["bytes"], f["bytes"]), key


def test_an_engine_that_never_enables_the_carousel_launches_nothing_and_gives_what_it_gives_with_it():
    """Stream 0 with packet mode, PAD and MOT on and the carousel never: zero k_carousel launches, dabx_get_carousel_stats all zero, nothing
    to read from the packet slots; data groups, logical frames and the MOT slot's objects are the models' and the oracle's -- and byte
    for byte those of the run with the carousel on."""
    eng = engine(1, len(KINDS))
    try:
        got, cases = _drive(eng, [0], [[B]] * cc.N_BATCHES, carousel=False)
        launches = kernel_launches(eng)
        nothing = [eng.read_mot_objects(0, j, 16) for j in _slots("car", "pkt", "plain")]
    finally:
        eng.close()
    assert launches["k_carousel"] == 0 and launches["k_packet"] == cc.N_BATCHES + 1 == launches["k_mot"], launches
    assert all(len(r) == 0 and len(b) == 0 for r, b in nothing)
    bad = _mismatches(got, cases, [0], carousel=False)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for (i, j), g in got.items():
            f = _runs["full"][(i, j)]
            assert g["rec"].tobytes() == f["rec"].tobytes() and np.array_equal(g["bytes"], f["bytes"]) and g["pstats"] == f["pstats"], j
            assert np.array_equal(g["frames"], f["frames"]) and np.array_equal(g["sf"], f["sf"]) and g["sfi"].tobytes() == f["sfi"].tobytes(), j
            if KINDS[j][1] == "mot":
                assert g["objects"].tobytes() == f["objects"].tobytes() and np.array_equal(g["object_bytes"], f["object_bytes"]) and g["mstats"] == f["mstats"]


def _single(layout, cifs, j, script, cuts=()):
    """One stream: packet mode on slot j from the start, script[b](eng) in front of batch b; after every batch the new data groups and the
    new objects (while the carousel is on) are taken.  cuts: further batch boundaries, in logical frames.  Returns (data groups, their
    bytes, per batch (carousel stats, new objects or None, bytes, first, first byte), group count in front of every batch, launches)."""
    eng = engine(1, len(layout))
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, j, cc.ADDRESS)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        groups, taken, before = packet_follower(layout[j].kbps), [], []
        objects = _follower()
        n = len(cifs) - H
        edges = sorted(set(range(0, n + 1, B)) | set(cuts) | {n})
        for b, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            if b in script:
                if script[b](eng) == "restart":
                    objects = _follower()
            before.append(eng.packet_stats(0, j)["dg_count"])
            dx.msc_inject(eng, 0, cifs[H + lo:H + hi])
            dx.msc_decode(eng, [hi - lo], B)
            groups.take(eng, 0, j)
            st = eng.carousel_stats(0, j)
            taken.append(objects.take(eng, 0, j) if st["active"] else (st, None, None, 0, 0))
        return groups.result() + (taken, before, kernel_launches(eng))
    finally:
        eng.close()


def _since(rec, by, first):
    """The data groups from group `first` on, byte_pos counted from the first of them."""
    r = rec[first:].copy()
    base = int(r["byte_pos"][0]) if len(r) else 0
    r["byte_pos"] -= base
    return r, by[base:]


def test_carousel_on_off_and_on_again_and_set_packet_mode_ends_it():
    """Stream 0's 64 kbit/s slot.  The carousel on for batch 0, off (NULL) for batch 1, on again from batch 2: the objects after each start
    are the model's on the data groups completed from then on (a slot that is switched on starts with an empty cache, in the middle of
    whatever is on air).  dabx_set_packet_mode in front of batch 6 ends the carousel decoding: the stats are all zero and nothing more is
    read, while the packet stage goes on."""
    layout, frames, cifs, want = cc.stream_case(0)
    j, cfg = 0, _cfg(0)
    script = {0: lambda eng: eng.set_carousel_mode(0, j, **cfg), 1: lambda eng: eng.set_carousel_mode(0, j, on=False),
              2: lambda eng: (eng.set_carousel_mode(0, j, **cfg), "restart")[1]}
    rec, by, taken, before, launches = _single(layout, cifs, j, script)
    assert launches["k_carousel"] == 1 + (cc.N_BATCHES - 2) and launches["k_packet"] == cc.N_BATCHES + 1, launches
    assert not any(taken[1][0].values()) and taken[1][1] is None
    dm = pkc.run_model(frames[j], cc.ADDRESS)
    assert rec.tobytes() == dm.records().tobytes() and np.array_equal(by, dm.all_bytes())
    for batches, upto in (((0,), before[1]), (range(2, cc.N_BATCHES), len(rec))):
        m = cc.run_model(*_since(rec[:upto], by, before[batches[0]]), **cfg)
        got = [taken[b] for b in batches if taken[b][1] is not None]
        objs, ob = np.concatenate([t[1] for t in got]), np.concatenate([t[2] for t in got])
        assert len(objs) >= 2 and objs.tobytes() == m.records().tobytes() and np.array_equal(ob, m.all_bytes()), batches
        st = taken[batches[-1]][0]
        assert all(st[k] == m.counters[k] for k in COUNTERS) and st["active"] == 1 and st["objects_lost"] == 0, (st, m.counters)

    def packet_again(eng):
        eng.set_carousel_mode(0, j, **cfg)
        eng.set_packet_mode(0, j, cc.ADDRESS)
    eng_script = {0: lambda eng: eng.set_carousel_mode(0, j, **cfg), 6: packet_again}
    eng = engine(1, len(layout))
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, j, cc.ADDRESS)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        active = []
        for b in range(cc.N_BATCHES):
            if b in eng_script:
                eng_script[b](eng)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            active.append(eng.carousel_stats(0, j))
        launches = kernel_launches(eng)
        late = eng.read_mot_objects(0, j, 16)
        pst = eng.packet_stats(0, j)
    finally:
        eng.close()
    assert launches["k_carousel"] == 6 and launches["k_packet"] == cc.N_BATCHES + 1, launches
    assert all(st["active"] == 1 for st in active[:6]) and all(not any(st.values()) for st in active[6:]) and len(late[0]) == 0 and pst["active"] == 1


def test_a_slot_that_moves_to_other_capacity_units_in_the_middle_of_an_object_loses_nothing_and_a_changed_one_loses_its_state():
    """dabx_set_subchannels with the carousel slot at other capacity units while the 4 096-byte object is under assembly: the slot "keeps
    decoding without interruption", and so do the packet and the carousel state -- every object equals the model's on the whole
    scenario.  Then the slot's protection level changes: a changed slot starts anew, without packet mode and carousel decoding."""
    kbps, groups, frames, cfg = cc.scenario("header", 0)
    old = dc.dabplus_layout([(64, pkc.PROT, 0), (kbps, pkc.PROT, 0)], dab_plus=[0, 0])
    new = dc.dabplus_layout([(64, pkc.PROT, 0), (kbps, pkc.PROT, 0)], dab_plus=[0, 0])
    new[1].cu_start = 400
    filler = pkc.scenario(64, 5, cc.N_FRAMES)
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    m = cc.model_of(pkc.run_model(frames, cc.ADDRESS), **cfg)
    r = m.records()
    done = int(r["frame"][r["body_len"] == 4096][0])
    cut = done - 10                                                   # the object takes more than 20 logical frames: the move falls inside it
    move = H + cut
    cifs = np.concatenate([c_old[:move], c_new[move:]])
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_packet_mode(0, 1, cc.ADDRESS)
        eng.set_carousel_mode(0, 1, **cfg)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        ring = _follower()
        edges = sorted(set(range(0, cc.N_FRAMES + 1, B)) | {cut})
        stored_at_move = None
        for lo, hi in zip(edges[:-1], edges[1:]):
            if lo == cut:
                stored_at_move = eng.carousel_stats(0, 1)["segments"]
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + lo:H + hi])
            dx.msc_decode(eng, [hi - lo], B)
            st = ring.take(eng, 0, 1)[0]
        rec, by = ring.result()
        changed = dc.dabplus_layout([(64, pkc.PROT, 0), (kbps, 2, 0)], dab_plus=[0, 0])
        eng.set_subchannels(changed, stream=0)
        after, after_pkt = eng.carousel_stats(0, 1), eng.packet_stats(0, 1)
    finally:
        eng.close()
    assert rec.tobytes() == r.tobytes() and np.array_equal(by, m.all_bytes()), (len(rec), len(r))
    assert all(st[k] == m.counters[k] for k in COUNTERS) and st["objects_lost"] == 0 and 0 < stored_at_move < st["segments"], (st, m.counters)
    assert not any(after.values()) and not any(after_pkt.values()), (after, after_pkt)


def test_set_carousel_mode_refuses_a_slot_that_is_not_in_packet_mode_and_sizes_out_of_range():
    layout = cc.stage_layout()
    eng = engine(1, len(KINDS) + 1)
    L = dx.load()
    fresh = dict(dict.fromkeys(dx.CAROUSEL_STATS.names, 0), active=1)
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_pad_mode(0, 3)
        for j in (0, 1, 3, 4, 5, 6, -1):                               # slots not in packet mode, a PAD slot, an empty slot, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_carousel_mode(0, j)
        with pytest.raises(dx.DabxError):
            eng.set_carousel_mode(1, 0)                                # no such stream
        eng.set_carousel_mode(0, 0, on=False)                          # NULL on a slot without carousel decoding: nothing to do
        eng.set_packet_mode(0, 0, cc.ADDRESS)
        for kw in (dict(max_object_bytes=255), dict(max_object_bytes=(4 << 20) + 1), dict(max_dir_objects=1010), dict(max_dir_bytes=255),
                   dict(max_dir_bytes=(1 << 20) + 1), dict(max_dir_bytes=0xFFFFFFFF)):
            with pytest.raises(dx.DabxError):
                eng.set_carousel_mode(0, 0, **kw)
        assert eng.carousel_stats(0, 0)["active"] == 0
        for kw in (dict(max_object_bytes=256, max_dir_objects=1, max_dir_bytes=256), dict(max_object_bytes=65536, max_dir_objects=1009, max_dir_bytes=1 << 20), {}):
            eng.set_carousel_mode(0, 0, **kw)
            assert eng.carousel_stats(0, 0) == fresh
        short = dx.CarouselConfig(size=4, max_object_bytes=1, max_dir_objects=5000, max_dir_bytes=1)      # the fields are read only when size covers them
        dx.check(L.dabx_set_carousel_mode(eng._h, 0, 0, C.byref(short)))
        eng.set_packet_mode(0, 0, cc.ADDRESS)                          # the packet stage restarts: carousel decoding ends
        assert eng.carousel_stats(0, 0)["active"] == 0 and eng.packet_stats(0, 0)["active"] == 1
        eng.set_carousel_mode(0, 0)
        eng.set_packet_mode(0, 0, None)                                # ... and so it does when packet mode is switched off
        assert eng.carousel_stats(0, 0)["active"] == 0 and eng.packet_stats(0, 0)["active"] == 0
        with pytest.raises(dx.DabxError):
            eng.set_carousel_mode(0, 0)
        eng.set_packet_mode(0, 2, cc.ADDRESS)                          # another packet slot changes the packet job table: slot 1 follows
        eng.set_packet_mode(0, 1, cc.ADDRESS)
        eng.set_carousel_mode(0, 1)
        eng.set_packet_mode(0, 0, cc.ADDRESS)
        assert eng.carousel_stats(0, 1)["active"] == 1 and eng.carousel_stats(0, 0)["active"] == 0 and eng.carousel_stats(0, 2)["active"] == 0
        with pytest.raises(dx.DabxError):
            eng.set_pad_mode(0, 1, source="mp2")                       # a slot is a PAD slot or a packet slot, never both
    finally:
        eng.close()


def test_object_rings_overrun_on_purpose_count_exactly_what_is_lost():
    """max_object_bytes 1 024: a byte ring of 32 KiB.  One object of 250 bytes and 300 further one-byte segments behind its last flag,
    each of which emits it again a byte longer, and nobody reads: at the end the newest objects that the rings still hold whole are
    returned -- the rule of out_ring.h restated in packet_cases.intact_window --, they are the model's newest, and every older one is
    counted in objects_lost -- once."""
    kbps, repeats = 64, 300
    groups = cc.overrun_groups(9, repeats)
    cfg = dict(max_object_bytes=1024, max_dir_objects=1, max_dir_bytes=256)
    w = cc.Writer(kbps, np.random.default_rng(9))
    for g in groups:
        w.emit(w.cut(g, cc.ADDRESS))
    w.pad_frame()
    n_frames = -(-len(w.frames) // B) * B
    while len(w.frames) < n_frames:
        w.pad(w.gran)
    frames = np.frombuffer(b"".join(w.frames), np.uint8).reshape(n_frames, 3 * kbps)
    layout = dc.dabplus_layout([(kbps, pkc.PROT, 0)], dab_plus=[0])
    cifs = dc.cifs_of(layout, [frames], np.random.default_rng(4))
    m = cc.model_of(pkc.run_model(frames, cc.ADDRESS), **cfg)
    assert len(m.rows) == repeats + 1 and len(m.payloads[-1]) == 250 + repeats
    eng = engine(1, 1)
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, 0, cc.ADDRESS)
        eng.set_carousel_mode(0, 0, **cfg)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        for b in range(n_frames // B):
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
        rec, by = eng.read_mot_objects(0, 0, 256, max_bytes=1 << 16)
        st = eng.carousel_stats(0, 0)
        rec2, by2 = eng.read_mot_objects(0, 0, 3, max_bytes=1 << 16)
        st2 = eng.carousel_stats(0, 0)
    finally:
        eng.close()
    all_rec, all_by = m.records(), m.all_bytes()
    _, first = pkc.intact_window(all_rec["byte_pos"], len(all_by), 256, 32768, asm_room=0)
    keep = len(all_rec) - first
    want = all_rec[first:].copy()
    base = int(want["byte_pos"][0])
    want["byte_pos"] -= base
    assert 50 < keep < 100 and len(rec) == keep and rec.tobytes() == want.tobytes() and np.array_equal(by, all_by[base:]), (keep, len(rec))
    assert st["objects"] == repeats + 1 and st["objects_lost"] == first and all(st[k] == m.counters[k] for k in COUNTERS), (st, m.counters)
    assert rec["repeat"].max() == 255 and rec["repeat"].min() > 200
    want3 = want[-3:].copy()
    b3 = int(want3["byte_pos"][0])
    want3["byte_pos"] -= b3
    assert len(rec2) == 3 and rec2.tobytes() == want3.tobytes() and np.array_equal(by2, by[b3:]) and st2 == st
