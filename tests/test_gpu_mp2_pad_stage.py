"""The PAD stage's MP2 source -- k_pad_mp2 as dabx_process launches it beside k_pad on the MSC batch's stream -- against the model of
tests/mp2_pad_cases.py (mp2processor.cpp:250-285 and :611-747 restated bit by bit, on top of PadModel), built like test_gpu_pad_stage.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen bit by bit (tests/mp2_pad_cases.py lists it; test_mp2_pad_cases.py proves on the
model that the scenarios reach every line).  Four streams, two layouts that mix MP2 PAD slots at 8, 48, 56, 128 and 384 kbit/s with DAB+
PAD slots, a packet-mode slot and a plain slot.  After EVERY batch the new items, their bytes, every dabx_pad_stats counter and every
dabx_mp2_sync_stats field of every MP2 slot are compared with the model's state after as many logical frames, exactly -- records by
.tobytes(), bytes by np.array_equal, counters by ==."""
import ctypes as C

import numpy as np
import pytest

import dabplus_cases as dc
import mp2_pad_cases as mc
import packet_cases as pkc
import pad_cases as pc
from dabstar_amd import lib as dx
from stage_driver import PAD_ITEMS, Follower, drive, engine, kernel_launches, mp2_batch_mismatches, mp2_final_mismatches, packet_follower

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH


def _slots(s, *kinds):
    return [j for j, (_, kind) in enumerate(mc.kinds(s)) if kind in kinds]


def _state(eng, i, s):
    """Everything the stage holds for stream i, for "a stream that received nothing stays unchanged"."""
    out = []
    for j in _slots(s, "mp2", "pad"):
        rec, by = eng.read_pad_items(i, j, 4)
        out.append((sorted(eng.pad_stats(i, j).items()), sorted(eng.mp2_sync_stats(i, j).items()), rec.tobytes(), by.tobytes()))
    return out


def _switch_on(eng, i, s, mp2):
    for j, (kbps, kind) in enumerate(mc.kinds(s)):
        if kind == "pad":
            eng.set_pad_mode(i, j)
        elif kind == "mp2" and mp2:
            eng.set_pad_mode(i, j, source="mp2")
        elif kind == "pkt":
            eng.set_packet_mode(i, j, mc.PACKET_ADDRESS)


def _follower(kbps, kind):
    if kind == "pkt":
        return packet_follower(kbps)
    return Follower(PAD_ITEMS, 112 if kind == "mp2" else 144)      # pad_core.h: 28 logical frames, or 6 super frames x 6 AUs, x 4 sub-fields


def _drive(eng, streams, schedule, mp2=True):
    """stage_driver.drive on streams (indices into mc.STAGE_STREAMS).  After every batch the MP2 slots are compared with the model, the new
    logical frames of every slot, the new items of the DAB+ PAD slots and the new data groups of the packet slot are read and appended; a
    stream that received nothing must hold byte for byte what it held.  mp2 = False: the same streams with their MP2 slots left as plain
    slots."""
    cases = [mc.stream_case(s) for s in streams]
    followers = {(i, j): _follower(kbps, kind) for i, s in enumerate(streams) for j, (kbps, kind) in enumerate(mc.kinds(s))
                 if kind in ("pad", "pkt") or (kind == "mp2" and mp2)}
    bad = []

    def after_batch(i, n, taken):
        for j, (kbps, kind) in enumerate(mc.kinds(streams[i])):
            if kind == "mp2" and mp2:
                tag = "stream %d slot %d (%d kbit/s, %s): " % (i, j, kbps, kind)
                bad.extend(mp2_batch_mismatches(tag, mc.slot_model(streams[i], j), n, taken[j], eng.mp2_sync_stats(i, j)))

    got = drive(eng, cases, schedule, lambda eng, i: _switch_on(eng, i, streams[i], mp2), followers, lambda eng, i: _state(eng, i, streams[i]), after_batch)
    for (i, j), g in got.items():
        g["pstats"], g["sync"], g["kstats"] = eng.pad_stats(i, j), eng.mp2_sync_stats(i, j), eng.packet_stats(i, j)
        if mc.kinds(streams[i])[j][1] == "pkt":                     # the packet slot's groups are no PAD items
            g["dg"], g["dg_bytes"], g["rec"], g["bytes"] = g["rec"], g["bytes"], g["rec"][:0], g["bytes"][:0]
    return got, cases, bad


_runs = {}


def test_every_mp2_slot_equals_the_model_after_every_batch_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  The stage (k_pad and k_pad_mp2 inside one marker) ran once per
    batch."""
    streams = list(range(len(mc.STAGE_STREAMS)))
    eng = engine(len(streams), 5)
    try:
        got, cases, bad = _drive(eng, streams, [[B] * len(streams)] * mc.N_BATCHES)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_pad"] == mc.N_BATCHES + 1 == launches["k_dabplus"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
    bad += mp2_final_mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    total = {k: sum(g["pstats"][k] for (i, j), g in got.items() if mc.kinds(streams[i])[j][1] == "mp2") for k in pc.PAD_COUNTERS}
    assert all(v > 0 for v in total.values()), total                # every counter was exercised on the device by the MP2 slots alone
    _runs["full"] = got


def test_sync_and_items_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """The boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): sync words, headers, MP2 frames of
    two logical frames, labels and groups stay open across batch ends and across batches in which a stream receives nothing.  k_msc_frame is
    the only decoder here; the results are also byte for byte those of the full-batch run."""
    streams = list(range(len(mc.STAGE_STREAMS)))
    schedule = mc.boundary_schedule(len(streams))
    eng = engine(len(streams), 5, fast_min=1 << 30, class_min=0)
    try:
        got, cases, bad = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_pad"] == len(schedule) + 1 == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, launches
    bad += mp2_final_mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            assert g["rec"].tobytes() == _runs["full"][key]["rec"].tobytes() and np.array_equal(g["bytes"], _runs["full"][key]["bytes"]), key


def test_the_dabplus_pad_slots_and_the_packet_slot_give_what_they_give_without_any_mp2_source_slot():
    """Streams 0 and 1 (both layouts) once more with their MP2 slots left plain: the items, bytes and counters of the DAB+ PAD slots and the
    data groups and counters of the packet-mode slot are exactly those of the run with the MP2 source on, and so are all logical frames."""
    streams = [0, 1]
    runs = []
    for mp2 in (True, False):
        if mp2 and "full" in _runs:
            runs.append({k: g for k, g in _runs["full"].items() if k[0] in streams})
            continue
        eng = engine(len(streams), 5)
        try:
            got, cases, bad = _drive(eng, streams, [[B] * len(streams)] * mc.N_BATCHES, mp2=mp2)
        finally:
            eng.close()
        bad += mp2_final_mismatches(got, cases, streams, mp2=mp2)
        assert not bad, "\n".join(bad[:25])
        runs.append(got)
    n_pad = n_pkt = 0
    for (i, j), a in sorted(runs[0].items()):
        b = runs[1][(i, j)]
        kind = mc.kinds(streams[i])[j][1]
        assert np.array_equal(a["frames"], b["frames"]), (i, j)
        if kind == "pad":
            assert a["rec"].tobytes() == b["rec"].tobytes() and np.array_equal(a["bytes"], b["bytes"]) and a["pstats"] == b["pstats"] and len(a["rec"]) > 0, (i, j)
            n_pad += 1
        elif kind == "pkt":
            assert a["dg"].tobytes() == b["dg"].tobytes() and np.array_equal(a["dg_bytes"], b["dg_bytes"]) and a["kstats"] == b["kstats"] and len(a["dg"]) > 0, (i, j)
            n_pkt += 1
        elif kind == "mp2":
            assert not any(b["pstats"].values()) and not any(b["sync"].values()) and len(b["rec"]) == 0, (i, j, b["pstats"])
    assert n_pad == 2 and n_pkt == 1


def test_mp2_pad_on_off_and_on_again_leaves_the_logical_frames_the_oracles_and_the_launch_counts():
    """Stream 1's layout on three engines.  The first has no PAD slot of either source: dabx_get_profile shows zero launches of the stage,
    dabx_get_pad_stats and dabx_get_mp2_sync_stats are all zero.  The second has only MP2 source slots (0 and 2): one launch per batch.  The
    third has the MP2 source on slot 2 for batches 0-1, off (NULL) for batches 2-3 and on again from batch 4: the logical frames of every slot
    are the oracle's in all three, and the items after the second start are the model's on the frames from then on (a slot that is switched
    on starts with empty state, searching for sync)."""
    s, j = 1, 2
    layout, frames, cifs, want = mc.stream_case(s)
    assert mc.kinds(s)[j] == (128, "mp2")
    results = []
    for mode in ("never", "mp2 only", "toggled"):
        eng = engine(1, len(layout))
        try:
            eng.set_subchannels(layout, stream=0)
            dx.msc_inject(eng, 0, cifs[:H])
            dx.msc_decode(eng, [H], H)
            if mode == "mp2 only":
                eng.set_pad_mode(0, 0, source="mp2"); eng.set_pad_mode(0, j, source="mp2")
            got = [[] for _ in layout]
            for b in range(mc.N_BATCHES):
                if mode == "toggled" and b in (0, 2, 4):
                    eng.set_pad_mode(0, j, on=b != 2, source="mp2")
                dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
                dx.msc_decode(eng, [B], B)
                eng.subch = list(layout)
                for k in range(len(layout)):
                    got[k].append(eng.read_msc(0, k, B))
                if mode == "toggled" and b == 3:
                    assert eng.pad_stats(0, j)["active"] == 0 and not any(eng.mp2_sync_stats(0, j).values()) and len(eng.read_pad_items(0, j, 8)[0]) == 0
            for k in range(len(layout)):
                assert np.array_equal(np.concatenate(got[k]), want[k]["frames"]), (mode, k)
            results.append((eng.pad_stats(0, j), eng.mp2_sync_stats(0, j), eng.read_pad_items(0, j, 512), kernel_launches(eng)))
        finally:
            eng.close()
    st, sy, (rec, by), launches = results[0]
    assert launches["k_pad"] == 0 and launches["k_dabplus"] == mc.N_BATCHES + 1 and not any(st.values()) and not any(sy.values()) and len(rec) == 0, (launches, st, sy)
    st, sy, (rec, by), launches = results[1]
    m = mc.slot_model(s, j)
    assert launches["k_pad"] == mc.N_BATCHES and sy == m.sync_stats() and all(st[k] == m.pad.counters[k] for k in pc.PAD_COUNTERS), (launches, sy, st)
    st, sy, (rec, by), launches = results[2]
    assert launches["k_pad"] == 2 + (mc.N_BATCHES - 4), launches
    m = mc.run_model(128, frames[j][4 * B:], first=4 * B)
    assert m.pad.counters["labels"] > 0 and m.pad.counters["groups"] > 0 and rec.tobytes() == m.pad.records().tobytes() and np.array_equal(by, m.pad.all_bytes())
    assert all(st[k] == m.pad.counters[k] for k in pc.PAD_COUNTERS) and st["items_lost"] == 0 and st["active"] == 1 and sy == m.sync_stats(), (st, sy, m.sync_stats())


def test_an_mp2_slot_that_moves_to_other_capacity_units_in_the_middle_of_the_long_group_loses_nothing():
    """dabx_set_subchannels with the 384 kbit/s MP2 PAD slot at other capacity units while the 16 383-byte group is under assembly: the slot
    "keeps decoding without interruption", and so do the sync state and the PAD state -- every item equals the model's on the whole scenario.
    Then the slot's protection level changes: a changed slot starts anew, without PAD decoding."""
    kbps, seed = 384, mc.seed_of(0, 1)
    frames = mc.scenario(kbps, seed, 0)[0]
    old = dc.dabplus_layout([(64, mc.PROT, 0), (kbps, mc.PROT, 0)], dab_plus=[0, 0])
    new = dc.dabplus_layout([(64, mc.PROT, 0), (kbps, mc.PROT, 0)], dab_plus=[0, 0])
    new[1].cu_start = 400
    filler = pkc.scenario(64, 5, mc.N_FRAMES)
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    m = mc.run_model(kbps, frames)
    r = m.pad.records()
    done = int(r["frame"][(r["kind"] == dx.PAD_DATAGROUP) & (r["length"] == 16383)][0])
    b_move = (done - 20) // B
    assert done - 80 < b_move * B < done - 5, (done, b_move)          # the group takes 86 logical frames: the move falls inside it
    move = H + b_move * B
    cifs = np.concatenate([c_old[:move], c_new[move:]])
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_pad_mode(0, 1, source="mp2")
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        ring, bad = Follower(PAD_ITEMS, 112), []
        for b in range(mc.N_BATCHES):
            if b == b_move:
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            bad += mp2_batch_mismatches("batch %d: " % b, m, B * (b + 1), ring.take(eng, 0, 1), eng.mp2_sync_stats(0, 1))
        eng.subch = list(new)
        last = eng.read_msc(0, 1, B)
        changed = dc.dabplus_layout([(64, mc.PROT, 0), (kbps, 2, 0)], dab_plus=[0, 0])
        eng.set_subchannels(changed, stream=0)
        after, after_sync = eng.pad_stats(0, 1), eng.mp2_sync_stats(0, 1)
    finally:
        eng.close()
    assert not bad, "\n".join(bad[:25])
    assert np.array_equal(last, frames[-B:]) and ring.seen == len(m.pad.rows) and np.array_equal(ring.result()[1], m.pad.all_bytes())
    assert not any(after.values()) and not any(after_sync.values()), (after, after_sync)


def test_the_refusals():
    """Source MP2 is refused for a DAB+ slot, a packet-mode slot, an inactive slot and no slot at all; an unknown source is refused; source
    DAB+ on a plain slot is refused as before; a slot whose PAD decoding is on cannot become a packet-mode slot; a configuration too short to
    hold `source` means DAB+."""
    layout = mc.stage_layout(0)                                       # 8 mp2, 384 mp2, 64 DAB+, 16 pkt, 56 mp2
    eng = engine(1, 6)
    L = dx.load()
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, 3, mc.PACKET_ADDRESS)
        for j in (2, 3, 5, 6):                                        # a DAB+ slot, a packet-mode slot, a slot that is not configured, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_pad_mode(0, j, source="mp2")
        for src in (2, -1, 255):
            with pytest.raises(dx.DabxError):
                eng.set_pad_mode(0, 0, source=src)
            with pytest.raises(dx.DabxError):
                eng.set_pad_mode(0, 2, source=src)
        with pytest.raises(dx.DabxError):
            eng.set_pad_mode(0, 0)                                    # source DAB+ on a plain slot: refused as before
        with pytest.raises(dx.DabxError):
            eng.set_pad_mode(0, 0, on=False)                          # ... and so is NULL for it
        assert eng.pad_stats(0, 0)["active"] == 0 and not any(eng.mp2_sync_stats(0, 0).values())
        eng.set_pad_mode(0, 0, source="mp2")
        assert eng.pad_stats(0, 0)["active"] == 1
        assert eng.mp2_sync_stats(0, 0) == dict(syncs=0, frames=0, hdr_refused=0, rate_unsupported=0, sample_rate=48000, state=0, bit_count=0,
                                                header_count=0, last_sync_bit=-1, active=1)
        with pytest.raises(dx.DabxError):
            eng.set_packet_mode(0, 0, 5)                              # PAD decoding is on
        eng.set_pad_mode(0, 0, on=False)                              # NULL switches an MP2 source slot off
        assert eng.pad_stats(0, 0)["active"] == 0 and not any(eng.mp2_sync_stats(0, 0).values())
        eng.set_packet_mode(0, 0, 5)                                  # ... and now it may
        with pytest.raises(dx.DabxError):
            eng.set_pad_mode(0, 0, source="mp2")
        eng.set_packet_mode(0, 0, None)
        short = dx.PadConfig(size=4, source=1)                        # `source` is read only when size >= 8
        dx.check(L.dabx_set_pad_mode(eng._h, 0, 2, C.byref(short)))
        assert eng.pad_stats(0, 2)["active"] == 1 and not any(eng.mp2_sync_stats(0, 2).values())
        with pytest.raises(dx.DabxError):
            dx.check(L.dabx_set_pad_mode(eng._h, 0, 1, C.byref(short)))      # ... so this asks for DAB+ PAD on a plain slot
        with pytest.raises(dx.DabxError):
            eng.set_packet_mode(0, 2, 5)                              # a DAB+ slot, PAD or not
    finally:
        eng.close()
