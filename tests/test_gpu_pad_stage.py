"""The PAD stage -- k_pad as dabx_process launches it behind k_dabplus on the MSC batch's stream -- against the model of tests/pad_cases.py
(mp4processor.cpp:345-353 and PadHandler, pad_handler.cpp:67-547, restated), built like test_gpu_packet_stage.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen byte by byte (tests/pad_cases.py lists it; test_pad_cases.py proves on the model
that the scenarios reach every branch and each side of every guard).  Four streams, two layouts that mix PAD-enabled DAB+ slots, plain DAB+
slots, a packet-mode slot and a plain slot at 8 .. 192 kbit/s.  After every batch the new items, bytes and counters of every PAD slot are
read; at the end everything is compared with the model EXACTLY -- records by .tobytes(), bytes by np.array_equal, counters by == -- and the
logical frames, super frames, records and counters of every slot with the oracle back end's."""
import numpy as np
import pytest

import dabplus_cases as dc
import packet_cases as pkc
import pad_cases as pc
from dabstar_amd import lib as dx
from stage_driver import PAD_ITEMS, Follower, drive, engine, kernel_launches, oracle_mismatches, pad_mismatches

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH


def _kinds(s):
    return pc.STAGE_LAYOUTS[pc.STAGE_STREAMS[s]]


def _pad_slots(s):
    return [j for j, (_, kind) in enumerate(_kinds(s)) if kind == "pad"]


def _pad_state(eng, i, s):
    out = []
    for j in _pad_slots(s):
        rec, by = eng.read_pad_items(i, j, 4)
        out.append((sorted(eng.pad_stats(i, j).items()), rec.tobytes(), by.tobytes()))
    return out


def _switch_on(eng, i, s):
    for j, (kbps, kind) in enumerate(_kinds(s)):
        if kind == "pad":
            eng.set_pad_mode(i, j)
        elif kind == "pkt":
            eng.set_packet_mode(i, j, pc.PACKET_ADDRESS)


def _drive(eng, streams, schedule):
    """stage_driver.drive on streams (indices into pc.STAGE_STREAMS) with their PAD slots followed: after every batch the new logical
    frames and super frames of every slot and the new items of the PAD slots are read and appended; a stream that received nothing must
    hold byte for byte what it held."""
    cases = [pc.stream_case(s) for s in streams]
    followers = {(i, j): Follower(PAD_ITEMS, 144) for i, s in enumerate(streams) for j in _pad_slots(s)}       # pad_core.h: 6 super frames x 6 AUs x 4 sub-fields
    got = drive(eng, cases, schedule, lambda eng, i: _switch_on(eng, i, streams[i]), followers, lambda eng, i: _pad_state(eng, i, streams[i]))
    for (i, j), g in got.items():
        g["pstats"] = eng.pad_stats(i, j)
    return got, cases


def _totals(got):
    t = dict.fromkeys(pc.PAD_COUNTERS, 0)
    for g in got.values():
        for k in t:
            t[k] += g["pstats"][k]
    return t


_runs = {}


def test_every_stream_and_slot_equals_the_model_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  k_pad ran once per batch."""
    streams = list(range(len(pc.STAGE_STREAMS)))
    eng = engine(len(streams), 5)
    try:
        got, cases = _drive(eng, streams, [[B] * len(streams)] * pc.N_BATCHES)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches, _totals(got))
    assert launches["k_pad"] == pc.N_BATCHES + 1 == launches["k_dabplus"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
    bad = pad_mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    assert all(v > 0 for v in _totals(got).values()), _totals(got)          # every guard and every counter was exercised on the device
    _runs["full"] = got


def test_items_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """The boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): labels and groups stay open across
    batch ends and across batches in which a stream receives nothing, so PadHandler's state, the text and the group under assembly are
    carried from launch to launch.  k_msc_frame is the only decoder here; the results are also byte for byte those of the full-batch run."""
    streams = list(range(len(pc.STAGE_STREAMS)))
    schedule = pc.boundary_schedule(len(streams))
    eng = engine(len(streams), 5, fast_min=1 << 30, class_min=0)
    try:
        got, cases = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_pad"] == len(schedule) + 1 == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, launches
    bad = pad_mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            assert g["rec"].tobytes() == _runs["full"][key]["rec"].tobytes() and np.array_equal(g["bytes"], _runs["full"][key]["bytes"]), key


def test_pad_on_off_and_on_again_leaves_every_result_the_oracles_and_no_pad_slot_means_no_launch():
    """Stream 1's layout on two engines.  The first never enables PAD: dabx_get_profile shows zero k_pad launches, dabx_get_pad_stats is all
    zero and dabx_read_pad_items returns nothing.  The second has PAD on slot 2 for batches 0-1, off (NULL) for batches 2-3 and on again from
    batch 4: logical frames, super frames, dabx_superframe_info and dabx_subch_stats of every slot are the oracle's in both, and the items
    after the second start are the model's on the super frames completed from then on (a slot that is switched on starts with empty state)."""
    s, j = 1, 2
    layout, frames, cifs, want = pc.stream_case(s)
    assert _kinds(s)[j] == (64, "pad")
    results = []
    for toggle in (False, True):
        eng = engine(1, len(layout))
        try:
            eng.set_subchannels(layout, stream=0)
            dx.msc_inject(eng, 0, cifs[:H])
            dx.msc_decode(eng, [H], H)
            got = {k: {"frames": [], "sf": [], "sfi": [], "seen": 0} for k in range(len(layout))}
            sf_at_start = None
            for b in range(pc.N_BATCHES):
                if toggle and b in (0, 2, 4):
                    eng.set_pad_mode(0, j, on=b != 2)
                    if b == 4:
                        eng.subch = list(layout)
                        sf_at_start = eng.subch_stats(0, j)["sf_count"]
                dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
                dx.msc_decode(eng, [B], B)
                eng.subch = list(layout)
                for k in range(len(layout)):
                    g = got[k]
                    g["frames"].append(eng.read_msc(0, k, B))
                    new = eng.subch_stats(0, k)["sf_count"] - g["seen"]
                    if new:
                        g["sf"].append(eng.read_superframes(0, k, new)); g["sfi"].append(eng.read_superframe_info(0, k, new))
                    g["seen"] += new
                if toggle and b == 3:
                    assert eng.pad_stats(0, j)["active"] == 0 and len(eng.read_pad_items(0, j, 8)[0]) == 0
            for k, g in got.items():
                g["frames"] = np.concatenate(g["frames"])
                g["sf"] = np.concatenate(g["sf"]) if g["sf"] else np.zeros((0, 110 * layout[k].kbps // 8), np.uint8)
                g["sfi"] = np.concatenate(g["sfi"]) if g["sfi"] else np.zeros(0, dx.SUPERFRAME_INFO)
                g["stats"] = eng.subch_stats(0, k)
            st, (rec, by) = eng.pad_stats(0, j), eng.read_pad_items(0, j, 512)
            launches = kernel_launches(eng)
        finally:
            eng.close()
        bad = [line for k, g in got.items() for line in oracle_mismatches("PAD %s, slot %d: " % ("toggled" if toggle else "never on", k), g, want[k], frames[k])]
        assert not bad, "\n".join(bad)
        results.append((st, rec, by, launches, sf_at_start))
    st, rec, by, launches, _ = results[0]
    assert launches["k_pad"] == 0 and launches["k_dabplus"] == pc.N_BATCHES + 1 and not any(st.values()) and len(rec) == 0 and len(by) == 0, (launches, st)
    st, rec, by, launches, n0 = results[1]
    assert launches["k_pad"] == 2 + (pc.N_BATCHES - 4), launches
    m = pc.run_model(want[j]["sf"][n0:], want[j]["sfi"][n0:])
    assert m.counters["labels"] > 0 and m.counters["groups"] > 0 and rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes())
    assert all(st[k] == m.counters[k] for k in pc.PAD_COUNTERS) and st["items_lost"] == 0 and st["active"] == 1, (st, m.counters)


def test_a_slot_that_moves_to_other_capacity_units_in_the_middle_of_a_group_loses_nothing_and_a_changed_one_loses_its_state():
    """dabx_set_subchannels with the PAD slot at other capacity units while the 16 383-byte group is under assembly: the slot "keeps
    decoding without interruption", and so does the PAD state -- every item equals the model's on the whole scenario.  Then the slot's
    protection level changes: a changed slot starts anew, without PAD decoding."""
    kbps, seed = 192, pc.seed_of(1, 0)
    frames = pc.scenario(kbps, seed)[0]
    old = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, pc.PROT, 0)], dab_plus=[0, 1])
    new = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, pc.PROT, 0)], dab_plus=[0, 1])
    new[1].cu_start = 400
    filler = pkc.scenario(64, 5, pc.N_FRAMES)
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    o = dc.oracle_results(old, c_old)[1]
    m = pc.run_model(o["sf"], o["sfi"])
    r = m.records()
    done = int(r["frame"][(r["kind"] == dx.PAD_DATAGROUP) & (r["length"] == 16383)][0])      # it took 75 logical frames
    b_move = (done - 20) // B
    assert done - 70 < b_move * B < done - 5, (done, b_move)
    move = H + b_move * B                                             # the CIF from which the sub-channel is at its new place
    cifs = np.concatenate([c_old[:move], c_new[move:]])
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_pad_mode(0, 1)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        ring = Follower(PAD_ITEMS, 144)
        for b in range(pc.N_BATCHES):
            if b == b_move:
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            st = ring.take(eng, 0, 1)[0]
        rec, by = ring.result()
        eng.subch = list(new)
        last = eng.read_msc(0, 1, B)
        changed = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, 2, 0)], dab_plus=[0, 1])
        eng.set_subchannels(changed, stream=0)
        after = eng.pad_stats(0, 1)
    finally:
        eng.close()
    assert np.array_equal(last, frames[-B:])
    assert st["labels"] + st["groups"] == len(m.rows) and st["items_lost"] == 0, (st, len(m.rows))
    assert np.array_equal(rec["length"], r["length"]) and np.array_equal(by, m.all_bytes())
    assert all(st[k] == m.counters[k] for k in pc.PAD_COUNTERS), (st, m.counters)
    assert after["active"] == 0 and not any(after.values()), after


def test_set_pad_mode_refuses_an_inactive_a_non_dabplus_and_a_packet_mode_slot():
    layout = pc.stage_layout(0)
    eng = engine(1, 6)
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, 3, pc.PACKET_ADDRESS)
        for j in (3, 5, 6):                                            # a packet-mode slot (not DAB+), a slot that is not configured, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_pad_mode(0, j)
        plain = pc.stage_layout(1)
        eng.set_subchannels(plain, stream=0)
        with pytest.raises(dx.DabxError):
            eng.set_pad_mode(0, 1)                                     # a plain slot: dab_plus == 0
        eng.set_pad_mode(0, 4, on=False)                               # NULL on a slot without PAD decoding: nothing to do
        eng.set_pad_mode(0, 4)                                         # the "dab+" slot of the layout: any DAB+ slot may have it
        assert eng.pad_stats(0, 4)["active"] == 1 and eng.pad_stats(0, 0)["active"] == 0
        with pytest.raises(dx.DabxError):
            eng.set_packet_mode(0, 4, 5)                               # ... and a DAB+ slot is no packet-mode slot
    finally:
        eng.close()
