"""The packet-mode stage -- k_packet as dabx_process launches it behind the batched MSC decoder, in front of k_dabplus -- against the model of
tests/packet_cases.py (DataProcessor, data_processor.cpp:106-254, restated), built like test_gpu_dabplus_stage.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen byte by byte (tests/packet_cases.py lists it; test_packet_cases.py proves on the
model that the scenarios reach every branch and both guards).  Four streams, two layouts that mix packet-mode, DAB+ and plain slots at 8 ..
384 kbit/s, two packet addresses on the same kind of traffic.  After every batch the new records, bytes and counters of every packet slot are
read; at the end everything is compared with the model EXACTLY -- records by .tobytes(), bytes by np.array_equal, counters by == -- and the
logical frames of every slot and the super frames, records and counters of the DAB+ slots beside them with the oracle back end's."""
import numpy as np
import pytest

import dabplus_cases as dc
import packet_cases as pc
from dabstar_amd import lib as dx
from stage_driver import drive, engine, kernel_launches, packet_follower, packet_mismatches

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH


def _packet_slots(s):
    lay, address = pc.STAGE_STREAMS[s]
    return [(j, kbps, address) for j, (kbps, kind) in enumerate(pc.STAGE_LAYOUTS[lay]) if kind == "pkt"]


def _packet_state(eng, i, s):
    out = []
    for j, _, _ in _packet_slots(s):
        rec, by = eng.read_datagroups(i, j, 4)
        out.append((sorted(eng.packet_stats(i, j).items()), rec.tobytes(), by.tobytes()))
    return out


def _drive(eng, streams, schedule):
    """stage_driver.drive on streams (indices into pc.STAGE_STREAMS) with their packet slots switched on and followed: after every batch
    the new logical frames of every slot, the new super frames of the DAB+ slots and the new groups of the packet slots are read and
    appended; a stream that received nothing must hold byte for byte what it held."""
    cases = [pc.stream_case(s) for s in streams]

    def switch_on(eng, i):
        for j, _, address in _packet_slots(streams[i]):
            eng.set_packet_mode(i, j, address)

    followers = {(i, j): packet_follower(kbps) for i, s in enumerate(streams) for j, kbps, _ in _packet_slots(s)}
    got = drive(eng, cases, schedule, switch_on, followers, lambda eng, i: _packet_state(eng, i, streams[i]))
    for (i, j), g in got.items():
        g["pstats"] = eng.packet_stats(i, j)
    return got, cases


def _totals(got):
    t = dict.fromkeys(pc.PACKET_COUNTERS, 0)
    for g in got.values():
        for k in t:
            t[k] += g["pstats"][k]
    return t


_runs = {}


def test_every_stream_and_slot_equals_the_model_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  k_packet ran once per batch."""
    streams = list(range(len(pc.STAGE_STREAMS)))
    eng = engine(len(streams), 5)
    try:
        got, cases = _drive(eng, streams, [[B] * len(streams)] * pc.N_BATCHES)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches, _totals(got))
    assert launches["k_packet"] == pc.N_BATCHES + 1 == launches["k_dabplus"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
    bad = packet_mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    assert all(v > 0 for v in _totals(got).values()), _totals(got)          # both guards and every counter were exercised on the device
    _runs["full"] = got


def test_groups_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """The boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): series stay open across batch
    ends and across batches in which a stream receives nothing (asserted on the model in test_packet_cases.py), so the expected index, the
    series state, its fill, CRC register and first frame are carried from launch to launch.  k_msc_frame is the only decoder here; the
    results are also byte for byte those of the full-batch run behind the other decoder."""
    streams = list(range(len(pc.STAGE_STREAMS)))
    schedule = pc.boundary_schedule(len(streams))
    eng = engine(len(streams), 5, fast_min=1 << 30, class_min=0)
    try:
        got, cases = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_packet"] == len(schedule) + 1 == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, launches
    bad = packet_mismatches(got, cases, streams)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            assert g["rec"].tobytes() == _runs["full"][key]["rec"].tobytes() and np.array_equal(g["bytes"], _runs["full"][key]["bytes"]), key


def test_packet_mode_on_and_off_leaves_the_logical_frames_untouched_and_no_packet_slot_means_no_launch():
    """Stream 2's layout on two engines.  The first never switches a slot to packet mode: dabx_get_profile shows zero k_packet launches,
    dabx_get_packet_stats is all zero and dabx_read_datagroups returns nothing.  The second switches slot 1 on before batch 1, off (NULL)
    before batch 2 and on again, with another address, before batch 3: the logical frames of every slot are the oracle's in both, and the
    third batch's groups are the model's on those 28 frames alone (a slot that is switched on starts with empty state)."""
    s = 2
    layout, frames, cifs, want = pc.stream_case(s)
    j, kbps = 1, 64
    assert pc.STAGE_LAYOUTS[pc.STAGE_STREAMS[s][0]][j] == (kbps, "pkt")
    results = []
    for toggle in (False, True):
        eng = engine(1, len(layout))
        try:
            eng.set_subchannels(layout, stream=0)
            dx.msc_inject(eng, 0, cifs[:H])
            dx.msc_decode(eng, [H], H)
            out = []
            for b in range(3):
                if toggle:
                    eng.set_packet_mode(0, j, (pc.ADDRESS_B, None, pc.ADDRESS_A)[b])
                dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
                dx.msc_decode(eng, [B], B)
                eng.subch = list(layout)
                out.append([eng.read_msc(0, k, B) for k in range(len(layout))])
                if toggle and b == 1:
                    assert eng.packet_stats(0, j)["active"] == 0 and len(eng.read_datagroups(0, j, 8)[0]) == 0
            st, (rec, by) = eng.packet_stats(0, j), eng.read_datagroups(0, j, 4096, max_bytes=1 << 20)
            launches = kernel_launches(eng)
        finally:
            eng.close()
        for b in range(3):
            for k in range(len(layout)):
                assert np.array_equal(out[b][k], want[k]["frames"][B * b:B * (b + 1)]), (toggle, b, k)
        results.append((st, rec, by, launches))
    st, rec, by, launches = results[0]
    assert launches["k_packet"] == 0 and launches["k_dabplus"] == 4 and not any(st.values()) and len(rec) == 0 and len(by) == 0, (launches, st)
    st, rec, by, launches = results[1]
    assert launches["k_packet"] == 2, launches                       # batches 1 and 3
    m = pc.run_model(frames[j][2 * B:3 * B], pc.ADDRESS_A, first_frame=2 * B)
    assert m.counters["dg_count"] > 0 and rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes())
    assert all(st[k] == m.counters[k] for k in pc.PACKET_COUNTERS) and st["dg_lost"] == 0 and st["packet_address"] == pc.ADDRESS_A, (st, m.counters)


def test_a_slot_that_moves_to_other_capacity_units_keeps_its_assembly_and_a_changed_one_loses_it():
    """dabx_set_subchannels with the packet slot at other capacity units in the middle of the scenario (series open, a long group under
    way): the slot "keeps decoding without interruption", and so do the packet walk and the assembly -- every group equals the model's on
    the whole scenario.  Then the slot's protection level changes: a changed slot starts anew and is back in plain logical frames."""
    kbps, address, seed = 32, pc.ADDRESS_A, pc.seed_of(3, 2)
    frames = pc.scenario(kbps, seed)
    old = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, pc.PROT, 0)], dab_plus=[0, 0])
    new = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, pc.PROT, 0)], dab_plus=[0, 0])
    new[1].cu_start = 400
    filler = pc.scenario(64, 5)
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    move = H + 2 * B                                                  # the CIF from which the sub-channel is at its new place
    cifs = np.concatenate([c_old[:move], c_new[move:]])
    m = pc.run_model(frames, address)
    r = m.records()
    assert ((r["first_frame"] < 2 * B) & (r["last_frame"] >= 2 * B)).any()          # a group is under way at the move
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_packet_mode(0, 1, address)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        for b in range(pc.N_BATCHES):
            if b == 2:
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
        eng.subch = list(new)
        st = eng.packet_stats(0, 1)
        rec, by = eng.read_datagroups(0, 1, 4096, max_bytes=1 << 20)
        last = eng.read_msc(0, 1, B)
        changed = dc.dabplus_layout([(64, pc.PROT, 0), (kbps, 2, 0)], dab_plus=[0, 0])
        eng.set_subchannels(changed, stream=0)
        after = eng.packet_stats(0, 1)
    finally:
        eng.close()
    assert np.array_equal(last, frames[-B:])
    assert st["dg_count"] == len(rec) == len(m.rows) and st["dg_lost"] == 0, (st, len(rec), len(m.rows))
    assert rec.tobytes() == r.tobytes() and np.array_equal(by, m.all_bytes())
    assert all(st[k] == m.counters[k] for k in pc.PACKET_COUNTERS), (st, m.counters)
    assert after["active"] == 0 and not any(after.values()), after


def test_set_packet_mode_refuses_what_it_cannot_walk():
    layout = pc.stage_layout(0)
    eng = engine(1, 6)
    try:
        eng.set_subchannels(layout, stream=0)
        for j, address in ((1, 5), (5, 5), (0, 1024), (0, -1), (6, 5)):           # a DAB+ slot, a slot that is not configured, addresses out of range, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_packet_mode(0, j, address)
        eng.set_packet_mode(0, 3, None)                                         # NULL on a slot that is not in packet mode: nothing to do
        eng.set_packet_mode(0, 0, 1023)
        assert eng.packet_stats(0, 0)["active"] == 1 and eng.packet_stats(0, 0)["packet_address"] == 1023 and eng.packet_stats(0, 3)["active"] == 0
    finally:
        eng.close()
