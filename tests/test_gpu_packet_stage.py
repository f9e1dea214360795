"""The packet-mode stage -- k_packet as dabx_process launches it behind the batched MSC decoder, in front of k_dabplus -- against the model of
tests/packet_cases.py (DataProcessor, data_processor.cpp:106-254, restated), built like test_gpu_dabplus_stage.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen byte by byte (tests/packet_cases.py lists it; test_packet_cases.py proves on the
model that the scenarios reach every branch and both guards).  Four streams, two layouts that mix packet-mode, DAB+ and plain slots at 8 ..
384 kbit/s, two packet addresses on the same kind of traffic.  After every batch the new records, bytes and counters of every packet slot are
read; at the end everything is compared with the model EXACTLY -- records by .tobytes(), bytes by np.array_equal, counters by == -- and the
logical frames of every slot and the super frames, records and counters of the DAB+ slots beside them with the oracle back end's."""
import ctypes as C

import numpy as np
import pytest

import dabplus_cases as dc
import packet_cases as pc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH
SF_COUNTERS = (("cifs_decoded", "cif_out"), ("sf_ok", "sf_ok"), ("sf_fail", "sf_fail"), ("rs_corrected", "rs_corr"), ("rs_failed", "rs_fail"),
               ("fc_corrected", "fc_corr"), ("au_ok", "au_ok"), ("au_bad", "au_bad"))


def _engine(n_streams, max_subch, fast_min=1, class_min=1):
    eng = dx.Engine(n_streams=n_streams, ring_frames=2, max_subch=max_subch, out_frames=1, msc_fast_min_jobs=fast_min, msc_class_min_jobs=class_min)
    dx.check(dx.load().dabx_set_profiling(eng._h, 1))
    return eng


def _kernel_launches(eng):
    ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)(); names = (C.c_char_p * 16)()
    nk = dx.check(dx.load().dabx_get_profile(eng._h, ms, cnt, names))
    return {names[i].decode(): int(cnt[i]) for i in range(nk)}


def _packet_slots(s):
    lay, address = pc.STAGE_STREAMS[s]
    return [(j, kbps, address) for j, (kbps, kind) in enumerate(pc.STAGE_LAYOUTS[lay]) if kind == "pkt"]


def _packet_state(eng, s):
    out = []
    for j, _, _ in _packet_slots(s):
        rec, by = eng.read_datagroups(s, j, 4)
        out.append((sorted(eng.packet_stats(s, j).items()), rec.tobytes(), by.tobytes()))
    return out


def _drive(eng, streams, schedule):
    """Configures streams (indices into pc.STAGE_STREAMS), 16 CIFs of history, then one MSC batch per row of `schedule`.  After every batch
    the new logical frames of every slot, the new super frames of the DAB+ slots and the new groups of the packet slots are read and
    appended; a stream that received nothing must hold byte for byte what it held."""
    cases = [pc.stream_case(s) for s in streams]
    S = len(streams)
    got = {}
    for i, s in enumerate(streams):
        layout, _, cifs, _ = cases[i]
        eng.set_subchannels(layout, stream=i)
        for j, kbps, address in _packet_slots(s):
            eng.set_packet_mode(i, j, address)
        dx.msc_inject(eng, i, cifs[:H])
        for j, sc in enumerate(layout):
            got[(i, j)] = {"frames": [], "sf": [], "sfi": [], "seen": 0, "rec": [], "bytes": [], "dg_seen": 0, "byte_seen": 0}
    dx.msc_decode(eng, [H] * S, H)
    at = [H] * S
    for counts in schedule:
        before = {i: _packet_state(eng, streams[i]) for i in range(S) if counts[i] == 0}
        for i in range(S):
            if counts[i]:
                dx.msc_inject(eng, i, cases[i][2][at[i]:at[i] + counts[i]])
        dx.msc_decode(eng, counts, B)
        for i, s in enumerate(streams):
            if counts[i] == 0:
                assert _packet_state(eng, s) == before[i], "stream %d received nothing in this batch and changed" % i
                continue
            at[i] += counts[i]
            layout = cases[i][0]
            eng.subch = list(layout)
            for j, sc in enumerate(layout):
                g = got[(i, j)]
                fr = eng.read_msc(i, j, counts[i])
                assert fr.shape[0] == counts[i], (i, j, fr.shape)
                g["frames"].append(fr)
                new = eng.subch_stats(i, j)["sf_count"] - g["seen"]
                if new:
                    g["sf"].append(eng.read_superframes(i, j, new)); g["sfi"].append(eng.read_superframe_info(i, j, new))
                g["seen"] += new
            for j, kbps, _ in _packet_slots(s):
                g = got[(i, j)]
                st = eng.packet_stats(i, j)
                new = st["dg_count"] - g["dg_seen"]
                assert 0 <= new <= B * (kbps // 8), (i, j, new)
                if new:
                    rec, by = eng.read_datagroups(i, j, new, max_bytes=B * (kbps // 8) * 127 + dx.DG_MAX_BYTES)
                    assert len(rec) == new and rec["byte_pos"][0] == 0 and len(by) == st["dg_bytes"] - g["byte_seen"], (i, j, new, len(rec), len(by))
                    rec = rec.copy()
                    rec["byte_pos"] += g["byte_seen"]
                    g["rec"].append(rec); g["bytes"].append(by)
                g["dg_seen"] += new
                g["byte_seen"] = st["dg_bytes"]
    for (i, j), g in got.items():
        sc = cases[i][0][j]
        g["frames"] = np.concatenate(g["frames"])
        g["sf"] = np.concatenate(g["sf"]) if g["sf"] else np.zeros((0, 110 * sc.kbps // 8), np.uint8)
        g["sfi"] = np.concatenate(g["sfi"]) if g["sfi"] else np.zeros(0, dx.SUPERFRAME_INFO)
        g["rec"] = np.concatenate(g["rec"]) if g["rec"] else np.zeros(0, dx.DATAGROUP_INFO)
        g["bytes"] = np.concatenate(g["bytes"]) if g["bytes"] else np.zeros(0, np.uint8)
        g["stats"] = eng.subch_stats(i, j)
        g["pstats"] = eng.packet_stats(i, j)
    return got, cases


def _mismatches(got, cases, streams):
    """Every difference between the device and the model / the oracle as a line that names the stream, the slot and the bit rate."""
    bad = []
    for (i, j), g in sorted(got.items()):
        s = streams[i]
        layout, frames, _, want = cases[i]
        kbps, kind = pc.STAGE_LAYOUTS[pc.STAGE_STREAMS[s][0]][j]
        tag = "stream %d slot %d (%d kbit/s, %s): " % (i, j, kbps, kind)
        o = want[j]
        # the soft bits decode to the intended frames, on the oracle and on the device; DAB+ results equal the oracle back end's
        if not np.array_equal(o["frames"], frames[j]):
            bad.append(tag + "the oracle's logical frames are not the intended ones")
        if not np.array_equal(g["frames"], o["frames"]):
            bad.append(tag + "logical frames differ from the oracle's")
        if g["sfi"].tobytes() != o["sfi"].tobytes() or not np.array_equal(g["sf"], o["sf"]):
            bad.append(tag + "super frames or their records differ from the oracle's (%d, the oracle has %d)" % (len(g["sfi"]), len(o["sfi"])))
        for mine, theirs in SF_COUNTERS:
            if g["stats"][mine] != o["stats"][theirs]:
                bad.append(tag + "%s = %d, the oracle's %d" % (mine, g["stats"][mine], o["stats"][theirs]))
        if kind != "pkt":
            if g["pstats"]["active"] or any(g["pstats"].values()) or len(g["rec"]):
                bad.append(tag + "not in packet mode and shows packet results: %s" % g["pstats"])
            continue
        m = pc.run_model(frames[j], pc.STAGE_STREAMS[s][1])
        if g["rec"].tobytes() != m.records().tobytes():
            d = [k for k in range(min(len(g["rec"]), len(m.rows))) if g["rec"][k].tobytes() != m.records()[k].tobytes()][:3]
            bad.append(tag + "%d records, the model has %d; first differences %s" % (len(g["rec"]), len(m.rows), [(k, g["rec"][k].tolist(), m.rows[k]) for k in d]))
        if not np.array_equal(g["bytes"], m.all_bytes()):
            bad.append(tag + "data-group bytes differ (%d, the model has %d)" % (len(g["bytes"]), len(m.all_bytes())))
        for k in pc.PACKET_COUNTERS:
            if g["pstats"][k] != m.counters[k]:
                bad.append(tag + "%s = %d, the model's %d" % (k, g["pstats"][k], m.counters[k]))
        if g["pstats"]["dg_lost"] != 0 or g["pstats"]["active"] != 1 or g["pstats"]["packet_address"] != pc.STAGE_STREAMS[s][1]:
            bad.append(tag + "dg_lost / active / packet_address: %s" % g["pstats"])
    return bad


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
    eng = _engine(len(streams), 5)
    try:
        got, cases = _drive(eng, streams, [[B] * len(streams)] * pc.N_BATCHES)
        launches = _kernel_launches(eng)
    finally:
        eng.close()
    print(launches, _totals(got))
    assert launches["k_packet"] == pc.N_BATCHES + 1 == launches["k_dabplus"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
    bad = _mismatches(got, cases, streams)
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
    eng = _engine(len(streams), 5, fast_min=1 << 30, class_min=0)
    try:
        got, cases = _drive(eng, streams, schedule)
        launches = _kernel_launches(eng)
    finally:
        eng.close()
    print(launches)
    assert launches["k_packet"] == len(schedule) + 1 == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, launches
    bad = _mismatches(got, cases, streams)
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
        eng = _engine(1, len(layout))
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
            launches = _kernel_launches(eng)
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
    eng = _engine(1, 2)
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
    eng = _engine(1, 6)
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
