"""The AAC stream stage -- k_aac_stream as dabx_process launches it behind k_dabplus on the MSC batch's stream -- against the model of
tests/aac_stream_cases.py (bit_writer.cpp:29-59 and mp4processor.cpp:320-391, :395-445 restated bit by bit), built like
test_gpu_mp2_audio_stage.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen byte by byte (tests/aac_stream_cases.py lists it; test_aac_stream_cases.py proves
on the model that the scenarios reach every line).  Four streams, two layouts with slots at 8, 32, 64, 72, 192 and 384 kbit/s beside a DAB+
slot that has PAD decoding and the AAC stream mode, a DAB+ slot with PAD decoding only, an MP2 audio slot and a packet-mode slot.  After
EVERY batch the new records, their bytes and every dabx_aac_stream_stats field of every slot with the mode are compared with the model's
state after as many super frames, exactly -- records by .tobytes(), bytes by np.array_equal, counters by ==.  There is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import aac_stream_cases as ac
import dabplus_cases as dc
import pad_cases as pc
from dabstar_amd import lib as dx
from stage_driver import PAD_ITEMS, Follower, Ring, drive, engine, kernel_launches, oracle_mismatches, packet_follower

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH
AAC_FRAMES = Ring("aac_stream_stats", ("records",), ("frame_bytes",), "read_aac_frames", dx.AAC_FRAME)
MP2_AUDIO = Ring("mp2_audio_stats", ("frames_out",), ("pcm_bytes",), "read_mp2_audio", dx.MP2_AUDIO_FRAME)


def aac_follower(kbps):
    return Follower(AAC_FRAMES, 36, max_bytes=dx.aac_ring_bytes(kbps))       # a batch completes at most 6 super frames of at most 6 access units


_want = {}


def _wanted(m):
    """(records, bytes) of a model, computed once"""
    if id(m) not in _want:
        _want[id(m)] = (m, m.records(), m.all_bytes())
    return _want[id(m)][1:]


def batch_mismatches(tag, m, n_sf, taken, first_sf=0):
    """A slot after n_sf super frames against the model's snapshot: what its follower took (the new records and bytes, the stats)."""
    bad = []
    n_rec, n_bytes, counters = m.snaps[n_sf]
    st, rec, by, first, first_byte = taken
    for k in ac.COUNTERS:
        if st[k] != counters[k]:
            bad.append(tag + "after %d super frames %s = %d, the model's %d" % (n_sf, k, st[k], counters[k]))
    if st["lost"] != 0:
        bad.append(tag + "after %d super frames lost = %d" % (n_sf, st["lost"]))
    if first + (0 if rec is None else len(rec)) != n_rec:
        bad.append(tag + "after %d super frames %d records, the model has %d" % (n_sf, first + (0 if rec is None else len(rec)), n_rec))
    if rec is not None:
        want, stream = _wanted(m)
        if rec.tobytes() != want[first:n_rec].tobytes():
            d = [k for k in range(min(len(rec), n_rec - first)) if rec[k].tobytes() != want[first + k].tobytes()][:3]
            bad.append(tag + "after %d super frames the new records differ; first differences %s" % (n_sf, [(k, rec[k].tolist(), want[first + k].tolist()) for k in d]))
        w = stream[first_byte:n_bytes]
        if not np.array_equal(by, w):
            k = min(len(by), len(w))
            d = np.flatnonzero(by[:k] != w[:k])
            bad.append(tag + "after %d super frames the new bytes differ (%d, the model has %d; %d differ, the first at %d)" % (n_sf, len(by), len(w), len(d), d[0] if len(d) else k))
    return bad


def _switch_on(eng, i, s, aac=True):
    for j, (kbps, kind) in enumerate(ac.kinds(s)):
        if kind in ("pad", "aac+pad"):
            eng.set_pad_mode(i, j)
        elif kind == "pkt":
            eng.set_packet_mode(i, j, ac.PACKET_ADDRESS)
        elif kind == "mp2":
            eng.set_mp2_audio_mode(i, j)
        if ac.is_aac(kind) and aac:
            eng.set_aac_stream_mode(i, j)


def _state(eng, i, s):
    out = []
    for j, (kbps, kind) in enumerate(ac.kinds(s)):
        if ac.is_aac(kind):
            rec, by = eng.read_aac_frames(i, j, 8)
            out.append((sorted((k, v) for k, v in eng.aac_stream_stats(i, j).items() if k != "launches"), rec.tobytes(), by.tobytes()))      # (launches is the engine's)
    return out


def _drive(eng, streams, schedule, aac=True):
    cases = [ac.stream_case(s) for s in streams]
    followers = {}
    for i, s in enumerate(streams):
        for j, (kbps, kind) in enumerate(ac.kinds(s)):
            if ac.is_aac(kind) and aac:
                followers[(i, j)] = aac_follower(kbps)
            elif kind in ("pad", "aac+pad"):
                followers[(i, j)] = Follower(PAD_ITEMS, 144)
            elif kind == "pkt":
                followers[(i, j)] = packet_follower(kbps)
            elif kind == "mp2":
                followers[(i, j)] = Follower(MP2_AUDIO, B, max_bytes=B * dx.MP2_PCM_BYTES)
    bad = []

    def after_batch(i, n, taken):
        for j, (kbps, kind) in enumerate(ac.kinds(streams[i])):
            if ac.is_aac(kind) and aac:
                n_sf = eng.subch_stats(i, j)["sf_count"]         # the mode was switched on before the first super frame
                bad.extend(batch_mismatches("stream %d slot %d (%d kbit/s): " % (i, j, kbps), ac.slot_model(streams[i], j), n_sf, taken[j]))

    got = drive(eng, cases, schedule, lambda eng, i: _switch_on(eng, i, streams[i], aac), followers, lambda eng, i: _state(eng, i, streams[i]), after_batch)
    for (i, j), g in got.items():
        kbps, kind = ac.kinds(streams[i])[j]
        bad += oracle_mismatches("stream %d slot %d (%d kbit/s, %s): " % (i, j, kbps, kind), g, cases[i][3][j], cases[i][1][j])
        g["astats"] = eng.aac_stream_stats(i, j)
        g["pstats"], g["kstats"], g["mstats"] = eng.pad_stats(i, j), eng.packet_stats(i, j), eng.mp2_audio_stats(i, j)
        if kind == "aac+pad":
            g["pad"] = eng.read_pad_items(i, j, 512)
        if ac.is_aac(kind) and aac:
            m = ac.slot_model(streams[i], j)
            want, stream = _wanted(m)
            if g["rec"].tobytes() != want.tobytes() or not np.array_equal(g["bytes"], stream):
                bad.append("stream %d slot %d: the whole run's records or bytes differ from the model's" % (i, j))
        elif any(v for k, v in g["astats"].items() if k != "launches"):
            bad.append("stream %d slot %d (%s): the mode is off and the slot shows AAC stream results: %s" % (i, j, kind, g["astats"]))
    return got, cases, bad


_runs = {}


def test_every_slot_with_the_mode_equals_the_model_after_every_batch_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  k_aac_stream ran once per batch."""
    streams = list(range(len(ac.STAGE_STREAMS)))
    eng = engine(len(streams), ac.MAX_SUBCH)
    try:
        got, cases, bad = _drive(eng, streams, [[B] * len(streams)] * ac.N_BATCHES)
        launches = kernel_launches(eng)
        mine = eng.aac_stream_stats(0, 0)["launches"]
    finally:
        eng.close()
    print(launches, mine)
    assert mine == ac.N_BATCHES + 1 == launches["k_dabplus"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, (mine, launches)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    total = {k: sum(g["astats"][k] for (i, j), g in got.items() if ac.is_aac(ac.kinds(streams[i])[j][1])) for k in ac.COUNTERS}
    assert all(v > 0 for v in total.values()), total
    for (i, j), g in got.items():
        kbps, kind = ac.kinds(streams[i])[j]
        if ac.is_aac(kind):
            assert g["astats"]["frames"] > 60 and g["astats"]["lost"] == 0, (i, j, g["astats"])
        if (streams[i], j) in ac.OVERLAP_SLOTS:                      # the table out of order: more bytes than an in-order super frame can emit
            r = g["rec"]
            per_sf = {}
            for q in r:
                per_sf[int(q["first_frame"])] = per_sf.get(int(q["first_frame"]), 0) + int(q["length"])
            assert max(per_sf.values()) > 110 * (kbps // 8) + 72, (i, j)
        if kind == "mp2":
            assert g["mstats"]["frames_out"] > 20 and len(g["rec"]) == g["mstats"]["frames_out"], (i, j, g["mstats"])
    _runs["full"] = got


def test_super_frames_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """The boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): batches that complete no super
    frame, one, or six, and batches in which a stream receives nothing.  k_msc_frame is the only decoder here; the results are also byte
    for byte those of the full-batch run."""
    streams = list(range(len(ac.STAGE_STREAMS)))
    schedule = ac.boundary_schedule(len(streams))
    eng = engine(len(streams), ac.MAX_SUBCH, fast_min=1 << 30, class_min=0)
    try:
        got, cases, bad = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
        mine = eng.aac_stream_stats(0, 0)["launches"]
    finally:
        eng.close()
    print(launches, mine)
    assert mine == len(schedule) + 1 == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, (mine, launches)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            assert g["rec"].tobytes() == _runs["full"][key]["rec"].tobytes() and np.array_equal(g["bytes"], _runs["full"][key]["bytes"]), key


def test_pad_results_of_the_shared_slot_and_all_other_slots_equal_a_run_without_the_mode():
    """Streams 0 and 1 (both layouts) once more with the AAC stream mode off everywhere: the PAD items, bytes and dabx_pad_stats of the slot
    that has both modes, the items of the PAD-only slots, the PCM of the MP2 audio slot and the data groups of the packet-mode slot are
    exactly those of the run with the mode on, and so are all logical frames; without the mode nothing is launched and the profile's rows
    are what they are with it."""
    streams = [0, 1]
    runs, rows = [], []
    for aac in (True, False):
        eng = engine(len(streams), ac.MAX_SUBCH)
        try:
            got, cases, bad = _drive(eng, streams, [[B] * len(streams)] * ac.N_BATCHES, aac=aac)
            launches = eng.aac_stream_stats(0, 0)["launches"]
            rows.append(kernel_launches(eng))
        finally:
            eng.close()
        assert not bad, "\n".join(bad[:25])
        assert launches == (ac.N_BATCHES + 1 if aac else 0), launches
        runs.append(got)
    assert rows[0] == rows[1] and len(rows[0]) == 16 and not any("aac" in k for k in rows[0]), rows       # the profile table has no row for the stage
    n_shared = n_pad = n_pkt = n_mp2 = 0
    for (i, j), a in sorted(runs[0].items()):
        b = runs[1][(i, j)]
        kind = ac.kinds(streams[i])[j][1]
        assert np.array_equal(a["frames"], b["frames"]) and a["pstats"] == b["pstats"] and a["kstats"] == b["kstats"], (i, j)
        assert {k: v for k, v in a["mstats"].items() if k != "launches"} == {k: v for k, v in b["mstats"].items() if k != "launches"}, (i, j)
        if kind == "aac+pad":
            assert a["pad"][0].tobytes() == b["pad"][0].tobytes() and np.array_equal(a["pad"][1], b["pad"][1]), (i, j)
            assert a["pstats"]["active"] == 1 and a["pstats"]["aus"] > 50 and len(a["pad"][0]) > 0, (i, j, a["pstats"])
            o = cases[i][3][j]
            want = pc.run_model(o["sf"], o["sfi"])
            assert a["pstats"]["aus"] == want.counters["aus"] == a["astats"]["frames"], (a["pstats"], a["astats"])      # both stages take the same access units
            n_shared += 1
        elif kind in ("pad", "pkt", "mp2"):
            assert a["rec"].tobytes() == b["rec"].tobytes() and np.array_equal(a["bytes"], b["bytes"]) and len(a["rec"]) > 0, (i, j)
            n_pad += kind == "pad"; n_pkt += kind == "pkt"; n_mp2 += kind == "mp2"
    assert (n_shared, n_pad, n_pkt, n_mp2) == (1, 2, 1, 1)


def test_on_off_and_on_again_restarts_empty_and_no_slot_with_the_mode_launches_nothing():
    """Stream 1's layout on three engines.  The first never has the mode on: zero launches, all-zero stats, nothing to read, and the rows of
    dabx_get_profile count what they count with it.  The second has it on slots 0 and 1 throughout: one launch per batch.  The third has it
    on slot 1 for batches 0-1, off (NULL) for batches 2-3 and on again from batch 4: what is read after the second start is the model's on
    the super frames completed from then on (a slot that is switched on starts with empty rings and counts)."""
    s, j = 1, 1
    layout, frames, cifs, oracle = ac.stream_case(s)
    assert ac.kinds(s)[j] == (64, "aac")
    results = []
    for mode in ("never", "on", "toggled"):
        eng = engine(1, len(layout))
        try:
            eng.set_subchannels(layout, stream=0)
            dx.msc_inject(eng, 0, cifs[:H])
            dx.msc_decode(eng, [H], H)
            if mode == "on":
                eng.set_aac_stream_mode(0, 0); eng.set_aac_stream_mode(0, j)
            sf_at_start = 0
            for b in range(ac.N_BATCHES):
                if mode == "toggled" and b in (0, 2, 4):
                    eng.set_aac_stream_mode(0, j, on=b != 2)
                    sf_at_start = eng.subch_stats(0, j)["sf_count"]
                dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
                dx.msc_decode(eng, [B], B)
                if mode == "toggled" and b == 3:
                    st = eng.aac_stream_stats(0, j)
                    assert st["launches"] == 2 and not any(v for k, v in st.items() if k != "launches") and len(eng.read_aac_frames(0, j, 8)[0]) == 0, st
            results.append((eng.aac_stream_stats(0, j), eng.read_aac_frames(0, j, 128), kernel_launches(eng), sf_at_start))
        finally:
            eng.close()
    st, (rec, by), launches, _ = results[0]
    assert launches["k_dabplus"] == ac.N_BATCHES + 1 and not any(st.values()) and len(rec) == 0, (launches, st)
    assert launches == results[1][2], (launches, results[1][2])          # the rows of the profile are unchanged by the stage
    st, (rec, by), launches, _ = results[1]
    m = ac.slot_model(s, j)
    assert st["launches"] == ac.N_BATCHES and all(st[k] == m.counters[k] for k in ac.COUNTERS), (st, m.counters)
    st, (rec, by), launches, first = results[2]
    o = oracle[j]
    assert 0 < first < len(o["sf"]) - 10
    m = ac.run_model(o["sf"][first:], o["sfi"][first:])
    assert st["launches"] == 2 + (ac.N_BATCHES - 4) and m.counters["frames"] > 20, (st, m.counters)
    assert all(st[k] == m.counters[k] for k in ac.COUNTERS) and st["lost"] == 0, (st, m.counters)
    assert len(m.rows) <= 128 and rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes())


def test_a_slot_that_moves_to_other_capacity_units_loses_nothing_and_a_changed_slot_starts_anew_with_the_mode_off():
    """dabx_set_subchannels with the 64 kbit/s slot at other capacity units in the middle of the run: the slot "keeps decoding without
    interruption" and so does the stage -- every record and byte equals the model's on the whole scenario.  Then the slot's protection
    level changes: a changed slot starts anew, with the mode off."""
    kbps = 64
    frames = ac.scenario(kbps, 77)[0]
    old = dc.dabplus_layout([(32, ac.PROT, 0), (kbps, ac.PROT, 0)])
    new = dc.dabplus_layout([(32, ac.PROT, 0), (kbps, ac.PROT, 0)])
    new[1].cu_start = 400
    filler = ac.scenario(32, 78)[0]
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    o = dc.oracle_results(old, c_old)[1]
    m = ac.run_model(o["sf"], o["sfi"])
    b_move = 3
    move = H + b_move * B
    cifs = np.concatenate([c_old[:move], c_new[move:]])
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_aac_stream_mode(0, 1)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        ring, bad = aac_follower(kbps), []
        for b in range(ac.N_BATCHES):
            if b == b_move:
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            bad += batch_mismatches("batch %d: " % b, m, eng.subch_stats(0, 1)["sf_count"], ring.take(eng, 0, 1))
        eng.subch = list(new)
        last = eng.read_msc(0, 1, B)
        changed = dc.dabplus_layout([(32, ac.PROT, 0), (kbps, 2, 0)])
        eng.set_subchannels(changed, stream=0)
        after = eng.aac_stream_stats(0, 1)
        n_after = len(eng.read_aac_frames(0, 1, 8)[0])
    finally:
        eng.close()
    assert not bad, "\n".join(bad[:25])
    assert np.array_equal(last, frames[-B:]) and ring.seen == len(m.rows) > 100 and np.array_equal(ring.result()[1], m.all_bytes())
    assert ring.result()[0].tobytes() == m.records().tobytes()
    assert not any(v for k, v in after.items() if k != "launches") and n_after == 0, after


def test_the_refusals():
    """The mode is refused for a slot that is not DAB+, a packet-mode slot, an inactive slot and no slot at all; NULL for a slot whose mode
    is off is refused in the same cases and accepted for a DAB+ slot; format != 0, a reserved word that is not 0 and a configuration that
    cannot hold its fields are refused; a slot with the mode on does not become a packet-mode slot; the mode is independent of the slot's
    PAD mode, in either order."""
    layout = ac.stage_layout(0)                                       # 8 aac, 384 aac, 64 aac+pad, 32 pad, 48 mp2, 16 pkt
    eng = engine(1, 7)
    L = dx.load()
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, 5, ac.PACKET_ADDRESS)
        for j in (4, 5, 6, 7):                                        # a DAB audio slot, a packet-mode slot, a slot that is not configured, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_aac_stream_mode(0, j)
            with pytest.raises(dx.DabxError):
                eng.set_aac_stream_mode(0, j, on=False)
        with pytest.raises(dx.DabxError):
            eng.aac_stream_stats(0, 7)
        eng.set_aac_stream_mode(0, 0, on=False)                       # nothing to switch off: accepted for a slot that could have it
        assert not any(eng.aac_stream_stats(0, 0).values())
        for cfg in (dx.AacStreamConfig(size=32, format=1), dx.AacStreamConfig(size=32, format=-1), dx.AacStreamConfig(size=8, format=0),
                    dx.AacStreamConfig(size=2, format=0), dx.AacStreamConfig(size=32, format=0, reserved=(C.c_int32 * 6)(0, 0, 0, 0, 0, 1))):
            assert L.dabx_set_aac_stream_mode(eng._h, 0, 0, C.byref(cfg)) == -2, (cfg.size, cfg.format)
        assert not any(eng.aac_stream_stats(0, 0).values())
        eng.set_aac_stream_mode(0, 0)
        assert eng.aac_stream_stats(0, 0) == dict.fromkeys(dx.AAC_STREAM_STATS.names, 0)
        assert len(eng.read_aac_frames(0, 0, 8)[0]) == 0
        with pytest.raises(dx.DabxError, match="AAC stream mode|DAB\\+ slot"):
            eng.set_packet_mode(0, 0, 5)                              # the mode is on (and the slot is DAB+)
        eng.set_pad_mode(0, 0)                                        # PAD decoding beside it ...
        assert eng.pad_stats(0, 0)["active"] == 1
        eng.set_pad_mode(0, 0, on=False)                              # ... and gone again: the mode stays
        with pytest.raises(dx.DabxError):
            eng.set_packet_mode(0, 0, 5)
        eng.set_pad_mode(0, 2)                                        # ... and in the other order
        eng.set_aac_stream_mode(0, 2)
        eng.set_aac_stream_mode(0, 2, on=False)
        assert eng.pad_stats(0, 2)["active"] == 1
        eng.set_aac_stream_mode(0, 0, on=False)
        assert not any(eng.aac_stream_stats(0, 0).values())
        with pytest.raises(dx.DabxError):
            eng.set_packet_mode(0, 0, 5)                              # (a DAB+ slot never may)
    finally:
        eng.close()
