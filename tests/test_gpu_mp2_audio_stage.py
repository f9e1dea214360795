"""The MP2 audio stage -- k_mp2_audio as dabx_process launches it behind k_dabplus on the MSC batch's stream -- against the model of
tests/mp2_audio_cases.py (mp2processor.cpp:197-243, :292-609 and :678-763 restated bit by bit), built like test_gpu_mp2_pad_stage.py.

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode) and decode to exactly the
intended logical frames, so what the stage sees is chosen bit by bit (tests/mp2_audio_cases.py lists it; test_mp2_audio_cases.py proves on
the model that the scenarios reach every line).  Four streams, two layouts with audio slots at 8, 48, 56, 96, 128 and 384 kbit/s beside a
DAB+ PAD slot, a packet-mode slot and -- on the 56 and 128 kbit/s audio slots themselves -- PAD decoding from the MP2 frames.  After EVERY
batch the new records, their PCM and every dabx_mp2_audio_stats field of every audio slot are compared with the model's state after as many
logical frames, exactly -- records by .tobytes(), PCM by np.array_equal, counters by ==.  There is no tolerance anywhere."""
import numpy as np
import pytest

import dabplus_cases as dc
import mp2_audio_cases as ac
import packet_cases as pkc
from dabstar_amd import lib as dx
from stage_driver import PAD_ITEMS, Follower, Ring, drive, engine, kernel_launches, packet_follower

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH
MP2_AUDIO = Ring("mp2_audio_stats", ("frames_out",), ("pcm_bytes",), "read_mp2_audio", dx.MP2_AUDIO_FRAME)


def audio_follower():
    return Follower(MP2_AUDIO, B, max_bytes=B * dx.MP2_PCM_BYTES)         # a logical frame completes at most one MP2 frame


_want = {}


def _wanted(m):
    """(records, PCM bytes) of a model, computed once"""
    if id(m) not in _want:
        _want[id(m)] = (m, m.records(), m.all_pcm())
    return _want[id(m)][1:]


def batch_mismatches(tag, m, n, taken):
    """An audio slot after n logical frames against the model's snapshot: what its follower took (the new records and PCM, the stats)."""
    bad = []
    n_rec, stats = m.snaps[n]
    st, rec, by, first, first_byte = taken
    for k in ac.STAT_FIELDS:
        if st[k] != stats[k]:
            bad.append(tag + "after %d frames %s = %d, the model's %d" % (n, k, st[k], stats[k]))
    if st["frames_lost"] != 0:
        bad.append(tag + "after %d frames frames_lost = %d" % (n, st["frames_lost"]))
    if first + (0 if rec is None else len(rec)) != n_rec:
        bad.append(tag + "after %d frames %d records, the model has %d" % (n, first + (0 if rec is None else len(rec)), n_rec))
    if rec is not None:
        want, pcm = _wanted(m)
        if rec.tobytes() != want[first:n_rec].tobytes():
            d = [k for k in range(min(len(rec), n_rec - first)) if rec[k].tobytes() != want[first + k].tobytes()][:3]
            bad.append(tag + "after %d frames the new records differ; first differences %s" % (n, [(k, rec[k].tolist(), want[first + k].tolist()) for k in d]))
        w = pcm[first_byte:n_rec * dx.MP2_PCM_BYTES]
        if not np.array_equal(by, w):
            k = min(len(by), len(w))
            d = np.flatnonzero(by[:k] != w[:k])
            bad.append(tag + "after %d frames the new PCM differs (%d bytes, the model has %d; %d differ, the first at %d = frame %d sample %d)"
                       % (n, len(by), len(w), len(d), d[0] if len(d) else k, (d[0] if len(d) else k) // 4608, ((d[0] if len(d) else k) % 4608) // 2))
    return bad


def _switch_on(eng, i, s, audio=True):
    for j, (kbps, kind) in enumerate(ac.kinds(s)):
        if kind == "pad":
            eng.set_pad_mode(i, j)
        elif kind == "pkt":
            eng.set_packet_mode(i, j, ac.PACKET_ADDRESS)
        if kind == "aud+pad":
            eng.set_pad_mode(i, j, source="mp2")
        if ac.is_audio(kind) and audio:
            eng.set_mp2_audio_mode(i, j)


def _state(eng, i, s):
    out = []
    for j, (kbps, kind) in enumerate(ac.kinds(s)):
        if ac.is_audio(kind):
            rec, by = eng.read_mp2_audio(i, j, 4)
            out.append((sorted((k, v) for k, v in eng.mp2_audio_stats(i, j).items() if k != "launches"), rec.tobytes(), by.tobytes()))      # (launches is the engine's)
    return out


def _drive(eng, streams, schedule, audio=True):
    cases = [ac.stream_case(s) for s in streams]
    followers = {}
    for i, s in enumerate(streams):
        for j, (kbps, kind) in enumerate(ac.kinds(s)):
            if ac.is_audio(kind) and audio:
                followers[(i, j)] = audio_follower()
            elif kind == "pad":
                followers[(i, j)] = Follower(PAD_ITEMS, 144)
            elif kind == "pkt":
                followers[(i, j)] = packet_follower(kbps)
    bad = []

    def after_batch(i, n, taken):
        for j, (kbps, kind) in enumerate(ac.kinds(streams[i])):
            if ac.is_audio(kind) and audio:
                bad.extend(batch_mismatches("stream %d slot %d (%d kbit/s): " % (i, j, kbps), ac.slot_model(streams[i], j), n, taken[j]))

    got = drive(eng, cases, schedule, lambda eng, i: _switch_on(eng, i, streams[i], audio), followers, lambda eng, i: _state(eng, i, streams[i]), after_batch)
    for (i, j), g in got.items():
        kbps, kind = ac.kinds(streams[i])[j]
        if not np.array_equal(g["frames"], cases[i][1][j]):
            bad.append("stream %d slot %d: the logical frames are not the intended ones" % (i, j))
        g["astats"] = eng.mp2_audio_stats(i, j)
        g["pstats"], g["kstats"] = eng.pad_stats(i, j), eng.packet_stats(i, j)
        if kind == "aud+pad":
            g["pad"] = eng.read_pad_items(i, j, 512)
        if ac.is_audio(kind) and audio:
            m = ac.slot_model(streams[i], j)
            want, pcm = _wanted(m)
            if g["rec"].tobytes() != want.tobytes() or not np.array_equal(g["bytes"], pcm) or g["astats"]["active"] != 1:
                bad.append("stream %d slot %d: the whole run's records or PCM differ from the model's" % (i, j))
        elif any(v for k, v in g["astats"].items() if k != "launches"):
            bad.append("stream %d slot %d (%s): the mode is off and the slot shows MP2 audio results: %s" % (i, j, kind, g["astats"]))
    return got, cases, bad


_runs = {}


def test_every_audio_slot_equals_the_model_after_every_batch_behind_the_lane_per_trellis_decoder():
    """Full batches of 28 CIFs, k_msc_prep + k_msc_vitT as the only decoder.  k_mp2_audio ran once per batch."""
    streams = list(range(len(ac.STAGE_STREAMS)))
    eng = engine(len(streams), 5)
    try:
        got, cases, bad = _drive(eng, streams, [[B] * len(streams)] * ac.N_BATCHES)
        launches = kernel_launches(eng)
        mine = eng.mp2_audio_stats(0, 0)["launches"]
    finally:
        eng.close()
    print(launches, mine)
    assert mine == ac.N_BATCHES + 1 == launches["k_dabplus"] == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, (mine, launches)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    total = {k: sum(g["astats"][k] for (i, j), g in got.items() if ac.is_audio(ac.kinds(streams[i])[j][1])) for k in ("frames_out", "bad_header", "refused", "overread")}
    assert all(v > 0 for v in total.values()), total
    # over-reading headers at 8 and 56 kbit/s count; the same headers at 96 kbit/s and above must not
    for (i, j), g in got.items():
        kbps, kind = ac.kinds(streams[i])[j]
        if ac.is_audio(kind):
            assert (g["astats"]["overread"] > 0) == (kbps < 96), (i, j, kbps, g["astats"])
            assert (int((g["rec"]["flags"] & dx.MP2_AUDIO_OVERREAD).sum()) == g["astats"]["overread"]), (i, j)
    _runs["full"] = got


def test_frames_across_batch_boundaries_and_idle_batches_behind_the_wave_per_trellis_decoder():
    """The boundary schedule (28, 0, 1, 4, 5, 6, 27, 13 CIFs per batch, every stream from its own place): sync words, headers and MP2 frames of
    two and three logical frames stay open across batch ends and across batches in which a stream receives nothing.  k_msc_frame is the
    only decoder here; the results are also byte for byte those of the full-batch run."""
    streams = list(range(len(ac.STAGE_STREAMS)))
    schedule = ac.boundary_schedule(len(streams))
    eng = engine(len(streams), 5, fast_min=1 << 30, class_min=0)
    try:
        got, cases, bad = _drive(eng, streams, schedule)
        launches = kernel_launches(eng)
        mine = eng.mp2_audio_stats(0, 0)["launches"]
    finally:
        eng.close()
    print(launches, mine)
    assert mine == len(schedule) + 1 == launches["k_msc_frame"] and launches["k_msc_vitT"] == 0, (mine, launches)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    if "full" in _runs:
        for key, g in got.items():
            assert g["rec"].tobytes() == _runs["full"][key]["rec"].tobytes() and np.array_equal(g["bytes"], _runs["full"][key]["bytes"]), key


def test_pad_items_and_stats_of_the_shared_slots_and_all_other_slots_equal_a_run_without_audio():
    """Streams 0 and 1 (both layouts) once more with the audio mode off everywhere: the PAD items, bytes, dabx_pad_stats and
    dabx_mp2_sync_stats of the slots that decode both, the items of the DAB+ PAD slots and the data groups of the packet-mode slot are
    exactly those of the run with audio on, and so are all logical frames."""
    streams = [0, 1]
    runs = []
    for audio in (True, False):
        eng = engine(len(streams), 5)
        try:
            got, cases, bad = _drive(eng, streams, [[B] * len(streams)] * ac.N_BATCHES, audio=audio)
            for (i, j), g in got.items():
                g["sync"] = eng.mp2_sync_stats(i, j)
            launches = eng.mp2_audio_stats(0, 0)["launches"]
        finally:
            eng.close()
        assert not bad, "\n".join(bad[:25])
        assert launches == (ac.N_BATCHES + 1 if audio else 0), launches
        runs.append(got)
    n_shared = n_pad = n_pkt = 0
    for (i, j), a in sorted(runs[0].items()):
        b = runs[1][(i, j)]
        kind = ac.kinds(streams[i])[j][1]
        assert np.array_equal(a["frames"], b["frames"]) and a["pstats"] == b["pstats"] and a["kstats"] == b["kstats"] and a["sync"] == b["sync"], (i, j)
        if kind == "aud+pad":
            assert a["pad"][0].tobytes() == b["pad"][0].tobytes() and np.array_equal(a["pad"][1], b["pad"][1]), (i, j)
            assert a["pstats"]["active"] == 1 and a["pstats"]["aus"] > 50 and a["sync"]["frames"] == a["astats"]["decode_calls"], (i, j, a["pstats"], a["sync"])
            n_shared += 1
        elif kind == "pad":
            assert a["rec"].tobytes() == b["rec"].tobytes() and np.array_equal(a["bytes"], b["bytes"]) and len(a["rec"]) > 0, (i, j)
            n_pad += 1
        elif kind == "pkt":
            assert a["rec"].tobytes() == b["rec"].tobytes() and np.array_equal(a["bytes"], b["bytes"]) and len(a["rec"]) > 0, (i, j)
            n_pkt += 1
    assert (n_shared, n_pad, n_pkt) == (2, 2, 1)


def test_on_off_and_on_again_restarts_empty_and_no_audio_slot_launches_nothing():
    """Stream 1's layout on three engines.  The first never has the mode on: zero launches, all-zero stats, nothing to read.  The second
    has it on slots 0 and 1 throughout: one launch per batch.  The third has it on slot 1 for batches 0-1, off (NULL) for batches 2-3 and on
    again from batch 4: the logical frames of every slot are the intended ones in all three, and what is read after the second start is the
    model's on the frames from then on (a slot that is switched on starts as a fresh Mp2Processor)."""
    s, j = 1, 1
    layout, frames, cifs = ac.stream_case(s)
    assert ac.kinds(s)[j] == (96, "aud")
    results = []
    for mode in ("never", "on", "toggled"):
        eng = engine(1, len(layout))
        try:
            eng.set_subchannels(layout, stream=0)
            dx.msc_inject(eng, 0, cifs[:H])
            dx.msc_decode(eng, [H], H)
            if mode == "on":
                eng.set_mp2_audio_mode(0, 0); eng.set_mp2_audio_mode(0, j)
            got = [[] for _ in layout]
            for b in range(ac.N_BATCHES):
                if mode == "toggled" and b in (0, 2, 4):
                    eng.set_mp2_audio_mode(0, j, on=b != 2)
                dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
                dx.msc_decode(eng, [B], B)
                eng.subch = list(layout)
                for k in range(len(layout)):
                    got[k].append(eng.read_msc(0, k, B))
                if mode == "toggled" and b == 3:
                    st = eng.mp2_audio_stats(0, j)
                    assert st["launches"] == 2 and not any(v for k, v in st.items() if k != "launches") and len(eng.read_mp2_audio(0, j, 8)[0]) == 0, st
            for k in range(len(layout)):
                assert np.array_equal(np.concatenate(got[k]), frames[k]), (mode, k)
            results.append((eng.mp2_audio_stats(0, j), eng.read_mp2_audio(0, j, 64), kernel_launches(eng)))
        finally:
            eng.close()
    st, (rec, by), launches = results[0]
    assert launches["k_dabplus"] == ac.N_BATCHES + 1 and not any(st.values()) and len(rec) == 0, (launches, st)
    st, (rec, by), launches = results[1]
    m = ac.slot_model(s, j)
    assert st["launches"] == ac.N_BATCHES and all(st[k] == m.all_stats()[k] for k in ac.STAT_FIELDS), (st, m.all_stats())
    st, (rec, by), launches = results[2]
    m = ac.run_model(96, frames[j][4 * B:], first=4 * B)
    assert st["launches"] == 2 + (ac.N_BATCHES - 4) and m.stats["frames_out"] > 20, (st, m.stats)
    assert all(st[k] == m.all_stats()[k] for k in ac.STAT_FIELDS) and st["frames_lost"] == 0, (st, m.all_stats())
    assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_pcm())


def test_an_audio_slot_that_moves_to_other_capacity_units_loses_nothing_and_a_changed_slot_starts_anew_with_the_mode_off():
    """dabx_set_subchannels with the 96 kbit/s audio slot at other capacity units in the middle of the run: the slot "keeps decoding without
    interruption", and so do the sync state, MP2frame and V -- every record and sample equals the model's on the whole scenario.  Then the
    slot's protection level changes: a changed slot starts anew, with the mode off."""
    kbps = 96
    frames = ac.scenario(kbps, 77, 21)[0]
    old = dc.dabplus_layout([(64, ac.PROT, 0), (kbps, ac.PROT, 0)], dab_plus=[0, 0])
    new = dc.dabplus_layout([(64, ac.PROT, 0), (kbps, ac.PROT, 0)], dab_plus=[0, 0])
    new[1].cu_start = 400
    filler = pkc.scenario(64, 5, ac.N_FRAMES)
    c_old = dc.cifs_of(old, [filler, frames], np.random.default_rng(3))
    c_new = dc.cifs_of(new, [filler, frames], np.random.default_rng(3))
    m = ac.run_model(kbps, frames)
    b_move = 3
    move = H + b_move * B
    cifs = np.concatenate([c_old[:move], c_new[move:]])
    eng = engine(1, 2)
    try:
        eng.set_subchannels(old, stream=0)
        eng.set_mp2_audio_mode(0, 1)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        ring, bad = audio_follower(), []
        for b in range(ac.N_BATCHES):
            if b == b_move:
                eng.set_subchannels(new, stream=0)
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
            bad += batch_mismatches("batch %d: " % b, m, B * (b + 1), ring.take(eng, 0, 1))
        eng.subch = list(new)
        last = eng.read_msc(0, 1, B)
        changed = dc.dabplus_layout([(64, ac.PROT, 0), (kbps, 2, 0)], dab_plus=[0, 0])
        eng.set_subchannels(changed, stream=0)
        after = eng.mp2_audio_stats(0, 1)
        n_after = len(eng.read_mp2_audio(0, 1, 8)[0])
    finally:
        eng.close()
    assert not bad, "\n".join(bad[:25])
    assert np.array_equal(last, frames[-B:]) and ring.seen == len(m.rows) > 100 and np.array_equal(ring.result()[1], m.all_pcm())
    assert not any(v for k, v in after.items() if k != "launches") and n_after == 0, after


def test_the_refusals():
    """The mode is refused for a DAB+ slot, a packet-mode slot, an inactive slot and no slot at all -- the rules of the PAD stage's MP2
    source --; NULL for a slot whose mode is off is refused in the same cases and accepted for a plain audio slot; a slot with the mode on
    cannot become a packet-mode slot; the mode is independent of the slot's PAD mode, in either order."""
    layout = ac.stage_layout(0)                                       # 8 aud, 384 aud, 64 DAB+, 16 pkt, 56 aud
    eng = engine(1, 6)
    try:
        eng.set_subchannels(layout, stream=0)
        eng.set_packet_mode(0, 3, ac.PACKET_ADDRESS)
        for j in (2, 3, 5, 6):                                        # a DAB+ slot, a packet-mode slot, a slot that is not configured, no such slot
            with pytest.raises(dx.DabxError):
                eng.set_mp2_audio_mode(0, j)
            with pytest.raises(dx.DabxError):
                eng.set_mp2_audio_mode(0, j, on=False)
        with pytest.raises(dx.DabxError):
            eng.mp2_audio_stats(0, 6)
        eng.set_mp2_audio_mode(0, 0, on=False)                        # nothing to switch off: accepted for a slot that could have it
        assert not any(eng.mp2_audio_stats(0, 0).values())
        eng.set_mp2_audio_mode(0, 0)
        assert eng.mp2_audio_stats(0, 0) == dict(decode_calls=0, frames_out=0, bad_header=0, refused=0, overread=0, launches=0, sample_rate=48000,
                                                 frames_lost=0, number_of_frames=0, error_frames=0, voffs=0, active=1, pcm_bytes=0)
        with pytest.raises(dx.DabxError):
            eng.set_packet_mode(0, 0, 5)                              # the mode is on
        eng.set_pad_mode(0, 0, source="mp2")                          # PAD decoding beside it ...
        assert eng.pad_stats(0, 0)["active"] == 1 and eng.mp2_audio_stats(0, 0)["active"] == 1
        eng.set_pad_mode(0, 0, on=False)                              # ... and gone again: the audio mode stays
        assert eng.pad_stats(0, 0)["active"] == 0 and eng.mp2_audio_stats(0, 0)["active"] == 1
        eng.set_pad_mode(0, 4, source="mp2")                          # ... and in the other order
        eng.set_mp2_audio_mode(0, 4)
        eng.set_mp2_audio_mode(0, 4, on=False)
        assert eng.pad_stats(0, 4)["active"] == 1 and eng.mp2_audio_stats(0, 4)["active"] == 0
        eng.set_mp2_audio_mode(0, 0, on=False)
        assert not any(eng.mp2_audio_stats(0, 0).values())
        eng.set_packet_mode(0, 0, 5)                                  # ... and now it may
        with pytest.raises(dx.DabxError):
            eng.set_mp2_audio_mode(0, 0)
        L = dx.load()
        short = dx.Mp2AudioConfig(size=2)                             # a configuration that cannot hold its size
        import ctypes as C
        with pytest.raises(dx.DabxError):
            dx.check(L.dabx_set_mp2_audio_mode(eng._h, 0, 1, C.byref(short)))
    finally:
        eng.close()
