"""The DAB+ super-frame stage -- k_dabplus as dabx_process launches it behind the batched MSC decoder -- on adversarial super frames,
against the oracle back end (oracle/msc.c), at every bit rate 8 .. 384 kbit/s (R = 1 .. 48 RS code words per super frame).

Noise-free coded soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode: no IQ, no front
end) and decode to exactly the intended logical frames, so what the stage sees is chosen byte by byte: all four header layouts (2, 3,
4, 6 AUs), AU tables with edge lengths, unsorted starts and starts beyond the end, wrong AU CRCs, fire-code bursts and garbage headers,
1 .. 5 and 6, 8, 20 byte errors per RS code word (all of them, only the first, only the last, a subset, parity bytes only), lost
logical frames, junk in front, slips that cost the sync, and a decoy header the slide locks on.  Generators and scenarios:
tests/dabplus_cases.py; that they reach the branches they are meant to reach is asserted on the oracle alone in
tests/test_dabplus_cases.py, on the very same sets.

Every comparison is exact and covers every (stream, slot): logical frames and super frames with np.array_equal, the 32-byte records
with .tobytes(), the counters cifs_decoded, sf_ok, sf_fail, rs_corrected, rs_failed, fc_corrected, au_ok, au_bad and sf_count with ==.
The device keeps the newest 16 super frames per slot and a batch completes at most 6, so the new rows are read after every batch.

The end-of-frame guard `au_start + len + 2 > end` (an AU whose length passes the 0 .. 960 check but which would end behind the super
frame) is the oracle's and the kernel's; mp4processor.cpp:311 has no such test and would read past the super frame there.  The guard is
kept and compared; the reference's out-of-bounds read is not reproduced."""
import numpy as np
import pytest

import dabplus_cases as dc
from dabstar_amd import lib as dx
from stage_driver import SF_COUNTERS, drive, engine, kernel_launches

pytestmark = pytest.mark.gpu

B = dc.BATCH


def _state(eng, lay, s):
    """All a stream's slots hold, as bytes: the newest logical frames, super frames and records, and the counters."""
    eng.subch = list(lay)
    out = []
    for j, sc in enumerate(lay):
        if sc.kbps:
            out.append((eng.read_msc(s, j, B).tobytes(), eng.read_superframes(s, j, 16).tobytes(), eng.read_superframe_info(s, j, 16).tobytes(),
                        sorted(eng.subch_stats(s, j).items())))
    return out


def _drive(eng, lays, cifs, schedule):
    """stage_driver.drive on per stream (layout, CIFs): after every batch the new logical frames, super frames and records of every slot
    are read and appended; a stream that received nothing must hold byte for byte what it held.  Returns ({(s, j): {"frames", "sf", "sfi",
    "stats"}}, per stream the batches that completed no super frame)."""
    got = drive(eng, [(lays[s], None, cifs[s]) for s in range(len(lays))], schedule, lambda eng, s: None, {}, lambda eng, s: _state(eng, lays[s], s))
    idle = []
    for s in range(len(lays)):
        per_slot = [g["sf_new"] for (i, j), g in got.items() if i == s and lays[s][j].dab_plus]
        idle.append(sum(not any(batch) for batch in zip(*per_slot)))
    return got, idle


def _mismatches(got, lays, want):
    """Every difference between the device and the oracle (want[s][j]) as a line that names the bit rate, the stream, the slot and the
    super frame (its number and its first logical frame)."""
    bad = []
    for (s, j), g in sorted(got.items()):
        sc, o = lays[s][j], want[s][j]
        tag = "%d kbit/s (R = %d), stream %d, slot %d: " % (sc.kbps, sc.kbps // 8, s, j)
        if g["frames"].shape != o["frames"].shape:
            bad.append(tag + "%d logical frames, the oracle has %d" % (g["frames"].shape[0], o["frames"].shape[0]))
        else:
            for k in np.flatnonzero((g["frames"] != o["frames"]).any(axis=1))[:3]:
                bad.append(tag + "logical frame %d differs" % k)
        if len(g["sfi"]) != len(o["sfi"]) or g["stats"]["sf_count"] != len(o["sfi"]):
            bad.append(tag + "%d super frames (sf_count %d), the oracle has %d; first logical frames %s against %s"
                       % (len(g["sfi"]), g["stats"]["sf_count"], len(o["sfi"]), g["sfi"]["first_frame"].tolist(), o["sfi"]["first_frame"].tolist()))
        for i in range(min(len(g["sfi"]), len(o["sfi"]))):
            where = tag + "super frame %d (first logical frame %d): " % (i, int(o["sfi"][i]["first_frame"]))
            if g["sfi"][i].tobytes() != o["sfi"][i].tobytes():
                bad.append(where + "record %s, the oracle's %s %s" % (g["sfi"][i].tolist(), o["sfi"][i].tolist(), dx.SUPERFRAME_INFO.names))
            if not np.array_equal(g["sf"][i], o["sf"][i]):
                d = np.flatnonzero(g["sf"][i] != o["sf"][i])
                bad.append(where + "%d bytes differ, the first at %s (code words %s)" % (len(d), d[:8].tolist(), sorted(set((d % (sc.kbps // 8)).tolist()))[:8]))
        for mine, theirs in SF_COUNTERS:
            if g["stats"][mine] != o["stats"][theirs]:
                bad.append(tag + "%s = %d, the oracle's %d" % (mine, g["stats"][mine], o["stats"][theirs]))
    return bad


def _totals(got, lays):
    t = dict.fromkeys([m for m, _ in SF_COUNTERS] + ["sf_count"], 0)
    for (s, j), g in got.items():
        if lays[s][j].dab_plus:
            for k in t:
                t[k] += g["stats"][k]
    return t


def _assert_not_vacuous(t):
    """Where test_dabplus_cases.py demands an event of the oracle, the device counted it too (both sides already agree on the numbers)."""
    assert all(t[k] > 0 for k in ("sf_ok", "sf_fail", "rs_corrected", "rs_failed", "fc_corrected", "au_ok", "au_bad", "sf_count")), t


def _full_batches(S):
    return [[B] * S for _ in range(dc.N_BATCHES)]


def _case(set_no, lays):
    """Per stream the CIFs and the oracle's results of dabplus_cases.stream_case."""
    cases = [dc.stream_case(set_no, lays[s], s) for s in range(len(lays))]
    return [c[2] for c in cases], [c[3] for c in cases]


def test_every_bit_rate_on_adversarial_super_frames_equals_the_oracle():
    """All 48 rates at EEP 4-A, packed into layouts of at most 16 lane-per-trellis classes, two streams per layout with scenarios of
    their own: 16 CIFs of history, then seven batches of 28.  Every slot accepts more than 16 super frames, so its ring of 16 wraps.
    k_dabplus ran once per batch, k_msc_frame never."""
    S = dc.EVERY_RATE_STREAMS
    bad, seen, total = [], [], None
    for layout in dc.every_rate_layouts():
        lays = [layout] * S
        cifs, want = _case(0, lays)
        eng = engine(S, len(layout))
        try:
            got, _idle = _drive(eng, lays, cifs, _full_batches(S))
            launches = kernel_launches(eng)
            assert launches["k_dabplus"] == dc.N_BATCHES + 1 == launches["k_msc_vitT"] and launches["k_msc_frame"] == 0, launches
        finally:
            eng.close()
        bad += _mismatches(got, lays, want)
        seen += [c.kbps for c in layout]
        assert all(g["stats"]["sf_count"] >= 16 for g in got.values()), sorted((lays[s][j].kbps, s, g["stats"]["sf_count"]) for (s, j), g in got.items())
        t = _totals(got, lays)
        total = t if total is None else {k: total[k] + t[k] for k in t}
    assert sorted(seen) == dc.RATES
    print("device counters summed over 48 rates x %d streams:" % S, total)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    _assert_not_vacuous(total)


def test_super_frames_across_batch_boundaries_and_streams_that_receive_nothing():
    """R = 1, 3, 8, 9, 17, 48 on five streams whose CIF counts differ inside every batch (28, 0, 1, 4, 5, 6, 27, 13 in turn, each stream
    from its own place): the five-frame windows straddle the batch ends at every place (asserted in test_dabplus_cases.py), blocks_in_buf
    and sf_sync are carried from launch to launch, some batches complete no super frame for a stream, and a stream that received
    nothing keeps its logical frames, super frames, records and counters byte for byte (_drive)."""
    layout = dc.boundary_layout()
    S = dc.BOUNDARY_STREAMS
    lays = [layout] * S
    cifs, want = _case(1, lays)
    schedule = dc.boundary_schedule()
    eng = engine(S, len(layout))
    try:
        got, idle = _drive(eng, lays, cifs, schedule)
        launches = kernel_launches(eng)
        assert launches["k_dabplus"] == len(schedule) + 1, launches
    finally:
        eng.close()
    assert all(n > 0 for n in idle), idle                      # batches in which a stream got CIFs and completed no super frame
    bad = _mismatches(got, lays, want)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    _assert_not_vacuous(_totals(got, lays))


def test_both_decoders_feed_the_stage_the_same():
    """The same inputs with k_msc_frame as the only decoder (msc_fast_min_jobs = 1 << 30), with the default thresholds (which, for two
    streams, choose k_msc_frame as well: the launches are printed) and with k_msc_prep + k_msc_vitT as the only one (both thresholds 1):
    super frames and records are identical, and each run equals the oracle."""
    layout = dc.boundary_layout()
    S = 2
    lays = [layout] * S
    cifs, want = _case(1, lays)
    runs = []
    for fast_min, class_min in ((1 << 30, 0), (0, 0), (1, 1)):
        eng = engine(S, len(layout), fast_min=fast_min, class_min=class_min)
        try:
            got, _idle = _drive(eng, lays, cifs, _full_batches(S))
            launches = kernel_launches(eng)
            assert launches["k_dabplus"] == dc.N_BATCHES + 1, launches
            if fast_min == 1 << 30:
                assert launches["k_msc_vitT"] == 0 and launches["k_msc_frame"] == dc.N_BATCHES + 1, launches
            if fast_min == 1:
                assert launches["k_msc_vitT"] == dc.N_BATCHES + 1 and launches["k_msc_frame"] == 0, launches
            print("msc_fast_min_jobs", fast_min, launches)
        finally:
            eng.close()
        bad = _mismatches(got, lays, want)
        assert not bad, "msc_fast_min_jobs = %d: %d differences:\n%s" % (fast_min, len(bad), "\n".join(bad[:25]))
        _assert_not_vacuous(_totals(got, lays))
        runs.append(got)
    for other in runs[1:]:
        for key in runs[0]:
            assert np.array_equal(runs[0][key]["sf"], other[key]["sf"]) and runs[0][key]["sfi"].tobytes() == other[key]["sfi"].tobytes(), key


def test_a_slot_that_is_not_dab_plus_and_one_that_is_not_configured_next_to_dab_plus_slots():
    """Stream 0: slot 1 is not configured, slot 2 is configured with dab_plus = 0 and carries a complete DAB+ scenario all the same.  The
    DAB+ slots on both sides equal the oracle; the slot that is not DAB+ delivers its logical frames, no super frame and no record, and
    all its sf_* counters stay 0; the slot that is not configured stays untouched.  Stream 1 has all four slots DAB+."""
    lays = dc.neighbour_layouts()
    assert lays[0][1].kbps == 0 and lays[0][2].kbps and not lays[0][2].dab_plus and all(c.dab_plus for c in lays[1])
    cifs, want = _case(2, lays)
    eng = engine(2, 4)
    try:
        got, _idle = _drive(eng, lays, cifs, _full_batches(2))
        idle_slot = eng.subch_stats(0, 1)
        eng.subch = list(lays[1])
        nothing = (eng.read_superframes(0, 2, 16).shape[0], eng.read_superframe_info(0, 2, 16).shape[0])
    finally:
        eng.close()
    bad = _mismatches(got, lays, want)
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:25]))
    st = got[(0, 2)]["stats"]
    assert st["cifs_decoded"] == dc.N_FRAMES and got[(0, 2)]["frames"].shape[0] == dc.N_FRAMES
    assert all(st[k] == 0 for k in ("sf_count", "sf_ok", "sf_fail", "rs_corrected", "rs_failed", "fc_corrected", "au_ok", "au_bad")), st
    assert nothing == (0, 0) and len(got[(0, 2)]["sfi"]) == 0
    assert idle_slot["active"] == 0 and all(idle_slot[k] == 0 for k in ("cifs_decoded", "sf_count", "sf_ok", "sf_fail", "au_ok", "au_bad")), idle_slot
    assert (0, 1) not in got and want[0][1] is None
    _assert_not_vacuous(_totals(got, lays))
