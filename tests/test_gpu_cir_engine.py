"""The CIR and correlation plot stage inside the running engine (dabx_set_cir_mode, dabx_read_cir; pipeline.hip k_cir, k_cir_finish,
k_cir_corr), through IQ, for cf32 / s16 / u8 rings.  Three streams of one FIC-only engine, every sample committed before the first step:

  stream 0  the mode on from the start (both kinds).  Its signal begins with 1.2 frames of noise that keep it searching, so the first CIR
            rows are computed while it is out of lock; the phase reference symbol of its ninth frame is replaced by noise, so one
            correlation in lock fails behind the first show ("accumulated but not counted") and the stream searches again.
  stream 1  switched on after two steps, at a read position that is no multiple of 512.
  stream 2  stream 1's signal, the mode off throughout: nothing for it.

Every signal has a second path 300 samples late and 6 dB down, so a show lists two indices.  After EVERY dabx_process call the new
records are held against the models of tests/cir_cases.py: the CIR from dabx_read_iq of the window's positions, the correlation plot
from the oracle receiver's trace of the same (quantised) samples -- window position, NCO phase and frequency, threshold, which calls
failed.  Indices, counters and positions exactly, floats to 2e-5 of the largest model value (the averaged plot: times the terms
accumulated since the stream was enabled).  Steps of one frame and calls of seven frames give byte-identical records.

Admissibility: every comparison a walk evaluates is at least 2e-5 max(pk) wide in the model; the noise seed moves on until that holds
(MOVED counts how many seeds had to; docs/history/cir.md has the figure)."""
import os
import sys

import numpy as np
import pytest

import cir_cases as cc
import oracle_lib as ol
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from tools import iq_files as iqf  # noqa: E402

pytestmark = pytest.mark.gpu
TF, TU = ds.TF, 2048
KINDS = ["cf32", "s16", "u8"]
S, OFF = 3, 2
N_FRAMES = 16                                   # ensemble frames behind stream 0's prefix
PREFIX = int(1.2 * TF)
FAIL_FRAME = 8                                  # its phase reference symbol is noise
ENABLE_AFTER = 2                                # steps before stream 1 is switched on
STEPS = 22                                      # (calls of seven frames restart the search after the failed frame a few steps late: room for them)
ECHO = (300, 0.5)
MOVED = {}


def echo(x):
    y = x.astype(np.complex64).copy()
    y[ECHO[0]:] += np.complex64(ECHO[1]) * x[:-ECHO[0]]
    return y


def float_signals(seed):
    subch = ds.default_subchannels(1, 64)
    rng = np.random.default_rng(1000 + seed)
    ens = ds.build_ensemble(20, subch, seed=70)            # (a whole number of super frames)
    a = echo(ds.channel(ens.iq, snr_db=25.0, cfo_hz=310.0, timing_offset=3001, seed=seed, n_out=N_FRAMES * TF))
    # where the frames of `a` lie: the oracle's own symbol-0 positions
    sym0 = ol.oracle_run(a, [], front=1)["sym0"]
    assert len(sym0) >= N_FRAMES - 2
    lvl = float(np.sqrt(np.mean(np.abs(a) ** 2)))
    noise = lambda n: (lvl * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)   # noqa: E731
    p = int(sym0[FAIL_FRAME])
    a[p - 504:p + TU] = noise(504 + TU)
    x0 = np.concatenate([noise(PREFIX), a])
    x1 = echo(ds.channel(ens.iq, snr_db=22.0, cfo_hz=-120.0, timing_offset=4243, seed=seed + 1, n_out=N_FRAMES * TF + 999))
    return [x0, x1, x1.copy()]


def to_ring(x, kind):
    """-> (what is pushed, the float samples those stand for)"""
    if kind == "cf32":
        return x, x
    g = 0.25 / np.sqrt(np.mean(np.abs(x) ** 2))
    codes = iqf.to_u8(x, g) if kind == "u8" else iqf.to_int(x, 16, g).astype(np.int16)
    c = codes.astype(np.float32)
    v = (c - np.float32(127.38)) / np.float32(128) if kind == "u8" else c / np.float32(32768)
    return np.ascontiguousarray(codes), np.ascontiguousarray(v).view(np.complex64)


def rnd(v):
    return int(np.floor(abs(float(v)) + 0.5)) * (1 if v >= 0 else -1)        # roundf


def head_calls(vals):
    """The calls of correlate_with_phase_ref_and_find_max_peak the frame chain makes, from the oracle receiver's run on the same samples:
    [(window position, NCO phase in front of it, rounded frequency, threshold factor, frame index or -1 if the call failed, frames decoded
    in front of the call)].  A failed
    correlation of a search candidate (directly behind the end of a dip) would be the search's own, which k_cir_corr, in front of the frame
    head, does not see (include/dabx.h, the stated deviation): the signals here must have none, and that is asserted."""
    res = ol.oracle_run(vals, [], trace=1 << 16, front=1)
    calls, k, prev = [], 0, None
    f_bb = 0.0
    for ev in res["trace"]:
        kind = int(ev["kind"])
        if kind == ol.EV_CORR_OK:
            if k >= res["n"]:                                               # the samples ran out inside this frame
                break
            f = rnd(f_bb)
            start = int(res["start"][k])
            pos = int(ev["pos"]) - TU
            assert pos + start == int(res["sym0"][k])
            calls.append((pos, int((int(res["phase_sym1"][k]) + (start + TU) * f) % cc.INPUT_RATE), f, 3.0 if prev == ol.EV_DIP_END else 6.0, k, k))
        elif kind == ol.EV_CORR_FAILED and prev == ol.EV_FRAME_DONE:
            calls.append((int(ev["pos"]) - TU, int(res["phase_end"][k - 1]), rnd(f_bb), 6.0, -1, k))
        elif kind == ol.EV_CORR_FAILED:
            # a search candidate that fails: the search's own call, which the plot would not see (the stated deviation) -- these signals have none
            raise AssertionError("a search candidate failed its correlation at %d" % int(ev["pos"]))
        elif kind == ol.EV_FRAME_DONE:
            f_bb = float(res["fbb_end"][k])
            k += 1
        prev = kind
    return calls, res


def corr_model(vals, calls, from_frame, starts=None):
    """The plot's state machine over the head calls from the first call of frame `from_frame` on (the stream is enabled in front of it):
    -> ([(frames decoded when the show is made, window position, mean, threshold, indices, terms)], CorrPlot)"""
    plot, shows = cc.CorrPlot(), []
    for pos, phase0, f, thr, k, frames in calls:
        if frames < from_frame:
            continue
        mixed, _ = cc.nco_mix(vals[pos:pos + TU], phase0, f)
        start, show = plot.call(cc.corr_pk(mixed), thr)
        assert (start >= 0) == (k >= 0), (pos, start, k)                    # the model fails where the oracle failed ...
        assert k < 0 or starts is None or start == int(starts[k]), (k, start)   # ... and finds the oracle's start index where it did not
        if show is not None:
            shows.append((frames, pos, show[0], show[1], show[2], plot.terms))
    return shows, plot


def signals(kind):
    """The pushed arrays, their float values and the head calls of streams 0 and 1: the noise seed moves on until every walk is admissible."""
    for seed in range(5, 5 + 8):
        pushed, vals = zip(*[to_ring(x, kind) for x in float_signals(seed)])
        calls = [head_calls(vals[0]), head_calls(vals[1])]
        plots = [corr_model(vals[0], calls[0][0], 0, calls[0][1]["start"])[1], corr_model(vals[1], calls[1][0], ENABLE_AFTER, calls[1][1]["start"])[1]]
        if min(p.margin for p in plots) >= cc.BAR:
            MOVED[kind] = seed - 5
            return pushed, vals, calls
    raise AssertionError("no admissible seed")


def cir_model(iq):
    """y[385] of one window from its 198 656 samples (cir_cases.row_model, all rows at once)"""
    x = np.asarray(iq, np.complex64).astype(np.complex128)
    rows = np.lib.stride_tricks.as_strided(x, (cc.ROWS, TU), (cc.ROW_STEP * x.itemsize, x.itemsize))
    z = np.fft.ifft(np.fft.fft(rows, axis=1) * np.conj(cc.PRS)[None, :], axis=1) * TU
    return np.sqrt((z.real ** 2 + z.imag ** 2).max(axis=1)) / cc.SCALE


def run(kind, pushed, batch):
    """One engine; batch = frames per dabx_process call behind the first ENABLE_AFTER single steps.
    -> per call [(steps so far, frames decoded per stream, new records per stream)], base of stream 1, the FIBs, the windows' samples"""
    eng = dx.Engine(n_streams=S, ring_frames=18, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, ring_format=kind)
    try:
        for s in range(S):
            eng.push_iq(s, pushed[s])
        assert eng.cir_stats(0) == dict(shows=[0, 0], lost=0, rows_untrusted=0, launches=0) and eng.read_cir(0) == ([], 0)   # nothing exists yet
        eng.set_cir_mode(0, cir=True, correlation=True)
        log, steps, base1, fibs = [], 0, None, [[] for _ in range(S)]
        seen = [0] * S
        while steps < STEPS:
            if steps == ENABLE_AFTER:
                base1 = int(dx.front_read(eng, 1, spectra=False)["rd"])
                eng.set_cir_mode(1, cir=True, correlation=True)
            m = 1 if steps < ENABLE_AFTER else min(batch, STEPS - steps)
            assert eng.process(m) == m
            steps += m
            frames, new = [], []
            for s in range(S):
                frames.append(eng.stats(s)["frames"])
                if frames[s] > seen[s]:
                    f, _ = eng.read_fibs(s, frames[s] - seen[s])
                    fibs[s].append(f.copy())
                    seen[s] = frames[s]
                recs, lost = eng.read_cir(s, 4)
                assert lost == 0
                new.append([(r.copy(), v.copy(), i.copy()) for r, v, i in recs])
            log.append((steps, frames, new))
        stats = [eng.cir_stats(s) for s in range(S)]
        windows = {}
        for s in (0, 1):
            for _, _, new in log:
                for r, _, _ in new[s]:
                    if int(r["kind"]) == dx.CIR_KIND_CIR:
                        windows[s, int(r["first_sample"])] = eng.read_iq(s, int(r["first_sample"]), cc.WINDOW)
        return log, base1, [np.concatenate(f) if f else np.zeros((0, 12, 32), np.uint8) for f in fibs], windows, stats
    finally:
        eng.close()


@pytest.fixture(scope="module", params=KINDS)
def world(request):
    """Per ring format: the signals, the models and the two runs.  Computed once, shared, left unchanged."""
    kind = request.param
    pushed, vals, calls = signals(kind)
    a = run(kind, pushed, 1)
    b = run(kind, pushed, 7)
    return dict(kind=kind, pushed=pushed, vals=vals, calls=calls, a=a, b=b)


def check_cir(r, v, idx, want_first, iq):
    assert (int(r["kind"]), int(r["n_values"]), int(r["n_indices"]), int(r["rows_untrusted"]), float(r["threshold"])) == (0, cc.ROWS, 0, 0, 0.0)
    assert int(r["first_sample"]) == want_first and len(v) == cc.ROWS and len(idx) == 0
    y = cir_model(iq)
    err = float(np.abs(v.astype(np.float64) - y).max() / y.max())
    assert err <= cc.BAR, err
    return err


def check_corr(r, v, idx, show):
    frames, pos, mean, thr, indices, terms = show
    assert (int(r["kind"]), int(r["n_values"]), int(r["rows_untrusted"])) == (1, TU, 0)
    assert int(r["first_sample"]) == pos and int(r["frame"]) == frames
    assert idx.tolist() == indices and int(r["n_indices"]) == len(indices)
    err = float(np.abs(v.astype(np.float64) - mean).max() / mean.max())
    terr = abs(float(r["threshold"]) - thr) / thr
    assert err <= cc.BAR * terms and terr <= cc.BAR, (err, terr, terms)
    return err, terr


def test_every_call_against_the_models(world):
    log, base1, fibs, windows, stats = world["a"]
    vals, calls = world["vals"], world["calls"]
    assert base1 % 512 != 0 and base1 > TF
    shows = [corr_model(vals[0], calls[0][0], 0), ([], None)]
    walks = [cc.Walk(0), None]
    got = [dict(cir=0, corr=0), dict(cir=0, corr=0)]
    worst = dict(cir=0.0, corr=0.0, thr=0.0)
    print()
    for steps, frames, new in log:
        assert new[OFF] == []                                                # the mode is off on this stream throughout
        for s in (0, 1):
            if s == 1 and steps <= ENABLE_AFTER:
                assert new[1] == []
                continue
            if s == 1 and walks[1] is None:
                walks[1] = cc.Walk(base1)
                assert frames[1] >= 1                                        # stream 1 was in lock when it was switched on
                shows[1] = corr_model(vals[1], calls[1][0], world["a"][0][ENABLE_AFTER - 1][1][1])
            # the CIR record this call completes (this log is the run of one frame per call: one step, one window at the most)
            w0 = walks[s].w0()
            want_cir = [w0] if walks[s].step(len(vals[s]))[2] else []
            got_cir = [x for x in new[s] if int(x[0]["kind"]) == 0]
            got_corr = [x for x in new[s] if int(x[0]["kind"]) == 1]
            assert [int(r["first_sample"]) for r, _, _ in got_cir] == want_cir, (s, steps)
            for (r, v, i), w0 in zip(got_cir, want_cir):
                worst["cir"] = max(worst["cir"], check_cir(r, v, i, w0, windows[s, w0]))
            got[s]["cir"] += len(got_cir)
            # the shows made by the head calls up to the frames decoded so far
            due = [sh for sh in shows[s][0] if sh[0] < frames[s]]
            assert got[s]["corr"] + len(got_corr) == len(due), (s, steps, frames[s])
            for (r, v, i), sh in zip(got_corr, due[got[s]["corr"]:]):
                e, t = check_corr(r, v, i, sh)
                worst["corr"], worst["thr"] = max(worst["corr"], e / sh[5]), max(worst["thr"], t)
                print("%s stream %d show at frame %2d: %d indices %s, %d terms, err %.2e of the bar x terms, threshold err %.2e"
                      % (world["kind"], s, sh[0], len(sh[4]), sh[4], sh[5], e / (cc.BAR * sh[5]), t))
            got[s]["corr"] += len(got_corr)
    print("%s worst: CIR %.2e, plot / terms %.2e, threshold %.2e (bar %.0e); seeds moved %d" % (world["kind"], worst["cir"], worst["corr"], worst["thr"], cc.BAR, MOVED[world["kind"]]))
    # what the inputs are there for
    assert got[0]["cir"] >= 2 and got[1]["cir"] >= 2 and got[0]["corr"] >= 2 and got[1]["corr"] >= 1
    assert all(len(sh[4]) >= 2 for sh in shows[0][0] + shows[1][0])
    assert {"accumulated_but_not_counted", "counted", "show_2_indices"} <= shows[0][1].branches
    assert any(c[4] < 0 for c in calls[0][0]) and not any(c[4] < 0 for c in calls[1][0]) and all(c[4] >= 0 for c in calls[0][0][:6])
    # rows were computed while stream 0 was still searching
    assert log[0][1][0] == 0 and world["a"][4][0]["shows"][0] >= 1 and [x for x in log[0][2][0] if int(x[0]["kind"]) == 0]
    # the uncleared mean matters: the second show differs from a plot that clears it by far more than the bar
    second = shows[0][0][1]
    assert second[5] > 6
    cleared = cc.CorrPlot()
    for pos, phase0, f, thr, k, _ in calls[0][0][6:]:
        st, sh = cleared.call(cc.corr_pk(cc.nco_mix(vals[0][pos:pos + TU], phase0, f)[0]), thr)
        if sh is not None:
            break
    assert np.abs(sh[0] - second[2]).max() > 100 * cc.BAR * second[5] * second[2].max()
    for s in (0, 1):
        assert stats[s]["shows"] == [got[s]["cir"], got[s]["corr"]] and stats[s]["lost"] == 0 and stats[s]["rows_untrusted"] == 0
        assert stats[s]["launches"] > 0
    assert stats[OFF]["shows"] == [0, 0]


def test_steps_of_one_frame_and_calls_of_seven_give_identical_records(world):
    (la, base_a, fibs_a, _, stats_a), (lb, base_b, fibs_b, _, stats_b) = world["a"], world["b"]
    assert base_a == base_b

    def flat(log, s):
        return [(r.tobytes(), v.tobytes(), i.tobytes()) for _, _, new in log for r, v, i in new[s]]
    for s in range(S):
        assert flat(la, s) == flat(lb, s) and (s != OFF or flat(la, s) == [])
    assert [{k: v for k, v in st.items() if k != "launches"} for st in stats_a] == [{k: v for k, v in st.items() if k != "launches"} for st in stats_b]


def test_mode_off_everywhere_is_an_engine_without_the_stage(world):
    kind, pushed = world["kind"], world["pushed"]

    def go(touch):
        eng = dx.Engine(n_streams=S, ring_frames=18, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, ring_format=kind)
        try:
            for s in range(S):
                eng.push_iq(s, pushed[s])
            if touch:
                eng.set_cir_mode(-1, cir=True, correlation=True)
                eng.set_cir_mode(-1, enable=False)
            fibs, seen = [[] for _ in range(S)], [0] * S
            for _ in range(6):
                eng.process(1)
                for s in range(S):
                    n = eng.stats(s)["frames"]
                    if n > seen[s]:
                        fibs[s].append(eng.read_fibs(s, n - seen[s])[0].copy())
                        seen[s] = n
            return [np.concatenate(f) if f else np.zeros((0, 12, 32), np.uint8) for f in fibs], eng.counters(), [eng.cir_stats(s) for s in range(S)], [eng.read_cir(s) for s in range(S)], [eng.scope_stats(s) for s in range(S)]
        finally:
            eng.close()
    plain, touched = go(False), go(True)
    for x, y in zip(plain[0], touched[0]):
        assert np.array_equal(x, y)
    assert sum(len(x) for x in plain[0]) >= 10
    assert plain[1] == touched[1] and plain[4] == touched[4]
    assert all(st == dict(shows=[0, 0], lost=0, rows_untrusted=0, launches=0) for st in plain[2] + touched[2])
    assert all(r == ([], 0) for r in plain[3] + touched[3])
    # and with the mode on, the receiver decodes what it decodes without it
    fibs_on = world["a"][2]
    for s in range(S):
        assert np.array_equal(plain[0][s], fibs_on[s][:len(plain[0][s])])


def test_five_unread_correlation_shows_give_four_records_and_one_lost():
    """The overrun of a record ring other than the scope's (csrc/rec_ring.h): CIR_RING = 4 slots, so RING + 1 correlation shows left unread
    lose the oldest.  One stream, the correlation plot alone, cf32, a clean signal: the plot shows once per PER_SHOW counted calls
    (mDisplayCounter > FRAMES_PER_SECOND / 2, phasereference.cpp:181; CirState::corr_counter), one call per frame in lock, so RING + 1 shows
    take (RING + 1) * PER_SHOW frames in lock -- plus two for the search and a cut first frame and two to spare, fewer than a further show
    would take.  Read once at the end, the records are byte for byte the newest RING of the same run read after every step."""
    RING = 4                                                              # cir_core.h, CIR_RING
    PER_SHOW = cc.CorrPlot.FRAMES_PER_SECOND // 2 + 1
    n_shows = RING + 1
    n_frames = n_shows * PER_SHOW + 4
    assert 4 < PER_SHOW
    ens = ds.build_ensemble(20, ds.default_subchannels(1, 64), seed=70)
    x = echo(ds.channel(ens.iq, snr_db=25.0, cfo_hz=-120.0, timing_offset=4243, seed=6, n_out=n_frames * TF))

    def go(read_every_step):
        eng = dx.Engine(n_streams=1, ring_frames=n_frames + 2, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, ring_format="cf32")
        try:
            eng.push_iq(0, x)
            eng.set_cir_mode(0, cir=False, correlation=True)
            got = []
            for _ in range(n_frames + 1):
                assert eng.process(1) == 1
                if read_every_step:
                    recs, lost = eng.read_cir(0, 4)
                    assert lost == 0
                    got += [(r.tobytes(), v.tobytes(), i.tobytes()) for r, v, i in recs]
            if read_every_step:
                return got, eng.cir_stats(0)
            recs, lost = eng.read_cir(0, 8)
            return [(r.tobytes(), v.tobytes(), i.tobytes()) for r, v, i in recs], lost, eng.cir_stats(0), eng.read_cir(0, 8)
        finally:
            eng.close()
    every, stats_every = go(True)
    assert len(every) == n_shows and stats_every["shows"] == [0, n_shows] and stats_every["lost"] == 0
    assert all(np.frombuffer(r, dx.CIR_RECORD)[0]["kind"] == dx.CIR_KIND_CORRELATION for r, _, _ in every)
    once, lost, stats_once, again = go(False)
    assert lost == 1 and once == every[-RING:]
    assert stats_once["shows"] == [0, n_shows] and stats_once["lost"] == 1
    assert again == ([], 0)


def test_arguments():
    eng = dx.Engine(n_streams=2, ring_frames=4, max_subch=1, fic_only=True)
    try:
        L = dx.load()
        L.dabx_set_cir_mode.argtypes = [dx.C.c_void_p, dx.C.c_int, dx.C.c_void_p]
        for bad in (dx.CirConfig(enable=1, cir=0, correlation=0), dx.CirConfig(enable=1, cir=2, correlation=0), dx.CirConfig(enable=1, cir=1, correlation=-1)):
            assert L.dabx_set_cir_mode(eng._h, 0, dx.C.byref(bad)) == -2
        r = dx.CirConfig(enable=1, cir=1, correlation=0)
        r.reserved[4] = 1
        assert L.dabx_set_cir_mode(eng._h, 0, dx.C.byref(r)) == -2
        assert L.dabx_set_cir_mode(eng._h, 2, None) == -2 and L.dabx_set_cir_mode(eng._h, -2, None) == -2
        assert L.dabx_set_cir_mode(eng._h, -1, None) == 0 and eng.cir_stats(1)["launches"] == 0      # off on an engine without the stage: nothing
    finally:
        eng.close()
