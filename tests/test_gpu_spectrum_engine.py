"""The spectrum / waterfall stage inside the running engine (dabx_set_spectrum_mode, dabx_read_spectrum; pipeline.hip k_spectrum), through
IQ, for cf32 / s16 / u8 rings.  Three streams of one FIC-only engine, every sample committed before the first step
(tests/spectrum_cases.py engine_float_signals): 0 clean; 1 with an echo and a carrier offset, averaging fast and zoom 100; 2 behind 2.9
frames of noise -- its first window is shown while it searches -- and with a drop-out that loses and regains the lock.  After EVERY
dabx_process call the new records are held against the schedule model (the oracle receiver's trace of the same quantised samples through
sample_reader.cpp:285-296): first_sample, the frame counter, the number of records and the counters exactly; db, the limits and the
waterfall row under the comparison rule.  Steps of one frame and calls of seven frames give byte-identical records; switching stream 0
off and on restarts its state at the read position."""
import numpy as np
import pytest

import spectrum_cases as sp
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu
KINDS = ["cf32", "s16", "u8"]
S = 3
STEPS = 18
RESTART_AFTER = 8                                # steps before stream 0 is switched off and on
MODES = [("medium", 0), ("fast", 100), ("medium", 0)]


def run(kind, pushed, batch):
    """-> per call [(steps so far, read position per stream, frames per stream, new records per stream)], stream 0's read position at its restart, stats"""
    eng = dx.Engine(n_streams=S, ring_frames=18, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, ring_format=kind)
    try:
        for s in range(S):
            eng.push_iq(s, pushed[s])
        assert eng.spectrum_stats(0) == dict(shows=0, untrusted=0, lost=0, launches=0, inexact=0) and eng.read_spectrum(0) == ([], 0)
        for s in range(S):
            eng.set_spectrum_mode(s, averaging=MODES[s][0], zoom=MODES[s][1])
        log, steps, restart = [], 0, None
        while steps < STEPS:
            if steps == RESTART_AFTER:
                restart = int(dx.front_read(eng, 0, spectra=False)["rd"])
                eng.set_spectrum_mode(0, enable=False)
                eng.set_spectrum_mode(0, averaging=MODES[0][0], zoom=MODES[0][1])
            m = 1 if steps == 0 else min(batch, (RESTART_AFTER if steps < RESTART_AFTER else STEPS) - steps)
            assert eng.process(m) == m
            steps += m
            rd = [int(dx.front_read(eng, s, spectra=False)["rd"]) for s in range(S)]
            frames = [eng.stats(s)["frames"] for s in range(S)]
            new = []
            for s in range(S):
                recs, lost = eng.read_spectrum(s, 8)
                assert lost == 0
                new.append([(r.copy(), l.copy(), d.copy(), w.copy()) for r, l, d, w in recs])
            log.append((steps, rd, frames, new, [eng.spectrum_stats(s) for s in range(S)]))
        return log, restart, [eng.spectrum_stats(s) for s in range(S)]
    finally:
        eng.close()


@pytest.fixture(scope="module", params=KINDS)
def world(request):
    """Per ring format: the signals, the schedule models and the two runs.  Computed once, shared, left unchanged."""
    kind = request.param
    pushed, vals = zip(*[sp.to_ring(x, kind) for x in sp.engine_float_signals()])
    a = run(kind, pushed, 1)
    b = run(kind, pushed, 7)
    sched = [sp.engine_schedule(v) for v in vals]
    assert all(q[2] == 0 for q in sched)                  # no search candidate fails its correlation: every show position is exact
    return dict(kind=kind, vals=vals, a=a, b=b, sched=sched)


class Model:
    """one stream's SpectrumViewer in float64 with the bounds of the comparison rule"""

    def __init__(self, averaging, zoom):
        self.row, self.lim, self.bl, self.alpha, self.zoom = sp.Row64(), list(sp.LIMITS0), 0.0, sp.ALPHA[averaging], zoom

    def check(self, rec, lim, db, row, W, frames, x):
        assert (int(rec["first_sample"]), int(rec["frame"]), int(rec["untrusted"]), int(rec["inexact"])) == (W, frames, 0, 0)
        y, v, d, ext, b, bd = self.row.show(x)
        assert (np.abs(db.astype(np.float64) - d) <= bd).all(), float((np.abs(db - d) / bd).max())
        self.lim, y_min, y_max, valid, _ = sp.limits32(ext, self.lim, self.alpha, self.zoom)
        self.bl = (1.0 - self.alpha) * self.bl + self.alpha * bd.max()
        got = [float(lim[k]) for k in ("glob_max", "glob_min", "loc_max", "loc_min")]
        assert (np.abs(np.array(got) - np.array(self.lim, np.float64)) <= self.bl + sp.LIMIT_SLACK).all(), (got, self.lim)
        tol = self.bl + sp.Y_SLACK                         # (spectrum_cases.py: the float32 operations themselves)
        assert abs(float(lim["y_min"]) - y_min) <= tol and abs(float(lim["y_max"]) - y_max) <= tol and int(rec["row_valid"]) == int(valid)
        want, t255 = sp.pixels(d, float(y_min), float(y_max))
        diff = row.astype(np.int64) != want
        near = np.abs(t255 - np.round(t255)) <= bd * 255.0 / float(y_max - y_min)
        assert (np.abs(row.astype(np.int64) - want) <= 1).all() and not (diff & ~near).any() and diff.sum() <= 0.02 * sp.BINS, int(diff.sum())
        return float((np.abs(db - d) / bd).max())


def test_every_call_against_the_schedule_and_the_models(world):
    log, restart, stats = world["a"]
    print()
    seen_what = set()
    for s in range(S):
        shows, end, _, tr = world["sched"][s]
        if s == 0:
            assert restart is not None
            later, _ = sp.shows_of_trace(tr, restart)
            shows = [q for q in shows if q[1] <= restart] + later
            assert len(later) >= 1 and later[0][0] == restart
        model, k = Model(*MODES[s]), 0
        for steps, rd, frames, new, st_now in log:
            if s == 0 and steps == RESTART_AFTER + 1:
                model = Model(*MODES[s])                  # a fresh viewer behind the restart
            due = [q for q in shows[k:] if q[1] <= rd[s]]
            assert len(new[s]) == len(due), (world["kind"], s, steps, [int(r[0]["first_sample"]) for r in new[s]], due)
            for (rec, lim, db, row), (W, E, fr, what) in zip(new[s], due):
                worst = model.check(rec, lim, db, row, W, fr, world["vals"][s][W:W + sp.SIZE])
                seen_what.add(what)
                print("%s stream %d step %2d: W %8d shown at %8d (%s), %d frames decoded, dB error / bound %.3f" % (world["kind"], s, steps, W, E, what, fr, worst))
            k += len(due)
            assert st_now[s] == dict(shows=k, untrusted=0, lost=0, launches=steps, inexact=0), (steps, st_now[s])     # the counters, after every call
        assert k >= 4
        assert stats[s] == dict(shows=k, untrusted=0, lost=0, launches=STEPS, inexact=0), stats[s]
    assert seen_what == {"search", "frame"}


def test_steps_of_one_frame_and_calls_of_seven_give_identical_records(world):
    (la, ra, sa), (lb, rb, sb) = world["a"], world["b"]
    assert ra == rb and sa == sb
    for s in range(S):
        fa = [x for _, _, _, new, _ in la for x in new[s]]
        fb = [x for _, _, _, new, _ in lb for x in new[s]]
        assert len(fa) == len(fb) >= 4
        for x, y in zip(fa, fb):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def test_switching_off_and_on_restarts_the_state(world):
    log, restart, _ = world["a"]
    recs = [x for _, _, _, new, _ in log for x in new[0]]
    after = [x for x in recs if int(x[0]["first_sample"]) >= restart]
    assert int(after[0][0]["first_sample"]) == restart
    # a fresh display buffer holds 0.2 val; the one of the record before, its third show, 1 - 0.8^3 = 0.488 val of much the same spectrum
    before = [x for x in recs if int(x[0]["first_sample"]) < restart]
    assert len(before) == 3 and np.abs(after[0][2]).max() < 0.5 * np.abs(before[-1][2]).max()
    assert [float(after[0][1][k]) for k in ("glob_max", "glob_min")] != [float(before[-1][1][k]) for k in ("glob_max", "glob_min")]


def test_a_window_that_is_not_trusted_is_not_evaluated():
    """One stream of noise, searching.  Its first window starts at the read position at which the mode is switched on and is looked at
    behind the search of the same step, so it lies behind the read position: with a producer that commits without saying how far it
    writes (the write horizon is ~0 from the commit on) no clause of the trust rule holds -- the record is emitted with untrusted = 1, db,
    limits and row as they stood (a fresh viewer: zeros and the initial limits), the IIR does not move, and the window is counted.  The twin
    whose samples were all pushed (the horizon is what was pushed, less than a ring length) evaluates the same window."""
    rng = np.random.default_rng(7)
    x = (0.2 * (rng.standard_normal(5 * sp.TF) + 1j * rng.standard_normal(5 * sp.TF))).astype(np.complex64)
    out = []
    for zero_copy in (True, False):
        eng = dx.Engine(n_streams=1, ring_frames=8, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1)
        try:
            eng.push_iq(0, x)
            if zero_copy:
                eng.commit(0)                              # a zero-copy commit (of nothing more): the producer's writes are unknown from here on
            eng.set_spectrum_mode(0)
            recs = []
            for _ in range(4):
                eng.process(1)
                recs += eng.read_spectrum(0)[0]
            assert eng.stats(0)["frames"] == 0
            out.append((recs, eng.spectrum_stats(0)))
        finally:
            eng.close()
    (bad, bad_stats), (good, good_stats) = out
    assert len(bad) == len(good) == 1
    rec, lim, db, row = bad[0]
    assert (int(rec["first_sample"]), int(rec["frame"]), int(rec["untrusted"]), int(rec["row_valid"]), int(rec["inexact"])) == (0, 0, 1, 0, 0)
    assert not db.any() and not row.any()
    assert [float(lim[k]) for k in ("glob_max", "glob_min", "loc_max", "loc_min", "y_min", "y_max")] == list(sp.LIMITS0) + [0.0, 0.0]
    assert bad_stats == dict(shows=1, untrusted=1, lost=0, launches=4, inexact=0)
    rec, lim, db, row = good[0]
    assert (int(rec["first_sample"]), int(rec["untrusted"]), int(rec["row_valid"])) == (0, 0, 1) and good_stats == dict(shows=1, untrusted=0, lost=0, launches=4, inexact=0)
    y, v, d, ext, b, bd = sp.Row64().show(x[:sp.SIZE])
    assert (np.abs(db.astype(np.float64) - d) <= bd).all()
