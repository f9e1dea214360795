"""The inputs and models of the spectrum / waterfall tests (tests/spectrum_cases.py) qualify, on the CPU alone: the float32 line-by-line
transcription against the float64 model on the crafted windows -- the measured float-vs-float64 deviation, which must stay under a quarter
of the 2e-5 bar the device is held to --; the condition of the comparison rule (every bin's dB bound <= 0.01 dB outside the notch and zero
windows); the waterfall's excusable pixels (at most 2 % per case for the transcription alone); and the schedule model on the oracle
receiver's trace of the engine test's own signals, which must contain a show while searching, a show at a symbol end in lock and a show in
the first frame after a lost lock.  `pytest -s` prints the tables (docs/history/spectrum.md)."""
import numpy as np
import pytest

import oracle_lib as ol
import spectrum_cases as sp

MOVED = 3          # cases that had to be moved to meet the condition: tone_bin_centre, tone_between_bins and tone_1024 had a largest bound of
                   # 0.0133, 0.0116 and 0.0135 dB over a noise floor of 2.0; the floor under every tone is 3.0 now.  None for the pixel cap.


def fft32(x):
    return ol.ora_fft(x)


@pytest.fixture(scope="module")
def rows():
    """every crafted window through a fresh display buffer: (name, model tuple, transcription tuple)"""
    out = []
    for name, x, why in sp.windows():
        m = sp.Row64().show(x)
        t = sp.row32(x, np.zeros(sp.BINS, np.float32), fft32)
        out.append((name, m, t, why))
    return out


def test_the_float32_transcription_against_the_float64_model(rows):
    """Linear values: the bar is 2e-5 of the window's largest model value; the transcription alone must lie within a quarter of it."""
    print()
    worst = 0.0
    assert len(rows) == 15
    for name, (y, v, d, ext, b, bd), (y32, v32, d32), why in rows:
        if name in sp.EXACT_NAN:
            assert np.isnan(d32).all() and np.isnan(d).all(), name
            assert sp.extrema(list(d32)) == [-1000.0, 1000.0, -1000.0, 1000.0]
            print("%-18s NaN in every bin, the extrema untouched  %s" % (name, why))
            continue
        if name == "zeros":
            assert (y32 == 0).all() and (v32.view(np.uint32) == np.float32(sp.VAL_OF_ZERO).view(np.uint32)).all()
            assert abs(float(sp.VAL_OF_ZERO) + 120.0) < 1e-4
            print("%-18s every val %.9g (bits %08x)  %s" % (name, float(sp.VAL_OF_ZERO), int(np.float32(sp.VAL_OF_ZERO).view(np.uint32)), why))
            continue
        rel = float(np.abs(y32.astype(np.float64) - y).max() / y.max())
        dberr = float((np.abs(v32.astype(np.float64) - v) / b).max())
        worst = max(worst, rel)
        print("%-18s largest lin %-12.6g lin rel %.2e  dB error / bound %.3f  largest bound %.2e dB  %s" % (name, y.max(), rel, dberr, b.max(), why))
        assert dberr <= 1.0, name
    print("largest float32-vs-float64 deviation of the linear values: %.2e (a quarter of the bar: %.1e)" % (worst, sp.BAR / 4))
    assert worst <= sp.BAR / 4


def test_the_condition_of_the_comparison_rule_holds(rows):
    """In every case except the notch and the zero windows every bin's bound is <= 0.01 dB."""
    for name, (y, v, d, ext, b, bd), _, _ in rows:
        if sp.IN_CONDITION(name):
            assert b.max() <= 0.01, (name, b.max())


def test_the_waterfall_pixels_of_the_transcription_stay_under_the_cap(rows):
    """An index may differ from the model's by 1, and only where the model's t * 255 lies within the bin's dB bound x 255 / yRange of an
    integer; at most 2 % of a case's 512 pixels may be excused.  The transcription alone stays under that on every case, for zoom 0 and 100."""
    print()
    for name, (y, v, d, ext, b, bd), (y32, v32, d32), _ in rows:
        if name in sp.EXACT_NAN:
            continue
        for zoom in (0, 100):
            lim, y_min, y_max, valid, _ = sp.limits32(ext, sp.LIMITS0, sp.ALPHA["fast"], zoom)      # (fast: the limits are the show's own extrema, the row spans the scale)
            assert valid
            want, t255 = sp.pixels(d, float(y_min), float(y_max))
            got, _ = sp.pixels(d32, y_min, y_max, np.float32)
            near = np.abs(t255 - np.round(t255)) <= bd * 255.0 / float(y_max - y_min)
            diff = got != want
            assert (np.abs(got - want) <= 1).all() and not (diff & ~near).any(), (name, zoom)
            print("%-18s zoom %3d: %d pixels differ by 1, %d excusable" % (name, zoom, int(diff.sum()), int(near.sum())))
            assert diff.sum() <= 0.02 * sp.BINS, (name, zoom)


def test_the_iir_walk_of_the_sequence():
    """six windows through one state: the transcription follows the model within the bound that goes through the same recurrence"""
    m, d32 = sp.Row64(), np.zeros(sp.BINS, np.float32)
    for k, x in enumerate(sp.sequence()):
        y, v, d, ext, b, bd = m.show(x)
        _, _, d32 = sp.row32(x, d32, fft32)
        assert (np.abs(d32.astype(np.float64) - d) <= bd).all(), k
        assert bd.max() <= 0.01
    assert abs(d).max() > 10.0


def test_the_schedule_model_on_the_engine_tests_signals():
    """The engine test is admissible only if the oracle's run of its signals has a show while searching, one at a symbol end in lock and
    one in the first frame after a lost lock -- and no search candidate whose correlation fails (the stated deviation)."""
    print()
    xs = sp.engine_float_signals()
    for kind in ("cf32", "s16", "u8"):
        what = set()
        for s, x in enumerate(xs):
            _, vals = sp.to_ring(x, kind)
            shows, end, search_fails, tr = sp.engine_schedule(vals)
            assert search_fails == 0 and len(shows) >= 4
            kinds = [int(e["kind"]) for e in tr]
            lost_at = [sum(1 for q in kinds[:k] if q == sp.EV_FRAME_DONE) for k in range(1, len(kinds))
                       if kinds[k] == sp.EV_CORR_FAILED and kinds[k - 1] == sp.EV_FRAME_DONE]
            for W, E, frames, doing in shows:
                what.add("searching" if doing == "search" else "in_lock")
                if doing == "frame" and frames in lost_at:
                    what.add("first_frame_after_a_lost_lock")
                if doing == "frame":
                    assert any((E - int(e["pos"]) + sp.TN) % sp.TS == 0 for e in tr if int(e["kind"]) == sp.EV_FRAME_DONE and int(e["pos"]) > E)
                assert E - W > sp.PERIOD
            print(kind, "stream", s, [(W, E, f, d) for W, E, f, d in shows], "lock lost with", lost_at, "frames decoded")
        assert what == {"searching", "in_lock", "first_frame_after_a_lost_lock"}, (kind, what)


def test_the_librarys_look_follows_the_oracle_trace():
    """spectrum_look (csrc/spectrum_core.h), the function that decides the schedule inside k_spectrum, through dabx_spectrum_look: driven
    step by step with what the search and the frame head leave (spectrum_cases.looks_of_trace), it shows where the call-by-call Reader
    shows -- on the engine test's signals, and on hand-made traces with a search candidate whose correlation fails: exact where sample
    W + 512 000 lies outside the candidate's T_u block (inexact is set all the same: the look cannot know), up to 2048 samples early
    where it lies inside -- the stated deviation, measured here."""
    from dabstar_amd import lib as dx
    TU, TS, TN, P = sp.TU, sp.TS, sp.TN, sp.PERIOD
    for s, x in enumerate(sp.engine_float_signals()):
        shows, end, search_fails, tr = sp.engine_schedule(x)
        got = sp.looks_of_trace(tr, dx.spectrum_look)
        assert [(E, 0, fr) for _, E, fr, _ in shows] == got, s
        # switched on later, at a frame's end
        at = [int(e["pos"]) for e in tr if int(e["kind"]) == sp.EV_FRAME_DONE][3]
        later, _ = sp.shows_of_trace(tr, at)
        assert [(E, 0, fr) for _, E, fr, _ in later] == sp.looks_of_trace(tr, dx.spectrum_look, at) and later[0][0] == at

    def frame(D, start):
        return [(sp.EV_DIP_END, D), (sp.EV_CORR_OK, D + TU), (sp.EV_FRAME_DONE, D + TU + start + 75 * TS + TN)]

    def follow(events):
        tr = sp.trace_of(events)
        want, _ = sp.shows_of_trace(tr)
        return [E for _, E, _, _ in want], sp.looks_of_trace(tr, dx.spectrum_look)
    # a candidate fails well in front of sample 512 000, the search goes on and gives up a frame later: exact
    want, got = follow([(sp.EV_SEEDED, 20 * TU), (sp.EV_DIP_END, 300000), (sp.EV_CORR_FAILED, 300000 + TU), (sp.EV_NO_DIP, 300000 + TU + sp.TF + 50),
                        (sp.EV_NO_DIP, 300000 + TU + 2 * sp.TF + 100)])
    assert want == [P + 1] and got == [(P + 1, 0, 0)]               # (the failure lies in an earlier pass than the show: not even flagged)
    # ... the same in ONE pass of the search, sample 512 000 outside the block: exact, but flagged -- the look cannot know
    want, got = follow([(sp.EV_SEEDED, 20 * TU), (sp.EV_DIP_END, 400000), (sp.EV_CORR_FAILED, 400000 + TU), (sp.EV_NO_DIP, 400000 + TU + sp.TF + 50)])
    assert want == [P + 1] and got == [(P + 1, 1, 0)]
    # ... no candidate fails: exact, not flagged
    want, got = follow([(sp.EV_SEEDED, 20 * TU), (sp.EV_NO_DIP, 20 * TU + sp.TF + 50), (sp.EV_NO_DIP, 20 * TU + 2 * sp.TF + 100), (sp.EV_NO_DIP, 20 * TU + 3 * sp.TF + 150)])
    assert want == [P + 1] and got == [(P + 1, 0, 0)]
    # sample 512 000 inside the failed candidate's block: the reference shows with the first call behind the block, the look up to 2048 early
    early = []
    for into in (0, 1, 1000, TU - 1):
        D = P - into
        want, got = follow([(sp.EV_SEEDED, 20 * TU), (sp.EV_DIP_END, D), (sp.EV_CORR_FAILED, D + TU), (sp.EV_NO_DIP, D + TU + sp.TF + 50)])
        assert want == [D + TU + 1] and got == [(P + 1, 1, 0)]
        early.append(want[0] - got[0][0])
    assert early == [TU, TU - 1, TU - 1000, 1] and max(early) <= TU
    # ... and the candidate correlates: the block and the rest of symbol 0 do not show, the first symbol end does -- exact, the search held no failure
    for into in (0, 1000, TU - 1):
        D = P - into
        want, got = follow([(sp.EV_SEEDED, 20 * TU)] + frame(D, 504))
        assert want == [D + TU + 504 + TS] and got == [(want[0], 0, 0)]
    # a correlation that fails in lock: the block the head read does not show, the search behind it does -- exact, not flagged, also where
    # sample 512 000 lies inside that block (the look knows where the head's block lay)
    for D0, inside in ((100000, False), (P - 393212 - 1000, True)):
        f1 = frame(D0, 504)
        end1 = f1[-1][1]
        f2 = [(sp.EV_CORR_OK, end1 + TU), (sp.EV_FRAME_DONE, end1 + TU + 500 + 75 * TS + TN)]       # (a second frame, then the failure)
        end2 = f2[-1][1]
        assert (end2 <= P < end2 + TU) == inside
        want, got = follow([(sp.EV_SEEDED, 20 * TU)] + f1 + f2 + [(sp.EV_CORR_FAILED, end2 + TU)] +
                           [(sp.EV_NO_DIP, end2 + TU + k * (sp.TF + 50)) for k in range(1, 5)])
        assert len(want) == 2 and [g[0] for g in got] == want and all(g[1] == 0 for g in got) and got[1][2] == 2
        assert want[0] == (end2 + TU + 1 if inside else P + 1) and want[1] == want[0] + P + 1
    L = dx.load()
    assert L.dabx_spectrum_look(None, 0, 0, 0, 0, 0, None) == -2
