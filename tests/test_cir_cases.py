"""The inputs and models of the CIR / correlation plot tests (tests/cir_cases.py) qualify, on the CPU alone: the float64 row model against
the oracle's own float transform path on the crafted rows -- the measured float-vs-float64 deviation, which must stay under a quarter of the
bar the device is held to --; the correlation model's start index against the oracle correlator's on the windows of tests/sync_cases.py;
the branches every input reaches; the window schedule a host sees that commits a frame per step.  `pytest -s` prints the tables
(docs/history/cir.md)."""
import numpy as np

import cir_cases as cc
import oracle_lib as ol
import sync_cases as sc


def oracle_row(x):
    """cir_viewer.cpp:69-93 through the oracle's float transform (ol.ora_fft, unnormalised), every step in float32"""
    X = ol.ora_fft(np.asarray(x, np.complex64))
    ref = cc.PRS.astype(np.complex64)
    a, b = X.view(np.float32).reshape(-1, 2), ref.view(np.float32).reshape(-1, 2)
    p = np.empty_like(a)
    p[:, 0] = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]                          # X * conj(ref), four products and two sums in float
    p[:, 1] = a[:, 1] * b[:, 0] - a[:, 0] * b[:, 1]
    z = ol.ora_fft(p.view(np.complex64).reshape(-1), inverse=True).view(np.float32).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        n = z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]
    mx = np.float32(0)
    for v in n:
        if v > mx:
            mx = v
    return np.sqrt(mx) / np.float32(cc.SCALE)


def test_the_row_model_against_the_oracles_float_transform():
    """The bar is 2e-5 of the row's model value.  The oracle's float path alone must lie within a quarter of it of the float64 model, or the
    bar would have to be four times what is measured here; the exact rows are exact in float as well."""
    print()
    worst = 0.0
    rows = cc.rows()
    assert len(rows) == 15
    for name, x, why in rows:
        kind, want = cc.row_expectation(name, x)
        got = float(oracle_row(x))
        if kind == "exact":
            assert got == want, (name, got, want)
            print("%-22s exact %-10g %s" % (name, want, why))
        else:
            rel = abs(got - want) / want
            worst = max(worst, rel)
            print("%-22s model %-14.8g oracle float %-14.8g rel %.2e  %s" % (name, want, got, rel, why))
    print("largest float-vs-float64 deviation of the oracle's own path: %.2e (a quarter of the bar: %.1e)" % (worst, cc.BAR / 4))
    assert worst <= cc.BAR / 4
    # the unit tap, wherever it lies
    assert all(abs(cc.row_model(x) / (np.sqrt(1536.0) * 2048 / cc.SCALE) - 1) < 1e-6 for _, x, _ in rows[:5])    # (the samples are floats)
    # strict `>` from 0: a row of zeros, and a row whose squares all vanish, never enter the maximum
    assert cc.row_model(np.zeros(cc.TU, np.complex64)) == 0.0


def test_the_correlation_model_finds_the_oracle_correlators_index():
    """CorrPlot.call on |corr| of the sync_cases windows: its start index (first-peak mode) is the oracle correlator's, under every threshold;
    windows whose magnitudes leave the float range are listed and left out (the model is float64)."""
    L = ol.oracle()
    print()
    n, left_out, branches = 0, [], set()
    for w in sc.correlator_windows():
        for thr in sc.THRESHOLDS:
            m = sc.model_correlate(w.x, thr)
            if m[5]["overflow"] or (m[5]["all_zero"] and w.name != "zeros") or not m[5]["normal"]:
                left_out.append((w.name, thr))
                continue
            pr = L.ora_phaseref_new()
            want = L.ora_phaseref_correlate(pr, w.x, thr)
            L.ora_phaseref_free(pr)
            plot = cc.CorrPlot()
            start, show = plot.call(cc.corr_pk(w.x), thr)
            assert start == want == m[0] and show is None, (w.name, thr, start, want)
            assert plot.margin >= cc.BAR or w.name == "zeros", (w.name, plot.margin)
            branches |= plot.branches
            print("%-20s thr %4.1f start %4d %s" % (w.name, thr, start, " ".join(sorted(plot.branches))))
            n += 1
    print("left out (outside the float range):", sorted(set(k for k, _ in left_out)))
    assert n >= 75 and {"zero_sum", "accumulated_but_not_counted", "counted"} <= branches
    assert set(k for k, _ in left_out) <= {"scale_1e-20", "scale_1e+15"}


def test_the_state_machine_shows_every_sixth_counted_call_and_keeps_the_mean():
    """:121, :128, :171, :179-193 on a scripted sequence of windows: the mean takes every call, only calls with an accepted peak count, the
    sixth of them shows mean / 6 with all its indices, and the next show carries a sixth of the one before."""
    good = cc.corr_pk(sc.make_window([(504, 1.0), (804, 0.5)], 0.05, 1))
    weak = cc.corr_pk(sc.make_window([], 1.0, 2))                            # noise: nothing above 6 x the mean
    zero = np.zeros(cc.TU)
    plot, shows, script = cc.CorrPlot(), [], [good, weak, good, zero, good, good, good, good, good, weak, good, good, good, good, good]
    total = np.zeros(cc.TU)
    one = cc.CorrPlot()
    one.counter = 5
    indices = one.call(good, 6.0)[1][2]                                      # what one call's walk accepts: both paths, in walk order
    assert indices[0] == 504 and 804 in indices and indices == sorted(indices)
    for k, pk in enumerate(script):
        start, show = plot.call(pk, 6.0)
        total += pk
        assert (start >= 0) == (pk is good)
        if show is not None:
            shows.append((k, show))
            total /= 6
            assert np.array_equal(show[0], total) and show[2] == indices
            assert show[1] == good.sum() / cc.TU * 6.0
    assert [k for k, _ in shows] == [7, 14]                                  # the sixth and the twelfth counted call
    assert plot.terms == len(script) and {"zero_sum", "accumulated_but_not_counted", "counted", "show_2_indices"} == plot.branches
    first, second = shows[0][1][0], shows[1][1][0]
    assert np.abs(second - (first + weak + 6 * good) / 6).max() < 1e-9 * second.max()     # the uncleared mean
    # the bound of the index list: a comb of equal peaks 11 apart fills it
    comb = np.zeros(cc.TU)
    comb[cc.I0:cc.I1:11] = 1000.0
    plot = cc.CorrPlot()
    plot.counter = 5
    start, show = plot.call(comb + 1.0, 3.0)
    assert start == cc.I0 and len(show[2]) == cc.MAX_INDICES == 69 and show[2][-1] == cc.I0 + 68 * 11 < cc.I1


def test_the_schedule_of_a_host_that_commits_a_frame_per_step():
    """The rows of a window become due while its 198 656 samples are committed: with a frame per step, 381 rows in the step that brings the
    window's first frame, the last 4 in the next, none in the four steps behind -- and a step with nothing due launches nothing."""
    w, per_step, done_at = cc.Walk(0), [], []
    for step in range(1, 14):
        n, first, done = w.step(step * cc.TF)
        per_step.append(n)
        if done:
            done_at.append(step)
    assert per_step == [381, 4, 0, 0, 0, 0, 381, 4, 0, 0, 0, 0, 381] and done_at == [2, 8]
    # a host that commits everything first: a window per step, 385 rows each
    w = cc.Walk(4243)
    assert [w.step(40 * cc.TF)[::2] for _ in range(3)] == [(385, 1)] * 3 and w.win == 3
    # the trust table has both answers for every clause
    t = cc.trust_table()
    assert any(x[4] and x[0] < x[1] for x in t) and any(not x[4] for x in t) and any(x[4] and x[0] >= x[1] and x[2] == cc.U64 for x in t)
