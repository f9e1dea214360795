"""The inputs of the device tests of the PRS correlator and the coarse CFO search (tests/sync_cases.py) qualify, on the CPU alone: the
float64 models decide as the oracle does on every case, every comparison a correlator walk evaluates is at least 2e-5 max(pk) wide,
every branch the cases are there for is taken, the non-finite cases give what the oracle gives, and the distance D from an integer
beyond which the oracle's truncation equals the model's is measured.  `pytest -s` prints the tables (docs/history/sync_stage_tests.md)."""
import numpy as np
import pytest

import oracle_lib as ol
import sync_cases as sc

INT_MIN = sc.INT_MIN


@pytest.fixture(scope="module")
def corr():
    """per window, per threshold: (model result, (oracle first-peak mode, oracle strongest-peak mode))"""
    L = ol.oracle()
    out = {}
    for w in sc.correlator_windows():
        for thr in sc.THRESHOLDS:
            ora = []
            for strongest in (0, 1):
                pr = L.ora_phaseref_new()
                L.ora_phaseref_set_strongest(pr, strongest)
                ora.append(L.ora_phaseref_correlate(pr, w.x, thr))
                L.ora_phaseref_free(pr)
            out[w.name, thr] = (w, sc.model_correlate(w.x, thr), tuple(ora))
    return out


@pytest.fixture(scope="module")
def coarse():
    L = ol.oracle()
    pr = L.ora_phaseref_new()
    out = [(s, sc.model_coarse(s.X), int(L.ora_phaseref_coarse_cfo(pr, s.X))) for s in sc.coarse_spectra()]
    L.ora_phaseref_free(pr)
    return out


# ------------------------------------------------------------------------------------------------ correlator
def test_correlator_model_equals_the_oracle_in_both_modes(corr):
    print()
    for (name, thr), (w, m, ora) in corr.items():
        print("%-20s seed %4d thr %4.1f  model %4d / %4d  oracle %4d / %4d  margin %.1e  peak/mean %7.2f  %s"
              % (name, w.seed, thr, m[0], m[1], ora[0], ora[1], m[3], m[4], " ".join(sorted(m[2]))))
    assert len(corr) == 30 * len(sc.THRESHOLDS)
    for (name, thr), (w, m, ora) in corr.items():
        assert (m[0], m[1]) == ora, (name, thr, m[:2], ora)


def test_every_comparison_of_every_walk_is_at_least_2e_5_wide(corr):
    for (name, thr), (w, m, ora) in corr.items():
        assert m[3] >= sc.MIN_MARGIN and m[5]["clear"], (name, thr, m[3], m[5])


def test_the_cases_pin_what_they_are_there_for(corr):
    for (name, thr), (w, m, ora) in corr.items():
        if w.expect is not None and thr == 3.0:
            assert ora == w.expect, (name, ora, w.expect)
    # strict > from both sides of a near tie, under every threshold
    assert all(corr["near_tie_above", t][2] == (300, 330) and corr["near_tie_below", t][2] == (300, 300) for t in sc.THRESHOLDS)
    # peak / mean at 0.9 x and 1.1 x each threshold: the peak at 504 is taken above and not below (at 3 a noise value may clear it)
    for thr in sc.THRESHOLDS:
        lo, hi = corr["ratio_0.9x%g" % thr, thr], corr["ratio_1.1x%g" % thr, thr]
        assert abs(sc.peak_ratio(lo[0].x, 504) / thr - 0.9) < 1e-3 and abs(sc.peak_ratio(hi[0].x, 504) / thr - 1.1) < 1e-3
        assert 504 not in lo[2] and hi[2] != (-1, -1)
    assert all(corr["ratio_0.9x%g" % t, t][2] == (-1, -1) and corr["ratio_1.1x%g" % t, t][2] == (504, 504) for t in (6.0, 12.0))
    # the scales: recorded, not assumed.  1e15 puts |z|^2 of the peak beyond FLT_MAX: the mean is inf and nothing is above it
    for s, want in (("1e-20", 504), ("1e-10", 504), ("1e+10", 504), ("1e+14", 504), ("1e+15", -1)):
        assert all(corr["scale_" + s, t][2] == (want, want) for t in sc.THRESHOLDS), s
    assert corr["scale_1e+15", 3.0][1][2] == {"overflow"} and corr["zeros", 3.0][1][2] == {"zero_sum"}


def test_every_branch_of_the_walk_is_taken(corr):
    taken = set().union(*[m[2] for _w, m, _o in corr.values()])
    need = {"lookahead_rejects_at_%d" % j for j in (1, 9)} | {"pass_0", "pass_1", "pass_2", "lookahead_cut_at_the_end", "second_peak",
            "later_peak_is_larger", "later_peak_is_not_larger", "skip_jumps_a_larger_value", "nothing_above", "zero_sum", "overflow"}
    assert need <= taken, sorted(need - taken)
    # the look-ahead that crosses the border of the first two passes, and the two modes told apart
    assert "lookahead_rejects_at_7" in corr["pair_505_512", 3.0][1][2]
    assert sum(o[0] != o[1] for _w, _m, o in corr.values()) >= 6


# ------------------------------------------------------------------------------------------------ coarse search
def test_coarse_model_equals_the_oracle(coarse):
    print()
    for s, m, ora in coarse:
        print("%-16s %-5s oracle %11d  model %11d  index %6d  offset*1000 %12.4f  from integer %.1e  runner-up %.1e  5 avg %.1e  %-5s %s"
              % (s.name, s.kind, ora, m["hz"], m["index"], m["hz1000"], m["m_int"], m["m_runner_up"], m["m_found"], sc.coarse_class(m),
                 " ".join(sorted(m["taken"]))))
    for s, m, ora in coarse:
        cls = sc.coarse_class(m)
        assert cls in ("exact", "pm1"), s.name
        assert ora == m["hz"] if cls == "exact" else abs(ora - m["hz"]) <= 1, (s.name, ora, m["hz"])
    n_pm1 = sum(sc.coarse_class(m) == "pm1" for _s, m, _o in coarse)
    assert 10 * n_pm1 <= len(coarse), (n_pm1, len(coarse))


def test_coarse_distance_from_an_integer_beyond_which_truncation_agrees(coarse):
    """D: the largest distance of offset * 1000 from an integer at which the oracle's integer differed from trunc(model)"""
    finite = [(s, m, ora) for s, m, ora in coarse if m["found"] and np.isfinite(m["hz1000"])]
    differ = [(m["m_int"], s.name, ora, m["hz1000"]) for s, m, ora in finite if ora != m["hz"]]
    d = max([x[0] for x in differ], default=0.0)
    print("\nD = %.3e  (%d of %d finite cases differ: %s)" % (d, len(differ), len(finite), differ))
    assert d <= sc.COARSE_D
    assert len(finite) >= 160


def test_coarse_cases_pin_what_they_are_there_for(coarse):
    by = {s.name: (m, ora) for s, m, ora in coarse}
    taken = set().union(*[m["taken"] for m, _o in by.values()])
    assert {"index_+70", "index_-70", "inside", "negative", "positive", "not_found", "all_zero", "all_inf", "some_inf",
            "inf_between_finite_neighbours"} <= taken
    for k in range(-70, 71):                                           # every index of the window is the maximum once
        assert by["roll_%+d" % k][0]["index"] == k and by["roll_%+d" % k][0]["found"]
    for k in (-100, -72, -71, 71, 72, 100):                            # outside it: whatever a side lobe gives, with margin
        assert abs(by["roll_%+d" % k][0]["index"]) <= 70
    # truncation is toward zero on both signs; the argmax changes bin between .499 and .501
    assert by["frac_+0.250"][1] == 42 and by["frac_-4.750"][1] == -4957
    for k in (-70, -5, 0, 5, 69):
        assert by["frac_%+.3f" % (k + 0.501)][0]["index"] == by["frac_%+.3f" % (k + 0.499)][0]["index"] + 1
    # index +-70 interpolates with bin +-71; beyond, the peak has left the window
    assert by["frac_+70.400"][1] > 70000 and by["frac_-70.400"][1] < -70000
    assert abs(by["frac_+70.600"][0]["index"]) < 70 and abs(by["frac_-70.600"][0]["index"]) < 70
    # mx against 5 avg from both sides (the two nearest tell avg / 141 from avg / 140: 0.7 %)
    for t, found in ((0.9, False), (0.99, False), (0.995, False), (1.005, True), (1.01, True), (1.1, True)):
        m, ora = by["noise_%.3f" % t]
        assert m["found"] == found and (ora != sc.IDX_NOT_FOUND) == found
        assert abs((1 / (1 - m["m_found"]) if found else 1 / (1 + m["m_found"])) - t) < 1e-3
    assert by["mix_0.9_1.1"][0]["index"] == -20 and by["mix_1.1_0.9"][0]["index"] == 10
    assert by["white"][1] == sc.IDX_NOT_FOUND
    # non-finite, recorded: all magnitudes 0 -> INT_MIN; seven inf, the first of them between finite neighbours -> its index; more -> INT_MIN
    want = {"zeros": INT_MIN, "scale_1e-25": INT_MIN, "scale_1e-12": 82, "scale_10000": 82, "scale_100000": -64000, "scale_300000": INT_MIN,
            "scale_1e+06": INT_MIN, "scale_1e+09": INT_MIN}
    assert {k: by[k][1] for k in want} == want
    assert "scale_1e-16" not in by and "scale_1e-14" not in by     # squares neither normal nor all zero: left out
