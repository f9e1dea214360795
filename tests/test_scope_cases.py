"""What tests/scope_cases.py promises, shown without a device: the counter model gives the reference's cadence, the cases reach what the
plots can do wrong, the plan of test_gpu_scope_stage.py covers every built plot type, and the model's spread between the two oracle builds
is what scope_cases.py records (so the comparison rule's bar, the project's existing one, lies far outside it)."""
import numpy as np
import pytest

import demap_cases as dc
import scope_cases as sc

LIM = np.float32(np.float32(np.pi / 180.0) * np.float32(20.0))


def _present(s):
    return [f["present"] for f in dc.stream_frames(s)]


def test_the_counter_model_gives_the_references_cadence():
    # from a fresh decoder: decoded frames 3, 5, 7 at symbol 1, then frame 9 at symbol 2 (0-based: 2, 4, 6, 8)
    assert sc.cadence([1] * 10) == [(2, 1), (4, 1), (6, 1), (8, 2)]
    assert sc.cadence(_present(4)) == [(2, 1), (4, 1), (6, 1), (8, 2)]            # the ten-frame integrator stream
    # stream 5 of the plan has an absent frame: no decode_symbol call, neither counter moves -- the cadence of its five decoded frames
    assert _present(5) == [1, 0, 1, 1, 1, 1]
    assert sc.cadence(_present(5)) == sc.cadence([1] * 5) == [(2, 1), (4, 1)]
    steps = [i for i, p in enumerate(_present(5)) if p]
    assert [steps[f] for f, _ in sc.cadence(_present(5))] == [3, 5]               # engine steps: a model that counted the absent frame would say 2, 4
    # the statistics counter moves the symbol on every 6 frames (381 = 5 * 75 + 6 calls), 75 wraps to 1, never 0
    c, syms = sc.Counters(), []
    for _ in range(1000):
        l = c.frame()
        if l:
            syms.append(l)
    assert set(syms) == set(range(1, 76)) and 0 not in syms
    d = np.diff(syms)
    assert set(d.tolist()) <= {0, 1, -74} and (d == -74).sum() >= 1


def test_the_plan_covers_every_built_plot_type_outside_the_undefined_frames():
    carr, iq = set(), set()
    for sym in sc.FIXED_SYMBOLS:
        for s in range(dc.N_STREAMS):
            for step, fr in enumerate(dc.stream_frames(s)):
                if fr["present"] and fr["name"] not in sc.UNDEFINED_NAMES:
                    i, c = sc.plot_plan(sym, s, step)
                    iq.add(i)
                    carr.add(c)
    assert carr == set(sc.CARRIER_TYPES) and iq == set(sc.IQ_TYPES)
    assert sc.UNDEFINED_NAMES == {"zero_carrier", "zero_carrier_next", "zero_reference", "zero_reference_next"}


def test_the_cases_reach_the_branches_of_the_plots():
    # the integrator at both +-20 degree stops, seen by PHASE_ERROR (clock_err = 0: the plot is the integrator in degrees)
    r = sc.model(4, 1, {9: (75,)})[(9, 75)]
    assert (r["integ_front"] == LIM).sum() >= 100 and (r["integ_front"] == -LIM).sum() >= 100
    pe = r["carr"][sc.PHASE_ERROR]
    assert np.isclose(pe.max(), 20.0, atol=1e-4) and np.isclose(pe.min(), -20.0, atol=1e-4)
    assert sc.plot_plan(75, 4, 9)[1] == sc.PHASE_ERROR
    # SB_WEIGHT at 100 % (the upper limit of limit_min_max) on every carrier of a first symbol; the weight is a product of non-negative factors,
    # so the lower limit is reached only by a weight of exactly 0: the zero carrier itself (generators 2 and 3; generator 1 divides 0 by 0)
    sb = sc.model(3, 3, {2: (1,)})[(2, 1)]["carr"][sc.SB_WEIGHT]
    assert (sb == 100.0).sum() >= 100 and ((sb > 0) & (sb < 100.0)).sum() >= 100 and sc.plot_plan(1, 3, 2)[1] == sc.SB_WEIGHT
    _, _, rel = dc._tables()
    for gen in (2, 3):
        z = sc.model(0, gen, {3: (dc.ZERO_SYMBOL,)})[(3, dc.ZERO_SYMBOL)]
        assert z["name"] == "zero_carrier" and z["carr"][sc.SB_WEIGHT][rel[dc.ZERO_CARRIER]] == 0.0
    assert np.isnan(sc.model(0, 1, {3: (dc.ZERO_SYMBOL,)})[(3, dc.ZERO_SYMBOL)]["carr"][sc.SB_WEIGHT][rel[dc.ZERO_CARRIER]])
    # signal_power <= 0 (:225-226)
    na = sc.model(3, 1, {2: (1, 3)})
    assert na[(2, 1)]["name"] == "null_above_signal" and na[(2, 1)]["signal_power_le0"] >= 500 and na[(2, 3)]["signal_power_le0"] >= 500
    # null power exactly 0: SNR is +inf and NULL_OVR_POW is -inf on every carrier
    oa = sc.model(1, 1, {0: (1, 3, 4)})
    assert oa[(0, 1)]["name"] == "on_axes"
    assert np.isposinf(oa[(0, 1)]["carr"][sc.SNR]).all() and np.isneginf(oa[(0, 3)]["carr"][sc.NULL_OVR_POW]).all()
    # an unwrap with jumps beyond +-180
    assert (np.abs(oa[(0, 4)]["unwrap_raw_diff"]) > 180.0).sum() >= 100
    un = oa[(0, 4)]["carr"][sc.PRS_PHASE_UNWRAP]
    assert np.abs(np.diff(un)).max() <= 180.0 + 1e-9 and np.ptp(un) > 360.0
    # the start-up symbol: the running mMeanPowerOvrAll (:214, inside the carrier loop) and the value behind the symbol differ by more than a
    # factor of 10 -- a device that used the block value for REL_POWER / NULL_OVR_POW is 10 dB off and more
    g = sc.model(2, 1, {0: (1,)})[(0, 1)]
    assert g["name"] == "gain_1e5" and g["mpa"] == 1.0
    assert g["mpa_behind"] / g["mpa_running"][0] > 10.0 and g["mpa_behind"] / g["mpa_running"][K_HALF] > 10.0 / 6
    assert np.isclose(g["mpa_running"][-1], g["mpa_behind"], rtol=1e-5)                  # the closed form against the oracle's serial float recurrence
    assert sc.plot_plan(1, 2, 0) == (1, sc.REL_POWER)
    rp_block = 10.0 * np.log10(g["mpa_running"][-1] / g["mpa_running"])
    assert rp_block.max() > 10.0                                                         # ... in dB, against a bound of 0.02


K_HALF = dc.K // 2


def test_nothing_is_left_out_and_what_the_literal_rule_names_is_recorded():
    """Every degree value and every first difference compares modulo 360, so the wrap decision at +-180 never enters and compare_carr leaves
    nothing out (0 <= LEFT_OUT_CAP).  What the literal rule names -- raw first differences of PRS_PHASE within the bound of +-180 -- is 0 on
    every frame but on_axes, whose PRS phases are exact multiples of 90 degrees (a quarter of its differences are +-180 exactly)."""
    for s in range(dc.N_STREAMS):
        n = sum(_present(s))
        for (f, _), r in sc.model(s, 1, {i: (1,) for i in range(n)}).items():
            share = sc.left_out_share(r["unwrap_raw_diff"])
            if r["name"] == "on_axes":
                assert 0.2 < share < 0.3
            elif r["name"] not in sc.UNDEFINED_NAMES:
                assert share == 0.0, (r["name"], share)
    # the comparison is indifferent to the wrap decision: the model against itself with every +-180 difference flipped
    oa = sc.model(1, 1, {0: (4,)})[(0, 4)]["carr"][sc.PRS_PHASE_UNWRAP]
    d = np.diff(oa)
    flipped = np.concatenate([oa[:1], oa[0] + np.cumsum(np.where(np.abs(np.abs(d) - 180.0) < 1e-6, -d, d))])
    assert not np.allclose(flipped, oa) and sc.compare_carr(flipped, oa, sc.PRS_PHASE_UNWRAP)[0] == 0


def test_the_rule_refuses_what_it_should():
    r = sc.model(2, 1, {0: (1,)})[(0, 1)]
    x = r["carr"][sc.REL_POWER]
    assert sc.compare_carr(x.astype(np.float32), x, sc.REL_POWER)[0] == 0
    assert sc.compare_carr(x + 0.03, x, sc.REL_POWER)[0] == dc.K
    shift = np.zeros(dc.K)
    shift[dc._tables()[2]] = 10.0 * np.log10(r["mpa_running"] / r["mpa_running"][-1])
    assert sc.compare_carr(x + shift, x, sc.REL_POWER)[0] > 1000                         # the block value instead of the running one
    oa = sc.model(1, 1, {0: (1,)})[(0, 1)]["carr"][sc.SNR]
    assert sc.compare_carr(oa, oa, sc.SNR)[0] == 0 and sc.compare_carr(-oa, oa, sc.SNR)[0] == dc.K and sc.compare_carr(np.zeros(dc.K), oa, sc.SNR)[0] == dc.K
    iq = r["iq"][1]
    assert sc.compare_iq(iq.astype(np.complex64), iq)[0] == 0 and sc.compare_iq(iq * (1 + 2e-4), iq)[0] > 1000
    ang = r["carr"][sc.FOUR_QUAD_PHASE]
    assert sc.compare_carr(ang + 360.0, ang, sc.FOUR_QUAD_PHASE)[0] == 0 and sc.compare_carr(ang + 0.02, ang, sc.FOUR_QUAD_PHASE)[0] == dc.K


@pytest.mark.parametrize("s", range(dc.N_STREAMS))
def test_spread_between_the_two_oracle_builds_is_as_recorded(s):
    """The model on the IEEE oracle against the model on the build with the reference's own float flags, symbols 1, 4, 10, 75 of every frame
    outside the zero_* frames: |d| / (1 + |x|) stays under the recorded constants, and no value changes its class (NaN, +inf, -inf)."""
    n = sum(_present(s))
    want = {i: sc.SPREAD_SYMBOLS for i in range(n)}
    worst_sb = worst = 0.0
    for gen in dc.GENERATORS:
        a, b = sc.run_model(s, gen, want), sc.run_model(s, gen, want, fast=True)
        assert a.keys() == b.keys() and len(a) == 4 * n
        for key, ra in a.items():
            if ra["name"] in sc.UNDEFINED_NAMES:
                continue
            rb = b[key]
            vals = [(t, ra["carr"][t], rb["carr"][t]) for t in sc.CARRIER_TYPES]
            vals += [("iq", np.concatenate([ra["iq"][t].real, ra["iq"][t].imag]), np.concatenate([rb["iq"][t].real, rb["iq"][t].imag])) for t in sc.IQ_TYPES]
            for t, x, y in vals:
                if t == sc.PRS_PHASE_UNWRAP:
                    x, y = np.concatenate([x[:1], np.diff(x)]), np.concatenate([y[:1], np.diff(y)])
                fin = np.isfinite(x)
                assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~fin & ~np.isnan(x)], y[~fin & ~np.isnan(x)]), (key, ra["name"], t)
                assert np.isfinite(y[fin]).all(), (key, ra["name"], t)
                if not fin.any():
                    continue
                d = np.abs(sc._wrap180(x[fin] - y[fin])) if t in sc.DEGREE else np.abs(x[fin] - y[fin])
                v = float((d / (1.0 + np.abs(x[fin]))).max())
                if t == sc.SB_WEIGHT:
                    worst_sb = max(worst_sb, v)
                else:
                    worst = max(worst, v)
    print("stream %d: largest |d| / (1 + |x|) between the oracle builds: SB_WEIGHT %.2e, every other plot %.2e" % (s, worst_sb, worst))
    assert worst_sb <= sc.SPREAD_SB_WEIGHT and worst <= sc.SPREAD_OTHER
    assert sc.SPREAD_SB_WEIGHT < sc.REL / 5 and sc.SPREAD_OTHER < sc.REL / 50           # far inside the rule's bar
