"""The inputs of the null-symbol search's stage test, on the oracle alone (no device): what the crafted signals of tests/acquire_cases.py
reach -- asserted from the oracle's event trace: kinds, block positions, residues, counts, the margin count --, that each named
off-by-one variant of the search (oracle/receiver.c, ora_set_search_variant) moves the expected stop of at least one (case, prefix) pair,
and that the prefix model answers every pair tests/test_gpu_acquire_stage.py runs."""
import functools

import numpy as np
import pytest

import acquire_cases as ac
import oracle_lib as ol
from acquire_cases import CORR_FAILED, CORR_OK, DIP_END, FRAME_DONE, NO_DIP, NO_END, TF, TN

f32 = np.float32


def test_the_library_constants_parsed():
    assert ac.ACQ_NEED == 20 * ac.TU + 50 + (TF + 1) + (TN + 50 + 21) + 64 == 240410
    assert ac.FRAME_NEED == TF + 2 * ac.TU == 200704


def _recs(fmt):
    """every search event any prefix of family A reaches, with the acquire_stream call that evaluates it"""
    out = []
    for case in ac.family_a(fmt):
        for r in case.records():
            out.append(dict(r, case=case.name, ev=case.trace[r["i"]]))
    return out


def _rel(r, key):
    return r[key] - r["call_base"]


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_block_grid_entries_are_reached(fmt):
    recs = [r for r in _recs(fmt) if r["case"] in ("grid_residues", "grid_special")]
    ends = [r for r in recs if r["kind"] == DIP_END]
    # Begin positions come as edge pairs: the end found at count T_n + 70, the last that is compared, and a dip one sample longer (NO_END).
    # A begin taken a sample early turns the first into a time-out, one taken late the second into a dip end: the begin decides the stop.
    once = lambda rs: list({(r["case"], r["i"]): r for r in rs}.values())      # noqa: E731  (an event is recorded once per way its call went on)
    last_count = once(r for r in ends if r["ev"]["dip_len"] == TN + 70)
    by_one = once(r for r in recs if r["kind"] == NO_END)
    for group in (last_count, by_one):
        assert {_rel(r, "begin") % 16 for r in group} == set(range(16))
        assert set(ac.SPECIAL_POS) <= {_rel(r, "begin") % ac.BLOCK for r in group}
    assert sorted(_rel(r, "begin") % ac.BLOCK for r in last_count) == sorted(_rel(r, "begin") % ac.BLOCK for r in by_one) and len(by_one) == 25
    for name in ("grid_residues", "grid_special"):
        case = next(c for c in ac.family_a(fmt) if c.name == name)
        n_pairs = sum(r["case"] == name for r in by_one)
        inside = lambda tr: tr[tr["pos"] <= case.trace["pos"][[r["i"] for r in by_one if r["case"] == name][-1]] + 1]   # noqa: E731
        # ... by one sample each: with `>= T_n + 70` none of the last-count dips ends, with the end searched a sample late every NO_END does
        tr3, tr4 = (inside(ol.oracle_trace(case.values, case.threshold, 0, variant=v)) for v in (3, 4))
        assert ((tr3["kind"] == DIP_END) & (tr3["dip_len"] >= TN + 69)).sum() == 0 and (tr3["kind"] == NO_END).sum() >= 2 * n_pairs
        assert (tr4["kind"] == NO_END).sum() == 0 and (tr4["dip_len"] == TN + 70).sum() == n_pairs
    # ends: every residue (r + 6 behind a begin at residue r) and the nine block positions
    assert {_rel(r, "end") % 16 for r in ends} == set(range(16))
    assert set(ac.SPECIAL_POS) <= {_rel(r, "end") % ac.BLOCK for r in ends}
    same = [r for r in ends if _rel(r, "begin") // 16 == _rel(r, "end") // 16 and r["end"] > r["begin"]]
    neighbours = [r for r in ends if _rel(r, "end") // 16 == _rel(r, "begin") // 16 + 1]
    blocks = [r for r in ends if _rel(r, "end") // ac.BLOCK != _rel(r, "begin") // ac.BLOCK]
    across = [r for r in ends if _rel(r, "begin") % ac.BLOCK >= ac.BLOCK - 16 and _rel(r, "end") % ac.BLOCK < 16 and r["end"] - r["begin"] < 32]
    assert same and neighbours and len(blocks) >= 16 and across
    # call bases: sample 0 (the seeding call) and the sample after a failed correlation; restarts after NO_END stay in their call
    assert {r["call_base"] for r in recs if r["i"] == 1} == {0} and sum(r["call_base"] > 0 for r in recs) >= 25
    # streams rest at the by-one time-outs themselves and behind every last-count dip
    case = next(c for c in ac.family_a(fmt) if c.name == "grid_residues")
    stops = [int(case.trace["kind"][ac.expected_stop(case.trace, n)["event"]]) for n in case.prefixes]
    assert stops.count(NO_END) == 16 and stops.count(CORR_FAILED) == 16 and stops.count(DIP_END) >= 4


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_attempt_start_and_time_out_entries_are_reached(fmt):
    recs = _recs(fmt)
    tr = {c.name: c.trace for c in ac.family_a(fmt)}
    under_way = [r for r in recs if r["kind"] == DIP_END and r["ev"]["dip_begin"] == 50 and tr[r["case"]]["kind"][r["i"] - 1] == CORR_FAILED]
    assert under_way                                                       # begin at 50, the first position that counts: a dip already under way
    if ("begin at 51 / large sample 49", fmt) not in ac.ENTRY_NOT_APPLICABLE:
        assert [r for r in recs if r["ev"]["dip_begin"] == 51]
        assert [r for r in recs if r["case"] == "attempt_start" and r["ev"]["dip_begin"] in range(99, 102)]   # the large sample 49 leaves the window
    restarts = [r for r in recs if r["attempt_start"] != r["call_base"] and r["call_base"] > 0]
    assert {_rel(r, "attempt_start") % 16 for r in restarts} == set(range(16))          # the `q16 < q` patch, every residue
    assert [r for r in restarts if ac.BLOCK - 50 < _rel(r, "attempt_start") % ac.BLOCK < ac.BLOCK]   # first 50 samples across a block boundary
    # NO_DIP
    t = tr["timeouts"]
    assert (t["kind"][1:17] == NO_DIP).all() and (np.diff(t["pos"][:17]) == TF + 51).all()
    assert t["kind"][17] == DIP_END and t["dip_begin"][17] == TF + 50              # the last comparable position
    assert t["kind"][19] == DIP_END and t["dip_begin"][19] == TF + 50 - 40         # in the segment cut at the time-out (51 samples: the attempt began its call)
    # ... and 300 in front of it in an attempt that restarted 600 samples into a block: the cut segment is 651 samples long.  All three end behind the cut.
    mid = next(r for r in recs if r["case"] == "timeouts" and r["i"] == 22)
    assert t["kind"][21] == NO_END and t["kind"][22] == DIP_END and t["dip_begin"][22] == TF + 50 - 300 and _rel(mid, "attempt_start") % ac.BLOCK == 600
    assert all(t["dip_len"][k] > 700 for k in (17, 19, 22))
    assert t["kind"][24] == NO_DIP and t["kind"][25] == DIP_END and t["dip_begin"][25] == 50   # one sample behind the last position: the next attempt takes it
    # NO_END
    n = tr["no_end"]
    assert n["dip_len"][1] == TN + 69 and n["dip_len"][3] == TN + 70 and n["kind"][5] == NO_END
    assert n["pos"][5] - n["pos"][4] == n["dip_begin"][5] + TN + 71                 # T_n + 71 is read, never compared
    runs = [r for r in recs if r["kind"] == NO_END and r["ev"]["dip_begin"] == 50]
    assert len(runs) >= 19                                                 # silence: NO_END after NO_END, each attempt restarting inside it
    # pass ends: by the pass's budget of one frame, by the ring running out, and neither (the same call tries again)
    assert {"budget", "space", "same call"} <= {r["then"] for r in recs}
    assert sum(r["then"] == "budget" for r in recs if r["case"] == "timeouts") >= 16


def _moving_sum(values, start, stop):
    """timesyncer.cpp:49-66 in float32 from the attempt that starts at sample `start`: the level before sample `stop`"""
    env = np.sqrt((values.real[start:stop].astype(f32)) ** 2 + (values.imag[start:stop].astype(f32)) ** 2).astype(f32)
    level = f32(0)
    for i in range(len(env)):
        level = f32(level + env[i]) if i < 50 else f32(level + f32(env[i] - env[i - 50]))
    return level


@pytest.mark.parametrize("fmt", ["cf32", "s16"])
def test_exact_zero_entries_are_reached(fmt):
    case = next(c for c in ac.family_a(fmt) if c.name == "zeros")
    mag = np.abs(case.values)
    z = np.flatnonzero(mag == 0)
    starts = z[np.r_[True, np.diff(z) > 1]]
    ends = z[np.r_[np.diff(z) > 1, True]]
    assert len(starts) == 3 and (ends - starts > 2 * (TN + 121)).all()
    recs = sorted(case.records(), key=lambda r: r["i"])
    first = [next(r for r in recs if r["begin"] is not None and s <= r["begin"] <= s + 60) for s in starts]
    # entered at level zero: the moving sum of exact magnitudes cancels exactly, so the zeros behind it are `0 + 0` (level_sum_block's shortcut) ...
    assert _moving_sum(case.values, first[0]["attempt_start"], int(starts[0]) + 60) == 0
    # ... and after one sample of 1e5 among samples of 1 it does not (float cancellation leaves a residue): the walk must run
    assert abs(mag[starts[1] - 10] / (ac.FMT_MAX[fmt] * ac.FMT_SCALE[fmt]) - 1) < 1e-3 and mag[starts[1] - 11] < 0.1 * mag[starts[1] - 10]
    residue = _moving_sum(case.values, first[1]["attempt_start"], int(starts[1]) + 60)
    assert (residue != 0) == (("residue behind a sample of 1e5", fmt) not in ac.ENTRY_NOT_APPLICABLE)
    # attempts restarting inside zeros, and zeros that end mid-group
    inside = [r for r in recs if r["kind"] == NO_END and case.trace["dip_begin"][r["i"]] == 50 and mag[r["attempt_start"]:r["attempt_start"] + 50].max() == 0]
    assert len(inside) >= 6
    last = next(r for r in recs if r["kind"] == DIP_END and r["end"] > ends[2])
    assert (int(ends[2]) - last["call_base"]) % 16 == 6 and int(ends[2]) == case.note["last_zero"]


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_level_swing_entries_are_reached(fmt):
    case = next(c for c in ac.family_a(fmt) if c.name == "swings")
    mag = np.abs(case.values).astype(np.float64)
    step = mag[1:] / np.maximum(mag[:-1], 1e-30)
    depth = 80.0 if ("60 dB step", fmt) in ac.ENTRY_NOT_APPLICABLE else 999.0
    assert step.max() >= depth and step.min() <= 1 / depth
    if ("20 margin events", fmt) not in ac.ENTRY_NOT_APPLICABLE:
        m = case.trace["margin"]
        assert m[-1] >= 20
        k = int(np.flatnonzero(case.trace["kind"] == DIP_END)[-1])
        assert m[k] - m[k - 1] >= 20 and case.trace["dip_len"][k] > 300      # both crossings in one attempt: begin and end comparisons counted
        assert {ac.expected_stop(case.trace, n)["margin"] for n in case.prefixes} >= {0, int(m[k])}


def test_the_tie_is_a_tie():
    case = next(c for c in ac.family_a("cf32") if c.name == "equality")
    ev, tie_at = case.trace[1], case.note["tie_at"]
    assert ev["kind"] == DIP_END and 20 * ac.TU + ev["dip_begin"] == tie_at
    # the comparison made before sample tie_at is read, recomputed: the moving sum of the attempt (it starts behind the seed) over 50, and 0.55 sLevel
    mean = f32(_moving_sum(case.values, 20 * ac.TU, tie_at) / f32(50))
    level = f32(ol.oracle().ora_level_walk(np.ascontiguousarray(case.values[:tie_at]), tie_at, f32(0.1)))
    assert mean == f32(f32(0.55) * level) and mean > 0
    before = f32(_moving_sum(case.values, 20 * ac.TU, tie_at - 1) / f32(50))
    assert before > f32(f32(0.55) * f32(ol.oracle().ora_level_walk(np.ascontiguousarray(case.values[:tie_at - 1]), tie_at - 1, f32(0.1))))


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_family_a_correlations_fail_far_below_the_threshold(fmt):
    n = 0
    for case in ac.family_a(fmt):
        tr = case.trace
        assert not (tr["kind"] == CORR_OK).any() and not (tr["kind"] == FRAME_DONE).any()
        r = tr["ratio"][tr["kind"] == CORR_FAILED]
        assert np.isfinite(r).all() and (r < 1.0e9).all() and (r < 10).all()
        n += len(r)
    assert n >= 40


def test_family_c_meets_its_margins():
    for case in ac.family_c():
        tr = case.trace
        ok, failed = [], []
        for k in range(len(tr)):
            if tr["kind"][k] in (CORR_OK, CORR_FAILED):
                thr = case.threshold * (2 if tr["kind"][k - 1] == FRAME_DONE else 1)         # doubled in lock
                (ok if tr["kind"][k] == CORR_OK else failed).append(tr["ratio"][k] / thr)
        assert len(ok) >= 12 and min(ok) >= 2.0, (case.name, min(ok))
        assert len(failed) >= 7 and max(failed) <= 0.5, (case.name, max(failed))
        # six frames in lock, the crafted stretch (every kind of search event in it), frames again
        p6, n_end = case.note["p6"], case.note["n_end"]
        assert (tr["kind"][tr["pos"] <= p6] == FRAME_DONE).sum() == 6
        inside = tr[(tr["pos"] > p6) & (tr["pos"] <= n_end)]
        assert {NO_DIP, NO_END, DIP_END, CORR_FAILED} <= set(inside["kind"].tolist())
        assert (tr["kind"][tr["pos"] > n_end] == FRAME_DONE).sum() >= 6
        recs = [r for r in case.records() if r["kind"] == DIP_END and p6 < r["end"] <= n_end]
        got = [((r["begin"] - r["call_base"]) % ac.BLOCK, (r["end"] - r["call_base"]) % ac.BLOCK) for r in sorted(recs, key=lambda r: r["i"])]
        assert got[:len(case.note["want"])] == case.note["want"]
        stops = [ac.expected_stop(tr, n) for n in case.prefixes]
        assert len(stops) == ac.EXPECTED_C_STREAMS
        assert (sum(s["event"] + 1 for s in stops), sum(s["frames"] for s in stops)) == ac.EXPECTED_C_EVENTS
        assert {ac.ST_WAIT_SYNC, ac.ST_EVAL_SYNC} == {s["state"] for s in stops}


def test_family_b_reaches_its_edges():
    inside, outside, clock = ac.family_b()
    corr = lambda c: c.trace["ratio"][c.trace["kind"] == FRAME_DONE]          # noqa: E731  (what the coarse search returned, frame by frame)
    # 34 900 Hz: f_sync stays
    assert inside.ora["n"] >= 12 and abs(corr(inside)[0] - 34900) < 500 and (np.abs(inside.ora["fbb_end"] - 34900) < 100).all()
    assert not (inside.trace["kind"] == CORR_FAILED).any()
    # 35 400 Hz: |f_sync| > 35 000 resets it to 0, frame after frame -- and every second frame's coarse search returns not-found
    c = corr(outside)
    assert outside.ora["n"] >= 8 and (np.abs(outside.ora["fbb_end"]) < 200).all()
    assert (c[0::2] > 35000).all() and (c[1::2] == 100000).all() and len(c) >= 8
    assert (outside.trace["kind"] == CORR_FAILED).sum() >= 7
    # a null symbol 40 samples short before frame 8, one 40 samples long before frame 14: the estimate is beyond +-307.2 and is clamped,
    # in frames whose coarse search did not correct anything
    ce, c = clock.ora["clock_err"], corr(clock)
    assert (c[5:] == 0).all()
    assert ce[7] == 0 and ce[8] == f32(f32(0.1) * f32(-307.2)) and ce[14] == f32(ce[13] + f32(0.1) * f32(f32(307.2) - ce[13]))
    assert clock.ora["start"][8] == clock.ora["start"][7] - 40 and clock.ora["start"][14] == clock.ora["start"][13] + 40


def _stops(case, trace):
    out = []
    for n in case.prefixes:
        try:
            s = ac.expected_stop(trace, n)
            out.append((s["samples_consumed"], s["margin"]))
        except AssertionError:
            out.append(None)                                       # the variant never comes to rest inside the signal
    return out


# which case tells each variant from the restatement (at least): the catalogue entry built for it
CAUGHT_BY = {1: "attempt_start", 2: "timeouts", 3: "no_end", 4: "no_end", 5: "equality", 6: "timeouts", 7: "lock_cfo_911"}


@functools.lru_cache(maxsize=None)
def _moved():
    """{variant: names of the cases in which it moves the expected stop (position or margin count) of at least one prefix}"""
    out = {}
    for variant in sorted(ol.SEARCH_VARIANTS):
        out[variant] = []
        for case in list(ac.family_a("cf32")) + list(ac.family_c()):
            if (variant == 7) != (case.subch is not None):
                continue                                           # (no lock in family A: the oscillator's phase stays 0; family C is there for variant 7)
            tr = ol.oracle_trace(case.values, case.threshold, case.strongest, variant=variant)
            want, got = _stops(case, case.trace), _stops(case, tr)
            assert None not in want
            if want != got:
                out[variant].append(case.name)
    return out


@pytest.mark.parametrize("variant", sorted(ol.SEARCH_VARIANTS))
def test_every_variant_moves_an_expected_stop(variant):
    assert CAUGHT_BY[variant] in _moved()[variant], (variant, ol.SEARCH_VARIANTS[variant], _moved()[variant])


def test_every_case_is_moved_by_a_rule_variant():
    """Variant 6 (the level not restarted) moves nearly everything and so says little about any one case.  Every case of family A must be
    moved by one of the rule variants 1 .. 5 as well: the grids by the time-out variants 3 and 4 (their begins sit on both sides of the NO_END
    edge), `equality` by 5 alone."""
    moved = _moved()
    for case in ac.family_a("cf32"):
        by = [v for v in (1, 2, 3, 4, 5) if case.name in moved[v]]
        assert by, case.name
        if case.name.startswith("grid"):
            assert {3, 4} <= set(by)
    assert moved[5] == ["equality"] and moved[7]


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_the_prefix_model_answers_every_pair(fmt):
    cases = ac.family_a(fmt)
    for g, names in enumerate(ac.GROUPS):
        pairs = [(c, n) for c in cases if c.name in names for n in c.prefixes]
        assert len(pairs) == ac.EXPECTED_STREAMS[fmt][g] and 16 <= len(pairs) <= 48
        assert sum(ac.expected_stop(c.trace, n)["event"] + 1 for c, n in pairs) == ac.EXPECTED_EVENTS[fmt][g]
    for (name, f), why in ac.NOT_APPLICABLE.items():
        assert why and (f != fmt or name not in [c.name for c in cases])
    for case in list(cases) + (list(ac.family_b()) + list(ac.family_c()) if fmt == "cf32" else []):
        tr, n_all = case.trace, len(case.values)
        assert len(set(case.prefixes)) == len(case.prefixes) and max(case.prefixes) <= n_all
        # N = len(x): the stream rests at the last event the oracle reached, minus what the need rule withholds
        k, _ = ac.simulate(tr, n_all)
        assert k is not None and all(ac.need_of(int(tr["kind"][j])) is None or n_all - int(tr["pos"][j]) < ac.need_of(int(tr["kind"][j]))
                                     for j in range(k, len(tr)))
        # the trace is causal: the oracle on a prefix alone reaches the same events up to the stop
        n = case.prefixes[len(case.prefixes) // 2]
        stop = ac.expected_stop(tr, n)
        part = ol.oracle_trace(case.values[:n], case.threshold, case.strongest)
        assert stop["event"] < len(part) and part[:stop["event"] + 1].tobytes() == tr[:stop["event"] + 1].tobytes()
        # every pinned event is a different one, and a pin rests at its event or at an earlier one that needs more
        stops = [ac.expected_stop(tr, m)["event"] for m in case.prefixes]
        assert stops == sorted(stops)
    if fmt == "cf32":
        # the start: fewer than ACQ_NEED samples and nothing is read
        s = ac.expected_stop(cases[0].trace, ac.ACQ_NEED - 1)
        assert (s["event"], s["samples_consumed"], s["state"]) == (-1, 0, ac.ST_INIT)
