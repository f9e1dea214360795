"""No device: the cases of tests/dciq_cases.py are what they are named for, the two float64 references agree, the float32 restatement
of k_dciq's tile algorithm stays where the stored bounds say, and each named mutation of it breaks those bounds.  `pytest -s` prints the
tables of docs/history/dciq_tests.md."""
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import dciq_cases as dc

WORKERS = min(8, os.cpu_count() or 1)
_CASES = dc.all_cases()


def _measure(i):
    """one case: its figures and the ratio every mutation reaches (the long wrap cases: only the mutations a wrap can show)"""
    group, make = _CASES[i]
    c = dc.finish(make())
    muts = dc.MUTATIONS if group != "wrap" else ("inclusive", "clamp")
    reach, finite = {}, {}          # (inf: a NaN or a non-zero where f64 has none)
    for m in muts:
        r = dc.ratios(c, *dc.restate(c["data"], c["groups"], c["mode"], mutation=m))
        every = np.concatenate([np.r_[o, st] for o, st in r])
        reach[m] = float(every.max())
        finite[m] = float(every[np.isfinite(every)].max())
    fig = {"name": c["name"], "group": group, "mode": c["mode"], "A": c["A"],
           "dist_out": max(d["out"] for d in c["dist"]) / c["A"], "dist_st": np.max([d["st"] for d in c["dist"]], axis=0),
           "noise_out": max(d["out"] for d in c["ref_noise"]) / c["A"], "noise_st": np.max([d["st"] for d in c["ref_noise"]], axis=0),
           "bound_out": max(b["out"] for b in c["bound"]) / c["A"], "bound_st": np.max([b["st"] for b in c["bound"]], axis=0)}
    fig["finite"] = finite
    return fig, reach


@pytest.fixture(scope="module")
def measured():
    with ProcessPoolExecutor(max_workers=WORKERS) as pool:
        return list(pool.map(_measure, range(len(_CASES))))


def test_closed_form_equals_the_oracles_f64_run():
    """y_n = (1 - a)^n y_0 + a (1 - a)^n cumsum(x_k / (1 - a)^k), level by level, against the sample-by-sample double recurrence"""
    worst = 0.0
    for make in (lambda: dc.partition_case(1), lambda: dc.partition_case(2), lambda: dc.family_case(0, 3e-4, 2), lambda: dc.family_case(1, 60.0, 2),
                 lambda: dc.family_case(2, 0.26, 2), lambda: dc.family_case(1, 0.26, 1), lambda: dc.wrap_case("b", 2)):
        c = make()
        for s in range(dc.S):
            n = len(c["data"][s])
            out, st = dc.run_reference(c["data"][s], [n], c["mode"], "f64")
            cf, cst = dc.closed_form(c["data"][s], c["mode"])
            # the oracle rounds its outputs to float once: half an ulp of the value, and nothing else to speak of
            err = np.maximum(np.abs(out.real - cf.real) - 2.0 ** -24 * np.abs(cf.real), np.abs(out.imag - cf.imag) - 2.0 ** -24 * np.abs(cf.imag))
            assert err.max() <= 1e-9 * c["A"], (c["name"], s, err.max())
            for j in range(5):
                scale = max(abs(st[0, j]), c["A"] ** (1 if j < 2 else 2))
                worst = max(worst, abs(cst[j] - st[0, j]) / scale)
                assert abs(cst[j] - st[0, j]) <= 1e-9 * scale, (c["name"], s, dc.STATE_NAMES[j], cst[j], st[0, j])
    print("\nclosed form against the oracle's f64 states: at most %.2g of the state's scale" % worst)


def test_restatement_stays_within_what_the_bounds_are_made_of(measured):
    """Where the stored bounds come from: the restatement's distance from f64 on every case (the reference's own float recurrence beside
    it, for the record: it is no bound).  The distance is finite everywhere -- NaN and exact zeros where f64 has them -- and small."""
    print("\n%-24s %9s %9s %9s   %s" % ("case", "ref noise", "restated", "bound", "states: restated (bound), relative, worst of the five"))
    for fig, _ in measured:
        j = int(np.argmax(fig["dist_st"]))
        print("%-24s %9.2e %9.2e %9.2e   %s %.2e (%.2e); ref noise %.2e" % (fig["name"], fig["noise_out"], fig["dist_out"], fig["bound_out"],
                                                                            dc.STATE_NAMES[j], fig["dist_st"][j], fig["bound_st"][j], fig["noise_st"].max()))
        assert np.isfinite(fig["dist_out"]) and np.isfinite(fig["dist_st"]).all(), fig
        # a correct scan: outputs within a few roundings of the output (mode 1) or of the gain and phase estimates (mode 2)
        assert fig["dist_out"] <= (2.0 ** -22 if fig["mode"] == 1 else 2.0 ** -18), fig
        assert fig["bound_out"] >= dc.FLOOR and (fig["bound_st"] >= dc.FLOOR).all()
    # the reference's float recurrence is no yardstick for the scan: far off on long runs, closer than the scan on short ones
    long_run = [f for f, _ in measured if f["group"] == "wrap"]
    assert all(f["noise_st"].max() > 10 * f["dist_st"][:2].max() for f in long_run)


def test_every_mutation_breaks_the_bounds_in_each_mode_and_every_case_separates(measured):
    print("\nlargest distance / bound of each mutated restatement, per mode (case that shows it)")
    for m in dc.MUTATIONS:
        print("  %s: %s" % (m, dc.MUTATION_TEXT[m]))
        for mode in (1, 2):
            best = max(((reach[m], fig["name"]) for fig, reach in measured if fig["mode"] == mode and m in reach), key=lambda t: t[0])
            n_cases = sum(1 for fig, reach in measured if fig["mode"] == mode and reach.get(m, 0) >= 4.0)
            fin = max(((fig["finite"][m], fig["name"]) for fig, reach in measured if fig["mode"] == mode and m in reach), key=lambda t: t[0])
            print("  %-12s mode %d: %9.3g x (%s)%s; %d cases at 4 x or more" % (m, mode, fin[0], fin[1], ", inf in " + best[1] if np.isinf(best[0]) else "", n_cases))
            assert best[0] >= 4.0, (m, mode, best)
    for fig, reach in measured:
        assert max(reach.values()) >= 4.0, (fig["name"], reach)


def test_partition_cover():
    for mode in (1, 2):
        c = dc.partition_case(mode)
        cov = dc.cover_of(c["groups"])
        for s in range(dc.S):
            lens = [to - frm for frm, to in dc.launch_ranges(c["groups"], s)]
            assert set(dc.LENGTHS) <= set(lens), (s, sorted(set(dc.LENGTHS) - set(lens)))
        orders = [tuple(to - frm for frm, to in dc.launch_ranges(c["groups"], s))[:10] for s in range(dc.S)]
        assert len(set(orders)) == dc.S
        assert cov["partial_n"] == set(range(1, 16)), cov["partial_n"]
        assert cov["wave_boundary_ends"] >= 1
        idle_some = sum(1 for g in c["groups"] if 0 in g)
        assert idle_some > len(c["groups"]) // 2
        assert (0, 0, 1) in cov["busy_patterns"] and (1, 0, 0) in cov["busy_patterns"] and (0, 1, 0) in cov["busy_patterns"]
        assert max(len(d) for d in c["data"]) <= 450000
    print("\npartition: lengths %s; n of the partly filled thread %s; %d launches end on a wave boundary; busy patterns %s"
          % (sorted(cov["lengths"]), sorted(cov["partial_n"]), cov["wave_boundary_ends"], sorted(cov["busy_patterns"])))
    e = dc.cover_of(dc.entry_case(1)["groups"])
    assert (1, 1, 1) in e["busy_patterns"] and any(sum(p) == 2 for p in e["busy_patterns"])
    for mode in (1, 2):
        for g in range(len(dc.FAMILY_GROUPS)):
            c = dc.family_case(g, 0.26, mode)
            for s in range(dc.S):
                hit = [(frm, to) for frm, to in dc.launch_ranges(c["groups"], s) if frm <= c["step_at"][s] < to]
                d = c["step_at"][s] - hit[0][0]
                assert (d % dc.TILE) // dc.PER == 128 and d % dc.PER == 8 and d // dc.TILE == 1      # mid-tile, mid-thread, not the first tile


def test_wrap_cover():
    seen = {}
    for which in ("a", "b"):
        c = dc.wrap_case(which, 1)
        for s, (name, before, length) in enumerate(c["wraps"]):
            ranges = dc.launch_ranges(c["groups"], s)
            crossing = [(frm, to) for frm, to in ranges if frm <= dc.RING < to]
            assert crossing == [(before, before + length)] and ranges[-1][0] == before + length, (name, crossing)
            seen[name] = dc.wrap_place(before, length)
            assert len(c["data"][s]) <= 450000
    print("\nwrap: (tile, thread, offset in the thread, samples in that tile) %s" % seen)
    assert seen["at_from"][:3] == (0, 0, 0)
    assert seen["thread_boundary"][2] == 0 and seen["thread_boundary"][1] > 0
    assert seen["thread_offset_1"][2] == 1 and seen["thread_offset_15"][2] == 15
    assert seen["last_partial_tile"][0] == 1 and seen["last_partial_tile"][3] < dc.TILE
    assert seen["short_launch"][3] == 17


@pytest.mark.parametrize("mode", [1, 2])
def test_one_nan_in_the_serial_reference(mode):
    """What the GPU file expects of the NaN case is what the serial recurrence does, in float and in double: nothing before the sample
    changes, from it on every output and every state the sample reaches is NaN, and stays so over the next launch."""
    c, clean = dc.finish(dc.isolation_case(mode)), dc.finish(dc.isolation_case(mode, with_nan=False))
    k = c["nan_at"]
    ranges = dc.launch_ranges(c["groups"], 1)
    hit = [i for i, (frm, to) in enumerate(ranges) if frm <= k < to][0]
    d = k - ranges[hit][0]
    assert d % dc.PER not in (0, 15) and (d % dc.TILE) // dc.PER >= 64 and hit + 1 < len(ranges)          # inside a thread, not in the first wave
    for which in ("f64", "f32"):
        out, st = c[which][1]
        ref, _ = clean[which][1]
        assert np.array_equal(out[:k].view(np.uint32), ref[:k].view(np.uint32))
        assert np.isnan(out[k:].real).all() and np.isnan(out[k:].imag).all()
        touched = [0, 1] if mode == 1 else [0, 1, 2, 3, 4]
        groups_of_1 = [g for g, grp in enumerate(c["groups"]) if grp[1]]
        for g in range(len(c["groups"])):
            after = g >= groups_of_1[hit]
            assert np.isnan(st[g, touched]).all() == after == bool(np.isnan(st[g, touched]).any()) and np.isfinite(st[g, [j for j in range(5) if j not in touched]]).all(), (which, g)
        assert sum(1 for g in groups_of_1 if g > groups_of_1[hit]) >= 1
        for s in (0, 2):
            assert np.array_equal(c[which][s][0].view(np.uint32), clean[which][s][0].view(np.uint32))
    # the restatement does the same (its distance is finite only if NaN stands exactly where f64 has it)
    assert all(np.isfinite(d["out"]) and np.isfinite(d["st"]).all() for d in c["dist"])
