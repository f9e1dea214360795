"""tests/demap_cases.py without a device: every class reaches the branch it is named for (counted on the oracle), the part of the soft bits
the rule leaves out stays under its cap, and the two figures the rule rests on -- the spread between the IEEE oracle and the build with the
reference's float flags, and the list of (case, generator) pairs those two builds disagree on -- are as demap_cases.py records them."""
import functools

import numpy as np
import pytest

import demap_cases as dc


def _frames(gen):
    """{case name: oracle record} over all streams."""
    return {r["name"]: r for s in range(dc.N_STREAMS) for r in dc.oracle_stream(s, gen)}


def test_plan_has_the_shape_the_doc_states():
    names = [f["name"] for p in dc.PLAN for f in p["frames"]]
    assert len(names) == len(set(names)) == 3 * 5 + 7 + 10 + 6
    assert [len(p["frames"]) for p in dc.PLAN] == [5, 5, 7, 5, 10, 6]
    assert sum(1 for p in dc.PLAN for f in p["frames"] if not f["present"]) == 1
    assert {f["ce"] for p in dc.PLAN for f in p["frames"]} == {0.0, 12.5, -12.5, 400.0, -400.0}
    assert {f["np_sel"] for f in dc.PLAN[3]["frames"]} == {0, 1}
    fr = dc.stream_frames(1)[0]                                      # on_axes: the first symbol sits on the axes, with both signs of zero
    used = dc._tables()[1]
    x = fr["spec"][1, used]
    assert (x.real == 0).sum() > 300 and (x.imag == 0).sum() > 300
    assert np.signbit(x.real[x.real == 0]).any() and not np.signbit(x.real[x.real == 0]).all()
    z = dc.stream_frames(0)[3]["spec"]
    assert z[dc.ZERO_SYMBOL, used[dc.ZERO_CARRIER]] == 0 and (z[:, used] == 0).sum() == 1
    z = dc.stream_frames(1)[3]["spec"]
    assert z[0, used[dc.ZERO_CARRIER]] == 0 and (z[:, used] == 0).sum() == 1


@pytest.mark.parametrize("gen", dc.GENERATORS)
def test_every_class_reaches_its_branch(gen):
    fr = _frames(gen)
    ax = {n: np.abs(r["prod"].astype(np.float64)) for n, r in fr.items()}

    def band(n, lo, hi):
        with np.errstate(invalid="ignore"):
            return int(((ax[n] >= lo) & (ax[n] < hi)).sum())
    # natural / noise_free: no overflow at all once the stream has settled (the first frames of generator 2 overflow in ordinary operation)
    assert band("clock_err_+12.5", 32768.0, np.inf) == 0 or gen == 2
    if gen == 2:
        assert band("natural", 32768.0, np.inf) > 0
    # dropout: the int16 wrap band and [2^22, 2^31) (generators 2 and 3: far past int16)
    assert band("dropout", 2.0 ** 15, 2.0 ** 22) > 100
    if gen != 1:
        assert band("dropout", 2.0 ** 22, dc.TWO31) > 1000
    # ... and `soft + 127` wraps where the saturating conversion gives 255: soft bits in [32641, 32767], counted where the integer layer
    # observes them -- in the FIC symbols and in sub-channel bits whose logical frame comes out (the two `wrap` pairs are there for this)
    n_fic = n_msc = 0
    for s in range(dc.N_STREAMS):
        recs = dc.oracle_stream(s, gen)
        fic, msc = dc.decoded_mask(len(recs))
        w = np.stack([r["soft"] for r in recs]) >= 32641
        n_fic, n_msc = n_fic + int((w & fic).sum()), n_msc + int((w & msc).sum())
    assert n_fic >= 4 and n_msc >= 8, (gen, n_fic, n_msc)
    # gain 1e5 sends generator 3 over 2^31
    if gen == 3:
        assert band("gain_1e5", dc.TWO31, np.inf) > 1000
        x = fr["int_indefinite"]["prod"].astype(np.float64)
        ks = np.concatenate([np.arange(64) * 24 + j for j in range(3)])
        rows = [l - 1 for l in dc.INT_INDEFINITE_SYMBOLS]
        big = np.abs(x) >= dc.TWO31
        assert (x[big] > 0).sum() >= 20 and (x[big] < 0).sum() >= 20
        known = np.zeros_like(big)
        for j, l in enumerate(rows):
            k = np.arange(64) * 24 + j
            known[l, k] = known[l, dc.K + k] = True
        assert not (big & ~known).any()                              # on the known set only ...
        sub = np.abs(x[known])
        assert (sub < dc.TWO31).sum() >= 20                          # ... which the products cross: some below, some above
        assert len(ks) == 192
    # null_above_signal: signal_power <= 0 on a third of the carriers, and nowhere in a natural frame
    assert fr["null_above_signal"]["sp_le0"] >= 75 * 500 and fr["clock_err_+12.5"]["sp_le0"] == 0
    # both integrator stops hold at the end of the integrator stream, none in its first frame
    assert fr["integrator_stops_9"]["stop_hi"] >= 700 and fr["integrator_stops_9"]["stop_lo"] >= 700
    assert fr["integrator_stops_0"]["stop_hi"] == 0 and fr["integrator_stops_0"]["stop_lo"] == 0
    # a zero carrier / a zero reference: mMeanValue becomes NaN and stays NaN, the rest of the frame's soft bits are 0
    for n, first in (("zero_carrier", dc.ZERO_SYMBOL), ("zero_reference", 1)):
        r = fr[n]
        assert r["nan_mean"] >= 75 - first - 1, (n, r["nan_mean"])
        assert not r["soft"][first + 2:].any() and np.isnan(r["prod"][first + 2:]).all(), n
        d = fr[n + "_next"]                                      # ... and so are all of the next frame's
        assert d["nan_mean"] == 75 and not d["soft"].any() and np.isnan(d["prod"]).all(), n


def test_decoded_mask_is_what_the_oracle_back_end_reads():
    """The MSC half of decoded_mask, proven on oracle/msc.c: other soft bits everywhere outside the mask leave every logical frame as it is,
    and other soft bits inside it -- in one CIF at a time -- change some frame; likewise for the FIC half and oracle/fic.c."""
    n = 5
    soft = np.stack([r["soft"] for r in dc.oracle_stream(0, 1)[:n]])
    fic, msc = dc.decoded_mask(n)
    assert msc.sum() == sum(sc.cu_size for sc in dc.SUBCH) * 64 * (4 * n - 16) and not (fic & msc).any()
    rng = np.random.default_rng(3)
    other = rng.integers(-300, 301, soft.shape).astype(np.int16)
    base_msc, base_fic = dc.msc_of(soft, 0), dc.fic_of(soft, 0)

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    outside = np.where(fic | msc, soft, other)
    assert same(dc.msc_of(outside, 0), base_msc)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(dc.fic_of(outside, 0), base_fic))
    for f in range(n):                                               # every frame's share of the mask is read
        inside = soft.copy()
        inside[f][msc[f]] = other[f][msc[f]]
        assert not same(dc.msc_of(inside, 0), base_msc), f
    # the mirror image (t + delay), which selects as many bits, is not it
    i = np.arange(55296)
    wrong = np.zeros((4 * n, 55296), bool)
    in_sc = msc[:, 3:].reshape(4 * n, 55296).any(axis=0)
    for t in range(4 * n):
        out = t + dc.ds.INTERLEAVE_MAP[i & 15]
        wrong[t] = in_sc & (out >= 16) & (out < 4 * n)
    wrong3 = np.zeros_like(msc)
    wrong3[:, 3:] = wrong.reshape(n, 72, dc.K2)
    assert wrong3.sum() == msc.sum()
    assert not same(dc.msc_of(np.where(fic | wrong3, soft, other), 0), base_msc)


@pytest.mark.parametrize("gen", dc.GENERATORS)
def test_what_the_rule_leaves_out_stays_under_the_cap(gen):
    worst = ("", 0.0)
    for n, r in _frames(gen).items():
        _, left, _ = dc.classify(r["prod"])
        frac = float(left.mean())
        worst = max(worst, (n, frac), key=lambda t: t[1])
        assert frac <= dc.LEFT_OUT_CAP, (n, gen, frac)
    print("generator %d: most left out: %s %.4f" % (gen, *worst))


@functools.lru_cache(maxsize=None)
def _two_builds():
    """Per (case, generator): (spread over finite products with |x| > 1, the rule's verdict on the fast build's soft bits)."""
    out = {}
    for gen in dc.GENERATORS:
        for s in range(dc.N_STREAMS):
            for a, b in zip(dc.oracle_stream(s, gen), dc.run_oracle(s, gen, fast=True)):
                x, y = a["prod"].astype(np.float64), b["prod"].astype(np.float64)
                with np.errstate(invalid="ignore"):
                    m = np.isfinite(x) & np.isfinite(y) & (np.abs(x) > 1)
                spread = float((np.abs(y[m] - x[m]) / np.abs(x[m])).max()) if m.any() else 0.0
                same_class = bool((np.isfinite(x) == np.isfinite(y)).all())
                out[(a["name"], gen)] = (spread, dc.compare(b["soft"], a["soft"], a["prod"]), same_class)
    return out


def test_spread_and_undefined_list_are_as_recorded():
    res = _two_builds()
    disagree = {k for k, (_, c, _) in res.items() if not (c["n_zero_bad"] == 0 and c["n_hard_bad"] == 0 and c["frac_soft_bad"] <= 1e-3)}
    spread = {k: v[0] for k, v in res.items() if k not in disagree}
    top = sorted(spread.items(), key=lambda t: -t[1])[:4]
    print("largest spreads:", top)
    print("disagree:", sorted(disagree), {k: {q: res[k][1][q] for q in ("n_zero_bad", "n_hard_bad", "frac_soft_bad", "worst")} for k in disagree})
    assert disagree == set(dc.UNDEFINED)
    assert all(n in ("zero_carrier", "zero_carrier_next", "zero_reference", "zero_reference_next") for n, _ in dc.UNDEFINED)   # the two classes' frames
    assert max(spread.values()) <= dc.SPREAD_MEASURED
    assert dc.REL == 4 * dc.SPREAD_MEASURED
