"""Inputs for the two decisions in front of the frame chain -- the PRS correlator (prs_correlate_block, csrc/ofdm_core.h) and the coarse
CFO search (coarse_cfo_block) -- and float64 models of both (phasereference.cpp:126-212 and :223-280) that also report which branches a
case takes and how close every comparison came to going the other way.

The device transforms in float (tests/test_gpu_stages.py::test_fft_matches_oracle_dft: 2e-6 max|X| per transform); the correlator has two
transforms with a unit-modulus product in between, 4e-6 max(pk) in all.  A correlator case whose every evaluated comparison is at least
MIN_MARGIN = 2e-5 max(pk) wide (five times that) must give the same start index on the device as in the oracle: the margin is a condition
on the INPUTS (tests/test_sync_cases.py proves it on the CPU), not a tolerance on the kernel.  The coarse search ends in a truncation
to integer Hz; its cases carry the distance of offset * 1000 from an integer, and the tests demand equality where that distance is large
enough (COARSE_D, measured on the CPU) and +-1 Hz elsewhere."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

TU, TG = 2048, 504
I0, I1, GAP = TG - 250, TG + 500, 10            # phasereference.cpp:136-139
MIN_MARGIN = 2e-5
THRESHOLDS = (3.0, 6.0, 12.0)                   # the two defaults in use and the engine's doubled in-lock value of the second
IDX_NOT_FOUND = 100000
INT_MIN = -2 ** 31
SQRT_FLT_MAX = float(np.sqrt(np.float64(np.finfo(np.float32).max)))   # |z| beyond this: re^2 + im^2 is inf in float
FLT_MIN = float(np.finfo(np.float32).tiny)
# offset * 1000 is truncated to integer Hz.  The function's own floats put a floor under how near an integer it may come before the integer
# is no longer decided: offset = index + r is rounded to float (half an ulp of 70: 3.8e-6 carriers = 3.8e-3 Hz) and so is the product with
# 1000 (half an ulp of 70 000: 3.9e-3 Hz) -- 8e-3 Hz in all.  tests/test_sync_cases.py measures the smallest D at which the oracle equals
# trunc(model) on every case at least D from an integer and asserts that it is no larger than this; the device is held to the oracle's
# integer from 4 D on (its transforms are float: r moves by up to 4 * 2e-6 twice, 1.6e-2 Hz) and to +-1 Hz below.
COARSE_D = 8e-3
COARSE_DECISION_MARGIN = 1e-4                   # of the maximum: first maximum against the runner-up, mx against 5 avg

PRS = ds.prs_spectrum()                                    # bin order, unit modulus on the 1536 carriers
P_TIME = np.fft.ifft(PRS) * TU / np.sqrt(1536.0)           # the phase reference symbol in time, unit power


# ------------------------------------------------------------------------------------------------ correlator
def model_correlate(x, thr):
    """-> (first-peak index, strongest-peak index, branches taken, smallest margin / max(pk), max(pk) / mean, float-range report)"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    z = np.fft.ifft(np.fft.fft(x) * np.conj(PRS)) * TU
    pk = np.abs(z)
    rng_rep = _float_range(pk)
    if rng_rep["overflow"]:
        # some |z|^2 is inf in float: the mean is inf, every quotient 0 or NaN, nothing clears the threshold
        return -1, -1, {"overflow"}, np.inf, np.nan, rng_rep
    mean = pk.sum() / TU
    if mean == 0:
        return -1, -1, {"zero_sum"}, np.inf, np.nan, rng_rep
    top, margin, taken = pk.max(), np.inf, set()
    first, max_index, max_l = -1, -1, -1000.0
    i = I0
    while i < I1:
        margin = min(margin, abs(pk[i] - thr * mean) / top)
        if pk[i] / mean > thr:
            found = True
            for j in range(1, GAP):
                if i + j >= I1:
                    taken.add("lookahead_cut_at_the_end")
                    break
                margin = min(margin, abs(pk[i + j] - pk[i]) / top)
                if pk[i + j] > pk[i]:
                    found = False
                    taken.add("lookahead_rejects_at_%d" % j)
                    break
            if found:
                taken.add("pass_%d" % ((i - I0) // 256))
                if first < 0:
                    first = i
                else:
                    taken.add("second_peak")
                margin = min(margin, abs(pk[i] - max_l) / top)
                if pk[i] > max_l:
                    if max_index >= 0:
                        taken.add("later_peak_is_larger")
                    max_l, max_index = pk[i], i
                elif max_index >= 0:
                    taken.add("later_peak_is_not_larger")
                if i + GAP + 1 < I1 and pk[i + 1:i + GAP + 1].max() > pk[i]:
                    taken.add("skip_jumps_a_larger_value")
                i += GAP
        i += 1
    if max_l / mean < thr:
        taken.add("nothing_above")
        return -1, -1, taken, margin, pk[I0:I1].max() / mean, rng_rep
    return first, max_index, taken, margin, pk[I0:I1].max() / mean, rng_rep


def _float_range(mags):
    """where sqrtf(re^2 + im^2) leaves the float range: overflow / all_zero as the model sees them; `clear` if no magnitude sits within a
    factor 1.001 of the overflow limit and what the squares lose below the normal range (denormals are kept, on the host and in the
    gfx950 build alike: a square is off by at most three denormal ulps, 4.2e-45, and a magnitude by that over 2 |z|, or by all of itself)
    is either everything, down to exact zeros, or moves the mean by less than 1e-7 of the largest magnitude (the mean is compared with
    a peak after a factor of at most 12: a twentieth of MIN_MARGIN)"""
    mags = np.asarray(mags, np.float64)
    over = mags > SQRT_FLT_MAX
    rep = dict(overflow=bool(over.any()), all_overflow=bool(over.all()), all_zero=bool((mags ** 2 < 1e-47).all()),
               over_margin=float(np.abs(mags / SQRT_FLT_MAX - 1.0).min()))
    sub = mags[mags ** 2 < 4 * FLT_MIN]
    rep["normal"] = bool(np.minimum(sub, 4.2e-45 / (2 * np.maximum(sub, 1e-300))).sum() / len(mags) <= 1e-7 * mags.max())
    rep["clear"] = rep["over_margin"] >= 1e-3 and (rep["normal"] or rep["all_zero"])
    return rep


Window = namedtuple("Window", "name x taps noise seed scale expect")


def make_window(taps, noise, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x = np.zeros(TU, np.complex128)
    for d, a in taps:
        x += a * np.roll(P_TIME, d)
    x = x + noise * (rng.standard_normal(TU) + 1j * rng.standard_normal(TU)) / np.sqrt(2.0)
    return (x * scale).astype(np.complex64)


def _admissible(x):
    return all(model_correlate(x, thr)[3] >= MIN_MARGIN and model_correlate(x, thr)[5]["clear"] for thr in THRESHOLDS)


def _window(name, taps, noise=0.05, seed=0, scale=1.0, expect=None):
    """the noise seed moves on until every comparison of the walk, under every threshold, is at least MIN_MARGIN wide"""
    for s in range(seed, seed + 1000, 50):
        x = make_window(taps, noise, s, scale)
        if _admissible(x):
            return Window(name, x, tuple(taps), noise, s, scale, expect)
    raise AssertionError("no admissible seed for " + name)


def peak_ratio(x, d):
    """pk[d] / mean of the float64 model"""
    pk = np.abs(np.fft.ifft(np.fft.fft(np.asarray(x, np.complex64).astype(np.complex128)) * np.conj(PRS))) * TU
    return float(pk[d] / (pk.sum() / TU))


def _noise_for_ratio(taps, target, seed):
    """the noise level that puts pk[d] / mean of the first tap at `target` (bisection on one noise realisation)"""
    lo, hi = 1e-3, 1e3
    for _ in range(60):
        mid = np.sqrt(lo * hi)
        lo, hi = (mid, hi) if peak_ratio(make_window(taps, mid, seed), taps[0][0]) > target else (lo, mid)
    return float(np.sqrt(lo * hi))


def correlator_windows():
    """-> list of Window.  expect = (first, strongest) at threshold 3 where the case is there to pin one (None: whatever the oracle says)"""
    w = []
    # the window's edges (the correlation of a tap has side lobes: a peak just outside is seen through its neighbour inside)
    for d, e in ((253, 254), (254, 254), (1003, 1003), (1004, 1003)):
        w.append(_window("single_%d" % d, [(d, 1.0)], seed=d, expect=(e, e)))
    # the borders of the three passes i0 + tid + 256 n of the first-peak search
    for d in (509, 510, 765, 766):
        w.append(_window("single_%d" % d, [(d, 1.0)], seed=d, expect=(d, d)))
    w.append(_window("pair_505_512", [(505, 1.0), (512, 1.3)], seed=1, expect=(512, 512)))
    for d, e in ((9, (309, 309)), (10, (300, 300)), (11, (300, 311))):
        w.append(_window("pair_300_%d" % (300 + d), [(300, 1.0), (300 + d, 1.2)], seed=10 + d, expect=e))
    w.append(_window("pair_995_1003", [(995, 1.0), (1003, 1.5)], seed=2, expect=(1003, 1003)))
    w.append(_window("weak_early_300_600", [(300, 0.5), (600, 1.0)], seed=3, expect=(300, 600)))
    w.append(_window("near_tie_above", [(300, 1.0), (330, 1.001)], noise=0.002, seed=4, expect=(300, 330)))
    w.append(_window("near_tie_below", [(300, 1.0), (330, 0.999)], noise=0.002, seed=5, expect=(300, 300)))
    # peak / mean at 0.9 x and 1.1 x each threshold
    for thr in THRESHOLDS:
        for f in (0.9, 1.1):
            seed = int(100 * thr + 10 * f)
            for s in range(seed, seed + 1000, 50):
                x = make_window([(504, 1.0)], _noise_for_ratio([(504, 1.0)], f * thr, s), s)
                if _admissible(x):
                    break
            else:
                raise AssertionError("no admissible seed")
            w.append(Window("ratio_%.1fx%g" % (f, thr), x, ((504, 1.0),), None, s, 1.0, None))
    w.append(_window("outside_only", [(100, 1.0), (1500, 1.0)], seed=6, expect=(-1, -1)))
    w.append(_window("noise_only", [], noise=1.0, seed=7))
    w.append(Window("zeros", np.zeros(TU, np.complex64), (), 0.0, 0, 1.0, (-1, -1)))
    for sc in (1e-20, 1e-10, 1e10, 1e14, 1e15):        # (1e14: the largest of them whose squares stay finite)
        w.append(_window("scale_%g" % sc, [(504, 1.0)], noise=0.1, seed=8, scale=sc))
    return w


# ------------------------------------------------------------------------------------------------ coarse search
def _relative_phase(f):
    o = np.zeros(TU, np.complex128)
    o[:-1] = np.conj(f[:-1]) * f[1:]
    return o


REF_ARG_CONJ = np.conj(np.fft.ifft(_relative_phase(PRS)) * TU)             # phasereference.cpp:47-69


def model_coarse(X):
    """The four steps of :223-280 in float64 -> dict(index, found, hz1000 = offset * 1000 before truncation (nan where it is not finite),
    branches, the margins, the float-range report of the 143 magnitudes the function reads)"""
    X = np.asarray(X, np.complex64).astype(np.complex128)
    with np.errstate(all="ignore"):
        b = np.fft.fft(np.fft.ifft(_relative_phase(X)) * TU * REF_ARG_CONJ)
        mag = np.abs(b[np.arange(-71, 72) % TU])                           # bins -71..71; mag[71 + i] is bin i
    rep = _float_range(mag)
    taken = set()
    win = mag[1:142]
    res = dict(range=rep, taken=taken, m_runner_up=np.inf, m_found=np.inf, m_int=np.inf, index=IDX_NOT_FOUND, found=True, hz1000=np.nan)
    if rep["overflow"] or rep["all_zero"]:
        # The float magnitudes are inf where |z| is beyond sqrt(FLT_MAX), or all 0.  All 0: nothing is > 0, index stays IDX_NOT_FOUND, 0 < 0
        # is false, the three bins (Tu + index + i - 1) % Tu are 0 too: 0 / 0.  Some inf: the first of them is the maximum, avg is inf,
        # inf < inf is false; a neighbour that is inf as well gives inf - inf or inf / inf, two finite neighbours give index + x / inf.
        # NaN converts to INT_MIN (cvttss2si).
        taken.add("all_inf" if rep["all_overflow"] else "some_inf" if rep["overflow"] else "all_zero")
        res["hz"] = INT_MIN
        if rep["overflow"]:
            inf = mag > SQRT_FLT_MAX
            index = int(np.argmax(inf[1:142])) - 70 if inf[1:142].any() else None
            if index is None:                                              # only bin -71 or 71: they feed no maximum
                raise AssertionError("overflow outside the search window only: not a case")
            res["index"] = index
            if not inf[71 + index - 1] and not inf[71 + index + 1]:
                res["hz"] = index * 1000
                taken.add("inf_between_finite_neighbours")
        return res
    order = np.argsort(-win, kind="stable")
    index = int(order[0]) - 70                                             # argsort is stable: the first maximum, as val > mx
    top, avg = win[order[0]], win.sum() / 141.0
    res.update(index=index, m_runner_up=(top - win[order[1]]) / top, m_found=abs(top - 5 * avg) / top)
    if top < 5 * avg:
        taken.add("not_found")
        res.update(found=False, hz=IDX_NOT_FOUND)
        return res
    p0, p1, p2 = mag[71 + index - 1], mag[71 + index], mag[71 + index + 1]
    rep["clear"] = rep["clear"] and min(p0, p1, p2) ** 2 >= 4 * FLT_MIN        # the interpolation divides them by one another
    hz = (index + (p2 - p0) / (p0 + p1 + p2)) * 1000.0
    taken.add("index_%s70" % ("+" if index > 0 else "-") if abs(index) == 70 else "inside")
    taken.add("negative" if hz < 0 else "positive")
    res.update(hz1000=hz, hz=trunc(hz), m_int=min(hz - np.floor(hz), np.ceil(hz) - hz) if hz != np.round(hz) else 0.0)
    return res


def coarse_class(m):
    """'exact': the device must return the oracle's integer; 'pm1': +-1 Hz (offset * 1000 within 4 D of an integer); None: not a case"""
    if not m["range"]["clear"]:
        return None
    if m["range"]["overflow"] or m["range"]["all_zero"]:
        return "exact"
    if m["m_found"] < COARSE_DECISION_MARGIN or (m["found"] and m["m_runner_up"] < COARSE_DECISION_MARGIN):
        return None
    return "exact" if (not m["found"] or m["m_int"] >= 4 * COARSE_D) else "pm1"


Spectrum = namedtuple("Spectrum", "name X kind")


def _spectrum_of(x_time):
    return np.fft.fft(x_time).astype(np.complex64)


def coarse_spectra():
    """-> list of Spectrum; kind: 'int' (an integer number of carriers: offset * 1000 sits ON an integer, +-1 Hz allowed),
    'pure' (the same without noise), 'frac', 'noise', 'mix', 'none' (nothing to find), 'scale'"""
    n = np.arange(TU)
    amp = TU / np.sqrt(1536.0)
    sp = []
    for k in (-70, 0, 70):                                 # as they are: offset * 1000 sits ON an integer (+-1 Hz class)
        sp.append(Spectrum("pure_roll_%+d" % k, (amp * np.roll(PRS, k)).astype(np.complex64), "pure"))
    # ... and every k under white noise 40 dB down, which moves offset * 1000 off the integer by a few Hz; the seed moves on until the
    # distance is at least 4 D and the maximum is where the roll put it
    for k in list(range(-72, 73)) + [-100, 100]:
        for seed in range(1000 + k, 3000, 173):
            r = np.random.default_rng(seed)
            X = (amp * (np.roll(PRS, k) + 0.01 * (r.standard_normal(TU) + 1j * r.standard_normal(TU)) / np.sqrt(2.0))).astype(np.complex64)
            m = model_coarse(X)
            if coarse_class(m) == "exact" and (abs(k) > 70 or (m["found"] and m["index"] == k)):
                break
        else:
            raise AssertionError("no admissible seed for roll %d" % k)
        sp.append(Spectrum("roll_%+d" % k, X, "int"))
    fr = [k + f for k in (-70, -5, 0, 5, 69) for f in (0.25, 0.499, 0.501, 0.75)] + [70.4, -70.4, 70.6, -70.6]
    for f in fr:
        sp.append(Spectrum("frac_%+.3f" % f, _spectrum_of(P_TIME * np.exp(2j * np.pi * f * n / TU)), "frac"))
    rng = np.random.default_rng(41)
    wn = (rng.standard_normal(TU) + 1j * rng.standard_normal(TU)) / np.sqrt(2.0)
    base = _spectrum_of(P_TIME * np.exp(2j * np.pi * 3.3 * n / TU)).astype(np.complex128)
    for target in (0.9, 0.99, 0.995, 1.005, 1.01, 1.1):
        lo, hi = 1e-2, 1e4
        for _ in range(80):
            mid = np.sqrt(lo * hi)
            m = model_coarse((base + mid * wn).astype(np.complex64))
            # m_found is |mx - 5 avg| / mx: mx / (5 avg) from it and the found flag
            r = 1.0 / (1.0 - m["m_found"]) if m["found"] else 1.0 / (1.0 + m["m_found"])
            lo, hi = (mid, hi) if r > target else (lo, mid)
        sp.append(Spectrum("noise_%.3f" % target, (base + np.sqrt(lo * hi) * wn).astype(np.complex64), "noise"))
    for (wa, wb) in ((0.9, 1.1), (1.1, 0.9)):
        sp.append(Spectrum("mix_%.1f_%.1f" % (wa, wb), (amp * (wa * np.roll(PRS, 10) + wb * np.roll(PRS, -20))).astype(np.complex64), "mix"))
    sp.append(Spectrum("white", (40.0 * wn).astype(np.complex64), "none"))
    sp.append(Spectrum("zeros", np.zeros(TU, np.complex64), "none"))
    shifted = _spectrum_of(np.roll(P_TIME, 0) * np.exp(2j * np.pi * 0.3 * n / TU)).astype(np.complex128)
    # 1e-16, 1e-14, 1e6, 1e9 and one scale for each thing that can happen: all magnitudes 0 (1e-25), small and normal (1e-12), large and
    # finite (1e4), seven of them inf (1e5), most (3e5), all (1e6, 1e9).  A scale at which squares are neither normal nor all 0 is left out.
    for sc in (1e-25, 1e-16, 1e-14, 1e-12, 1e4, 1e5, 3e5, 1e6, 1e9):
        X = (shifted * sc).astype(np.complex64)
        if coarse_class(model_coarse(X)) is not None:
            sp.append(Spectrum("scale_%g" % sc, X, "scale"))
    return sp


def trunc(v):
    return int(np.trunc(v))
