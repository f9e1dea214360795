"""Shared by test_demap_cases.py (no device) and test_gpu_demap_stage.py: crafted spectra for the engine's demapper (demap_frame_body,
csrc/pipeline.hip, with demap_pair / cvt4_i16_x86 of csrc/ofdm_core.h), the oracle run that gives every expected value, and the rule by
which the device's soft bits are compared with it.  docs/history/demap_stage_tests.md tells the whole story.

Shape: six streams, a different case per stream and frame, all three soft-bit generators on the same spectra.  Four frames of cases per
stream and a fifth behind them (the integrator stream: ten, the stream with an absent frame: six, the stream with the `wrap` pairs: seven;
see PLAN): the time de-interleaver hands
out its first logical frame with the 17th CIF, so only a fifth frame puts MSC bytes behind the demapper's ring stores.  Carrier magnitudes stay within [1e-6, 1e6]: denormal intermediates are out of scope.

The rule (compare): per soft bit, with x the IEEE oracle's float product r1 * w2 in front of the (i16) cast
  * x NaN, +-inf or |x| >= 2^31 (1 + 1e-4): the device value must be exactly 0 (cvttss2si's "integer indefinite", low 16 bits);
  * |x| within a factor 1 +- 1e-4 of 2^31: left out;
  * otherwise d = device - oracle int16 modulo 2^16, folded into [-2^15, 2^15): |d| <= 3 + REL |x| always, |d| <= 1 + REL |x| on
    >= 99.9 % of the compared bits of a case -- the stage test's bar (tests/test_gpu_stages.py), made relative for large products;
  * a product whose bound 3 + REL |x| exceeds 2^13 is left out (the comparison modulo 2^16 would mean little);
  * what is left out may be at most 2 % of the soft bits of any (case, generator).
REL: the largest relative difference between the IEEE oracle and the build with the reference's own float flags (-O3 -ffast-math
-fsingle-precision-constant, `make -C oracle fastmath`), over all finite products with |x| > 1 of all cases, times 4 -- the device
replaces about ten chained divisions and roots by 1-ulp v_rcp / v_rsq / v_sqrt and sums mMeanValue in another order (the project's own
bound for that: 1e-5).  tests/test_demap_cases.py asserts that the measured spread still lies under SPREAD_MEASURED."""
import ctypes as C
import functools
import os
import sys

import numpy as np

import oracle_lib as ol

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

K, K2, TU = 1536, 3072, 2048
N_STREAMS = 6
GENERATORS = (1, 2, 3)

# measured on the CPU (test_demap_cases.py, test_spread_and_undefined_list_are_as_recorded): the largest relative difference of a
# finite product with |x| > 1 between the two oracle builds, all cases and generators outside UNDEFINED
SPREAD_MEASURED = 1.3e-5                  # 1.28e-5: gain_1e-5_5, generator 2 (signal power = mean power - noise power cancels); 1.6e-6 outside that stream
REL = 4 * SPREAD_MEASURED
# (case, generator) pairs in which the two oracle builds disagree beyond the rule: undefined in the reference, compared on the integer
# layer only.  Only the frames of the zero_carrier and zero_reference classes may appear here (the frame with the zero and the one behind it:
# the IEEE build's stream is dead from the zero on, the other build's generator 3 is not).
UNDEFINED = frozenset({("zero_carrier", 3), ("zero_carrier_next", 3), ("zero_reference", 3), ("zero_reference_next", 3)})

TWO31 = 2147483648.0
NEAR = 1e-4
BOUND_MAX = 8192.0
LEFT_OUT_CAP = 0.02

# three sub-channels of different sizes (EEP 3-A, 2-A, 1-A), not DAB+; the first spans an OFDM symbol boundary of the CIF (48 CU per symbol),
# the last ends with the CIF
SUBCH = [ds.SubCh(1, 40, 48, 64, 2, 0, dab_plus=0), ds.SubCh(2, 500, 8, 8, 1, 0, dab_plus=0), ds.SubCh(3, 864 - 48, 48, 32, 0, 0, dab_plus=0)]

# ---- the plan: stream -> frames.  Keys: name, kind, gain (carrier amplitudes are gain * [lo, hi] of the stream), sigma (noise per
# component relative to gain), ce (clock_err), np_sel, null (amplitude of the injected null spectrum relative to gain, None: no null
# spectrum), present.
# A fifth frame follows each stream's four cases (20 CIFs: four logical frames per sub-channel; behind a zero carrier it shows the dead stream).
# The integrator stream has ten frames: the integrator moves by 1e-3 * (phase offset < pi/4) per symbol, so from rest no input reaches a
# 20-degree stop in fewer than 0.349 / 0.785e-3 = 445 symbols, and a 40-degree tilt needs ln 2 / 1e-3 = 693 of them (9.3 frames).  The other
# streams have no frame in the steps behind their last one.
def _f(name, kind="natural", gain=1.0, sigma=0.07, ce=0.0, np_sel=0, null=0.05, present=1, quiet=1.0):
    return dict(name=name, kind=kind, gain=gain, sigma=sigma, ce=ce, np_sel=np_sel, null=null, present=present, quiet=quiet)


PLAN = [
    dict(amp=(0.5, 1.5), frames=[_f("natural"), _f("clock_err_+12.5", ce=12.5), _f("clock_err_-400", ce=-400.0), _f("zero_carrier", kind="zero_carrier"),
                                 _f("zero_carrier_next")]),
    dict(amp=(0.5, 1.5), frames=[_f("on_axes", kind="on_axes", sigma=0.0, null=None), _f("noise_free", sigma=0.0), _f("clock_err_+400", ce=400.0),
                                 _f("zero_reference", kind="zero_reference"), _f("zero_reference_next")]),
    dict(amp=(0.5, 1.5), frames=[_f("gain_1e5", gain=1e5), _f("int_indefinite", kind="int_indefinite", gain=5e-3), _f("clock_err_-12.5", ce=-12.5),
                                 _f("wrap_deep", kind="wrap", gain=1e3, quiet=1e-8), _f("wrap_shallow", kind="wrap", quiet=2e-4),
                                 _f("wrap_deep_2", kind="wrap", gain=1e3, quiet=1e-8), _f("wrap_shallow_2", kind="wrap", quiet=2e-4)]),
    dict(amp=(2.0, 4.0), frames=[_f("dropout", kind="dropout"), _f("np_sel_1", np_sel=1, null=0.3), _f("null_above_signal", kind="null_above", null=10.0),
                                 _f("np_sel_1_again", np_sel=1, null=0.1), _f("np_sel_0", null=0.2)]),
    dict(amp=(0.5, 1.5), frames=[_f("integrator_stops_%d" % i, kind="tilt", sigma=0.02, null=None if i else 0.05) for i in range(10)]),
    # (gain 1e-5 has a stream of its own: behind gain 1e5 the per-carrier means are 1e20 times the signal power and the squares of the
    #  weighted carriers fall below FLT_MIN -- denormal intermediates, out of scope)
    dict(amp=(0.5, 1.5), frames=[_f("gain_1e-5", gain=1e-5), _f("absent", gain=1e-5, present=0, null=None), _f("gain_1e-5_after_absent", gain=1e-5),
                                 _f("gain_1e-5_np_sel_1", gain=1e-5, np_sel=1, null=0.2), _f("gain_1e-5_4", gain=1e-5), _f("gain_1e-5_5", gain=1e-5)]),
]
N_STEPS = max(len(p["frames"]) for p in PLAN)
INT_INDEFINITE_SYMBOLS = (10, 30, 50)          # 1-based OFDM symbols of the int_indefinite frame that carry 64 boosted carriers each
# The two `wrap` frames exist for the symbol conversion: soft_to_sym and soft_to_sym_sat differ for soft bits in [32641, 32767] only, and the
# integer layer sees them only where the FIC or a sub-channel decodes them.  Behind a quiet symbol the products of a full-level one are
# about 100 / sqrt(quiet) (generator 1) or 140 / quiet (generators 2, 3) times a per-carrier factor: with quiet = 1e-8 generator 1's, with
# 2e-4 the other two's spread over many multiples of 2^16, and 127 / 65536 of them fall into that band.  The quiet symbols stand in front
# of FIC symbol 2 and of the symbols that hold sub-channel 3 (the last of a CIF) and sub-channel 1 (the first two of the next CIF).
WRAP_QUIET_SYMBOLS = [1, 19, 20, 37, 38, 55, 56, 73, 74]
ZERO_SYMBOL, ZERO_CARRIER = 10, 777            # zero_carrier: carrier k = 777 of OFDM symbol 10 is exactly 0; zero_reference: of symbol 0


def frame_of(s, step):
    """The plan entry of stream s in engine step `step`, or None (the stream has run out of frames: it has none in this step)."""
    fr = PLAN[s]["frames"]
    return fr[step] if step < len(fr) else None


@functools.lru_cache(maxsize=None)
def _tables():
    perm = ds.freq_perm()                                    # carrier k -> signed carrier index (-768 .. 768 without 0)
    bins = (perm % TU).astype(np.int64)
    rel = np.where(perm < 0, perm + K // 2, perm + K // 2 - 1)
    return perm, bins, rel


@functools.lru_cache(maxsize=None)
def ensemble():
    """One multiplex for all streams: the FIC and three sub-channels, N_STEPS frames (not cyclic: the first CIFs' interleaver history is empty)."""
    return ds.build_ensemble(N_STEPS, SUBCH, seed=91, cyclic=False)


def _noise(rng, shape, sigma):
    return sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


@functools.lru_cache(maxsize=None)
def stream_frames(s):
    """The frames of stream s: list of dict(plan entry + spec [76, 2048] complex64 in FFT bin order, null_fft [2048] complex64 or None)."""
    _, bins, rel = _tables()
    tx = ensemble().tx_bits
    srng = np.random.default_rng([4711, s])
    lo, hi = PLAN[s]["amp"]
    amp = np.zeros(TU)
    amp[bins] = lo + (hi - lo) * srng.random(K)
    prs = ds.prs_spectrum()
    out = []
    for f, p in enumerate(PLAN[s]["frames"]):
        rng = np.random.default_rng([4712, s, f])
        g, kind = p["gain"], p["kind"]
        bits = tx[f]
        if kind == "on_axes":
            # quarter-turn constellation on a real symbol 0 of either sign: the first symbol lands exactly on the axes, with both signs of zero
            z = amp.astype(np.complex128)
            turns = np.array([1, 1j, -1, -1j])
            y = turns[2 * bits[:, :K] + bits[:, K:]]
        else:
            z = prs * amp
            y = ((1 - 2.0 * bits[:, :K]) + 1j * (1 - 2.0 * bits[:, K:])) / np.sqrt(2)
        # what the demapper takes out again: the clock-error ramp over the carriers (ofdm_decoder.cpp:192) ...
        y = y * np.exp(1j * (p["ce"] / 1024.0 * np.pi * (K // 2 - rel) / (K // 2)))[None, :]
        if kind == "tilt":                                   # ... and, for the integrator, +40 / -40 degrees per symbol on alternating carriers
            y = y * np.exp(1j * np.deg2rad(40.0) * np.where(np.arange(K) & 1, -1.0, 1.0))[None, :]
        spec = np.zeros((76, TU), np.complex128)
        spec[0] = z
        for l in range(1, 76):
            yy = np.ones(TU, np.complex128)
            yy[bins] = y[l - 1]
            z = z * yy
            spec[l] = z
        scale = np.ones((76, 1))
        if kind == "wrap":                                   # quiet symbols in front of a FIC symbol and of symbols that lie in sub-channels
            scale[WRAP_QUIET_SYMBOLS] = p["quiet"]
            if p["name"].endswith("_2"):                      # the second pair: FIC symbols 1 and 2 quiet, symbol 3 behind them
                scale[2] = p["quiet"]
        if kind == "dropout":                                # 4 symbols at 1e-4, later 3 at 1e-6, full level in between and after
            scale[20:24] = 1e-4
            scale[48:51] = 1e-6
        spec = (spec + _noise(rng, spec.shape, p["sigma"])) * (g * scale)
        if kind == "on_axes":
            spec = np.where(np.abs(prs)[None, :] > 0, spec, 0)
            spec32 = (spec.real.astype(np.float32) + 1j * spec.imag.astype(np.float32)).astype(np.complex64)
            # exact quarter turns of float values, computed in float: products with 0 keep the sign of zero a complex multiply gives them
            spec32[0] = np.where(np.abs(prs) > 0, (g * amp * np.where(srng.random(TU) < 0.5, -1.0, 1.0)).astype(np.float32), 0).astype(np.complex64)
            t32 = np.array([1, 1j, -1, -1j], np.complex64)
            for l in range(1, 76):
                yy = np.ones(TU, np.complex64)
                yy[bins] = t32[2 * bits[l - 1, :K] + bits[l - 1, K:]]
                spec32[l] = spec32[l - 1] * yy
        else:
            spec32 = spec.astype(np.complex64)
        if kind == "int_indefinite":
            # 64 known carriers per chosen symbol, boosted by 1e7 .. 1e8: generator 3's products there are about 99 * boost, on both sides of 2^31,
            # with the signs of the data
            for j, l in enumerate(INT_INDEFINITE_SYMBOLS):
                ks = np.arange(64) * 24 + j
                spec32[l, bins[ks]] *= np.float32(1e7) * np.float32(10.0) ** (np.arange(64, dtype=np.float32) / 63)
        if kind == "zero_carrier":
            spec32[ZERO_SYMBOL, bins[ZERO_CARRIER]] = 0
        if kind == "zero_reference":
            spec32[0, bins[ZERO_CARRIER]] = 0
        null = None
        if p["null"] is not None:
            nl = _noise(rng, TU, p["null"] * g)
            if kind == "null_above":                         # a third of the carriers: null power far above the carrier power
                nl = _noise(rng, TU, 0.05 * g)
                nl[bins[::3]] = p["null"] * g * hi * np.exp(2j * np.pi * rng.random(len(bins[::3])))
            null = nl.astype(np.complex64)
        a = np.abs(spec32[:, bins])
        if kind not in ("zero_carrier", "zero_reference"):
            assert a.min() >= 1e-6 and a.max() <= 1e6, (p["name"], a.min(), a.max())
        spec32.setflags(write=False)
        out.append(dict(p, spec=spec32, null_fft=null))
    return out


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def _state(L, h, which, n):
    return np.ctypeslib.as_array(L.ora_demap_state(h, which), (n,))


def run_oracle(s, gen, fast=False):
    """oracle/ofdm.c over the present frames of stream s with soft-bit generator gen (fast: the build with the reference's float flags).
    Two noise-power buffers are kept as the engine keeps them: a frame's null spectrum advances the one its np_sel names, and the demapper
    reads that one.  One record per present frame: soft [75, 3072] int16, prod [75, 3072] float32 (the products in front of the cast),
    snr_db, mer_db, and the branch counters of test_demap_cases.py."""
    L = ol.oracle_fastmath() if fast else ol.oracle()
    h = L.ora_demap_new()
    L.ora_demap_set_type(h, gen)
    _, bins, _ = _tables()
    npw = [np.zeros(TU, np.float32), np.zeros(TU, np.float32)]
    lim = np.float32(np.float32(np.pi / 180.0) * np.float32(20.0))
    out = []
    try:
        cur = _state(L, h, 3, TU)
        integ, mean_power = _state(L, h, 0, K), _state(L, h, 1, K)
        for fr in stream_frames(s):
            if not fr["present"]:
                continue
            sel = fr["np_sel"]
            cur[:] = npw[sel]
            if fr["null_fft"] is not None:
                L.ora_demap_store_null(h, fr["null_fft"])
                npw[sel][:] = cur
            L.ora_demap_store_ref(h, np.ascontiguousarray(fr["spec"][0]))
            soft = np.zeros((75, K2), np.int16)
            prod = np.zeros((75, K2), np.float32)
            nan_mean = sp_le0 = stop_hi = stop_lo = 0
            for l in range(75):
                L.ora_demap_symbol_products(h, np.ascontiguousarray(fr["spec"][1 + l]), np.float32(fr["ce"]), soft[l], prod[l])
                nan_mean += int(np.isnan(L.ora_demap_mean_value(h)))
                sp_le0 += int((mean_power - cur[bins] <= 0).sum())
            stop_hi, stop_lo = int((integ == lim).sum()), int((integ == -lim).sum())
            out.append(dict(name=fr["name"], soft=soft, prod=prod, snr_db=float(L.ora_demap_snr_db(h)), mer_db=float(L.ora_demap_mer_db(h)),
                            nan_mean=nan_mean, sp_le0=sp_le0, stop_hi=stop_hi, stop_lo=stop_lo))
    finally:
        L.ora_demap_free(h)
    return out


@functools.lru_cache(maxsize=None)
def oracle_stream(s, gen):
    return run_oracle(s, gen)


@functools.lru_cache(maxsize=None)
def decoded_mask(n_frames):
    """(fic [n_frames, 75, 3072] bool, msc likewise): the soft bits of a stream's n_frames present frames that the integer layer observes --
    all of symbols 1..3 (every FIC soft bit enters a trellis), and the bits of the three sub-channels that a logical frame which comes out
    is made of: received bit i of CIF t belongs to logical frame r = t - delay(i & 15) (the transmitter puts bit i of coded CIF r into CIF
    r + delay), and with 4 n_frames CIFs the frames r = 0 .. 4 n_frames - 17 come out.  test_demap_cases.py proves the MSC half on the
    oracle back end: soft bits outside the mask do not reach its bytes, soft bits inside do."""
    fic = np.zeros((n_frames, 75, K2), bool)
    fic[:, :3] = True
    cif = np.zeros((4 * n_frames, 55296), bool)
    i = np.arange(55296)
    in_sc = np.zeros(55296, bool)
    for sc in SUBCH:
        in_sc |= (i >= sc.cu_start * 64) & (i < (sc.cu_start + sc.cu_size) * 64)
    for t in range(4 * n_frames):
        r = t - ds.INTERLEAVE_MAP[i & 15]
        cif[t] = in_sc & (r >= 0) & (r <= 4 * n_frames - 17)
    msc = np.zeros((n_frames, 75, K2), bool)
    msc[:, 3:] = cif.reshape(n_frames, 72, K2)
    return fic, msc


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def classify(x):
    """(must_be_zero, left_out, bound) per product x (IEEE oracle, float32): the three bands of the rule and 3 + REL |x| elsewhere."""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    zero = ~np.isfinite(x) | (ax >= TWO31 * (1 + NEAR))
    with np.errstate(invalid="ignore"):
        near = ~zero & (ax > TWO31 * (1 - NEAR))
        bound = 3.0 + REL * np.where(zero, 0.0, ax)
        left = near | (~zero & (bound > BOUND_MAX))
    return zero, left, bound


def fold16(d):
    return ((np.asarray(d, np.int64) + 32768) & 0xFFFF) - 32768


def compare(got, exp_soft, prod):
    """The rule on one frame of one stream ([75, 3072] each): dict(ok, n_zero_bad, n_hard_bad, frac_soft_bad, frac_left_out, worst)."""
    zero, left, bound = classify(prod)
    got = np.asarray(got, np.int16)
    d = np.abs(fold16(got.astype(np.int64) - exp_soft.astype(np.int64)))
    cmp_ = ~zero & ~left
    n_zero_bad = int((got[zero] != 0).sum())
    n_hard_bad = int((d[cmp_] > bound[cmp_]).sum())
    soft_bad = float((d[cmp_] > bound[cmp_] - 2.0).mean()) if cmp_.any() else 0.0
    frac_left = float(left.mean())
    worst = float((d[cmp_] - REL * np.abs(prod[cmp_].astype(np.float64))).max()) if cmp_.any() else 0.0
    ok = n_zero_bad == 0 and n_hard_bad == 0 and soft_bad <= 1e-3 and frac_left <= LEFT_OUT_CAP
    return dict(ok=ok, n_zero_bad=n_zero_bad, n_hard_bad=n_hard_bad, frac_soft_bad=soft_bad, frac_left_out=frac_left, worst=worst,
                n_zero=int(zero.sum()), n_compared=int(cmp_.sum()))


# ---- the integer layer: the oracle back ends on the device's own soft bits ------------------------------------------------------------
def fic_of(soft_frames, mode):
    """oracle/fic.c on captured frames [n, 75, 3072] int16 of one stream: per frame (fibs [12, 32], crc [12])."""
    import fic_cases as fc
    frames = np.ascontiguousarray(np.asarray(soft_frames, np.int16)[:, :3].reshape(-1, 3 * K2))
    recs = fc.oracle_calls(fc.symbol_calls(frames), mode)
    return [(r["fibs"], r["crc"]) for r in recs[2::3]]


def msc_of(soft_frames, mode):
    """oracle/msc.c on the same: per slot of SUBCH the logical frames [4 n - 16, 3 kbps] (symbols 4..75 of a frame are its four CIFs)."""
    import msc_cases as mc
    cifs = np.ascontiguousarray(np.asarray(soft_frames, np.int16)[:, 3:].reshape(-1, mc.CIF_BITS))
    return mc.oracle_frames(SUBCH, cifs, tie_mode=mode, threads=3)
