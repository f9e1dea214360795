"""Shared by test_scope_cases.py (no device) and test_gpu_scope_stage.py: the model of the IQ scope and the carrier plots (k_scope,
csrc/pipeline.hip with csrc/scope_core.h), the integer model of the two counters that decide which symbol is shown, and the rule by which
the device's records are compared with the model.  docs/history/scope.md tells the whole story.

The model is a float64 numpy evaluation of ofdm_decoder.cpp:162-165, 188-226, 258-291, 305-318 on the oracle's state, no device involved:
oracle/ofdm.c is driven over demap_cases.stream_frames exactly as demap_cases.run_oracle drives it; in front of a shown symbol
integ_abs_phase, phase_ref, mean_value and mean_power_ovr_all are taken from the oracle's (public) struct ora_demap, behind it the
per-carrier vectors mean_power, mean_sigma_sq and std_dev_sq; everything between the two is evaluated here in float64.

The rule (compare): per value x of the model the device may differ by A + REL |x|, REL = demap_cases.REL -- the project's accepted bar
between the device demapper and the oracle on the soft-bit products, which are formed from the same fftBin, mean power, sigma and null
power the plots are formed from.  A = REL times the plot's scale: 1 for the normed IQ vectors (|x| = the modulus of the complex value, for
both of its components), 100 for the percent plots, 180 for the degree plots; A = 0.02 for the four dB plots, the project's bar for the
SNR / MER from the same state (tests/test_gpu_demap_stage.py).  Angles compare modulo 360; PRS_PHASE_UNWRAP compares its first element and
its first differences modulo 360.  A non-finite model value demands the same class (NaN, +inf, -inf) from the device.  Frames of the
demap_cases.UNDEFINED classes (all generators: the state is NaN) compare the record's header only.
Left out: values where the model's wrapped first difference lies within the bound of +-180 would be ambiguous if the wrap decision
entered the comparison; it does not -- every degree value and every first difference is compared modulo 360 -- so the set is empty by
construction and the cap (at most LEFT_OUT_CAP of a (case, plot type)) holds with 0 left out.  left_out_share() still counts what the
literal rule names, for the record (test_scope_cases.py).
The record's two scalars: mean_value (the block sum of |r1|, a soft-bit product) compares relative to REL; mean_power_all is the state the
SNR is made from and compares within the same 0.02 dB as the SNR (the oracle's own float32 recurrence x += (0.005 / 1536) (p - x) adds
increments of 3e-6 x to x, a 2 % rounding error each, and on these inputs wanders up to 2.6e-4 relative away from the exact evaluation of
the same recurrence, which the device's closed form follows to 1e-6: csrc/ofdm_core.h, "mMeanPowerOvrAll"; docs/history/scope.md)."""
import ctypes as C
import functools

import numpy as np

import demap_cases as dc
import oracle_lib as ol

K, TU = dc.K, dc.TU
REL = dc.REL
LEFT_OUT_CAP = 0.02
IQ_TYPES = (0, 1, 2)                                            # EIqPlotType: PHASE_CORR_CARR_NORMED, PHASE_CORR_MEAN_NORMED, RAW_MEAN_NORMED
SB_WEIGHT, EVM_PER, EVM_DB, STD_DEV, PHASE_ERROR, PRS_PHASE, PRS_PHASE_UNWRAP, FOUR_QUAD_PHASE, REL_POWER, SNR = range(10)
NULL_OVR_POW = 13
CARRIER_TYPES = tuple(range(10)) + (NULL_OVR_POW,)              # ECarrierPlotType, the built ones
CARRIER_NAMES = {0: "SB_WEIGHT", 1: "EVM_PER", 2: "EVM_DB", 3: "STD_DEV", 4: "PHASE_ERROR", 5: "PRS_PHASE", 6: "PRS_PHASE_UNWRAP",
                 7: "FOUR_QUAD_PHASE", 8: "REL_POWER", 9: "SNR", 13: "NULL_OVR_POW"}
PERCENT, DEGREE, DB = (SB_WEIGHT, EVM_PER), (STD_DEV, PHASE_ERROR, PRS_PHASE, PRS_PHASE_UNWRAP, FOUR_QUAD_PHASE), (EVM_DB, REL_POWER, SNR, NULL_OVR_POW)
UNDEFINED_NAMES = frozenset(n for n, _ in dc.UNDEFINED)         # the zero_* frames and the frame behind each, every generator

# measured on the CPU (test_scope_cases.py, test_spread_between_the_two_oracle_builds_is_as_recorded): the largest |d| / (1 + |x|) of a model
# value between the IEEE and the fast-math oracle build, symbols 1, 4, 10, 75 of every frame outside UNDEFINED_NAMES, all generators
SPREAD_SYMBOLS = (1, 4, 10, 75)
SPREAD_SB_WEIGHT = 7.5e-6                 # 7.2e-6: gain_1e-5_5, generator 2
SPREAD_OTHER = 7e-7


class OraDemap(C.Structure):
    """struct ora_demap of oracle/dab_oracle.h: the two scalars have no getter."""
    _fields_ = [("phase_ref", C.c_float * (2 * TU)), ("integ_abs_phase", C.c_float * K), ("mean_power", C.c_float * K),
                ("mean_sigma_sq", C.c_float * K), ("std_dev_sq", C.c_float * K), ("mean_null_power", C.c_float * TU),
                ("mean_power_ovr_all", C.c_float), ("mean_value", C.c_float), ("perm", C.c_int16 * K), ("soft_bit_type", C.c_int),
                ("overflow_count", C.c_longlong)]


# ---- the two counters (ofdm_decoder.cpp:154-157, 323, 349-351; ofdm_decoder.h:86-88) ---------------------------------------------------
class Counters:
    """mShowCntIqScope, mShowCntStatistics, mNextShownOfdmSymbIdx: frame() is the 75 decode_symbol calls of one decoded frame and returns
    the symbol shown in it (0: none).  An absent frame calls nothing."""

    def __init__(self):
        self.cnt_iq, self.cnt_stat, self.next_sym = 0, 0, 1

    def frame(self):
        shown = 0
        for l in range(1, 76):
            self.cnt_iq += 1
            self.cnt_stat += 1
            show_scope = self.cnt_iq > 76 and l == self.next_sym
            show_stat = self.cnt_stat > 5 * 76 and l == self.next_sym
            if show_scope:
                shown, self.cnt_iq = l, 0
            if show_stat:
                self.cnt_stat = 0
                self.next_sym = (self.next_sym + 1) % 76 or 1
        return shown


def cadence(present):
    """[(index among the decoded frames, symbol)] of the shows the reference's cadence gives a stream whose steps are `present` (0 / 1)."""
    c, out, f = Counters(), [], 0
    for p in present:
        if not p:
            continue
        l = c.frame()
        if l:
            out.append((f, l))
        f += 1
    return out


# ---- which plot on which stream and frame (test_gpu_scope_stage.py; test_scope_cases.py shows that it covers every built type) ----------
FIXED_SYMBOLS = (1, 3, 4, 75)      # the first symbol (prev = phase reference, mean_value of the last frame), the last FIC symbol, the first MSC symbol, the longest replay
# (symbol, stream, step) -> carrier type: the frames in which a plot can go wrong in a way of its own
_MUST = {(1, 2, 0): REL_POWER,             # gain_1e5, start-up: the running mMeanPowerOvrAll is orders of magnitude away from the block value
         (3, 2, 0): REL_POWER, (4, 2, 0): NULL_OVR_POW,
         (1, 1, 0): SNR, (3, 1, 0): NULL_OVR_POW,      # on_axes: no null spectrum yet, the null power is exactly 0
         (4, 1, 0): PRS_PHASE_UNWRAP, (75, 1, 0): PRS_PHASE,   # ... and a real symbol 0: PRS phases at multiples of 90 degrees, jumps beyond +-180
         (75, 4, 9): PHASE_ERROR,                      # the integrator at both stops
         (1, 3, 2): SB_WEIGHT, (3, 3, 2): SNR, (4, 3, 2): EVM_DB}    # null_above_signal: signal_power <= 0
_MUST_IQ = {(1, 2, 0): 1, (3, 2, 0): 2}


def plot_plan(symbol, s, step):
    """(iq_type, carrier_type) of stream s in engine step `step` of the run that shows `symbol` in every frame."""
    i = FIXED_SYMBOLS.index(symbol)
    return (_MUST_IQ.get((symbol, s, step), (s + step + i) % 3), _MUST.get((symbol, s, step), CARRIER_TYPES[(s + step + 3 * i) % len(CARRIER_TYPES)]))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _wrap180(d):
    return (np.asarray(d, np.float64) + 180.0) % 360.0 - 180.0


def evaluate(front, behind, x, ce, gen, null_bins, spec0):
    """One shown symbol in float64.  front: integ [K], prev [K] (the phase reference at the carriers' bins), mean_value, mpa; behind:
    mean_power, mean_sigma_sq, std_dev_sq [K]; x [K] the symbol at the carriers' bins; null_bins [K]; spec0 [TU] the frame's symbol 0.
    -> dict(iq={type: [K] complex128 by nomCarrIdx}, carr={type: [K] float64 by realCarrRelIdx}, mean_value, mpa, mpa_running [K])."""
    _, bins, rel = dc._tables()
    f8 = np.float64
    with np.errstate(all="ignore"):
        prev = front["prev"].astype(np.complex128)
        pabs = np.abs(prev)
        raw = x.astype(np.complex128) * np.conj(prev) / pabs                                 # :188-189
        phase_err = f8(ce) / 1024.0 * np.pi * (K // 2 - rel) / (K // 2) + front["integ"].astype(f8)   # :192
        a = -phase_err                                                                        # cmplx_from_phase2, :70-88
        a2 = a * a
        sine = a * (a2 * f8(np.float32(-0.16034401953220367431640625)) + f8(np.float32(0.99903142452239990234375)))
        cosine = f8(np.float32(0.9994032382965087890625)) + a2 * (a2 * f8(np.float32(3.679168224334716796875e-2)) + f8(np.float32(-0.495580852031707763671875)))
        b = raw * (cosine + 1j * sine)                                                        # :194
        power = b.real * b.real + b.imag * b.imag                                             # :211
        mp, ms, sd = (behind[k].astype(f8) for k in ("mean_power", "mean_sigma_sq", "std_dev_sq"))
        mean_level = np.sqrt(mp)                                                              # :217
        nl = null_bins.astype(f8)
        sp = mp - nl                                                                          # :225-226
        sp = np.where(sp <= 0, 0.1, sp)
        mv, mpa0 = f8(front["mean_value"]), f8(front["mpa"])
        if gen == 3:                                                                          # :231-251
            w1, w2 = pabs, -140.0 / mv
        elif gen == 2:
            w1, w2 = pabs / ms / (nl / sp + f8(np.float32(0.7))), -140.0 / mv
        else:
            babs = np.sqrt(power)
            w1, w2 = np.sqrt(babs * pabs) * mean_level / (nl / sp + f8(np.float32(0.7))) / (ms * babs), -100.0 / mv
        r1 = b * w1
        inv = 1.0 / np.sqrt(mpa0) if mpa0 > 0 else 1.0                                         # :162
        # :214 inside the carrier loop: x_k after carriers 0..k, x += alpha (p_k - x), in closed form
        al = f8(np.float32(0.005)) / K
        k = np.arange(K, dtype=f8)
        d = 1.0 - al
        run = d ** (k + 1) * mpa0 + al * d ** k * np.cumsum(power * d ** (-k))
        iq = {0: b / mean_level, 1: b * inv, 2: raw * inv}                                    # :262-264
        w = (np.abs(r1.real) + np.abs(r1.imag)) / 2.0 * (-w2)                                 # :273-275, limit_min_max keeps a NaN
        w = np.where(w < 0, 0.0, np.where(w > 127.0, 127.0, w))
        prs = spec0.astype(np.complex128)[bins] * np.conj(dc.ds.prs_spectrum()[bins])          # :142
        by_k = {SB_WEIGHT: 100.0 / 127.0 * w, EVM_PER: 100.0 * np.sqrt(ms) / mean_level, EVM_DB: 10.0 * np.log10(ms / mp),
                STD_DEV: np.rad2deg(np.sqrt(sd)), PHASE_ERROR: np.rad2deg(phase_err), PRS_PHASE: np.rad2deg(np.angle(prs)),
                FOUR_QUAD_PHASE: np.rad2deg(np.angle(b)), REL_POWER: 10.0 * np.log10(mp / run), SNR: 10.0 * np.log10(mp / nl),
                NULL_OVR_POW: 10.0 * np.log10(nl / run)}
        carr = {}
        for t, v in by_k.items():
            o = np.zeros(K, f8)
            o[rel] = v
            carr[t] = o
        p = carr[PRS_PHASE]                                                                   # :305-318
        df = np.diff(p)
        df = np.where(df > 180.0, df - 360.0, np.where(df < -180.0, df + 360.0, df))
        carr[PRS_PHASE_UNWRAP] = np.concatenate([p[:1], p[0] + np.cumsum(df)])
    return dict(iq=iq, carr=carr, mean_value=float(mv), mpa=float(mpa0), mpa_running=run, unwrap_raw_diff=np.diff(p), phase_err=phase_err,
                sb_raw=(np.abs(r1.real) + np.abs(r1.imag)) / 2.0 * (-w2), signal_power_le0=int((mp - nl <= 0).sum()), power=power)


def run_model(s, gen, want, fast=False):
    """The model over the present frames of stream s with soft-bit generator gen.  want: {index among the present frames: symbols (1-based)}.
    -> {(frame, symbol): evaluate(...) + name}.  The oracle is driven exactly as demap_cases.run_oracle drives it."""
    L = ol.oracle_fastmath() if fast else ol.oracle()
    h = L.ora_demap_new()
    L.ora_demap_set_type(h, gen)
    D = C.cast(h, C.POINTER(OraDemap)).contents
    _, bins, _ = dc._tables()
    npw = [np.zeros(TU, np.float32), np.zeros(TU, np.float32)]
    out, f = {}, 0
    soft, prod = np.zeros(dc.K2, np.int16), np.zeros(dc.K2, np.float32)
    arr = lambda field, n: np.ctypeslib.as_array(field).reshape(n)            # noqa: E731
    try:
        cur = dc._state(L, h, 3, TU)
        for fr in dc.stream_frames(s):
            if not fr["present"]:
                continue
            sel = fr["np_sel"]
            cur[:] = npw[sel]
            if fr["null_fft"] is not None:
                L.ora_demap_store_null(h, fr["null_fft"])
                npw[sel][:] = cur
            L.ora_demap_store_ref(h, np.ascontiguousarray(fr["spec"][0]))
            symbols = set(want.get(f, ()))
            for l in range(1, 76):
                if l in symbols:
                    pr = arr(D.phase_ref, 2 * TU).copy().view(np.complex64)
                    front = dict(integ=arr(D.integ_abs_phase, K).copy(), prev=pr[bins], mean_value=float(D.mean_value), mpa=float(D.mean_power_ovr_all))
                L.ora_demap_symbol_products(h, np.ascontiguousarray(fr["spec"][l]), np.float32(fr["ce"]), soft, prod)
                if l in symbols:
                    behind = dict(mean_power=arr(D.mean_power, K).copy(), mean_sigma_sq=arr(D.mean_sigma_sq, K).copy(), std_dev_sq=arr(D.std_dev_sq, K).copy())
                    r = evaluate(front, behind, fr["spec"][l][bins], fr["ce"], gen, cur[bins].copy(), fr["spec"][0])
                    r["name"] = fr["name"]
                    r["integ_front"] = front["integ"]
                    r["mpa_behind"] = float(D.mean_power_ovr_all)
                    out[(f, l)] = r
            f += 1
    finally:
        L.ora_demap_free(h)
    return out


@functools.lru_cache(maxsize=None)
def _model_cached(s, gen, want_key):
    return run_model(s, gen, {f: ls for f, ls in want_key})


def model(s, gen, want):
    """run_model on the IEEE oracle, computed once per (stream, generator, set of shows) and shared: do not write into what it returns."""
    return _model_cached(s, gen, tuple(sorted((f, tuple(sorted(ls))) for f, ls in want.items())))


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def scale_of(carrier_type):
    return 100.0 if carrier_type in PERCENT else 180.0


def _classes_differ(got, exp):
    ge, ee = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    nf = ~np.isfinite(ee)
    bad = np.zeros(ee.shape, bool)
    bad[nf] = ~((np.isnan(ee[nf]) & np.isnan(ge[nf])) | (ge[nf] == ee[nf]))
    bad[~nf] = ~np.isfinite(ge[~nf])
    return bad, nf


def compare_carr(got, exp, carrier_type):
    """-> (n_bad, worst excess over the bound's REL |x| part as a multiple of A, largest |d|)."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    bad, nf = _classes_differ(got, exp)
    fin = ~nf & ~bad
    A = 0.02 if carrier_type in DB else REL * scale_of(carrier_type)
    with np.errstate(all="ignore"):
        if carrier_type == PRS_PHASE_UNWRAP:
            g = np.concatenate([got[:1], np.diff(got)])
            x = np.concatenate([exp[:1], np.diff(exp)])
            fin = fin & np.concatenate([[True], fin[:-1]])
            d = np.abs(_wrap180(g - x))
        elif carrier_type in DEGREE:
            x, d = exp, np.abs(_wrap180(got - exp))
        else:
            x, d = exp, np.abs(got - exp)
        over = fin & (d > A + REL * np.abs(x))
    n_bad = int(bad.sum() + over.sum())
    dmax = float(d[fin].max()) if fin.any() else 0.0
    return n_bad, dmax


def compare_iq(got, exp):
    got, exp = np.asarray(got, np.complex128), np.asarray(exp, np.complex128)
    n_bad, dmax = 0, 0.0
    with np.errstate(all="ignore"):
        mod = np.abs(exp)
    for g, x in ((got.real, exp.real), (got.imag, exp.imag)):
        bad, nf = _classes_differ(g, x)
        fin = ~nf & ~bad
        with np.errstate(all="ignore"):
            d = np.abs(g - x)
            over = fin & (d > REL * 1.0 + REL * np.where(np.isfinite(mod), mod, np.abs(x)))
        n_bad += int(bad.sum() + over.sum())
        if fin.any():
            dmax = max(dmax, float((d[fin] / (1.0 + np.where(np.isfinite(mod), mod, np.abs(x))[fin])).max()))
    return n_bad, dmax


def scalar_ok(got, exp):
    if not np.isfinite(exp):
        return (np.isnan(exp) and np.isnan(got)) or got == exp
    return abs(float(got) - float(exp)) <= REL * abs(float(exp)) + 1e-37


def mpa_ok(got, exp):
    """mean_power_all of the record: within 0.02 dB (see the module's text)."""
    if not np.isfinite(exp) or exp <= 0:
        return scalar_ok(got, exp)
    return got > 0 and abs(10.0 * np.log10(float(got) / float(exp))) <= 0.02


def left_out_share(exp_unwrap_raw_diff):
    """What the literal rule names: the share of the model's raw first differences of PRS_PHASE within the bound of +-180."""
    d = np.abs(np.asarray(exp_unwrap_raw_diff, np.float64))
    with np.errstate(all="ignore"):
        return float((np.abs(d - 180.0) <= REL * 180.0 + REL * d).mean())
