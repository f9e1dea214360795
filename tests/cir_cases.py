"""Inputs and float64 models for the channel impulse response plot and the correlation plot (csrc/cir_core.h; pipeline.hip k_cir,
k_cir_finish, k_cir_corr; docs/history/cir.md), line-cited to the reference:

  row_model        one CIR row, CirViewer::show_cir (base/spectrum_viewer/cir_viewer.cpp:66-95, scalar build)
  Walk             the window / row schedule: which rows of which window a front-end step computes (sample_reader.cpp:179-196, :250-265 give
                   the window, the step-wise schedule is the engine's: cir_rows_due / cir_rows_advance)
  trusted          the trust rule, and TRUST_TABLE, the table the host entry is held to
  CorrPlot         the display state machine of PhaseReference::correlate_with_phase_ref_and_find_max_peak, a literal transcription of
                   base/ofdm/phasereference.cpp:110-195
The bar for floats is the project's figure for this correlation, 2e-5 x the row's (window's) largest model value
(docs/history/sync_stage_tests.md: two float transforms of 2e-6 each with a unit-modulus product between them, five times over)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import sync_cases as sc  # noqa: E402

TU, TG, TF = 2048, 504, 196608
ROW_STEP = 512                                  # cir_viewer.cpp:68
WINDOW = 97 * TU                                # CIR_BUFF_SIZE / CIR_SPECTRUMSIZE
ROWS = (WINDOW - TU) // ROW_STEP + 1            # sPlotLength, :56
PERIOD = 6 * TF                                 # sample_reader.cpp: a capture every six frames' worth of samples
SCALE = 26000.0                                 # :93
BAR = 2e-5                                      # x the largest model value of the row / the window
I0, I1, GAP = sc.I0, sc.I1, sc.GAP              # phasereference.cpp:136-139
MAX_INDICES = 69
INPUT_RATE = 2048000
assert ROWS == 385 and PERIOD == 1179648 and WINDOW == 198656 and -(-(I1 - I0) // (GAP + 1)) == MAX_INDICES
PRS, P_TIME = sc.PRS, sc.P_TIME
SQRT_FLT_MAX = sc.SQRT_FLT_MAX


# ------------------------------------------------------------------------------------------------ the row
def row_power(x):
    """|backward(forward(x) conj(ref))|^2 of one row, float64, unnormalised transforms (:69, :74-77, :79)"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    z = np.fft.ifft(np.fft.fft(x) * np.conj(PRS)) * TU
    return z.real ** 2 + z.imag ** 2


def row_model(x):
    """y of one row (:86-93): sqrt(max) / 26000 with max starting at 0 and a strict `>`.  A NaN anywhere makes every output of the
    transforms NaN, no comparison is won and the row is 0; a largest square beyond the float range is inf in float, and so is the row."""
    x = np.asarray(x, np.complex64)
    if not np.isfinite(x.view(np.float32)).all():
        return 0.0                              # (an inf sample: inf - inf in the first butterfly, NaN everywhere)
    p = row_power(x)
    mx = 0.0
    for v in p:                                 # :87-92, literally
        if v > mx:
            mx = v
    if mx > float(np.finfo(np.float32).max):
        return float("inf")
    return float(np.sqrt(mx)) / SCALE


def make_row(taps, noise=0.0, seed=0, scale=1.0):
    """the phase reference symbol in time at the taps' delays and weights (cyclic), plus noise"""
    return sc.make_window(taps, noise, seed, scale)


def rows():
    """-> list of (name, x [2048] complex64, what the row is there for).  Scales at which squares are neither normal floats nor all zero
    are left out, as in sync_cases.py."""
    r = []
    for d in (0, 1, 511, 512, 2047):
        r.append(("delay_%d" % d, make_row([(d, 1.0)]), "the peak's position does not matter, every lag is looked at"))
    r.append(("two_taps", make_row([(100, 1.0), (420, 0.35)]), "the larger tap wins"))
    r.append(("two_taps_late_larger", make_row([(100, 0.6), (1900, 1.0)]), "the larger tap wins, wherever it lies"))
    r.append(("three_taps", make_row([(7, 0.8), (300, 1.0), (301, 0.5)]), "neighbouring lags"))
    r.append(("tap_and_noise", make_row([(700, 1.0)], noise=0.5, seed=11), "a peak over a noise floor"))
    r.append(("noise_only", make_row([], noise=1.0, seed=12), "no peak: the largest noise lag"))
    r.append(("zeros", np.zeros(TU, np.complex64), "exactly 0"))
    x = make_row([(300, 1.0)], noise=0.1, seed=13)
    x[1234] = complex(np.nan, 0.0)
    r.append(("nan_sample", x, "exactly 0: a NaN wins no comparison"))
    r.append(("overflow", make_row([(300, 1.0)], noise=0.1, seed=14, scale=1e17), "the peak's square overflows: inf"))
    r.append(("all_squares_zero", make_row([(300, 1.0)], noise=0.1, seed=15, scale=1e-28), "every square is 0: exactly 0"))
    r.append(("large_finite", make_row([(300, 1.0)], noise=0.1, seed=16, scale=1e14), "the largest scale whose squares stay finite"))
    return r


def row_expectation(name, x):
    """-> ('exact', value) or ('bar', model value)"""
    if name in ("zeros", "nan_sample", "all_squares_zero"):
        return "exact", 0.0
    if name == "overflow":
        return "exact", float("inf")
    return "bar", row_model(x)


# ------------------------------------------------------------------------------------------- the window walk
class Walk:
    """cir_rows_due / cir_rows_advance (csrc/cir_core.h): base, the window being computed, the rows of it that are done"""

    def __init__(self, base, win=0, rows_done=0):
        self.base, self.win, self.rows_done = int(base), int(win), int(rows_done)

    def w0(self):
        return self.base + self.win * PERIOD

    def step(self, wr, cap=ROWS):
        """one front-end step with wr committed samples -> (rows due, first sample of the first of them, 1 if the record completes)"""
        first = self.w0() + self.rows_done * ROW_STEP
        n = 0
        while (n < cap and self.rows_done + n < ROWS                                   # never beyond the window, never more than cap
               and self.w0() + (self.rows_done + n) * ROW_STEP + TU <= wr):            # the row's last sample is committed
            n += 1
        self.rows_done += n
        done = 0
        if self.rows_done == ROWS:                                                     # row 384 completes the record
            self.rows_done, self.win, done = 0, self.win + 1, 1
        return n, first, done


def walk_table():
    """(base, win, rows_done, wr, cap) tuples for the host entry: every row boundary +-1 sample around wr, the last row, the hand-over to
    window n + 1, a window further on, caps that bind"""
    t = []
    for base in (0, 4243, 196608 * 3 + 77):
        for win in (0, 1, 5):
            w0 = base + win * PERIOD
            for j in range(ROWS):                                                      # EVERY row boundary
                for d in (-1, 0, 1):
                    wr = w0 + j * ROW_STEP + TU + d                                    # row j's last sample +-1
                    for rows_done in sorted({0, max(0, j - 1), j, min(j + 1, ROWS - 1)}):
                        for cap in ((ROWS, 64, 1, 0) if j in (0, 1, 2, 63, 64, 383, 384) else (ROWS, 3)):
                            t.append((base, win, rows_done, wr, cap))
            for wr in (0, w0, w0 + TU - 1, w0 + WINDOW - 1, w0 + WINDOW, w0 + WINDOW + 1, w0 + PERIOD + TU, w0 + 3 * PERIOD):
                for rows_done in (0, 200, 384):
                    t.append((base, win, rows_done, wr, ROWS))
    return t


# -------------------------------------------------------------------------------------------- the trust rule
def trusted(first, rd, horizon, ring_len):
    """a row may be read if its first sample has not been read yet, or nothing issued reaches round the ring to it"""
    return first >= rd or first >= horizon - ring_len


U64 = 2 ** 64 - 1


def trust_table():
    """(first, rd, horizon, ring_len, expected): first == rd, first == horizon - ring_len +- 1, horizon = ~0, a horizon below the ring length"""
    t = []
    for ring_len in (4096, 23 * TF):
        for first in (0, 1, 511, 512, 10 * TF + 5, 40 * TF):
            for rd in sorted({0, max(first - 1, 0), first, first + 1, first + 2 * TF}):
                for horizon in sorted({0, ring_len - 1, ring_len, first + ring_len - 1, first + ring_len, first + ring_len + 1, first + 2 * ring_len, U64}):
                    t.append((first, rd, horizon, ring_len, bool(trusted(first, rd, horizon, ring_len))))
    return t


# --------------------------------------------------------------------------------------- the correlation plot
class CorrPlot:
    """PhaseReference's display state (phasereference.h: mMeanCorrPeakValues, mDisplayCounter) and
    correlate_with_phase_ref_and_find_max_peak, phasereference.cpp:110-195, line by line in float64.  call(pk, thr) takes |corr| of one
    sync window and returns (start index or -1, the show or None); a show is (mean [2048], threshold line, indices)."""
    FRAMES_PER_SECOND = 10                                   # cFramesPerSecond (glob_defs.h)

    def __init__(self):
        self.mean = np.zeros(TU, np.float64)
        self.counter = 0
        self.terms = 0                                       # |corr| vectors accumulated since the stream was enabled (for the bar)
        self.margin = np.inf                                 # the narrowest comparison any walk evaluated, / max(pk)
        self.branches = set()

    def call(self, pk, thr):
        pk = np.asarray(pk, np.float64)
        self.mean += pk                                      # :121 -- on every call, in front of every return
        self.terms += 1
        s = pk.sum()                                         # :122
        s /= TU                                              # :126
        if s == 0:                                           # :128
            self.branches.add("zero_sum")
            return -1, None
        indices = []                                         # :133
        max_index, max_l = -1, -1000.0                       # :134-135
        top = pk.max()
        i = I0
        while i < I1:                                        # :143
            self.margin = min(self.margin, abs(pk[i] - thr * s) / top)
            if pk[i] / s > thr:                              # :145
                found_one = True
                j = 1
                while j < GAP and i + j < I1:                # :149
                    self.margin = min(self.margin, abs(pk[i + j] - pk[i]) / top)
                    if pk[i + j] > pk[i]:                    # :151
                        found_one = False
                        break
                    j += 1
                if found_one:
                    indices.append(i)                        # :159
                    if pk[i] > max_l:                        # :161
                        max_l, max_index = pk[i], i
                    i += GAP                                 # :166
            i += 1
        if max_l / s < thr:                                  # :171 -- returns without counting
            self.branches.add("accumulated_but_not_counted")
            return -1, None
        show = None
        self.counter += 1                                    # :179
        if self.counter > self.FRAMES_PER_SECOND // 2:       # :181
            self.mean /= (self.FRAMES_PER_SECOND // 2 + 1)   # :188
            show = (self.mean.copy(), s * thr, list(indices))   # :191-192
            self.counter = 0                                 # :193 -- and nothing clears the mean
            self.branches.add("show_%d_indices" % min(len(indices), 2))
        else:
            self.branches.add("counted")
        return indices[0], show                              # :211 (first-peak mode)


def corr_pk(x):
    """|corr| over the 2048 lags of one (already mixed) sync window, float64 (:90-105, :119)"""
    x = np.asarray(x, np.complex128)
    return np.abs(np.fft.ifft(np.fft.fft(x) * np.conj(PRS)) * TU)


def nco_mix(x, phase0, f):
    """SampleReader's oscillator on n samples that follow phase `phase0` at the rounded frequency f: sample i is multiplied by the table entry
    at (phase0 - (i + 1) f) mod 2 048 000 (sample_reader.cpp:205-214); -> (mixed samples in float64, the phase behind them)"""
    n = len(x)
    p = (phase0 - (np.arange(1, n + 1, dtype=np.int64) * int(f))) % INPUT_RATE
    osc = np.exp(2j * np.pi * p.astype(np.float64) / INPUT_RATE).astype(np.complex64).astype(np.complex128)
    return np.asarray(x, np.complex64).astype(np.complex128) * osc, int((phase0 - n * int(f)) % INPUT_RATE)
