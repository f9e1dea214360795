"""Inputs and models for the RF spectrum and waterfall stage (csrc/spectrum_core.h; pipeline.hip k_spectrum; docs/history/spectrum.md),
line-cited to the reference:

  window           create_flattop_window (common/glob_defs.h:252-266): double, cast to float
  row64 / Row64    one show in float64: SpectrumViewer::show_spectrum (base/spectrum_viewer/spectrum_viewer.cpp:169-218)
  row32            the same lines in float32, operation by operation (the transform is the oracle's float one)
  limits32         spectrum_viewer.cpp:220-230 with _calc_spectrum_display_limits (:112-139) and waterfall_scope.cpp:57-60, float32 line by line:
                   what dabx_spectrum_limits is held to EXACTLY
  pixels           waterfall_scope.cpp:73-74
  Reader           the capture schedule: SampleReader's specBuffIdx / sampleCount (base/ofdm/sample_reader.cpp:198-205, :267-272, :285-296),
                   call by call; shows_of_trace replays the oracle receiver's event trace through it
The bars (the issue's comparison rule): linear values within 2e-5 of the window's largest model value (docs/history/sync_stage_tests.md);
one un-averaged dB value within 20 log10(1 + 2e-5 m_max / (m_i + 1e-6 * 512)) + 1e-4 dB; averaged values: the bound through the same 0.2
recurrence; extrema and limits: the largest per-bin bound of the show, through the alpha recurrence."""
import numpy as np

TU, TS, TN, TF = 2048, 2552, 2656, 196608
SIZE, BINS, OVR = 2048, 512, 4
PERIOD = 2048000 // 4                            # sample_reader.cpp:287, compared with a strict >
LOC_BEGIN, LOC_END = 64, 447                     # signalBeginIdx, signalEndIdx (spectrum_viewer.cpp:201-202), inclusive
ALPHA = {"slow": 0.01, "medium": 0.10, "fast": 1.00}     # spectrum_viewer.cpp:400-402
LIMITS0 = (-30.0, -90.0, -31.0, -50.0)           # dab_constants.h:100-101: Glob {Max, Min}, Loc {Max, Min}
BAR = 2e-5
DB_SLACK = 1e-4                                  # log10f's 2 ulp and the product's rounding below 128 dB: about 3e-5
F32 = np.float32
# What the float32 arithmetic of the limits adds on top of the rule's bound, which starts at 0 and stays below float32 resolution over the first
# shows: half a spacing of a float32 near -99 (the largest magnitude a limit takes) per operation -- the filter step is 3 operations and
# _calc_spectrum_display_limits at most 4 more (:129-135); yMin / yMax are 5 operations on top of the limits they are made of.
F32_HALF_STEP = abs(float(np.spacing(np.float32(-99.0)))) / 2.0          # 3.8e-6
LIMIT_SLACK = 7 * F32_HALF_STEP                  # 2.7e-5 dB
Y_SLACK = 12 * F32_HALF_STEP                     # 4.6e-5 dB
assert LOC_BEGIN == int(BINS * (1.0 - 1536000.0 / 2048000) / 2.0) and LOC_END == BINS - LOC_BEGIN - 1


def window():
    """glob_defs.h:252-266, literally"""
    a = (0.21557895, -0.41663158, 0.277263158, -0.083578947, 0.006947368)
    w = np.zeros(SIZE, np.float32)
    for i in range(SIZE):
        x = 0.0
        for j in range(5):
            x += a[j] * np.cos(j * i * 2.0 * np.pi / (SIZE - 1))
        w[i] = x
    return w


WINDOW = window()


# ------------------------------------------------------------------------------------------------ the row
def lin64(x):
    """mYValVec in float64 (:169-194): the window, the forward transform, the mean of |X| over the four bins of a display bin, the upper
    half of the transform first"""
    x = np.asarray(x, np.complex64).astype(np.complex128) * WINDOW.astype(np.float64)
    m = np.abs(np.fft.fft(x))
    y = np.zeros(BINS)
    for i in range(BINS // 2):
        y[BINS // 2 + i] = m[OVR * i:OVR * i + OVR].sum() / OVR
        y[i] = m[SIZE // 2 + OVR * i:SIZE // 2 + OVR * i + OVR].sum() / OVR
    return y


def val64(y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(y / BINS + float(F32(1.0e-6)))            # :207


def extrema(disp):
    """:196-218: strict comparisons from -1000 / +1000, in bin order; a NaN wins none -> [glob max, glob min, loc max, loc min]"""
    t = type(disp[0])
    gmax, gmin, lmax, lmin = t(-1000.0), t(1000.0), t(-1000.0), t(1000.0)
    for i, v in enumerate(disp):
        if v > gmax:
            gmax = v
        if v < gmin:
            gmin = v
        if LOC_BEGIN <= i <= LOC_END:
            if v > lmax:
                lmax = v
            if v < lmin:
                lmin = v
    return [gmax, gmin, lmax, lmin]


class Row64:
    """the display buffer of one SpectrumViewer in float64, with the bound every averaged value carries"""

    def __init__(self):
        self.disp = np.zeros(BINS)
        self.bound = np.zeros(BINS)

    def show(self, x):
        """-> (lin, val, disp, ext, per-bin bound of val, per-bin bound of disp)"""
        finite = np.isfinite(np.asarray(x, np.complex64).view(np.float32)).all()
        y = lin64(x) if finite else np.full(BINS, np.nan)
        v = val64(y)
        self.disp = self.disp + 0.2 * (v - self.disp)                    # :209
        b = db_bound(y) if finite else np.full(BINS, np.nan)
        self.bound = 0.8 * self.bound + 0.2 * b
        return y, v, self.disp.copy(), extrema(list(self.disp)), b, self.bound.copy()


def db_bound(y):
    """the bound of one un-averaged dB value, per bin"""
    return 20.0 * np.log10(1.0 + BAR * y.max() / (y + 1e-6 * BINS)) + DB_SLACK


def row32(x, disp, fft):
    """:169-218 in float32, line by line; fft = a float32 transform of 2048 complex64 (the oracle's).  disp [512] float32 in -> (lin, val, disp)
    |X| is sqrtf(re^2 + im^2), the stated deviation from std::abs."""
    x = np.asarray(x, np.complex64).copy()
    xr = x.view(np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        xr[:, 0] *= WINDOW
        xr[:, 1] *= WINDOW                                               # :169-172
        X = fft(x).view(np.float32).reshape(-1, 2)                       # :174
        m = np.sqrt(X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1])
        y = np.zeros(BINS, np.float32)
        for i in range(BINS // 2):
            f = F32(0)
            for j in range(OVR):
                f = F32(f + m[OVR * i + j])                              # :179-183
            y[BINS // 2 + i] = f / F32(OVR)
            f = F32(0)
            for j in range(OVR):
                f = F32(f + m[SIZE // 2 + OVR * i + j])                  # :187-191
            y[i] = f / F32(OVR)
        v = (F32(20.0) * np.log10(y / F32(BINS) + F32(1.0e-6))).astype(np.float32)      # :207
        d = (disp + F32(0.2) * (v - disp)).astype(np.float32)            # :209
    return y, v, d


VAL_OF_ZERO = F32(20.0) * np.log10(F32(0) / F32(BINS) + F32(1.0e-6))     # what every bin of a window of zeros gives, in float32


# ------------------------------------------------------------------------------------------------ the limits
def calc_limits32(mx, mn):
    """_calc_spectrum_display_limits (:112-139) in float32 -> (changed, Max, Min, the branches taken)"""
    lo, rng = F32(-99.0), F32(20.0)
    changed, br = False, []
    if mn < lo:
        changed, mn = True, lo
        br.append("min_below")
    if F32(mx - mn) < rng:
        changed = True
        mean = F32(F32(mx + mn) / F32(2))
        mn = F32(mean - F32(rng / F32(2)))
        mx = F32(mean + F32(rng / F32(2)))
        br.append("range_under_20")
        if mn < lo:
            mx = F32(mx + F32(lo - mn))
            mn = lo
            br.append("second_shift")
    return changed, mx, mn, br


def limits32(ext, lim, alpha, zoom):
    """ext = [glob max, glob min, loc max, loc min] of a show, lim = [Glob.Max, Glob.Min, Loc.Max, Loc.Min] -> (lim, yMin, yMax, valid, branches)"""
    a = F32(alpha)
    e = [F32(v) for v in ext]
    l = [F32(v) for v in lim]
    with np.errstate(all="ignore"):
        l = [F32(l[k] + F32(a * F32(e[k] - l[k]))) for k in range(4)]    # :220-223 (mean_filter, glob_defs.h:217-220)
        changed, l[0], l[1], br = calc_limits32(l[0], l[1])              # :226
        br = ["glob_" + b for b in br]
        if changed:
            _, l[2], l[3], b2 = calc_limits32(l[2], l[3])                # :229
            br += ["loc_" + b for b in b2] + ["loc_looked_at"]
        else:
            br.append("glob_unchanged")
        s = F32(F32(zoom) / F32(100.0))                                  # waterfall_scope.cpp:83
        one = F32(F32(1.0) - s)
        y_max = F32(F32(F32(l[0] + F32(5.0)) * one) + F32(l[2] * s))     # :57
        y_min = F32(F32(l[1] * one) + F32(l[3] * s))                     # :58
        valid = not (F32(y_max - y_min) <= F32(0))                       # :60
    return l, y_min, y_max, valid, br


def pixels(disp, y_min, y_max, dtype=np.float64):
    """waterfall_scope.cpp:73-74 -> (index [n] int, t * 255 [n])"""
    d = np.asarray(disp, dtype)
    with np.errstate(all="ignore"):
        t = (d - dtype(y_min)) / dtype(dtype(y_max) - dtype(y_min))
        t = np.where(t < 0, dtype(0), np.where(t > 1, dtype(1), t))
        t255 = (t * dtype(255.0)).astype(dtype)
    return np.where(np.isnan(t255), 0, np.nan_to_num(t255)).astype(np.int64), t255


def limits_table():
    """(ext, lim, what it reaches): every branch of :112-139"""
    return [
        ((-20.0, -80.0, -25.0, -60.0), LIMITS0, "nothing changes: Glob unchanged, Loc not looked at although its range is under 20"),
        ((-20.0, -200.0, -25.0, -60.0), (-30.0, -98.0, -31.0, -50.0), "Min below -99"),
        ((-50.0, -60.0, -52.0, -58.0), (-50.0, -60.0, -52.0, -58.0), "range under 20, no second shift; Loc recentred too"),
        ((-90.0, -98.0, -92.0, -97.0), (-90.0, -98.0, -92.0, -97.0), "range under 20 with the second shift, Glob and Loc"),
        ((-20.0, -150.0, -25.0, -150.0), (-30.0, -97.0, -31.0, -98.5), "Glob Min below -99, Loc Min below -99 as well"),
        ((-30.0, -90.0, -40.0, -45.0), (-30.0, -90.0, -40.0, -45.0), "Glob unchanged, so Loc is not looked at (range 5)"),
        ((-10.0, -95.0, -12.0, -120.0), (-10.0, -95.0, -12.0, -120.0), "Glob unchanged, Loc Min below -99 stays"),
        ((5.0, -30.0, 0.0, -20.0), LIMITS0, "a strong signal"),
        ((-1000.0, 1000.0, -1000.0, 1000.0), LIMITS0, "the extrema of a show whose every bin is a NaN"),
    ]


# ------------------------------------------------------------------------------------------------ the crafted windows
def _noise(seed, sigma):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(SIZE) + 1j * r.standard_normal(SIZE)) * (sigma / np.sqrt(2.0))).astype(np.complex64)


def _tone(fbin, amp=1.0):
    return (amp * np.exp(2j * np.pi * fbin * np.arange(SIZE) / SIZE)).astype(np.complex64)


def dab_symbol(seed, notch_db=30.0, lo=200, hi=400):
    """one OFDM symbol's useful part: QPSK on 1536 carriers, the carriers lo..hi (of the positive half) notch_db down"""
    r = np.random.default_rng(seed)
    X = np.zeros(SIZE, np.complex128)
    k = np.r_[1:769, SIZE - 768:SIZE]
    X[k] = (r.choice([-1.0, 1.0], k.size) + 1j * r.choice([-1.0, 1.0], k.size)) / np.sqrt(2.0)
    X[lo:hi] *= 10.0 ** (-notch_db / 20.0)
    return (np.fft.ifft(X) * np.sqrt(SIZE)).astype(np.complex64)


FLOOR = 3.0        # the noise under every tone: keeps every bin within 35 dB of the window's largest (the rule's condition; at 2.0 three
                   # tone windows had a largest bound of 0.012-0.014 dB and were moved: test_spectrum_cases.py, MOVED)


def windows():
    """-> list of (name, x [2048] complex64, why).  'zeros' and 'notch' are outside the condition of the comparison rule; 'nan' and 'inf' have
    exact expectations."""
    w = []
    w.append(("tone_bin_centre", _tone(4 * 100 + 1.5) + _noise(1, FLOOR), "a tone on the centre of display bin 356"))
    w.append(("tone_between_bins", _tone(777.37) + _noise(2, FLOOR), "a tone between two transform bins"))
    w.append(("tone_1023", _tone(1023) + _noise(3, FLOOR), "the seam of the half swap, its lower side: display bin 511"))
    w.append(("tone_1024", _tone(1024) + _noise(4, FLOOR), "the seam of the half swap, its upper side: display bin 0"))
    w.append(("tone_0", _tone(0) + _noise(5, FLOOR), "transform bin 0: display bin 256"))
    w.append(("dc_only", np.full(SIZE, 0.7 + 0.4j, np.complex64) + _noise(6, FLOOR), "a DC spur over the floor"))
    w.append(("zeros", np.zeros(SIZE, np.complex64), "every val is exactly 20 log10f(1e-6f)"))
    w.append(("noise_1e-5", _noise(7, 1e-5), "below the +1e-6 of :207"))
    w.append(("noise_1", _noise(8, 1.0), "white noise"))
    w.append(("noise_1e5", _noise(9, 1e5), "large values"))
    w.append(("notch", dab_symbol(10) + _noise(11, 0.003), "a DAB symbol with a 30 dB notch and the band edges"))
    q = _noise(12, 0.25)
    w.append(("u8_noise", ((np.clip(np.round(q.view(np.float32) * 128.0 + 127.5), 0, 255) - 127.5) / 128.0).astype(np.float32).view(np.complex64),
              "noise as a u8 ring holds it"))
    q = _noise(13, 0.1)
    w.append(("s16_noise", (np.clip(np.round(q.view(np.float32) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32).view(np.complex64),
              "noise as an s16 ring holds it"))
    x = _noise(14, 1.0)
    x[1234] = complex(np.nan, 0.0)
    w.append(("nan", x, "disp becomes NaN in every bin and stays, the extrema stay at -1000 / +1000"))
    x = _noise(15, 1.0)
    x[77] = complex(np.inf, 0.0)
    w.append(("inf", x, "inf - inf in the transform: NaN in every bin"))
    return w


def sequence():
    """six windows through one state, to walk the IIR: noise at changing gains with a tone coming and going"""
    g = (1.0, 3.0, 0.5, 10.0, 1.0, 0.1)
    return [(_noise(20 + k, g[k] * FLOOR) + (_tone(300.0 + k, 2.0 * g[k]) if k % 2 else 0)).astype(np.complex64) for k in range(6)]


IN_CONDITION = lambda name: name not in ("zeros", "notch", "nan", "inf")      # noqa: E731
EXACT_NAN = ("nan", "inf")


# ------------------------------------------------------------------------------------------------ the schedule
class Reader:
    """SampleReader's capture state, call by call: specBuffIdx, sampleCount (sample_reader.cpp:198-205, :285-296).  pos = samples consumed.
    shows = [(W, E)]: the window [W, W + 2048) was shown by the call that ended at E."""

    def __init__(self, pos=0):
        self.pos, self.W, self.idx, self.count, self.shows = pos, pos, 0, 0, []

    def get_samples(self, n, show):
        if self.idx < SIZE:                                              # :199-205
            self.idx += min(SIZE - self.idx, n)
        self.pos += n
        self.count += n                                                  # :285
        if self.count > PERIOD and show and self.idx >= SIZE:            # :287
            self.shows.append((self.W, self.pos))
            self.idx, self.count, self.W = 0, 0, self.pos                # :294-295

    def search(self, n):
        """n single-sample calls with iShowSpec true (sample_reader.cpp:96-99), without walking the ones that cannot show"""
        while n > 0:
            quiet = min(n, max(PERIOD - self.count, 0))                  # calls after which sampleCount is still <= 512 000
            if quiet:
                self.idx = min(SIZE, self.idx + quiet)
                self.pos += quiet
                self.count += quiet
                n -= quiet
            if n > 0:
                self.get_samples(1, True)
                n -= 1

    def frame(self, start):
        """behind a T_u block that correlated: the rest of symbol 0 (dab_processor.cpp:409), symbols 1..75 (:321), the null symbol (:270)"""
        if start:
            self.get_samples(start, False)
        for _ in range(75):
            self.get_samples(TS, True)
        self.get_samples(TN, False)


EV_SEEDED, EV_NO_DIP, EV_NO_END, EV_DIP_END, EV_CORR_FAILED, EV_CORR_OK, EV_FRAME_DONE = range(7)


def shows_of_trace(trace, enable_at=0):
    """The oracle receiver's event trace (ora_rx_enable_trace: kind, pos) through a Reader switched on at sample `enable_at` (a position at
    which the receiver stands between two calls) -> (shows [(W, E, frames decoded at E, what the stream was doing)], the position reached).
    Between the events: SEEDED closes the 20 T_u reads (dab_processor.cpp:141, no show); NO_DIP / NO_END / DIP_END close single-sample
    calls; CORR_FAILED / CORR_OK close the T_u block of :392; FRAME_DONE closes the rest of symbol 0, the 75 symbols and the null symbol:
    the symbol ends are FRAME_DONE.pos - 2656 - 2552 (75 - j)."""
    rd, p, frames, out = None, 0, 0, []

    def piece(fn, end, what, fr):
        nonlocal rd, p
        if rd is None and p >= enable_at:
            assert p == enable_at, (p, enable_at)
            rd = Reader(p)
        if rd is None:
            p = end
            return
        k = len(rd.shows)
        fn(rd)
        assert rd.pos == end, (rd.pos, end)
        out.extend((W, E, fr, what) for W, E in rd.shows[k:])
        p = end

    for ev in trace:
        kind, pos = int(ev["kind"]), int(ev["pos"])
        if kind == EV_SEEDED:
            piece(lambda r: [r.get_samples(TU, False) for _ in range((pos - p) // TU)], pos, "seed", frames)
        elif kind in (EV_NO_DIP, EV_NO_END, EV_DIP_END):
            piece(lambda r: r.search(pos - p), pos, "search", frames)
        elif kind in (EV_CORR_FAILED, EV_CORR_OK):
            assert pos - p == TU
            piece(lambda r: r.get_samples(TU, False), pos, "block", frames)
        else:
            start = pos - p - 75 * TS - TN
            assert 0 <= start < TU
            piece(lambda r: r.frame(start), pos, "frame", frames)
            frames += 1
    return out, p


# ------------------------------------------------------------------------------------------------ the engine test's signals
ENGINE_FRAMES = 14                               # ensemble frames per stream
ENGINE_PREFIX = int(2.9 * TF)                    # noise in front of stream 2's signal: more than 512 001 samples of search
ENGINE_FAIL_FRAME = 5                            # stream 2: this frame's phase reference symbol is noise, the lock is lost and regained


def engine_float_signals():
    """Three streams: 0 clean; 1 with an echo 300 samples late and 6 dB down and a carrier offset; 2 behind 2.9 frames of noise (the first
    window is shown while it searches) and with a drop-out over one phase reference symbol."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    from tools import dab_synth as ds
    import oracle_lib as ol
    subch = ds.default_subchannels(1, 64)
    ens = ds.build_ensemble(20, subch, seed=70)
    x0 = ds.channel(ens.iq, snr_db=25.0, cfo_hz=0.0, timing_offset=3001, seed=1, n_out=ENGINE_FRAMES * TF)
    x1 = ds.channel(ens.iq, snr_db=22.0, cfo_hz=310.0, timing_offset=911, seed=2, n_out=ENGINE_FRAMES * TF + 999)
    x1[300:] += np.complex64(0.5) * x1[:-300].copy()
    a = ds.channel(ens.iq, snr_db=25.0, cfo_hz=-120.0, timing_offset=4243, seed=3, n_out=ENGINE_FRAMES * TF)
    sym0 = ol.oracle_run(a, [], front=1)["sym0"]
    rng = np.random.default_rng(1)
    lvl = float(np.sqrt(np.mean(np.abs(a) ** 2)))
    noise = lambda n: (lvl * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)   # noqa: E731
    p = int(sym0[ENGINE_FAIL_FRAME])
    a[p - 504:p + TU] = noise(504 + TU)
    return [x0, x1, np.concatenate([noise(ENGINE_PREFIX), a])]


def to_ring(x, kind):
    """-> (what is pushed into a ring of this format, the float samples those stand for)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    from tools import iq_files as iqf
    if kind == "cf32":
        return x, x
    g = 0.25 / np.sqrt(np.mean(np.abs(x) ** 2))
    codes = iqf.to_u8(x, g) if kind == "u8" else iqf.to_int(x, 16, g).astype(np.int16)
    c = codes.astype(np.float32)
    v = (c - np.float32(127.38)) / np.float32(128) if kind == "u8" else c / np.float32(32768)
    return np.ascontiguousarray(codes), np.ascontiguousarray(v).view(np.complex64)


def engine_schedule(vals, enable_at=0):
    """the shows of one stream from the oracle receiver's trace of its (quantised) samples, and whether a search candidate's correlation failed"""
    import oracle_lib as ol
    tr = ol.oracle_trace(vals)
    kinds = [int(e["kind"]) for e in tr]
    search_fails = sum(1 for k in range(1, len(kinds)) if kinds[k] == EV_CORR_FAILED and kinds[k - 1] == EV_DIP_END)
    shows, end = shows_of_trace(tr, enable_at)
    return shows, end, search_fails, tr


def looks_of_trace(trace, look, enable_at=0):
    """The oracle receiver's event trace as a sequence of front-end steps, each ending in one look of k_spectrum (`look` =
    dabstar_amd.lib.spectrum_look): what the search (k_acquire) and the frame head leave behind them -- read position, state, failed-correlation
    count, frame_ok, sym0_pos.  A step out of lock: one pass of the search, which goes on behind a candidate whose correlation failed and ends
    where time_sync gives up (NO_DIP / NO_END) or a candidate correlates; then the head begins that frame.  A step in lock: the head
    correlates the T_u block and begins a frame or fails.  -> [(E, inexact, frames decoded)] of the looks that showed."""
    ev = [(int(e["kind"]), int(e["pos"])) for e in trace]
    walk, out = None, []
    state, rd, lost, frames, i = 0, 0, 0, 0, 0                      # ST_INIT

    def one(frame_ok, sym0_pos):
        nonlocal walk
        if walk is None:
            return
        E, inexact, walk = look(walk, rd, state, lost, frame_ok, sym0_pos)
        if E is not None:
            out.append((E, inexact, frames))

    def frame_end(k):
        """the FRAME_DONE behind the CORR_OK at index k -> (its index, start index of the frame) or None if the samples ran out"""
        if k + 1 < len(ev) and ev[k + 1][0] == EV_FRAME_DONE:
            return k + 1, ev[k + 1][1] - ev[k][1] - 75 * TS - TN
        return None

    while i < len(ev):
        if walk is None and rd >= enable_at:
            assert rd == enable_at
            walk = [rd, rd, lost, state]
        if state != 2:                                              # the search's pass
            begun = None
            while i < len(ev):
                kind, pos = ev[i]
                if kind == EV_SEEDED:
                    i += 1
                    continue
                if kind in (EV_NO_DIP, EV_NO_END):
                    rd, state, i = pos, 1, i + 1
                    break
                assert kind == EV_DIP_END
                D = pos
                k2, p2 = ev[i + 1] if i + 1 < len(ev) else (None, None)
                if k2 == EV_CORR_FAILED:
                    rd, lost, state, i = p2, lost + 1, 1, i + 2
                    continue                                        # straight back to the search, in the same pass
                rd, state = D, 2
                fe = frame_end(i + 1) if k2 == EV_CORR_OK else None
                if fe is None:
                    i = len(ev)
                    break
                begun = (D + fe[1], fe[0])
                break
            if begun is None:
                one(0, 0)
            else:
                one(1, begun[0])
                rd, frames, i = ev[begun[1]][1], frames + 1, begun[1] + 1
        else:                                                       # the head of a stream in lock
            kind, pos = ev[i]
            if kind == EV_CORR_FAILED:
                rd, lost, state, i = pos, lost + 1, 1, i + 1
                one(0, 0)
            else:
                assert kind == EV_CORR_OK
                fe = frame_end(i)
                if fe is None:
                    break
                one(1, rd + fe[1])
                rd, frames, i = ev[fe[0]][1], frames + 1, fe[0] + 1
    return out


def trace_of(events):
    """a hand-made trace: [(kind, pos)]"""
    t = np.zeros(len(events), np.dtype([("kind", "<i4"), ("pos", "<i8")]))
    for k, (kind, pos) in enumerate(events):
        t[k] = (kind, pos)
    return t
