"""Crafted IQ for the frame chain (k_frame_head -> k_symbols_persistent -> k_frame_tail, csrc/pipeline.hip), a float64 model of what the
chain computes, and the plan of which stream of which engine carries what.  No device anywhere in this file: tests/test_front_cases.py
proves the inputs and the model on the oracle alone, tests/test_gpu_front_stage.py holds the device to the model.

A STREAM is a noise-free real ensemble (three frames in lock, one frame behind) with four CRAFTED frames in between: the null symbol and
the phase reference symbol of a crafted frame stay, symbols 1..75 are the test's own samples, spliced in after the channel model (and, for
the native rings, in the ring's own codes), so that the values are exact.  Families:
  steer    every symbol's cyclic prefix is its tail turned so that the summed correlation has the phase theta (fine-CFO clamp, atan2 at +-pi)
  zero     zeros but for impulses that have no partner one T_u away: all 75 correlations are exactly 0
  impulse  zeros but for samples (3+4j) 2^a and (1+2j) 2^b at the edges of the kernel's access classes: every product and sum is exact
  white    every sample distinct (Gaussian; uniform codes over the whole range for the native rings)
and after two of the crafted frames the null symbol is replaced by noise of amplitude 0.1, so that the noise power and the TII sum carry
its transform.  Each stream's timing offset puts the boundary of a two-frame ring at one chosen frame-relative PLACE (PLACES below) in
two of its crafted frames.

The MODEL (model_frame) is numpy, complex128: the samples as the ring holds them, mixed with e^{j 2 pi phase / 2 048 000} where phase is
the integer oscillator chain, np.fft.fft of each window; positions, frequencies and phases come from the oracle's capture alone."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as ol

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from tools import dab_synth as ds  # noqa: E402

TU, TG, TS, TN, TF, K, FS = 2048, 504, 2552, 2656, 196608, 1536, 2048000
assert (ds.TU, ds.TG, ds.TS, ds.TN, ds.TF) == (TU, TG, TS, TN, TF)
N_LOCK, N_CRAFT = 3, 4                                   # frames in lock (start index = T_g) in front of the crafted ones; one frame behind them
RING = 2 * TF                                            # ring_frames = 2
KINDS = ("cf32", "s16", "u8")

# carrier offsets: the first seven are the issue's (two of them next to the 35 kHz reset of f_sync); the others sit in the middle of the
# four quadrant ranges of |f| mod 1000, both signs, for the zero-correlation frames
OFFSETS = (0.0, 1234.5, -1234.5, 1600.0, -1600.0, 33000.0, -34900.0, 1125.0, -1125.0, 1375.0, -1375.0, 1625.0, -1625.0, 1875.0, -1875.0, 640.0)
THETAS = (0.0, 19.9, -19.9, 20.1, -20.1, 90.0, -90.0, 179.99, -179.99, 45.0)      # degrees; -179.99 = 180 + 0.01
ORDERS = (("steer", "zero", "impulse", "white"), ("steer", "white", "zero", "impulse"))
NULL_AFTER = (0, 2)                                      # crafted frames (by order index) whose null symbol is crafted too

# ---- the places of the ring boundary, relative to the first sample of the T_u part of symbol 0 (sym0) --------------------------------
# k_symbols_persistent: block g of G walks symbols g, g + G, ...; symbols 7, 37 and 67 (0-based) are first, middle and last of their
# block for G = 25 (blocks of 3) and G = 15 (blocks of 5) alike
SYMS = (("first", 7), ("middle", 37), ("last", 67))
IN_SYM = (("sym_first", 0), ("sym_second", 1), ("prefix_247|248", 248), ("prefix_503|504", 504), ("partner", TU + 100),
          ("window_x256", TG + 3 * 256), ("window_x256+1", TG + 3 * 256 + 1))
PLACES = [("head_sample0", -TG), ("head_sample1024", -TG + 1024), ("head_overlap", -TG + TU + 100)]
PLACES += [("%s@%s" % (n, w), TU + l0 * TS + j) for w, l0 in SYMS for n, j in IN_SYM]
PLACES += [("null_guard", TU + 75 * TS + 100), ("null_window", TU + 75 * TS + TG + 1000), ("null_tail", TU + 75 * TS + TG + TU + 50)]
# one block per symbol (G = 75): first, middle and last are the same thing
PLACES_G75 = PLACES[:3] + [p for p in PLACES if p[0].endswith("@middle")] + PLACES[-3:]


def grid_of(n_streams):
    """blocks per stream of the k_symbols launch (sym_blocks_per_stream, csrc/pipeline.hip)"""
    return 15 if n_streams >= 48 else (25 if n_streams >= 16 else 75)


# (n_streams, ring kind, variant): the engines the GPU test runs.  A variant moves the plan on by n_streams streams, so that the engines
# of one grid shape together reach every place.
CASES = [(3, "cf32", 0), (3, "s16", 1), (3, "cf32", 2), (3, "u8", 3), (3, "cf32", 4),
         (16, "cf32", 0), (16, "s16", 1), (16, "u8", 0),
         (48, "cf32", 0), (48, "s16", 0)]


def stream_plan(n_streams, variant, s):
    places = PLACES_G75 if grid_of(n_streams) == 75 else PLACES
    i = variant * n_streams + s
    cfo, theta = OFFSETS[i % len(OFFSETS)], THETAS[i % len(THETAS)]
    if cfo < -34800.0:
        # 100 Hz from the reset: four clamped steps down would cross it, f_sync would go to 0 and the lock would be lost (dab_processor.cpp:
        # 205-224).  The steered frame steps UP by a full clamp, so that the three frames behind it cannot reach -35 kHz
        theta = 20.1
    return dict(index=i, cfo=cfo, theta=theta, order=ORDERS[(i // 2) % 2], cif_start=4 * ((i // 3) % 2),
                place=places[i % len(places)], seed=1000 + i)


# ---- codes and values ---------------------------------------------------------------------------------------------------------------
def values(codes, kind):
    """the float of each code by ring_fmt.h's two maps (float32 arithmetic, one rounding per operation); cf32: the samples themselves"""
    if kind == "cf32":
        return np.ascontiguousarray(codes, np.complex64)
    c = np.ascontiguousarray(codes).astype(np.float32)
    v = (c - np.float32(127.38)) / np.float32(128) if kind == "u8" else c / np.float32(32768)
    return np.ascontiguousarray(v).view(np.complex64)


def to_codes(z, kind):
    """complex values -> the ring's codes (interleaved I, Q), rounded to the nearest code and clipped"""
    z = np.asarray(z, np.complex128)
    if kind == "cf32":
        return z.astype(np.complex64)
    iq = np.empty(2 * len(z))
    iq[0::2], iq[1::2] = z.real, z.imag
    if kind == "s16":
        return np.clip(np.rint(iq * 32768.0), -32768, 32767).astype(np.int16)
    return np.clip(np.rint(iq * 128.0 + 127.38), 0, 255).astype(np.uint8)


def _put(codes, kind, pos, seg):
    if kind == "cf32":
        codes[pos:pos + len(seg)] = seg
    else:
        codes[2 * pos:2 * pos + len(seg)] = seg


# ---- the crafted symbols (75 x 2552 samples, as codes) --------------------------------------------------------------------------------
PREFIX_EDGES = (0, 247, 248, 255, 256, 503)              # first / second prefix sample of a thread, the last thread that has two, ...
WINDOW_EDGES = (504, 759, 760, 2551)
IMP_A, IMP_B = (3 + 4j) / 32.0, (1 + 2j) / 64.0          # s16: codes (3072, 4096) and (512, 1024); |A| = 5 / 32 exactly


def impulse_positions(l0):
    """{sample of symbol l0 (0-based): value}: two prefix samples with their partners one T_u later, and one window sample; symbol 74 has no
    partner pair at all"""
    out = {}
    if l0 != 74:
        for p in (PREFIX_EDGES[l0 % 6], PREFIX_EDGES[(l0 + 3) % 6]):
            out[p] = IMP_A
            out[p + TU] = IMP_B
    w = WINDOW_EDGES[l0 % 4]
    if w not in out and (w - TU) not in out:
        out[w] = IMP_A
    return out


def zero_positions(l0):
    """impulses without partners: a prefix sample whose partner is zero, a partner whose prefix sample is zero, one window sample"""
    p, q = PREFIX_EDGES[l0 % 6], PREFIX_EDGES[(l0 + 2) % 6]
    return {p: IMP_A, q + TU: IMP_B, 600 + 17 * l0: -IMP_A}


def _sparse(kind, positions):
    z = np.zeros((75, TS), np.complex128)
    for l0 in range(75):
        for p, v in positions(l0).items():
            z[l0, p] = v
    if kind == "u8":                                     # (code 127 is the nearest to zero, -0.003: nothing is exact in a u8 ring)
        z = np.where(z == 0, (127 - 127.38) / 128.0 * (1 + 1j), z * 8)
    return to_codes(z.reshape(-1), kind)


def craft_symbols(family, kind, rng, theta_deg=0.0, f=0):
    n = 75 * TS
    if family == "impulse":
        return _sparse(kind, impulse_positions)
    if family == "zero":
        return _sparse(kind, zero_positions)
    if family == "white":
        if kind == "cf32":
            return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (0.25 / np.sqrt(2))).astype(np.complex64)
        lo, hi = (-32768, 32768) if kind == "s16" else (0, 256)
        c = rng.integers(lo, hi, 2 * n).astype(np.int16 if kind == "s16" else np.uint8)
        c[0:4] = [lo, hi - 1, hi - 1, lo]                # the extreme codes, at a symbol's first samples ...
        c[2 * TS - 4:2 * TS] = [hi - 1, lo, lo, hi - 1]  # ... and at its last
        return c
    assert family == "steer"
    # the reference correlates MIXED samples: x'[Tu+i] conj(x'[i]) = x[Tu+i] conj(x[i]) e^{-j 2 pi f Tu / fs}, and f Tu / fs = f / 1000
    rot = np.exp(-1j * np.deg2rad(theta_deg)) * np.exp(-2j * np.pi * (f % 1000) / 1000.0)
    z = (rng.standard_normal((75, TS)) + 1j * rng.standard_normal((75, TS))) * (0.2 / np.sqrt(2))
    tail = values(to_codes(z[:, TU:].reshape(-1), kind), kind).astype(np.complex128).reshape(75, TG)    # the tail as the ring will hold it
    z[:, TU:] = tail
    z[:, :TG] = tail * rot
    return to_codes(z.reshape(-1), kind)


def rotate_prefix(seg, kind, m):
    """the 75 cyclic prefixes times j^m, in the ring's own codes (the negative of a code: -c, 32767 for -32768, 255 - c for u8): turns the
    summed correlation by (-j)^m and keeps every sample a code"""
    if m % 4 == 0:
        return seg
    c = (np.stack([seg.real, seg.imag], -1) if kind == "cf32" else seg.reshape(-1, 2)).reshape(75, TS, 2).copy()

    def neg(a):
        if kind == "cf32":
            return -a
        return (255 - a.astype(np.int64)).astype(np.uint8) if kind == "u8" else np.clip(-a.astype(np.int64), -32768, 32767).astype(np.int16)
    i, q = c[:, :TG, 0].copy(), c[:, :TG, 1].copy()
    c[:, :TG, 0], c[:, :TG, 1] = ((neg(q), i), (neg(i), neg(q)), (q, neg(i)))[m % 4 - 1]
    return (c[..., 0] + 1j * c[..., 1]).astype(np.complex64).reshape(-1) if kind == "cf32" else c.reshape(-1)


def summed_correlation(seg, kind, f):
    """what the reference sums over the 75 symbols of a crafted segment mixed with the integer frequency f (float64)"""
    x = values(seg, kind).astype(np.complex128).reshape(75, TS)
    return np.sum(x[:, TU:] * np.conj(x[:, :TG])) * np.exp(-2j * np.pi * (f % 1000) / 1000.0)


def fine_step(corr):
    """the fine-CFO step in Hz the reference takes on that sum (dab_processor.cpp:236-242, :366)"""
    return float(np.clip(np.degrees(np.arctan2(corr.imag, corr.real)), -20.0, 20.0)) / 360.0 * 1000.0


def craft_null(kind, rng):
    return to_codes((rng.standard_normal(TN) + 1j * rng.standard_normal(TN)) * (0.1 / np.sqrt(2)), kind)


# ---- one stream ---------------------------------------------------------------------------------------------------------------------
_ENS = {}


def _ensemble(cif_start):
    if cif_start not in _ENS:
        _ENS[cif_start] = ds.build_ensemble(5, [], seed=77, cif_start=cif_start)
    return _ENS[cif_start]


def _oracle(vals, front, frames=None):
    r = ol.oracle_run(vals, [], trace=256, front=front, front_frames=frames)
    done = r["trace"][r["trace"]["kind"] == ol.EV_FRAME_DONE]
    r["correction"] = done["ratio"].astype(np.int64)     # what the coarse search returned, per frame (0 where it did not run)
    return r


def timing_for(place_rel):
    """the cyclic timing offset that puts sample sym0 + place_rel of every frame on a multiple of T_F (sym0 = offset + T_n + T_g mod T_F),
    hence on the ring's boundary in every other frame"""
    return (-place_rel - TN - TG) % TF


def build_stream(n_streams, kind, variant, s, spectra=True):
    """-> dict(plan, kind, codes (what is pushed), vals (complex64, what the ring holds), ora (the oracle's capture on vals), families
    {frame: family}, null_crafted {frame}, wrap {frame: (place name, frame-relative sample)} for the crafted frames the boundary falls in)"""
    plan = stream_plan(n_streams, variant, s)
    rng = np.random.default_rng(plan["seed"])
    ens = _ensemble(plan["cif_start"])
    t = timing_for(plan["place"][1])
    x = ds.channel(ens.iq, snr_db=300.0, cfo_hz=plan["cfo"], timing_offset=t, seed=plan["seed"], n_out=14 * TF)
    codes = to_codes(x, kind)
    base = _oracle(values(codes, kind), 1)
    # the coarse search needs one to four frames to settle (start index 504 from then on); three frames in lock, then the crafted ones
    settled = next(k for k in range(base["n"]) if np.all(base["start"][k:] == TG))
    first = settled + N_LOCK
    crafted = tuple(range(first, first + N_CRAFT))
    n_frames = first + N_CRAFT + 1
    assert base["n"] >= n_frames, (plan, base["n"], base["start"])
    sym0 = base["sym0"].astype(np.int64)
    n_keep = int(sym0[n_frames - 1]) + TF + 2 * TU + 1000   # the last frame whole, and what a frame head wants to see beyond it (T_F + 2 T_u)
    codes = codes[:n_keep] if kind == "cf32" else codes[:2 * n_keep]
    families, null_crafted = {}, set()
    # The frequency each crafted frame will be mixed with is predicted: the oracle is causal, so the first one's is what the base run gave,
    # and every later one follows from the step the frame before it provokes.  A fine-CFO error beyond some 100 Hz moves the first
    # correlation peak above the threshold (the start index leaves 504), so every frame behind the steered one has its prefixes turned by
    # the multiple of 90 degrees that steps the frequency BACK towards the carrier: the drift never exceeds one clamp (55.6 Hz).
    f_pred, drift = float(base["fbb"][first]), 0.0
    for c, fam in enumerate(plan["order"]):
        k = first + c
        f = int(np.floor(abs(f_pred) + 0.5) * np.sign(f_pred))                     # roundf
        seg = craft_symbols(fam, kind, rng, plan["theta"], f)
        corr = summed_correlation(seg, kind, f)
        if fam != "steer" and corr != 0:
            want = 1j if drift <= 0 else -1j
            m = max(range(4), key=lambda m: (corr * (-1j) ** m / want).real)
            seg = rotate_prefix(seg, kind, m)
            corr = summed_correlation(seg, kind, f)
        if corr != 0:
            f_pred += fine_step(corr)
            drift += fine_step(corr)
        _put(codes, kind, int(sym0[k]) + TU, seg)
        families[k] = fam
        if c in NULL_AFTER:
            _put(codes, kind, int(sym0[k]) + TU + 75 * TS, craft_null(kind, rng))
            null_crafted.add(k)
    vals = values(codes, kind)
    ora = _oracle(vals, 2 if spectra else 1, crafted)
    wrap = {}
    for k in crafted:
        if k < ora["n"] and (int(ora["sym0"][k]) + plan["place"][1]) % RING == 0:
            wrap[k] = plan["place"]
    return dict(plan=plan, kind=kind, codes=codes, vals=vals, ora=ora, base_sym0=sym0, families=families, null_crafted=null_crafted, wrap=wrap,
                timing=t, crafted=crafted, n_frames=n_frames)


_CASES = {}


def warm_up():
    """before any thread: the oracle is loaded, its oscillator table (built by the first receiver) and the two ensembles exist"""
    L = ol.oracle()
    L.ora_rx_destroy(L.ora_rx_create(ol.make_descs([]), 0))
    _ensemble(0), _ensemble(4)


def build_case(n_streams, kind, variant, spectra=True):
    key = (n_streams, kind, variant, spectra)
    if key not in _CASES:
        warm_up()
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            _CASES[key] = list(pool.map(lambda s: build_stream(n_streams, kind, variant, s, spectra), range(n_streams)))
    return _CASES[key]


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _mix(x, phase):
    return x * np.exp(2j * np.pi * (np.asarray(phase, np.int64) % FS) / FS)


def model_frame(vals, ora, k):
    """Frame k of the oracle's capture `ora` on ring values `vals`, in complex128.  phase_ref [2048], spec [75, 2048] and null [2048] in
    FFT bin order; cp [75] = sum x[Tu+i] conj(x[i]), i < 504, on the RAW samples (as k_symbols_persistent sums them), cp_abs [75] the same
    sum of moduli; abs [75] = sum |x| over a symbol's 2552 samples, nnz [75] its non-zero samples; phase_end the chain after the null symbol."""
    sym0, ph1, f, f2 = int(ora["sym0"][k]), int(ora["phase_sym1"][k]), int(ora["f_sym"][k]), int(ora["f_null"][k])
    f0 = int(ora["f_null"][k - 1])                       # symbol 0 was read with the frequency the previous frame ended on
    j = np.arange(TU, dtype=np.int64)
    # the oscillator steps BEFORE it is used (sample_reader.cpp:274-281): ph1 is the phase of symbol 0's last sample
    phase_ref = np.fft.fft(_mix(vals[sym0:sym0 + TU].astype(np.complex128), ph1 + f0 * (TU - 1 - j)))
    base = sym0 + TU
    x = vals[base:base + 75 * TS].astype(np.complex128).reshape(75, TS)
    n = np.arange(75 * TS, dtype=np.int64).reshape(75, TS)
    spec = np.fft.fft(_mix(x, ph1 - f * (n + 1))[:, TG:], axis=1)
    cp = np.sum(x[:, TU:] * np.conj(x[:, :TG]), axis=1)
    cp_abs = np.sum(np.abs(x[:, TU:]) * np.abs(x[:, :TG]), axis=1)
    nb = base + 75 * TS
    xn = vals[nb:nb + TN].astype(np.complex128)
    jn = np.arange(TN, dtype=np.int64)
    ph_null = ph1 - f * 75 * TS - f2 * (jn + 1)
    null = np.fft.fft(_mix(xn, ph_null)[TG:TG + TU])
    return dict(phase_ref=phase_ref, spec=spec, null=null, cp=cp, cp_abs=cp_abs, abs=np.sum(np.abs(x), axis=1), nnz=np.sum(x != 0, axis=1),
                phase_end=int(ph_null[-1] % FS), phase_sym1_chain=None if k == 0 else
                int((int(ora["phase_end"][k - 1]) - f0 * (int(ora["start"][k]) + TU)) % FS))


def carrier_bins():
    """carrier k of the engine's spectra -> FFT bin (the oracle's frequency interleaver table)"""
    p16 = np.zeros(K, np.int16)
    ol.oracle().ora_freq_interleaver(p16)
    return p16.astype(np.int64) % TU


def quadrant(f):
    """(sign of f, quadrant 0..3 of |f| mod 1000): what decides the signs of cos and sin of k_frame_tail's rotation by e^{-j 2 pi f Tu / fs}"""
    return (1 if f >= 0 else -1, (abs(int(f)) % 1000) // 250)
