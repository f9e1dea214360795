"""The frame chain k_frame_head -> k_symbols_persistent -> k_frame_tail (csrc/pipeline.hip) on crafted IQ, read back through
dx.front_read (the library's internal test entry: plain copies, no kernel) and held to the float64 model of tests/front_cases.py.

Engines of 3, 16 and 48 streams (k_symbols grids of 75, 25 and 15 blocks per stream: one, three and five symbols per persistent block),
two-frame rings fed between process(1) calls, cf32, s16 and u8 rings.  Every stream carries four crafted frames (steered, zero-correlation,
impulse, white; two crafted null symbols) and has the ring's boundary at one chosen place of two of them; tests/test_front_cases.py proves
without a device that the inputs are what they are named for and that the model equals the oracle to 4e-7.

Per stream and frame the device must give
  integers    sym0_pos, start_index, correction, f_frame, phase_sym1, nco_phase equal to the oracle's; clock_err bit-equal
  frequency   f_bb within 0.05 Hz of the oracle's; on a zero-correlation frame phase_offs = 0 and a step of exactly 0.0, as the oracle
  spectra     phase_ref and the 75 spectra within 2e-6 max|X_model| of that symbol (the bound of test_fft_matches_oracle_dft)
  cp_part     equal to the model where every term is exact (impulse and zero frames, cf32 and s16); else within 506 2^-24 sum |x[Tu+i]| |x[i]|
  abs_part    relative error at most 2 * 2^-24 (non-zero samples + 2)
  noise power |d| <= 0.05 (2 |X| delta + delta^2) + 4 * 2^-24 max(old, new), delta the spectrum bound (null_power_next); unchanged on TII frames
  TII sum     within delta (+ one rounding of the sum) per accumulated symbol
and a native-ring engine's read-back equals, bit for bit, that of a cf32 engine fed the floats of the same codes (ring_fmt.h).

The null-symbol checks follow the branch k_frame_tail took (told by the counter of summed null symbols), and that branch is held to the
oracle's is_tii under its own name: it is the FIC stage's CIF count, so a stream whose demapper or FIC decoder parts from the oracle shows
there and nowhere else.  (It did: a phase reference bin that the float transform cancels to exactly (0, 0) used to put a NaN into the
demapper for good -- stream 5 of the 16- and 48-stream cf32 cases; docs/history/front_stage_tests.md.)"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import front_cases as fc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -24
SPEC_REL = 2e-6
K_MIN_NOISE = np.float32(1.0 / 32767.0) * np.float32(1.0 / 32767.0)
USED_BINS = np.r_[1:fc.K // 2 + 1, fc.TU - fc.K // 2:fc.TU]


def run_engine(streams, ring_kind):
    """The streams through one engine with a two-frame ring of `ring_kind` (a cf32 ring takes the floats of the codes).  Samples are pushed
    between process(1) calls, as much as the ring has room for.  -> per stream {frame: dx.front_read after the step that finished it}."""
    S = len(streams)
    data = [st["codes"] if ring_kind != "cf32" else st["vals"] for st in streams]
    per = [1 if ring_kind == "cf32" else 2 for _ in streams]
    total = [len(st["vals"]) for st in streams]
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=0, fic_only=True, out_frames=4, ring_format=ring_kind)
    got = [{} for _ in range(S)]
    try:
        pos, used, frames, idle = [0] * S, [0] * S, [0] * S, 0
        while idle < 4 and any(frames[s] < streams[s]["n_frames"] for s in range(S)):
            for s in range(S):
                m = min(fc.RING - (pos[s] - used[s]), total[s] - pos[s])
                if m > 0:
                    eng.push_iq(s, data[s][per[s] * pos[s]:per[s] * (pos[s] + m)])
                    pos[s] += m
            eng.process(1)
            idle += 1
            for s in range(S):
                st = eng.stats(s)
                if st["samples_consumed"] != used[s]:
                    used[s], idle = st["samples_consumed"], 0
                if st["frames"] > frames[s]:
                    assert st["frames"] == frames[s] + 1, (s, st["frames"], frames[s])
                    frames[s] = st["frames"]
                    k = frames[s] - 1
                    if k < streams[s]["n_frames"]:
                        got[s][k] = dx.front_read(eng, s, spectra=k in streams[s]["crafted"])
        assert all(frames[s] >= streams[s]["n_frames"] for s in range(S)), frames
    finally:
        eng.close()
    return got


class Figures:
    """largest value / bound per check, printed before anything is asserted; failures by (stream, frame, what)"""

    def __init__(self):
        self.worst, self.bad = {}, []

    def check(self, what, where, err, bound):
        err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        w = float(np.max(ratio)) if ratio.size else 0.0
        if w > self.worst.get(what, (-1.0, None))[0]:
            self.worst[what] = (w, where)
        if w > 1.0:
            self.bad.append((what, where, w))

    def merge(self, other):
        for what, (w, where) in other.worst.items():
            if w > self.worst.get(what, (-1.0, None))[0]:
                self.worst[what] = (w, where)
        self.bad += other.bad

    def equal(self, what, where, a, b):
        if not np.array_equal(a, b):
            self.bad.append((what, where, a if np.ndim(a) == 0 else "arrays differ", b if np.ndim(b) == 0 else ""))


def check_stream(fig, s, st, got, bins):
    o, kind = st["ora"], st["kind"]
    for k in range(st["n_frames"]):
        assert k in got, (s, k, sorted(got))
        g, w = got[k], (s, k, st["families"].get(k, "real"))
        for name, want in (("frame_ok", 1), ("frames", k + 1), ("sym0_pos", int(o["sym0"][k])), ("start_index", int(o["start"][k])),
                           ("correction", int(o["correction"][k])), ("f_frame", int(o["f_sym"][k])), ("phase_sym1", int(o["phase_sym1"][k])),
                           ("nco_phase", int(o["phase_end"][k])), ("rd", int(o["sym0"][k]) + fc.TU + 75 * fc.TS + fc.TN)):
            fig.equal(name, w, g[name], want)
        fig.equal("clock_err bits", w, np.float32(g["clock_err"]).tobytes(), np.float32(o["clock_err"][k]).tobytes())
        fig.check("f_bb [0.05 Hz]", w, abs(float(g["f_bb"]) - float(o["fbb_end"][k])), 0.05)
        fig.equal("f_sync = f_bb", w, np.float32(g["f_sync"]), np.float32(g["f_bb"]))
    for k in st["crafted"]:
        g, prev, fam = got[k], got[k - 1], st["families"][k]
        w = (s, k, fam)
        m = fc.model_frame(st["vals"], o, k)
        # ---- fine CFO on an exactly-zero correlation: no step, as the oracle (whose step on these frames is exactly 0.0)
        if fam == "zero" and kind != "u8":
            assert o["fbb_end"][k] == o["fbb"][k] and not o["fc"][k].any()
            fig.equal("zero correlation: phase_offs", w, float(g["phase_offs"]), 0.0)
            corr = int(o["correction"][k])
            fig.equal("zero correlation: f_bb steps by exactly 0.0", w, np.float32(g["f_bb"]),
                      np.float32(np.float32(prev["f_bb"]) + np.float32(corr if corr != 100000 else 0)))
            if np.float32(prev["f_bb"]) == np.float32(o["fbb_end"][k - 1]):
                fig.equal("zero correlation: f_bb = the oracle's", w, np.float32(g["f_bb"]), np.float32(o["fbb_end"][k]))
        # ---- spectra
        mx0 = np.abs(m["phase_ref"]).max()
        fig.check("phase_ref", w, np.abs(g["phase_ref"].astype(np.complex128) - m["phase_ref"]), SPEC_REL * mx0)
        mx = np.abs(m["spec"]).max(axis=1)
        fig.check("spectra", w, np.abs(g["spectra"].astype(np.complex128) - m["spec"][:, bins]), (SPEC_REL * mx)[:, None])
        # ---- per-symbol sums
        cp = g["cp_part"].astype(np.complex128)
        if fam in ("impulse", "zero") and kind != "u8":
            assert np.array_equal(m["cp"].astype(np.complex64).astype(np.complex128), m["cp"])            # every term and sum is a float
            fig.equal("cp_part (exact)", w, g["cp_part"], m["cp"].astype(np.complex64))
        fig.check("cp_part", w, np.abs(cp - m["cp"]), 506 * EPS * m["cp_abs"])
        fig.check("abs_part", w, np.abs(g["abs_part"].astype(np.float64) - m["abs"]), 2 * EPS * (m["nnz"] + 2) * m["abs"])
        # ---- null symbol: noise power (the buffer np_sel names after the frame, against the one it named before) or TII sum
        delta = SPEC_REL * np.abs(m["null"]).max()
        fig.equal("np_sel flips", w, g["np_sel"], prev["np_sel"] ^ 1)
        old = prev["null_power"][prev["np_sel"]][USED_BINS].astype(np.float64)
        new = g["null_power"][g["np_sel"]][USED_BINS].astype(np.float64)
        X = np.abs(m["null"][USED_BINS])
        # which branch k_frame_tail took is the FIC stage's doing (the CIF count of the last good FIG 0/0): told by the counter of summed null
        # symbols, held to the oracle under its own name, and each branch is then checked for what it must have done
        dev_tii = int(g["tii_cnt"][0]) - int(prev["tii_cnt"][0])
        fig.equal("is_tii (CIF count of the FIC stage)", w, dev_tii, int(o["is_tii"][k]))
        fig.equal("tii epoch", w, int(g["tii_cnt"][1]), int(prev["tii_cnt"][1]))
        if dev_tii:
            fig.equal("noise power carried over a TII frame", w, new, old)
            acc = g["tii_acc"].astype(np.complex128)
            fig.check("tii_acc", w, np.abs(acc - prev["tii_acc"].astype(np.complex128) - m["null"]), delta + 2 * EPS * np.abs(acc))
        else:
            want = old + 0.05 * (X * X + float(K_MIN_NOISE) - old)
            fig.check("null_power", w, np.abs(new - want), 0.05 * (2 * X * delta + delta * delta) + 4 * EPS * np.maximum(old, new))
            fig.equal("tii_acc untouched", w, g["tii_acc"], prev["tii_acc"])
        fig.equal("phase chain", w, m["phase_end"], int(g["nco_phase"]))


def same_bits(a, b):
    """two read-backs, bit for bit"""
    diff = []
    for key in a:
        x, y = a[key], b[key]
        if x is None or y is None:
            same = x is None and y is None
        elif isinstance(x, np.ndarray):
            same = x.tobytes() == y.tobytes()
        else:
            same = np.asarray(x).tobytes() == np.asarray(y).tobytes()
        if not same:
            diff.append(key)
    return diff


def run_case(n_streams, kind, variant):
    streams = fc.build_case(n_streams, kind, variant, spectra=False)
    got = run_engine(streams, kind)
    bins = fc.carrier_bins()
    fig = Figures()

    def one(s):
        f = Figures()
        check_stream(f, s, streams[s], got[s], bins)
        return f
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:      # (the model is numpy: FFTs and exponentials outside the GIL)
        for f in pool.map(one, range(len(streams))):
            fig.merge(f)
    print("\n%d streams (G = %d), %s ring, variant %d: largest value / bound, at (stream, frame, family)" % (n_streams, fc.grid_of(n_streams), kind, variant))
    for what, (w, where) in sorted(fig.worst.items()):
        print("  %-16s %.3g  %r" % (what, w, where))
    native_diff = []
    if kind != "cf32":
        ref = run_engine(streams, "cf32")
        for s, st in enumerate(streams):
            for k in range(st["n_frames"]):
                d = same_bits(got[s][k], ref[s][k])
                if d:
                    native_diff.append((s, k, st["families"].get(k, "real"), d))
        print("  %s ring against a cf32 ring on the same codes: %d read-backs differ" % (kind, len(native_diff)))
    return fig, native_diff


@pytest.mark.parametrize("case", fc.CASES, ids=["%d_%s_v%d" % c for c in fc.CASES])
def test_frame_chain_equals_the_model_on_crafted_frames(case):
    fig, native_diff = run_case(*case)
    assert not fig.bad and not native_diff, (len(fig.bad), fig.bad[:8], native_diff[:8])
    # ... and the bounds are not idle: the float transform is at least a hundredth of its bound away from the float64 one
    assert fig.worst["spectra"][0] > 0.01 and fig.worst["phase_ref"][0] > 0.01


def test_the_entry_refuses_what_it_cannot_do():
    eng = dx.Engine(n_streams=2, max_subch=0, fic_only=True, out_frames=2, ring_frames=2)
    try:
        L = dx.load()
        L.dabx_internal_front_read.argtypes = [dx.C.c_void_p, dx.C.c_int] + [dx.C.c_void_p] * 7
        sc = np.zeros(1, dx.FRONT_SCALARS)
        E_ARG = -2                                                          # DABX_E_ARG (include/dabx.h)
        for stream in (-1, 2):
            assert L.dabx_internal_front_read(eng._h, stream, dx._p(sc), None, None, None, None, None, None) == E_ARG
        assert L.dabx_internal_front_read(eng._h, 0, None, None, None, None, None, None, None) == E_ARG
        assert L.dabx_internal_front_read(None, 0, dx._p(sc), None, None, None, None, None, None) == E_ARG
        assert L.dabx_internal_front_read(eng._h, 1, dx._p(sc), None, None, None, None, None, None) == 0      # scalars alone
        r = dx.front_read(eng, 1)                                           # a fresh engine: no frame, nothing written
        assert r["frame_ok"] == 0 and r["frames"] == 0 and r["rd"] == 0 and not r["spectra"].any() and not r["cp_part"].any()
    finally:
        eng.close()


def test_the_entry_and_the_frame_chain_work_in_the_hipmodule_form():
    """One 3-stream case and the refusals with the binding pointed at hipmodule/libdabx.so."""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_front_stage.py", "-k", "3_s16_v1 or refuses"], cwd=ROOT, env=hipmodule_env(), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
