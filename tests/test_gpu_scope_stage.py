"""The IQ scope and the carrier plots on the device (k_scope, csrc/pipeline.hip with csrc/scope_core.h; dabx_set_scope_mode / dabx_read_scope)
against the float64 model of tests/scope_cases.py, on the six streams of tests/demap_cases.py.

The spectra go where the front end leaves them (dx.demap_inject / dx.demap_frame), so k_scope runs directly in front of the first demapper
launch of each of the three schedules, as in the engine.  After every frame the records, their frame, symbol, types and scalars and both
vectors are compared under the rule of scope_cases.py; a stream with the mode off and an absent frame produce no record; the demapper's
own results with the mode on equal those with it off, byte for byte.  tests/test_scope_cases.py proves without a device that the cases
reach what they are named for and that the plan covers every built plot type."""
import os
import subprocess
import sys

import numpy as np
import pytest

import demap_cases as dc
import scope_cases as sc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S = dc.N_STREAMS
E_ARG, E_STATE = -2, -5                                # DABX_E_ARG, DABX_E_STATE (include/dabx.h)
# (symbol, generator, schedule): every fixed symbol, every generator and every schedule; the longest replay with all three of each
FIXED_RUNS = [(1, 3, 0), (3, 1, 1), (4, 2, 2), (75, 1, 2), (75, 2, 0), (75, 3, 1)]


def _engine(gen, mer=1):
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=len(dc.SUBCH), out_frames=2, capture_soft=True, soft_bit_type=gen, viterbi_tie_mode=0)
    eng.set_subchannels(dc.SUBCH, dab_plus=False)
    eng.set_lcd_statistics(mer)
    return eng


def _inject(eng, frames, step):
    present = [0] * S
    for s in range(S):
        fr = frames[s][step] if step < len(frames[s]) else None
        if fr is None:
            continue
        present[s] = fr["present"]
        if fr["present"]:
            dx.demap_inject(eng, s, fr["spec"], fr["null_fft"], fr["ce"], fr["np_sel"])
        else:                                               # an absent stream gets spectra all the same: showing them would show
            dx.demap_inject(eng, s, fr["spec"] * np.complex64(2j), None, frames[s][step - 1]["ce"], frames[s][step - 1]["np_sel"])
    return present


class Figures:
    """The device's largest deviation per plot type, printed before anything is asserted on it."""

    def __init__(self):
        self.worst, self.bad = {}, []

    def note(self, key, d, where):
        if d > self.worst.get(key, (-1.0, None))[0]:
            self.worst[key] = (d, where)

    def check(self, rec, iq, carr, m, gen, frame, symbol, types, where):
        hdr = (int(rec["frame"]), int(rec["symbol"]), int(rec["iq_type"]), int(rec["carrier_type"]), int(rec["soft_bit_type"]), int(rec["reserved0"]),
               rec["reserved"].tolist())
        if hdr != (frame, symbol, types[0], types[1], gen, 0, [0, 0]):
            self.bad.append((where, "header", hdr))
        if m["name"] in sc.UNDEFINED_NAMES:                 # NaN state in every generator: the record and its header only
            return
        for k, got, exp in (("mean_value", rec["mean_value"], m["mean_value"]), ("mean_power_all", rec["mean_power_all"], m["mpa"])):
            if np.isfinite(exp) and exp != 0:
                self.note(k + " (relative)", abs(float(got) - exp) / abs(exp), where)
            if not (sc.mpa_ok(float(got), exp) if k == "mean_power_all" else sc.scalar_ok(float(got), exp)):
                self.bad.append((where, k, float(got), exp))
        n_bad, d = sc.compare_iq(iq, m["iq"][types[0]])
        self.note("IQ type %d, |d| / (1 + |x|)" % types[0], d, where)
        if n_bad:
            self.bad.append((where, "iq", types[0], n_bad, d))
        n_bad, d = sc.compare_carr(carr, m["carr"][types[1]], types[1])
        self.note("%s, |d|" % sc.CARRIER_NAMES[types[1]], d, where)
        if n_bad:
            self.bad.append((where, sc.CARRIER_NAMES[types[1]], n_bad, d))

    def report(self, title):
        for k in sorted(self.worst):
            print("%s: %-40s %.3e  (%s)" % (title, k, self.worst[k][0], self.worst[k][1]))


def _run_fixed(symbol, gen, schedule, off_stream=None, collect=False, scope=True):
    """Every step of the plan with `symbol` shown in every decoded frame, the plot types of scope_cases.plot_plan, changed before every frame.
    -> (Figures, per stream (captures, FIBs, CRC verdicts, {slot: logical frames}) when collect)."""
    frames = [dc.stream_frames(s) for s in range(S)]
    want = [{f: (symbol,) for f in range(sum(fr["present"] for fr in frames[s]))} for s in range(S)]
    fig = Figures()
    cap, fibs, crcs = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    msc = [{j: [] for j in range(len(dc.SUBCH))} for _ in range(S)]
    seen = [[0] * len(dc.SUBCH) for _ in range(S)]
    eng = _engine(gen)
    try:
        at, shows = [0] * S, [0] * S
        for step in range(dc.N_STEPS):
            types = {}
            for s in range(S):
                if scope and s != off_stream and step < len(frames[s]):
                    types[s] = sc.plot_plan(symbol, s, step)
                    eng.set_scope_mode(s, iq_type=types[s][0], carrier_type=types[s][1], symbol=symbol)
            present = _inject(eng, frames, step)
            dx.demap_frame(eng, present, schedule)
            for s in range(S):
                recs, lost = eng.read_scope(s) if scope else ([], 0)
                if not present[s] or s == off_stream or not scope:
                    assert recs == [] and lost == 0, (step, s)                        # an absent frame, a stream with the mode off: no record
                    assert not scope or eng.scope_stats(s)["shows"] == shows[s], (step, s)
                    continue
                assert len(recs) == 1 and lost == 0, (step, s, len(recs), lost)
                shows[s] += 1
                m = sc.model(s, gen, want[s])[(at[s], symbol)]
                fig.check(recs[0][0], recs[0][1], recs[0][2], m, gen, at[s], symbol, types[s], "%s, symbol %d, generator %d" % (m["name"], symbol, gen))
            for s in range(S):
                if present[s]:
                    if collect:
                        cap[s].append(eng.read_soft(s))
                    at[s] += 1
            dx.fic_decode_frame(eng, present)                # (the frame count moves here: the next record's frame index)
            if collect:
                dx.msc_decode(eng, [4 * p for p in present], 4)
                for s in range(S):
                    if not present[s]:
                        continue
                    f, c = eng.read_fibs(s, 1)
                    fibs[s].append(f[0]); crcs[s].append(c[0])
                    for j in range(len(dc.SUBCH)):
                        n = eng.subch_stats(s, j)["cifs_decoded"]
                        if n > seen[s][j]:
                            msc[s][j].extend(eng.read_msc(s, j, n - seen[s][j]))
                            seen[s][j] = n
        if scope:
            st = eng.scope_stats(0)
            assert st["launches"] == dc.N_STEPS and st["lost"] == 0
    finally:
        eng.close()
    out = [(np.stack(cap[s]), np.stack(fibs[s]), np.stack(crcs[s]), {j: np.array(v) for j, v in msc[s].items()}) for s in range(S)] if collect else None
    return fig, out


@pytest.mark.parametrize("run", FIXED_RUNS, ids=["symbol%d_gen%d_schedule%d" % r for r in FIXED_RUNS])
def test_fixed_symbols_equal_the_model_frame_by_frame(run):
    """One engine per run, six streams, every step of the plan, LCD statistics on; stream 0 has the mode off in the run of symbol 3."""
    symbol, gen, schedule = run
    fig, _ = _run_fixed(symbol, gen, schedule, off_stream=0 if symbol == 3 else None)
    fig.report("symbol %d gen %d schedule %d" % run)
    assert not fig.bad, (len(fig.bad), fig.bad[:8])


def test_the_references_cadence_on_all_streams_and_the_counters_keep_still_without_a_frame():
    """symbol = 0: the ten-frame integrator stream shows exactly what the counter model gives (decoded frames 3, 5, 7 at symbol 1, 9 at symbol
    2); stream 5's absent frame moves neither counter (its shows come in steps 3 and 5, not 2 and 4); stream 0 has the mode off in steps 0
    and 1 and starts counting with step 2 (one show, in step 4); changing the plot types of an enabled stream keeps the counters."""
    gen, schedule = 2, 1
    frames = [dc.stream_frames(s) for s in range(S)]
    expect, model_of = {}, {}
    for s in range(S):
        pres = [fr["present"] for fr in frames[s]]
        steps = [i for i, p in enumerate(pres) if p]
        cad = sc.cadence(pres[2:]) if s == 0 else sc.cadence(pres)
        off = 2 if s == 0 else 0                             # (stream 0: every one of its frames is present)
        expect[s] = {steps[f + off]: (f + off, l) for f, l in cad}
        w = {}
        for f, l in expect[s].values():
            w.setdefault(f, []).append(l)
        model_of[s] = sc.model(s, gen, w)
    assert expect[4] == {2: (2, 1), 4: (4, 1), 6: (6, 1), 8: (8, 2)} and sorted(expect[5]) == [3, 5] and expect[0] == {4: (4, 1)}
    fig = Figures()
    eng = _engine(gen)
    try:
        got = {s: [] for s in range(S)}
        for step in range(dc.N_STEPS):
            types = {}
            for s in range(S):
                if step >= (2 if s == 0 else 0):
                    types[s] = ((s + step) % 3, sc.CARRIER_TYPES[(2 * s + step) % len(sc.CARRIER_TYPES)])
                    eng.set_scope_mode(s, iq_type=types[s][0], carrier_type=types[s][1], symbol=0)
            present = _inject(eng, frames, step)
            dx.demap_frame(eng, present, schedule)
            for s in range(S):
                recs, lost = eng.read_scope(s)
                assert lost == 0
                if step in expect[s] and present[s]:
                    f, l = expect[s][step]
                    assert len(recs) == 1, (step, s)
                    m = model_of[s][(f, l)]
                    fig.check(recs[0][0], recs[0][1], recs[0][2], m, gen, f, l, types[s], "%s, cadence symbol %d" % (m["name"], l))
                    got[s].append(step)
                else:
                    assert recs == [], (step, s, [int(r[0]["symbol"]) for r in recs])
            dx.fic_decode_frame(eng, present)
        assert {s: got[s] for s in range(S)} == {s: sorted(expect[s]) for s in range(S)}
        assert eng.scope_stats(4)["shows"] == 4
    finally:
        eng.close()
    fig.report("cadence")
    assert not fig.bad, (len(fig.bad), fig.bad[:8])


def test_the_demappers_results_are_the_same_bytes_with_the_mode_on_and_off():
    """Soft captures, FIBs, CRC verdicts and MSC bytes of a run with the mode on (symbol 75: k_scope replays the whole frame in front of
    the demapper) equal those of a run with it off."""
    (_, on), (_, off) = _run_fixed(75, 2, 1, collect=True), _run_fixed(75, 2, 1, collect=True, scope=False)
    for s in range(S):
        a, b = on[s], off[s]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), s
        assert a[3].keys() == b[3].keys() and all(np.array_equal(a[3][j], b[3][j]) for j in a[3]), s
        assert a[0].shape[0] == sum(fr["present"] for fr in dc.stream_frames(s))
    assert sum(int(on[s][2].sum()) for s in range(S)) >= 12 * 8          # ... and they are results: the FIC of the undisturbed frames decodes


def _small_engine(**kw):
    return dx.Engine(n_streams=2, max_subch=0, fic_only=True, out_frames=2, ring_frames=2, capture_soft=True, **kw)


def test_the_refusals():
    eng = _small_engine()
    try:
        L = dx.load()
        L.dabx_set_scope_mode.argtypes = [dx.C.c_void_p, dx.C.c_int, dx.C.c_void_p]

        def set_mode(stream, **kw):
            return L.dabx_set_scope_mode(eng._h, stream, dx.C.byref(dx.ScopeConfig(**dict(dict(enable=1), **kw))))
        for iq in (3, 4, -1, 5):                              # the DC-offset plots, and what is no type at all
            assert set_mode(0, iq_type=iq) == E_ARG
        for ct in (10, 11, 12, 14, -1):                       # the three NULL_* level plots, and what is no type at all
            assert set_mode(0, carrier_type=ct) == E_ARG
        for stream in (-2, 2):
            assert set_mode(stream) == E_ARG
        for symbol in (-1, 76):
            assert set_mode(0, symbol=symbol) == E_ARG
        assert eng.scope_stats(0) == dict(shows=0, lost=0, launches=0) and eng.read_scope(0) == ([], 0)      # nothing exists yet
        assert set_mode(0, carrier_type=sc.STD_DEV) == E_STATE                        # needs the LCD statistics
        eng.set_lcd_statistics(1)
        assert set_mode(0, carrier_type=sc.STD_DEV) == 0
        assert set_mode(-1, carrier_type=sc.NULL_OVR_POW, iq_type=2, symbol=75) == 0
        assert set_mode(0, enable=0, iq_type=99) == 0                                  # switching off looks at nothing else
        with pytest.raises(dx.DabxError):
            eng.set_scope_mode(0, iq_type=3)
        L.dabx_read_scope.argtypes = [dx.C.c_void_p, dx.C.c_int, dx.C.c_int, dx.C.c_void_p, dx.C.c_void_p, dx.C.c_void_p, dx.C.c_void_p]
        assert L.dabx_read_scope(eng._h, 2, 1, None, None, None, None) == E_ARG and L.dabx_read_scope(eng._h, 0, 1, None, None, None, None) == E_ARG
        assert L.dabx_read_scope(eng._h, 0, 0, None, None, None, None) == 0
    finally:
        eng.close()


def test_nine_shows_unread_give_eight_records_and_one_lost():
    frames = dc.stream_frames(4)
    eng = _small_engine(soft_bit_type=1)
    try:
        eng.set_scope_mode(1, iq_type=1, carrier_type=sc.EVM_PER, symbol=1)
        for f in range(9):
            dx.demap_inject(eng, 1, frames[f]["spec"], frames[f]["null_fft"], frames[f]["ce"], frames[f]["np_sel"])
            dx.demap_frame(eng, [0, 1], 0)
            dx.fic_decode_frame(eng, [0, 1])
        recs, lost = eng.read_scope(1, max_records=16)
        assert lost == 1 and [int(r[0]["frame"]) for r in recs] == list(range(1, 9))
        assert eng.scope_stats(1) == dict(shows=9, lost=1, launches=9) and eng.read_scope(1) == ([], 0) and eng.read_scope(0) == ([], 0)
        m = sc.model(4, 1, {f: (1,) for f in range(9)})
        fig = Figures()
        for r in recs:
            f = int(r[0]["frame"])
            fig.check(r[0], r[1], r[2], m[(f, 1)], 1, f, 1, (1, sc.EVM_PER), "ring, frame %d" % f)
        assert not fig.bad, fig.bad[:4]
    finally:
        eng.close()


def test_the_mode_works_in_the_hipmodule_form():
    """One run of the fixed-symbol test, the refusals and the ring, with the binding pointed at hipmodule/libdabx.so: k_scope is found in
    the code object of pipeline.hip and launched through hipModuleLaunchKernel."""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_scope_stage.py",
                        "-k", "symbol75_gen3_schedule1 or refusals or nine_shows"], cwd=ROOT, env=hipmodule_env(), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
