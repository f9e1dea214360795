"""k_dciq (csrc/pipeline.hip), SampleReader's DC removal and IQ-imbalance correction as a block scan, on the crafted streams of
tests/dciq_cases.py: engines of three streams with a two-frame ring, every stream its own samples and its own partition into launches,
read back through dabx_read_iq and dx.dciq_read (the library's internal test entry: plain copies, no kernel).

After every launch group and for every stream the device must give
  outputs   every sample still in the ring within the case's bound of the oracle's float64 run (NaN exactly where that run has NaN)
  state     meanI, meanQ, meanII, meanQQ, meanIQ within the case's relative bounds of the float64 states; an expected 0 is 0
  done      dciq_done = the number of samples committed to the stream
  idle      a stream without new samples: ring window and state byte for byte what they were
The bounds are not fixed here: 4 x the distance of the float32 restatement of the kernel from float64 on that case and stream, at least
2^-23 of the scale (tests/test_dciq_cases.py shows on the CPU where they come from and that every named mutation of the scan breaks them).
In mode 1 the device also has to equal the restatement bit for bit; in mode 2 the number of differing values is printed.
docs/history/dciq_tests.md has the measured figures."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dciq_cases as dc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def make_engine(mode):
    return dx.Engine(n_streams=dc.S, ring_frames=2, max_subch=0, fic_only=True, out_frames=4, dc_iq_correction=mode)


def snapshot(eng, wr):
    """per stream: (first index of the window, the samples still in the ring, state, done)"""
    snap = []
    for s in range(dc.S):
        lo = max(0, wr[s] - dc.RING)
        got = eng.read_iq(s, lo, wr[s] - lo) if wr[s] > lo else np.zeros(0, np.complex64)
        state, done = dx.dciq_read(eng, s)
        snap.append((lo, got, state, done))
    return snap


def feed_push(eng, case, g, wr):
    for s in range(dc.S):
        if g[s]:
            eng.push_iq(s, case["data"][s][wr[s]:wr[s] + g[s]])               # (a refused push raises)


def feed_commit(eng, case, g, wr, hip):
    """a zero-copy producer: the samples go into the ring through its device pointer, then dabx_commit_iq (equal counts: stream = -1)"""
    for s in range(dc.S):
        if g[s]:
            ptr, cap = eng.ring_ptr(s)
            assert cap == dc.RING and wr[s] % dc.RING + g[s] <= cap
            src = np.ascontiguousarray(case["data"][s][wr[s]:wr[s] + g[s]])
            assert hip.hipMemcpy(C.c_void_p(ptr + 8 * (wr[s] % dc.RING)), C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), 1) == 0
    if len(set(g)) == 1:
        eng.commit(g[0], -1)
    else:
        for s in range(dc.S):
            if g[s]:
                eng.commit(g[s], s)


def run_groups(case, feed, eng=None):
    """the case's launch groups through one engine -> snapshots per group"""
    own = eng is None
    eng = eng or make_engine(case["mode"])
    snaps, wr = [], [0] * dc.S
    try:
        for gi, g in enumerate(case["groups"]):
            for _ in range(case.get("process_before", {}).get(gi, 0)):
                eng.process(1)
            feed(eng, case, g, wr)
            wr = [wr[s] + int(g[s]) for s in range(dc.S)]
            snaps.append(snapshot(eng, wr))
    finally:
        if own:
            eng.close()
    return snaps


class Figures:
    """largest value / bound per check, printed before anything is asserted; failures by (stream, group, what)"""

    def __init__(self):
        self.worst, self.bad = {}, []

    def check(self, what, where, ratio):
        if ratio > self.worst.get(what, (-1.0, None))[0]:
            self.worst[what] = (ratio, where)
        if not ratio <= 1.0:
            self.bad.append((what, where, ratio))

    def equal(self, what, where, a, b):
        if not np.array_equal(a, b):
            self.bad.append((what, where, "differ"))


def _out_ratio(got, want, bound):
    r = 0.0
    for a, b in ((got.real, want.real), (got.imag, want.imag)):
        fin = np.isfinite(b)
        if not np.array_equal(np.isfinite(a), fin) or not np.array_equal(np.isnan(a), np.isnan(b)):
            return np.inf
        if fin.any():
            r = max(r, float(np.abs(a[fin].astype(np.float64) - b[fin]).max()) / bound)
    return r


def _differ(a, b):
    """float32 values that differ in their bits (a NaN equals any NaN)"""
    a, b = np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32)
    return int(np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))))


def check_case(case, snaps, fig=None):
    """every snapshot against the float64 run under the case's bounds -> (Figures, values that differ from the restatement: outputs, states)"""
    dc.finish(case)
    fig = fig or Figures()
    r_out, r_st = case["restated"]
    diff_out = diff_st = 0
    wr = [0] * dc.S
    for gi, g in enumerate(case["groups"]):
        wr = [wr[s] + int(g[s]) for s in range(dc.S)]
        for s in range(dc.S):
            lo, got, state, done = snaps[gi][s]
            want, wst = case["f64"][s]
            b, w = case["bound"][s], (case["name"], s, gi)
            fig.equal("done == wr", w, done, wr[s])
            fig.check("outputs", w, _out_ratio(got, want[lo:wr[s]], b["out"]))
            for j in range(5):
                x, v = float(wst[gi, j]), float(state[j])
                if not np.isfinite(x):
                    ok = np.isnan(v) == np.isnan(x) and not np.isfinite(v)
                    fig.check(dc.STATE_NAMES[j], w, 0.0 if ok else np.inf)
                elif x == 0.0:
                    fig.check(dc.STATE_NAMES[j], w, 0.0 if v == 0.0 else np.inf)
                else:
                    fig.check(dc.STATE_NAMES[j], w, abs(v - x) / abs(x) / b["st"][j] if np.isfinite(v) else np.inf)
            if not g[s] and gi:
                plo, pgot, pstate, pdone = snaps[gi - 1][s]
                fig.equal("idle stream: ring unchanged", w, (lo, got.tobytes()), (plo, pgot.tobytes()))
                fig.equal("idle stream: state unchanged", w, (state.tobytes(), done), (pstate.tobytes(), pdone))
            if g[s]:
                frm = wr[s] - int(g[s])
                diff_out += _differ(got[frm - lo:], r_out[s][frm:wr[s]])
            diff_st += _differ(state, r_st[gi][s])
    return fig, diff_out, diff_st


def report(case, fig, diff_out, diff_st):
    print("\n%s: largest value / bound, at (case, stream, launch group)" % case["name"])
    for what, (w, where) in sorted(fig.worst.items()):
        print("  %-10s %.3g  %r" % (what, w, where))
    print("  values that differ from the float32 restatement: %d outputs, %d states" % (diff_out, diff_st))
    print("  bounds (largest of the streams): outputs %.3g of full scale, states %s of their own value"
          % (max(b["out"] for b in case["bound"]) / case["A"], np.array2string(np.max([b["st"] for b in case["bound"]], axis=0), precision=2)))


def hold(case, snaps):
    fig, diff_out, diff_st = check_case(case, snaps)
    report(case, fig, diff_out, diff_st)
    assert not fig.bad, (len(fig.bad), fig.bad[:8])
    if case["mode"] == 1:                                            # plain IEEE additions and multiplications in one order: bit for bit
        assert diff_out == 0 and diff_st == 0, (case["name"], diff_out, diff_st)
    return fig


@pytest.mark.parametrize("mode", [1, 2])
def test_every_launch_length_and_idle_pattern(mode):
    case = dc.partition_case(mode)
    hold(case, run_groups(case, feed_push))


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("mode", [1, 2])
def test_launches_across_the_ring_boundary(mode, which):
    case = dc.wrap_case(which, mode)
    hold(case, run_groups(case, feed_push))


@pytest.mark.parametrize("amp", dc.AMPS, ids=["A%g" % a for a in dc.AMPS])
@pytest.mark.parametrize("group", range(len(dc.FAMILY_GROUPS)), ids=["g%d" % g for g in range(len(dc.FAMILY_GROUPS))])
@pytest.mark.parametrize("mode", [1, 2], ids=["m1", "m2"])
def test_signal_families_at_three_levels(mode, group, amp):
    case = dc.family_case(group, amp, mode)
    hold(case, run_groups(case, feed_push))


@pytest.mark.parametrize("mode", [1, 2])
def test_one_nan_stays_in_its_stream_and_behind_its_sample(mode):
    """As the serial reference: stream 1 is right up to the NaN and NaN from there on, outputs and state, also after the next launch (the
    float64 run has exactly that, tests/test_dciq_cases.py); streams 0 and 2 are bit for bit what they are without the NaN."""
    case, clean = dc.isolation_case(mode), dc.isolation_case(mode, with_nan=False)
    snaps, ref = run_groups(case, feed_push), run_groups(clean, feed_push)
    hold(case, snaps)
    hold(clean, ref)
    k = case["nan_at"]
    last = snaps[-1][1]
    assert last[0] == 0 and np.isnan(last[1][k:].real).all() and np.isnan(last[1][k:].imag).all() and np.isfinite(last[1][:k].view(np.float32)).all()
    assert np.isnan(last[2][:2]).all()
    for gi in range(len(snaps)):
        for s in (0, 2):
            a, b = snaps[gi][s], ref[gi][s]
            assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3], (gi, s)


def _slab_formats(kind, payloads):
    if kind == "cf32":
        return [dx.IqFormat(1, 5, 0, 0, 32, 2048000, 0, p.nbytes) for p in payloads]           # wav, float32
    return [dx.IqFormat(1, 2, 0, 0, 16, 2500000, 0, p.nbytes) for p in payloads]               # wav, int16 at 2.5 MS/s


def _committed(eng, s, at_least):
    """samples committed to stream s of an engine, found through dabx_read_iq's own bound (whole 1-ms blocks of 2048)"""
    n = at_least
    while True:
        try:
            eng.read_iq(s, n + 2047, 1)
        except dx.DabxError:
            return n
        n += 2048


def run_slabs(mode, kind, payloads, commits):
    """The commits through a slab ingest of the engine under test and of a twin WITHOUT the correction (what the twin's ring holds is the
    correction's input: decode and resampler are not part of the comparison) -> (input per stream, launch groups, snapshots)."""
    eng, twin = make_engine(mode), make_engine(0)
    try:
        slabs, twin_slabs = [e.ingest_open_formats(_slab_formats(kind, payloads), slabs=2, max_frames=1)[0] for e in (eng, twin)]
        pos, wr, groups, snaps = [0] * dc.S, [0] * dc.S, [], []
        for k, c in enumerate(commits):
            nb = []
            for s in range(dc.S):
                raw = np.ascontiguousarray(payloads[s]).view(np.uint8)
                bps = raw.size // (len(payloads[s]) if kind == "cf32" else len(payloads[s]) // 2)
                take = raw[pos[s] * bps:(pos[s] + c[s]) * bps]
                for sl in (slabs, twin_slabs):
                    sl[k % 2][s, :take.size] = take
                nb.append(take.size)
                pos[s] += c[s]
            for e in (eng, twin):
                e.ingest_submit_bytes(k % 2, nb)
                e.ingest_commit(k % 2)
            new = [wr[s] + c[s] if kind == "cf32" else _committed(twin, s, wr[s]) for s in range(dc.S)]
            groups.append(tuple(new[s] - wr[s] for s in range(dc.S)))
            wr = new
            snaps.append(snapshot(eng, wr))
        data = [twin.read_iq(s, 0, wr[s]) for s in range(dc.S)]
        for s in range(dc.S):
            st, done = dx.dciq_read(twin, s)
            assert done == 0 and np.array_equal(st, np.array(dc.INIT, np.float32))          # the twin's correction never ran
        for e in (eng, twin):
            e.ingest_close()
    finally:
        eng.close(); twin.close()
    return data, groups, snaps


@pytest.mark.parametrize("mode", [1, 2])
def test_every_entry_path_launches_the_same_correction(mode):
    """dabx_push_iq, ring pointer + dabx_commit_iq (per stream and stream = -1) and a cf32 slab ingest with unequal counts carry the same
    samples in the same launch ranges: each is held to the model, and all three leave the same bits."""
    hip = C.CDLL("libamdhip64.so")
    case = dc.entry_case(mode)
    pushed = run_groups(case, feed_push)
    hold(case, pushed)
    committed = run_groups(case, lambda e, c, g, wr: feed_commit(e, c, g, wr, hip))
    hold(case, committed)
    data, groups, slab = run_slabs(mode, "cf32", case["data"], case["groups"])
    assert groups == [tuple(g) for g in case["groups"]]
    for s in range(dc.S):
        assert np.array_equal(data[s].view(np.uint32), case["data"][s].view(np.uint32)), s         # the float slab is decoded as it stands
    hold(case, slab)
    for gi in range(len(pushed)):
        for s in range(dc.S):
            for other in (committed, slab):
                a, b = pushed[gi][s], other[gi][s]
                assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3], (gi, s)


@pytest.mark.parametrize("mode", [1, 2])
def test_slab_ingest_behind_the_resampler(mode):
    """int16 recordings at 2.5 MS/s through the slab ingest's 1-ms resampler, unequal counts per stream and commit, 0 among them.  The
    correction's input is what a twin engine without the correction holds after the same calls; the bounds are made on the CPU from
    that input, as those of the stored cases are."""
    data, groups, snaps = run_slabs(mode, "s16", dc.resampled_payloads(mode), dc.RESAMPLED_COMMITS)
    assert all(sum(g[s] for g in groups) >= 4 * 2048 for s in range(dc.S)) and any(0 in g for g in groups) and any(len(set(g)) == 3 for g in groups), groups
    case = dc.model_case(data, groups, mode, name="resampled_m%d" % mode)
    hold(case, snaps)


def test_a_step_queued_right_behind_a_push_reads_corrected_samples():
    """dabx_process(sync = 0) at once behind every push: the search of the unlocked streams reads what k_dciq has left, as it does when
    the engine is drained first -- every statistic of every stream the same, and not what an engine without the correction finds."""
    case = dc.wrap_case("a", 2)
    pieces = [dc.TF - 1000, dc.TF + 1000]

    def run(mode, drain):
        eng = make_engine(mode)
        try:
            at = 0
            for n in pieces:
                for s in range(dc.S):
                    eng.push_iq(s, case["data"][s][at:at + n])
                at += n
                if drain:
                    eng.synchronize()
                eng.process(1, sync=False)
            eng.synchronize()
            return [repr(sorted(eng.stats(s).items())) for s in range(dc.S)], [dx.dciq_read(eng, s)[0].tobytes() for s in range(dc.S)]
        finally:
            eng.close()
    at_once, drained, uncorrected = run(2, False), run(2, True), run(0, True)
    assert at_once == drained
    assert all(a != b for a, b in zip(drained[0], uncorrected[0]))


def test_the_entry_refuses_what_it_cannot_do():
    eng = make_engine(1)
    try:
        L = dx.load()
        L.dabx_internal_dciq_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        st, done = np.zeros(5, np.float32), C.c_uint64(7)
        E_ARG = -2                                                          # DABX_E_ARG (include/dabx.h)
        for stream in (-1, dc.S):
            assert L.dabx_internal_dciq_read(eng._h, stream, dx._p(st), C.byref(done)) == E_ARG
        assert L.dabx_internal_dciq_read(eng._h, 0, None, C.byref(done)) == E_ARG
        assert L.dabx_internal_dciq_read(eng._h, 0, dx._p(st), None) == E_ARG
        assert L.dabx_internal_dciq_read(None, 0, dx._p(st), C.byref(done)) == E_ARG
        assert done.value == 7 and not st.any()
        for s in range(dc.S):                                               # a fresh engine: the reference's initial values
            state, upto = dx.dciq_read(eng, s)
            assert upto == 0 and np.array_equal(state, np.array(dc.INIT, np.float32))
    finally:
        eng.close()


def test_the_entry_and_the_correction_work_in_the_hipmodule_form():
    """One small case and the refusals with the binding pointed at hipmodule/libdabx.so."""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_dciq_stage.py", "-k", "m2-g0-A0.26 or refuses"], cwd=ROOT, env=hipmodule_env(), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
