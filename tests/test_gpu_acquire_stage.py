"""GPU: the null-symbol search (acquire_stream / k_acquire, sync_failed, the hand-over to and from k_frame_head) on the crafted signals of
tests/acquire_cases.py, event by event.  One signal with E events is E streams of one engine, each fed the prefix that makes a drained
engine rest at one event (the stop rule of acquire_cases); every stream must then report, exactly, what the oracle's trace has at that
event: samples_consumed, state, the bits of signal_level and peak_level, level_margin_events -- and the engine's sync_lost counter the sum
over its streams.  Every stream of every engine is compared.  What the inputs reach is proven on the oracle alone by
tests/test_acquire_cases.py; docs/history/acquire_stage_tests.md has the counts."""
import numpy as np
import pytest

import acquire_cases as ac
from dabstar_amd import lib as dx
from test_gpu_engine import _check_frame_scalars

pytestmark = pytest.mark.gpu


def bits(v):
    return ac.f32_bits(v)


def _slice(case, n):
    return case.codes[:n] if case.fmt == "cf32" else case.codes[:2 * n]


def _report(eng, s):
    st = eng.stats(s)
    return dict(samples_consumed=st["samples_consumed"], state=st["state"], s_level_bits=bits(st["signal_level"]),
                peak_level_bits=bits(st["peak_level"]), margin=st["level_margin_events"], frames=st["frames"])


def _drain(eng, n_streams, feed=None, max_steps=1500):
    """dabx_process(1) until samples_consumed has not moved for four steps (and the feeder, if any, has nothing left)"""
    idle, last = 0, None
    for _ in range(max_steps):
        more = feed() if feed else False
        eng.process(1)
        now = [eng.stats(s)["samples_consumed"] for s in range(n_streams)]
        idle = idle + 1 if (now == last and not more) else 0
        last = now
        if idle >= 4:
            return
    raise AssertionError("the engine did not come to rest")


def _compare(eng, streams, exact_in_lock=True):
    """every stream against the model; returns the number of trace events the engine walked through"""
    events = 0
    lost = 0
    for s, (case, n) in enumerate(streams):
        want = ac.expected_stop(case.trace, n)
        got = _report(eng, s)
        keys = ["samples_consumed", "state", "margin", "frames"]
        if exact_in_lock or want["event"] < 0 or case.trace["kind"][want["event"]] != ac.FRAME_DONE:
            keys += ["s_level_bits", "peak_level_bits"]
        else:
            # Behind a frame the default tracker has advanced sLevel chunk by chunk: "relative error ~1e-5" (include/dabx.h, exact_level_tracker);
            # ten times that is the bound.  peakLevel is not tracked in lock in this mode.
            a, b = (float(np.array([v["s_level_bits"]], np.uint32).view(np.float32)[0]) for v in (got, want))
            assert abs(a - b) <= 1.0e-4 * b, (case.name, n, a, b)
        assert {k: got[k] for k in keys} == {k: want[k] for k in keys}, (case.name, n, want["event"], got, want)
        events += want["event"] + 1
        lost += want["sync_lost"]
    assert eng.counters()["sync_lost"] == lost
    return events


def _engine(streams, fmt, ring_frames=None, **kw):
    if ring_frames is None:
        ring_frames = max(n for _c, n in streams) // ac.TF + 2
    thr = streams[0][0].threshold
    assert all(c.threshold == thr for c, _n in streams)
    return dx.Engine(n_streams=len(streams), ring_frames=ring_frames, max_subch=0, fic_only=True, sync_threshold=thr, ring_format=fmt, **kw)


def _streams(fmt, group):
    cases = [c for c in ac.family_a(fmt) if c.name in ac.GROUPS[group]]
    return [(c, n) for c in cases for n in c.prefixes]


@pytest.mark.parametrize("group", range(len(ac.GROUPS)))
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_family_a_every_prefix_rests_where_the_oracle_says(fmt, mode, exact, group):
    streams = _streams(fmt, group)
    assert len(streams) == ac.EXPECTED_STREAMS[fmt][group] and 16 <= len(streams) <= 48
    eng = _engine(streams, fmt, acquire_mode=mode, exact_level_tracker=exact)
    for s, (case, n) in enumerate(streams):
        eng.push_iq(s, _slice(case, n))
    _drain(eng, len(streams))
    events = _compare(eng, streams)
    assert events == ac.EXPECTED_EVENTS[fmt][group]
    eng.close()


@pytest.mark.parametrize("fmt,group", [("cf32", 2), ("s16", 0), ("u8", 3)])
def test_family_a_through_a_ring_of_two_frames(fmt, group):
    """ring_frames = 2, fed piecewise as space frees up: the blocks of the search, the T_u window of a failed correlation and the level
    tracker's reads wrap the ring many times.  The producer leaves the last T_u samples behind the read cursor alone: a stream that waited
    at a dip's end for its frame's worth of samples has its failed correlation in k_frame_head, and the level is then re-walked from the
    anchor at that dip's end -- exact only while those T_u samples are still in the ring (include/dabx.h, exact_level_tracker); no stream
    may have lost them."""
    streams = _streams(fmt, group)
    eng = _engine(streams, fmt, ring_frames=2, acquire_mode=1)
    ring = 2 * ac.TF
    pushed = [0] * len(streams)

    def feed():
        more = False
        for s, (case, n) in enumerate(streams):
            if pushed[s] < n:
                free = ring - ac.TU - (pushed[s] - eng.stats(s)["samples_consumed"])
                m = min(n - pushed[s], free, 150001)
                if m > 0:
                    lo = pushed[s]
                    eng.push_iq(s, case.codes[lo:lo + m] if fmt == "cf32" else case.codes[2 * lo:2 * (lo + m)])
                    pushed[s] += m
                more = more or pushed[s] < n
        return more

    _drain(eng, len(streams), feed)
    assert pushed == [n for _c, n in streams]
    assert sum(eng.stats(s)["level_unanchored_events"] for s in range(len(streams))) == 0
    _compare(eng, streams)
    eng.close()


@pytest.mark.parametrize("fmt,exact", [("cf32", 0), ("cf32", 1), ("s16", 0)])
def test_family_a_correlation_that_fails_in_the_frame_head(fmt, exact):
    """Every second stream gets its prefix in two pushes, split while the stream rests in ST_EVAL_SYNC at an earlier end of a dip: the
    correlation that fails then runs in k_frame_head, the level over its T_u window is k_level_exact's (exact_level_tracker = 1) or the
    re-walk from the anchor's (0), and the stream goes back to k_acquire"""
    streams = _streams(fmt, 0)
    eng = _engine(streams, fmt, acquire_mode=1, exact_level_tracker=exact)
    first = []
    for s, (case, n) in enumerate(streams):
        k = ac.expected_stop(case.trace, n)["event"]
        ends = [j for j in case.held() if j < k]                            # ends of a dip at which a prefix can make the stream rest
        first.append(ac.pin(case.trace, ends[-1]) if (s % 2 == 0 and ends) else n)
        eng.push_iq(s, _slice(case, first[s]))
    assert sum(f != n for f, (_c, n) in zip(first, streams)) >= len(streams) // 3
    _drain(eng, len(streams))
    held = 0
    for s, (case, n) in enumerate(streams):
        if first[s] != n:
            want = ac.expected_stop(case.trace, first[s])
            got = _report(eng, s)
            assert got["state"] == ac.ST_EVAL_SYNC and got["samples_consumed"] == want["samples_consumed"], (case.name, n, got, want)
            held += 1
            lo = first[s]
            eng.push_iq(s, case.codes[lo:n] if fmt == "cf32" else case.codes[2 * lo:2 * n])
    _drain(eng, len(streams))
    _compare(eng, streams)
    assert held >= len(streams) // 3 and sum(eng.stats(s)["level_unanchored_events"] for s in range(len(streams))) == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ families B and C: real frames
class _Scalars:
    """what _check_frame_scalars reads from an engine: the per-frame scalars of ONE stream"""

    def __init__(self):
        self.scalars = dict(clock_err=[], fic_ratio=[], snr_db=[], mer_db=[])
        self.fbbs, self.walk = [], []


def _run_frames(streams, max_steps=400, **kw):
    """every stream's prefix pushed at once, one step at a time: the frame walk and the scalars of every frame, then the drained engine"""
    case0 = streams[0][0]
    eng = dx.Engine(n_streams=len(streams), ring_frames=max(n for _c, n in streams) // ac.TF + 2, max_subch=0, fic_only=True, out_frames=4,
                    sync_threshold=case0.threshold, sync_strongest=bool(case0.strongest), **kw)
    for s, (case, n) in enumerate(streams):
        assert (case.threshold, case.strongest) == (case0.threshold, case0.strongest)
        eng.push_iq(s, case.codes[:n])
    rec = [_Scalars() for _ in streams]
    idle, last = 0, None
    for _ in range(max_steps):
        eng.process(1)
        now = []
        for s in range(len(streams)):
            st = eng.stats(s)
            now.append(st["samples_consumed"])
            if st["frames"] > len(rec[s].walk):
                assert st["frames"] == len(rec[s].walk) + 1
                pos, sti = eng.read_frame_info(s, 1)
                rec[s].walk.append((int(pos[0]), int(sti[0])))
                rec[s].fbbs.append(st["freq_offs_bb_hz"])
                rec[s].scalars["clock_err"].append(st["clock_err_hz"]); rec[s].scalars["fic_ratio"].append(st["fic_ratio_percent"])
                rec[s].scalars["snr_db"].append(st["snr_db_est"]); rec[s].scalars["mer_db"].append(st["mer_db_est"])
        idle = idle + 1 if now == last else 0
        last = now
        if idle >= 4:
            break
    else:
        raise AssertionError("the engine did not come to rest")
    return eng, rec


def _compare_frames(eng, rec, streams, exact):
    frames = 0
    for s, (case, n) in enumerate(streams):
        want = ac.expected_stop(case.trace, n)
        k = want["frames"]
        assert len(rec[s].walk) == k, (case.name, n, len(rec[s].walk), k)
        assert [w[0] for w in rec[s].walk] == case.ora["sym0"][:k].tolist() and [w[1] for w in rec[s].walk] == case.ora["start"][:k].tolist(), (case.name, n)
        if k >= 4:
            _check_frame_scalars(rec[s], rec[s].fbbs, case.ora, k)
        frames += k
    events = _compare(eng, streams, exact_in_lock=bool(exact))
    return events, frames


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("which", range(len(ac.C_CFOS)))
def test_family_c_the_search_after_a_lock(which, mode, exact):
    """the oscillator stands where the last frame left it: the envelope the search sees is |x osc|, the level |x|"""
    case = ac.family_c()[which]
    streams = [(case, n) for n in case.prefixes]
    assert len(streams) == ac.EXPECTED_C_STREAMS and 16 <= len(streams) <= 48
    eng, rec = _run_frames(streams, acquire_mode=mode, exact_level_tracker=exact)
    events, frames = _compare_frames(eng, rec, streams, exact)
    assert (events, frames) == ac.EXPECTED_C_EVENTS
    eng.close()


@pytest.mark.parametrize("exact", [0, 1])
def test_family_b_edges_of_the_frame_chain(exact):
    """+-35 kHz: inside f_sync stays, outside it is reset frame after frame (and every second frame's coarse search finds nothing); a null
    symbol 40 samples short and one 40 samples long: the clock-error estimate at its clamp, both signs"""
    streams = [(case, n) for case in ac.family_b() for n in case.prefixes]
    assert len(streams) == 3
    eng, rec = _run_frames(streams, acquire_mode=1, exact_level_tracker=exact)
    _compare_frames(eng, rec, streams, exact)
    eng.close()
