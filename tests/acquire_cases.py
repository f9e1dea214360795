"""Inputs and model of the null-symbol search's stage test (no device).

The search (acquire_stream / k_acquire in csrc/pipeline.hip, with sync_failed and the hand-over to and from k_frame_head) restates
timesyncer.cpp:40-90 -- a sample-serial loop -- as a four-wave pipeline over 1024-sample blocks.  This module makes the signals that
steer it through its block grid, its time-outs, its restarts and its shortcuts, and the model that says where a drained engine must
rest for every prefix of such a signal.

THE STOP RULE.  A drained engine (dabx_process(1) repeated until samples_consumed stops moving) rests at a known event of the oracle's
trace (oracle/dab_oracle.h, ora_trace_event).  With N samples committed it rests at the first event whose state needs more than is left:
  ACQ_NEED   samples where the stream goes on searching (the start, NO_DIP, NO_END, CORR_FAILED),
  FRAME_NEED samples where the frame chain takes it (DIP_END: k_acquire or k_frame_head correlates only with a frame's worth in the ring;
             FRAME_DONE: the next frame).
SEEDED and CORR_OK are no resting points of the library: acquire_stream seeds and searches in one call (ACQ_NEED covers the 20 T_u reads
plus one whole attempt), and k_frame_head reads the frame in the step in which its correlation succeeds.  The rule is the library's, not
the reference's; both constants are read from csrc/pipeline.h.  Committing N = pos_k + need_k - 1 samples pins event k: one signal with E
events becomes E streams of one engine, each with its own prefix, and each must report the oracle's samples_consumed, state, sLevel and
peakLevel bits, margin count and lost-sync count at that event.

Family A: envelopes a[n] u[n], u[n] in {1, j, -1, -j} (every magnitude exact, the spectrum white), sync_threshold 1e9 on both sides so that
every correlation fails and the search never hands a stream to the frame chain for longer than one correlation.
Family C: real frames at 30 dB with a carrier offset, a crafted stretch spliced in after six frames in lock: the search runs with the
oscillator phase where the last frame left it (the envelope is |x osc|, the level |x|).
Family B: real frames at the edges of the frame chain's frequency and clock-error limits."""
import functools
import os
import re
import sys

import numpy as np

import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import dab_synth as ds  # noqa: E402

TU, TF, TN = ds.TU, ds.TF, 2656
BLOCK = 1024                                 # ACQ_CH of csrc/pipeline.hip: the search evaluates 1024 positions at once, 64 groups of 16
ST_INIT, ST_WAIT_SYNC, ST_EVAL_SYNC = 0, 1, 2
SEEDED, NO_DIP, NO_END, DIP_END, CORR_FAILED, CORR_OK, FRAME_DONE = range(7)
SEARCH_EVENTS = (NO_DIP, NO_END, DIP_END)
FORMATS = ("cf32", "s16", "u8")
A_THRESHOLD = 1.0e9


def library_needs(path=os.path.join(ROOT, "dabstar_amd", "csrc", "pipeline.h")):
    """(ACQ_NEED, FRAME_NEED) from their two constexpr lines."""
    text = open(path).read()
    env = {"TU": TU, "TF": TF, "TN": TN, "__builtins__": {}}
    out = []
    for name in ("ACQ_NEED", "FRAME_NEED"):
        m = re.search(r"^constexpr int %s = ([0-9TUFN+*() ]+);" % name, text, re.M)
        assert m, name
        out.append(int(eval(m.group(1), env)))          # digits, T_U / T_F / T_N, + * ( ) only
    return tuple(out)


ACQ_NEED, FRAME_NEED = library_needs()
TAIL = ACQ_NEED + TF                          # constant tail behind every crafted stretch


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


# ------------------------------------------------------------------------------------------------------------ the model
def need_of(kind):
    """samples that must be left in the ring for the stream to move on from an event of this kind (None: no resting point)"""
    if kind in (NO_DIP, NO_END, CORR_FAILED):
        return ACQ_NEED
    if kind in (DIP_END, FRAME_DONE):
        return FRAME_NEED
    return None


def simulate(trace, n_committed):
    """k_acquire's passes over the first n_committed samples of the signal the trace belongs to, all of them in the ring from the start.
    Returns (index of the event the drained engine rests at; -1 = before the first sample; None = the trace ends first,
             one record per search event up to there: the acquire_stream call it belongs to and where in that call's block grid it lies)."""
    recs = []
    if n_committed < ACQ_NEED:
        return -1, recs
    assert trace[0]["kind"] == SEEDED
    pass_start = call_base = 0
    attempt_start = int(trace[0]["pos"])
    for i in range(1, len(trace)):
        ev = trace[i]
        kind, pos = int(ev["kind"]), int(ev["pos"])
        if kind in SEARCH_EVENTS:
            b = attempt_start + int(ev["dip_begin"]) if ev["dip_begin"] >= 0 else None
            e = b + int(ev["dip_len"]) if ev["dip_len"] >= 0 else None
            rec = dict(i=i, kind=kind, call_base=call_base, attempt_start=attempt_start, begin=b, end=e, then=None)
            recs.append(rec)
            if kind == DIP_END:
                if n_committed - pos < FRAME_NEED:
                    return i, recs
            else:
                if n_committed - pos < ACQ_NEED:
                    rec["then"] = "space"
                    return i, recs
                if pos - call_base < TF - (call_base - pass_start):     # consumed < budget_samples: the same call tries again
                    rec["then"] = "same call"
                else:
                    rec["then"] = "budget"
                    pass_start = call_base = pos
                attempt_start = pos
        elif kind == CORR_FAILED:
            if n_committed - pos < ACQ_NEED:
                return i, recs
            if n_committed - pos < ACQ_NEED + FRAME_NEED or pos - pass_start >= TF or int(trace[i - 1]["kind"]) == FRAME_DONE:
                pass_start = pos
            call_base = attempt_start = pos
        elif kind == FRAME_DONE:
            if n_committed - pos < FRAME_NEED:
                return i, recs
    return None, recs


def expected_stop(trace, n_committed):
    """What a drained engine reports for the first n_committed samples: dict(event, samples_consumed, state, s_level_bits, peak_level_bits,
    margin, sync_lost, frames)."""
    k, _ = simulate(trace, n_committed)
    assert k is not None, "the trace ends before the stream rests: the signal's tail is too short"
    if k < 0:
        return dict(event=-1, samples_consumed=0, state=ST_INIT, s_level_bits=f32_bits(0.1), peak_level_bits=f32_bits(-1.0e6), margin=0,
                    sync_lost=0, frames=0)
    ev = trace[k]
    kinds = trace["kind"][:k + 1]
    return dict(event=k, samples_consumed=int(ev["pos"]), state=ST_EVAL_SYNC if int(ev["kind"]) in (DIP_END, FRAME_DONE) else ST_WAIT_SYNC,
                s_level_bits=int(ev["s_level_bits"]), peak_level_bits=int(ev["peak_level_bits"]), margin=int(ev["margin"]),
                sync_lost=int((kinds == CORR_FAILED).sum()), frames=int((kinds == FRAME_DONE).sum()))


def pin(trace, k):
    """the prefix length that pins event k"""
    return int(trace[k]["pos"]) + need_of(int(trace[k]["kind"])) - 1


# ------------------------------------------------------------------------------------------------------------ sample formats
def to_codes(x, fmt):
    """what is pushed into an engine of that ring format"""
    if fmt == "cf32":
        return np.ascontiguousarray(x, np.complex64)
    from test_gpu_ring_format import quantise
    return np.ascontiguousarray(quantise(x, fmt, 1.0))


def to_values(codes, fmt):
    """what the oracle is fed: the values the codes stand for"""
    if fmt == "cf32":
        return codes
    from test_gpu_ring_format import values
    return values(codes, fmt)


# base amplitude of the envelopes (relative amplitude 1) and the largest relative amplitude the format holds
FMT_SCALE = {"cf32": 1.0, "s16": 0.125, "u8": 0.5}
FMT_MAX = {"cf32": 1.0e5, "s16": 7.99, "u8": 1.99}


# ------------------------------------------------------------------------------------------------------------ family A
class Craft:
    """An envelope under construction: the seed (20 T_u samples at relative amplitude 1), then segments appended one by one, each placed by
    running the oracle on the signal so far plus a constant tail and shifting lengths until its edges land where they are wanted."""

    def __init__(self, fmt, seed, continuous_phase=False, before=None, after=None, tone_hz=None, scale=None, threshold=A_THRESHOLD, strongest=0):
        """before / after: samples in front of the envelope instead of its seed / behind it instead of the constant tail (family C: real frames);
        tone_hz: the envelope's carrier is one tone instead of random quarter turns"""
        self.fmt = fmt
        self.rng = np.random.default_rng(seed)
        self.before, self.after, self.threshold, self.strongest = before, after, threshold, strongest
        self.scale = FMT_SCALE[fmt] if scale is None else scale
        self.amp = [np.ones(20 * TU, np.float32)] if before is None else [np.zeros(0, np.float32)]
        n_max = 7 * 1000 * 1000
        if tone_hz is not None:
            self.unit = np.exp(2j * np.pi * tone_hz * np.arange(n_max // 4) / ds.FS).astype(np.complex64)
        elif continuous_phase:
            self.unit = np.exp(2j * np.pi * self.rng.random(n_max)).astype(np.complex64)
        else:
            self.unit = np.array([1, 1j, -1, -1j], np.complex64)[self.rng.integers(0, 4, n_max)]
        self.tail_level = 1.0

    def built(self):
        """samples so far, everything in front included"""
        return sum(len(p) for p in self.amp) + (0 if self.before is None else len(self.before))

    def amps(self, extra=(), tail=TAIL):
        parts = self.amp + [np.asarray(e, np.float32) for e in extra]
        if tail and self.after is None:
            parts = parts + [np.full(tail, self.tail_level, np.float32)]
        return np.concatenate(parts)

    def codes(self, extra=(), tail=TAIL):
        a = self.amps(extra, tail)
        a = np.minimum(a, np.float32(FMT_MAX[self.fmt]))
        x = ((a * np.float32(self.scale)).astype(np.float32) * self.unit[:len(a)]).astype(np.complex64)
        if self.before is not None:
            x = np.concatenate([self.before, x] + ([self.after] if tail and self.after is not None else []))
        return to_codes(x, self.fmt)

    def values(self, extra=(), tail=TAIL):
        return to_values(self.codes(extra, tail), self.fmt)

    def trace(self, extra=(), tail=TAIL):
        return ol.oracle_trace(self.values(extra, tail), self.threshold, self.strongest)

    def append(self, *segs):
        self.amp += [np.asarray(s, np.float32) for s in segs]

    def flat(self, n, level=1.0):
        self.append(np.full(n, level, np.float32))

    def add_dip(self, gap=400, lo_len=1000, lo=0.0, boost=None, want_b=None, want_e=None, want_rel_begin=None, want_len=None,
                want_kind=DIP_END, lo_range=(300, 2000), post=TU + 100):
        """gap samples at 1, lo_len at lo, then (boost = (amplitude, samples)) and post samples at 1 (enough for the dip to end and the T_u
        window of the failed correlation to be read inside the segment).  The search event this makes -- the first one
        behind the events already there -- gets its dip begin at block position want_b and its end at want_e of the acquire_stream call that
        evaluates them (positions mod 1024), or at an attempt-relative begin / a dip length.  Returns its record of simulate()."""
        n0 = self.built()
        k0 = None
        for it in range(60):
            if it % 12 == 11 and want_rel_begin is None:
                gap += BLOCK                                                 # (a crossing too close to its threshold to move by single samples: another level)
            segs = [np.ones(gap, np.float32), np.full(lo_len, lo, np.float32)]
            if boost:
                segs.append(np.full(boost[1], boost[0], np.float32))
            segs.append(np.ones(post, np.float32))
            tr = self.trace(segs)
            if k0 is None:
                k0 = int((tr["pos"] <= n0).sum())
            _, recs = simulate(tr, 1 << 40)
            rec = next(r for r in recs if r["i"] >= k0)
            if rec["kind"] == NO_END and want_kind == DIP_END and isinstance(want_len, int):
                lo_len -= 16                                                 # (too long for an end to be found at all)
                continue
            assert rec["kind"] == want_kind or want_kind is None, (ol.EV_NAMES[rec["kind"]], gap, lo_len)
            ev = tr[rec["i"]]
            d_gap = d_len = 0
            if want_b is not None:
                d_gap = (want_b - (rec["begin"] - rec["call_base"]) + BLOCK // 2) % BLOCK - BLOCK // 2
            if want_rel_begin is not None:
                d_gap = want_rel_begin - int(ev["dip_begin"])
            if gap + d_gap < 150 and want_rel_begin is None:
                d_gap += BLOCK
            if want_e is not None:
                d_len = (want_e - (rec["end"] + d_gap - rec["call_base"]) + BLOCK // 2) % BLOCK - BLOCK // 2
                if lo_len + d_len < lo_range[0]:
                    d_len += BLOCK
                if lo_len + d_len > lo_range[1]:
                    d_len -= BLOCK
            if isinstance(want_len, tuple):                                  # a short dip: any length in the range (a low sample more is ~1.5 more)
                got = int(ev["dip_len"])
                miss = want_len[0] - got if got < want_len[0] else (want_len[1] - got if got > want_len[1] else 0)
                d_len = 0 if miss == 0 else (miss * 2 // 3 if abs(miss) > 2 else (1 if miss > 0 else -1))
            elif want_len is not None:
                d_len = want_len - int(ev["dip_len"])
            if d_gap == 0 and d_len == 0:
                rec["gap_index"] = len(self.amp)
                self.append(*segs)
                rec["event"] = ev
                return rec
            gap += d_gap
            lo_len += d_len
        raise AssertionError("the dip does not settle where it is wanted")


def add_edge_pair(c, want_b, lo, gap=400):
    """Two dips with the begin at block position want_b: one whose end is found at count T_n + 70, the last that is compared, and one a sample
    longer (NO_END).  A begin taken one sample early turns the first into a time-out, one taken late turns the second into a dip end: the
    begin itself decides where the stream rests, which an ordinary dip's end does not tell."""
    c.add_dip(gap=gap, lo=lo, lo_len=TN, want_b=want_b, want_len=TN + 70)
    add_no_end_by_one(c, want_b, lo)


def add_no_end_by_one(c, want_b, lo):
    """a dip one sample too long for its end to be compared: NO_END with the envelope already back up, so the attempt that restarts there is clean"""
    r = c.add_dip(lo=lo, lo_len=TN, want_b=want_b, want_len=TN + 70)
    g = r["gap_index"] + 1
    c.amp[g] = np.full(len(c.amp[g]) + 1, lo, np.float32)


class Case:
    """One signal: codes (what an engine of ring format fmt is pushed), values (what the oracle is fed), the oracle's trace, the prefixes that
    are run (one stream each), and the catalogue entries its builder claims (checked from the trace by tests/test_acquire_cases.py)."""

    def __init__(self, name, fmt, codes, threshold=A_THRESHOLD, pins=None, subch=None, note=None, strongest=0):
        self.name, self.fmt, self.codes, self.threshold, self.strongest = name, fmt, codes, threshold, strongest
        self.values = to_values(codes, fmt)
        self.subch = subch
        self.note = note or {}
        if subch is None:
            self.trace = ol.oracle_trace(self.values, threshold, strongest)
            self.ora = None
        else:
            self.ora = ol.oracle_run(self.values, subch, config=(threshold, strongest, 1), trace=1 << 14)
            self.trace = self.ora["trace"]
        restable = [k for k in range(len(self.trace)) if need_of(int(self.trace[k]["kind"])) is not None]
        ks = restable if pins is None else [k for k in pins if k in restable]
        n = len(self.values)
        self.prefixes = sorted({pin(self.trace, k) for k in ks if pin(self.trace, k) <= n})

    def held(self):
        """the ends of a dip at which a prefix can make the stream rest, in ST_EVAL_SYNC with the correlation still to come (most cannot:
        the failed correlation in front of them needs ACQ_NEED - FRAME_NEED samples more than they do)"""
        tr = self.trace
        return [k for k in range(len(tr)) if tr["kind"][k] == DIP_END and pin(tr, k) <= len(self.values) and simulate(tr, pin(tr, k))[0] == k]

    def records(self):
        """simulate() records of every search event any of the prefixes reaches, with the prefix's own passes"""
        out = {}
        for n in self.prefixes:
            for r in simulate(self.trace, n)[1]:
                out.setdefault((r["i"], r["call_base"], r["then"]), r)
        return list(out.values())


SPECIAL_POS = (0, 1, 15, 16, 17, 1007, 1008, 1022, 1023)


def _finish(c, name, fmt, note=None, keep=None):
    """the case of a finished envelope: one prefix for every event inside the crafted stretch at which a stream can rest (keep(trace, k):
    only those events)"""
    case = Case(name, fmt, c.codes(), pins=[], note=note)
    tr = case.trace
    by_stop = {}
    for k in range(1, int((tr["pos"] <= c.built() + TU + 64).sum())):
        if need_of(int(tr["kind"][k])) is not None:
            stop = simulate(tr, pin(tr, k))[0]
            if keep is None or keep(tr, stop):
                by_stop.setdefault(stop, pin(tr, k))
    case.prefixes = sorted(by_stop.values())
    return case


def grid_residues(fmt):
    """dip begin at every residue 0..15 of the 16-sample group, each twice: with the end found at the last count that is compared (at residue
    r + 6: every residue as well) and with the dip a sample longer"""
    c = Craft(fmt, 101)
    for r in range(16):
        # (every fourth pair lies more than ACQ_NEED - FRAME_NEED samples behind the last event: only then can a prefix make the stream rest
        #  at the dip's end, in ST_EVAL_SYNC, with the correlation still to come)
        add_edge_pair(c, 16 * ((5 * r + 2) % 60 + 2) + r, 0.0 if fmt != "u8" else 0.01, gap=40400 if r % 4 == 0 else 400)
    return _finish(c, "grid_residues", fmt)


def grid_special(fmt):
    """dip begin (as edge pairs) and dip end at block positions 0, 1, 15, 16, 17, 1007, 1008, 1022, 1023; begin and end in the same group, in
    neighbouring groups, and with the begin in the last group of a block and the end in the first group of the next"""
    c = Craft(fmt, 102)
    lo = 0.0 if fmt != "u8" else 0.01
    for wb in SPECIAL_POS:
        add_edge_pair(c, wb, lo)
    for i, we in enumerate(SPECIAL_POS):
        c.add_dip(want_b=100 + 37 * i, want_e=we, lo=lo)
    # short dips, six to eleven samples from begin to end: just enough low samples, then 12 at three times the level bring the moving sum straight back
    short = dict(lo_len=44, lo=lo, boost=(3.0, 12), want_len=(6, 11), lo_range=(0, 100))
    c.add_dip(want_b=16 * 21 + 2, **short)                                   # same group
    c.add_dip(want_b=16 * 33 + 10, **short)                                  # neighbouring groups
    c.add_dip(want_b=1019, **short)                                          # last group of a block -> first group of the next
    return _finish(c, "grid_special", fmt)


def attempt_start(fmt):
    """a dip already under way when the attempt starts (begin at attempt-relative sample 50, the first that counts); begin at 51; a large sample 49
    (a search that accepted a dip from sample 49 would take it there); attempts restarting inside a low stretch, one of them with its first
    50 samples across a block boundary"""
    c = Craft(fmt, 103)
    lo = 0.0 if fmt != "u8" else 0.01
    big = 40.0 if fmt != "u8" else 1.99
    # (1) the dip ends, the T_u window of the failed correlation is read, and the next attempt starts inside a second low stretch
    r = c.add_dip(lo=lo, lo_len=800, post=0)
    n_built = sum(len(p) for p in c.amp)
    end_abs = r["end"]
    next_start = end_abs + TU                                                # where the next attempt starts
    c.flat(next_start - 100 - n_built)
    c.flat(700, lo)                                                          # under way for 100 samples when the attempt starts -> begin at 50
    c.flat(TU + 600)
    # (2) begin at 51: sample 0 of the attempt carries the whole window, then low
    r = c.add_dip(lo=lo, lo_len=800, post=0)
    n_built = sum(len(p) for p in c.amp)
    next_start = r["end"] + TU
    c.flat(next_start - 60 - n_built)
    c.flat(60, lo)
    c.append([big])
    c.flat(700, lo)
    c.flat(TU + 600)
    # (3) samples 0..48 low, sample 49 large: no dip at 50; the large sample leaves the window 50 samples later
    r = c.add_dip(lo=lo, lo_len=800, post=0)
    n_built = sum(len(p) for p in c.amp)
    next_start = r["end"] + TU
    c.flat(next_start - 60 - n_built)
    c.flat(60 + 49, lo)
    c.append([big])
    c.flat(700, lo)
    c.flat(TU + 600)
    # (4) a low stretch of 20 attempts: every restart is mid-block (stride T_n + 121 = 2777 = 9 mod 16: every residue of the group), the first
    #     dip placed so that the second restart's first 50 samples lie across a block boundary
    c.add_dip(lo=lo, lo_len=20 * (TN + 121) + 300, want_b=(1000 - 2 * (TN + 71 + 50) + 50) % BLOCK, want_kind=NO_END, lo_range=(0, 1 << 30))
    c.flat(TU + 600)
    return _finish(c, "attempt_start", fmt)


def timeouts(fmt):
    """Sixteen NO_DIP time-outs in a row on a constant envelope.  Then dips that begin in the segment the search cuts at the NO_DIP time-out
    and end behind it: at the last comparable position (attempt-relative T_F + 50), 40 samples in front of it, and -- in an attempt that
    restarted mid-block after a NO_END, so that the cut segment is long -- 300 samples in front of it.  Then one that begins a sample behind
    the last position: NO_DIP, and the next attempt finds it under way."""
    c = Craft(fmt, 104)
    lo = 0.0 if fmt != "u8" else 0.01
    c.flat(16 * (TF + 51))
    assert (c.trace()["kind"][1:17] == NO_DIP).all()
    c.add_dip(gap=TF - 500, lo=lo, lo_len=900, want_rel_begin=TF + 50)
    c.add_dip(gap=TF - 500, lo=lo, lo_len=900, want_rel_begin=TF + 50 - 40)
    # a NO_END whose restart lies 600 samples into a block: the segment cut at that attempt's NO_DIP time-out is 651 samples long
    add_no_end_by_one(c, (600 - (TN + 71)) % BLOCK, lo)
    c.add_dip(gap=TF - TU - 1000, lo=lo, lo_len=900, want_rel_begin=TF + 50 - 300)
    r = c.add_dip(gap=TF - 500, lo=lo, lo_len=900, want_rel_begin=TF + 50)   # placed at T_F + 50 ...
    c.amp[r["gap_index"]] = np.ones(len(c.amp[r["gap_index"]]) + 1, np.float32)   # ... and moved one sample on
    c.flat(600)
    # (of the sixteen time-outs the 1st, 2nd, 3rd, 9th and 16th are rested at: a time-out found early or late moves every later one)
    return _finish(c, "timeouts", fmt, keep=lambda tr, k: not (4 <= k <= 15 and k != 9))


def no_end(fmt):
    """a dip whose end is found at counts T_n + 69 and T_n + 70 (the last that is compared), one a sample longer (NO_END)"""
    c = Craft(fmt, 105)
    lo = 0.0 if fmt != "u8" else 0.01
    c.add_dip(lo=lo, lo_len=TN + 20, want_len=TN + 69)
    c.add_dip(lo=lo, lo_len=TN + 20, want_len=TN + 70)
    r = c.add_dip(lo=lo, lo_len=TN + 20, want_len=TN + 70)
    g = r["gap_index"] + 1
    c.amp[g] = np.full(len(c.amp[g]) + 1, lo, np.float32)                    # the same dip one sample longer: T_n + 71 is never compared
    c.flat(TN + TU + 600)
    return _finish(c, "no_end", fmt)


def zeros(fmt):
    """exact zeros: a stretch entered at level zero (the moving sum of exact amplitudes cancels exactly: no walk), the same stretch entered
    after one sample of 1e5 among samples of 1 (the cancellation leaves a residue: the walk must run), zeros that end mid-group, attempts
    restarting inside zeros"""
    assert fmt != "u8"
    c = Craft(fmt, 106)
    spike = FMT_MAX[fmt]
    c.add_dip(lo=0.0, lo_len=4 * (TN + 121) + 500, want_kind=NO_END, lo_range=(0, 1 << 30))
    c.flat(TU + 500)
    c.flat(300, 0.7)                                                         # (0.7 is no dyadic fraction: next to 1e5 its sums round)
    c.append([spike])
    c.flat(9, 0.7)
    c.flat(4 * (TN + 121) + 500, 0.0)
    c.flat(3 * TU)
    # the zeros end mid-group: the last zero at residue 6 of its group in the call that evaluates it
    n2 = sum(len(p) for p in c.amp)
    for extra in range(64):
        n_zero = 3 * (TN + 121) + 100 + extra
        segs = [np.ones(400, np.float32), np.zeros(n_zero, np.float32), np.ones(2 * TU + 600, np.float32)]
        tr = c.trace(segs)
        last_zero = n2 + 400 + n_zero - 1
        rec = next(r for r in simulate(tr, 1 << 40)[1] if r["kind"] == DIP_END and r["end"] is not None and r["end"] > last_zero)
        if (last_zero - rec["call_base"]) % 16 == 6:
            break
    else:
        raise AssertionError("no zero stretch ends at residue 6")
    c.append(*segs)
    return _finish(c, "zeros", fmt, note=dict(last_zero=last_zero))


def _level_now(c):
    """sLevel behind what is built so far, in relative amplitude"""
    x = np.ascontiguousarray(c.values(tail=0))
    return float(ol.oracle().ora_level_walk(x, len(x), np.float32(0.1))) / c.scale


def add_ramps(c, n_ramp=30000):
    """a slow ramp down across 0.55 sLevel and -- inside the same attempt -- one up across 0.75 sLevel: many comparisons near their threshold"""
    n0 = c.built()
    S = _level_now(c)
    ramp = np.linspace(0.60 * S, 0.60 * S - 6.0e-6 * S * n_ramp, n_ramp).astype(np.float32)
    tr = c.trace([ramp])
    rec = next(r for r in simulate(tr, 1 << 40)[1] if r["begin"] is not None and r["begin"] > n0 + 100)
    cut = rec["begin"] - n0 + 300
    assert 1000 < cut < n_ramp
    c.append(ramp[:cut])
    S2 = _level_now(c)
    c.append(np.linspace(0.744 * S2, 0.744 * S2 + 6.0e-6 * S2 * 4000, 4000).astype(np.float32))
    c.flat(TU + 600, float(c.amp[-1][-1]))


def swings(fmt):
    """a step of 60 dB down, one of 60 dB up (the smallest u8 magnitude is 39 dB below the base level: the step is that deep there), and slow
    ramps across both thresholds"""
    c = Craft(fmt, 107, continuous_phase=(fmt == "cf32"))
    c.flat(3000)
    c.flat(5000, 1.0e-3)
    c.flat(4 * TN, 1.0)
    add_ramps(c)
    n_all = c.built()
    tr = c.trace()
    inside = [k for k in range(1, len(tr)) if tr["pos"][k] <= n_all]
    # (the step's first events and everything around the ramps' crossings)
    return _finish(c, "swings", fmt, keep=lambda tr, k: k in inside[:5] + inside[-7:])


def equality(fmt="cf32"):
    """A comparison that is an exact tie: level / 50 == 0.55 sLevel, float for float, at the sample where the dip then begins (a search that
    read `>` as `>=` goes on).  Forty-nine samples at c ~ 0.55 sLevel and a fiftieth searched, one float at a time, until the moving sum
    lands on the tie (not every float is a quotient by 50: the length in front is varied until one is); then straight to three times the level."""
    assert fmt == "cf32"
    L = ol.oracle()
    f = np.float32
    walk = lambda x: f(L.ora_level_walk(np.ascontiguousarray(x, np.complex64), len(x), f(0.1)))   # noqa: E731
    for n_flat in range(30000, 30000 + 17 * 40, 17):
        c = Craft(fmt, 108)
        c.flat(n_flat)
        base = c.values(tail=0)
        cval = f(f(0.55) * walk(base))
        for _ in range(4):                                                   # c follows the level it drags down
            cval = f(f(0.55) * walk(np.concatenate([base, np.full(49, cval, np.complex64)])))
        S49 = walk(np.concatenate([base, np.full(49, cval, np.complex64)]))
        lev = f(50.0)                                                        # fifty samples of exactly 1
        for _ in range(49):
            lev = f(lev + f(cval - f(1.0)))
        v = f(cval * f(1.001))
        for _ in range(40000):
            S50 = f(S49 + f(f(0.00001) * f(v - S49)))
            lev50 = f(lev + f(v - f(1.0)))
            mean, thr = f(lev50 / f(50.0)), f(f(0.55) * S50)
            if mean == thr:
                c.unit[len(base):len(base) + 50] = 1
                c.append(np.full(49, cval, np.float32), [v])
                c.flat(60, 3.0)
                c.flat(TU + 2000)
                return _finish(c, "equality", fmt, note=dict(tie_at=len(base) + 50))
            if mean < thr:
                break
            v = np.nextafter(v, f(0))
    raise AssertionError("no exact tie found")


A_BUILDERS = (grid_residues, grid_special, attempt_start, timeouts, no_end, zeros, swings, equality)
NOT_APPLICABLE = {("zeros", "u8"): "u8 has no code for zero: (c - 127.38) / 128 is never 0",
                  ("equality", "u8"): "the tie needs a sample chosen one float at a time; codes are 1/128 apart",
                  ("equality", "s16"): "the tie needs a sample chosen one float at a time; codes are 1/32768 apart"}


# catalogue entries inside a case that a format cannot hold (the case runs all the same; tests/test_acquire_cases.py skips the entry's assertion)
ENTRY_NOT_APPLICABLE = {
    ("begin at 51 / large sample 49", "s16"): "full scale is 8 x the base level: one sample cannot carry a 50-sample window above 0.55 sLevel",
    ("begin at 51 / large sample 49", "u8"): "full scale is 2 x the base level: one sample cannot carry a 50-sample window above 0.55 sLevel",
    ("residue behind a sample of 1e5", "s16"): "16-bit magnitudes add exactly: the moving sum returns to 0 and the shortcut applies again",
    ("60 dB step", "u8"): "the smallest u8 magnitude is 39 dB below the base level: the step is that deep",
    ("20 margin events", "u8"): "a ramp of codes 1/128 apart is a staircase: no slow crossing"}


@functools.lru_cache(maxsize=None)
def family_a(fmt):
    return tuple(b(fmt) for b in A_BUILDERS if (b.__name__, fmt) not in NOT_APPLICABLE)


# one engine per group of cases (16 .. 48 streams each)
GROUPS = (("grid_residues",), ("grid_special",), ("attempt_start", "no_end", "equality"), ("timeouts", "zeros", "swings"))
# what tests/test_gpu_acquire_stage.py runs per ring format and group: (case, prefix) pairs = streams, and the trace events they walk through
EXPECTED_STREAMS = {"cf32": (36, 31, 34, 31), "s16": (36, 31, 32, 31), "u8": (36, 31, 32, 17)}
EXPECTED_EVENTS = {"cf32": (912, 773, 576, 382), "s16": (912, 773, 571, 382), "u8": (912, 773, 571, 247)}


# ------------------------------------------------------------------------------------------------------------ families B and C
# Chosen from the trace (docs/history/acquire_stage_tests.md): the first real correlation of the -17 350 Hz stream -- before any frequency
# correction -- has ratio 5.48, every later one 143.8 .. 341.4, every crafted one 1.000 .. 1.007.  With 2.5 (5.0 in lock) the real ones are at
# least 2.19 x above and the crafted ones at least 2.48 x below.  The receiver takes the strongest peak (sync_strongest): with the first peak above a threshold
# this low it locks on side lobes of the phase-reference correlation and never decodes a FIB.
C_THRESHOLD, C_STRONGEST = 2.5, 1
C_CFOS = (911.0, -17350.0)


def real_frames(cfo_hz, seed, n_frames, snr_db=30.0):
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(5, subch, seed=seed)
    return ds.channel(ens.iq, snr_db=snr_db, cfo_hz=cfo_hz, timing_offset=1234 + 977 * seed, seed=seed, n_out=n_frames * TF)


def frame_case(name, x, threshold, prefixes=None, note=None, window=None, strongest=0):
    """a case whose oracle run keeps the frame walk and the per-frame scalars; pins on the restable events inside window = (first, last) sample"""
    case = Case(name, "cf32", np.ascontiguousarray(x, np.complex64), threshold=threshold, subch=[], pins=[], note=note, strongest=strongest)
    tr = case.trace
    if prefixes is None:
        ks = [k for k in range(len(tr)) if need_of(int(tr["kind"][k])) is not None and window[0] <= tr["pos"][k] <= window[1]]
        by_stop = {}
        for n in sorted({pin(tr, k) for k in ks if pin(tr, k) <= len(x)}):
            by_stop.setdefault(simulate(tr, n)[0], n)                        # one prefix per event a stream can rest at
        prefixes = sorted(by_stop.values())
    case.prefixes = list(prefixes)
    return case


def family_c_case(cfo_hz):
    """Real frames with a carrier offset, six of them in lock, then a crafted stretch -- block-grid dips, a NO_DIP time-out, large samples and
    slow ramps, a low stretch and exact zeros (seven NO_END) -- carried by one tone that lands on an active carrier behind the receiver's oscillator (its correlation is
    flat: ratio ~1), then the real frames again."""
    real = real_frames(cfo_hz, 11, 18)
    tr0 = ol.oracle_trace(real, C_THRESHOLD, C_STRONGEST)
    done = tr0["pos"][tr0["kind"] == FRAME_DONE]
    p6 = int(done[5])
    before, after = real[:p6], real[p6:p6 + 8 * TF]
    amp = float(np.abs(before[-TF:]).mean())
    c = Craft("cf32", 300, before=before, tone_hz=200000.0 + cfo_hz, scale=amp, threshold=C_THRESHOLD, strongest=C_STRONGEST)
    c.flat(3000)
    want = [(83, 700), (1023, 16), (527, 1008), (16, 1), (1007, 330)]
    for wb, we in want:
        c.add_dip(want_b=wb, want_e=we, lo=0.0)
    c.flat(TF + 200)                                                         # NO_DIP
    # Eight large samples, then slow ramps across both thresholds.  |x osc| and |x| differ in the last place of a float now and then; at
    # 1e4 times the level that last place is worth 1e-3 of the level, it stays in the moving sum as a residue when the sample leaves the
    # window, and the ramps turn it into a different sample of the dip's begin and end: what tells the envelope in front of the oscillator
    # product from the one behind it
    for i in range(8):                                                       # (40 apart: one of them is always in the window, no dip in between)
        c.append([1.0e4 * (1 + 0.1 * i)])
        c.flat(40, 1.5)
    c.flat(200, 0.6 * _level_now(c))                                         # the level has doubled: stay above 0.55 of it until the ramp
    add_ramps(c)
    c.add_dip(lo=0.02, lo_len=3 * (TN + 121) + 300, want_kind=NO_END, lo_range=(0, 1 << 30))
    c.add_dip(lo=0.0, lo_len=2 * (TN + 121) + 300, want_kind=NO_END, lo_range=(0, 1 << 30))
    c.flat(1500)
    n_end = c.built()
    c.after = after
    return frame_case("lock_cfo_%d" % round(cfo_hz), c.codes(), C_THRESHOLD, window=(p6 - 2 * TF - 100, n_end + 4 * TF), strongest=C_STRONGEST,
                      note=dict(p6=p6, n_end=n_end, want=want))


@functools.lru_cache(maxsize=None)
def family_c():
    return tuple(family_c_case(f) for f in C_CFOS)


B_THRESHOLD = 3.0


@functools.lru_cache(maxsize=None)
def family_b():
    """Edges of the frame chain: a carrier offset just inside and just outside the +-35 kHz the reference follows, and a null symbol 40
    samples short / 40 samples long (the clock-error estimate beyond its clamp of +-307.2 Hz, both signs)."""
    cases = []
    for cfo in (34900.0, 35400.0):
        x = real_frames(cfo, 21, 14)
        cases.append(frame_case("cfo_%d" % round(cfo), x, B_THRESHOLD, prefixes=[len(x)]))
    x = real_frames(300.0, 22, 21)
    sym0 = ol.oracle_run(x, [], config=(B_THRESHOLD, 0, 1))["sym0"]
    cut, ins = int(sym0[8]) - ds.TG - 1500, int(sym0[14]) - ds.TG - 1500
    x = np.concatenate([x[:cut], x[cut + 40:ins], x[ins:ins + 40], x[ins:]])
    cases.append(frame_case("null_symbol_40_short_40_long", x, B_THRESHOLD, prefixes=[len(x)]))
    return tuple(cases)
EXPECTED_C_STREAMS = 22                      # per carrier offset
EXPECTED_C_EVENTS = (598, 139)               # trace events walked through and frames compared, per carrier offset
