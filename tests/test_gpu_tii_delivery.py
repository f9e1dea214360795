"""The TII stage of the engine (dabx_set_tii_mode, deliver.hip k_tii) and its section of the bulk delivery (DABX_DELIVER_TII, dabx_chunk_header_ext,
dabx_chunk_tii; deliver.hip k_deliver_tii), through IQ: four streams of one FIC-only engine -- three ETSI transmitters, a non-ETSI one beside
an ETSI one, an ensemble without any TII signal, and one whose IQ has a silence that loses the lock after the first event --, min_frames
= 2, a consumer thread beside dabx_process calls of 5, 7, 3 and 6 frames.  The events over the chunks are what a second engine gives
that is stepped frame by frame with dabx_read_tii(min_frames = 2) after every frame -- the host detector, pinned to the reference's object
code --, and what dabx_read_tii_events of the same engine gives; without the bit nothing of a slab changes."""
import os
import sys
import threading

import numpy as np
import pytest

from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = (5, 7, 3, 6)
S, F, THR, MIN_FRAMES = 4, 7, 8, 2
GAP = 3                                   # the stream with the silence
# the float tolerance of tests/test_gpu_tii_stage.py (measured there and here, docs/history/tii_device.md)
from test_gpu_tii_stage import REL_TOL, DEG_TOL  # noqa: E402
WORST = {"rel": 0.0, "deg": 0.0}


def signals():
    subch = ds.default_subchannels(2, 64)
    tx = [[(3, 1, 1.0, True), (40, 17, 0.6, True), (69, 23, 0.3, True)], [(25, 9, 1.0, False), (7, 2, 0.7, True)], None, [(12, 5, 1.0, True)]]
    xs = []
    for s in range(S):
        ens = ds.build_ensemble(10, subch, seed=80 + s, tii=tx[s])
        xs.append(ds.channel(ens.iq, snr_db=25.0, cfo_hz=40.0 * s, timing_offset=3000 + 777 * s, seed=s, n_out=21 * ds.TF).copy())
    xs[GAP][int(8.3 * ds.TF):int(10.1 * ds.TF)] = 0
    return xs


class Sink(threading.Thread):
    """The consumer thread: keeps a copy of every slab and of what Chunk.tii returns."""

    def __init__(self, eng):
        super().__init__(daemon=True)
        self.eng, self.chunks = eng, []
        self.want, self.seq, self.error = 0, 0, None
        self.cv = threading.Condition()

    def run(self):
        try:
            while True:
                with self.cv:
                    self.cv.wait_for(lambda: self.want > self.seq or self.want < 0)
                    if self.want < 0:
                        return
                ch = self.eng.delivery_next(wait=True)
                if ch is None:
                    continue
                assert ch.seq == self.seq
                q = dict(raw=ch.raw.copy(), header=ch.header.copy(), ext=None if ch.header_ext is None else ch.header_ext.copy(),
                         table=None if ch.tii_table is None else ch.tii_table.copy(),
                         tii=[[(ev.copy(), res.copy()) for ev, res in ch.tii(s)] for s in range(S)])
                self.chunks.append(q)
                ch.release()
                with self.cv:
                    self.seq += 1
                    self.cv.notify_all()
        except BaseException as ex:              # noqa: B036 (kept for the test's thread to raise)
            self.error = ex
            with self.cv:
                self.cv.notify_all()

    def expect(self, chunks):
        with self.cv:
            self.want += chunks
            self.cv.notify_all()
            assert self.cv.wait_for(lambda: self.seq >= self.want or self.error is not None, timeout=60), "the consumer did not get its chunks"
        if self.error is not None:
            raise self.error

    def finish(self):
        with self.cv:
            self.want = -1
            self.cv.notify_all()
        self.join(10)


def engine(xs, schedule=1):
    # acquire_mode 1: the search runs in step, so that what a step does to a stream does not depend on timing.  schedule 1 (every kernel on
    # the front-end stream): in the overlapped schedule the demapper of the MSC symbols, on its own HIP stream, writes the SNR and MER estimates
    # of the stream table while a chunk may be closing, and which frame's estimate a slab shows depends on timing -- here slabs are
    # compared byte by byte.  The events do not depend on the schedule: one run below has the default one.
    eng = dx.Engine(n_streams=S, ring_frames=23, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, schedule=schedule)
    for s, x in enumerate(xs):
        eng.push_iq(s, x)
    return eng


def run_bulk(xs, what, mode, after=None, schedule=1):
    """One engine with the delivery open: (chunks, per stream the events read_tii_events gave after every call, slab bytes, stats of stream 0, after(eng))"""
    eng = engine(xs, schedule)
    try:
        if mode:
            eng.set_tii_mode(-1, min_frames=MIN_FRAMES, threshold_db=THR)
        eng.delivery_open(slots=4, what=what)
        slab = eng.delivery_slab_bytes()
        sink = Sink(eng)
        read = [[] for _ in range(S)]
        sink.start()
        try:
            for m in CALLS:
                eng.process(m, sync=False)
                sink.expect((m + 6) // 7)
                for s in range(S):
                    evs, lost = eng.read_tii_events(s)
                    assert lost == 0
                    read[s] += [(ev.copy(), res.copy()) for ev, res in evs]
            eng.synchronize()
        finally:
            sink.finish()
        assert sink.error is None and eng.delivery_next(wait=False) is None
        stats = [dict(eng.tii_stats(s), frames=eng.stats(s)["frames"]) for s in range(S)]
        extra = after(eng) if after else None
        eng.delivery_close()
    finally:
        eng.close()
    return sink.chunks, read, slab, stats, extra


def run_stepped(xs):
    """The host path, frame by frame: per stream the events as (frame, frames_in_sum, epoch, results of the host detector (up to 64), the sum)"""
    eng = engine(xs)
    out = [[] for _ in range(S)]
    try:
        # (a few steps more than the calls have: a call that queues its steps sees a loss of lock later than one that waits after every step, and
        #  starts the search a step or two later -- the same frames, some of them in later steps)
        for _ in range(sum(CALLS) + 4):
            eng.process(1)
            for s in range(S):
                fr = dx.front_read(eng, s, spectra=False)
                if fr["tii_cnt"][0] >= MIN_FRAMES:
                    res, k = eng.read_tii(s, min_frames=MIN_FRAMES, threshold_db=THR)
                    assert k == fr["tii_cnt"][0]
                    out[s].append((eng.stats(s)["frames"] - 1, k, int(fr["tii_cnt"][1]), res, fr["tii_acc"].copy()))
    finally:
        eng.close()
    return out


def same_results(res, n_found, want, where):
    assert n_found == len(want) and len(res) == min(len(want), dx.TII_MAX_RESULTS), (where, len(res), n_found, len(want))
    got = dx._tii_tuples(res)
    assert [(g[0], g[1], g[4]) for g in got] == [(w[0], w[1], w[4]) for w in want[:len(got)]], where
    for g, w in zip(got, want):
        rel = abs(np.float32(g[2]) - np.float32(w[2])) / abs(w[2])
        deg = abs((float(np.float32(g[3])) - float(np.float32(w[3])) + 180.0) % 360.0 - 180.0)
        WORST["rel"], WORST["deg"] = max(WORST["rel"], float(rel)), max(WORST["deg"], deg)
        assert rel <= REL_TOL and deg <= DEG_TOL, (where, g, w, rel, deg)


@pytest.fixture(scope="module")
def world():
    """The signals and the runs: computed once, shared, left unchanged."""
    xs = signals()

    def old_path(eng):
        with pytest.raises(dx.DabxError, match="error -5"):          # DABX_E_STATE: the device's detector owns the sum
            eng.read_tii(1, min_frames=MIN_FRAMES, threshold_db=THR)
        with pytest.raises(dx.DabxError, match="error -2"):          # DABX_E_ARG: the bit alone names nothing a chunk is made of
            eng.delivery_open(slots=4, what=dx.DELIVER_TII)
        eng.set_tii_mode(1, enable=False)
        on_1 = eng.read_tii(1, min_frames=1000)                       # ... and with the mode switched off again the host path works
        with pytest.raises(dx.DabxError, match="error -5"):
            eng.read_tii(0, min_frames=MIN_FRAMES)
        return on_1

    w = dict(xs=xs, stepped=run_stepped(xs))
    w["tii"] = run_bulk(xs, dx.DELIVER_FIB | dx.DELIVER_TII, True, after=old_path)
    w["fib"] = run_bulk(xs, dx.DELIVER_FIB, False)
    w["fib_mode"] = run_bulk(xs, dx.DELIVER_FIB, True)
    w["zero"] = run_bulk(xs, 0, False)
    w["zero_mode"] = run_bulk(xs, 0, True)
    w["tii_overlapped"] = run_bulk(xs, dx.DELIVER_FIB | dx.DELIVER_TII, True, schedule=0)
    return w


def events_of(chunks, s):
    return [e for q in chunks for e in q["tii"][s]]


def test_the_events_are_the_host_paths_frame_by_frame(world):
    chunks = world["tii"][0]
    assert len(chunks) == sum((m + 6) // 7 for m in CALLS)
    for s in range(S):
        got, want = events_of(chunks, s), world["stepped"][s]
        # every event the stepped engine completed within the frames this engine decoded, and no other
        decoded = world["tii"][3][s]["frames"]
        want = [w for w in want if w[0] < decoded]
        assert len(got) == len(want) and len(want) >= (2 if s == GAP else 3), (s, len(got), len(want), decoded)
        for k, ((ev, res), (frame, in_sum, epoch, hres, _)) in enumerate(zip(got, want)):
            assert (int(ev["frame"]), int(ev["frames_in_sum"]), int(ev["epoch"]), int(ev["threshold_db"])) == (frame, in_sum, epoch, THR), (s, k, ev)
            assert in_sum == MIN_FRAMES and int(ev["n_results"]) == len(res)
            same_results(res, int(ev["n_found"]), hres, (s, k))
    assert {(m, c, e) for m, c, _, _, e in dx._tii_tuples(events_of(chunks, 0)[-1][1])} == {(3, 1, 0), (40, 17, 0), (69, 23, 0)}
    assert {(m, c, e) for m, c, _, _, e in dx._tii_tuples(events_of(chunks, 1)[-1][1])} == {(25, 9, 1), (7, 2, 0)}
    print("largest deviation from the host detector: %.3g relative, %.3g degrees" % (WORST["rel"], WORST["deg"]))


def test_the_chunks_events_are_read_tii_events_of_the_same_engine(world):
    chunks, read, _, stats, _ = world["tii"]
    for s in range(S):
        a, b = events_of(chunks, s), read[s]
        assert len(a) == len(b)
        for (ev, res), (ev2, res2) in zip(a, b):
            assert ev.tobytes() == ev2.tobytes() and np.array_equal(res, res2)     # (field by field: a copy of a record array drops its padding)
        assert stats[s]["events"] == len(a) and stats[s]["results"] == sum(len(r) for _, r in a) and stats[s]["truncated"] == 0
        assert stats[s]["launches"] == sum(CALLS)
        # every event is in a chunk: none lost, the tables count on from chunk to chunk
        nxt = 0
        for q in chunks:
            r = q["table"][s]
            assert int(r["events_lost"]) == 0 and int(r["first_event"]) == nxt and int(r["n_events"]) <= 4
            nxt += int(r["n_events"])
            assert int(r["events_total"]) == nxt
        assert nxt == len(a)


def test_the_overlapped_schedule_makes_the_same_events(world):
    for s in range(S):
        a, b = events_of(world["tii"][0], s), events_of(world["tii_overlapped"][0], s)
        assert len(a) == len(b)
        for (ev, res), (ev2, res2) in zip(a, b):
            assert ev.tobytes() == ev2.tobytes() and np.array_equal(res, res2)


def test_an_ensemble_without_tii_still_has_events_with_no_result(world):
    ev = events_of(world["tii"][0], 2)
    assert ev and any(int(e["n_results"]) == 0 and len(r) == 0 for e, r in ev)


def test_a_loss_of_lock_clears_the_detectors_state(world):
    ev, host = events_of(world["tii"][0], GAP), world["stepped"][GAP]
    epochs = [int(e["epoch"]) for e, _ in ev]
    assert epochs[0] < epochs[-1]
    k = next(i for i, p in enumerate(epochs) if p != epochs[0])
    assert k >= 1                                            # the first event lies in front of the silence
    # the first event after it: what a detector that has never seen a sum makes of that event's sum
    det = dx.Tii()
    det.add(host[k][4])
    fresh = det.process(THR)
    det.close()
    same_results(ev[k][1], int(ev[k][0]["n_found"]), fresh, ("fresh", k))
    assert fresh and [r[:2] for r in fresh] == [(12, 5)]
    # (the search in front of the first lock moves the epoch too: every stream's first event counts one reset, this stream's later one another)
    resets = [world["tii"][3][s]["resets"] for s in range(S)]
    assert resets[GAP] == 2 and all(resets[s] == 1 for s in range(S) if s != GAP), resets
    for s in range(S):
        if s != GAP:
            assert len({int(e["epoch"]) for e, _ in events_of(world["tii"][0], s)}) == 1


def test_the_old_path_is_refused_only_where_the_mode_is_on(world):
    res, k = world["tii"][4]
    assert res == [] and k >= 0


def head_bytes(ext):
    n = 128 + (64 if ext else 0)
    a16 = lambda v: (v + 15) // 16 * 16   # noqa: E731
    n = a16(n + S * 72)
    n = a16(n + S * 1 * 144)
    n = a16(n + S * F * 384)
    n = a16(n + S * F * 12)
    n = a16(n + S * F * 16)
    return n


@pytest.mark.parametrize("what", ["fib", "zero"])
def test_without_the_bit_a_slab_is_what_it_was(world, what):
    chunks, _, slab, stats, _ = world[what]
    chunks2, read2, slab2, stats2, _ = world[what + "_mode"]
    assert slab == slab2 == (head_bytes(False) + 255) // 256 * 256
    assert all(st["launches"] == 0 and st["events"] == 0 for st in stats) and all(st["launches"] == sum(CALLS) for st in stats2)
    assert len(chunks) == len(chunks2)
    for q, q2 in zip(chunks, chunks2):
        assert q["ext"] is None and q["table"] is None and int(q["header"]["off_stream"]) == 128 and not int(q["header"]["what"]) & dx.DELIVER_TII
        assert len(q["raw"]) == slab and q["raw"].tobytes() == q2["raw"].tobytes()      # the detectors beside it change no delivered byte
    # ... while the engine with the mode on made the very events of the delivery with the bit
    for s in range(S):
        assert [e.tobytes() for e, _ in read2[s]] == [e.tobytes() for e, _ in events_of(world["tii"][0], s)]


def test_with_the_bit_the_extension_announces_the_section(world):
    chunks, _, slab, _, _ = world["tii"]
    plain = world["fib"][0]
    off_tii = head_bytes(True)
    assert slab == (off_tii + S * (32 + 4 * dx.TII_EVENT_SLOT_BYTES) + 255) // 256 * 256
    for q, p in zip(chunks, plain):
        h, x = q["header"], q["ext"]
        assert int(h["off_stream"]) == 192 and int(h["what"]) == dx.DELIVER_FIB | dx.DELIVER_TII and int(h["bytes"]) == slab
        assert int(x["magic"]) == dx.CHUNK_EXT_MAGIC and q["raw"][128:132].tobytes() == b"DBXE" and int(x["bytes"]) == 64
        assert int(x["off_tii"]) == off_tii and not x["reserved"].any()
        for s in range(S):
            assert int(q["table"][s]["ev_off"]) == off_tii + S * 32 + s * 4 * dx.TII_EVENT_SLOT_BYTES
        # the FIB section, the CRC flags, the frame records and the stream table: the bytes of the engine without the bit
        for k, n in (("off_fib", S * F * 384), ("off_crc", S * F * 12), ("off_frame", S * F * 16), ("off_stream", S * 72)):
            a, b = int(h[k]), int(p["header"][k])
            assert a == b + 64 and q["raw"][a:a + n].tobytes() == p["raw"][b:b + n].tobytes(), k
