"""The scope section of the bulk delivery (DABX_DELIVER_SCOPE, dabx_chunk_header_ext.off_scope, dabx_chunk_scope; deliver.hip k_deliver_records)
and k_scope inside the running engine, through IQ: two streams of one FIC-only engine, stream 1 with the mode on (OFDM symbol 4 of every
decoded frame, so a chunk of seven frames fills its seven record slots), a consumer thread beside dabx_process calls of 5, 7, 3 and 6 frames.
The slab's records and vectors are dabx_read_scope's of the same engine, byte for byte; the few-stream schedule (k_scope on the demapper's
HIP stream, behind the same sequence-number wait as k_demap_whole) makes the same records as the serial one; without the bit nothing of a
slab changes."""
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
S, F, ON = 2, 7, 1
MODE = dict(iq_type=0, carrier_type=8, symbol=4)          # PHASE_CORR_CARR_NORMED, REL_POWER (the prefix scan), the first MSC symbol


def signals():
    subch = ds.default_subchannels(2, 64)
    xs = []
    for s in range(S):
        ens = ds.build_ensemble(10, subch, seed=60 + s)
        xs.append(ds.channel(ens.iq, snr_db=25.0, cfo_hz=40.0 * s, timing_offset=3000 + 777 * s, seed=s, n_out=21 * ds.TF).copy())
    return xs


class Sink(threading.Thread):
    """The consumer thread: keeps a copy of every slab and of what Chunk.scope returns."""

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
                self.chunks.append(dict(raw=ch.raw.copy(), header=ch.header.copy(), ext=None if ch.header_ext is None else ch.header_ext.copy(),
                                        table=None if ch.scope_table is None else ch.scope_table.copy(),
                                        scope=[[(r.tobytes(), iq.copy(), carr.copy()) for r, iq, carr in ch.scope(s)] for s in range(S)]))
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


def run_bulk(xs, what, mode, schedule=1, after=None):
    """One engine with the delivery open: (chunks, per stream the records read_scope gave after every call, slab bytes, scope stats, frames)"""
    # acquire_mode 1, schedule 1: what a step does to a stream does not depend on timing, and slabs are compared byte by byte (tests/test_gpu_tii_delivery.py)
    eng = dx.Engine(n_streams=S, ring_frames=23, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, schedule=schedule)
    try:
        for s, x in enumerate(xs):
            eng.push_iq(s, x)
        if mode:
            eng.set_scope_mode(ON, **MODE)
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
                    recs, lost = eng.read_scope(s)
                    assert lost == 0
                    read[s] += [(r.tobytes(), iq.copy(), carr.copy()) for r, iq, carr in recs]
            eng.synchronize()
        finally:
            sink.finish()
        assert sink.error is None and eng.delivery_next(wait=False) is None
        stats = [eng.scope_stats(s) for s in range(S)]
        frames = [eng.stats(s)["frames"] for s in range(S)]
        if after:
            after(eng)
        eng.delivery_close()
    finally:
        eng.close()
    return sink.chunks, read, slab, stats, frames


@pytest.fixture(scope="module")
def world():
    """The signals and the runs: computed once, shared, left unchanged."""
    xs = signals()

    def refusals(eng):
        for what in (dx.DELIVER_SCOPE, dx.DELIVER_SCOPE | dx.DELIVER_TII, dx.DELIVER_SCOPE | dx.DELIVER_ETI | dx.DELIVER_AAC | dx.DELIVER_MP2_AUDIO,
                     4096, 4096 | dx.DELIVER_FIB, 1024 | dx.DELIVER_FIB, 4096 | dx.DELIVER_SCOPE | dx.DELIVER_FIB, 16384 | dx.DELIVER_FIB):
            with pytest.raises(dx.DabxError, match="error -2"):          # DABX_E_ARG
                eng.delivery_open(slots=4, what=what)

    w = dict(xs=xs)
    w["scope"] = run_bulk(xs, dx.DELIVER_FIB | dx.DELIVER_SCOPE, True, after=refusals)
    w["scope_few"] = run_bulk(xs, dx.DELIVER_FIB | dx.DELIVER_SCOPE, True, schedule=0)
    w["fib"] = run_bulk(xs, dx.DELIVER_FIB, False)
    w["fib_mode"] = run_bulk(xs, dx.DELIVER_FIB, True)
    w["zero"] = run_bulk(xs, 0, False)
    w["zero_mode"] = run_bulk(xs, 0, True)
    return w


def records_of(chunks, s):
    return [r for q in chunks for r in q["scope"][s]]


def test_the_slabs_records_are_read_scopes_byte_for_byte(world):
    chunks, read, _, stats, frames = world["scope"]
    assert len(chunks) == sum((m + 6) // 7 for m in CALLS)
    a, b = records_of(chunks, ON), read[ON]
    assert len(a) == len(b) == stats[ON]["shows"] and len(a) >= 10 and frames[ON] >= len(a)
    for (r, iq, carr), (r2, iq2, carr2) in zip(a, b):
        assert r == r2 and iq.tobytes() == iq2.tobytes() and carr.tobytes() == carr2.tobytes()
    recs = np.frombuffer(b"".join(r for r, _, _ in a), dx.SCOPE_RECORD)
    assert (np.diff(recs["frame"]) == 1).all() and (recs["symbol"] == MODE["symbol"]).all() and (recs["carrier_type"] == MODE["carrier_type"]).all()
    assert (recs["iq_type"] == MODE["iq_type"]).all() and (recs["soft_bit_type"] == 1).all() and not recs["reserved"].any()
    # a locked stream at 25 dB: the constellation normed per carrier sits on the four points, the relative power near 0 dB
    iq, carr = a[-1][1], a[-1][2]
    assert np.isfinite(iq.view(np.float32)).all() and np.isfinite(carr).all()
    assert abs(float(np.median(np.abs(iq))) - 1.0) < 0.1 and abs(float(np.median(carr))) < 1.0
    assert np.median(np.abs(np.abs(iq.real) - np.abs(iq.imag))) < 0.2
    # every record is in a chunk: none lost, the tables count on from chunk to chunk; a full chunk fills its seven slots
    nxt = 0
    for q in chunks:
        r = q["table"][ON]
        assert int(r["records_lost"]) == 0 and int(r["first_record"]) == nxt and int(r["n_records"]) <= F
        nxt += int(r["n_records"])
        assert int(r["records_total"]) == nxt
    assert nxt == len(a) and max(int(q["table"][ON]["n_records"]) for q in chunks) == F
    assert stats[ON]["launches"] == sum(CALLS) and stats[ON]["lost"] == 0


def test_the_stream_without_the_mode_delivers_nothing(world):
    chunks, read, _, stats, _ = world["scope"]
    assert records_of(chunks, 1 - ON) == [] and read[1 - ON] == [] and stats[1 - ON]["shows"] == 0
    for q in chunks:
        r = q["table"][1 - ON]
        assert (int(r["n_records"]), int(r["records_lost"]), int(r["rec_off"]), int(r["records_total"])) == (0, 0, 0, 0)


def test_the_few_stream_schedule_makes_the_same_records(world):
    """schedule 0 with two streams: both demapper launches on their own HIP stream with device-side hand-overs, k_scope in front of them."""
    a, b = records_of(world["scope"][0], ON), records_of(world["scope_few"][0], ON)
    n = min(len(a), len(b))
    assert n >= 10 and abs(len(a) - len(b)) <= 2              # (a call that queues its steps may lock a step later: the same frames, fewer of them)
    for (r, iq, carr), (r2, iq2, carr2) in zip(a[:n], b[:n]):
        assert r == r2 and iq.tobytes() == iq2.tobytes() and carr.tobytes() == carr2.tobytes()


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
    assert all(st == dict(shows=0, lost=0, launches=0) for st in stats) and stats2[ON]["launches"] == sum(CALLS)
    assert len(chunks) == len(chunks2)
    for q, q2 in zip(chunks, chunks2):
        assert q["ext"] is None and q["table"] is None and int(q["header"]["off_stream"]) == 128 and not int(q["header"]["what"]) & dx.DELIVER_SCOPE
        assert len(q["raw"]) == slab and q["raw"].tobytes() == q2["raw"].tobytes()      # k_scope beside it changes no delivered byte
    # ... while the engine with the mode on made the very records of the delivery with the bit
    assert [r for r, _, _ in read2[ON]] == [r for r, _, _ in records_of(world["scope"][0], ON)]
    assert all(a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() for a, b in zip(read2[ON], records_of(world["scope"][0], ON)))


def test_with_the_bit_the_extension_announces_the_section(world):
    chunks, _, slab, _, _ = world["scope"]
    plain = world["fib"][0]
    off_scope = head_bytes(True)
    assert slab == (off_scope + S * 32 + F * dx.SCOPE_SLOT_BYTES + 255) // 256 * 256            # room for the one stream with the mode on
    for q, p in zip(chunks, plain):
        h, x = q["header"], q["ext"]
        assert int(h["off_stream"]) == 192 and int(h["what"]) == dx.DELIVER_FIB | dx.DELIVER_SCOPE and int(h["bytes"]) == slab
        assert int(x["magic"]) == dx.CHUNK_EXT_MAGIC and int(x["bytes"]) == 64 and int(x["off_scope"]) == off_scope
        assert not x["reserved"].any() and not int(x["off_tii"]) and not int(x["off_mp2_audio"]) and not int(x["off_aac"])
        assert int(q["table"][ON]["rec_off"]) == off_scope + S * 32
        # the FIB section, the CRC flags, the frame records and the stream table: the bytes of the engine without the bit
        for k, n in (("off_fib", S * F * 384), ("off_crc", S * F * 12), ("off_frame", S * F * 16), ("off_stream", S * 72)):
            a, b = int(h[k]), int(p["header"][k])
            assert a == b + 64 and q["raw"][a:a + n].tobytes() == p["raw"][b:b + n].tobytes(), k
