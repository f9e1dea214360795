"""The ETI stage of the bulk delivery (DABX_DELIVER_ETI, include/dabx.h dabx_chunk_eti; deliver.hip k_eti_*), through IQ: three streams of
one engine -- 18 x 64 kbit/s DAB+ whose CIF counter wraps, a small mixed layout with a slot that is not DAB+ and a short-form profile,
noise that never locks --, out_frames = 8, a consumer thread beside dabx_process calls of 5, 7, 3 and 6 frames.  The rows over the chunks
are dabx_read_eti's frames of the same engine and the oracle's assembly, byte for byte; without the bit nothing of a slab changes."""
import os
import sys
import threading

import numpy as np
import pytest

import oracle_lib as ol
import stage_driver as sd
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = (5, 7, 3, 6)
ALL3 = dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF


class EtiSink(threading.Thread):
    """The consumer thread (the interface of delivery_sink.Sink): keeps, per chunk, a copy of the whole slab and what Chunk's readers return."""

    def __init__(self, eng, S, M):
        super().__init__(daemon=True)
        self.eng, self.S, self.M = eng, S, M
        self.chunks = []
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
                h = ch.header
                q = dict(raw=ch.raw.copy(), header=h.copy(), streams=ch.streams.copy(), subch=ch.subch.copy(), eti=[], rows=[], msc={}, sf={}, sfi={})
                assert (ch.eti_table is None) == (int(h["off_eti"]) == 0)
                for s in range(self.S):
                    r, rows = ch.eti(s)
                    q["eti"].append(None if r is None else r.copy()); q["rows"].append(rows.copy())
                    for j in range(self.M):
                        if h["what"] & dx.DELIVER_MSC:
                            q["msc"][(s, j)] = ch.msc(s, j).copy()
                        if h["what"] & dx.DELIVER_SF:
                            q["sf"][(s, j)] = ch.superframes(s, j).copy(); q["sfi"][(s, j)] = ch.superframe_info(s, j).copy()
                if h["what"] & dx.DELIVER_FIB:
                    q["fibs"], q["crc"], q["frames"] = ch.fibs.copy(), ch.crc.copy(), ch.frames.copy()
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

    def rows(self, s):
        return np.concatenate([q["rows"][s] for q in self.chunks])


def run(streams, what, calls=CALLS, before=None, between=None, profile=False, **engine_args):
    """streams = [(x, subch)]: one engine, the delivery opened with `what` (after before(eng), if given), the calls with the consumer beside
    them and dabx_read_eti of every stream after every call.  Returns (sink, per stream the frames dabx_read_eti returned, frames decoded
    per stream, dabx_delivery_slab_bytes, kernel launches)."""
    S, M = len(streams), max(1, max(len(c) for _, c in streams))
    # acquire_mode 1: the search of the stream that never locks runs in step, so that its scalars in a slab do not depend on timing
    eng = dx.Engine(n_streams=S, ring_frames=23, max_subch=M, out_frames=8, acquire_mode=1, **engine_args)
    try:
        if profile:
            dx.check(dx.load().dabx_set_profiling(eng._h, 1))
        for s, (x, subch) in enumerate(streams):
            if subch:
                eng.set_subchannels(subch, stream=s)
            eng.push_iq(s, x)
        if before:
            before(eng)
        eng.delivery_open(slots=4, what=what)
        slab = eng.delivery_slab_bytes()
        sink = EtiSink(eng, S, M)
        read = [[] for _ in range(S)]
        sink.start()
        try:
            for i, m in enumerate(calls):
                if between:
                    between(eng, i)
                eng.process(m, sync=False)
                sink.expect((m + 6) // 7)
                for s in range(S):
                    f, lost = eng.read_eti(s, 64)
                    assert lost == 0
                    read[s].append(f)
            eng.synchronize()
        finally:
            sink.finish()
        assert sink.error is None and eng.delivery_next(wait=False) is None
        frames = [eng.stats(s)["frames"] for s in range(S)]
        launches = sd.kernel_launches(eng) if profile else None
        eng.delivery_close()
    finally:
        eng.close()
    return sink, [np.concatenate(r) for r in read], frames, slab, launches


def mixed_subchannels():
    uep = (ol.ora_uep_map(32, 3)[1] >= 0).astype(np.uint8)
    return [ds.SubCh(3, 0, 24, 32, 3, 1, mask=uep, dab_plus=0),                    # UEP 32k level 3 (short form), not DAB+
            ds.SubCh(7, 30, 48, 32, 0, 0), ds.SubCh(33, 300, 48, 64, 2, 0)]         # EEP 1-A, EEP 3-A


@pytest.fixture(scope="module")
def world():
    """The signals, the oracle receiver's results, and the run with the bit beside FIB | MSC | SF: computed once, shared, left unchanged."""
    sub0, sub1 = ds.default_subchannels(18, 64), mixed_subchannels()
    ens0 = ds.build_ensemble(10, sub0, seed=12, cif_start=240)           # the CIF counter wraps 249 -> 0 inside the run
    x0 = ds.channel(ens0.iq, snr_db=22.0, cfo_hz=77.0, timing_offset=2222, seed=4, n_out=22 * ds.TF)
    ens1 = ds.build_ensemble(10, sub1, seed=31)
    x1 = ds.channel(ens1.iq, snr_db=20.0, cfo_hz=-410.0, timing_offset=7001, seed=8, n_out=22 * ds.TF)
    rng = np.random.default_rng(3)
    x2 = (0.05 * (rng.standard_normal(22 * ds.TF) + 1j * rng.standard_normal(22 * ds.TF))).astype(np.complex64)
    streams = [(x0, sub0), (x1, sub1), (x2, [])]
    w = dict(streams=streams, ora=[ol.oracle_run(x0, sub0), ol.oracle_run(x1, sub1)])
    w["with"] = run(streams, ALL3 | dx.DELIVER_ETI, profile=True)
    return w


def oracle_rows(ora, subch, n_rows):
    """The ETI frames of CIFs 16 .. 16 + n_rows - 1 from the oracle receiver's FIBs and logical frames (oracle/eti.c)."""
    descs = [dx.SubchDesc(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, 1, 0) for c in subch]
    out = np.zeros((n_rows, 6144), np.uint8)
    for i in range(n_rows):
        r = 16 + i
        F, k = divmod(r, 4)
        fib = ora["fibs"][F].reshape(-1)
        hi, lo = int(fib[4] & 0x1F), int(fib[5])                          # FIG 0/0 leads FIB 0 of every CIF in the synthetic
        for g in range(4):                                                # ensemble: the state after the frame is FIB 9's
            if ora["crc"][F][3 * g]:
                hi, lo = int(ora["fibs"][F][3 * g][4] & 0x1F), int(ora["fibs"][F][3 * g][5])
        msc = [ora["msc"][j].reshape(-1, 3 * c.kbps)[r - 16] for j, c in enumerate(subch)]
        out[i], _ = ol.ora_eti_frame(hi, lo, k, descs, fib[96 * k:96 * k + 96], msc)
    return out


def check_bookkeeping(sink, frames):
    """(b) 4 * frames - 16 rows per locked stream, (c) first_cif consecutive and nothing lost, (d) the noise stream has none"""
    for s in range(3):
        nxt, total = None, 0
        for q in sink.chunks:
            r = q["eti"][s]
            assert r["cifs_lost"] == 0 and r["cifs_refused"] == 0 and 0 <= r["n_eti"] <= 28 and len(q["rows"][s]) == r["n_eti"]
            assert int(r["rows_off"]) + 28 * 6144 <= int(q["header"]["bytes"]) and int(r["rows_off"]) >= int(q["header"]["off_msc"])
            if nxt is not None:
                assert r["first_cif"] == nxt, (s, int(r["first_cif"]), nxt)
            nxt = int(r["first_cif"]) + int(r["n_eti"])
            total += int(r["n_eti"])
            if s == 2:
                assert r["n_eti"] == 0 and r["cifs_waiting"] == 0
        if s < 2:
            assert frames[s] >= 20 and total == 4 * frames[s] - 16 and nxt == 4 * frames[s], (s, frames[s], total)
            assert sum(int(q["eti"][s]["cifs_waiting"]) for q in sink.chunks) == 16        # the de-interleavers' fill
            last = sink.chunks[-1]["eti"][s]
            assert last["fib_frames"] == frames[s] and 0 <= last["cif_hi"] < 32 and 0 <= last["cif_lo"] < 250
    assert frames[2] == 0


def test_rows_are_read_etis_frames_and_the_oracles_assembly(world):
    """(a) - (d)"""
    sink, read, frames, slab, launches = world["with"]
    assert len(sink.chunks) == 4 and all(int(q["header"]["what"]) == ALL3 | dx.DELIVER_ETI and int(q["header"]["off_eti"]) for q in sink.chunks)
    check_bookkeeping(sink, frames)
    for s in range(2):
        rows = sink.rows(s)
        assert rows.shape == read[s].shape == (4 * frames[s] - 16, 6144)
        assert np.array_equal(rows, read[s]), (s, np.flatnonzero((rows != read[s]).any(axis=1))[:4])
        want = oracle_rows(world["ora"][s], world["streams"][s][1], len(rows))
        assert np.array_equal(rows, want), (s, np.flatnonzero((rows != want).any(axis=1))[:4])
    fct = sink.rows(0)[:, 4]
    assert fct.min() < 10 and fct.max() > 240                             # stream 0's FCT ran through the 249 -> 0 wrap
    assert sink.rows(2).shape == (0, 6144) and read[2].shape[0] == 0
    assert launches["k_eti"] == 2 * len(sink.chunks)                      # one front launch and one back launch per chunk


def test_the_bit_alone_gives_a_slab_of_tables_and_rows(world):
    """(e) what = DELIVER_ETI: no FIB, no MSC bytes; the documented size; the same rows"""
    sink, read, frames, slab, _ = run(world["streams"], dx.DELIVER_ETI)
    S, M, up = 3, 18, lambda v, a: (v + a - 1) // a * a
    off = up(128 + S * 72, 16)
    off = up(off + S * M * 144, 16)
    off_eti = up(off, 16)
    rows_off = up(up(off_eti + S * 64, 256), 256)
    assert slab == rows_off + S * 4 * dx.CHUNK_FRAMES * 6144
    for q in sink.chunks:
        h = q["header"]
        assert int(h["what"]) == dx.DELIVER_ETI and int(h["bytes"]) == slab == len(q["raw"])
        assert h["off_fib"] == h["off_crc"] == h["off_frame"] == h["off_sf"] == off and h["off_eti"] == off_eti and h["off_msc"] == up(off_eti + S * 64, 256)
        assert (q["subch"]["n_cifs"] == 0).all() and (q["subch"]["msc_off"] == 0).all() and (q["subch"]["sf_off"] == 0).all()
        assert [int(r["rows_off"]) for r in q["eti"]] == [rows_off + s * 28 * 6144 for s in range(S)]
    check_bookkeeping(sink, frames)
    for s in range(3):
        assert np.array_equal(sink.rows(s), world["with"][0].rows(s)) and np.array_equal(sink.rows(s), read[s])


@pytest.mark.parametrize("what", [0, 7])
def test_without_the_bit_a_slab_is_what_it_was_and_the_stage_disturbs_nothing_beside_it(world, what):
    """(f) no ETI section, no k_eti launch, a second engine fed the same samples delivers the same bytes; (g) with the bit the FIB, MSC and
    SF sections are these"""
    a = run(world["streams"], what, profile=True)
    b = run(world["streams"], what)
    assert a[3] == b[3] and a[4]["k_eti"] == 0 and a[4]["k_dabplus"] > 0
    assert len(a[0].chunks) == len(b[0].chunks) == 4
    for qa, qb in zip(a[0].chunks, b[0].chunks):
        assert int(qa["header"]["off_eti"]) == 0 and int(qa["header"]["what"]) == 7 and qa["eti"] == [None] * 3
        assert int(qa["header"]["bytes"]) == a[3] and np.array_equal(qa["raw"], qb["raw"])
    w = world["with"][0]
    # the section's table (192 bytes) moves off_msc by d = 0 or 256; the rows lie behind the logical frames from the next multiple of 256
    d = int(w.chunks[0]["header"]["off_msc"]) - int(a[0].chunks[0]["header"]["off_msc"])
    rows_off = (a[3] + d + 255) // 256 * 256
    assert d in (0, 256) and int(w.chunks[0]["eti"][0]["rows_off"]) == rows_off and world["with"][3] == rows_off + 3 * 28 * 6144
    for qa, qw in zip(a[0].chunks, w.chunks):
        for k in ("fibs", "crc", "frames", "streams"):
            assert qa[k].tobytes() == qw[k].tobytes(), k
        for k in ("msc", "sf", "sfi"):
            assert qa[k].keys() == qw[k].keys()
            for sj in qa[k]:
                assert qa[k][sj].tobytes() == qw[k][sj].tobytes(), (k, sj)
        for k in dx.CHUNK_SUBCH.names:
            if k not in ("msc_off", "sf_off", "sfi_off"):
                assert np.array_equal(qa["subch"][k], qw["subch"][k]), k
        assert ((qw["subch"]["msc_off"] - qa["subch"]["msc_off"])[qa["subch"]["msc_off"] > 0] == d).all()


def test_a_delivery_opened_on_a_running_stream_starts_with_the_cifs_decoded_from_then_on(world):
    """(h) five frames processed, then the delivery: the counter is unknown until the first delivered frame's FIG 0/0 -- which every
    frame of this ensemble carries --, so the rows are the stream's frames from CIF 20 on"""
    sink, read, frames, _, _ = run(world["streams"][:1], dx.DELIVER_ETI, calls=(7, 3, 6), before=lambda eng: eng.process(5))
    rows, ref = sink.rows(0), world["with"][0].rows(0)
    first = sink.chunks[0]["eti"][0]
    assert frames[0] == world["with"][2][0] and first["first_cif"] == 20 and first["n_eti"] == 28 and first["cifs_waiting"] == 0
    assert np.array_equal(rows, ref[4:]) and len(rows) == 4 * frames[0] - 20
    assert np.array_equal(read[0], ref)           # dabx_read_eti's own cursor went back to the rings' oldest CIF: the two are independent


def test_a_moved_subchannel_carries_its_old_start_address_up_to_the_move(world):
    """(i) dabx_set_subchannels_at moves slot 2 to other capacity units in the middle of a frame: the rows are dabx_read_eti's across the
    move, and the STC words before move_cif carry the old start address"""
    x1, sub1 = world["streams"][1]
    moved = sub1[:2] + [ds.SubCh(33, 500, 48, 64, 2, 0)]
    at = {}

    def between(eng, i):
        if i == 1:
            at["cif"] = 4 * eng.stats(0)["frames"] + 2
            eng.set_subchannels_at(moved, 0, at["cif"])

    sink, read, frames, _, _ = run([(x1, sub1)], dx.DELIVER_ETI, between=between)
    rows = sink.rows(0)
    assert at["cif"] == 4 * 5 + 2 and len(rows) == 4 * frames[0] - 16 and np.array_equal(rows, read[0])
    sad = ((rows[:, 8 + 4 * 2].astype(int) & 3) << 8) | rows[:, 8 + 4 * 2 + 1]
    cif = 16 + np.arange(len(rows))
    assert (sad[cif < at["cif"]] == 300).all() and (sad[cif >= at["cif"]] == 500).all() and (cif < at["cif"]).sum() == 6
    assert np.array_equal(rows[:6], world["with"][0].rows(1)[:6])         # (up to the move: the frames of the engine that never moved it)


def test_engines_that_cannot_serve_the_stage_refuse_the_bit():
    """(j) DABX_E_STATE (-5) from a FIC-only engine, as dabx_read_eti, and from an engine whose FIB ring is shorter than a chunk"""
    for args in (dict(fic_only=True, out_frames=8), dict(out_frames=4)):
        eng = dx.Engine(n_streams=1, ring_frames=4, max_subch=2, **args)
        try:
            for what in (dx.DELIVER_ETI, ALL3 | dx.DELIVER_ETI):
                with pytest.raises(dx.DabxError, match="libdabx error -5"):
                    eng.delivery_open(slots=2, what=what)
            with pytest.raises(dx.DabxError, match="libdabx error -2"):
                eng.delivery_open(slots=2, what=256)                      # no such bit
        finally:
            eng.close()
