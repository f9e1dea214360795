"""What the tests of the delivery slab's ring sections share (test_gpu_packet_delivery.py, test_gpu_pad_delivery.py,
test_gpu_mp2_pad_delivery.py): the consumer thread that takes the chunks while dabx_process runs and checks a section's bookkeeping, and the
slab size computed from the documented layout."""
import collections
import threading

import numpy as np

from dabstar_amd import lib as dx

CHUNK_COUNTERS = ("superframes", "aus", "pad_aus", "pad_bad", "labels", "label_bytes", "groups", "group_bytes", "dg_crc_bad", "dl_overflow", "li_bad")

# A section with an output ring: the chunk's table and reader, the header's offset field, the table's fields (first item, items, lost, offset
# of the records), the fields that add up to the slot's items and bytes so far, the caps on a chunk's items and bytes, the records' dtype.
Section = collections.namedtuple("Section", "table reader header_off table_dtype first n lost rec_off count bytes max_n max_bytes dtype")
DG = Section("dg", "datagroups", "off_dg", dx.CHUNK_DG, "first_dg", "n_dg", "dg_lost", "rec_off", ("dg_count",), ("dg_bytes",), None, None, dx.DATAGROUP_INFO)
PAD = Section("pad", "pad_items", "off_pad", dx.CHUNK_PAD, "first_item", "n_items", "items_lost", "item_off", ("labels", "groups"),
              ("label_bytes", "group_bytes"), 144, 144 * 256 + 16896, dx.PAD_ITEM)


class Sink(threading.Thread):
    """The consumer thread: takes every chunk as it lands (dabx_delivery_next with wait), checks the section's bookkeeping, keeps copies:
    per slot the section's records and bytes (items()), the table row of the newest chunk (last), the super frames (sf) and, with
    keep_msc, the logical frames (msc); per chunk its size, `what`, and the header's offset of the section (off: 0 = the slab has none)."""

    def __init__(self, eng, S, M, section, keep_msc=False):
        super().__init__(daemon=True)
        self.eng, self.S, self.M, self.section, self.keep_msc = eng, S, M, section, keep_msc
        self.rec = {}; self.by = {}; self.next = {}; self.last = {}; self.sf = {}; self.msc = {}
        self.sizes, self.whats, self.off = [], [], []
        self.want, self.seq, self.error = 0, 0, None
        self.cv = threading.Condition()

    def run(self):
        sec = self.section
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
                table = getattr(ch, sec.table)
                assert (table is None) == (int(ch.header[sec.header_off]) == 0)
                self.sizes.append(ch.nbytes); self.whats.append(int(ch.header["what"])); self.off.append(int(ch.header[sec.header_off]))
                for s in range(self.S):
                    for j in range(self.M):
                        if ch.header["what"] & dx.DELIVER_SF and ch.subch[s, j]["n_sf"]:
                            self.sf.setdefault((s, j), []).append(ch.superframes(s, j).copy())
                        if self.keep_msc and ch.header["what"] & (dx.DELIVER_MSC | dx.DELIVER_MSC_NOT_DABPLUS) and ch.subch[s, j]["n_cifs"]:
                            self.msc.setdefault((s, j), []).append(ch.msc(s, j).copy())
                        if table is None:
                            continue
                        t = table[s, j]
                        if not int(t[sec.rec_off]):
                            assert not any(int(t[k]) for k in sec.table_dtype.names), (s, j)
                            continue
                        r, b = getattr(ch, sec.reader)(s, j)
                        count, total = sum(int(t[k]) for k in sec.count), sum(int(t[k]) for k in sec.bytes)
                        assert t[sec.lost] == 0 and len(r) == t[sec.n] and len(b) == t["n_bytes"] and t[sec.first] + t[sec.n] == count
                        assert sec.max_n is None or (len(r) <= sec.max_n and len(b) <= sec.max_bytes)
                        assert t[sec.first] == self.next.get((s, j), t[sec.first]), (s, j, int(t[sec.first]))
                        assert ch.header[sec.header_off] < t[sec.rec_off] < t["bytes_off"] < ch.header["off_msc"]
                        self.next[(s, j)] = count
                        r = r.copy()
                        r["byte_pos"] += total - int(t["n_bytes"])                      # from the chunk's own base to the slot's sequence
                        self.rec.setdefault((s, j), []).append(r); self.by.setdefault((s, j), []).append(b.copy())
                        self.last[(s, j)] = t.copy()
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

    def items(self, s, j):
        r, b = self.rec.get((s, j), []), self.by.get((s, j), [])
        return (np.concatenate(r) if r else np.zeros(0, self.section.dtype)), (np.concatenate(b) if b else np.zeros(0, np.uint8))


def run_calls(eng, sink, calls):
    """dabx_process calls of the given lengths with the consumer beside them: a call of m frames lands ceil(m / 7) chunks."""
    sink.start()
    try:
        for m in calls:
            eng.process(m, sync=False)
            sink.expect((m + 6) // 7)
        eng.synchronize()
    finally:
        sink.finish()
    assert sink.error is None and eng.delivery_next(wait=False) is None


def run(x, subch, what, section, streams, ring_frames, switch_on, direct, calls=(3, 7, 1, 14, 4), keep_msc=False):
    """`streams` streams fed the same IQ; switch_on(eng, s) sets the modes of stream s's slots and returns those it switched on; process
    calls of different lengths, a consumer thread beside them.  Returns (sink, {(s, j): direct(eng, s, j)} read from the engine after the
    run for the slots switched on, frames decoded per stream, slab size)."""
    M = len(subch)
    eng = dx.Engine(n_streams=streams, ring_frames=ring_frames, max_subch=M, out_frames=8)
    try:
        eng.set_subchannels(subch)
        on = {s: switch_on(eng, s) for s in range(streams)}
        eng.delivery_open(slots=4, what=what)
        slab = eng.delivery_slab_bytes()
        for s in range(streams):
            eng.push_iq(s, x)
        sink = Sink(eng, streams, M, section, keep_msc)
        run_calls(eng, sink, calls)
        res = {(s, j): direct(eng, s, j) for s in range(streams) for j in on[s]}
        frames = [eng.stats(s)["frames"] for s in range(streams)]
        eng.delivery_close()
    finally:
        eng.close()
    return sink, res, frames, slab


def assert_tail_is_what_the_reader_returns(rec, by, r2, b2, n=None):
    """The newest records and bytes of a slot's section (rec, by: the whole run) are what the per-slot reader returned (r2, b2: its
    byte_pos counts from its own first record).  n: the reader was asked for n and its ring holds that many, so it returned no fewer."""
    k = len(r2)
    assert 0 < k <= len(rec) and (n is None or k == min(len(rec), n))
    tail = rec[-k:].copy()
    tail["byte_pos"] -= tail["byte_pos"][0]
    assert r2.tobytes() == tail.tobytes() and np.array_equal(b2, by[len(by) - len(b2):])


def documented_slab_bytes(S, subch, packet_slots=(), pad_slots=()):
    """dabx_delivery_slab_bytes from the layout include/dabx.h and DESIGN 4 document, for what = everything: header, stream table, slot table,
    FIBs, CRC flags, frame records (16-byte aligned areas), per DAB+ slot 6 super-frame rows and 6 records, [the data-group section: table,
    then per packet slot one record per possible packet and the chunk's logical-frame bytes + DABX_DG_MAX_BYTES], [the PAD section: table,
    then per PAD slot 144 records and 144 * 256 + 16 896 bytes], from a 256-byte boundary the logical frames of every slot."""
    up = lambda v, a: (v + a - 1) // a * a           # noqa: E731
    M, F = len(subch), 7
    off = up(128 + S * 72, 16)
    off = up(off + S * M * 144, 16)
    off = up(off + S * F * 384, 16); off = up(off + S * F * 12, 16); off = up(off + S * F * 16, 16)
    for _ in range(S):
        for c in subch:
            if c.dab_plus:
                off = up(off + 6 * ((110 * (c.kbps // 8) + 3) & ~3), 16) + 6 * 32
    if packet_slots:
        off = up(off, 16) + S * M * 128
        for _ in range(S):
            for j in packet_slots:
                off += 4 * F * (subch[j].kbps // 8) * 32
                off = up(off + 4 * F * 3 * subch[j].kbps + dx.DG_MAX_BYTES, 16)
    if pad_slots:
        off = up(off, 16) + S * M * 128
        for _ in range(S):
            for j in pad_slots:
                off += 144 * 32
                off = up(off + 144 * 256 + 16896, 16)
    off = up(off, 256)
    for _ in range(S):
        for c in subch:
            off = up(off + 4 * F * 3 * c.kbps, 16)
    return off
