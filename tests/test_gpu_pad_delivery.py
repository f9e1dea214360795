"""The PAD section of the delivery slab (include/dabx.h, dabx_chunk_pad; k_deliver_pad behind k_deliver_dg), through IQ: an ensemble whose
DAB+ sub-channels 1 and 4 carry the PAD scenarios of tests/pad_cases.py is pushed as IQ on two streams, a delivery is open and a consumer
thread takes the chunks while dabx_process runs -- k_pad inside the real chain, behind k_dabplus on the MSC batch's stream.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of items of the model run on the oracle receiver's super frames
of the same IQ -- records by .tobytes(), bytes by np.array_equal, counters by == --, it equals dabx_read_pad_items and
dabx_get_pad_stats, and items_lost == 0."""
import os
import sys
import threading

import numpy as np
import pytest

import pad_cases as pc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from test_gpu_engine import _oracle_run  # noqa: E402
from test_gpu_packet_delivery import _documented_slab_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
PAD = {1: (64, 31), 4: (32, 32)}            # sub-channel index -> (kbit/s, scenario seed)
CHUNK_COUNTERS = ("superframes", "aus", "pad_aus", "pad_bad", "labels", "label_bytes", "groups", "group_bytes", "dg_crc_bad", "dl_overflow", "li_bad")


def _layout():
    return [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 48, 64, 2, 0), ds.SubCh(2, 96, 48, 64, 2, 0, dab_plus=0), ds.SubCh(3, 144, 72, 96, 2, 0),
            ds.SubCh(4, 216, 24, 32, 2, 0), ds.SubCh(5, 240, 24, 32, 2, 0, dab_plus=0)]


_case = {}


def _signal():
    """(sub-channels, IQ, the oracle receiver's results) -- built once, shared, left unchanged."""
    if not _case:
        subch = _layout()
        # (the time de-interleaver fills for 16 CIFs: the scenario starts there, behind sixteen frames of its end)
        pay = {j: np.concatenate([pc.scenario(k, seed)[0][-16:], pc.scenario(k, seed)[0][:4 * N_TX - 16]]) for j, (k, seed) in PAD.items()}
        ens = ds.build_ensemble(N_TX, subch, seed=11, payloads=pay)
        x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=217.0, timing_offset=5555, seed=11, n_out=(N_TX + 1) * ds.TF)
        _case["v"] = (subch, x, _oracle_run(x, subch))
    return _case["v"]


class Sink(threading.Thread):
    """The consumer thread: takes every chunk as it lands (dabx_delivery_next with wait), checks the section's bookkeeping, keeps copies."""

    def __init__(self, eng, S, M):
        super().__init__(daemon=True)
        self.eng, self.S, self.M = eng, S, M
        self.rec = {}; self.by = {}; self.next_item = {}; self.last = {}; self.sf = {}
        self.sizes, self.whats, self.off_pad = [], [], []
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
                self.sizes.append(ch.nbytes); self.whats.append(int(ch.header["what"])); self.off_pad.append(int(ch.header["off_pad"]))
                for s in range(self.S):
                    for j in range(self.M):
                        if ch.header["what"] & dx.DELIVER_SF and ch.subch[s, j]["n_sf"]:
                            self.sf.setdefault((s, j), []).append(ch.superframes(s, j).copy())
                        if ch.pad is None:
                            continue
                        t = ch.pad[s, j]
                        if not int(t["item_off"]):
                            assert not any(int(t[k]) for k in dx.CHUNK_PAD.names), (s, j)
                            continue
                        r, b = ch.pad_items(s, j)
                        assert t["items_lost"] == 0 and len(r) == t["n_items"] <= 144 and len(b) == t["n_bytes"] <= 144 * 256 + 16896
                        assert t["first_item"] + t["n_items"] == t["labels"] + t["groups"]
                        assert t["first_item"] == self.next_item.get((s, j), t["first_item"]), (s, j, int(t["first_item"]))
                        assert ch.header["off_pad"] < t["item_off"] < t["bytes_off"] < ch.header["off_msc"]
                        self.next_item[(s, j)] = int(t["labels"] + t["groups"])
                        r = r.copy()
                        r["byte_pos"] += int(t["label_bytes"] + t["group_bytes"]) - int(t["n_bytes"])      # from the chunk's own base to the slot's sequence
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
        return (np.concatenate(r) if r else np.zeros(0, dx.PAD_ITEM)), (np.concatenate(b) if b else np.zeros(0, np.uint8))


def _run(x, subch, what, streams=2, pad=True, calls=(3, 7, 1, 14, 4)):
    """`streams` streams fed the same IQ; process calls of different lengths, a consumer thread beside them.  Returns (sink, per (stream,
    slot) PAD stats, the newest items as dabx_read_pad_items gives them and the slot's super-frame count, frames decoded, slab size)."""
    M = len(subch)
    eng = dx.Engine(n_streams=streams, ring_frames=N_TX + 2, max_subch=M, out_frames=8)
    try:
        eng.set_subchannels(subch)
        if pad:
            for s in range(streams):
                for j in PAD:
                    eng.set_pad_mode(s, j)
        eng.delivery_open(slots=4, what=what)
        slab = eng.delivery_slab_bytes()
        for s in range(streams):
            eng.push_iq(s, x)
        sink = Sink(eng, streams, M)
        sink.start()
        try:
            for m in calls:
                eng.process(m, sync=False)
                sink.expect((m + 6) // 7)
            eng.synchronize()
        finally:
            sink.finish()
        assert sink.error is None and eng.delivery_next(wait=False) is None
        direct = {}
        if pad:
            for s in range(streams):
                for j in PAD:
                    direct[(s, j)] = (eng.pad_stats(s, j), eng.read_pad_items(s, j, 512), eng.subch_stats(s, j)["sf_count"])
        frames = [eng.stats(s)["frames"] for s in range(streams)]
        eng.delivery_close()
    finally:
        eng.close()
    return sink, direct, frames, slab


def _check_against_model(sink, direct, frames, ora, streams=2):
    for s in range(streams):
        assert frames[s] >= 26, frames
        for j, (kbps, _) in PAD.items():
            st, (r2, b2), n_sf = direct[(s, j)]
            sfs = ora["sf"][j].reshape(-1, 110 * kbps // 8)[:n_sf]
            sfi = ora["sfi"][j].view(dx.SUPERFRAME_INFO)[:n_sf]
            assert n_sf >= 15 and len(sfs) == n_sf
            m = pc.run_model(sfs, sfi)
            assert m.counters["labels"] >= 1 and m.counters["pad_aus"] >= 15 and (kbps != 64 or m.counters["groups"] >= 3), (j, m.counters)      # there is traffic to deliver
            rec, by = sink.items(s, j)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            assert all(st[k] == m.counters[k] for k in pc.PAD_COUNTERS), (s, j, st, m.counters)
            assert all(st[k] == int(sink.last[(s, j)][k]) for k in CHUNK_COUNTERS), (s, j, st, sink.last[(s, j)])
            assert st["items_lost"] == 0 and st["active"] == 1
            # ... and they are what the per-slot reader returns (its byte_pos counts from its own first item)
            k = len(r2)
            assert k == min(len(rec), 512) > 0
            tail = rec[-k:].copy()
            tail["byte_pos"] -= tail["byte_pos"][0]
            assert r2.tobytes() == tail.tobytes() and np.array_equal(b2, by[len(by) - len(b2):])


def test_the_section_carries_every_item_of_the_model_on_the_oracle_receivers_super_frames():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=0)
    assert all(sink.off_pad) and all(w == 7 | dx.DELIVER_PAD for w in sink.whats) and all(n == slab for n in sink.sizes)
    _check_against_model(sink, direct, frames, ora)
    # the super frames of the PAD slots are delivered as before
    for j, (kbps, _) in PAD.items():
        got = np.concatenate(sink.sf[(0, j)])
        assert np.array_equal(got, ora["sf"][j].reshape(-1, 110 * kbps // 8)[:len(got)]) and len(got) == direct[(0, j)][2]
    _case["items"] = {k: sink.items(*k) for k in direct}


def test_fib_and_pad_alone_deliver_the_same_items():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=dx.DELIVER_FIB | dx.DELIVER_PAD)
    assert all(w == dx.DELIVER_FIB | dx.DELIVER_PAD for w in sink.whats) and not sink.sf
    _check_against_model(sink, direct, frames, ora)
    if "items" in _case:
        for k, (rec, by) in _case["items"].items():
            assert sink.items(*k)[0].tobytes() == rec.tobytes() and np.array_equal(sink.items(*k)[1], by)


def _documented(S, subch, pad_slots=()):
    """dabx_delivery_slab_bytes from the layout include/dabx.h and DESIGN 4 document, for what = everything and no packet-mode slot:
    header, stream table, slot table, FIBs, CRC flags, frame records (16-byte aligned areas), per DAB+ slot 6 super-frame rows and 6
    records, [the PAD section: table, then per PAD slot 144 records and 144 * 256 + 16 896 bytes], from a 256-byte boundary the logical
    frames of every slot."""
    up = lambda v, a: (v + a - 1) // a * a           # noqa: E731
    M, F = len(subch), 7
    off = up(128 + S * 72, 16)
    off = up(off + S * M * 144, 16)
    off = up(off + S * F * 384, 16); off = up(off + S * F * 12, 16); off = up(off + S * F * 16, 16)
    for _ in range(S):
        for c in subch:
            if c.dab_plus:
                off = up(off + 6 * ((110 * (c.kbps // 8) + 3) & ~3), 16) + 6 * 32
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


def test_without_a_pad_slot_the_slab_is_what_it_has_always_been():
    """No PAD slot: with what = 0 and with DABX_DELIVER_PAD set explicitly the slabs have no section (off_pad = 0, the header's `what`
    without the bit), the size is dabx_delivery_slab_bytes computed from the documented layout -- the layout before this section existed --
    and the two runs' slabs carry the same super frames.  With PAD slots the size grows by exactly the documented section: the table and,
    per PAD slot, 144 records and 144 * 256 + 16 896 bytes."""
    subch, x, ora = _signal()
    a = _run(x, subch, what=0, streams=1, pad=False, calls=(7, 7))
    b = _run(x, subch, what=7 | dx.DELIVER_PAD, streams=1, pad=False, calls=(7, 7))
    want = _documented_slab_bytes(1, subch)
    for sink, _, _, slab in (a, b):
        assert slab == want and all(n == want for n in sink.sizes) and not any(sink.off_pad) and all(w == 7 for w in sink.whats), (slab, want, sink.whats)
    for k in a[0].sf:
        assert np.array_equal(np.concatenate(a[0].sf[k]), np.concatenate(b[0].sf[k]))
    assert want == _documented(1, subch)
    c = _run(x, subch, what=0, streams=1, pad=True, calls=(7,))
    assert c[3] == _documented(1, subch, tuple(PAD)) > want, (c[3], want)
