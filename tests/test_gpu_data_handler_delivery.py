"""The data section of the delivery slab (include/dabx.h, DABX_DELIVER_DATA: dabx_chunk_header_ext2 at byte 192, dabx_chunk_data;
k_deliver_data behind k_data_handler), through IQ: an ensemble with three packet-mode sub-channels that carry the crafted and random groups
of tests/data_handler_cases.py -- one per handler -- and a DAB+ sub-channel is pushed as IQ on two streams, a delivery is open and a
consumer thread takes the chunks while dabx_process runs: k_data_handler inside the real chain, behind k_packet on the MSC batch's stream.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of items of the handler's model run on the packet model's groups of
the oracle receiver's logical frames of the same IQ -- records by .tobytes(), bytes by np.array_equal --, it equals dabx_read_data_items and
dabx_get_data_stats, and items_lost == 0.  Stream 1's Journaline slot has only_new_revisions on."""
import os
import sys

import numpy as np
import pytest

import data_handler_cases as dh
import packet_cases as pkc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import Section, Sink, assert_tail_is_what_the_reader_returns, documented_slab_bytes, run_calls  # noqa: E402
from oracle_lib import oracle_run  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
KINDS = {0: "tdc", 1: "ip", 2: "journaline"}      # sub-channel index -> handler; sub-channel 3 is a DAB+ slot
BASE = dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF
OPT_IN = (dx.DELIVER_ETI, dx.DELIVER_TII, dx.DELIVER_MP2_AUDIO, dx.DELIVER_AAC, dx.DELIVER_SCOPE, dx.DELIVER_CIR, dx.DELIVER_SPECTRUM, dx.DELIVER_FIG)
DATA_SECTION = Section("data_table", "data", "off_data", dx.CHUNK_DATA, "first_item", "n_items", "items_lost", "rec_off", ("items",), ("bytes",), 256, None, dx.DATA_ITEM)


def _layout():
    return [ds.SubCh(0, 0, 48, 64, 2, 0, dab_plus=0), ds.SubCh(1, 48, 48, 64, 2, 0, dab_plus=0), ds.SubCh(2, 96, 48, 64, 2, 0, dab_plus=0),
            ds.SubCh(3, 144, 24, 32, 2, 0)]


_case = {}


def _signal():
    """(sub-channels, IQ, the oracle receiver's results) -- built once, shared, left unchanged."""
    if not _case:
        subch = _layout()
        # (the time de-interleaver fills for 16 CIFs: the scenarios start there, behind sixteen frames of their end -- padding packets)
        behind = lambda f: np.concatenate([f[-16:], f[:4 * N_TX - 16]])      # noqa: E731
        pay = {j: behind(dh.frames_of(64, dh.sequence(k) + dh.random_groups(k, 60), [11, j])) for j, k in KINDS.items()}
        ens = ds.build_ensemble(N_TX, subch, seed=15, payloads=pay)
        x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=-311.0, timing_offset=4444, seed=15, n_out=(N_TX + 1) * ds.TF)
        _case["v"] = (subch, x, oracle_run(x, subch))
    return _case["v"]


class DataSink(Sink):
    """delivery_sink.Sink for a section that the SECOND extension announces: the same bookkeeping checks, and the extension itself"""

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
                h, what = ch.header, int(ch.header["what"])
                self.sizes.append(ch.nbytes); self.whats.append(what)
                if what & dx.DELIVER_DATA:                    # the first extension is full: a second one at byte 192, the stream table at 256
                    x2 = ch.header_ext2
                    assert int(h["off_stream"]) == 256 and int(x2["magic"]) == dx.CHUNK_EXT2_MAGIC and int(x2["bytes"]) == 64 and not x2["reserved"].any()
                    assert ch.header_ext is not None and int(ch.header_ext["bytes"]) == 64
                    self.off.append(int(x2["off_data"]))
                else:
                    assert int(h["off_stream"]) == (192 if what & ~255 else 128) and ch.header_ext2 is None and ch.data_table is None
                    self.off.append(0)
                table = ch.data_table
                assert (table is None) == (self.off[-1] == 0)
                for s in range(self.S):
                    for j in range(self.M):
                        if table is None:
                            assert ch.data(s, j)[0] is None and len(ch.data(s, j)[1]) == 0
                            continue
                        t = table[s, j]
                        if not int(t["rec_off"]):
                            assert not any(int(np.sum(t[k])) for k in dx.CHUNK_DATA.names) and ch.data(s, j)[0] is None, (s, j)
                            continue
                        row, r, b = ch.data(s, j)
                        assert t["items_lost"] == 0 and len(r) == t["n_items"] <= 256 and len(b) == t["n_bytes"] == int(r["length"].sum())
                        assert t["first_item"] + t["n_items"] == t["items"] and t["first_item"] == self.next.get((s, j), t["first_item"]), (s, j)
                        assert self.off[-1] < t["rec_off"] < t["bytes_off"] < h["off_msc"] and not t["reserved"].any()
                        self.next[(s, j)] = int(t["items"])
                        r = r.copy()
                        r["byte_pos"] += int(t["bytes"]) - int(t["n_bytes"])             # from the chunk's own base to the slot's sequence
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


def _run(x, subch, what, streams=2, handlers=True, calls=(3, 7, 1, 14, 4)):
    """`streams` streams fed the same IQ, packet mode on sub-channels 0..2 and their handlers with it, process calls of different lengths with
    the consumer beside them.  Returns (sink, {(s, j): (data_stats, read_data_items)}, frames decoded per stream, slab size)."""
    M = len(subch)
    eng = dx.Engine(n_streams=streams, ring_frames=N_TX + 2, max_subch=M, out_frames=8)
    try:
        eng.set_subchannels(subch)
        for s in range(streams):
            for j, kind in KINDS.items():
                eng.set_packet_mode(s, j, dh.ADDRESS)
                if handlers:
                    eng.set_data_mode(s, j, kind, only_new_revisions=dh.ONLY_NEW[s])
        eng.delivery_open(slots=4, what=what)
        slab = eng.delivery_slab_bytes()
        for s in range(streams):
            eng.push_iq(s, x)
        sink = DataSink(eng, streams, M, DATA_SECTION)
        run_calls(eng, sink, calls)
        res = {(s, j): (eng.data_stats(s, j), eng.read_data_items(s, j, 256, max_bytes=1 << 17)) for s in range(streams) for j in KINDS}
        frames = [eng.stats(s)["frames"] for s in range(streams)]
        eng.delivery_close()
    finally:
        eng.close()
    return sink, res, frames, slab


def _check_against_model(sink, direct, frames, ora, streams=2):
    for s in range(streams):
        assert frames[s] >= 26, frames
        for j, kind in KINDS.items():
            lf = ora["msc"][j].reshape(-1, 3 * 64)[:4 * frames[s] - 16]
            m = dh.model_of(kind, pkc.run_model(lf, dh.ADDRESS), dh.ONLY_NEW[s])
            assert m.counters["items"] >= 8 and m.counters["groups"] >= 40, (j, m.counters)      # there is traffic to deliver
            st, (r2, b2) = direct[(s, j)]
            rec, by = sink.items(s, j)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            assert all(st[k] == m.counters[k] for k in dx.DATA_COUNTERS), (s, j, st, m.counters)
            assert all(st[k] == int(sink.last[(s, j)][k]) for k in ("groups", "items", "bytes")), (s, j, st, sink.last[(s, j)])
            assert st["lost"] == 0 and st["active"] == 1 and st["dg_overrun"] == 0
            assert_tail_is_what_the_reader_returns(rec, by, r2, b2, 256)
        assert (s, 3) not in sink.last


def test_the_section_carries_every_item_of_the_models_and_equals_the_reader():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=BASE | dx.DELIVER_DATA)
    assert all(sink.off) and all(w == BASE | dx.DELIVER_DATA for w in sink.whats) and all(n == slab for n in sink.sizes)
    _check_against_model(sink, direct, frames, ora)
    _case["items"] = {k: sink.items(*k) for k in direct}


def test_fib_and_data_alone_deliver_the_same_items():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=dx.DELIVER_FIB | dx.DELIVER_DATA)
    assert all(sink.off) and all(w == dx.DELIVER_FIB | dx.DELIVER_DATA for w in sink.whats) and not sink.sf
    _check_against_model(sink, direct, frames, ora)
    if "items" in _case:
        for k, (rec, by) in _case["items"].items():
            assert sink.items(*k)[0].tobytes() == rec.tobytes() and np.array_equal(sink.items(*k)[1], by)


def test_data_alone_or_with_only_opt_in_bits_is_refused_and_the_refused_masks_stay_refused():
    subch = _layout()
    eng = dx.Engine(n_streams=1, ring_frames=4, max_subch=len(subch), out_frames=8)
    L = dx.load()
    try:
        eng.set_subchannels(subch)
        masks = [dx.DELIVER_DATA] + [dx.DELIVER_DATA | b for b in OPT_IN] + [dx.DELIVER_DATA | sum(OPT_IN)]
        masks += [1 | dx.DELIVER_DATA | b for b in (1024, 4096, 16384, 131072)] + [1 | b for b in (1024, 4096, 16384, 131072, 1 << 20)]
        for what in masks:
            cfg = dx.DeliveryConfig(host_slabs=4, what=what, copy_engine=0)
            assert L.dabx_delivery_open(eng._h, dx.C.byref(cfg)) == -2, what
        eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_DATA)
        eng.delivery_close()
    finally:
        eng.close()


def _documented(S, subch, head, data_slots):
    """delivery_sink.documented_slab_bytes for what = FIB | MSC | SF with `head` bytes of header and extensions in front of the stream table
    and the data section of include/dabx.h behind the super frames: the table and, per slot with a handler, 256 records and the packet
    slot's room (4 * 7 logical frames + DABX_DG_MAX_BYTES)."""
    up = lambda v, a: (v + a - 1) // a * a           # noqa: E731
    M, F = len(subch), 7
    off = up(head + S * 72, 16)
    off = up(off + S * M * 144, 16)
    off = up(off + S * F * 384, 16); off = up(off + S * F * 12, 16); off = up(off + S * F * 16, 16)
    for _ in range(S):
        for c in subch:
            if c.dab_plus:
                off = up(off + 6 * ((110 * (c.kbps // 8) + 3) & ~3), 16) + 6 * 32
    if data_slots:
        off = up(off, 16) + S * M * 128
        for _ in range(S):
            for j in data_slots:
                off += 256 * 32
                off = up(off + 4 * F * 3 * subch[j].kbps + dx.DG_MAX_BYTES, 16)
    off = up(off, 256)
    for _ in range(S):
        for c in subch:
            off = up(off + 4 * F * 3 * c.kbps, 16)
    return off


def test_without_the_bit_a_slab_is_what_it_was_and_with_it_it_grows_by_the_documented_extension_and_section():
    """Handlers on and the bit off: no second extension, the stream table where it was, the size dabx_delivery_slab_bytes computed from the
    documented layout of before (what = 0: with the data-group section).  The bit on and no handler slot: the second extension, off_stream
    256, off_data 0, no section.  The bit and the handlers: the documented section."""
    subch, x, ora = _signal()
    pk = tuple(KINDS)
    a = _run(x, subch, what=0, streams=1, calls=(7, 7))
    assert a[3] == documented_slab_bytes(1, subch, packet_slots=pk) and not any(a[0].off) and all(n == a[3] for n in a[0].sizes)
    b = _run(x, subch, what=BASE, streams=1, calls=(7,))
    assert b[3] == _documented(1, subch, 128, ()) and not any(b[0].off)
    c = _run(x, subch, what=BASE | dx.DELIVER_DATA, streams=1, handlers=False, calls=(7, 7))
    assert c[3] == _documented(1, subch, 256, ()) and not any(c[0].off) and all(w == BASE | dx.DELIVER_DATA for w in c[0].whats)
    d = _run(x, subch, what=BASE | dx.DELIVER_DATA, streams=1, calls=(7,))
    assert d[3] == _documented(1, subch, 256, pk) > c[3] and all(d[0].off)
