"""The data-group section of the delivery slab (include/dabx.h, dabx_chunk_dg; k_deliver_dg behind k_deliver_msc), through IQ: an ensemble
with packet-mode payloads in two sub-channels next to DAB+ ones is pushed as IQ, a delivery is open and a consumer thread takes the chunks
while dabx_process runs -- k_packet inside the real chain, on the MSC batch's stream between the logical-frame gather and k_dabplus.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of groups of the model (tests/packet_cases.py) run on the oracle
receiver's logical frames of the same IQ -- records by .tobytes(), bytes by np.array_equal, counters by == --, it equals dabx_read_datagroups
and dabx_get_packet_stats, and dg_lost == 0."""
import os
import sys
import threading

import numpy as np
import pytest

import packet_cases as pc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from test_gpu_engine import _oracle_run  # noqa: E402
from test_gpu_reconfig import _oracle as _oracle_moved  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames (cyclic: a whole number of super frames)
# sub-channel index -> (kbit/s, packet address of the slot in stream 0 and in stream 1, scenario seed)
PKT = {2: (64, (pc.ADDRESS_A, pc.ADDRESS_B), 21), 5: (32, (pc.ADDRESS_A, pc.ADDRESS_A), 22)}


def _layout():
    subch = [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 48, 64, 2, 0), ds.SubCh(2, 96, 48, 64, 2, 0, dab_plus=0), ds.SubCh(3, 144, 72, 96, 2, 0),
             ds.SubCh(4, 216, 24, 32, 2, 0), ds.SubCh(5, 240, 24, 32, 2, 0, dab_plus=0), ds.SubCh(6, 264, 24, 32, 2, 0, dab_plus=0)]
    return subch


_case = {}


def _signal():
    """(sub-channels, IQ, the oracle receiver's results) -- built once, shared, left unchanged."""
    if not _case:
        subch = _layout()
        pay = {j: np.concatenate([pc.scenario(k, seed), pc.scenario(k, seed + 1)])[:4 * N_TX] for j, (k, _, seed) in PKT.items()}
        ens = ds.build_ensemble(N_TX, subch, seed=9, payloads=pay)
        x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=-431.0, timing_offset=7777, seed=9, n_out=(N_TX + 1) * ds.TF)
        _case["v"] = (subch, x, _oracle_run(x, subch))
    return _case["v"]


class Sink(threading.Thread):
    """The consumer thread: takes every chunk as it lands (dabx_delivery_next with wait), checks the section's bookkeeping, keeps copies."""

    def __init__(self, eng, S, M):
        super().__init__(daemon=True)
        self.eng, self.S, self.M = eng, S, M
        self.rec = {}; self.by = {}; self.next_dg = {}; self.last = {}; self.msc = {}
        self.sizes, self.whats, self.has_dg = [], [], []
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
                self.sizes.append(ch.nbytes); self.whats.append(int(ch.header["what"])); self.has_dg.append(ch.dg is not None)
                for s in range(self.S):
                    for j in range(self.M):
                        if ch.header["what"] & (dx.DELIVER_MSC | dx.DELIVER_MSC_NOT_DABPLUS) and ch.subch[s, j]["n_cifs"]:
                            self.msc.setdefault((s, j), []).append(ch.msc(s, j).copy())
                        if ch.dg is None:
                            continue
                        t = ch.dg[s, j]
                        if not int(t["rec_off"]):
                            assert not any(int(t[k]) for k in dx.CHUNK_DG.names), (s, j)
                            continue
                        r, b = ch.datagroups(s, j)
                        assert t["dg_lost"] == 0 and len(r) == t["n_dg"] and len(b) == t["n_bytes"] and t["first_dg"] + t["n_dg"] == t["dg_count"]
                        assert t["first_dg"] == self.next_dg.get((s, j), t["first_dg"]), (s, j, int(t["first_dg"]))
                        assert ch.header["off_dg"] < t["rec_off"] < t["bytes_off"] < ch.header["off_msc"]
                        self.next_dg[(s, j)] = int(t["dg_count"])
                        r = r.copy()
                        r["byte_pos"] += int(t["dg_bytes"]) - int(t["n_bytes"])        # from the chunk's own base to the slot's sequence
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

    def groups(self, s, j):
        r, b = self.rec.get((s, j), []), self.by.get((s, j), [])
        return (np.concatenate(r) if r else np.zeros(0, dx.DATAGROUP_INFO)), (np.concatenate(b) if b else np.zeros(0, np.uint8))


def _run(x, subch, what, streams=2, packet=True, calls=(3, 7, 1, 14, 4)):
    """`streams` streams fed the same IQ, stream s's packet slots read with their addresses; process calls of different lengths, a
    consumer thread beside them.  Returns (sink, per (stream, slot) packet stats and the newest groups as dabx_read_datagroups gives them,
    frames decoded, slab size)."""
    M = len(subch)
    eng = dx.Engine(n_streams=streams, ring_frames=N_TX + 2, max_subch=M, out_frames=8)
    try:
        eng.set_subchannels(subch)
        if packet:
            for s in range(streams):
                for j, (_, address, _) in PKT.items():
                    eng.set_packet_mode(s, j, address[s])
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
        if packet:
            for s in range(streams):
                for j in PKT:
                    direct[(s, j)] = (eng.packet_stats(s, j), eng.read_datagroups(s, j, 4096))
        frames = [eng.stats(s)["frames"] for s in range(streams)]
        eng.delivery_close()
    finally:
        eng.close()
    return sink, direct, frames, slab


def _check_against_model(sink, direct, frames, ora, streams=2):
    for s in range(streams):
        assert frames[s] >= 26, frames
        for j, (kbps, addresses, _) in PKT.items():
            address = addresses[s]
            lf = ora["msc"][j].reshape(-1, 3 * kbps)[:4 * frames[s] - 16]
            m = pc.run_model(lf, address)
            rec, by = sink.groups(s, j)
            if address == pc.ADDRESS_A:          # the scenarios' faults are sent to this address; the other one sees good groups between them
                assert m.counters["dg_count"] >= 10 and m.counters["crc_bad"] and m.counters["continuity_err"], (j, m.counters)
            assert m.counters["dg_count"] >= 1, (j, m.counters)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            st, (r2, b2) = direct[(s, j)]
            assert all(st[k] == m.counters[k] == int(sink.last[(s, j)][k]) for k in pc.PACKET_COUNTERS), (s, j, st, m.counters)
            assert st["dg_lost"] == 0
            # ... and they are what the per-slot reader returns (its byte_pos counts from its own first group)
            k = len(r2)
            assert k == min(len(rec), k) > 0
            tail = rec[-k:].copy()
            tail["byte_pos"] -= tail["byte_pos"][0]
            assert r2.tobytes() == tail.tobytes() and np.array_equal(b2, by[len(by) - len(b2):])


def test_the_section_carries_every_group_of_the_model_on_the_oracle_receivers_frames():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=0)
    assert all(sink.has_dg) and all(w == 7 | dx.DELIVER_DG for w in sink.whats) and all(n == slab for n in sink.sizes)
    _check_against_model(sink, direct, frames, ora)
    # the logical frames of the packet slots are delivered as before
    for j, (kbps, _, _) in PKT.items():
        got = np.concatenate(sink.msc[(0, j)])
        assert np.array_equal(got, ora["msc"][j].reshape(-1, 3 * kbps)[:len(got)]) and len(got) == 4 * frames[0] - 16
    _case["groups"] = {k: sink.groups(*k) for k in direct}


def test_fib_and_dg_alone_deliver_the_same_groups():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=dx.DELIVER_FIB | dx.DELIVER_DG)
    assert all(w == dx.DELIVER_FIB | dx.DELIVER_DG for w in sink.whats) and not sink.msc
    _check_against_model(sink, direct, frames, ora)
    if "groups" in _case:
        for k, (rec, by) in _case["groups"].items():
            assert sink.groups(*k)[0].tobytes() == rec.tobytes() and np.array_equal(sink.groups(*k)[1], by)


def _documented_slab_bytes(S, subch, packet_slots=()):
    """dabx_delivery_slab_bytes from the layout include/dabx.h and DESIGN 4 document, for what = everything: header, stream table, slot table,
    FIBs, CRC flags, frame records (16-byte aligned areas), per DAB+ slot 6 super-frame rows and 6 records, [the data-group section: table,
    then per packet slot one record per possible packet and the chunk's logical-frame bytes + DABX_DG_MAX_BYTES], from a 256-byte boundary
    the logical frames of every slot."""
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
    off = up(off, 256)
    for _ in range(S):
        for c in subch:
            off = up(off + 4 * F * 3 * c.kbps, 16)
    return off


def test_without_a_packet_slot_the_slab_is_what_it_has_always_been():
    """No slot in packet mode: with what = 0 and with DABX_DELIVER_DG set explicitly the slabs have no section (off_dg = 0, the header's
    `what` without the bit), the size is dabx_delivery_slab_bytes computed from the documented layout -- the layout before this section
    existed --, and the two runs' slabs carry the same logical frames.  With packet slots the size grows by exactly the documented section."""
    subch, x, ora = _signal()
    a = _run(x, subch, what=0, streams=1, packet=False, calls=(7, 7))
    b = _run(x, subch, what=7 | dx.DELIVER_DG, streams=1, packet=False, calls=(7, 7))
    want = _documented_slab_bytes(1, subch)
    for sink, _, _, slab in (a, b):
        assert slab == want and all(n == want for n in sink.sizes) and not any(sink.has_dg) and all(w == 7 for w in sink.whats), (slab, want, sink.whats)
    for k in a[0].msc:
        assert np.array_equal(np.concatenate(a[0].msc[k]), np.concatenate(b[0].msc[k]))
    c = _run(x, subch, what=0, streams=1, packet=True, calls=(7,))
    assert c[3] == _documented_slab_bytes(1, subch, tuple(PKT)) > want


def test_a_reconfiguration_that_moves_the_packet_sub_channel_mid_group_loses_nothing():
    """The packet sub-channel moves to other capacity units at an announced CIF (FIG 0/0 change flags, dabx_follow_fic,
    dabx_set_subchannels_at) while a group is under way: the section's groups are the model's on the logical frames of an oracle back end
    that is handed its slice from the new address from that CIF on."""
    kbps, address = 64, pc.ADDRESS_A
    a = [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 48, 64, 2, 0, dab_plus=0), ds.SubCh(2, 96, 48, 64, 2, 0)]
    b = [a[0], ds.SubCh(1, 400, 48, 64, 2, 0, dab_plus=0), a[2]]
    n_frames, switch_frame = 27, 13
    # long groups around the switch: the 64 kbit/s scenario from the place where its 4 KB groups are
    pay = pc.scenario(kbps, 21)[-4 * n_frames:]
    ens = ds.build_reconfigured_ensemble(n_frames, a, b, switch_frame, announce_frames=7, seed=5, payloads={1: pay})
    x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=310.0, timing_offset=3000, seed=5, cyclic=False)
    ora_a = _oracle_moved(x, a)
    c0_ora = dx.parse_fibs(ora_a["fibs"][2][:1], np.ones(1, np.uint8))[1] - 8
    ora = _oracle_moved(x, a, move=(1, 400, ens.switch_cif - c0_ora))
    eng = dx.Engine(n_streams=1, ring_frames=n_frames + 2, max_subch=3, out_frames=8)
    try:
        eng.set_subchannels(a)
        eng.set_packet_mode(0, 1, address)
        eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_DG | dx.DELIVER_MSC_NOT_DABPLUS)
        eng.push_iq(0, x)
        sink = Sink(eng, 1, 3)
        sink.start()
        at_cif, applied = None, False
        try:
            for _ in range(ora["n"] + 3):
                rc = eng.follow_fic(0)
                if rc["pending"]:
                    at_cif = rc["at_cif"]
                    nxt = eng.next_subchannels(0)
                if at_cif is not None and not applied and eng.stats(0)["frames"] == at_cif // 4:
                    by_id = {g.subch_id: g for g in nxt}
                    eng.set_subchannels_at([by_id[c.subch_id] for c in b], 0, at_cif)
                    applied = True
                eng.process(1, sync=False)
                sink.expect(1)
            eng.synchronize()
        finally:
            sink.finish()
        st = eng.packet_stats(0, 1)
        frames = eng.stats(0)["frames"]
        eng.delivery_close()
    finally:
        eng.close()
    assert applied and sink.error is None and frames >= n_frames - 2
    lf = ora["msc"][1][:4 * frames - 16]
    got = np.concatenate(sink.msc[(0, 1)])
    assert np.array_equal(got, lf)
    m = pc.run_model(lf, address)
    r = m.records()
    move_frame = at_cif - 16                                       # the slot's logical frame built from the first CIFs at the new address
    assert ((r["first_frame"] < move_frame) & (r["last_frame"] >= move_frame + 16)).any(), r[["first_frame", "last_frame"]]
    rec, by = sink.groups(0, 1)
    assert rec.tobytes() == r.tobytes() and np.array_equal(by, m.all_bytes()), (len(rec), len(r))
    assert all(st[k] == m.counters[k] for k in pc.PACKET_COUNTERS) and st["dg_lost"] == 0 and st["active"] == 1, (st, m.counters)
