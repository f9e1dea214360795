"""The data-group section of the delivery slab (include/dabx.h, dabx_chunk_dg; k_deliver_dg behind k_deliver_msc), through IQ: an ensemble
with packet-mode payloads in two sub-channels next to DAB+ ones is pushed as IQ, a delivery is open and a consumer thread takes the chunks
while dabx_process runs -- k_packet inside the real chain, on the MSC batch's stream between the logical-frame gather and k_dabplus.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of groups of the model (tests/packet_cases.py) run on the oracle
receiver's logical frames of the same IQ -- records by .tobytes(), bytes by np.array_equal, counters by == --, it equals dabx_read_datagroups
and dabx_get_packet_stats, and dg_lost == 0."""
import os
import sys

import numpy as np
import pytest

import packet_cases as pc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import DG, Sink, assert_tail_is_what_the_reader_returns, documented_slab_bytes, run  # noqa: E402
from oracle_lib import oracle_run, oracle_run_with_move  # noqa: E402

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
        _case["v"] = (subch, x, oracle_run(x, subch))
    return _case["v"]


def _run(x, subch, what, streams=2, packet=True, calls=(3, 7, 1, 14, 4)):
    """delivery_sink.run with stream s's packet slots read with their addresses.  Returns (sink, per (stream, slot) packet stats and the
    newest groups as dabx_read_datagroups gives them, frames decoded, slab size)."""
    def switch_on(eng, s):
        for j, (_, address, _) in PKT.items():
            if packet:
                eng.set_packet_mode(s, j, address[s])
        return list(PKT) if packet else []

    return run(x, subch, what, DG, streams, N_TX + 2, switch_on, lambda eng, s, j: (eng.packet_stats(s, j), eng.read_datagroups(s, j, 4096)),
               calls, keep_msc=True)


def _check_against_model(sink, direct, frames, ora, streams=2):
    for s in range(streams):
        assert frames[s] >= 26, frames
        for j, (kbps, addresses, _) in PKT.items():
            address = addresses[s]
            lf = ora["msc"][j].reshape(-1, 3 * kbps)[:4 * frames[s] - 16]
            m = pc.run_model(lf, address)
            rec, by = sink.items(s, j)
            if address == pc.ADDRESS_A:          # the scenarios' faults are sent to this address; the other one sees good groups between them
                assert m.counters["dg_count"] >= 10 and m.counters["crc_bad"] and m.counters["continuity_err"], (j, m.counters)
            assert m.counters["dg_count"] >= 1, (j, m.counters)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            st, (r2, b2) = direct[(s, j)]
            assert all(st[k] == m.counters[k] == int(sink.last[(s, j)][k]) for k in pc.PACKET_COUNTERS), (s, j, st, m.counters)
            assert st["dg_lost"] == 0
            # ... and they are what the per-slot reader returns (its byte_pos counts from its own first group)
            assert_tail_is_what_the_reader_returns(rec, by, r2, b2)


def test_the_section_carries_every_group_of_the_model_on_the_oracle_receivers_frames():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=0)
    assert all(sink.off) and all(w == 7 | dx.DELIVER_DG for w in sink.whats) and all(n == slab for n in sink.sizes)
    _check_against_model(sink, direct, frames, ora)
    # the logical frames of the packet slots are delivered as before
    for j, (kbps, _, _) in PKT.items():
        got = np.concatenate(sink.msc[(0, j)])
        assert np.array_equal(got, ora["msc"][j].reshape(-1, 3 * kbps)[:len(got)]) and len(got) == 4 * frames[0] - 16
    _case["groups"] = {k: sink.items(*k) for k in direct}


def test_fib_and_dg_alone_deliver_the_same_groups():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=dx.DELIVER_FIB | dx.DELIVER_DG)
    assert all(w == dx.DELIVER_FIB | dx.DELIVER_DG for w in sink.whats) and not sink.msc
    _check_against_model(sink, direct, frames, ora)
    if "groups" in _case:
        for k, (rec, by) in _case["groups"].items():
            assert sink.items(*k)[0].tobytes() == rec.tobytes() and np.array_equal(sink.items(*k)[1], by)


def test_without_a_packet_slot_the_slab_is_what_it_has_always_been():
    """No slot in packet mode: with what = 0 and with DABX_DELIVER_DG set explicitly the slabs have no section (off_dg = 0, the header's
    `what` without the bit), the size is dabx_delivery_slab_bytes computed from the documented layout -- the layout before this section
    existed --, and the two runs' slabs carry the same logical frames.  With packet slots the size grows by exactly the documented section."""
    subch, x, ora = _signal()
    a = _run(x, subch, what=0, streams=1, packet=False, calls=(7, 7))
    b = _run(x, subch, what=7 | dx.DELIVER_DG, streams=1, packet=False, calls=(7, 7))
    want = documented_slab_bytes(1, subch)
    for sink, _, _, slab in (a, b):
        assert slab == want and all(n == want for n in sink.sizes) and not any(sink.off) and all(w == 7 for w in sink.whats), (slab, want, sink.whats)
    for k in a[0].msc:
        assert np.array_equal(np.concatenate(a[0].msc[k]), np.concatenate(b[0].msc[k]))
    c = _run(x, subch, what=0, streams=1, packet=True, calls=(7,))
    assert c[3] == documented_slab_bytes(1, subch, packet_slots=tuple(PKT)) > want


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
    ora_a = oracle_run_with_move(x, a)
    c0_ora = dx.parse_fibs(ora_a["fibs"][2][:1], np.ones(1, np.uint8))[1] - 8
    ora = oracle_run_with_move(x, a, move=(1, 400, ens.switch_cif - c0_ora))
    eng = dx.Engine(n_streams=1, ring_frames=n_frames + 2, max_subch=3, out_frames=8)
    try:
        eng.set_subchannels(a)
        eng.set_packet_mode(0, 1, address)
        eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_DG | dx.DELIVER_MSC_NOT_DABPLUS)
        eng.push_iq(0, x)
        sink = Sink(eng, 1, 3, DG, keep_msc=True)
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
    rec, by = sink.items(0, 1)
    assert rec.tobytes() == r.tobytes() and np.array_equal(by, m.all_bytes()), (len(rec), len(r))
    assert all(st[k] == m.counters[k] for k in pc.PACKET_COUNTERS) and st["dg_lost"] == 0 and st["active"] == 1, (st, m.counters)
