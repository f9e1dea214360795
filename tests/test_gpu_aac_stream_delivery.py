"""The AAC section of the delivery slab (DABX_DELIVER_AAC), through IQ: an ensemble whose DAB+ sub-channels 0 (64 kbit/s) and 1 (32 kbit/s)
carry scenarios of tests/aac_stream_cases.py (AU tables in order) is pushed as IQ on two streams, a delivery is open and the chunks are taken
while dabx_process runs -- k_aac_stream inside the real chain, on the MSC batch's stream, k_deliver_aac behind it.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of records and bytes of the model run on the super frames and
records the same chunks deliver for the slot -- records by .tobytes(), bytes by np.array_equal, counters by == --, equals
dabx_read_aac_frames and dabx_get_aac_stream_stats, and frames_lost == 0.  Without the bit the slabs and their size are byte for byte those
of an engine that has no slot with the mode; the bit alone, or with only TII and / or MP2_AUDIO, is DABX_E_ARG, and so is 1024 still."""
import os
import sys

import numpy as np
import pytest

import aac_stream_cases as ac
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import assert_tail_is_what_the_reader_returns  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
S = 2
SLOTS = ((0, 64, 51), (1, 32, 52))          # slot, kbit/s, scenario seed
CALLS = (3, 7, 1, 14, 4)
BASE = dx.DELIVER_FIB | dx.DELIVER_SF
TABLE_COUNTERS = ("superframes", "records", "frames", "frame_bytes", "lost_len", "lost_crc")


def _layout():
    return [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 24, 32, 2, 0), ds.SubCh(2, 96, 24, 32, 2, 0, dab_plus=0)]


def run(x, what, aac):
    """One engine, the chunks of CALLS taken as they land: ([per chunk dict(raw, header, ext, per (s, j) table row, records, bytes, super
    frames, their records)], slab bytes, per (s, j) (stats, what dabx_read_aac_frames returns))."""
    subch = _layout()
    # acquire_mode 1 and schedule 1: what a slab's stream table shows does not depend on timing (slabs are compared byte by byte below)
    eng = dx.Engine(n_streams=S, ring_frames=N_TX + 2, max_subch=len(subch), out_frames=8, acquire_mode=1, schedule=1)
    chunks = []
    try:
        eng.set_subchannels(subch)
        if aac:
            for s in range(S):
                for j, _, _ in SLOTS:
                    eng.set_aac_stream_mode(s, j)
        eng.delivery_open(slots=4, what=what)
        slab = eng.delivery_slab_bytes()
        for s in range(S):
            eng.push_iq(s, x)
        for m in CALLS:
            eng.process(m, sync=False)
            for _ in range((m + 6) // 7):
                ch = eng.delivery_next(wait=True)
                assert ch is not None and ch.seq == len(chunks) and ch.nbytes == slab
                q = dict(raw=ch.raw.copy(), header=ch.header.copy(), ext=None if ch.header_ext is None else ch.header_ext.copy(), slots={})
                for s in range(S):
                    for j, _, _ in SLOTS:
                        t, rec, by = ch.aac(s, j)
                        q["slots"][(s, j)] = (None if t is None else t.copy(), rec.copy(), by.copy(), ch.superframes(s, j).copy(), ch.superframe_info(s, j).copy())
                chunks.append(q)
                ch.release()
        eng.synchronize()
        assert eng.delivery_next(wait=False) is None
        direct = {(s, j): (eng.aac_stream_stats(s, j), eng.read_aac_frames(s, j, 128)) for s in range(S) for j, _, _ in SLOTS}
        eng.delivery_close()
    finally:
        eng.close()
    return chunks, slab, direct


@pytest.fixture(scope="module")
def world():
    """The signal and the runs: computed once, shared, left unchanged."""
    subch = _layout()
    pay = {j: ac.scenario(kbps, seed, False, 4 * N_TX)[0] for j, kbps, seed in SLOTS}
    ens = ds.build_ensemble(N_TX, subch, seed=23, payloads=pay)
    x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=-311.0, timing_offset=4321, seed=23, n_out=(N_TX + 1) * ds.TF)
    return dict(with_bit=run(x, BASE | dx.DELIVER_AAC, True), base_on=run(x, BASE, True), base_off=run(x, BASE, False),
                bit_no_slot=run(x, BASE | dx.DELIVER_AAC, False), no_sf=run(x, dx.DELIVER_FIB | dx.DELIVER_AAC, True))


def _whole(chunks, s, j):
    """(records with byte_pos in the slot's stream, bytes, super frames, their records, the last table row) of a slot over all chunks."""
    recs, bys, sfs, sfis, nxt, at, t = [], [], [], [], None, 0, None
    for q in chunks:
        t, rec, by, sf, sfi = q["slots"][(s, j)]
        assert int(t["rec_off"]) and int(t["frames_lost"]) == 0 and len(rec) == int(t["n_frames"]) <= 36 and len(by) == int(t["n_bytes"])
        assert int(q["ext"]["off_aac"]) < int(t["rec_off"]) < int(t["bytes_off"]) <= int(q["header"]["off_msc"])
        assert int(t["bytes_off"]) == int(t["rec_off"]) + 36 * 32
        assert nxt is None or int(t["first_frame"]) == nxt
        nxt = int(t["first_frame"]) + int(t["n_frames"])
        assert nxt == int(t["records"])
        if len(rec):
            assert rec["byte_pos"][0] == 0 and int(rec["byte_pos"][-1]) + int(rec["length"][-1]) == len(by)
        rec = rec.copy()
        rec["byte_pos"] += at
        at += len(by)
        assert at == int(t["frame_bytes"])
        recs.append(rec); bys.append(by); sfs.append(sf); sfis.append(sfi)
    return np.concatenate(recs), np.concatenate(bys), np.concatenate(sfs), np.concatenate(sfis), t


def test_the_section_is_the_models_stream_on_the_delivered_super_frames_and_equals_the_per_slot_reader(world):
    chunks, slab, direct = world["with_bit"]
    assert len(chunks) == sum((m + 6) // 7 for m in CALLS)
    for q in chunks:
        h, x = q["header"], q["ext"]
        assert int(h["what"]) == BASE | dx.DELIVER_AAC and x is not None and int(x["magic"]) == dx.CHUNK_EXT_MAGIC and int(x["bytes"]) == 64
        assert int(h["off_stream"]) == 192 and int(x["off_tii"]) == 0 and int(x["off_mp2_audio"]) == 0
        assert 192 < int(x["off_aac"]) < int(h["off_msc"]) and int(x["off_aac"]) % 16 == 0 and not any(int(v) for v in x["reserved"])
    for s in range(S):
        for j, kbps, _ in SLOTS:
            st, (r2, b2) = direct[(s, j)]
            recs, by, sfs, sfis, last = _whole(chunks, s, j)
            assert len(sfs) >= 14, len(sfs)                  # >= 80 logical frames hold 16 windows; junk in front and a rejected header cost one each
            m = ac.run_model(sfs, sfis)
            assert m.counters["frames"] >= 25 and m.counters["lost_crc"] > 0 and m.counters["lost_len"] > 0, m.counters      # there is traffic to deliver
            assert recs.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(recs), len(m.rows))
            assert all(st[k] == m.counters[k] for k in ac.COUNTERS), (s, j, st, m.counters)
            assert len(ac.parse_loas(by)) == m.counters["frames"]
            assert all(int(last[k]) == st[k] for k in TABLE_COUNTERS), (s, j, last, st)
            assert st["launches"] == len(chunks)
            # the per-slot reader was not called during the run: what its rings no longer hold counts as lost there, and only there
            assert st["lost"] == len(recs) - len(r2), (s, j, st, len(recs), len(r2))
            assert_tail_is_what_the_reader_returns(recs, by, r2, b2)
        # the row of the slot that is not DAB+ is all zero
        for q in chunks:
            o = int(q["ext"]["off_aac"])
            table = q["raw"][o:o + S * 3 * 128].view(dx.CHUNK_AAC).reshape(S, 3)
            assert not any(int(table[s, 2][k]) for k in dx.CHUNK_AAC.names if k != "reserved")
    # a consumer of the stream can drop the super frames: FIB | AAC delivers the same section in a smaller slab
    chunks2, slab2, direct2 = world["no_sf"]
    assert slab2 < slab and all(int(q["header"]["what"]) == dx.DELIVER_FIB | dx.DELIVER_AAC for q in chunks2)
    for s in range(S):
        for j, kbps, _ in SLOTS:
            a, b = _whole(chunks, s, j), _whole(chunks2, s, j)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), (s, j)


def test_the_sections_room_is_what_the_header_documents(world):
    with_bit, base = world["with_bit"], world["base_on"]
    h, x = with_bit[0][0]["header"], with_bit[0][0]["ext"]
    # behind the table every slot with the mode on has room for 36 records and 6 * (110 * kbps / 8 + 72) bytes (a 16-byte boundary behind
    # each); the logical frames start at the next multiple of 256; everything behind off_msc is as large as without the bit
    end = int(x["off_aac"]) + S * 3 * 128
    for s in range(S):
        for j, kbps, _ in SLOTS:
            end = (end + 36 * 32 + 6 * (110 * kbps // 8 + 72) + 15) // 16 * 16
    assert int(h["off_msc"]) == (end + 255) // 256 * 256
    assert with_bit[1] - int(h["off_msc"]) == base[1] - int(base[0][0]["header"]["off_msc"])


def test_without_the_bit_slabs_sizes_and_launches_are_those_of_an_engine_without_the_mode(world):
    a, b = world["base_on"], world["base_off"]
    assert a[1] == b[1] and len(a[0]) == len(b[0])
    for qa, qb in zip(a[0], b[0]):
        assert qa["ext"] is None and int(qa["header"]["what"]) == BASE and np.array_equal(qa["raw"], qb["raw"])
    for key, (st, (rec, by)) in b[2].items():
        assert not any(st.values()) and len(rec) == 0, (key, st)
    for key, (st, (rec, by)) in a[2].items():          # the stage itself runs all the same: the per-slot reader has the frames
        assert st["frames"] >= 25 and st["launches"] == len(a[0]) and len(rec) > 0, (key, st)
    # the per-slot results do not depend on the delivery's mask
    for key in world["with_bit"][2]:
        sa, (ra, ba) = world["with_bit"][2][key]
        sb, (rb, bb) = world["base_on"][2][key]
        assert sa == sb and ra.tobytes() == rb.tobytes() and np.array_equal(ba, bb), key
    # the bit without a slot that has the mode on: the header's extension and no section; no launch
    chunks, slab, direct = world["bit_no_slot"]
    assert slab - b[1] in (0, 256)                     # 64 bytes more in the head part, which ends at a multiple of 256
    for q in chunks:
        assert q["ext"] is not None and int(q["ext"]["off_aac"]) == 0 and int(q["header"]["off_stream"]) == 192
        assert all(t is None and len(rec) == 0 for t, rec, *_ in q["slots"].values())
    assert all(not any(st.values()) for st, _ in direct.values())          # launches among them


def test_the_bit_alone_is_refused_and_1024_still_is():
    eng = dx.Engine(n_streams=1, ring_frames=2, max_subch=1, out_frames=8)
    try:
        for what in (dx.DELIVER_AAC, dx.DELIVER_AAC | dx.DELIVER_TII, dx.DELIVER_AAC | dx.DELIVER_MP2_AUDIO,
                     dx.DELIVER_AAC | dx.DELIVER_MP2_AUDIO | dx.DELIVER_TII, 1024, 1024 | dx.DELIVER_FIB, 1024 | dx.DELIVER_AAC | dx.DELIVER_FIB, 4096 | dx.DELIVER_FIB):
            with pytest.raises(dx.DabxError, match="error -2"):
                eng.delivery_open(slots=4, what=what)
        eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_AAC)
        eng.delivery_close()
    finally:
        eng.close()
