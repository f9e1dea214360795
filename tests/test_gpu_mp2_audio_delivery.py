"""The MP2 audio section of the delivery slab (DABX_DELIVER_MP2_AUDIO), through IQ: an ensemble whose DAB audio sub-channels 1 (64 kbit/s) and
2 (32 kbit/s) carry MP2 scenarios of tests/mp2_audio_cases.py is pushed as IQ on two streams, a delivery is open and the chunks are taken
while dabx_process runs -- k_mp2_audio inside the real chain, on the MSC batch's stream, k_deliver_mp2_audio behind it.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of records and PCM of the model run on the logical frames the same
chunks deliver for the slot -- records by .tobytes(), PCM by np.array_equal, counters by == --, equals dabx_read_mp2_audio and
dabx_get_mp2_audio_stats, and frames_lost == 0.  Without the bit the slabs and their size are byte for byte those of an engine that has no
audio slot at all, with what = FIB | MSC | SF and with what = 0; the bit alone is DABX_E_ARG."""
import os
import sys

import numpy as np
import pytest

import mp2_audio_cases as ac
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import assert_tail_is_what_the_reader_returns, documented_slab_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
S = 2
AUDIO = ((1, 64, 41, 11), (2, 32, 42, 6))   # slot, kbit/s, scenario seed, bit offset
CALLS = (3, 7, 1, 14, 4)
BASE = dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF
TABLE_COUNTERS = ("decode_calls", "frames_out", "bad_header", "refused", "overread", "sample_rate", "voffs", "number_of_frames", "error_frames")


def _layout():
    return [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 48, 64, 2, 0, dab_plus=0), ds.SubCh(2, 96, 24, 32, 2, 0, dab_plus=0)]


def run(x, what, audio):
    """One engine, the chunks of CALLS taken as they land: ([per chunk dict(raw, header, ext, per (s, j) table row, records, PCM, logical
    frames)], slab bytes, per (s, j) (stats, what dabx_read_mp2_audio returns), launches)."""
    subch = _layout()
    # acquire_mode 1 and schedule 1: what a slab's stream table shows does not depend on timing (slabs are compared byte by byte below)
    eng = dx.Engine(n_streams=S, ring_frames=N_TX + 2, max_subch=len(subch), out_frames=8, acquire_mode=1, schedule=1)
    chunks = []
    try:
        eng.set_subchannels(subch)
        if audio:
            for s in range(S):
                for j, _, _, _ in AUDIO:
                    eng.set_mp2_audio_mode(s, j)
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
                    for j, _, _, _ in AUDIO:
                        rec, by = ch.mp2_audio(s, j)
                        q["slots"][(s, j)] = (None if ch.mp2_audio_table is None else ch.mp2_audio_table[s, j].copy(), rec.copy(), by.copy(),
                                              ch.msc(s, j).copy())
                chunks.append(q)
                ch.release()
        eng.synchronize()
        assert eng.delivery_next(wait=False) is None
        direct = {(s, j): (eng.mp2_audio_stats(s, j), eng.read_mp2_audio(s, j, 64)) for s in range(S) for j, _, _, _ in AUDIO}
        eng.delivery_close()
    finally:
        eng.close()
    return chunks, slab, direct


@pytest.fixture(scope="module")
def world():
    """The signal and the runs: computed once, shared, left unchanged."""
    subch = _layout()
    pay = {j: ac.scenario(kbps, seed, off, 4 * N_TX)[0] for j, kbps, seed, off in AUDIO}
    ens = ds.build_ensemble(N_TX, subch, seed=21, payloads=pay)
    x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=-311.0, timing_offset=4321, seed=21, n_out=(N_TX + 1) * ds.TF)
    return dict(with_bit=run(x, BASE | dx.DELIVER_MP2_AUDIO, True), base_on=run(x, BASE, True), base_off=run(x, BASE, False),
                zero_on=run(x, 0, True), zero_off=run(x, 0, False), bit_no_slot=run(x, BASE | dx.DELIVER_MP2_AUDIO, False))


def test_the_section_is_the_models_pcm_on_the_delivered_logical_frames_and_equals_the_per_slot_reader(world):
    chunks, slab, direct = world["with_bit"]
    assert len(chunks) == sum((m + 6) // 7 for m in CALLS)
    for q in chunks:
        h, x = q["header"], q["ext"]
        assert int(h["what"]) == BASE | dx.DELIVER_MP2_AUDIO and x is not None and int(x["magic"]) == dx.CHUNK_EXT_MAGIC and int(x["bytes"]) == 64
        assert int(h["off_stream"]) == 192 and int(x["off_tii"]) == 0 and 192 < int(x["off_mp2_audio"]) < int(h["off_msc"]) and int(x["off_mp2_audio"]) % 16 == 0
        assert not any(int(v) for v in x["reserved"])
    for s in range(S):
        for j, kbps, _, _ in AUDIO:
            st, (r2, b2) = direct[(s, j)]
            recs, pcm, frames, nxt = [], [], [], None
            for q in chunks:
                t, rec, by, lf = q["slots"][(s, j)]
                frames.append(lf)
                assert int(t["rec_off"]) and int(t["frames_lost"]) == 0 and len(rec) == int(t["n_frames"]) <= 28 and len(by) == int(t["n_bytes"]) == 4608 * len(rec)
                assert int(q["ext"]["off_mp2_audio"]) < int(t["rec_off"]) < int(t["bytes_off"]) < int(q["header"]["off_msc"])
                assert int(t["bytes_off"]) == int(t["rec_off"]) + 28 * 32
                assert nxt is None or int(t["first_frame"]) == nxt
                nxt = int(t["first_frame"]) + int(t["n_frames"])
                assert nxt == int(t["frames_out"])
                assert list(rec["byte_pos"]) == [4608 * k for k in range(len(rec))]
                rec = rec.copy()
                rec["byte_pos"] += 4608 * int(t["first_frame"])
                recs.append(rec); pcm.append(by)
            recs, pcm, frames = np.concatenate(recs), np.concatenate(pcm), np.concatenate(frames)
            assert len(frames) >= 80, len(frames)
            m = ac.run_model(kbps, frames)
            assert m.stats["frames_out"] >= 40 and m.stats["bad_header"] > 0 and m.stats["refused"] > 0, m.stats      # there is traffic to deliver
            assert recs.tobytes() == m.records().tobytes() and np.array_equal(pcm, m.all_pcm()), (s, j, len(recs), len(m.rows))
            assert all(st[k] == m.all_stats()[k] for k in ac.STAT_FIELDS), (s, j, st, m.all_stats())
            # the per-slot reader was not called during the run: what its ring of 64 records no longer holds counts as lost there, and only there
            assert st["frames_lost"] == max(0, st["frames_out"] - 64), (s, j, st)
            last = chunks[-1]["slots"][(s, j)][0]
            assert all(int(last[k]) == st[k] for k in TABLE_COUNTERS), (s, j, last, st)
            assert st["launches"] == len(chunks)
            # ... and they are what the per-slot reader returns (its byte_pos counts from its own first record)
            assert_tail_is_what_the_reader_returns(recs, pcm, r2, b2, 64)
        # the DAB+ slot's row of the section is all zero
        for q in chunks:
            o = int(q["ext"]["off_mp2_audio"])
            table = q["raw"][o:o + S * 3 * 128].view(dx.CHUNK_MP2_AUDIO).reshape(S, 3)
            assert not any(int(table[s, 0][k]) for k in dx.CHUNK_MP2_AUDIO.names if k != "reserved")


def test_the_sections_room_is_what_the_header_documents(world):
    with_bit, base = world["with_bit"], world["base_on"]
    h, x = with_bit[0][0]["header"], with_bit[0][0]["ext"]
    # behind the table every slot with the mode on has room for 28 records and 28 * 4608 bytes; the logical frames start at the next
    # multiple of 256; everything behind off_msc is as large as without the bit
    end = int(x["off_mp2_audio"]) + S * 3 * 128 + S * len(AUDIO) * (28 * 32 + 28 * 4608)
    assert int(h["off_msc"]) == (end + 255) // 256 * 256
    assert with_bit[1] - int(h["off_msc"]) == base[1] - int(base[0][0]["header"]["off_msc"])


def test_without_the_bit_slabs_sizes_and_launches_are_those_of_an_engine_without_an_audio_slot(world):
    subch = _layout()
    for on, off in (("base_on", "base_off"), ("zero_on", "zero_off")):
        a, b = world[on], world[off]
        assert a[1] == b[1] == documented_slab_bytes(S, subch), (on, a[1], b[1])
        assert len(a[0]) == len(b[0])
        for qa, qb in zip(a[0], b[0]):
            assert qa["ext"] is None and int(qa["header"]["what"]) == BASE and np.array_equal(qa["raw"], qb["raw"]), on
        for key, (st, (rec, by)) in b[2].items():
            assert not any(st.values()) and len(rec) == 0, (off, key, st)
        for key, (st, (rec, by)) in a[2].items():      # the stage itself runs all the same: the per-slot reader has the frames
            assert st["active"] == 1 and st["frames_out"] >= 40 and len(rec) == min(64, st["frames_out"]), (on, key, st)
    # the per-slot results do not depend on the delivery's mask
    for key in world["with_bit"][2]:
        sa, (ra, ba) = world["with_bit"][2][key]
        sb, (rb, bb) = world["base_on"][2][key]
        assert sa == sb and ra.tobytes() == rb.tobytes() and np.array_equal(ba, bb), key
    # the bit without a slot that has the mode on: the header's extension and no section; no launch
    chunks, slab, direct = world["bit_no_slot"]
    assert slab - world["base_off"][1] in (0, 256)                    # 64 bytes more in the head part, which ends at a multiple of 256
    for q in chunks:
        assert q["ext"] is not None and int(q["ext"]["off_mp2_audio"]) == 0 and int(q["header"]["off_stream"]) == 192
    assert all(not any(st.values()) for st, _ in direct.values())


def test_the_bit_alone_is_refused():
    eng = dx.Engine(n_streams=1, ring_frames=2, max_subch=1, out_frames=8)
    try:
        for what in (dx.DELIVER_MP2_AUDIO, dx.DELIVER_MP2_AUDIO | dx.DELIVER_TII, 1024, 1024 | dx.DELIVER_FIB):
            with pytest.raises(dx.DabxError, match="error -2"):
                eng.delivery_open(slots=4, what=what)
        eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_MP2_AUDIO)
        eng.delivery_close()
    finally:
        eng.close()
