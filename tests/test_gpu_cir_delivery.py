"""The CIR section of the bulk delivery (DABX_DELIVER_CIR, dabx_chunk_header_ext.off_cir, dabx_chunk_cir; deliver.hip k_deliver_records):
two streams of one FIC-only engine, stream 1 with both kinds on, dabx_process calls of 5, 7, 3 and 6 frames.  What Chunk.cir returns is
dabx_read_cir of a twin engine without a delivery, record for record and byte for byte; every record is in a chunk or counted lost; the
refusals hold (the bit alone, the bit with only the other opt-in bits, and 1024 / 4096 / 16384 as ever); without the bit a slab has the
size it has without the stage."""
import os
import sys

import numpy as np
import pytest

from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = (5, 7, 3, 6)
S, ON = 2, 1
ENGINE = dict(n_streams=S, ring_frames=23, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, schedule=1)


def signals():
    subch = ds.default_subchannels(1, 64)
    xs = []
    for s in range(S):
        ens = ds.build_ensemble(10, subch, seed=80 + s)
        x = ds.channel(ens.iq, snr_db=25.0, cfo_hz=55.0 * s, timing_offset=2000 + 911 * s, seed=s, n_out=21 * ds.TF).copy()
        x[300:] += np.complex64(0.5) * x[:-300].copy()                       # a second path, 6 dB down
        xs.append(x)
    return xs


def run(xs, what):
    """what = None: the twin without a delivery -> per call the records dabx_read_cir gave; else -> per call the chunks' sections"""
    eng = dx.Engine(**ENGINE)
    try:
        for s, x in enumerate(xs):
            eng.push_iq(s, x)
        eng.set_cir_mode(ON, cir=True, correlation=True)
        slab = 0
        if what is not None:
            eng.delivery_open(slots=4, what=what)
            slab = eng.delivery_slab_bytes()
        out = []
        for m in CALLS:
            assert eng.process(m) == m
            if what is None:
                out.append([[(r.tobytes(), v.copy(), i.copy()) for r, v, i in eng.read_cir(s, 8)[0]] for s in range(S)])
                continue
            for _ in range((m + 6) // 7):
                ch = eng.delivery_next(wait=True)
                assert ch is not None and ch.header_ext is not None and int(ch.header_ext["off_cir"]) % 16 == 0 and ch.cir_table is not None
                out.append(dict(table=ch.cir_table.copy(), what=int(ch.header["what"]),
                                recs=[[(r.tobytes(), v.copy(), i.copy()) for r, v, i in ch.cir(s)] for s in range(S)]))
                ch.release()
        if what is not None:
            assert eng.delivery_next(wait=False) is None
            eng.delivery_close()
        return out, slab, [eng.cir_stats(s) for s in range(S)]
    finally:
        eng.close()


@pytest.fixture(scope="module")
def world():
    """The signals and the two runs: computed once, shared, left unchanged."""
    xs = signals()
    return xs, run(xs, None), run(xs, dx.DELIVER_FIB | dx.DELIVER_CIR)


def test_chunk_cir_is_read_cir_of_the_twin_record_for_record(world):
    xs, (twin, _, tstats), (chunks, slab, stats) = world
    assert tstats == stats and stats[ON]["shows"][0] >= 3 and stats[ON]["shows"][1] >= 2 and stats[0]["shows"] == [0, 0]
    flat_twin = [r for call in twin for r in call[ON]]
    flat_bulk = [r for ch in chunks for r in ch["recs"][ON]]
    # every record the stream completed is in a chunk or counted lost (a chunk has room for DABX_CIR_CHUNK_RECORDS, the newest are kept);
    # what was delivered is the twin's record of the same number
    lost = sum(int(ch["table"][ON]["records_lost"]) for ch in chunks)
    assert len(flat_bulk) + lost == len(flat_twin) == sum(stats[ON]["shows"]) and len(flat_bulk) >= 5
    numbers = [int(ch["table"][ON]["first_record"]) + k for ch in chunks for k in range(int(ch["table"][ON]["n_records"]))]
    assert len(numbers) == len(flat_bulk) and numbers == sorted(set(numbers))
    for (rb, vb, ib), k in zip(flat_bulk, numbers):
        rt, vt, it = flat_twin[k]
        assert rb == rt and vb.tobytes() == vt.tobytes() and ib.tobytes() == it.tobytes()
    kinds = [np.frombuffer(r, dx.CIR_RECORD)[0]["kind"] for r, _, _ in flat_bulk]
    assert set(int(k) for k in kinds) == {0, 1}
    # the tables: cursors that add up, room only for the stream that had the mode on, never more than the room
    total = 0
    for ch in chunks:
        assert ch["what"] & dx.DELIVER_CIR
        t = ch["table"]
        assert int(t[0]["rec_off"]) == 0 and int(t[0]["n_records"]) == 0 and int(t[ON]["rec_off"]) % 16 == 0 and int(t[ON]["rec_off"]) > 0
        assert int(t[ON]["first_record"]) == total + int(t[ON]["records_lost"]) and 0 <= int(t[ON]["n_records"]) <= dx.CIR_CHUNK_RECORDS
        total += int(t[ON]["records_lost"]) + int(t[ON]["n_records"])
        assert int(t[ON]["records_total"]) == total
    assert len(chunks) == sum((m + 6) // 7 for m in CALLS)


def test_the_refusals_hold_and_a_slab_without_the_bit_is_unchanged(world):
    xs, _, (_, slab_with, _) = world
    optin = dx.DELIVER_ETI | dx.DELIVER_TII | dx.DELIVER_MP2_AUDIO | dx.DELIVER_AAC | dx.DELIVER_SCOPE

    def slab_of(what, mode):
        eng = dx.Engine(**ENGINE)
        try:
            if mode:
                eng.set_cir_mode(ON, cir=True, correlation=True)
            eng.delivery_open(slots=2, what=what)
            n = eng.delivery_slab_bytes()
            eng.delivery_close()
            return n
        finally:
            eng.close()
    eng = dx.Engine(**ENGINE)
    try:
        eng.set_cir_mode(ON, cir=True, correlation=True)
        for bad in (dx.DELIVER_CIR, dx.DELIVER_CIR | optin, dx.DELIVER_CIR | dx.DELIVER_SCOPE, dx.DELIVER_CIR | dx.DELIVER_TII,
                    1024, 4096, 16384, dx.DELIVER_FIB | 1024, dx.DELIVER_FIB | 4096, dx.DELIVER_FIB | 16384, dx.DELIVER_FIB | dx.DELIVER_CIR | 16384, 65536):
            with pytest.raises(dx.DabxError):
                eng.delivery_open(slots=2, what=bad)
        eng.delivery_open(slots=2, what=0)                                   # what == 0 does not include the bit
        ch_what = eng.delivery_slab_bytes()
        eng.delivery_close()
    finally:
        eng.close()
    plain = slab_of(dx.DELIVER_FIB, False)
    assert slab_of(dx.DELIVER_FIB, True) == plain                            # the stage exists, the bit is not set: the slab it has always been
    assert ch_what == slab_of(0, False)
    room = 64 + 16 + S * 32 + dx.CIR_CHUNK_RECORDS * dx.CIR_SLOT_BYTES       # the extension, the table, one stream's record slots
    assert slab_of(dx.DELIVER_FIB | dx.DELIVER_CIR, True) == slab_with and plain < slab_with <= plain + room + 4096
    assert slab_of(dx.DELIVER_FIB | dx.DELIVER_CIR, False) < slab_with       # no stream has the mode on: the table alone
