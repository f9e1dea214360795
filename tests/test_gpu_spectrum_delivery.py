"""The spectrum section of the bulk delivery (DABX_DELIVER_SPECTRUM, dabx_chunk_header_ext.off_spectrum, dabx_chunk_spectrum; deliver.hip
k_deliver_records): two streams of one FIC-only engine, stream 1 with the mode on, dabx_process calls of 5, 7, 3 and 6 frames.  What
Chunk.spectrum returns is dabx_read_spectrum of a twin engine without a delivery, record for record and byte for byte; every record is in
a chunk or counted lost; the refusals hold (the bit alone, the bit with only the other opt-in bits, and 1024 / 4096 / 16384 as ever);
without the bit a slab is byte for byte the slab of an engine that has no spectrum stage at all, with a stream's mode on and shows being made."""
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
        xs.append(ds.channel(ens.iq, snr_db=25.0, cfo_hz=55.0 * s, timing_offset=2000 + 911 * s, seed=s, n_out=21 * ds.TF).copy())
    return xs


def flat(recs):
    return [(r.tobytes(), l.tobytes(), d.tobytes(), w.tobytes()) for r, l, d, w in recs]


def run(xs, what):
    """what = None: the twin without a delivery -> per call the records dabx_read_spectrum gave; else -> per chunk its section"""
    eng = dx.Engine(**ENGINE)
    try:
        for s, x in enumerate(xs):
            eng.push_iq(s, x)
        eng.set_spectrum_mode(ON, averaging="fast", zoom=50)
        slab = 0
        if what is not None:
            eng.delivery_open(slots=4, what=what)
            slab = eng.delivery_slab_bytes()
        out = []
        for m in CALLS:
            assert eng.process(m) == m
            if what is None:
                out.append([flat(eng.read_spectrum(s, 8)[0]) for s in range(S)])
                continue
            for _ in range((m + 6) // 7):
                ch = eng.delivery_next(wait=True)
                assert ch is not None and ch.header_ext is not None and int(ch.header_ext["off_spectrum"]) % 16 == 0 and ch.spectrum_table is not None
                assert ch.cir_table is None and int(ch.header_ext["off_cir"]) == 0
                out.append(dict(table=ch.spectrum_table.copy(), what=int(ch.header["what"]), recs=[flat(ch.spectrum(s)) for s in range(S)]))
                ch.release()
        if what is not None:
            assert eng.delivery_next(wait=False) is None
            eng.delivery_close()
        return out, slab, [eng.spectrum_stats(s) for s in range(S)]
    finally:
        eng.close()


@pytest.fixture(scope="module")
def world():
    """The signals and the two runs: computed once, shared, left unchanged."""
    xs = signals()
    return xs, run(xs, None), run(xs, dx.DELIVER_FIB | dx.DELIVER_SPECTRUM)


def test_chunk_spectrum_is_read_spectrum_of_the_twin_record_for_record(world):
    xs, (twin, _, tstats), (chunks, slab, stats) = world
    assert tstats == stats and stats[ON]["shows"] >= 6 and stats[0]["shows"] == 0 and stats[ON]["untrusted"] == 0
    flat_twin = [r for call in twin for r in call[ON]]
    flat_bulk = [r for ch in chunks for r in ch["recs"][ON]]
    lost = sum(int(ch["table"][ON]["records_lost"]) for ch in chunks)
    assert len(flat_bulk) + lost == len(flat_twin) == stats[ON]["shows"] and len(flat_bulk) >= 6 and lost == 0
    numbers = [int(ch["table"][ON]["first_record"]) + k for ch in chunks for k in range(int(ch["table"][ON]["n_records"]))]
    assert len(numbers) == len(flat_bulk) and numbers == sorted(set(numbers))
    for rec, k in zip(flat_bulk, numbers):
        assert rec == flat_twin[k]
    firsts = [int(np.frombuffer(r[0], dx.SPECTRUM_RECORD)[0]["first_sample"]) for r in flat_bulk]
    assert firsts == sorted(firsts) and all(b - a > dx.SPECTRUM_PERIOD for a, b in zip(firsts, firsts[1:]))
    total = 0
    for ch in chunks:
        assert ch["what"] & dx.DELIVER_SPECTRUM
        t = ch["table"]
        assert int(t[0]["rec_off"]) == 0 and int(t[0]["n_records"]) == 0 and int(t[ON]["rec_off"]) % 16 == 0 and int(t[ON]["rec_off"]) > 0
        assert int(t[ON]["first_record"]) == total + int(t[ON]["records_lost"]) and 0 <= int(t[ON]["n_records"]) <= dx.SPECTRUM_CHUNK_RECORDS
        total += int(t[ON]["records_lost"]) + int(t[ON]["n_records"])
        assert int(t[ON]["records_total"]) == total
    assert len(chunks) == sum((m + 6) // 7 for m in CALLS)


def test_without_the_bit_every_slab_is_byte_identical_to_one_without_the_stage(world):
    """what = DELIVER_FIB, the same signals and calls, once with stream 1's mode on (records are completed meanwhile) and once in an engine that
    never had the stage: every chunk's bytes -- header, no extension, tables, sections -- its size and its offsets are the same."""
    xs = world[0]

    def slabs(mode):
        eng = dx.Engine(**ENGINE)
        try:
            for s, x in enumerate(xs):
                eng.push_iq(s, x)
            if mode:
                eng.set_spectrum_mode(ON, averaging="fast", zoom=50)
            eng.delivery_open(slots=4, what=dx.DELIVER_FIB)
            size, out = eng.delivery_slab_bytes(), []
            for m in CALLS:
                assert eng.process(m) == m
                for _ in range((m + 6) // 7):
                    ch = eng.delivery_next(wait=True)
                    assert ch is not None and ch.header_ext is None and ch.spectrum_table is None
                    out.append((ch.raw.tobytes(), ch.header.tobytes(), int(ch.header["what"]), int(ch.nbytes)))
                    ch.release()
            eng.delivery_close()
            return size, out, eng.spectrum_stats(ON)["shows"], eng.spectrum_stats(ON)["launches"]
        finally:
            eng.close()
    size_on, on, shows_on, launches_on = slabs(True)
    size_off, off, shows_off, launches_off = slabs(False)
    assert shows_on >= 6 and launches_on == sum(CALLS) and (shows_off, launches_off) == (0, 0)     # the stage was at work in the one, absent in the other
    assert size_on == size_off and len(on) == len(off) == sum((m + 6) // 7 for m in CALLS)
    for k, (a, b) in enumerate(zip(on, off)):
        assert a[2] == b[2] == dx.DELIVER_FIB and a[3] == b[3], k
        assert a[1] == b[1], k                                           # the header: `what`, the size and every offset
        assert a[0] == b[0], k                                           # every byte of the slab


def test_the_refusals_hold_and_a_slab_without_the_bit_is_unchanged(world):
    xs, _, (_, slab_with, _) = world
    optin = dx.DELIVER_ETI | dx.DELIVER_TII | dx.DELIVER_MP2_AUDIO | dx.DELIVER_AAC | dx.DELIVER_SCOPE | dx.DELIVER_CIR

    def slab_of(what, mode):
        eng = dx.Engine(**ENGINE)
        try:
            if mode:
                eng.set_spectrum_mode(ON)
            eng.delivery_open(slots=2, what=what)
            n = eng.delivery_slab_bytes()
            eng.delivery_close()
            return n
        finally:
            eng.close()
    eng = dx.Engine(**ENGINE)
    try:
        eng.set_spectrum_mode(ON)
        for bad in (dx.DELIVER_SPECTRUM, dx.DELIVER_SPECTRUM | optin, dx.DELIVER_SPECTRUM | dx.DELIVER_CIR, dx.DELIVER_SPECTRUM | dx.DELIVER_SCOPE,
                    dx.DELIVER_SPECTRUM | dx.DELIVER_TII, dx.DELIVER_CIR | dx.DELIVER_SCOPE, 1024, 4096, 16384, dx.DELIVER_FIB | 1024,
                    dx.DELIVER_FIB | 4096, dx.DELIVER_FIB | 16384, dx.DELIVER_FIB | dx.DELIVER_SPECTRUM | 16384, 131072, dx.DELIVER_FIB | 131072):
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
    room = 64 + 16 + S * 32 + dx.SPECTRUM_CHUNK_RECORDS * dx.SPECTRUM_SLOT_BYTES      # the extension, the table, one stream's record slots
    assert slab_of(dx.DELIVER_FIB | dx.DELIVER_SPECTRUM, True) == slab_with and plain < slab_with <= plain + room + 4096
    assert slab_of(dx.DELIVER_FIB | dx.DELIVER_SPECTRUM, False) <= slab_with  # no stream has the mode on: the table alone
