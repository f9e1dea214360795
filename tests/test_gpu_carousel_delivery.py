"""The carousel slots' rows of the delivery slab's MOT section (include/dabx.h, dabx_chunk_mot; k_deliver_carousel behind k_deliver_mot),
through IQ: an ensemble with two packet-mode sub-channels that carry the carousel scenarios of tests/carousel_cases.py and a DAB+
sub-channel that carries a MOT scenario of tests/mot_cases.py in its X-PAD is pushed as IQ on two streams, a delivery is open and a consumer
thread takes the chunks while dabx_process runs -- k_carousel inside the real chain, behind k_packet on the MSC batch's stream.

Concatenated over the chunks, a carousel slot's section is the COMPLETE sequence of objects of MotHandlerModel run on the packet model's
groups of the oracle receiver's logical frames of the same IQ -- records by .tobytes(), bytes by np.array_equal, counters by == --, it
equals dabx_read_mot_objects and dabx_get_carousel_stats, and objects_lost == 0; the PAD-MOT slot of the same engine is delivered in the
same section as before."""
import os
import sys

import numpy as np
import pytest

import carousel_cases as cc
import mot_cases as mc
import packet_cases as pkc
import pad_cases as pc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import Section, assert_tail_is_what_the_reader_returns, documented_slab_bytes, run  # noqa: E402
from oracle_lib import oracle_run  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
CAR = {1: "header", 2: "directory"}         # sub-channel index -> carousel_cases' scenario it carries (stream 0's)
MOT = {0: (64, (1, 0))}                     # sub-channel index -> (kbit/s, (stream, slot) of mot_cases' scenario it carries)
MOT_SECTION = Section("mot", "mot_objects", "off_mot", dx.CHUNK_MOT, "first_object", "n_objects", "objects_lost", "rec_off", ("objects",),
                      ("object_bytes",), 16, 2 * 65536, dx.MOT_OBJECT)
CHUNK_COUNTERS = ("objects", "object_bytes", "groups", "headers", "segments", "crc_bad", "grp_short", "hdr_bad", "obj_overflow", "resets")


def _layout():
    return [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 48, 64, 2, 0, dab_plus=0), ds.SubCh(2, 96, 288, 384, 2, 0, dab_plus=0),
            ds.SubCh(3, 384, 24, 32, 2, 0), ds.SubCh(4, 408, 24, 32, 2, 0, dab_plus=0)]


def _cfg(j):
    return cc.SCENARIOS[CAR[j]][2]


_case = {}


def _signal():
    """(sub-channels, IQ, the oracle receiver's results) -- built once, shared, left unchanged."""
    if not _case:
        subch = _layout()
        # (the time de-interleaver fills for 16 CIFs: the scenarios start there, behind sixteen frames of their end -- padding packets)
        behind = lambda f: np.concatenate([f[-16:], f[:4 * N_TX - 16]])      # noqa: E731
        pay = {j: behind(cc.scenario(name, 0)[2]) for j, name in CAR.items()}
        pay.update({j: behind(mc.mot_frames(*key)[0]) for j, (_, key) in MOT.items()})
        ens = ds.build_ensemble(N_TX, subch, seed=14, payloads=pay)
        x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=211.0, timing_offset=5555, seed=14, n_out=(N_TX + 1) * ds.TF)
        _case["v"] = (subch, x, oracle_run(x, subch))
    return _case["v"]


def _run(x, subch, what, streams=2, carousel=True, mot=True, calls=(3, 7, 1, 14, 4)):
    """delivery_sink.run with packet mode on sub-channels 1 and 2 (and carousel decoding with it), PAD decoding on sub-channel 0 (and MOT
    decoding with it).  Returns (sink, per (stream, slot) what the engine says after the run, frames decoded, slab size)."""
    def switch_on(eng, s):
        for j in CAR:
            eng.set_packet_mode(s, j, cc.ADDRESS)
            if carousel:
                eng.set_carousel_mode(s, j, **_cfg(j))
        for j in MOT:
            eng.set_pad_mode(s, j)
            if mot:
                eng.set_mot_mode(s, j)
        return (list(CAR) if carousel else []) + (list(MOT) if mot else [])

    def direct(eng, s, j):
        return (eng.carousel_stats(s, j) if j in CAR else eng.mot_stats(s, j), eng.read_mot_objects(s, j, 256), eng.subch_stats(s, j)["sf_count"])

    return run(x, subch, what, MOT_SECTION, streams, N_TX + 2, switch_on, direct, calls)


def _check_against_model(sink, direct, frames, ora, streams=2):
    for s in range(streams):
        assert frames[s] >= 26, frames
        for j, name in CAR.items():
            kbps = cc.SCENARIOS[name][0]
            lf = ora["msc"][j].reshape(-1, 3 * kbps)[:4 * frames[s] - 16]
            m = cc.model_of(pkc.run_model(lf, cc.ADDRESS), **_cfg(j))
            assert m.counters["objects"] >= 8 and m.counters["groups"] >= 40, (j, m.counters)      # there is traffic to deliver
            st, (r2, b2), _ = direct[(s, j)]
            rec, by = sink.items(s, j)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            assert all(st[k] == m.counters[k] for k in dx.CAROUSEL_COUNTERS), (s, j, st, m.counters)
            assert all(st[k] == int(sink.last[(s, j)][k]) for k in CHUNK_COUNTERS) and int(sink.last[(s, j)]["progress_events"]) == 0, (s, j, st, sink.last[(s, j)])
            assert st["objects_lost"] == 0 and st["active"] == 1 and st["dg_overrun"] == 0
            assert_tail_is_what_the_reader_returns(rec, by, r2, b2, 256)
        assert dx.MOT_FLAG_DIR_ELEMENT in sink.items(s, 2)[0]["au"]
        for j, (kbps, _) in MOT.items():                               # the PAD-MOT slot beside them
            st, (r2, b2), n_sf = direct[(s, j)]
            sfs = ora["sf"][j].reshape(-1, 110 * kbps // 8)[:n_sf]
            sfi = ora["sfi"][j].view(dx.SUPERFRAME_INFO)[:n_sf]
            m = mc.mot_model_of(pc.run_model(sfs, sfi), 65536)
            assert m.counters["objects"] >= 8, (j, m.counters)
            rec, by = sink.items(s, j)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            assert all(st[k] == m.counters[k] for k in dx.MOT_COUNTERS) and st["objects_lost"] == 0, (s, j, st, m.counters)
            assert all(st[k] == int(sink.last[(s, j)][k]) for k in CHUNK_COUNTERS + ("progress_events",)), (s, j, st, sink.last[(s, j)])
            assert_tail_is_what_the_reader_returns(rec, by, r2, b2, 256)


def test_the_section_carries_every_object_of_the_models_for_carousel_and_pad_mot_slots_of_one_engine():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=0)
    assert all(sink.off) and all(w == 7 | dx.DELIVER_DG | dx.DELIVER_PAD | dx.DELIVER_MOT for w in sink.whats) and all(n == slab for n in sink.sizes)
    _check_against_model(sink, direct, frames, ora)
    _case["objects"] = {k: sink.items(*k) for k in direct}


def test_fib_and_mot_alone_deliver_the_same_objects_and_carousel_slots_alone_have_their_section():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=dx.DELIVER_FIB | dx.DELIVER_MOT)
    assert all(w == dx.DELIVER_FIB | dx.DELIVER_MOT for w in sink.whats) and not sink.sf
    _check_against_model(sink, direct, frames, ora)
    if "objects" in _case:
        for k, (rec, by) in _case["objects"].items():
            assert sink.items(*k)[0].tobytes() == rec.tobytes() and np.array_equal(sink.items(*k)[1], by)
    # no MOT slot at all: the carousel slots alone bring the section, filled by their own gather launch
    sink, direct, frames, slab = _run(x, subch, what=dx.DELIVER_FIB | dx.DELIVER_MOT, streams=1, mot=False, calls=(7, 14, 8))
    assert all(sink.off) and set(direct) == {(0, j) for j in CAR}
    if "objects" in _case:
        for k in direct:
            assert sink.items(*k)[0].tobytes() == _case["objects"][k][0].tobytes() and np.array_equal(sink.items(*k)[1], _case["objects"][k][1])


def _documented(S, subch, packet_slots, pad_slots, object_bytes):
    """documented_slab_bytes (delivery_sink.py) with the MOT section of include/dabx.h behind the PAD section: the table and, per MOT slot
    and then per carousel slot, 16 records and 2 * max_object_bytes bytes (object_bytes: max_object_bytes of each, in that order)."""
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
        for _ in range(S * len(pad_slots)):
            off = up(off + 144 * 32 + 144 * 256 + 16896, 16)
    if object_bytes:
        off = up(off, 16) + S * M * 128
        for _ in range(S):
            for n in object_bytes:
                off = up(off + 16 * 32 + 2 * n, 16)
    off = up(off, 256)
    for _ in range(S):
        for c in subch:
            off = up(off + 4 * F * 3 * c.kbps, 16)
    return off


def test_without_a_carousel_or_mot_slot_the_slab_is_what_it_has_always_been_and_with_one_it_grows_by_the_documented_section():
    """No carousel and no MOT slot (packet mode and PAD decoding on as before): with what = 0 and with DABX_DELIVER_MOT set explicitly the
    slabs have no MOT section (off_mot = 0, the header's `what` without the bit) and the size is dabx_delivery_slab_bytes computed from the
    documented layout of before this section existed.  With carousel slots the size grows by exactly the documented section: the table
    and, per slot, 16 records and 2 * max_object_bytes bytes."""
    subch, x, ora = _signal()
    pkts, pads = tuple(CAR), tuple(MOT)
    want = documented_slab_bytes(1, subch, packet_slots=pkts, pad_slots=pads)
    assert want == _documented(1, subch, pkts, pads, ())
    a = _run(x, subch, what=0, streams=1, carousel=False, mot=False, calls=(7, 7))
    b = _run(x, subch, what=7 | dx.DELIVER_DG | dx.DELIVER_PAD | dx.DELIVER_MOT, streams=1, carousel=False, mot=False, calls=(7, 7))
    for sink, _, _, slab in (a, b):
        assert slab == want and all(n == want for n in sink.sizes) and not any(sink.off), (slab, want, sink.whats)
        assert all(w == 7 | dx.DELIVER_DG | dx.DELIVER_PAD for w in sink.whats), sink.whats
    for k in a[0].sf:
        assert np.array_equal(np.concatenate(a[0].sf[k]), np.concatenate(b[0].sf[k]))
    sizes = [_cfg(j)["max_object_bytes"] or 65536 for j in CAR]
    c = _run(x, subch, what=0, streams=1, carousel=True, mot=False, calls=(7,))
    assert c[3] == _documented(1, subch, pkts, pads, sizes) > want, (c[3], want)
    d = _run(x, subch, what=0, streams=1, carousel=True, mot=True, calls=(7,))
    assert d[3] == _documented(1, subch, pkts, pads, [65536] + sizes) > c[3], (d[3], c[3])
