"""The MOT section of the delivery slab (include/dabx.h, dabx_chunk_mot; k_deliver_mot behind k_deliver_pad), through IQ: an ensemble whose
DAB+ sub-channels 0 and 1 carry the MOT scenarios of tests/mot_cases.py in their X-PADs is pushed as IQ on two streams, a delivery is open
and a consumer thread takes the chunks while dabx_process runs -- k_mot inside the real chain, behind k_pad on the MSC batch's stream.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of objects of MotModel run on the PAD model's items of the oracle
receiver's super frames of the same IQ -- records by .tobytes(), bytes by np.array_equal, counters by == --, it equals
dabx_read_mot_objects and dabx_get_mot_stats, and objects_lost == 0."""
import os
import sys

import numpy as np
import pytest

import mot_cases as mc
import pad_cases as pc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import Section, assert_tail_is_what_the_reader_returns, documented_slab_bytes, run  # noqa: E402
from oracle_lib import oracle_run  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
MOT = {0: (64, (1, 0)), 1: (64, (0, 0))}    # sub-channel index -> (kbit/s, (stream, slot) of mot_cases' scenario it carries)
MOT_SECTION = Section("mot", "mot_objects", "off_mot", dx.CHUNK_MOT, "first_object", "n_objects", "objects_lost", "rec_off", ("objects",),
                      ("object_bytes",), 16, 2 * 65536, dx.MOT_OBJECT)
CHUNK_COUNTERS = ("objects", "object_bytes", "groups", "headers", "segments", "crc_bad", "grp_short", "hdr_bad", "obj_overflow", "resets", "progress_events")


def _layout():
    return [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 48, 64, 2, 0), ds.SubCh(2, 96, 48, 64, 2, 0, dab_plus=0), ds.SubCh(3, 144, 72, 96, 2, 0),
            ds.SubCh(4, 216, 24, 32, 2, 0), ds.SubCh(5, 240, 24, 32, 2, 0, dab_plus=0)]


_case = {}


def _signal():
    """(sub-channels, IQ, the oracle receiver's results) -- built once, shared, left unchanged."""
    if not _case:
        subch = _layout()
        # (the time de-interleaver fills for 16 CIFs: the scenario starts there, behind sixteen frames of its end)
        pay = {j: np.concatenate([mc.mot_frames(*key)[0][-16:], mc.mot_frames(*key)[0][:4 * N_TX - 16]]) for j, (_, key) in MOT.items()}
        pay[4] = np.concatenate([pc.scenario(32, 32)[0][-16:], pc.scenario(32, 32)[0][:4 * N_TX - 16]])
        ens = ds.build_ensemble(N_TX, subch, seed=12, payloads=pay)
        x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=-183.0, timing_offset=4444, seed=12, n_out=(N_TX + 1) * ds.TF)
        _case["v"] = (subch, x, oracle_run(x, subch))
    return _case["v"]


def _run(x, subch, what, streams=2, mot=True, calls=(3, 7, 1, 14, 4)):
    """delivery_sink.run with PAD decoding on sub-channels 0, 1 and 4 and MOT decoding on 0 and 1.  Returns (sink, per (stream, slot) MOT
    stats, the newest objects as dabx_read_mot_objects gives them and the slot's super-frame count, frames decoded, slab size)."""
    def switch_on(eng, s):
        for j in list(MOT) + [4]:
            eng.set_pad_mode(s, j)
            if mot and j in MOT:
                eng.set_mot_mode(s, j)
        return list(MOT) if mot else []

    return run(x, subch, what, MOT_SECTION, streams, N_TX + 2, switch_on,
               lambda eng, s, j: (eng.mot_stats(s, j), eng.read_mot_objects(s, j, 256), eng.subch_stats(s, j)["sf_count"]), calls)


def _check_against_model(sink, direct, frames, ora, streams=2):
    for s in range(streams):
        assert frames[s] >= 26, frames
        for j, (kbps, _) in MOT.items():
            st, (r2, b2), n_sf = direct[(s, j)]
            sfs = ora["sf"][j].reshape(-1, 110 * kbps // 8)[:n_sf]
            sfi = ora["sfi"][j].view(dx.SUPERFRAME_INFO)[:n_sf]
            assert n_sf >= 15 and len(sfs) == n_sf
            m = mc.mot_model_of(pc.run_model(sfs, sfi), 65536)
            assert m.counters["objects"] >= 8 and m.counters["groups"] >= 40, (j, m.counters)      # there is traffic to deliver
            rec, by = sink.items(s, j)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            assert all(st[k] == m.counters[k] for k in dx.MOT_COUNTERS), (s, j, st, m.counters)
            assert all(st[k] == int(sink.last[(s, j)][k]) for k in CHUNK_COUNTERS), (s, j, st, sink.last[(s, j)])
            assert st["objects_lost"] == 0 and st["active"] == 1
            # ... and they are what the per-slot reader returns (its byte_pos counts from its own first object)
            assert_tail_is_what_the_reader_returns(rec, by, r2, b2, 256)


def test_the_section_carries_every_object_of_the_model_on_the_oracle_receivers_super_frames():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=0)
    assert all(sink.off) and all(w == 7 | dx.DELIVER_PAD | dx.DELIVER_MOT for w in sink.whats) and all(n == slab for n in sink.sizes)
    _check_against_model(sink, direct, frames, ora)
    _case["objects"] = {k: sink.items(*k) for k in direct}


def test_fib_and_mot_alone_deliver_the_same_objects():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=dx.DELIVER_FIB | dx.DELIVER_MOT)
    assert all(w == dx.DELIVER_FIB | dx.DELIVER_MOT for w in sink.whats) and not sink.sf
    _check_against_model(sink, direct, frames, ora)
    if "objects" in _case:
        for k, (rec, by) in _case["objects"].items():
            assert sink.items(*k)[0].tobytes() == rec.tobytes() and np.array_equal(sink.items(*k)[1], by)


def _documented(S, subch, pad_slots, mot_slots):
    """documented_slab_bytes (delivery_sink.py) with the MOT section of include/dabx.h behind the PAD section: the table and, per MOT
    slot, 16 records and 2 * max_object_bytes bytes."""
    up = lambda v, a: (v + a - 1) // a * a           # noqa: E731
    M, F = len(subch), 7
    off = up(128 + S * 72, 16)
    off = up(off + S * M * 144, 16)
    off = up(off + S * F * 384, 16); off = up(off + S * F * 12, 16); off = up(off + S * F * 16, 16)
    for _ in range(S):
        for c in subch:
            if c.dab_plus:
                off = up(off + 6 * ((110 * (c.kbps // 8) + 3) & ~3), 16) + 6 * 32
    for slots, recs, nbytes in ((pad_slots, 144, 144 * 256 + 16896), (mot_slots, 16, 2 * 65536)):
        if slots:
            off = up(off, 16) + S * M * 128
            for _ in range(S * len(slots)):
                off = up(off + recs * 32 + nbytes, 16)
    off = up(off, 256)
    for _ in range(S):
        for c in subch:
            off = up(off + 4 * F * 3 * c.kbps, 16)
    return off


def test_without_a_mot_slot_the_slab_is_what_it_has_always_been():
    """No MOT slot (PAD decoding on as before): with what = 0 and with DABX_DELIVER_MOT set explicitly the slabs have no MOT section
    (off_mot = 0, the header's `what` without the bit) and the size is dabx_delivery_slab_bytes computed from the documented layout of
    before this section existed.  With MOT slots the size grows by exactly the documented section."""
    subch, x, ora = _signal()
    pads = tuple(MOT) + (4,)
    want = documented_slab_bytes(1, subch, pad_slots=pads)
    assert want == _documented(1, subch, pads, ())
    a = _run(x, subch, what=0, streams=1, mot=False, calls=(7, 7))
    b = _run(x, subch, what=7 | dx.DELIVER_PAD | dx.DELIVER_MOT, streams=1, mot=False, calls=(7, 7))
    for sink, _, _, slab in (a, b):
        assert slab == want and all(n == want for n in sink.sizes) and not any(sink.off) and all(w == 7 | dx.DELIVER_PAD for w in sink.whats), (slab, want, sink.whats)
    for k in a[0].sf:
        assert np.array_equal(np.concatenate(a[0].sf[k]), np.concatenate(b[0].sf[k]))
    c = _run(x, subch, what=0, streams=1, mot=True, calls=(7,))
    assert c[3] == _documented(1, subch, pads, tuple(MOT)) > want, (c[3], want)
