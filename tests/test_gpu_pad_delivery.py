"""The PAD section of the delivery slab (include/dabx.h, dabx_chunk_pad; k_deliver_pad behind k_deliver_dg), through IQ: an ensemble whose
DAB+ sub-channels 1 and 4 carry the PAD scenarios of tests/pad_cases.py is pushed as IQ on two streams, a delivery is open and a consumer
thread takes the chunks while dabx_process runs -- k_pad inside the real chain, behind k_dabplus on the MSC batch's stream.

Concatenated over the chunks, a slot's section is the COMPLETE sequence of items of the model run on the oracle receiver's super frames
of the same IQ -- records by .tobytes(), bytes by np.array_equal, counters by == --, it equals dabx_read_pad_items and
dabx_get_pad_stats, and items_lost == 0."""
import os
import sys

import numpy as np
import pytest

import pad_cases as pc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import CHUNK_COUNTERS, PAD as PAD_SECTION, assert_tail_is_what_the_reader_returns, documented_slab_bytes, run  # noqa: E402
from oracle_lib import oracle_run  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
PAD = {1: (64, 31), 4: (32, 32)}            # sub-channel index -> (kbit/s, scenario seed)

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
        _case["v"] = (subch, x, oracle_run(x, subch))
    return _case["v"]


def _run(x, subch, what, streams=2, pad=True, calls=(3, 7, 1, 14, 4)):
    """delivery_sink.run with PAD decoding on the PAD slots.  Returns (sink, per (stream, slot) PAD stats, the newest items as
    dabx_read_pad_items gives them and the slot's super-frame count, frames decoded, slab size)."""
    def switch_on(eng, s):
        for j in PAD:
            if pad:
                eng.set_pad_mode(s, j)
        return list(PAD) if pad else []

    return run(x, subch, what, PAD_SECTION, streams, N_TX + 2, switch_on,
               lambda eng, s, j: (eng.pad_stats(s, j), eng.read_pad_items(s, j, 512), eng.subch_stats(s, j)["sf_count"]), calls)


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
            assert_tail_is_what_the_reader_returns(rec, by, r2, b2, 512)


def test_the_section_carries_every_item_of_the_model_on_the_oracle_receivers_super_frames():
    subch, x, ora = _signal()
    sink, direct, frames, slab = _run(x, subch, what=0)
    assert all(sink.off) and all(w == 7 | dx.DELIVER_PAD for w in sink.whats) and all(n == slab for n in sink.sizes)
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


def test_without_a_pad_slot_the_slab_is_what_it_has_always_been():
    """No PAD slot: with what = 0 and with DABX_DELIVER_PAD set explicitly the slabs have no section (off_pad = 0, the header's `what`
    without the bit), the size is dabx_delivery_slab_bytes computed from the documented layout -- the layout before this section existed --
    and the two runs' slabs carry the same super frames.  With PAD slots the size grows by exactly the documented section: the table and,
    per PAD slot, 144 records and 144 * 256 + 16 896 bytes."""
    subch, x, ora = _signal()
    a = _run(x, subch, what=0, streams=1, pad=False, calls=(7, 7))
    b = _run(x, subch, what=7 | dx.DELIVER_PAD, streams=1, pad=False, calls=(7, 7))
    want = documented_slab_bytes(1, subch)
    for sink, _, _, slab in (a, b):
        assert slab == want and all(n == want for n in sink.sizes) and not any(sink.off) and all(w == 7 for w in sink.whats), (slab, want, sink.whats)
    for k in a[0].sf:
        assert np.array_equal(np.concatenate(a[0].sf[k]), np.concatenate(b[0].sf[k]))
    c = _run(x, subch, what=0, streams=1, pad=True, calls=(7,))
    assert c[3] == documented_slab_bytes(1, subch, pad_slots=tuple(PAD)) > want, (c[3], want)
