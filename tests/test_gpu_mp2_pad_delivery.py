"""The PAD section of the delivery slab with an MP2 source slot in it, through IQ: an ensemble whose DAB audio sub-channel 2 carries an MP2
PAD scenario of tests/mp2_pad_cases.py and whose DAB+ sub-channel 1 carries a PAD scenario of tests/pad_cases.py is pushed as IQ on two
streams, a delivery is open and a consumer thread takes the chunks while dabx_process runs -- k_pad and k_pad_mp2 inside the real chain, on
the MSC batch's stream, k_deliver_pad behind them with no change of its own.

Concatenated over the chunks, the MP2 slot's section is the COMPLETE sequence of items of the model run on the oracle receiver's logical
frames of the same IQ, the DAB+ slot's that of pad_cases' model on the oracle receiver's super frames -- records by .tobytes(), bytes by
np.array_equal, counters by == --, both equal dabx_read_pad_items and dabx_get_pad_stats, and items_lost == 0."""
import os
import sys

import numpy as np
import pytest

import mp2_pad_cases as mc
import pad_cases as pc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from delivery_sink import CHUNK_COUNTERS, PAD, assert_tail_is_what_the_reader_returns, run  # noqa: E402
from oracle_lib import oracle_run  # noqa: E402

pytestmark = pytest.mark.gpu

N_TX = 30                                   # transmitted frames
DABPLUS = (1, 64, 31)                       # sub-channel index, kbit/s, scenario seed
MP2 = (2, 64, 33)                           # ... of the MP2 source slot (frame_plan variant 0: both rates and the refused headers in 120 frames)
STREAMS = 2


def _layout():
    return [ds.SubCh(0, 0, 48, 64, 2, 0), ds.SubCh(1, 48, 48, 64, 2, 0), ds.SubCh(2, 96, 48, 64, 2, 0, dab_plus=0), ds.SubCh(3, 144, 24, 32, 2, 0, dab_plus=0)]


def test_the_section_carries_every_item_of_both_sources_and_equals_the_per_slot_reader():
    subch = _layout()
    # (the time de-interleaver fills for 16 CIFs: the scenarios start there, behind sixteen frames of their ends)
    a = pc.scenario(DABPLUS[1], DABPLUS[2])[0]
    b = mc.scenario(MP2[1], MP2[2], 0, 4 * N_TX)[0]
    pay = {DABPLUS[0]: np.concatenate([a[-16:], a[:4 * N_TX - 16]]), MP2[0]: np.concatenate([b[-16:], b[:-16]])}
    ens = ds.build_ensemble(N_TX, subch, seed=12, payloads=pay)
    x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=217.0, timing_offset=5555, seed=12, n_out=(N_TX + 1) * ds.TF)
    ora = oracle_run(x, subch)
    def switch_on(eng, s):
        eng.set_pad_mode(s, DABPLUS[0])
        eng.set_pad_mode(s, MP2[0], source="mp2")
        return [DABPLUS[0], MP2[0]]

    sink, direct, frames, _ = run(x, subch, 0, PAD, STREAMS, N_TX + 2, switch_on,
                                  lambda eng, s, j: (eng.pad_stats(s, j), eng.read_pad_items(s, j, 512), eng.subch_stats(s, j), eng.mp2_sync_stats(s, j)))
    assert all(sink.off) and all(w == 7 | dx.DELIVER_PAD for w in sink.whats)
    for s in range(STREAMS):
        assert frames[s] >= 26, frames
        for j, kbps, _ in (DABPLUS, MP2):
            st, (r2, b2), sub, sync = direct[(s, j)]
            if j == MP2[0]:
                n = sub["cifs_decoded"]
                lf = np.frombuffer(ora["msc"][j], np.uint8).reshape(-1, 3 * kbps)[:n]
                assert n >= 80 and len(lf) == n
                mm = mc.run_model(kbps, lf)
                m, counters = mm.pad, mm.pad.counters
                assert sync == mm.sync_stats() and sync["syncs"] >= 60 and mm.branch["mp2:263 rate 48000 -> 24000"] >= 1, (s, sync, mm.sync_stats())
                assert counters["labels"] >= 3 and counters["groups"] >= 3 and counters["pad_aus"] >= 60, counters       # there is traffic to deliver
            else:
                n_sf = sub["sf_count"]
                m = pc.run_model(ora["sf"][j].reshape(-1, 110 * kbps // 8)[:n_sf], ora["sfi"][j].view(dx.SUPERFRAME_INFO)[:n_sf])
                counters = m.counters
                assert n_sf >= 15 and counters["labels"] >= 1 and counters["groups"] >= 3 and not any(sync.values()), (counters, sync)
            rec, by = sink.items(s, j)
            assert rec.tobytes() == m.records().tobytes() and np.array_equal(by, m.all_bytes()), (s, j, len(rec), len(m.rows))
            assert all(st[k] == counters[k] for k in pc.PAD_COUNTERS), (s, j, st, counters)
            assert all(st[k] == int(sink.last[(s, j)][k]) for k in CHUNK_COUNTERS), (s, j, st, sink.last[(s, j)])
            assert st["items_lost"] == 0 and st["active"] == 1
            # ... and they are what the per-slot reader returns (its byte_pos counts from its own first item)
            assert_tail_is_what_the_reader_returns(rec, by, r2, b2, 512)
