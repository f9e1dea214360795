"""The FIC followed on the device inside the engine (dabx_set_fig_mode, deliver.hip k_fig behind k_fic_frame): a FIC-only engine of 6 streams fed
through the FIC stage's test entries (dx.fic_inject / dx.fic_decode_frame: crafted FIBs as clean coded blocks, no front end), modes on for
streams 0, 2, 3, 5 and off for 1, 4, some streams absent in some steps.  After every frame the getters of the "on" streams equal a dabx_fibdec
fed with read_fibs of the same frames (and the Python model of tests/fig_cases.py for labels, counters and events), and fig_follow equals
what follow_fic reports on a twin engine with the mode off.  One case runs through the front end, in the few-stream and the many-stream
schedule."""
import os
import sys

import numpy as np
import pytest

import fic_cases as fc
import fig_cases as fg
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

pytestmark = pytest.mark.gpu

S = 6
ON = (0, 2, 3, 5)
SEQ = ("ensemble18", "reconf_flags_1_fig00_last", "reconf_flags_3_fig00_first", "restart_labels", "reconf_flags_2_fig00_first", "bad_crc")
ABSENT = {2: (3, 4), 4: (1,), 5: (0, 6)}     # stream -> steps in which it has no frame
N_FRAMES = 10                                # every sequence is 120 FIBs
E_STATE = "error -5"


def _frames(name):
    """a sequence as frames of 12 FIBs whose CRC verdict is the sequence's: a FIB that must fail gets a CRC bit flipped where it would pass"""
    fibs, crc = fg.sequences()[name]
    fibs = fibs.copy()
    for f, ok in zip(fibs, crc):
        if not ok and fc.crc_good(f):
            f[30] ^= 0x01
        assert fc.crc_good(f) == bool(ok)
    return fibs.reshape(-1, 12, 32), crc.reshape(-1, 12)


@pytest.fixture(scope="module")
def soft():
    """[stream][frame] -> the frame's 9216 FIC soft bits: computed once"""
    out = []
    for name in SEQ:
        fr, _ = _frames(name)
        assert fr.shape[0] == N_FRAMES
        out.append([np.concatenate([fc.coded_block(f[3 * g:3 * g + 3]) for g in range(4)]) for f in fr])
    return out


def _tab(descs):
    return [dx._subch_dict(q) for q in descs]


def _pk(a):
    return [tuple(int(v) for v in q) for q in a]


@pytest.mark.parametrize("quirks", [False, True], ids=["default_swap", "reference_quirks"])
def test_the_getters_equal_fibdec_and_the_twin_after_every_frame(soft, quirks):
    eng = dx.Engine(n_streams=S, max_subch=0, fic_only=True, out_frames=4, ring_frames=2)
    twin = dx.Engine(n_streams=S, max_subch=0, fic_only=True, out_frames=4, ring_frames=2)
    dec = {s: dx.FibDecoder(reference_quirks=quirks) for s in ON}
    model = {s: fg.Model(quirks) for s in ON}
    seen = {s: [] for s in ON}
    try:
        assert eng.fig_stats(0)["launches"] == 0
        for s in ON:
            eng.set_fig_mode(s, reference_quirks=quirks)
        eng.set_fig_reference_quirks(quirks)                                 # (the host decoders of the "off" streams: the engine's own setting)
        twin.set_fig_reference_quirks(quirks)
        at = [0] * S
        steps = 0
        while min(at) < N_FRAMES:
            present = [0 if (steps in ABSENT.get(s, ()) or at[s] >= N_FRAMES) else 1 for s in range(S)]
            for e in (eng, twin):
                for s in range(S):
                    x = soft[s][min(at[s], N_FRAMES - 1)]
                    dx.fic_inject(e, s, x if present[s] else -(x // 2) - 1)      # an absent stream's soft bits would decode to something else
                dx.fic_decode_frame(e, present)
            steps += 1
            for s in range(S):
                at[s] += present[s]
            for s in ON:
                if present[s]:
                    fibs, crc = eng.read_fibs(s, 1)
                    want_f, want_c = _frames(SEQ[s])
                    assert np.array_equal(fibs[0], want_f[at[s] - 1]) and np.array_equal(crc[0], want_c[at[s] - 1]), (steps, s)
                    dec[s].process(fibs[0], crc[0])
                    model[s].feed(fibs[0], crc[0])
                if at[s] == 0:
                    assert eng.fig_info(s)["fibs_processed"] == 0
                    continue
                where = (steps, s, at[s])
                assert eng.fig_info(s) == dec[s].info() == model[s].info(), where
                for nxt in (False, True):
                    assert _tab(eng.fig_subchannels(s, next=nxt)) == _tab(dec[s].subchannels(next=nxt)) == model[s].subch(int(nxt)), where
                    assert _pk(eng.fig_packet_components(s, next=nxt)) == _pk(dec[s].packet_components(next=nxt)) == model[s].packets(int(nxt)), where
                row = model[s].row()
                assert eng.fig_labels(s) == row["labels"], where
                st = eng.fig_stats(s)
                assert {k: st[k] for k in fg.COUNTERS} == row["stats"] and st["launches"] == steps, where
                ev, lost = eng.read_fig_events(s)
                seen[s] += ev
                assert lost == 0 and seen[s] == model[s].events, where
                assert eng.fig_follow(s) == twin.follow_fic(s) == model[s].follow(at[s]), where
            for s in range(S):
                if s in ON:
                    with pytest.raises(dx.DabxError, match=E_STATE):         # the device's decoder follows this stream
                        eng.follow_fic(s)
                else:                                                        # an "off" stream owns no state, and the host path still works on it
                    for call in (eng.fig_info, eng.fig_subchannels, eng.fig_packet_components, eng.fig_labels, eng.fig_follow, eng.read_fig_events):
                        with pytest.raises(dx.DabxError, match=E_STATE):
                            call(s)
                    assert eng.fig_stats(s)["fibs_good"] == 0
                    assert eng.follow_fic(s) == twin.follow_fic(s)
        assert steps == N_FRAMES + 2 and all(model[s].fibs == 12 * N_FRAMES for s in ON)
        assert any(model[s].n_changes for s in ON) and model[3].n_restarts == 2 and len(model[0].labels) >= 19
        # off and on again: an empty database, which then follows the next frame like a decoder that has skipped the frames before it
        eng.set_fig_mode(0, enable=False)
        with pytest.raises(dx.DabxError, match=E_STATE):
            eng.fig_info(0)
        assert eng.follow_fic(0)["frames_fed"] == N_FRAMES                  # the host path is back
        eng.set_fig_mode(0, reference_quirks=quirks)
        assert eng.fig_info(0) == fg.Model().info() and eng.fig_labels(0) == [] and eng.fig_subchannels(0) == [] and eng.read_fig_events(0) == ([], 0)
        dx.fic_inject(eng, 0, soft[0][0])
        dx.fic_decode_frame(eng, [1, 0, 0, 0, 0, 0])
        fresh = fg.Model(quirks)
        fresh.fibs = 12 * N_FRAMES
        fresh.feed(*[a[0] for a in _frames(SEQ[0])])
        assert eng.fig_info(0) == fresh.info() and eng.fig_info(0)["fig00_fib"] >= 12 * N_FRAMES
        assert _tab(eng.fig_subchannels(0)) == fresh.subch(0) and eng.fig_labels(0) == fresh.row()["labels"] and eng.read_fig_events(0) == (fresh.events, 0)
        assert eng.fig_info(2) == dec[2].info()                             # the others were not touched (stream 2 had no frame in that step)
    finally:
        for d in dec.values():
            d.close()
        eng.close()
        twin.close()


def test_an_engine_that_never_enables_the_mode_has_nothing_of_it():
    eng = dx.Engine(n_streams=2, max_subch=0, fic_only=True, out_frames=2, ring_frames=2)
    try:
        eng.set_fig_mode(-1, enable=False)                                   # switching off what was never on: nothing is created
        dx.fic_inject(eng, 0, np.concatenate([fc.coded_block([fc.FILLER] * 3)] * 4))
        dx.fic_decode_frame(eng, [1, 0])
        st = eng.fig_stats(0)
        assert st["launches"] == 0 and st["fibs_good"] == 0
        with pytest.raises(dx.DabxError, match=E_STATE):
            eng.fig_info(0)
        assert eng.follow_fic(0)["frames_fed"] == 1
        L = dx.load()
        assert L.dabx_set_fig_mode(eng._h, 2, None) == -2 and L.dabx_set_fig_mode(eng._h, -2, None) == -2 and L.dabx_fig_info(eng._h, 0, None) == -2
    finally:
        eng.close()


@pytest.mark.parametrize("n_streams", [1, 48], ids=["few_stream_chain", "many_stream_step"])
def test_through_the_front_end_the_table_is_the_discovered_one(n_streams):
    """A few frames (3 to 5 decode, by how quick the search is) of synthesiser IQ on stream 0: the device's current table is dabx_discover_subchannels' (FIG 0/1 and 0/2 of the same frames).
    The synthesiser sends no FIG 1: no label, and no label event."""
    sub = ds.default_subchannels(6, 64)
    ens = ds.build_ensemble(5, sub, seed=11)
    x = ds.channel(ens.iq, snr_db=30.0, timing_offset=2000, seed=1, n_out=5 * ds.TF + 8000)
    eng = dx.Engine(n_streams=n_streams, ring_frames=7, max_subch=0, fic_only=True, out_frames=8)
    try:
        eng.set_fig_mode(0)
        eng.push_iq(0, x)
        eng.process(8)
        frames = eng.stats(0)["frames"]
        assert 3 <= frames <= 5
        assert _tab(eng.fig_subchannels(0)) == _tab(eng.discover_subchannels(0)) and len(eng.fig_subchannels(0)) == 6
        info = eng.fig_info(0)
        assert info["fibs_processed"] == 12 * frames and info["cif_count"] == eng.stats(0)["cif_count"] and info["n_restarts"] == 0
        ev, lost = eng.read_fig_events(0)
        assert lost == 0 and ev and all(e["kind"] == dx.FIG_TABLE for e in ev) and eng.fig_labels(0) == []
        assert ev[-1]["n_subch"] == 6 and ev[-1]["n_components"] == 6
        fibs, crc = eng.read_fibs(0, frames)
        m = fg.Model().feed(fibs.reshape(-1, 32), crc.reshape(-1))
        assert ev == m.events and eng.fig_follow(0) == m.follow(frames)
        assert eng.fig_stats(0)["launches"] == 8
    finally:
        eng.close()
