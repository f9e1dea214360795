"""The service information followed inside the engine (dabx_fig_config.service_info; deliver.hip k_fig_si behind k_fic_frame, k_fig_directory):
a FIC-only engine of 6 streams fed through the FIC stage's test entries (dx.fic_inject / dx.fic_decode_frame, as tests/test_gpu_fig_engine.py
does), the switch on for streams 0, 2, 3, 5, the FIG mode without it for stream 1, nothing for stream 4, some streams absent in some steps.
After every frame the SI database, counters and events of the "on" streams equal the model of tests/fig_si_cases.py, and everything
dabx_fig_* returned before equals a twin engine that never sets the switch (its events minus kinds 6 .. 9).  dabx_fig_directory of all
streams in one call equals the per-stream calls and the model.  One small delivery case through IQ: the events of kinds 6 .. 9 arrive through
Chunk.fig, in both library forms."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fic_cases as fc
import fig_cases as fg
import fig_si_cases as si
from dabstar_amd import lib as dx
from test_gpu_fig_delivery import iq_of

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

S = 6
ON, PLAIN, OFF = (0, 2, 3, 5), 1, 4
SEQ = ("si_ensemble", "si_reconf_flags_1", "si_reconf_flags_3", "si_restart", "si_edges", "si_bad_crc")
ABSENT = {2: (3, 4), 3: (1,), 5: (0, 6)}     # stream -> steps in which it has no frame
N_FRAMES = 18
E_STATE = "error -5"
SI_GETTERS = ("fig_si_info", "fig_user_apps", "fig_global_defs", "fig_languages", "fig_programme_types", "fig_fec_schemes", "fig_clusters", "fig_si_stats",
              "fig_directory")


def _frames(name):
    """the first N_FRAMES frames of a sequence (a short one filled up with FIBs that hold no FIG), their CRC verdicts the sequence's"""
    fibs, crc = si.sequences()[name]
    n = 12 * N_FRAMES
    fibs = np.concatenate([fibs, np.stack([fc.FILLER] * n)])[:n].copy()
    crc = np.concatenate([crc, np.ones(n, np.uint8)])[:n]
    for f, ok in zip(fibs, crc):
        if not ok and fc.crc_good(f):
            f[30] ^= 0x01
        assert fc.crc_good(f) == bool(ok)
    return fibs.reshape(-1, 12, 32), crc.reshape(-1, 12)


@pytest.fixture(scope="module")
def soft():
    """[stream][frame] -> the frame's 9216 FIC soft bits: computed once"""
    return [[np.concatenate([fc.coded_block(f[3 * g:3 * g + 3]) for g in range(4)]) for f in _frames(name)[0]] for name in SEQ]


def _old_world(e, s, events=False):
    """everything the FIG mode returned before there was service information; dabx_fig_stats.events, the ring's index, counts the SI events of a
    stream with the switch on too: it is compared (events=True) where there can be none"""
    return dict(info=e.fig_info(s), sub=[[dx._subch_dict(q) for q in e.fig_subchannels(s, next=k)] for k in (False, True)],
                pk=[[tuple(int(v) for v in q) for q in e.fig_packet_components(s, next=k)] for k in (False, True)], labels=e.fig_labels(s),
                stats={k: v for k, v in e.fig_stats(s).items() if events or k != "events"}, follow=e.fig_follow(s))


@pytest.mark.parametrize("quirks", [False, True], ids=["default_swap", "reference_quirks"])
def test_the_si_database_equals_the_model_and_the_twin_is_not_disturbed(soft, quirks):
    kw = dict(n_streams=S, max_subch=0, fic_only=True, out_frames=4, ring_frames=2)
    eng, twin = dx.Engine(**kw), dx.Engine(**kw)
    model = {s: si.SiModel(quirks) for s in ON + (PLAIN,)}
    seen, seen_twin = {s: [] for s in ON + (PLAIN,)}, {s: [] for s in ON + (PLAIN,)}
    try:
        eng.set_fig_mode(PLAIN, reference_quirks=quirks)                     # first a stream without the switch: nothing of SI exists yet
        with pytest.raises(dx.DabxError, match=E_STATE):
            eng.fig_directory(-1)
        for s in ON:
            eng.set_fig_mode(s, reference_quirks=quirks, service_info=True)
        for s in ON + (PLAIN,):
            twin.set_fig_mode(s, reference_quirks=quirks)
        at, steps = [0] * S, 0
        while min(at) < N_FRAMES:
            present = [0 if (steps in ABSENT.get(s, ()) or at[s] >= N_FRAMES) else 1 for s in range(S)]
            for e in (eng, twin):
                for s in range(S):
                    x = soft[s][min(at[s], N_FRAMES - 1)]
                    dx.fic_inject(e, s, x if present[s] else -(x // 2) - 1)
                dx.fic_decode_frame(e, present)
            steps += 1
            for s in range(S):
                at[s] += present[s]
            for s in ON + (PLAIN,):
                if present[s]:
                    fibs, crc = eng.read_fibs(s, 1)
                    model[s].feed(fibs[0], crc[0])
                where = (steps, s, at[s])
                # the switch does not disturb what exists: the twin returns the same database, counters and -- but for the new kinds -- events
                assert _old_world(eng, s, s == PLAIN) == _old_world(twin, s, s == PLAIN), where      # (PLAIN: a stream without the switch inside a k_fig_si launch)
                ev, lost = eng.read_fig_events(s)
                ev2, lost2 = twin.read_fig_events(s)
                seen[s] += ev
                seen_twin[s] += ev2
                assert lost == lost2 == 0 and [e for e in seen[s] if e["kind"] < dx.FIG_SI_TABLE] == seen_twin[s], where
                if s == PLAIN:
                    assert seen[s] == seen_twin[s], where
                    continue
                assert seen[s] == model[s].events, where
                want = model[s].si_row()
                got = dict(info=eng.fig_si_info(s), stats=eng.fig_si_stats(s), global_defs=[eng.fig_global_defs(s, next=k) for k in (False, True)],
                           user_apps=[eng.fig_user_apps(s, next=k) for k in (False, True)], fec=[eng.fig_fec_schemes(s, next=k) for k in (False, True)],
                           clusters=[eng.fig_clusters(s, next=k) for k in (False, True)], languages=eng.fig_languages(s), ptys=eng.fig_programme_types(s))
                assert got == want, (where, [k for k in got if got[k] != want[k]])
                for k in (False, True):
                    assert eng.fig_directory(s, next=k) == model[s].directory(int(k)), (where, k)
            if steps in (1, 7, N_FRAMES):                                    # all streams in one launch and one copy
                for k in (False, True):
                    rows = eng.fig_directory(-1, next=k)
                    assert len(rows) == S and rows[PLAIN] == rows[OFF] == []
                    assert [rows[s] for s in ON] == [eng.fig_directory(s, next=k) for s in ON] == [model[s].directory(int(k)) for s in ON], (steps, k)
            for s in (PLAIN, OFF):                                           # the SI getters refuse a stream without the switch
                for name in SI_GETTERS:
                    with pytest.raises(dx.DabxError, match=E_STATE):
                        getattr(eng, name)(s)
        assert steps == N_FRAMES + 2 and all(model[s].fibs == 12 * N_FRAMES for s in ON)
        kinds = {e["kind"] for s in ON for e in seen[s]}
        assert {dx.FIG_SI_TABLE, dx.FIG_TIME, dx.FIG_ANNOUNCE_START, dx.FIG_ANNOUNCE_STOP} <= kinds
        assert model[PLAIN].n_changes == (0 if quirks else 1) and model[2].n_changes == 1 and model[3].n_restarts == 1 and model[5].cnt["fibs_bad"] > 30
        assert len(model[0].directory(0)) == 19 and sum(r["reference_defined"] for r in model[0].directory(0)) >= 18
        # a truncated directory: the count is the table's, the rows the caller's room
        L = dx.load()
        out, n = np.zeros(4, dx.FIG_SERVICE), np.zeros(1, np.int32)
        assert L.dabx_fig_directory(eng._h, 0, 0, dx._p(out), 4, dx._p(n)) == 0 and int(n[0]) == 19
        assert [dx.fig_service_dict(r) for r in out] == model[0].directory(0)[:4]
        assert L.dabx_fig_directory(eng._h, 0, 0, None, 0, dx._p(n)) == 0 and int(n[0]) == 19
        assert L.dabx_fig_directory(eng._h, S, 0, dx._p(out), 4, dx._p(n)) == -2 and L.dabx_fig_directory(eng._h, 0, 0, dx._p(out), 4, None) == -2
        # the switch off again and on again: the stream's FIG database stays, its service information starts afresh
        eng.set_fig_mode(0, reference_quirks=quirks)
        with pytest.raises(dx.DabxError, match=E_STATE):
            eng.fig_si_info(0)
        assert eng.fig_info(0) == model[0].info()
        eng.set_fig_mode(0, reference_quirks=quirks, service_info=True)
        assert eng.fig_si_info(0) == si.SiModel().si_row()["info"] and eng.fig_info(0) == model[0].info() and eng.fig_si_info(2) == model[2].si_row()["info"]
        # the twin never had anything of it
        for name in SI_GETTERS:
            with pytest.raises(dx.DabxError, match=E_STATE):
                getattr(twin, name)(0)
        # every stream's switch off again, the service information still allocated: the engine is back to k_fig, and a further frame of
        # every stream leaves it where it leaves the twin
        for s in ON:
            eng.set_fig_mode(s, reference_quirks=quirks)
            eng.read_fig_events(s), twin.read_fig_events(s)
        before = {s: (eng.fig_stats(s)["events"], twin.fig_stats(s)["events"]) for s in ON + (PLAIN,)}
        for e in (eng, twin):
            for s in range(S):
                dx.fic_inject(e, s, soft[s][0])
            dx.fic_decode_frame(e, [1] * S)
        for s in ON + (PLAIN,):
            assert _old_world(eng, s) == _old_world(twin, s), s
            assert eng.fig_info(s)["fibs_processed"] == 12 * (N_FRAMES + 1)
            new, new2 = eng.read_fig_events(s), twin.read_fig_events(s)
            assert new == new2 and all(e["kind"] < dx.FIG_SI_TABLE for e in new[0]), s
            assert eng.fig_stats(s)["events"] - before[s][0] == twin.fig_stats(s)["events"] - before[s][1] == len(new[0]), s
            with pytest.raises(dx.DabxError, match=E_STATE):
                eng.fig_si_info(s)
        with pytest.raises(dx.DabxError, match=E_STATE):
            eng.fig_directory(-1)
    finally:
        eng.close()
        twin.close()


# ---- the delivery: SI events through Chunk.fig -----------------------------------------------------------------------------------------------------
D_FRAMES, CALLS = 15, (7, 7)


def event_fibs():
    """15 frames: FIG 0/9, 0/10 and 0/18 at the head of every frame, a FIG 0/19 that meets the cluster's flags in six frames of seven and
    one that does not in the seventh: SI_TABLE, TIME in every frame, a start after five, a stop"""
    out = []
    for f in range(D_FRAMES):
        asw = 0x0000 if f % 7 == 6 else 0x0002
        out.append(fg.one_fib(si.f09(2, 0xE1, 1), si.f10(60000 + f, 10, f, 30), si.fig0(18, si.e18(0x1000, 0x0002, [2])), si.fig0(19, si.e19(2, asw, 5))))
        out += [fg.one_fib(si.fig0(5, si.e05(f, 8)))] + [fc.FILLER] * 10
    return np.stack(out)


def test_the_si_events_arrive_through_the_chunk():
    x = iq_of(event_fibs(), 1)
    eng = dx.Engine(n_streams=2, ring_frames=D_FRAMES + 2, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, schedule=1)
    try:
        for s in range(2):
            eng.push_iq(s, x)
        eng.set_fig_mode(0, service_info=True)
        eng.set_fig_mode(1)                                                  # the same signal without the switch
        eng.delivery_open(slots=4, what=dx.DELIVER_FIB | dx.DELIVER_FIG)
        m, kinds = si.SiModel(), set()
        for n in CALLS:
            eng.process(n)
            ch = eng.delivery_next(wait=True)
            assert ch is not None
            nf = int(ch.streams[0]["n_frames"])
            assert nf >= 6 and nf == int(ch.streams[1]["n_frames"])
            before = len(m.events)
            m.feed(ch.fibs[0, :nf].reshape(-1, 32), ch.crc[0, :nf].reshape(-1))
            new = m.events[before:]
            assert 0 < len(new) <= dx.FIG_CHUNK_RECORDS and ch.fig(0) == new == eng.read_fig_events(0)[0]
            assert ch.fig(1) == [e for e in new if e["kind"] < dx.FIG_SI_TABLE] == eng.read_fig_events(1)[0]
            kinds |= {e["kind"] for e in ch.fig(0)}
            ch.release()
        assert {dx.FIG_SI_TABLE, dx.FIG_TIME, dx.FIG_ANNOUNCE_START, dx.FIG_ANNOUNCE_STOP} <= kinds
        assert eng.fig_si_info(0) == m.si_row()["info"] and eng.fig_languages(0) == m.si_row()["languages"]
        eng.delivery_close()
    finally:
        eng.close()


def test_the_si_events_arrive_in_the_hipmodule_form():
    """the test above again with the binding pointed at hipmodule/libdabx.so: k_fig_si is found in the code objects"""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_fig_si_engine.py", "-k", "through_the_chunk"],
                       cwd=ROOT, env=hipmodule_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "1 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
