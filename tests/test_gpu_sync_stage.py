"""GPU: the two decisions in front of the frame chain on the crafted inputs of tests/sync_cases.py -- prs_correlate_block (lock / no lock,
start_index) through dx.prs_correlate and coarse_cfo_block (the +-70-carrier decision, the f_sync reset) through dx.coarse_cfo, one block
per row -- and both inside the engine on a stream whose coarse estimate is not finite.  The expected values are the oracle's; that the
inputs leave the device no room (every comparison of a correlator walk 2e-5 max(pk) wide, offset * 1000 at least 4 D from an integer) is
proven on the CPU by tests/test_sync_cases.py.  docs/history/sync_stage_tests.md has the figures."""
import numpy as np
import pytest

import oracle_lib as ol
import sync_cases as sc
from dabstar_amd import lib as dx
from test_gpu_engine import _check_frame_scalars

from tools import dab_synth as ds

pytestmark = pytest.mark.gpu


def _batched(fn, rows, sizes_and_turns):
    """fn on the rows all at once, in batches of 3 and one by one, the row order turned by another amount each time (a block that read its
    neighbour's row would answer for the wrong case) -> one result per (batch size), each back in the rows' own order"""
    n = len(rows)
    out = []
    for size, turn in sizes_and_turns:
        order = np.roll(np.arange(n), turn)
        got = np.zeros(n, np.int64)
        step = n if size is None else size
        for lo in range(0, n, step):
            idx = order[lo:lo + step]
            got[idx] = fn(rows[idx])
        out.append(got)
    return out


@pytest.fixture(scope="module")
def windows():
    w = sc.correlator_windows()
    L = ol.oracle()
    want = {}
    for thr in sc.THRESHOLDS:
        for strongest in (0, 1):
            pr = L.ora_phaseref_new()
            L.ora_phaseref_set_strongest(pr, strongest)
            want[thr, strongest] = np.array([L.ora_phaseref_correlate(pr, v.x, thr) for v in w], np.int64)
            L.ora_phaseref_free(pr)
    return w, np.array([v.x for v in w]), want


@pytest.mark.parametrize("strongest", [0, 1])
@pytest.mark.parametrize("thr", sc.THRESHOLDS)
def test_correlator_start_index_equals_the_oracle(windows, thr, strongest):
    w, rows, want = windows
    exp = want[thr, strongest]
    for (size, turn), got in zip(((None, 0), (None, 11), (3, 5), (1, 17)),
                                 _batched(lambda r: dx.prs_correlate(r, thr, bool(strongest)), rows, ((None, 0), (None, 11), (3, 5), (1, 17)))):
        bad = [(w[i].name, int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]
        print("\nthr %g strongest %d batch %s turn %d: %d of %d differ %s" % (thr, strongest, size, turn, len(bad), len(w), bad))
        assert not bad, (thr, strongest, size, turn, bad)


@pytest.fixture(scope="module")
def spectra():
    sp = sc.coarse_spectra()
    L = ol.oracle()
    pr = L.ora_phaseref_new()
    want = np.array([L.ora_phaseref_coarse_cfo(pr, s.X) for s in sp], np.int64)
    L.ora_phaseref_free(pr)
    models = [sc.model_coarse(s.X) for s in sp]
    return sp, np.array([s.X for s in sp]), want, models


def test_coarse_cfo_equals_the_oracle(spectra):
    """equal where offset * 1000 is at least 4 D from an integer (and on every not-found and non-finite case: sign and size exact); +-1 Hz on
    the rest, at most a tenth of the cases"""
    sp, rows, want, models = spectra
    exact = np.array([sc.coarse_class(m) == "exact" for m in models])
    assert all(sc.coarse_class(m) in ("exact", "pm1") for m in models) and 10 * int((~exact).sum()) <= len(sp)
    special = (want == sc.IDX_NOT_FOUND) | (want == sc.INT_MIN) | np.array([not np.isfinite(m["hz1000"]) for m in models])
    assert exact[special].all() and special.sum() >= 10
    for (size, turn), got in zip(((None, 0), (None, 50), (3, 7), (1, 23)), _batched(dx.coarse_cfo, rows, ((None, 0), (None, 50), (3, 7), (1, 23)))):
        d = np.abs(got - want)
        bad = [(sp[i].name, int(got[i]), int(want[i])) for i in np.nonzero(np.where(exact, d > 0, d > 1))[0]]
        print("\nbatch %s turn %d: %d of %d differ from the oracle (%d within 1 Hz where that is allowed) %s"
              % (size, turn, len(bad), len(sp), int(((d > 0) & ~exact).sum()), bad))
        assert not bad, (size, turn, bad)


def test_engine_on_a_stream_whose_coarse_estimate_is_not_finite():
    """One cf32 engine, two streams of the same eight frames (+1234.5 Hz, 30 dB): at scale 1, and at 1e6, where the magnitudes of the coarse
    search overflow -- the reference takes INT_MIN (or -70 000: an inf between finite neighbours) as found, f_sync goes back to 0 and
    clock_err to 0 in every frame, no FIB passes.  Per frame: f_bb, clock_err, the FIC ratio and SNR (_check_frame_scalars), start_index,
    the CRC flags, what the coarse search returned; f_sync after the last frame."""
    ens = ds.build_ensemble(5, seed=61, cyclic=True)
    x = ds.channel(ens.iq, snr_db=30.0, cfo_hz=1234.5, seed=61, n_out=8 * ds.TF)
    xs = [x, (x.astype(np.complex128) * 1e6).astype(np.complex64)]
    oras = [ol.oracle_run(v, [], trace=4096) for v in xs]
    corr = [o["trace"]["ratio"][o["trace"]["kind"] == ol.EV_FRAME_DONE].astype(np.float64) for o in oras]
    assert oras[0]["n"] == oras[1]["n"] == 6 and oras[0]["crc"][2:].all() and not oras[1]["crc"].any()
    assert set(corr[1]) == {float(sc.INT_MIN), -70000.0} and (oras[1]["fbb"] == 0).all()

    class Rec:
        def __init__(self):
            self.scalars = dict(clock_err=[], fic_ratio=[], snr_db=[], mer_db=[])
            self.fbbs, self.start, self.crc, self.front = [], [], [], []

    eng = dx.Engine(n_streams=2, ring_frames=9, max_subch=0, fic_only=True, out_frames=4)
    try:
        for s in range(2):
            eng.push_iq(s, xs[s])
        rec = [Rec(), Rec()]
        for _ in range(12):
            eng.process(1)
            for s in range(2):
                st = eng.stats(s)
                if st["frames"] > len(rec[s].start):
                    assert st["frames"] == len(rec[s].start) + 1
                    rec[s].front.append(dx.front_read(eng, s, spectra=False))
                    _f, c = eng.read_fibs(s, 1)
                    rec[s].crc.append(c[0]); rec[s].start.append(st["last_start_index"]); rec[s].fbbs.append(st["freq_offs_bb_hz"])
                    rec[s].scalars["clock_err"].append(st["clock_err_hz"]); rec[s].scalars["fic_ratio"].append(st["fic_ratio_percent"])
                    rec[s].scalars["snr_db"].append(st["snr_db_est"]); rec[s].scalars["mer_db"].append(st["mer_db_est"])
        for s in range(2):
            n, fr = oras[s]["n"], rec[s].front
            got_corr = [f["correction"] for f in fr]
            print("\nstream %d: start %s f_bb %s correction %s f_sync %s" % (s, rec[s].start, rec[s].fbbs, got_corr, [float(f["f_sync"]) for f in fr]))
            assert len(rec[s].start) >= n
            assert rec[s].start[:n] == oras[s]["start"].tolist() and [f["start_index"] for f in fr[:n]] == oras[s]["start"].tolist()
            assert np.array_equal(np.array(rec[s].crc[:n]), oras[s]["crc"])
            _check_frame_scalars(rec[s], rec[s].fbbs, oras[s], n)
            # what the coarse search returned: exact where it is not finite (stream 1) and in the last frame; a finite estimate on its way to
            # the carrier is the truncation of a float product (+-1 Hz, as tests/test_gpu_stages.py allows; f_bb above holds it to 0.05 Hz)
            d = np.abs(np.array(got_corr[:n], np.float64) - corr[s][:n])
            assert d.max() <= (1 if s == 0 else 0) and d[n - 1] == 0, (s, got_corr, corr[s])
            last = fr[n - 1]
            assert max(abs(float(last[k]) - float(oras[s]["fbb_end"][n - 1])) for k in ("f_sync", "f_bb")) <= 0.05
            assert np.array_equal(np.array([f["clock_err"] for f in fr[:n]], np.float32), oras[s]["clock_err"])
    finally:
        eng.close()
