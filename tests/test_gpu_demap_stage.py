"""The engine's demapper (demap_frame_body in every instance the engine launches: 3 soft-bit generators x 2 symbol conversions x MER on /
off x k_demap_frame6 / k_demap_fic / k_demap_whole) on crafted spectra, against oracle/ofdm.c.

The spectra go straight to where the front end leaves them (dx.demap_inject / dx.demap_frame: the library's internal test entries, no IQ,
no FFT), so the demapper sees exact zeros, drop-outs, gains of 1e5 and 1e-5, products beyond int16 and beyond 2^31.  Two layers:
  float    the captured soft bits against the oracle's under the rule of tests/demap_cases.py (relative for large products, exactly 0 where
           x86's conversion gives the "integer indefinite"), SNR and MER within the stage test's 0.02 dB;
  integer  FIBs, CRC verdicts and MSC bytes equal oracle/fic.c and the oracle back end fed the device's OWN captured soft bits under the
           same tie mode -- the symbol conversion, the LDS tile, the FIC dword path and the ring addresses, free of any float tolerance.
tests/test_demap_cases.py proves without a device that the cases reach what they are named for."""
import os
import subprocess
import sys

import numpy as np
import pytest

import demap_cases as dc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# the 12 dispatch rows of DABX_DEMAP_DISPATCH: (generator, viterbi_tie_mode, LCD statistics); tie mode 0 = the wrapping conversion, 1 and 2 = SAT
ROWS = [(g, m, mer) for g in dc.GENERATORS for m in (0, 1 + g % 2) for mer in (0, 1)]
S = dc.N_STREAMS


def _engine(gen, mode, mer):
    eng = dx.Engine(n_streams=S, ring_frames=2, max_subch=len(dc.SUBCH), out_frames=2, capture_soft=True, soft_bit_type=gen, viterbi_tie_mode=mode)
    eng.set_subchannels(dc.SUBCH, dab_plus=False)
    eng.set_lcd_statistics(mer)
    return eng


def _run(gen, mode, mer, schedule, float_layer=True):
    """All steps of the plan on one engine.  Returns per stream (captures [n, 75, 3072], FIBs [n, 12, 32], CRC verdicts [n, 12],
    {slot: logical frames}) and the float layer's failures."""
    exp = [dc.oracle_stream(s, gen) for s in range(S)]
    frames = [dc.stream_frames(s) for s in range(S)]
    cap, fibs, crcs = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    msc = [{j: [] for j in range(len(dc.SUBCH))} for _ in range(S)]
    seen = [[0] * len(dc.SUBCH) for _ in range(S)]
    bad, fig = [], []
    eng = _engine(gen, mode, mer)
    try:
        at = [0] * S
        for step in range(dc.N_STEPS):
            present = [0] * S
            for s in range(S):
                fr = frames[s][step] if step < len(frames[s]) else None
                if fr is None:
                    continue
                present[s] = fr["present"]
                if fr["present"]:
                    dx.demap_inject(eng, s, fr["spec"], fr["null_fft"], fr["ce"], fr["np_sel"])
                else:
                    # an absent stream gets spectra all the same (turned by 90 degrees and doubled): demapping them would show everywhere
                    dx.demap_inject(eng, s, fr["spec"] * np.complex64(2j), None, frames[s][step - 1]["ce"], frames[s][step - 1]["np_sel"])
            before = {s: (eng.read_soft(s), eng.stats(s)) for s in range(S) if not present[s]}
            dx.demap_frame(eng, present, schedule)
            for s in range(S):
                st = eng.stats(s)
                if not present[s]:
                    assert np.array_equal(eng.read_soft(s), before[s][0]) and repr(st) == repr(before[s][1]), (step, s)   # (repr: NaN statistics of a dead stream)
                    continue
                r = exp[s][at[s]]
                got = eng.read_soft(s)
                cap[s].append(got)
                if float_layer and (r["name"], gen) not in dc.UNDEFINED:
                    c = dc.compare(got, r["soft"], r["prod"])
                    fig.append((c["worst"], c["frac_soft_bad"], c["frac_left_out"], c["n_zero"], r["name"]))
                    if not c["ok"]:
                        bad.append((r["name"], c))
                    if np.isfinite(r["snr_db"]) and abs(st["snr_db_est"] - r["snr_db"]) > 0.02:
                        bad.append((r["name"], "snr_db", st["snr_db_est"], r["snr_db"]))
                    if mer and np.isfinite(r["mer_db"]) and abs(st["mer_db_est"] - r["mer_db"]) > 0.02:
                        bad.append((r["name"], "mer_db", st["mer_db_est"], r["mer_db"]))
                    if not mer and st["mer_db_est"] != 0.0:
                        bad.append((r["name"], "mer_db without LCD statistics", st["mer_db_est"]))
                at[s] += 1
            dx.fic_decode_frame(eng, present)
            dx.msc_decode(eng, [4 * p for p in present], 4)
            for s in range(S):
                if not present[s]:
                    continue
                f, c = eng.read_fibs(s, 1)
                fibs[s].append(f[0]); crcs[s].append(c[0])
                for j in range(len(dc.SUBCH)):
                    n = eng.subch_stats(s, j)["cifs_decoded"]
                    if n > seen[s][j]:
                        new = eng.read_msc(s, j, n - seen[s][j])
                        assert new.shape[0] == n - seen[s][j], (step, s, j)
                        msc[s][j].extend(new)
                        seen[s][j] = n
        assert at == [len(e) for e in exp]
        if fig:                                                  # the figures, before anything is asserted on them
            print("gen %d tie %d mer %d schedule %d: largest |d| - REL |x| = %.2f (%s), largest share beyond 1 + REL |x| = %.2e (%s), most left out %.4f, "
                  "%d products that must give 0" % (gen, mode, mer, schedule, max(fig)[0], max(fig)[4], max(f[1] for f in fig),
                                                     max(fig, key=lambda f: f[1])[4], max(f[2] for f in fig), sum(f[3] for f in fig)))
    finally:
        eng.close()
    return [(np.stack(cap[s]), np.stack(fibs[s]), np.stack(crcs[s]), {j: np.array(v) for j, v in msc[s].items()}) for s in range(S)], bad


def _check_integer_layer(out, mode):
    """FIBs, CRC verdicts and MSC bytes of every stream against the oracle back ends fed the device's own captures."""
    good_crc = 0
    for s, (cap, fibs, crcs, msc) in enumerate(out):
        want = dc.fic_of(cap, mode)
        assert len(want) == fibs.shape[0]
        for f, (wf, wc) in enumerate(want):
            assert np.array_equal(fibs[f], wf) and np.array_equal(crcs[f], wc), (s, f)
        good_crc += int(crcs.sum())
        for j, frames in enumerate(dc.msc_of(cap, mode)):
            assert frames.shape[0] == 4 * cap.shape[0] - 16 and frames.shape[0] >= 4, (s, j)
            assert msc[j].shape == frames.shape and np.array_equal(msc[j], frames), (s, j)
    return good_crc


@pytest.mark.parametrize("schedule", [0, 1, 2], ids=["frame6", "fic_then_frame6", "whole"])
@pytest.mark.parametrize("row", ROWS, ids=["gen%d_tie%d_mer%d" % r for r in ROWS])
def test_engine_demapper_equals_the_oracle_frame_by_frame(row, schedule):
    """One engine per dispatch row and schedule, six streams, every step of the plan.  After every frame: the float layer per stream (and a
    stream without a frame keeps its capture and its statistics); at the end the integer layer, overflow frames included."""
    gen, mode, mer = row
    out, bad = _run(gen, mode, mer, schedule)
    try:
        good, integer_layer = _check_integer_layer(out, mode), None
    except AssertionError as ex:
        good, integer_layer = 0, str(ex)[:300]
    assert not bad and integer_layer is None, (len(bad), bad[:6], integer_layer)
    assert good >= 12 * 8                                    # the FIC of the undisturbed frames decodes: the CRC verdicts are not all "bad"


def test_the_three_schedules_give_the_same_bytes():
    """One input (generator 2, tie mode 0, LCD statistics on), the three schedules: byte-identical captures, FIBs, CRC verdicts, MSC bytes."""
    outs = [_run(2, 0, 1, schedule, float_layer=False)[0] for schedule in (0, 1, 2)]
    for other in outs[1:]:
        for s in range(S):
            a, b = outs[0][s], other[s]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), s
            assert all(np.array_equal(a[3][j], b[3][j]) for j in a[3]), s


def test_an_absent_stream_keeps_its_fic_symbols_and_goes_on_as_if_nothing_had_been():
    """Stream 5 has no frame in step 1: its capture and statistics stay (checked in every run above) and its later frames are those of an
    oracle that never saw the step (the float layer of the runs above).  Here its FIC symbols: after the absent demapper step -- other
    spectra injected, every schedule -- the FIC decoder is run on the stored symbols AGAIN (present = 1), and must decode the FIBs and CRC
    verdicts of frame 0 once more; a demapper that had touched fic_sym would decode the turned spectra."""
    frames = dc.stream_frames(5)
    for schedule in (0, 1, 2):
        eng = _engine(1, 1, 0)
        try:
            present = [0] * S
            present[5] = 1
            dx.demap_inject(eng, 5, frames[0]["spec"], frames[0]["null_fft"], frames[0]["ce"], frames[0]["np_sel"])
            dx.demap_frame(eng, present, schedule)
            dx.fic_decode_frame(eng, present)
            f0, c0 = eng.read_fibs(5, 1)
            assert f0.shape[0] == 1 and c0.sum() == 12                      # a clean frame: twelve good FIBs
            dx.demap_inject(eng, 5, frames[1]["spec"] * np.complex64(2j), None, frames[0]["ce"], frames[0]["np_sel"])
            dx.demap_frame(eng, [0] * S, schedule)
            dx.fic_decode_frame(eng, present)                               # decodes whatever fic_sym holds now
            f1, c1 = eng.read_fibs(5, 1)
            assert eng.stats(5)["frames"] == 2
            assert np.array_equal(f0, f1) and np.array_equal(c0, c1), schedule
            # ... and the same entry does see new symbols when the stream has a frame
            dx.demap_frame(eng, present, schedule)
            dx.fic_decode_frame(eng, present)
            f2, c2 = eng.read_fibs(5, 1)
            assert not np.array_equal(f0, f2) or not np.array_equal(c0, c2), schedule
        finally:
            eng.close()


def test_the_test_entries_refuse_what_they_cannot_do():
    eng = dx.Engine(n_streams=2, max_subch=0, fic_only=True, out_frames=2, ring_frames=2, capture_soft=True)
    try:
        L = dx.load()
        L.dabx_internal_demap_inject.argtypes = [dx.C.c_void_p, dx.C.c_int, dx.C.c_void_p, dx.C.c_void_p, dx.C.c_float, dx.C.c_int]
        spec = np.zeros((76, 2048), np.complex64)
        E_ARG = -2                                                          # DABX_E_ARG (include/dabx.h)
        for stream, np_sel in ((-1, 0), (2, 0), (0, 2), (0, -1)):
            assert L.dabx_internal_demap_inject(eng._h, stream, dx._p(spec), None, 0.0, np_sel) == E_ARG
        assert L.dabx_internal_demap_inject(eng._h, 0, None, None, 0.0, 0) == E_ARG
        one = np.array([1, 0], np.int32)
        assert L.dabx_internal_demap_frame(eng._h, None, 0) == E_ARG
        for schedule in (-1, 3):
            assert L.dabx_internal_demap_frame(eng._h, dx._p(one), schedule) == E_ARG
        for present in ([2, 0], [0, -1]):
            assert L.dabx_internal_demap_frame(eng._h, dx._p(np.array(present, np.int32)), 0) == E_ARG
        with pytest.raises(ValueError):
            dx.demap_frame(eng, [1], 0)
        with pytest.raises(ValueError):
            dx.demap_inject(eng, 0, spec[:75])
        dx.demap_frame(eng, [0, 0], 2)                                     # nobody has a frame: nothing moves
        assert eng.stats(0)["frames"] == 0 and not eng.read_soft(0).any()
    finally:
        eng.close()


def test_the_entries_work_in_the_hipmodule_form():
    """One row and schedule of the engine test, and the refusals, with the binding pointed at hipmodule/libdabx.so: k_demap_inject and the
    demapper instances are found in the code objects and launched through hipModuleLaunchKernel."""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_demap_stage.py", "-k", "gen3_tie0_mer1-fic_then_frame6 or refuse"], cwd=ROOT, env=hipmodule_env(), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
