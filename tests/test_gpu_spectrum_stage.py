"""The row function of the spectrum stage (csrc/spectrum_core.h spectrum_row_block, the function k_spectrum runs) on crafted windows,
through dabx_spectrum_rows_device: 15 windows and a sequence of 6 (tests/spectrum_cases.py) against the float64 model of
SpectrumViewer::show_spectrum (spectrum_viewer.cpp:169-218) under the comparison rule -- linear values within 2e-5 of the window's
largest model value, dB values within the per-bin bound that goes through the 0.2 recurrence, extrema within the show's largest bound --,
the exact cases bit for bit, and the same floats whatever the batch (1, 3, all) and the order."""
import numpy as np
import pytest

import spectrum_cases as sp
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    """The windows, the models and the device's answers: computed once, shared, left unchanged."""
    ws = sp.windows()
    singles = [dx.spectrum_rows_device(x[None, :]) for _, x, _ in ws]
    models = [sp.Row64().show(x) for _, x, _ in ws]
    return ws, singles, models


def test_every_window_against_the_model(world):
    ws, singles, models = world
    print()
    worst = 0.0
    for (name, x, why), (lin, db, ext, st), (y, v, d, mext, b, bd) in zip(ws, singles, models):
        lin, db, ext = lin[0], db[0], ext[0]
        assert np.array_equal(st[:sp.BINS].view(np.uint32), db.view(np.uint32)) and np.array_equal(st[sp.BINS:].view(np.uint32), ext.view(np.uint32))
        if name in sp.EXACT_NAN:
            assert np.isnan(db).all() and np.isnan(lin).all(), name                    # disp NaN in every bin ...
            assert ext.tolist() == [-1000.0, 1000.0, -1000.0, 1000.0], name            # ... and the extrema untouched
            continue
        if name == "zeros":
            assert (lin == 0).all()
            want = np.float32(np.float32(0.2) * np.float32(sp.VAL_OF_ZERO))            # disp = 0 + 0.2f (val - 0)
            print("zeros: val = disp / 0.2f, device bits %08x, the transcription's %08x" % (int(db.view(np.uint32)[0]), int(want.view(np.uint32))))
            assert (db.view(np.uint32) == want.view(np.uint32)).all()
            assert ext.view(np.uint32).tolist() == [int(want.view(np.uint32))] * 4
            continue
        rel = float(np.abs(lin.astype(np.float64) - y).max() / y.max())
        err = float((np.abs(db.astype(np.float64) - d) / bd).max())
        worst = max(worst, rel)
        print("%-18s lin rel %.2e  dB error / bound %.3f" % (name, rel, err))
        assert rel <= sp.BAR, (name, rel)
        assert err <= 1.0, (name, err)
        assert (np.abs(ext.astype(np.float64) - np.array(mext)) <= bd.max()).all(), (name, ext, mext)
        # the half swap, by position: the largest display bin is where the model has it
        assert int(np.argmax(lin)) == int(np.argmax(y)), name
    print("largest deviation of the linear values: %.2e of the window's largest (bar %.0e)" % (worst, sp.BAR))
    names = [w[0] for w in ws]
    assert int(np.argmax(singles[names.index("tone_1023")][0][0])) == 511 and int(np.argmax(singles[names.index("tone_1024")][0][0])) == 0
    assert int(np.argmax(singles[names.index("tone_0")][0][0])) == 256 and int(np.argmax(singles[names.index("dc_only")][0][0])) == 256
    assert int(np.argmax(singles[names.index("tone_bin_centre")][0][0])) == 256 + 100


def test_batches_and_orders_give_the_same_floats(world):
    ws, singles, _ = world
    xs = np.stack([x for _, x, _ in ws])                                               # (the NaN windows are the last two)
    lin_all, db_all, ext_all, st_all = dx.spectrum_rows_device(xs)
    for k in range(len(ws)):                                                           # the linear values do not depend on the state
        assert lin_all[k].tobytes() == singles[k][0][0].tobytes(), ws[k][0]
    for batch in (1, 3):
        st, lins, dbs, exts = None, [], [], []
        for k in range(0, len(ws), batch):
            lin, db, ext, st = dx.spectrum_rows_device(xs[k:k + batch], st)
            lins.append(lin), dbs.append(db), exts.append(ext)
        assert np.concatenate(lins).tobytes() == lin_all.tobytes() and np.concatenate(dbs).tobytes() == db_all.tobytes()
        assert np.concatenate(exts).tobytes() == ext_all.tobytes() and st.tobytes() == st_all.tobytes()
    order = list(range(len(ws) - 2))[::-1] + [len(ws) - 2, len(ws) - 1]                # turned round, the NaN windows still last
    lin_r, db_r, _, _ = dx.spectrum_rows_device(xs[order])
    for pos, k in enumerate(order):
        assert lin_r[pos].tobytes() == lin_all[k].tobytes(), ws[k][0]
    assert not np.isnan(db_all[len(ws) - 3]).any() and np.isnan(db_all[len(ws) - 2:]).all()   # a NaN stays
    assert db_r[0].tobytes() == singles[order[0]][1][0].tobytes()


def test_the_sequence_walks_the_iir(world):
    seq = sp.sequence()
    lin, db, ext, st = dx.spectrum_rows_device(np.stack(seq))
    m = sp.Row64()
    lim_dev, lim_mod, bl = np.array(sp.LIMITS0, np.float32), list(sp.LIMITS0), 0.0
    for k, x in enumerate(seq):
        y, v, d, mext, b, bd = m.show(x)
        assert float(np.abs(lin[k].astype(np.float64) - y).max() / y.max()) <= sp.BAR, k
        assert (np.abs(db[k].astype(np.float64) - d) <= bd).all(), k
        assert (np.abs(ext[k].astype(np.float64) - np.array(mext)) <= bd.max()).all(), k
        # the limits, from the device's extrema through the library's own function, against the model's through the transcription
        lim_dev, y_dev, valid = dx.spectrum_limits(ext[k], lim_dev, "medium", 30)
        lim_mod, y_min, y_max, want_valid, _ = sp.limits32(mext, lim_mod, sp.ALPHA["medium"], 30)
        bl = 0.9 * bl + 0.1 * bd.max()                                                 # (the slacks: spectrum_cases.py, the float32 operations themselves)
        assert valid == want_valid and (np.abs(lim_dev.astype(np.float64) - np.array(lim_mod, np.float64)) <= bl + sp.LIMIT_SLACK).all(), k
        assert abs(y_dev[0] - y_min) <= bl + sp.Y_SLACK and abs(y_dev[1] - y_max) <= bl + sp.Y_SLACK
    assert np.abs(d).max() > 10.0
