"""The row function of the CIR stage on the device (csrc/cir_core.h cir_row_block, the body of k_cir; include/dabx.h dabx_cir_rows_device)
on the crafted rows of tests/cir_cases.py against the float64 model of cir_viewer.cpp:66-95: the phase reference in time at delays 0, 1,
511, 512, 2047, two and three taps of unequal weight, a tap plus noise, and the rows whose value is exact -- zeros, a NaN sample and a
scale at which every square is zero give exactly 0, a scale at which the peak's square overflows gives inf.  Batches of 1, 3 and all
rows, in turned orders: a row's value does not depend on its place in the launch.  A few dozen rows in all."""
import ctypes

import numpy as np
import pytest

import cir_cases as cc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu


def run_rows(xs):
    L = dx.load()
    L.dabx_cir_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    iq = np.ascontiguousarray(np.stack(xs).astype(np.complex64))
    y = np.full(len(xs), -7.0, np.float32)
    dx.check(L.dabx_cir_rows_device(dx._p(iq), len(xs), dx._p(y)))
    return y


@pytest.fixture(scope="module")
def world():
    """The rows, their expectations and the device's answer to all of them in one launch: computed once, shared, left unchanged."""
    rows = cc.rows()
    want = [cc.row_expectation(name, x) for name, x, _ in rows]
    return rows, want, run_rows([x for _, x, _ in rows])


def check(name, want, got):
    kind, v = want
    print("%-22s model %-14.8g device %-14.8g %s" % (name, v, got, "" if kind == "exact" else "rel %.2e" % (abs(got - v) / v)))
    if kind == "exact":
        assert got == np.float32(v), (name, got, v)
    else:
        assert abs(float(got) - v) <= cc.BAR * v, (name, got, v)          # one value per row: the row's largest model value is the value


def test_every_row_against_the_model(world):
    rows, want, got = world
    print()
    assert len(rows) == 15
    for (name, _, _), w, g in zip(rows, want, got):
        check(name, w, g)
    # the unit tap: sqrt(1536) * 2048 / 26000, wherever it lies
    for k in range(5):
        assert abs(float(got[k]) - np.sqrt(1536.0) * 2048 / 26000) <= cc.BAR * 3.1


def test_batches_of_1_and_3_and_turned_orders_give_the_same_floats(world):
    rows, want, got = world
    xs = [x for _, x, _ in rows]
    n = len(xs)
    for k in (0, 7, n - 1):                                                # alone
        assert run_rows([xs[k]])[0].tobytes() == got[k].tobytes(), rows[k][0]
    for trio in ((0, 10, 5), (12, 11, 13)):                                # three, the exact rows among finite ones
        y = run_rows([xs[k] for k in trio])
        assert y.tobytes() == got[list(trio)].tobytes(), trio
    for order in (list(range(n))[::-1], list(range(3, n)) + [0, 1, 2]):    # all, turned
        y = run_rows([xs[k] for k in order])
        assert y.tobytes() == got[order].tobytes()


def test_bad_arguments_are_refused():
    L = dx.load()
    L.dabx_cir_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    y = np.zeros(1, np.float32)
    x = np.zeros(cc.TU, np.complex64)
    assert L.dabx_cir_rows_device(None, 1, dx._p(y)) == -2 and L.dabx_cir_rows_device(dx._p(x), 0, dx._p(y)) == -2
    assert L.dabx_cir_rows_device(dx._p(x), 1, None) == -2
