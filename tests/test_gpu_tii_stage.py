"""dabx_tii_process_device: the device's TII detector (csrc/tii_core.h, one 256-thread block per detector, the device function of the
engine's k_tii) against the host detector dx.Tii, which tests/test_tii.py pins to the reference's object code -- round by round, the state
(pairs) carried by the caller.  Every detector of a call runs another scenario or another round of one, so a block that touched a
neighbour's sum, state or output would be caught; tests/test_tii_cases.py shows on the CPU that no decision of these inputs lies within
1e-5 of going the other way, so ids, sub-ids, flags, order and both counts must be EXACT; strength and phase differ from the host's by what
|z| and atan2f differ from libm's."""
import ctypes as C

import numpy as np
import pytest

import test_tii
import tii_cases as tc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu

# Measured on an MI355X over all 15 scenarios and all their rounds, and over the events of tests/test_gpu_tii_delivery.py
# (docs/history/tii_device.md): every strength was bit for bit the host's (largest relative deviation 0) and the largest phase deviation was
# 1.53e-5 degrees, an ulp of a float near 180.  The bounds are four times the maxima rounded up to one significant digit -- for the strength
# that is 0: equality --, under a ceiling of 2e-6 relative and 2e-4 degrees (about 30 chained float operations at half an ulp each).
REL_TOL = 0.0
DEG_TOL = 7e-5
assert REL_TOL <= 2e-6 and DEG_TOL <= 2e-4
SC = tc.all_scenarios()
NAMES = sorted(SC)
SHIFT = {1: NAMES.index("crowded"), 3: NAMES.index("collision_list_six"), 65: 0}
WORST = {"rel": 0.0, "deg": 0.0}
E_ARG = -2                                # DABX_E_ARG


@pytest.fixture(scope="module")
def host():
    """name -> (per round the host detector's results (up to 64), per round the float32 sum it was handed)"""
    return {name: (test_tii.run_dabx(c, s, thr, rounds), tc.round_sums(rounds)) for name, (c, s, thr, rounds) in SC.items()}


def compare(res, n_res, n_found, want, where):
    assert n_found == len(want) and n_res == min(len(want), dx.TII_MAX_RESULTS), (where, n_res, n_found, len(want))
    got = dx._tii_tuples(res[:n_res])
    assert [(g[0], g[1], g[4]) for g in got] == [(w[0], w[1], w[4]) for w in want[:n_res]], where
    for g, w in zip(got, want):
        rel = abs(np.float32(g[2]) - np.float32(w[2])) / abs(w[2])
        deg = abs((float(np.float32(g[3])) - float(np.float32(w[3])) + 180.0) % 360.0 - 180.0)
        WORST["rel"], WORST["deg"] = max(WORST["rel"], float(rel)), max(WORST["deg"], deg)
        assert rel <= REL_TOL and deg <= DEG_TOL, (where, g, w, rel, deg)


@pytest.mark.parametrize("n", [1, 3, 65])
def test_n_detectors_in_one_call_follow_the_host_detector_round_by_round(n, host):
    # detector d: scenario NAMES[(d + shift) % 15], started d // 15 calls late; while it has no round to run its enable is 0
    plan = [(NAMES[(d + SHIFT[n]) % len(NAMES)], d // len(NAMES)) for d in range(n)]
    calls = max(delay + len(SC[name][3]) for name, delay in plan)
    pairs = np.zeros((n, 768), np.complex64)
    sentinel = np.zeros((n, dx.TII_MAX_RESULTS), dx.TII_RESULT)
    sentinel["main_id"], sentinel["strength"] = 0xEE, -7.0
    for k in range(calls):
        sums = np.zeros((n, 2048), np.complex64)
        cfgs, live = [], []
        for d, (name, delay) in enumerate(plan):
            c, s, thr, rounds = SC[name]
            r = k - delay
            live.append(0 <= r < len(rounds))
            if live[-1]:
                sums[d] = host[name][1][r]
            cfgs.append(dict(enable=int(live[-1]), threshold_db=thr, collisions=c, collision_sub_id=s))
        before = pairs.copy()
        pairs, res, nr, nf = dx.tii_process_device(sums, pairs, cfgs, out=sentinel, n_results=np.full(n, -5, np.int32), n_found=np.full(n, -6, np.int32))
        for d, (name, delay) in enumerate(plan):
            if live[d]:
                compare(res[d], int(nr[d]), int(nf[d]), host[name][0][k - delay], (n, d, name, k - delay))
            else:                                            # enable = 0: the state and every output row are the caller's
                assert np.array_equal(pairs[d].view(np.uint32), before[d].view(np.uint32)) and nr[d] == -5 and nf[d] == -6, (n, d, k)
                assert np.array_equal(res[d], sentinel[d]), (n, d, k)
    print("n = %d: largest deviation so far %.3g relative, %.3g degrees" % (n, WORST["rel"], WORST["deg"]))


def test_zero_sums_decay_the_state_by_the_iirs_step_bit_for_bit():
    """p + 0.01f * (0 - p) per round, which is p scaled by 0.99 up to the step's own two roundings: in float32, in the host's order"""
    rng = np.random.default_rng(5)
    n = 3
    p0 = ((rng.standard_normal((n, 768)) + 1j * rng.standard_normal((n, 768))) * np.array([[1e-3], [1.0], [1e20]])).astype(np.complex64)
    pairs, want = p0.copy(), p0.copy().view(np.float32)
    cfgs = [dict(threshold_db=8)] * n
    for _ in range(3):
        pairs, res, nr, nf = dx.tii_process_device(np.zeros((n, 2048), np.complex64), pairs, cfgs)
        want = want + np.float32(0.01) * (np.float32(0) - want)
        assert want.dtype == np.float32 and np.array_equal(pairs.view(np.uint32), want.view(np.uint32))
    assert np.allclose(pairs, p0 * 0.99 ** 3, rtol=1e-6, atol=0)


def test_bad_arguments_are_refused():
    L = dx.load()
    L.dabx_tii_process_device.argtypes = [C.c_int] + [C.c_void_p] * 6
    sums, pairs = np.zeros((1, 2048), np.complex64), np.zeros((1, 768), np.complex64)
    cfg, out = (dx.TiiConfig * 1)(dx.TiiConfig(enable=1)), np.zeros((1, 32), dx.TII_RESULT)
    nr, nf = np.zeros(1, np.int32), np.zeros(1, np.int32)
    good = [dx._p(sums), dx._p(pairs), C.cast(cfg, C.c_void_p), dx._p(out), dx._p(nr), dx._p(nf)]
    assert L.dabx_tii_process_device(1, *good) == 0
    for n in (0, -1):
        assert L.dabx_tii_process_device(n, *good) == E_ARG
    for i in range(6):
        assert L.dabx_tii_process_device(1, *[None if j == i else a for j, a in enumerate(good)]) == E_ARG, i
