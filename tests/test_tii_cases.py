"""The inputs of the device TII tests (tests/tii_cases.py) qualify: on the CPU alone, the float64 model takes the decisions the host detector
(dx.Tii, pinned to the reference's object code by tests/test_tii.py) takes, every scenario reaches the branch it is named for, and no
decision of any round lies closer than 1e-5 (relative) to going the other way -- far beyond what the last bits of |z| can move, so a device
detector that keeps the host's order of arithmetic must give the same ids, sub-ids, flags and order."""
import numpy as np
import pytest

import test_tii
import tii_cases as tc

SC = tc.all_scenarios()


@pytest.fixture(scope="module")
def runs():
    return {name: (test_tii.run_dabx(c, s, thr, rounds), tc.run_model(c, s, thr, rounds)) for name, (c, s, thr, rounds) in SC.items()}


def test_the_eight_pinned_scenarios_are_all_here():
    assert set(test_tii.scenarios()) <= set(SC) and len(SC) == len(test_tii.scenarios()) + len(tc.new_scenarios()) and set(SC) == set(tc.BRANCH)


@pytest.mark.parametrize("name", sorted(SC))
def test_the_model_decides_as_the_host_detector(name, runs):
    host, model = runs[name]
    assert len(host) == len(model) == len(SC[name][3])
    for ri, (h, (m, _, _)) in enumerate(zip(host, model)):
        assert [(r[0], r[1], r[4]) for r in h] == [(r[0], r[1], r[4]) for r in m], (name, ri)
        for a, b in zip(h, m):                               # float32 against float64: the same numbers
            assert abs(a[2] - b[2]) <= 2e-6 * b[2] and abs((a[3] - b[3] + 180) % 360 - 180) <= 2e-4, (name, ri, a, b)


@pytest.mark.parametrize("name", sorted(SC))
def test_every_scenario_reaches_its_branch(name, runs):
    taken = set().union(*[t for _, _, t in runs[name][1]])
    assert tc.BRANCH[name] in taken, (name, sorted(taken))
    if name == "crowded":
        assert all(len(m) > 32 for m, _, _ in runs[name][1])
    if name == "state_carries":
        # round 2 has no transmitter in its input and still reports the one of round 1: the state did carry
        assert len(SC[name][3]) >= 3 and [(r[0], r[1]) for r in runs[name][0][1]] == [(30, 4)]
    if name in ("huge_1e11", "tiny_1e-11"):
        # ... and a float sqrtf(x * x + y * y) would indeed have left the range: the products' squares overflow / flush to zero
        sums = tc.round_sums(SC[name][3])
        p = np.abs(sums[0][tc.BIN].astype(np.complex128) * np.conj(sums[0][tc.BIN + 1].astype(np.complex128))) * 0.01
        sq = p.max() ** 2
        assert sq > float(np.finfo(np.float32).max) if name == "huge_1e11" else sq < float(np.finfo(np.float32).tiny) * 2.0 ** -23


@pytest.mark.parametrize("name", sorted(SC))
def test_every_rounds_smallest_margin_is_at_least_1e_5(name, runs):
    for ri, (_, margin, _) in enumerate(runs[name][1]):
        assert margin >= tc.MIN_MARGIN, (name, ri, margin)
