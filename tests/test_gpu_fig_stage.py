"""dabx_fig_walk_device: the device's FIG walk (csrc/fig_core.h, one wave per decoder, the device function of the engine's k_fig) on the
crafted FIB sequences of tests/fig_cases.py, 8 decoders per launch, under both swap rules.  Info, the three tables of both configurations
with their joins, labels, counters and the event list equal the models exactly: the library's host decoder dabx_fibdec for the configuration
(where the input stays below the caps), the Python model for the rest -- after the whole sequence for every input, and after every FIB for
the reconfiguration and restart cases (growing prefixes from a fresh state).  tests/test_fig_cases.py proves without a device that the inputs
reach every branch and that the model is the host build of the same walk."""
import ctypes as C

import numpy as np
import pytest

import fig_cases as fg
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu
LANES = 8                                   # decoders per launch


def _padded(names):
    """the sequences of `names` as one [len(names), n, 32] launch: shorter ones end in FIBs that fail their CRC (counted, not walked)"""
    seqs = [fg.sequences()[k] for k in names]
    n = max(len(f) for f, _ in seqs)
    fibs, crc = np.zeros((len(seqs), n, 32), np.uint8), np.zeros((len(seqs), n), np.uint8)
    for d, (f, c) in enumerate(seqs):
        fibs[d, :len(f)], crc[d, :len(f)] = f, c
    return fibs, crc


@pytest.fixture(scope="module")
def fibdec_rows():
    """the host decoder's configuration after every parity sequence, per swap rule: computed once"""
    out = {}
    for name in fg.PARITY:
        fibs, crc = fg.sequences()[name]
        for quirks in (False, True):
            d = dx.FibDecoder(reference_quirks=quirks)
            d.process(fibs, crc)
            out[name, quirks] = fg.fibdec_row(d)
            d.close()
    return out


@pytest.mark.parametrize("quirks", [False, True], ids=["default_swap", "reference_quirks"])
def test_every_input_ends_where_the_models_end(quirks, fibdec_rows):
    names = sorted(fg.sequences(), key=lambda k: len(fg.sequences()[k][0]))      # sequences of similar length share a launch
    for at in range(0, len(names), LANES):
        group = names[at:at + LANES]
        group = group + group[:LANES - len(group)]                               # always 8 decoders
        fibs, crc = _padded(group)
        rows = dx.fig_walk_device(fibs, crc, reference_quirks=quirks)
        assert len(rows) == LANES
        for name, row in zip(group, rows):
            m = fg.Model(quirks).feed(fibs[group.index(name)], crc[group.index(name)]).row()      # (the padding included)
            got = fg.plain(row)
            assert got == m, (name, [k for k in got if got[k] != m[k]])
            if name in fg.PARITY:
                want = dict(fibdec_rows[name, quirks])
                want["info"] = dict(want["info"], fibs_processed=fibs.shape[1])
                assert fg.config_part(got) == want, name


@pytest.mark.parametrize("quirks", [False, True], ids=["default_swap", "reference_quirks"])
def test_reconfigurations_and_restarts_equal_the_models_after_every_fib(quirks):
    """8 sequences of 120 FIBs (announcements with flags 1, 2 and 3, the clearing FIG 0/0 first or last in its FIB; restarts between labels; bad
    CRCs): one launch of 8 fresh decoders per prefix length.  The model's rows after every FIB are the host build's, FIB by FIB
    (tests/test_fig_cases.py), and there the host build is dabx_fibdec."""
    assert len(fg.STEPWISE) == LANES
    fibs, crc = _padded(fg.STEPWISE)
    assert fibs.shape[1] == 120 and all(len(fg.sequences()[k][0]) == 120 for k in fg.STEPWISE)
    want = [fg.model_rows(k, quirks, stepwise=True)[0] for k in fg.STEPWISE]
    for n in range(1, fibs.shape[1] + 1):
        rows = dx.fig_walk_device(fibs[:, :n], crc[:, :n], reference_quirks=quirks)
        for d, name in enumerate(fg.STEPWISE):
            got = fg.plain(rows[d])
            assert got == want[d][n - 1], (name, n, [k for k in got if got[k] != want[d][n - 1][k]])
    swaps = [want[d][-1]["info"]["n_changes"] for d in range(LANES)]
    assert swaps[:6] == ([0, 0, 0, 0, 1, 1] if quirks else [1] * 6)              # flags 1 and 2 swap under the default rule only


def test_many_decoders_of_hostile_fibs_in_one_launch():
    """tens of thousands of FIBs through the walk in one call: 64 decoders x 750 random and thinned FIBs each; every decoder ends where the
    model ends"""
    rnd, ok = fg.sequences()["random"]
    rng = np.random.default_rng(7)
    order = np.stack([rng.permutation(len(rnd))[:750] for _ in range(64)])
    fibs, crc = rnd[order], ok[order]
    rows = dx.fig_walk_device(fibs, crc)
    assert len(rows) == 64 and sum(r["info"]["fibs_processed"] for r in rows) == 48000
    for d in (0, 17, 63):
        assert fg.plain(rows[d]) == fg.Model().feed(fibs[d], crc[d]).row(), d
    assert all(r["stats"]["fibs_good"] == 750 for r in rows)


def test_the_entry_refuses_bad_arguments():
    L = dx.load()
    L.dabx_fig_walk_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9
    fibs, crc = np.zeros((1, 2, 32), np.uint8), np.ones((1, 2), np.uint8)
    none = [None] * 9
    assert L.dabx_fig_walk_device(dx._p(fibs), dx._p(crc), 1, 2, 0, *none) == 0               # every output is optional
    for args in ((None, dx._p(crc), 1, 2), (dx._p(fibs), None, 1, 2), (dx._p(fibs), dx._p(crc), 0, 2), (dx._p(fibs), dx._p(crc), 1, 0)):
        assert L.dabx_fig_walk_device(*args, 0, *none) == -2                                  # DABX_E_ARG
    with pytest.raises(ValueError):
        dx.fig_walk_device(np.zeros((2, 31), np.uint8), np.ones(2, np.uint8))
