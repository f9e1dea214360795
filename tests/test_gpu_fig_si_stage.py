"""dabx_fig_si_walk_device: the device's FIG walk with the service information followed (csrc/fig_si_core.h inside csrc/fig_core.h, one wave per
decoder: k_fig_si_batch, the device function of the engine's k_fig_si) and the service directory (k_fig_directory, a lane per component) on the
crafted FIB sequences of tests/fig_si_cases.py, under both swap rules.  Everything equals the Python model exactly: the configuration, labels,
counters and events of tests/fig_cases.py, the SI tables, the SI counters, the SI events and both directories.  The shapes are the smallest
that can go wrong: 1 and 7 decoders; FIG 0/8 tables of 63, 64, 65 and 129 entries (the ballot looks at 64 keys a round); a full cluster table;
directories of 0, 1, 64, 65 and DABX_FIG_MAX_COMPONENTS components (the directory steps by 64 lanes).  tests/test_fig_si_cases.py proves
without a device that the inputs reach every branch and that the model is the host build of the same walk."""
import ctypes as C

import numpy as np
import pytest

import fig_si_cases as si
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu


def _padded(names):
    """the sequences of `names` as one [len(names), n, 32] launch: shorter ones end in FIBs that fail their CRC (counted, not walked)"""
    seqs = [si.sequences()[k] for k in names]
    n = max(len(f) for f, _ in seqs)
    fibs, crc = np.zeros((len(seqs), n, 32), np.uint8), np.zeros((len(seqs), n), np.uint8)
    for d, (f, c) in enumerate(seqs):
        fibs[d, :len(f)], crc[d, :len(f)] = f, c
    return fibs, crc


def _check(names, quirks):
    fibs, crc = _padded(names)
    rows = dx.fig_si_walk_device(fibs, crc, reference_quirks=quirks)
    assert len(rows) == len(names)
    for d, name in enumerate(names):
        want = si.SiModel(quirks).feed(fibs[d], crc[d]).row()                    # (the padding included)
        got = si.plain(rows[d])
        assert got == want, (name, [k for k in got if got[k] != want[k]], [k for k in got["si"] if got["si"][k] != want["si"][k]])
    return rows


GROUPS = (("si_ensemble", "si_reconf_flags_1", "si_reconf_flags_3", "si_restart", "si_edges", "si_bad_crc", "si_clusters"),       # 7 decoders
          ("si_gd_63", "si_gd_64", "si_gd_65", "si_gd_129"), ("si_caps",), ("si_dir_1",))


@pytest.mark.parametrize("quirks", [False, True], ids=["default_swap", "reference_quirks"])
@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_every_input_ends_where_the_model_ends(group, quirks):
    assert {n for g in GROUPS for n in g} | {"si_random"} == set(si.sequences())
    rows = _check(group, quirks)
    by = dict(zip(group, rows))
    if "si_gd_63" in by:                                                         # the shapes the issue names, as the device saw them
        assert [by["si_gd_%d" % n]["si"]["info"]["n_global_defs"][0] for n in (63, 64, 65, 129)] == [63, 64, 65, 129]
        assert [len(by["si_gd_%d" % n]["dir"][0]) for n in (63, 64, 65, 129)] == [63, 64, 65, 129]
        assert all(by["si_gd_%d" % n]["si"]["stats"]["global_def_known"] == len(range(0, n, 7)) for n in (63, 64, 65, 129))
    if "si_clusters" in by:
        s = by["si_clusters"]["si"]
        assert s["info"]["n_clusters"][0] == dx.FIG_MAX_CLUSTERS and s["stats"]["cluster_fallback"] > 0 and s["stats"]["asw_start"] == 1
        assert by["si_edges"]["dir"] == [[], []]                                 # a directory of no component
    if "si_caps" in by:
        s = by["si_caps"]["si"]
        assert (s["info"]["n_global_defs"][0], s["info"]["n_user_apps"][0], s["info"]["n_languages"], s["info"]["n_ptys"], s["info"]["n_cluster_sids"][0]) == \
            (dx.FIG_MAX_GLOBAL_DEFS, dx.FIG_MAX_USER_APPS, dx.FIG_MAX_LANGUAGES, dx.FIG_MAX_PTYS, dx.FIG_MAX_CLUSTER_SIDS)
        assert len(by["si_caps"]["dir"][0]) == dx.FIG_MAX_COMPONENTS
    if "si_dir_1" in by:
        assert len(by["si_dir_1"]["dir"][0]) == 1 and by["si_dir_1"]["dir"][0][0]["joined"] == dx.FIG_JOIN["subch"]


def test_the_ensemble_after_every_frame_from_a_fresh_state():
    """growing prefixes of the ensemble with announcements, one decoder per prefix length (a frame more each): one launch of 18 decoders"""
    fibs, crc = si.sequences()["si_ensemble"]
    n = len(fibs) // 12
    batch, ok = np.zeros((n, len(fibs), 32), np.uint8), np.zeros((n, len(fibs)), np.uint8)
    for d in range(n):
        batch[d, :12 * (d + 1)], ok[d, :12 * (d + 1)] = fibs[:12 * (d + 1)], crc[:12 * (d + 1)]
    rows = dx.fig_si_walk_device(batch, ok)
    for d in range(n):
        want = si.SiModel().feed(batch[d], ok[d]).row()
        got = si.plain(rows[d])
        assert got == want, (d, [k for k in got if got[k] != want[k]])
    kinds = {e["kind"] for e in rows[-1]["events"]}
    assert {dx.FIG_SI_TABLE, dx.FIG_TIME, dx.FIG_ANNOUNCE_START, dx.FIG_ANNOUNCE_STOP} <= kinds


def test_hostile_fibs_and_the_walk_without_the_switch():
    """4 500 random, thinned and SI-headed FIBs through one decoder; and the same FIBs through dabx_fig_walk_device: what that entry returns
    is what the SI entry returns for the same keys -- the service information disturbs nothing that exists"""
    fibs, crc = si.sequences()["si_random"]
    row = _check(("si_random",), False)[0]
    plain = dx.fig_walk_device(fibs[None], crc[None])[0]
    for k in ("info", "n_tab", "subch", "labels"):
        assert plain[k] == row[k], k
    assert all(np.array_equal(a, b) for a, b in zip(plain["packets"], row["packets"]))
    assert {k: v for k, v in plain["stats"].items() if k != "events"} == {k: v for k, v in row["stats"].items() if k != "events"}
    old = [e for e in row["events"] if e["kind"] < dx.FIG_SI_TABLE]              # (both rings hold their newest 256: the SI ring fewer of the old kinds)
    assert old and old == plain["events"][-len(old):]
    assert row["si"]["stats"]["outside"] > 100 and row["si"]["stats"]["si_figs"] > 1000


def test_the_entry_refuses_bad_arguments():
    L = dx.load()
    L.dabx_fig_si_walk_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 19
    fibs, crc = np.zeros((1, 2, 32), np.uint8), np.ones((1, 2), np.uint8)
    none = [None] * 19
    assert L.dabx_fig_si_walk_device(dx._p(fibs), dx._p(crc), 1, 2, 0, *none) == 0            # every output is optional
    for args in ((None, dx._p(crc), 1, 2), (dx._p(fibs), None, 1, 2), (dx._p(fibs), dx._p(crc), 0, 2), (dx._p(fibs), dx._p(crc), 1, 0)):
        assert L.dabx_fig_si_walk_device(*args, 0, *none) == -2                               # DABX_E_ARG
