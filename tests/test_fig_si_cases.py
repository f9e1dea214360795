"""The service information of the device's FIG walk (csrc/fig_si_core.h inside csrc/fig_core.h) on the CPU alone: its host build, reached through
the internal entries dabx_internal_fig_si_host_* (dx.FigSiHostDecoder; not in include/dabx.h), against the line-cited Python model of
tests/fig_si_cases.py -- tables, counters, events and both service directories, on every input, after every FIB, under both swap rules.  And
the inputs themselves: every branch and guard is reached by at least one of them, and the parity inputs stay below every cap.  Plus the
declarations as a C compiler sees them, the switch off (nothing changes) and the stand-alone sanitizer program.  No device."""
import ctypes
import os
import subprocess

import pytest

import fig_cases as fg
import fig_si_cases as si
from dabstar_amd import lib as dx

ROOT = os.path.join(os.path.dirname(__file__), "..")


def test_every_branch_and_guard_is_reached_by_some_input():
    reached = set()
    for name in si.sequences():
        for quirks in (False, True):
            reached |= si.model_rows(name, quirks)[1]
    assert not (si.REQUIRED - reached), sorted(si.REQUIRED - reached)
    # by name: where the issue asks for a particular input
    ens = si.model_rows("si_ensemble", False)[0]
    kinds = [e["kind"] for e in ens["events"]]
    assert kinds.count(dx.FIG_ANNOUNCE_START) >= 2 and kinds.count(dx.FIG_ANNOUNCE_STOP) >= 2 and dx.FIG_TIME in kinds and dx.FIG_SI_TABLE in kinds
    assert ens["si"]["stats"]["asw_unknown"] == 1 and ens["si"]["stats"]["user_apps_new"] >= 5
    edges = si.model_rows("si_edges", False)[0]["si"]
    assert sorted(len(u["apps"]) for u in edges["user_apps"][0])[::len(edges["user_apps"][0]) - 1] == [0, 6] and edges["stats"]["user_apps_clamped"] == 1
    assert len(edges["user_apps"][1]) == 2 and edges["user_apps"][1][0] == edges["user_apps"][1][1]          # C/N 1: filed by every repetition
    assert edges["stats"]["outside"] >= 19
    for flags, quirks, want in ((1, False, 1), (1, True, 0), (3, False, 1), (3, True, 1)):
        row = si.model_rows("si_reconf_flags_%d" % flags, quirks)[0]
        assert row["info"]["n_changes"] == want
    strict = si.model_rows("si_reconf_flags_3", True, stepwise=True)[0]
    at = next(i for i, r in enumerate(strict) if r["info"]["n_changes"] == 1)
    assert strict[at - 1]["si"]["info"]["has_lto"] == 1 and strict[at]["si"]["info"]["has_lto"] == 0 and strict[at]["si"]["languages"] == []
    assert strict[at]["si"]["user_apps"] == [[], []] and strict[at]["si"]["global_defs"][0] == strict[at - 1]["si"]["global_defs"][1]
    loose = si.model_rows("si_reconf_flags_3", False, stepwise=True)[0]
    assert loose[at]["si"]["user_apps"][0] == loose[at - 1]["si"]["user_apps"][0] != [] and loose[at]["si"]["info"]["has_lto"] == 1
    rst = si.model_rows("si_restart", False, stepwise=True)[0]
    at = next(i for i, r in enumerate(rst) if r["info"]["n_restarts"] == 1)
    assert at % 12 not in (0, 11) and rst[at - 1]["si"]["info"]["time_set"] == 1 and rst[at]["si"]["info"]["time_set"] == 0 and rst[at]["si"]["ptys"] == []
    assert rst[-1]["si"]["info"]["time_set"] == 1 and rst[-1]["si"]["ptys"] != []
    rnd = si.sequences()["si_random"]
    assert len(rnd[0]) >= 3000 and rnd[1].all()


@pytest.mark.parametrize("quirks", [False, True])
def test_the_parity_inputs_stay_below_every_cap(quirks):
    """... at every FIB, on the model alone: no table fills and no guard counts, so nothing the bounded tables do can differ from the
    reference's unbounded vectors"""
    for name in si.PARITY:
        fibs, crc = si.sequences()[name]
        m = si.SiModel(quirks)
        for f, ok in zip(fibs, crc):
            m.walk(f, ok)
            for c, q in zip(m.cfg, m.si):
                assert len(c.comp) < fg.MAX_COMP and len(c.pkt) < fg.MAX_PKT, name
                assert len(q.gd) < si.MAX_GD and len(q.ua) < si.MAX_UA and len(q.cl) < si.MAX_CL and q.n_cm < si.MAX_CM, name
            assert len(m.lang) < si.MAX_LANG and len(m.pty) < si.MAX_PTY and all(v < fg.MAX_LAB for v in m.n_kind.values()), name
        assert [m.sc[k] for k in m.sc if k.startswith("over_")] == [0] * 5 and m.sc["cluster_fallback"] == 0, name
        assert (m.cnt["over_components"], m.cnt["over_packets"], m.cnt["over_labels"]) == (0, 0, 0), name


@pytest.mark.parametrize("quirks", [False, True])
@pytest.mark.parametrize("name", sorted(si.sequences()))
def test_the_host_build_of_the_walk_equals_the_model_fib_by_fib(name, quirks):
    fibs, crc = si.sequences()[name]
    # compared after every FIB; in the one long input (4 500 hostile FIBs) after every FIB of the first 300 and of the first 300 whose first
    # FIG is headed as an SI FIG (from FIB 3 000 on), and after every 53rd of the rest
    stops = [n for n in range(1, len(fibs) + 1) if len(fibs) <= 300 or n <= 300 or 3000 < n <= 3300 or n % 53 == 0 or n == len(fibs)]
    m = si.SiModel(quirks)
    host = dx.FigSiHostDecoder(quirks)
    at = 0
    for n in stops:
        m.feed(fibs[at:n], crc[at:n])
        host.walk(fibs[at:n], crc[at:n])
        at = n
        got, want = si.plain(host.read()), m.row()
        assert got == want, (name, n, [k for k in got if got[k] != want[k]], [k for k in got["si"] if got["si"][k] != want["si"][k]])
    assert at == len(fibs)


@pytest.mark.parametrize("name", sorted(fg.sequences()))
def test_without_the_switch_the_walk_is_the_walk_it_was(name):
    """the inputs of tests/fig_cases.py through the host build with and without the service information: the same configuration, labels and
    counters (fig0_other_ext included), the same events but for kinds 6 .. 9"""
    fibs, crc = fg.sequences()[name]
    a, b = dx.FigHostDecoder(), dx.FigSiHostDecoder()
    a.walk(fibs, crc); b.walk(fibs, crc)
    ra, rb = fg.plain(a.read()), fg.plain(b.read())
    for k in ("info", "n_tab", "subch", "packets", "labels"):
        assert ra[k] == rb[k], k
    assert {k: v for k, v in ra["stats"].items() if k != "events"} == {k: v for k, v in rb["stats"].items() if k != "events"}
    old = [e for e in rb["events"] if e["kind"] < dx.FIG_SI_TABLE]
    assert old == ra["events"][len(ra["events"]) - len(old):]
    assert ra == fg.model_rows(name, False)[0]


def test_the_internal_entries_are_not_public_and_the_public_ones_are_declared():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in ("dabx_fig_si_info", "dabx_fig_user_apps", "dabx_fig_global_defs", "dabx_fig_languages", "dabx_fig_programme_types", "dabx_fig_fec_schemes",
                 "dabx_fig_clusters", "dabx_get_fig_si_stats", "dabx_fig_directory", "dabx_fig_si_walk_device"):
        assert name in declared and hasattr(L, name), name
    for name in ("dabx_internal_fig_si_host_bytes", "dabx_internal_fig_si_host_init", "dabx_internal_fig_si_host_walk", "dabx_internal_fig_si_host_read"):
        assert name not in declared and hasattr(L, name), name


def test_sizes_and_constants_as_a_c_compiler_sees_them(tmp_path):
    consts = {"DABX_FIG_SI_TABLE": dx.FIG_SI_TABLE, "DABX_FIG_TIME": dx.FIG_TIME, "DABX_FIG_ANNOUNCE_START": dx.FIG_ANNOUNCE_START,
              "DABX_FIG_ANNOUNCE_STOP": dx.FIG_ANNOUNCE_STOP, "DABX_FIG_MAX_GLOBAL_DEFS": dx.FIG_MAX_GLOBAL_DEFS, "DABX_FIG_MAX_USER_APPS": dx.FIG_MAX_USER_APPS,
              "DABX_FIG_MAX_LANGUAGES": dx.FIG_MAX_LANGUAGES, "DABX_FIG_MAX_PTYS": dx.FIG_MAX_PTYS, "DABX_FIG_MAX_CLUSTERS": dx.FIG_MAX_CLUSTERS,
              "DABX_FIG_MAX_CLUSTER_SIDS": dx.FIG_MAX_CLUSTER_SIDS, "DABX_FIG_CLUSTER_LIST": dx.FIG_CLUSTER_LIST}
    consts.update({"DABX_FIG_SI_HAS_" + k.upper(): v for k, v in dx.FIG_SI_HAS.items()})
    consts.update({"DABX_FIG_JOIN_" + k.upper(): v for k, v in dx.FIG_JOIN.items()})
    structs = {"dabx_fig_si_scalars": dx.FIG_SI_INFO, "dabx_fig_global_def": dx.FIG_GLOBAL_DEF, "dabx_fig_user_apps_entry": dx.FIG_USER_APPS,
               "dabx_fig_language": dx.FIG_LANGUAGE, "dabx_fig_programme_type": dx.FIG_PTY, "dabx_fig_fec_scheme": dx.FIG_FEC, "dabx_fig_cluster": dx.FIG_CLUSTER,
               "dabx_fig_si_stats": dx.FIG_SI_STATS, "dabx_fig_service": dx.FIG_SERVICE}
    fields = [(s, k) for s, dt in structs.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dabx.h"\nint main(void)\n{\n' +
                   "".join('  printf("%%zu ", sizeof(%s));\n' % s for s in structs) + '  printf("%zu %zu ", sizeof(dabx_fig_config), offsetof(dabx_fig_config, service_info));\n' +
                   "".join('  printf("%%d ", (int)%s);\n' % c for c in consts) +
                   "".join('  printf("%%zu ", offsetof(%s, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    n = len(structs)
    assert got[:n] == [dt.itemsize for dt in structs.values()] == [128, 12, 64, 16, 16, 8, 128, 256, 128]
    assert got[n:n + 2] == [16, 8] and ctypes.sizeof(dx.FigConfig) == 16 and dx.FigConfig.service_info.offset == 8
    assert got[n + 2:n + 2 + len(consts)] == list(consts.values())
    assert got[n + 2 + len(consts):] == [structs[s].fields[k][1] for s, k in fields]


@pytest.mark.parametrize("san", [False, True])
def test_the_si_walk_stands_alone_under_a_host_compiler_and_the_sanitizers(san):
    """tests/cxx/fig_si_core_check.cpp: csrc/fig_core.h with the service information, plain g++, without HIP, over random, thinned and
    truncated FIBs, each in a heap block of its 30 bytes -- as it is, and with -fsanitize=address,undefined (a stand-alone program: nothing
    is loaded into Python)."""
    out = os.path.join(ROOT, "tests", "cxx", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fig_si_core_check_san" if san else "fig_si_core_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if san else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "dabstar_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cxx", "fig_si_core_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "fig_si_core_check ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
