"""The FIG walk of the device (csrc/fig_core.h) on the CPU alone: its host build, reached through the internal entries
dabx_internal_fig_host_* (dx.FigHostDecoder; not in include/dabx.h), against the library's own host decoder dabx_fibdec for the configuration
and against the Python model of tests/fig_cases.py for labels, events, guards and counters -- on every input, after every FIB, under both
swap rules.  And the inputs themselves: every branch and guard is reached by at least one of them, and the parity inputs stay below every
cap, so that dabx_fibdec alone is a complete model of their configuration.  Plus the stand-alone sanitizer program.  No device."""
import os
import subprocess

import numpy as np
import pytest

import fig_cases as fg
from dabstar_amd import lib as dx

ROOT = os.path.join(os.path.dirname(__file__), "..")


def test_every_branch_and_guard_is_reached_by_some_input():
    reached = set()
    for name in fg.sequences():
        for quirks in (False, True):
            reached |= fg.model_rows(name, quirks)[1]
    assert not (fg.REQUIRED - reached), sorted(fg.REQUIRED - reached)
    # by name: where the issue asks for a particular input
    assert "label_new_after_restart" in fg.model_rows("restart_labels", False)[1]
    row = fg.model_rows("restart_labels", False)[0]
    first = [e for e in row["events"] if e["kind"] == dx.FIG_LABEL_EVENT and e["label"]["label"] == fg.label16("First label")]
    assert [e["epoch"] for e in first] == [0, 1, 2]           # filed and reported again after each of the two restarts
    assert {"fig00_first"} <= fg.model_rows("reconf_flags_3_fig00_first", False)[1] and {"fig00_last"} <= fg.model_rows("reconf_flags_3_fig00_last", False)[1]
    caps = fg.model_rows("caps", False)[0]
    assert caps["n_tab"][0] == [0, fg.MAX_COMP, fg.MAX_PKT] and len(caps["labels"]) == 1 + 3 * fg.MAX_LAB
    assert (caps["stats"]["over_components"], caps["stats"]["over_packets"], caps["stats"]["over_labels"]) == (2, 2, 4)
    rnd = fg.sequences()["random"]
    assert len(rnd[0]) >= 2000 and rnd[1].all()


@pytest.mark.parametrize("quirks", [False, True])
def test_the_parity_inputs_stay_below_every_cap(quirks):
    """... at every FIB: the tables never fill, no guard counts, so nothing the device does there can differ from the unbounded host vectors"""
    for name in fg.PARITY:
        fibs, crc = fg.sequences()[name]
        m = fg.Model(quirks)
        for f, ok in zip(fibs, crc):
            m.walk(f, ok)
            for c in m.cfg:
                assert len(c.sub) <= fg.MAX_SUB and len(c.comp) < fg.MAX_COMP and len(c.pkt) < fg.MAX_PKT, name
            assert all(v < fg.MAX_LAB for v in m.n_kind.values()), name
        assert (m.cnt["over_components"], m.cnt["over_packets"], m.cnt["over_labels"]) == (0, 0, 0), name


@pytest.mark.parametrize("quirks", [False, True])
@pytest.mark.parametrize("name", sorted(fg.sequences()))
def test_the_host_build_of_the_walk_equals_fibdec_and_the_model_fib_by_fib(name, quirks):
    fibs, crc = fg.sequences()[name]
    rows, _ = fg.model_rows(name, quirks, stepwise=True)
    host = dx.FigHostDecoder(quirks)
    ref = dx.FibDecoder(reference_quirks=quirks) if name in fg.PARITY else None
    for i, (f, ok) in enumerate(zip(fibs, crc)):
        host.walk(f[None], [ok])
        got = fg.plain(host.read())
        assert got == rows[i], (name, i, [k for k in got if got[k] != rows[i][k]])
        if ref is not None:
            ref.process(f[None], [ok])
            assert fg.config_part(got) == fg.fibdec_row(ref), (name, i)
    if ref is not None:
        ref.close()
    # chunking of the calls changes nothing
    whole = dx.FigHostDecoder(quirks)
    whole.walk(fibs, crc)
    assert fg.plain(whole.read()) == rows[-1]


def test_the_internal_entries_are_not_public_and_the_public_ones_are_declared():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in ("dabx_set_fig_mode", "dabx_fig_info", "dabx_fig_subchannels", "dabx_fig_packet_components", "dabx_fig_follow", "dabx_fig_labels",
                 "dabx_get_fig_stats", "dabx_read_fig_events", "dabx_fig_walk_device"):
        assert name in declared and hasattr(L, name), name
    for name in ("dabx_internal_fig_host_bytes", "dabx_internal_fig_host_init", "dabx_internal_fig_host_walk", "dabx_internal_fig_host_read"):
        assert name not in declared and hasattr(L, name), name
    assert (dx.DELIVER_FIG, dx.CHUNK_HEADER_EXT.fields["off_fig"][1], dx.CHUNK_HEADER_EXT.itemsize) == (262144, 56, 64)


def test_sizes_and_constants_as_a_c_compiler_sees_them(tmp_path):
    consts = ("DABX_DELIVER_FIG", "DABX_FIG_MAX_COMPONENTS", "DABX_FIG_MAX_PACKETS", "DABX_FIG_MAX_LABELS", "DABX_FIG_MAX_EVENTS", "DABX_FIG_CHUNK_RECORDS",
              "DABX_FIG_ANNOUNCE", "DABX_FIG_SWAP", "DABX_FIG_RESTART", "DABX_FIG_TABLE", "DABX_FIG_LABEL")
    structs = {"dabx_fig_label": dx.FIG_LABEL, "dabx_fig_stats": dx.FIG_STATS, "dabx_chunk_fig": dx.CHUNK_FIG, "dabx_chunk_header_ext": dx.CHUNK_HEADER_EXT}
    fields = [(s, k) for s, dt in structs.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dabx.h"\nint main(void)\n{\n'
                   '  printf("%zu %zu %zu %zu %zu %zu ", sizeof(dabx_fig_config), sizeof(dabx_fig_label), sizeof(dabx_fig_event), sizeof(dabx_fig_stats),'
                   ' sizeof(dabx_chunk_fig), sizeof(dabx_chunk_header_ext));\n'
                   '  printf("%zu %zu %zu %zu %zu ", offsetof(dabx_fig_event, kind), offsetof(dabx_fig_event, epoch), offsetof(dabx_fig_event, frame),'
                   ' offsetof(dabx_fig_event, fib), offsetof(dabx_fig_event, cif));\n'
                   '  printf("%zu %zu %zu ", offsetof(dabx_fig_event, u), offsetof(dabx_fig_event, u.announce.at_cif), offsetof(dabx_fig_event, u.swap.n_packets));\n' +
                   "".join('  printf("%%d ", (int)%s);\n' % c for c in consts) +
                   "".join('  printf("%%zu ", offsetof(%s, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:6] == [16, 32, 64, 256, 32, 64]
    assert got[6:14] == [0, 4, 8, 16, 24, 32, 40, 44]
    assert [dx.FIG_EVENT.fields[k][1] for k in ("kind", "epoch", "frame", "fib", "cif", "words")] == [0, 4, 8, 16, 24, 32]
    assert got[14:14 + len(consts)] == [dx.DELIVER_FIG, dx.FIG_MAX_COMPONENTS, dx.FIG_MAX_PACKETS, dx.FIG_MAX_LABELS, dx.FIG_MAX_EVENTS, dx.FIG_CHUNK_RECORDS,
                                        dx.FIG_ANNOUNCE, dx.FIG_SWAP, dx.FIG_RESTART, dx.FIG_TABLE, dx.FIG_LABEL_EVENT]
    assert got[14 + len(consts):] == [structs[s].fields[k][1] for s, k in fields]
    import ctypes
    assert ctypes.sizeof(dx.FigConfig) == 16


@pytest.mark.parametrize("san", [False, True])
def test_the_walk_stands_alone_under_a_host_compiler_and_the_sanitizers(san):
    """tests/cxx/fig_core_check.cpp: csrc/fig_core.h with plain g++, without HIP, over random, thinned and truncated FIBs -- as it is, and with
    -fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python)."""
    out = os.path.join(ROOT, "tests", "cxx", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fig_core_check_san" if san else "fig_core_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if san else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "dabstar_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cxx", "fig_core_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "fig_core_check ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
