"""The data handlers of a packet-mode slot (csrc/data_core.h: TDC, IP, Journaline) on the CPU alone: the declarations as a C compiler and
lib.py see them, the host build of the handlers -- reached through the internal entry dabx_internal_data_walk_host (dx.data_walk; not in
include/dabx.h) -- against the Python models of tests/data_handler_cases.py on every input, the inputs themselves (every branch and guard is
reached, none outside the table), the caps of the engine scenarios on the models alone, dabx_data_handler_for against the switch of
data_processor.cpp:53-101, and the stand-alone sanitizer program.  No device.

One case of the issue cannot exist: "a checksum that a full fold accepts and the single fold refuses".  An IPv4 header has at most 30
half-words, so the 32-bit sum stays below 0x1E0000, one fold leaves at most 0x1001C, and a value in 0x10000 .. 0x1001C folds on to at most
0x1D: both rules accept exactly the sums whose single fold is 0xFFFF (test_a_second_fold_never_changes_the_verdict proves it over every
sum).  In its place stands the header that only a fold accepts at all: its 32-bit sum passes 0xFFFF ("ip:125 carries")."""
import os
import struct
import subprocess

import numpy as np
import pytest

import data_handler_cases as dh
import packet_cases as pkc
from dabstar_amd import lib as dx

ROOT = os.path.join(os.path.dirname(__file__), "..")


def _inputs(handler):
    groups = dh.sequence(handler) + dh.random_groups(handler)
    if handler == "tdc":
        groups = groups + [dh.tdc_long_group(np.random.default_rng(55)), dh.overrun_group(np.random.default_rng(1))]
    return groups


def test_sizes_offsets_and_constants_as_a_c_compiler_sees_them(tmp_path):
    consts = ("DABX_DATA_HANDLER_TDC", "DABX_DATA_HANDLER_IP", "DABX_DATA_HANDLER_JOURNALINE", "DABX_DATA_HANDLER_MOT", "DABX_DATA_TDC_0", "DABX_DATA_TDC_1",
              "DABX_DATA_UDP", "DABX_DATA_NML", "DABX_DATA_CRC_OK", "DABX_DATA_NEW_REVISION", "DABX_ABI_VERSION", "DABX_DELIVER_DATA", "DABX_CHUNK_EXT2_MAGIC")
    structs = {"dabx_data_item": dx.DATA_ITEM, "dabx_data_stats": dx.DATA_STATS, "dabx_chunk_data": dx.CHUNK_DATA, "dabx_chunk_header_ext2": dx.CHUNK_HEADER_EXT2}
    fields = [(s, k) for s, dt in structs.items() for k in dt.names]
    cfg = [k for k, _ in dx.DataConfig._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dabx.h"\nint main(void)\n{\n'
                   '  printf("%zu %zu %zu ", sizeof(dabx_data_config), sizeof(dabx_data_item), sizeof(dabx_data_stats));\n'
                   '  printf("%zu %zu %zu ", sizeof(dabx_chunk_header_ext2), sizeof(dabx_chunk_data), sizeof(dabx_chunk_header_ext));\n' +
                   "".join('  printf("%%d ", (int)%s);\n' % c for c in consts) +
                   "".join('  printf("%%zu ", offsetof(%s, %s));\n' % f for f in fields) +
                   "".join('  printf("%%zu ", offsetof(dabx_data_config, %s));\n' % k for k in cfg) + '  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:6] == [32, 32, 256, 64, 128, 64]
    got = got[3:]
    assert got[3:3 + len(consts)] == [dx.DATA_HANDLERS["tdc"], dx.DATA_HANDLERS["ip"], dx.DATA_HANDLERS["journaline"], dx.DATA_HANDLER_MOT, dx.DATA_TDC_0,
                                      dx.DATA_TDC_1, dx.DATA_UDP, dx.DATA_NML, dx.DATA_CRC_OK, dx.DATA_NEW_REVISION, 6, dx.DELIVER_DATA,
                                      dx.CHUNK_EXT2_MAGIC] == [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 6, 524288, 0x32584244]
    at = 3 + len(consts)
    assert got[at:at + len(fields)] == [structs[s].fields[k][1] for s, k in fields]
    assert got[at + len(fields):] == [getattr(dx.DataConfig, k).offset for k in cfg] == [0, 4, 8, 12]
    import ctypes
    assert ctypes.sizeof(dx.DataConfig) == 32
    assert [dx.DATA_ITEM.fields[k][1] for k in dx.DATA_ITEM.names] == [0, 8, 16, 18, 19, 20, 22, 24, 28]      # no holes
    assert dx.DATA_STATS.names[:5] == ("groups", "items", "bytes", "lost", "dg_overrun") and dx.DATA_STATS.names[-3:] == ("launches", "active", "handler")
    assert all(dx.DATA_STATS.fields[k][0] == np.dtype("<i8") for k in dx.DATA_STATS.names)


def test_the_entries_are_declared_or_internal():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in ("dabx_set_data_mode", "dabx_read_data_items", "dabx_get_data_stats", "dabx_data_handler_for"):
        assert name in declared and hasattr(L, name), name
    for name in ("dabx_internal_data_walk_host", "dabx_internal_data_walk_device"):
        assert name not in declared and hasattr(L, name), name


def test_data_handler_for_is_the_switch_of_data_processor():
    table = {(5, 0x44a): 3, (5, 1500): 0, (5, 4): 1, (5, 0): 0, (5, 0x44b): 0, (44, 0): 3, (44, 4): 3, (59, 0): 2, (59, 0x44a): 2, (60, 0): 4, (60, 4): 4}      # :53-101
    for dscty in range(-1, 65):
        for app in (0, 4, 0x44a, 1500, 7, -1, 65535):
            want = table.get((dscty, app), 3 if dscty == 44 else 2 if dscty == 59 else 4 if dscty == 60 else 0)
            assert dx.data_handler_for(dscty, app) == want, (dscty, app)


@pytest.mark.parametrize("only_new", [False, True])
@pytest.mark.parametrize("handler", dh.HANDLERS)
def test_the_host_build_of_the_handlers_equals_the_model_on_every_input(handler, only_new):
    rec, by = dh.records_of(_inputs(handler))
    m = dh.run_model(handler, rec, by, only_new)
    items, ob, st = dx.data_walk(handler, rec, by, only_new)
    assert items.tobytes() == m.records().tobytes(), [(k, items[k].tolist(), m.records()[k].tolist()) for k in range(min(len(items), len(m.rows)))
                                                      if items[k].tobytes() != m.records()[k].tobytes()][:3]
    assert np.array_equal(ob, m.all_bytes())
    assert {k: st[k] for k in dx.DATA_COUNTERS} == m.counters
    assert (st["lost"], st["launches"], st["active"], st["handler"]) == (0, 0, 1, dx.DATA_HANDLERS[handler])
    # group by group: a handler keeps nothing from one group to the next but the Journaline table
    if handler != "journaline":
        some = list(range(0, len(rec), 9))
        for k in some:
            one = rec[k:k + 1].copy()
            one["byte_pos"] = 0
            g = by[int(rec[k]["byte_pos"]):int(rec[k]["byte_pos"]) + int(rec[k]["length"])]
            i1, b1, _ = dx.data_walk(handler, one, g)
            w = m.records()[m.records()["group"] == k]
            assert len(i1) == len(w) and np.array_equal(i1["length"], w["length"]) and np.array_equal(i1["flags"], w["flags"]) and np.array_equal(i1["a"], w["a"]), k


@pytest.mark.parametrize("handler", dh.HANDLERS)
def test_every_branch_and_guard_is_reached_and_none_outside_the_table(handler):
    reached = set()
    for only_new in (False, True):
        rec, by = dh.records_of(dh.sequence(handler) + ([dh.tdc_long_group(np.random.default_rng(55))] if handler == "tdc" else []))
        reached |= dh.run_model(handler, rec, by, only_new).reached
    assert reached == dh.REQUIRED[handler], (sorted(dh.REQUIRED[handler] - reached), sorted(reached - dh.REQUIRED[handler]))
    # ... and by the slots of the engine scenarios too, each stream's
    for s in range(dh.N_STREAMS):
        rec, by = dh.records_of(dh.slot_groups(s, handler))
        got = dh.run_model(handler, rec, by, dh.ONLY_NEW[s]).reached
        # (a Journaline slot without only_new_revisions holds nothing back: that one key is its other stream's)
        may_miss = {"only_new_revisions"} if handler == "journaline" and not dh.ONLY_NEW[s] else set()
        assert dh.REQUIRED[handler] - got == may_miss and got <= dh.REQUIRED[handler], (s, sorted(dh.REQUIRED[handler] - got))


def test_a_second_fold_never_changes_the_verdict():
    total = np.arange(0, 30 * 0xFFFF + 1, dtype=np.int64)             # every sum of at most 30 half-words
    once = (total >> 16) + (total & 0xFFFF)
    full = (once >> 16) + (once & 0xFFFF)
    assert np.array_equal((~once & 0xFFFF) == 0, full == 0xFFFF)


def test_the_engine_scenarios_respect_the_caps():
    """On the models alone: the packet stage completes every crafted group (nothing is overrun or lost on the way), no batch of 28 logical
    frames and no boundary-schedule batch emits more than the 256 items of the record ring, and what a handler emits is never longer than
    the groups it read."""
    for s in range(dh.N_STREAMS):
        for j, (kbps, kind) in enumerate(dh.STAGE_LAYOUT):
            if kind not in dh.HANDLERS:
                continue
            frames = dh.slot_frames(s, j)
            dm = pkc.run_model(frames, dh.ADDRESS)
            want = dh.slot_groups(s, kind)
            assert dm.groups == want, (s, kind, len(dm.groups), len(want))
            assert dm.counters["dg_overflow"] == 0 and dm.counters["len_bad"] == 0 and dm.counters["crc_bad"] == 0
            ring_rec, ring_bytes = pkc.ring_sizes(kbps)
            m = dh.model_of(kind, dm, dh.ONLY_NEW[s])
            assert m.counters["dg_overrun"] == 0 and m.counters["bytes"] <= dm.counters["dg_bytes"]
            rec, last = m.records(), dm.records()["last_frame"]
            for lo in range(0, dh.N_FRAMES, pkc.BATCH):
                in_batch = (rec["frame"] >= lo) & (rec["frame"] < lo + pkc.BATCH)
                assert in_batch.sum() <= 256, (s, kind, lo)
                g_in = (last >= lo) & (last < lo + pkc.BATCH)
                assert g_in.sum() <= ring_rec // 2 and dm.records()["length"][g_in].sum() + dx.DG_MAX_BYTES <= ring_bytes
    # no chunk window -- 28 logical frames, wherever it starts -- emits more than a slot's room in the data section: 256 records and the
    # packet slot's bytes (4 * 7 logical frames and DABX_DG_MAX_BYTES); the engine scenarios and the payloads of the delivery test
    cases = [(kbps, dh.slot_frames(s, j), kind, dh.ONLY_NEW[s]) for s in range(dh.N_STREAMS) for j, (kbps, kind) in enumerate(dh.STAGE_LAYOUT) if kind in dh.HANDLERS]
    cases += [(64, dh.frames_of(64, dh.sequence(k) + dh.random_groups(k, 60), [11, j]), k, only) for j, k in enumerate(dh.HANDLERS) for only in (False, True)]
    for kbps, frames, kind, only in cases:
        rec = dh.model_of(kind, pkc.run_model(frames, dh.ADDRESS), only).records()
        for lo in range(dh.N_FRAMES):
            w = (rec["frame"] >= lo) & (rec["frame"] < lo + pkc.BATCH)
            assert w.sum() <= 256 and rec["length"][w].sum() <= pkc.BATCH * 3 * kbps + dx.DG_MAX_BYTES, (kind, lo)
    # the overrun case is the one input that passes the cap, by design
    g = dh.overrun_group(np.random.default_rng(1))
    rec, by = dh.records_of([g])
    assert dh.run_model("tdc", rec, by).counters["items"] == 300 > 256 and len(g) == 2100


@pytest.mark.parametrize("san", [False, True])
def test_the_handlers_stand_alone_under_a_host_compiler_and_the_sanitizers(san, tmp_path):
    """tests/cxx/data_core_check.cpp: csrc/data_core.h with plain g++, without HIP, over every crafted group and random groups, each in a heap
    block of exactly its length -- as it is, and with -fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python).
    The counters it prints for the crafted groups are the model's."""
    out = os.path.join(ROOT, "tests", "cxx", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "data_core_check_san" if san else "data_core_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if san else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "dabstar_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cxx", "data_core_check.cpp")], check=True)
    files, want = [], []
    for handler in dh.HANDLERS:
        for only_new in ((False, True) if handler == "journaline" else (False,)):
            rec, by = dh.records_of(_inputs(handler))
            m = dh.run_model(handler, rec, by, only_new)
            path = tmp_path / ("%s_%d.bin" % (handler, only_new))
            with open(path, "wb") as f:
                f.write(struct.pack("<III", dx.DATA_HANDLERS[handler], int(only_new), len(rec)))
                for r in rec:
                    p, n = int(r["byte_pos"]), int(r["length"])
                    f.write(struct.pack("<IBB", n, int(r["crc_flag"]), int(r["crc_ok"])) + by[p:p + n].tobytes())
            files.append(str(path))
            c = m.counters
            want.append("file handler %d: " % dx.DATA_HANDLERS[handler] + " ".join(str(v) for v in [c["groups"], c["items"], c["bytes"], 0] + [c[k] for k in dx.DATA_COUNTERS[3:]]))
    p = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "data_core_check ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert [ln for ln in p.stdout.splitlines() if ln.startswith("file")] == want
