"""No device: the PAD model and scenarios of tests/pad_cases.py on their own -- that the committed scenarios reach every branch of
mp4processor.cpp:345-353 and pad_handler.cpp:67-547 and each side of every guard (a coverage table keyed by reference line), that the
scenarios' super frames are accepted or rejected by the oracle back end (oracle/msc.c) as intended, that the model's check_crc_bytes is
the reference's, and that the new entry points are declared and exported.  The GPU tests compare the device with this model on exactly
these scenarios."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import pad_cases as pc
from dabstar_amd import lib as dx

NEW_SYMBOLS = ("dabx_set_pad_mode", "dabx_read_pad_items", "dabx_get_pad_stats")

# every branch of the restatement and each side of every guard, by reference line (pad_handler.cpp unless it says mp4)
COVERAGE = (
    "mp4:325 impossible length", "mp4:377 wrong AU CRC", "mp4:345 element id != 4",
    "G1 count 0", "G1 count 1", "G1 count 2", "G1 count 5", "G1 count 6", "G1 count > 6", "G1 ends at the super frame's end",
    "G1 one byte beyond the super frame", "G1 beyond the AU, inside the super frame",
    ":71 F-PAD type != 0", ":83 X-PAD indicator 0", ":83 X-PAD indicator 3",
    "G2 short X-PAD, iLast 2", "G2 short X-PAD, iLast 3",
    ":122 charset change", ":126 first segment clears", ":132 short, other application type", ":134 short, end marker",
    ":137 short, start of fragment", ":138 first and not last", ":154 short, continuation", ":163 append",
    ":173 short without CI, data taken", ":173 short without CI, nothing to take", ":183 append", ":183 unsolicited append",
    ":188 end of the last segment", ":193 signal_show_label",
    ":217 no-CI, mXPadLength not set", ":219 no-CI X-PAD shorter than mXPadLength", ":234 no-CI continuation of a label",
    ":239 no-CI continuation without mMscGroupElement", ":240 no-CI continuation of a group", ":242 no-CI, other last application type",
    ":259 end marker", ":262 four CIs, no end marker",
    "G3 CI list below index 0", "G3 CI list ends at index 0", "G3 sub-field below index 0", "G3 sub-field ends at index 0",
    ":294 data group length", ":298 length indicator, bad CRC", ":298 length indicator, length != 4",
    ":318 unknown application type, in the middle of the list", ":318 unknown application type, last of the list",
    ":350 first segment", ":353 charset change", ":361 segment number mismatch, missing or other", ":361 segment number mismatch, no first before",
    ":361 segment number mismatch, repeated", ":375 clear command", ":382 other command", ":396 segment continues", ":407 append",
    ":416 signal_show_label", ":433 continuation without mMoreXPad", ":435 continuation, more to come", ":440 continuation, complete",
    ":446 append", ":452 signal_show_label",
    "G4 text at the bound", "G4 dropped at :163", "G4 dropped at :183",
    ":475 single item", ":484 start of a group", ":494 type 13 without type 12", ":507 group continues", ":512 group complete",
    ":528 mDataGroupLength well below the buffer", ":530 size < 2", ":541 group with a good CRC", ":541 group with a bad CRC",
    ":541 group with no CRC flag", "group of 2 bytes", "group of 3 .. 255 bytes", "group of 256 .. 4095 bytes", "group of 16383 bytes",
    "label while a group is under assembly",
) + tuple(":367 segment %d" % n for n in range(2, 9)) + tuple("label segment of %d bytes" % n for n in range(1, 17)) + \
    tuple("sub-field of %d bytes" % n for n in pc.CI_LENGTHS)


def _pad_slots():
    return [(s, j, kbps) for s, lay in enumerate(pc.STAGE_STREAMS) for j, (kbps, kind) in enumerate(pc.STAGE_LAYOUTS[lay]) if kind == "pad"]


def test_new_symbols_are_declared_and_exported_in_both_library_forms_and_the_records_have_their_sizes(tmp_path):
    assert set(NEW_SYMBOLS) <= set(dx.declared_symbols())
    assert dx.PAD_ITEM.itemsize == 32 and dx.PAD_STATS.itemsize == 128 and dx.CHUNK_PAD.itemsize == 128 and C.sizeof(dx.PadConfig) == 32
    assert dx.Engine.set_pad_mode and dx.Engine.read_pad_items and dx.Engine.pad_stats and dx.DELIVER_PAD == 32
    L = dx.load()
    missing = [n for n in NEW_SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    so = os.path.join(os.path.dirname(os.path.abspath(dx.__file__)), "hipmodule", "libdabx.so")
    if not os.path.exists(so):
        from dabstar_amd import build as b
        b.build_hipmodule()
    M = C.CDLL(so)
    missing = [n for n in NEW_SYMBOLS if not hasattr(M, n)]
    assert not missing, missing
    src = tmp_path / "t.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(dabx_pad_item), offsetof(dabx_pad_item, length), offsetof(dabx_pad_item, kind),
         offsetof(dabx_pad_item, crc_ok), sizeof(dabx_pad_stats), offsetof(dabx_pad_stats, items_lost), offsetof(dabx_pad_stats, active),
         sizeof(dabx_pad_config), sizeof(dabx_chunk_pad), offsetof(dabx_chunk_header, off_pad), DABX_DL_MAX_BYTES, DABX_DELIVER_PAD, DABX_ABI_VERSION);
  return 0;
}
""")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    f, g = dx.PAD_ITEM.fields, dx.PAD_STATS.fields
    assert got == [32, f["length"][1], f["kind"][1], f["crc_ok"][1], 128, g["items_lost"][1], g["active"][1], 32, 128,
                   dx.CHUNK_HEADER.fields["off_pad"][1], dx.DL_MAX_BYTES, dx.DELIVER_PAD, 6], got
    assert got[1] == 16 and got[3] == 22 and got[9] == 104 and got[10] == 256


def test_the_model_on_hand_made_access_units():
    """The rules that are easy to get wrong, on PADs small enough to check by eye."""
    rng = np.random.default_rng(5)

    def run(pads):
        m = pc.PadModel()
        for k, p in enumerate(pads):
            m.frame, m.au = k, 0
            m.process_pad(p, len(p) - 3, p[-2], p[-1])
        return m
    L = lambda *a, **kw: pc.label_fields(rng, *a, **kw)      # noqa: E731
    # one segment, first and last; two segments; the text is not cleared by showing it, a second "last" shows it grown
    m = run([pc.var_ci(L(b"hello", 1, 1, charset=4)), pc.var_ci(L(b"ab", 1, 0) + L(b"cd", 0, 1, 1)), pc.var_ci(L(b"ef", 0, 1, 2))])
    assert m.payloads == [b"hello", b"abcd"] and [r[5] for r in m.rows] == [4, 0] and m.segment_no == -1
    # mXPadLength counts the CI bytes and the end marker: the no-CI continuation takes 6 + 2 bytes, of which the label wants 4
    m = run([pc.var_ci(L(b"12345678", 1, 1, size=6)[:1]), pc.var_noci(b"5678zzzz")])
    assert m.xpad_length == 8 and m.payloads == [b"12345678"]
    m = run([pc.var_ci(L(b"123456789012", 1, 1, size=6)[:1]), pc.var_noci(b"56789012"), pc.var_noci(b"!!!!!!!!")])
    assert m.payloads == [b"123456789012"] and m.more_xpad is False and m.branch[":433 continuation without mMoreXPad"] == 1
    # a data group over two X-PADs, the length indicator in front; a bad indicator leaves the length; type 13 alone goes nowhere
    g = pc.data_group(rng, 20, True)
    fs = pc.group_fields(rng, g, [12])
    m = run([pc.var_ci(fs[:2]), pc.var_ci([pc.length_indicator(rng, 9, good=False)] + fs[2:]), pc.var_ci([(13, bytes(8))])])
    assert m.payloads == [g] and m.rows[0][6:8] == (1, 1) and m.counters["li_bad"] == 1 and m.branch[":494 type 13 without type 12"] == 1
    # the group is cut at mDataGroupLength, the CRC is looked for there
    m = run([pc.var_ci([pc.length_indicator(rng, 10), (12, g[:12])])])
    assert m.payloads == [g[:10]] and m.rows[0][6:8] == (1, 0) and m.counters["dg_crc_bad"] == 1
    # G3: the walk stops in front of the sub-field that lies below index 0, with mXPadLength set and mLastAppType from the one before
    p = pc.var_ci(L(b"ab", 1, 0) + [(12, bytes(8))])
    m = run([p[1:]])
    assert m.counters["pad_bad"] == 1 and m.xpad_length == 4 + 8 + 3 and m.last_app_type == 2 and bytes(m.text) == b"ab" and not m.msc
    # G4: an append beyond 256 bytes is dropped whole
    m = pc.PadModel()
    m.text = bytearray(250)
    m.append(b"1234567", ":163")
    m.append(b"123456", ":163")
    assert len(m.text) == 256 and m.counters["dl_overflow"] == 1


def test_the_scenarios_reach_every_branch_and_each_side_of_every_guard():
    branch, counters = collections.Counter(), collections.Counter()
    rates = set()
    for s, j, kbps in _pad_slots():
        m = pc.slot_model(s, j)
        branch.update(m.branch)
        counters.update(m.counters)
        rates.add(kbps)
        facts = pc.scenario(kbps, pc.seed_of(s, j))[1]
        assert facts["scripted_left"] == 0, (s, j, kbps, facts["scripted_left"])          # everything the script lists went into an AU
        assert m.counters["labels"] > 0 and m.counters["groups"] > 0 and len(m.all_bytes()) == m.counters["label_bytes"] + m.counters["group_bytes"]
        assert m.max_msc <= 16382 + 196
    print(sorted(branch.items()), dict(counters))
    assert sorted(rates) == pc.RATES
    missing = [k for k in COVERAGE if branch[k] == 0]
    assert not missing, missing
    for k in pc.PAD_COUNTERS:
        assert counters[k] > 0, k
    # no line of the model that is not in the table (a new branch must be listed)
    extra = sorted(set(branch) - set(COVERAGE) - {"G1 count 3", "G1 count 4", "G1 beyond the super frame", "group of 4096 and more bytes"})
    assert not extra, extra


def test_the_four_au_layouts_at_every_rate_and_items_across_batch_boundaries():
    sched = pc.boundary_schedule(len(pc.STAGE_STREAMS))
    assert {c for row in sched for c in row} >= {0, 1, 4, 5, 6, 13, 27, 28}
    layouts = collections.defaultdict(set)
    over_batch = 0
    for s, j, kbps in _pad_slots():
        o = pc.stream_case(s)[3][j]
        layouts[kbps] |= {int(v) for v in o["sfi"]["num_aus"]}
        m = pc.slot_model(s, j)
        r = m.records()
        big = r[(r["kind"] == dx.PAD_DATAGROUP) & (r["length"] == 16383)]
        over_batch += len(big)
    assert all(layouts[k] == {2, 3, 4, 6} for k in (8, 32, 64)) and layouts[192] == {6}, dict(layouts)
    assert over_batch >= 2          # 16 383 bytes at 192 bytes per AU and 6 AUs per super frame: 15 super frames, 75 logical frames


def test_the_oracle_accepts_and_rejects_the_super_frames_as_intended():
    for s, lay in enumerate(pc.STAGE_STREAMS):
        layout, frames, _, want = pc.stream_case(s)
        for j, (kbps, kind) in enumerate(pc.STAGE_LAYOUTS[lay]):
            assert np.array_equal(want[j]["frames"], frames[j]), (s, j)
            if kind not in ("pad", "dab+"):
                assert len(want[j]["sf"]) == 0
                continue
            facts = pc.scenario(kbps, pc.seed_of(s, j))[1]
            o = want[j]
            assert len(o["sf"]) == len(facts["sf"]) == pc.N_FRAMES // 5 - len(facts["lost"]), (s, j, len(o["sf"]), len(facts["sf"]))
            assert all(np.array_equal(a, b) for a, b in zip(o["sf"], facts["sf"])), (s, j)
            got = sorted(set(range(pc.N_FRAMES // 5)) - {int(v) // 5 for v in o["sfi"]["first_frame"]})
            assert got == facts["lost"] and (kbps != 64 or len(got) == 1), (s, j, got, facts["lost"])
            bad_crc = sum(int(r["num_aus"]) - bin(int(r["au_crc_ok"])).count("1") - bin(int(r["au_len_bad"])).count("1") for r in o["sfi"])
            len_bad = sum(bin(int(r["au_len_bad"])).count("1") for r in o["sfi"])
            assert (bad_crc, len_bad) == ({32: 1, 64: 1}.get(kbps, 0), {32: 1, 64: 1}.get(kbps, 0)), (s, j, bad_crc, len_bad)


def test_check_crc_bytes_of_the_model_is_the_references_on_every_length_indicator_and_group():
    if not ol.have_ref():
        pytest.skip("oracle/_ref is not built")
    R = ol.ref()
    n = bad = 0
    for s, j, kbps in _pad_slots():
        for msg, ln in pc.slot_model(s, j).crc_calls:
            want = bool(R.ref_check_crc_bytes(np.frombuffer(msg, np.uint8).copy(), ln))
            assert pc.check_crc_bytes(msg, ln) == want, (s, j, n, ln)
            n += 1
            bad += not want
    assert n > 200 and 0 < bad < n
