"""No device: the MOT model and scenarios of tests/mot_cases.py on their own -- that the committed scenarios reach every branch of
pad_handler.cpp:539-622 and mot_object.cpp:71-323 and each side of the guards M1..M3 (a coverage table keyed by reference line), that the
builders put every crafted group into X-PADs from which PadHandler's restatement (tests/pad_cases.py) takes out exactly those groups, that
the rules that are easy to get wrong hold on groups small enough to check by eye, and that the new entry points are declared and exported
with the record layouts include/dabx.h states.  The GPU tests compare the device with this model on exactly these scenarios."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import mot_cases as mc
from dabstar_amd import lib as dx

NEW_SYMBOLS = ("dabx_set_mot_mode", "dabx_read_mot_objects", "dabx_get_mot_stats")

# every branch of the restatement and each side of every guard, by reference line (ph: pad_handler.cpp, mo: mot_object.cpp)
COVERAGE = (
    "ph:543 bad CRC", "ph:546 good CRC", "ph:550 no CRC flag", "ph:558 type 0", "ph:558 type 6", "ph:564 extension flag 0",
    "ph:564 extension flag 1", "ph:567 segment field", "ph:567 no segment field", "ph:579 no user access field",
    "ph:587 transport id, length indicator 0", "ph:587 transport id, length indicator 1", "ph:587 transport id, length indicator 2",
    "ph:587 transport id, length indicator 15", "ph:587 transport id, length indicator other", "ph:595 no transport id",
    "M1 segment field", "M1 user access field", "M1 transport id", "M1 segmentation header", "M1 segment ends exactly at length",
    "M1 segment one byte beyond length", "M1 segment beyond length",
    "M2 segment of 6 bytes", "M2 segment of fewer than 6 bytes", "M2 segment of 7 bytes", "M2 parameter byte beyond the segment",
    "M2 length byte beyond the segment", "M2 second length byte beyond the segment", "M2 name ends exactly at the segment's end",
    "M2 name one byte beyond the segment", "M2 name beyond the segment",
    "M3 exactly max_object_bytes", "M3 one byte beyond max_object_bytes", "M3 beyond max_object_bytes",
    "mo:75 transport id changes at a header", "mo:75 transport id changes at a header, object under way", "mo:106 pointer == headerSize",
    "mo:106 pointer != headerSize", "mo:111 header", "mo:119 segment number 8191", "mo:121 segment number -1", "mo:121 segment number 8192",
    "mo:121 segment number above 8192", "mo:125 transport id changes at a body segment",
    "mo:125 transport id changes at a body segment, object under way", "mo:141 duplicate segment", "mo:147 last flag", "mo:147 last flag moves",
    "mo:160 no progress: no header yet", "mo:160 no progress: bodySize 0", "mo:160 no progress: not an image", "mo:165 progress clamped",
    "mo:168 progress", "mo:182 ContentName", "mo:182 ContentName replaces a name", "mo:182 ContentName replaces a name, empty",
    "mo:182 ContentName, empty", "mo:201 parameter whose value is walked", "mo:204 unknown parameter", "mo:219 PLI 0", "mo:219 PLI 1",
    "mo:219 PLI 2", "mo:225 PLI 3, 15-bit length", "mo:230 PLI 3, 7-bit length", "mo:244 no header core",
    "mo:250 number of segments unknown", "mo:256 fewer segments than needed", "mo:273 a segment below the last is missing",
    "mo:288 a segment numbered beyond the last is emitted", "mo:293 no name", "mo:300 with a name", "mo:300 emit, repeat 0",
    "mo:300 emit, repeat 1", "mo:300 emit, repeat 2", "mo:300 emit, repeat 3 and more", "mo:313 reset",
)


def _slots():
    return [(s, j) for s in range(mc.N_STREAMS) for j, (_, kind) in enumerate(mc.STAGE_LAYOUT) if kind == "mot"]


def _model(s, j):
    rec, by = mc.items_of(mc.slot_groups(s, j))
    return mc.run_model(rec, by, mc.max_bytes_of(j))


def test_new_symbols_are_declared_and_exported_in_both_library_forms_and_the_records_have_their_layout(tmp_path):
    assert set(NEW_SYMBOLS) <= set(dx.declared_symbols())
    assert dx.MOT_OBJECT.itemsize == 32 and dx.MOT_STATS.itemsize == 128 and dx.CHUNK_MOT.itemsize == 128 and C.sizeof(dx.MotConfig) == 32
    assert dx.Engine.set_mot_mode and dx.Engine.read_mot_objects and dx.Engine.mot_stats and dx.DELIVER_MOT == 64
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
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(dabx_mot_object), offsetof(dabx_mot_object, frame), offsetof(dabx_mot_object, body_len),
         offsetof(dabx_mot_object, body_size), offsetof(dabx_mot_object, transport_id), offsetof(dabx_mot_object, content_type),
         offsetof(dabx_mot_object, name_len), offsetof(dabx_mot_object, au), offsetof(dabx_mot_object, repeat));
  printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(dabx_mot_stats), offsetof(dabx_mot_stats, objects_lost), offsetof(dabx_mot_stats, crc_bad),
         offsetof(dabx_mot_stats, progress_pct), offsetof(dabx_mot_stats, transport_id), offsetof(dabx_mot_stats, segments_stored),
         offsetof(dabx_mot_stats, active));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(dabx_mot_config), offsetof(dabx_mot_config, max_object_bytes), sizeof(dabx_chunk_mot),
         offsetof(dabx_chunk_mot, rec_off), offsetof(dabx_chunk_mot, objects), offsetof(dabx_chunk_mot, progress_events), sizeof(dabx_chunk_header),
         offsetof(dabx_chunk_header, off_mot), DABX_DELIVER_MOT, DABX_ABI_VERSION);
  return 0;
}
""")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    f, g, t = dx.MOT_OBJECT.fields, dx.MOT_STATS.fields, dx.CHUNK_MOT.fields
    assert got == [32] + [f[k][1] for k in ("frame", "body_len", "body_size", "transport_id", "content_type", "name_len", "au", "repeat")] + \
        [128] + [g[k][1] for k in ("objects_lost", "crc_bad", "progress_pct", "transport_id", "segments_stored", "active")] + \
        [32, 4, 128, t["rec_off"][1], t["objects"][1], t["progress_events"][1], 128, dx.CHUNK_HEADER.fields["off_mot"][1], dx.DELIVER_MOT, 6], got
    assert got[1:9] == [8, 16, 20, 24, 26, 28, 30, 31] and got[-3] == 112 and dx.MOT_OBJECT.names[0] == "byte_pos"


def test_the_model_on_hand_made_groups():
    """The rules that are easy to get wrong, on groups small enough to check by eye."""
    rng = np.random.default_rng(7)
    segs = [bytes([k]) * (10 + k) for k in range(4)]

    def run(groups, **kw):
        rec, by = mc.items_of(groups)
        return mc.run_model(rec, by, **kw)
    B = lambda tid, k, last=False, **kw: mc.msc_group(4, segs[k], tid, k, last, rng=rng, **kw)      # noqa: E731
    H = lambda tid, size, params=(), **kw: mc.msc_group(3, mc.mot_header(size, params, **kw), tid, rng=rng)      # noqa: E731
    # the body is the map in key order whatever the order of arrival, the name follows it; contentType 2 / subtype 0x101: 0x0201
    m = run([B(5, 2, True), B(5, 0), H(5, 33, [mc.name_param(b"a.jpg")], subtype=0x101), B(5, 1)])
    assert len(m.rows) == 1 and m.payloads[0] == segs[0] + segs[1] + segs[2] + b"a.jpg"
    assert m.rows[0] == (0, 5, 33, 33, 5, 0x0201, 5, 0, 0), m.rows
    assert m.progress == [100] and m.counters["transport_id"] == 5 and m.counters["segments_stored"] == 3
    # nothing is cleared after the emit: every further header emits again, a further segment too (and is part of the object)
    m = run([H(5, 21), B(5, 0), B(5, 1, True), H(5, 21), B(5, 3), H(5, 21)])
    assert [r[8] for r in m.rows] == [0, 1, 2, 3] and [r[2] for r in m.rows] == [21, 21, 34, 34] and m.payloads[2] == segs[0] + segs[1] + segs[3]
    assert m.progress[-1] == 100 and m.branch["mo:165 progress clamped"] == 1
    # a new transport id resets; the id of a header is taken even when the segment numbers then do not fit
    m = run([H(5, 21), B(5, 0), B(6, 1, True), H(6, 11)])
    assert not m.rows and m.counters["resets"] == 2 and m.counters["segments_stored"] == 1
    # content type 0x3f / subtype 0x1ff are cut to the masks of get_content_type
    m = run([H(9, 10, content_type=0x3F, subtype=0x1FF), B(9, 0, True)])
    assert m.rows[0][5] == 0x3FFF and m.rows[0][6] == 0 and not m.progress
    # M3 keeps the transport id: the next segment of the same id does not reset again
    m = run([B(9, 0), B(9, 1), B(9, 2)], max_object_bytes=21)
    assert m.counters["obj_overflow"] == 1 and m.counters["resets"] == 2 and m.counters["segments_stored"] == 0 and m.counters["transport_id"] == 9
    m = run([B(9, 0), B(9, 1)], max_object_bytes=21)
    assert m.counters["obj_overflow"] == 0 and m.branch["M3 exactly max_object_bytes"] == 1
    # the transport id is read behind the length byte whatever the length indicator says: with 0 it is the segmentation header
    g = mc.msc_group(4, segs[0], 0x1234, 0, True, li=0, rng=rng)
    m = run([g])
    assert m.counters["transport_id"] == (g[5] << 8 | g[6]) and (g[6], len(g)) == (10, 4 + 1 + 2 + 10 + 2) and m.counters["segments"] == 1


def test_the_scenarios_reach_every_branch_and_each_side_of_every_guard():
    branch = collections.Counter()
    for s, j in _slots():
        m = _model(s, j)
        branch.update(m.branch)
        assert len(m.rows) >= 15 and all(0 <= p <= 100 for p in m.progress), (s, j, len(m.rows))
    missing = [k for k in COVERAGE if not branch[k]]
    assert not missing, missing
    unlisted = [k for k in branch if k not in COVERAGE]
    assert not unlisted, unlisted
    # objects of a few segments of 20 .. 200 bytes, one of 3 000 bytes
    m = _model(0, 0)
    assert 3000 in m.records()["body_len"] and m.records()["repeat"].max() == 3 and set(m.records()["name_len"]) >= {0, 7, 12}


def test_every_crafted_group_travels_through_the_x_pad_unchanged_and_the_long_object_takes_several_batches():
    """PadHandler's restatement on the super frames the builder makes hands on exactly the crafted groups, in order, CRC verdicts included;
    MotModel on those items gives the objects of MotModel on the groups themselves."""
    for s, j in _slots():
        frames, sfs, sfi = mc.mot_frames(s, j)
        assert frames.shape == (mc.N_FRAMES, 3 * mc.STAGE_LAYOUT[j][0])
        pm = mc.pad_model_of(sfs, sfi)
        rows = pm.records()
        assert pm.counters["pad_bad"] == 0 and pm.counters["li_bad"] == 0 and pm.counters["dg_small"] == 0
        groups = mc.groups_only(mc.slot_groups(s, j))
        assert [p for p, r in zip(pm.payloads, rows) if r["kind"] == dx.PAD_DATAGROUP] == groups, (s, j)
        a, b = mc.mot_model_of(pm, mc.max_bytes_of(j)), _model(s, j)
        assert a.payloads == b.payloads and a.counters == b.counters and [r[2:7] for r in a.rows] == [r[2:7] for r in b.rows], (s, j)
        if j == 0:
            big = [g for g in groups if len(g) == 131 and g[0] & 0x0F == 4]      # header 2, segment field 2, user access 3, size 2, 120, CRC 2
            first = [int(r["frame"]) for p, r in zip(pm.payloads, rows) if p == big[0]][0]
            done = int(a.records()["frame"][a.records()["body_len"] == 3000][0])
            assert len(big) == 25 and done - first > 2 * mc.BATCH, (first, done)
