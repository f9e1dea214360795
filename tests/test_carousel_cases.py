"""No device: the carousel model and scenarios of tests/carousel_cases.py on their own -- that the committed scenarios reach every branch of
mot_handler.cpp:69-259 and mot_dir.cpp:28-156 and each side of the guards C1..C3, D1..D4 (a coverage table keyed by reference line), that
they stay within what the rings and a chunk of the bulk delivery hold, that the rules that are easy to get wrong hold on groups small
enough to check by eye, that a stream of one object at a time gives what the X-PAD's MotObject gives, and that the new entry points are
declared and exported with the record layouts include/dabx.h states.  The GPU tests compare the device with this model on exactly these
scenarios."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import carousel_cases as cc
import mot_cases as mc
import packet_cases as pkc
from dabstar_amd import lib as dx

NEW_SYMBOLS = ("dabx_set_carousel_mode", "dabx_get_carousel_stats")

# every branch of the restatement and each side of every guard, by reference line (mh: mot_handler.cpp, md: mot_dir.cpp, mo: mot_object.cpp)
COVERAGE = (
    "mh:88 empty group", "mh:93 bad CRC", "mh:91 good CRC", "mh:91 no CRC flag", "mh:96 extension flag 0", "mh:96 extension flag 1",
    "mh:101 segment field", "mh:101 no segment field", "mh:108 no user access field", "mh:115 transport id, length indicator 0",
    "mh:115 transport id, length indicator 2", "mh:115 transport id, length indicator 15", "mh:115 transport id, length indicator other",
    "mh:124 no transport id", "mh:143 header segment 1", "mh:148 header for a known id", "mh:161 object made from a body segment",
    "mh:179 segment 0 of the directory there is", "mh:184 the old directory is deleted", "mh:200 directory segment without its directory",
    "mh:206 type 0", "mh:218 handle in the cache", "mh:218 handle in the cache, and in the directory", "mh:226 no handle",
    "mh:233 a free entry", "mh:255 the oldest entry is evicted",
    "md:55 analysed at construction", "md:73 handle in the directory", "md:87 no component free: not registered",
    "md:103 directory segment already marked", "md:112 number of directory segments unknown", "md:115 a directory segment is missing",
    "md:117 all segments in: analysed", "md:117 all segments in: analysed again", "md:132 the walk ends at numObjects",
    "md:136 a zero id ends the walk", "md:150 directory object registered",
    "C1 segment field", "C1 user access field", "C1 transport id", "C1 payload of 1 byte", "C1 payload of no byte",
    "C1 payload of less than no byte", "C1 segment ends exactly at the payload's end", "C1 segment one byte beyond the payload",
    "C1 segment beyond the payload",
    "C2 segment of 6 bytes", "C2 segment of fewer than 6 bytes", "C2 segment of 7 bytes", "C2 parameter byte beyond the segment",
    "C2 length byte beyond the segment", "C2 second length byte beyond the segment", "C2 name one byte beyond the segment",
    "C2 name beyond the segment", "C2 name ends exactly at the segment's end",
    "C3 exactly max_object_bytes", "C3 one byte beyond max_object_bytes", "C3 beyond max_object_bytes",
    "D1 segment 0 of 12 bytes", "D1 segment 0 of 13 bytes", "D2 dirSize beyond max_dir_bytes", "D2 dirSize exactly max_dir_bytes",
    "D2 numObjects beyond max_dir_objects", "D2 numObjects exactly max_dir_objects", "D3 segment 0 clipped to dirSize",
    "D3 directory segment 511", "D3 directory segment 512", "D3 directory segment above 512", "D3 copy ends exactly at dirSize",
    "D3 copy one byte beyond dirSize", "D3 copy beyond dirSize", "D4 extension length beyond dirSize", "D4 entry id beyond dirSize",
    "D4 header core beyond dirSize", "D4 header core ends exactly at dirSize",
    "mo:75 transport id changes at a header", "mo:106 pointer == headerSize", "mo:106 pointer != headerSize", "mo:111 header",
    "mo:119 segment number 8191", "mo:121 segment number 8192", "mo:121 segment number above 8192", "mo:141 duplicate segment",
    "mo:147 last flag", "mo:160 no PAD element: no progress", "mo:182 ContentName", "mo:201 parameter whose value is walked",
    "mo:204 unknown parameter", "mo:219 PLI 0", "mo:219 PLI 1", "mo:219 PLI 2", "mo:230 PLI 3, 7-bit length", "mo:225 PLI 3, 15-bit length",
    "mo:244 no header core", "mo:250 number of segments unknown", "mo:256 fewer segments than needed",
    "mo:288 a segment numbered beyond the last is emitted", "mo:293 no name", "mo:300 with a name", "mo:300 emit, repeat 0",
    "mo:300 emit, repeat 1", "mo:300 dirElement 0", "mo:300 dirElement 1", "mo:313 reset",
)

def _models():
    for s in range(cc.N_STREAMS):
        for name in cc.SCENARIOS:
            kbps, groups, frames, cfg = cc.scenario(name, s)
            yield s, name, kbps, groups, frames, cfg


def test_new_symbols_are_declared_and_exported_in_both_library_forms_and_the_records_have_their_layout(tmp_path):
    assert set(NEW_SYMBOLS) <= set(dx.declared_symbols())
    assert dx.CAROUSEL_STATS.itemsize == 128 and C.sizeof(dx.CarouselConfig) == 32 and dx.MOT_FLAG_DIR_ELEMENT == 1
    assert dx.Engine.set_carousel_mode and dx.Engine.carousel_stats and len(dx.CAROUSEL_COUNTERS) == 27
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
    fields = [k for k in dx.CAROUSEL_STATS.names]
    src = tmp_path / "t.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void) {
  printf("%%zu %%zu %%zu %%zu %%zu %%d %%d %%d ", sizeof(dabx_carousel_config), offsetof(dabx_carousel_config, max_object_bytes),
         offsetof(dabx_carousel_config, max_dir_objects), offsetof(dabx_carousel_config, max_dir_bytes), sizeof(dabx_carousel_stats),
         DABX_MOT_FLAG_DIR_ELEMENT, DABX_MAX_KERNELS, DABX_ABI_VERSION);
%s
  printf("\\n");
  return 0;
}
""" % "\n".join('  printf("%%zu ", offsetof(dabx_carousel_stats, %s));' % k for k in fields))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    g = dx.CAROUSEL_STATS.fields
    cfg = dx.CarouselConfig
    assert got == [32, cfg.max_object_bytes.offset, cfg.max_dir_objects.offset, cfg.max_dir_bytes.offset, 128, dx.MOT_FLAG_DIR_ELEMENT, 16, 6] + \
        [g[k][1] for k in fields], got
    assert got[1:4] == [4, 8, 12] and g["groups"][1] == 24 and g["active"][1] == 124


def test_the_model_on_hand_made_groups():
    """The rules that are easy to get wrong, on groups small enough to check by eye."""
    rng = np.random.default_rng(7)
    segs = [bytes([k]) * (10 + k) for k in range(4)]

    def run(groups, **kw):
        rec, by = cc.items_of(groups)
        return cc.run_model(rec, by, **kw)
    B = lambda tid, k, last=False, **kw: cc.msc_group(4, segs[k], tid, k, last, rng=rng, **kw)      # noqa: E731
    H = lambda tid, size, params=(), **kw: cc.msc_group(3, cc.mot_header(size, params, **kw), tid, rng=rng)      # noqa: E731
    D = lambda tid, k, seg, last=False: cc.msc_group(6, seg, tid, k, last, rng=rng)      # noqa: E731
    # two objects whose segments interleave both complete; the body is the map in key order, the name follows; frame = the group's last_frame
    m = run([H(5, 21, [cc.name_param(b"a.jpg")]), H(6, 23), B(5, 1, True), B(6, 2, True), B(6, 0), B(5, 0), B(6, 1)])
    assert m.payloads == [segs[0] + segs[1] + b"a.jpg", segs[0] + segs[1] + segs[2]]
    assert m.rows == [(0, 5, 21, 21, 5, 0x0201, 5, 0, 0), (26, 6, 33, 23, 6, 0x0201, 0, 0, 0)], m.rows
    # the next cycle emits nothing: headers of known ids are ignored, segments are duplicates
    m = run(2 * [H(5, 21), B(5, 0), B(5, 1, True)])
    assert len(m.rows) == 1 and m.counters["hdr_known"] == 1 and m.counters["seg_duplicate"] == 2
    # a body segment for an unknown id is read as the header -- 0x00 * 10: bodySize 0, headerSize 0 -- and a later header changes nothing
    m = run([B(7, 0), H(7, 21, [cc.name_param(b"late")]), B(7, 1, True)])
    assert m.rows == [(0, 2, 21, 0, 7, 0, 0, 0, 0)] and m.counters["from_body"] == 1 and m.counters["hdr_known"] == 1 and m.counters["headers"] == 1
    # sixteen ids: the first is evicted, a segment for it makes a new object, which evicts the second
    m = run([H(100 + k, 10) for k in range(16)] + [B(100, 0, True), H(101, 10)])
    assert m.counters["evictions"] == 3 and m.counters["from_body"] == 1 and m.counters["hdr_known"] == 0 and len(m.rows) == 1
    assert sorted(e[1] for e in m.cache.values()) == [100, 101] + list(range(103, 116))
    # a directory in one segment; its objects carry flag bit 0; an id of the cache wins over the directory's
    d = cc.directory([(8, cc.mot_header(10)), (9, cc.mot_header(11, [cc.name_param(b"nine")]))])
    m = run([H(8, 10), D(50, 0, d, True), B(8, 0, True), B(9, 1, True), B(9, 0)])
    assert [(r[4], r[7]) for r in m.rows] == [(8, 0), (9, cc.MOT_FLAG_DIR_ELEMENT)] and m.payloads[1] == segs[0] + segs[1] + b"nine"
    assert m.counters["dir_objects"] == 2 and m.counters["dirs_begun"] == 1
    # ... in two segments, the second first: dropped, there is no directory yet; a new directory deletes the objects of the old one
    k = len(d) // 2
    m = run([D(50, 1, d[k:], True), D(50, 0, d[:k]), D(50, 1, d[k:], True), B(9, 0), D(51, 0, cc.directory([])), B(9, 1, True)])
    assert m.counters["dir_segments"] == 3 and m.counters["dir_objects"] == 2 and m.counters["from_body"] == 1 and m.counters["dirs_begun"] == 2
    assert not m.rows and m.dir["tid"] == 51


def test_the_scenarios_reach_every_branch_and_each_side_of_every_guard():
    branch = collections.Counter()
    for s, name, kbps, groups, frames, cfg in _models():
        rec, by = cc.items_of(groups)
        m = cc.run_model(rec, by, **cfg)
        branch.update(m.branch)
        assert len(m.rows) >= 8, (s, name, len(m.rows))
    missing = [k for k in COVERAGE if not branch[k]]
    assert not missing, missing
    unlisted = [k for k in branch if k not in COVERAGE]
    assert not unlisted, unlisted
    m = cc.run_model(*cc.items_of(cc.scenario("header")[1]), **cc.scenario("header")[3])
    assert m.counters["evictions"] >= 2 and 1 in m.records()["repeat"] and 4096 in m.records()["body_len"]
    m = cc.run_model(*cc.items_of(cc.scenario("directory")[1]), **cc.scenario("directory")[3])
    assert set(m.records()["au"]) == {0, 1} and m.counters["dirs_begun"] >= 10


def test_the_packets_carry_every_crafted_group_unchanged_and_the_scenarios_stay_within_the_rings_and_a_chunk():
    """DataProcessor's restatement on the logical frames the builder makes hands on exactly the crafted groups, in order, CRC verdicts
    included; no batch overruns the packet slot's rings (dg_lost == 0 before a device is involved) or emits more than the 256 records of the
    object ring, and no window of 32 logical frames emits more than a chunk of the delivery holds: 16 objects, 2 * max_object_bytes
    bytes.  So objects_lost == 0 is a condition the reference side meets."""
    for s, name, kbps, groups, frames, cfg in _models():
        assert frames.shape == (cc.N_FRAMES, 3 * kbps)
        pm = pkc.run_model(frames, cc.ADDRESS)
        assert pm.groups == [bytes(g) for g in groups], (s, name)
        c = pm.counters
        assert c["crc_bad"] == c["len_bad"] == c["continuity_err"] == c["dg_overflow"] == c["walk_short"] == 0, c
        a, b = cc.model_of(pm, **cfg), cc.run_model(*cc.items_of(groups), **cfg)
        assert a.payloads == b.payloads and a.counters == b.counters and [r[2:] for r in a.rows] == [r[2:] for r in b.rows], (s, name)
        rows = pm.records()
        ring_records, ring_bytes = pkc.ring_sizes(kbps)
        for bt in range(cc.N_BATCHES):
            in_batch = rows[(rows["last_frame"] >= bt * cc.BATCH) & (rows["last_frame"] < (bt + 1) * cc.BATCH)]
            assert len(in_batch) <= ring_records and int(in_batch["length"].sum()) + dx.DG_MAX_BYTES <= ring_bytes, (s, name, bt)
            assert sum(bt * cc.BATCH <= f < (bt + 1) * cc.BATCH for f in a.emissions) <= 256
        room = 2 * a.max_object_bytes
        for f0 in range(cc.N_FRAMES):
            inside = [len(p) for f, p in zip(a.emissions, a.payloads) if f0 <= f < f0 + cc.WINDOW]
            assert len(inside) <= cc.CHUNK_OBJECTS and sum(inside) <= room, (s, name, f0, inside)


def test_one_object_at_a_time_header_first_gives_what_the_x_pad_object_gives():
    """A stream that sends one object at a time, header first, each id once: the handler's objects have the bodies, names and header fields
    of mot_cases.MotModel -- the X-PAD's single MotObject -- on the same groups."""
    s = cc.Groups(5)
    s.obj(1, [50, 60, 70], [cc.name_param(b"first.jpg")])
    s.obj(2, [200], [cc.name_param(b"second.png", long=True), cc.param(0x30, s.rand(9))])
    s.obj(3, [20, 21], crc=False)
    s.obj(4, [1024, 1024, 100], [cc.param(0x25, b"\x07", pli=1), cc.name_param(b"fourth")])
    a = cc.run_model(*cc.items_of(s.out))
    b = mc.run_model(*mc.items_of(s.out))
    assert len(a.rows) == 4 and a.payloads == b.payloads
    assert [r[2:7] + r[8:] for r in a.rows] == [r[2:7] + r[8:] for r in b.rows]
    for k in ("headers", "segments", "resets", "hdr_bad", "seg_duplicate", "obj_overflow", "objects", "object_bytes"):
        assert a.counters[k] == b.counters[k], k
