"""No device: the packet-mode model and scenarios of tests/packet_cases.py on their own -- that the committed scenarios reach every branch of
DataProcessor (data_processor.cpp:123-254) and both guards, that the model's packet CRC is the reference's check_CRC_bits, that the FIB
decoder returns the FIG 0/3 + FIG 0/2 (TMId 3) the synthesiser built, and that both library forms export the new entry points.  The GPU
tests (test_gpu_packet_stage.py) compare the device with this model on exactly these scenarios."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import packet_cases as pc
from dabstar_amd import lib as dx
from tools import dab_synth as ds

NEW_SYMBOLS = ("dabx_set_packet_mode", "dabx_read_datagroups", "dabx_get_packet_stats", "dabx_fibdec_packet_components")


def _models():
    return [(kbps, seed, address, pc.run_model(pc.scenario(kbps, seed), address)) for kbps, seed, address in pc.all_scenarios()]


def test_new_symbols_are_declared_and_exported_in_both_library_forms():
    assert set(NEW_SYMBOLS) <= set(dx.declared_symbols())
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


def test_records_have_their_documented_sizes(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(dabx_datagroup_info), offsetof(dabx_datagroup_info, length), offsetof(dabx_datagroup_info, crc_ok),
         sizeof(dabx_packet_stats), offsetof(dabx_packet_stats, dg_lost), sizeof(dabx_packet_config), sizeof(dabx_packet_component), DABX_DG_MAX_BYTES);
  return 0;
}
""")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    f, g = dx.DATAGROUP_INFO.fields, dx.PACKET_STATS.fields
    assert got == [32, f["length"][1], f["crc_ok"][1], 128, g["dg_lost"][1], C.sizeof(dx.PacketConfig), dx.PACKET_COMPONENT.itemsize, dx.DG_MAX_BYTES]
    assert got[1] == 24 and got[2] == 27 and got[5] == 32 and got[7] == 16384 and dx.Engine.set_packet_mode and dx.Engine.read_datagroups


def test_the_model_on_hand_made_frames():
    """The rules that are easy to get wrong, on frames small enough to check by eye."""
    A = pc.ADDRESS_A
    P = lambda ci, fl, payload, **kw: pc.packet(0, ci, fl, A, payload, **kw)      # noqa: E731
    # a mismatch sets the expected index to 0 (not to index + 1); the index advances before the CRC is looked at
    m = pc.run_model([P(0, 3, b"a"), P(2, 3, b"b"), P(3, 3, b"c"), P(0, 3, b"d", good=False), P(1, 3, b"e")], A)
    assert m.groups == [b"a", b"e"] and m.counters["continuity_err"] == 2 and m.counters["crc_bad"] == 1
    # single inside a series: the series is abandoned, the single packet is not emitted
    m = pc.run_model([P(0, 2, b"ab"), P(1, 3, b"cd"), P(2, 1, b"ef"), P(3, 3, b"gh")], A)
    assert m.groups == [b"gh"] and m.branch["single_in_series"] == 1 and m.branch["orphan_fl1"] == 1
    # a bad CRC leaves the assembly as it was; first inside a series restarts it; records count frames and bytes
    m = pc.run_model([P(0, 2, b"ab") + P(1, 0, b"xx", good=False), P(2, 0, b"cd"), P(3, 2, b"\x40\x00"), P(0, 1, b"ef")], A)
    assert m.groups == [b"\x40\x00ef"] and m.records().tolist() == [(0, 2, 3, 4, 1, 0, 0)]
    g = pc.data_group(np.random.default_rng(1), 9, True)
    m = pc.run_model([P(0, 2, g[:5]), P(1, 1, g[5:])], A)
    assert m.records().tolist() == [(0, 0, 1, 9, 1, 1, 0)] and m.counters["dg_crc_bad"] == 0
    # useful length beyond the packet: delivered while inside the frame, dropped (state unchanged) when it passes the frame's end
    f = P(0, 3, b"z" * 19, ulen=30) + P(1, 3, b"q")
    m = pc.run_model([f], A)
    assert m.groups == [f[3:33], b"q"] and m.counters["len_bad"] == 0
    m = pc.run_model([P(0, 2, b"s") + P(1, 0, b"z" * 19, ulen=22), P(2, 1, b"t")], A)
    assert m.groups == [b"st"] and m.counters["len_bad"] == 1
    # a length code that overruns the frame ends the walk; another address is not looked at
    m = pc.run_model([P(0, 3, b"a") + pc.packet(1, 1, 3, A, b"b")[:24], pc.packet(0, 0, 3, 7, b"x") + P(1, 3, b"c")], A)
    assert m.groups == [b"a", b"c"] and m.counters["walk_short"] == 1 and m.counters["packets"] == 3 and m.counters["addr_match"] == 2


def test_the_scenarios_reach_every_branch_and_both_guards():
    runs = _models()
    assert sorted({k for k, _, _, _ in runs}) == pc.RATES
    branch, counters = collections.Counter(), collections.Counter()
    for _, _, _, m in runs:
        branch.update(m.branch)
        counters.update(m.counters)
    print(sorted(branch.items()), dict(counters))
    for k in pc.PACKET_COUNTERS:
        assert counters[k] > 0, k
    for k in ("first", "single", "orphan_fl0", "orphan_fl1", "intermediate", "last", "first_in_series", "single_in_series",      # the two tables
              "crc_bad_fl0", "crc_bad_fl1", "crc_bad_fl2", "crc_bad_fl3", "accepted_after_break_ci0", "padding", "other_address",
              "ulen0", "beyond_packet_inside_frame", "series_at_bound",
              "dg_empty", "dg_flag_len1", "dg_crc_ok", "dg_crc_bad", "dg_no_flag", "dg_over_frames", "dg_4096_and_more"):
        assert branch[k] > 0, k
    lengths = sorted({len(g) for _, _, _, m in runs for g in m.groups})
    assert lengths[0] == 0 and lengths[1] == 1 and lengths[-1] == 8191 and {4095, 4096} <= set(lengths), lengths
    # every run that is read with address A shows both guards' neighbours: a dropped and a repeated packet, bad CRCs, the short walk
    for kbps, seed, address, m in runs:
        if address == pc.ADDRESS_A:
            assert m.counters["continuity_err"] and m.counters["crc_bad"] == 4 and m.counters["len_bad"] == 1 and m.counters["walk_short"], (kbps, seed)
            assert kbps < 16 or m.branch["beyond_packet_inside_frame"], (kbps, seed)
        assert m.counters["dg_count"] > 0 and len(m.all_bytes()) == m.counters["dg_bytes"], (kbps, seed)
    # packets of all four lengths, walked and accepted
    codes = collections.Counter()
    for kbps, seed, _ in pc.all_scenarios():
        for f in pc.scenario(kbps, seed):
            f, at = f.tobytes(), 0
            while at < len(f) and at + ((f[at] >> 6) + 1) * 24 <= len(f):
                codes[f[at] >> 6] += 1
                at += ((f[at] >> 6) + 1) * 24
    assert all(codes[c] > 100 for c in range(4)), codes


def test_groups_span_the_batch_boundaries_of_the_boundary_schedule_and_idle_batches():
    """With the schedule of the batch-boundary test (0, 1, 4 ... 28 CIFs per batch) series are open at batch ends -- the device must carry
    expected index, state, fill, CRC register and first frame from launch to launch -- and across batches in which a stream receives nothing."""
    sched = pc.boundary_schedule(len(pc.STAGE_STREAMS))
    assert {c for row in sched for c in row} >= {0, 1, 4, 5, 6, 13, 27, 28}
    spans = idle_spans = 0
    for s, (lay, address) in enumerate(pc.STAGE_STREAMS):
        ends, idle_at, at = set(), set(), 0
        for row in sched:
            if row[s] == 0 and 0 < at < pc.N_FRAMES:
                idle_at.add(at)
            at += row[s]
            ends.add(at)
        for j, (kbps, kind) in enumerate(pc.STAGE_LAYOUTS[lay]):
            if kind != "pkt":
                continue
            r = pc.run_model(pc.scenario(kbps, pc.seed_of(s, j)), address).records()
            for e in ends:
                spans += int(((r["first_frame"] < e) & (r["last_frame"] >= e)).sum())
            for e in idle_at:
                idle_spans += int(((r["first_frame"] < e) & (r["last_frame"] >= e)).sum())
    assert spans > 20 and idle_spans > 0, (spans, idle_spans)


def test_the_late_reader_scenarios_overrun_the_rings_the_way_each_is_meant_to():
    """The model and the documented window rule alone on the three scenarios of test_gpu_ring_reads.py: A loses groups to the record ring, B
    to the byte ring alone, C to the byte ring with the surviving bytes across the ring's end.  A change of seed cannot hollow that test out."""
    seen = {}
    for name in pc.LATE_READER:
        kbps, frames = pc.late_reader_scenario(name)
        m = pc.run_model(frames, pc.ADDRESS_A)
        r, n_bytes = m.records(), m.counters["dg_bytes"]
        c = m.counters
        assert c["frames"] == pc.N_FRAMES and c["packets"] == c["addr_match"] and len(r) == c["dg_count"], (name, c)         # everything is valid
        assert not any(c[k] for k in ("continuity_err", "crc_bad", "len_bad", "walk_short", "dg_crc_bad", "dg_overflow")), (name, c)
        n_rec, n_ring = pc.ring_sizes(kbps)
        by_records, first = pc.intact_window(r["byte_pos"], n_bytes, n_rec, n_ring)
        base = int(r["byte_pos"][first])
        seen[name] = (len(r), n_bytes, n_rec, n_ring, by_records, first, base % n_ring + (n_bytes - base) > n_ring)
    print(seen)
    n, _, n_rec, _, by_records, first, _ = seen["A"]
    assert (n, n_rec, by_records, first) == (112, 64, 48, 48) and first % n_rec + (n - first) > n_rec      # the records come in two runs
    n, _, n_rec, _, by_records, first, _ = seen["B"]
    assert n < n_rec and by_records == 0 and 0 < first < n
    n, n_bytes, n_rec, n_ring, by_records, first, crosses = seen["C"]
    assert n < n_rec and by_records == 0 and 0 < first < n and n_bytes > n_ring and crosses


def test_packet_crc_of_the_model_is_the_references_check_crc_bits():
    if not ol.have_ref():
        pytest.skip("oracle/_ref is not built")
    R = ol.ref()
    n = bad = 0
    for f in pc.scenario(64, pc.seed_of(3, 1)):
        f, at = f.tobytes(), 0
        while at < len(f) and at + ((f[at] >> 6) + 1) * 24 <= len(f):
            pkt = f[at:at + ((f[at] >> 6) + 1) * 24]
            bits = np.ascontiguousarray(np.unpackbits(np.frombuffer(pkt, np.uint8)))
            want = bool(R.ref_check_crc_bits(bits, int(bits.size)))
            assert pc.packet_crc_ok(pkt) == want, (n, at)
            n += 1
            bad += not want
            at += len(pkt)
    assert n > 300 and 0 < bad < n


def test_fib_decoder_returns_fig_0_3_joined_with_fig_0_2_for_both_configurations():
    """FIG 0/3 with and without the CAOrg field, repeated, for the current and the next configuration (C/N flag); the SId from the FIG 0/2
    service whose TMId-3 component names the SCId (fib_decoder.cpp:362-411); the first description of an SCId wins."""
    cur = [(0x123, 5, 0x155, 59, 0, None), (0x7FF, 9, 0x2AA, 5, 1, 0xBEEF), (0x001, 63, 0x3FF, 60, 0, None)]
    nxt = [(0x123, 6, 0x011, 59, 0, 0x1234), (0x222, 7, 0x001, 24, 0, None)]
    late = [(0x7FF, 10, 0x111, 6, 0, 0x0001), (0x456, 11, 0x045, 60, 1, None)]           # 0x7FF again with other contents (ignored), then a new one
    figs = [ds.fig00_bytes(100), ds.fig03_bytes(cur), ds.fig02_packet_bytes([(0x4001, [0x123, 0x001]), (0x4002, [0x7FF])]),
            ds.fig03_bytes(nxt, cn=1), ds.fig02_packet_bytes([(0xE1C00001, [0x222])], cn=1, pd=1), ds.fig03_bytes(cur),
            ds.fig03_bytes(late), ds.fig03_bytes(nxt, cn=1)]
    d = dx.FibDecoder()
    try:
        fibs = np.concatenate([ds.pack_fibs(figs[:4]), ds.pack_fibs(figs[4:])]).reshape(-1, 32)
        d.process(fibs, np.ones(len(fibs), np.uint8))
        got = d.packet_components()
        assert [tuple(int(v) for v in r) for r in got] == [(0x123, 5, 0x155, 59, 0, 0x4001), (0x7FF, 9, 0x2AA, 5, 1, 0x4002), (0x001, 63, 0x3FF, 60, 0, 0x4001),
                                                          (0x456, 11, 0x045, 60, 1, 0)], got
        got = d.packet_components(next=True)
        assert [tuple(int(v) for v in r) for r in got] == [(0x123, 6, 0x011, 59, 0, 0), (0x222, 7, 0x001, 24, 0, 0xE1C00001)], got
        assert d.subchannels() == [] and d.info()["cif_count"] == 100
    finally:
        d.close()
