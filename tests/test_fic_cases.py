"""No device needed: the ground test_gpu_fic_stage.py stands on (tests/fic_cases.py).  The model of the CIF-counter rule against
oracle/fic.c (run for real through ora_fic_process_block) and against the library's own walk (csrc/fig00.h through
dabx_internal_fib_cif_count), FIB by FIB; the coverage of the schedules; and, on the oracle alone, that the inputs decide what they are
meant to decide: tie modes that differ, ties, both stops of the success ratio, halved BER counters."""
import ctypes as C

import numpy as np

import fic_cases as fc
import oracle_lib as ol
from dabstar_amd import lib as dx

# crafted cases on which the walk meets a FIG 0/0 header at byte 27, 28 or 29: oracle/fic.c (as the reference) reads the neighbour's bits
LATE_GROUP = {"header_at_27", "header_at_28", "header_at_29", "fig00_then_zeros", "all_zero", "zeros_then_bytes"}
# crafted cases on which dabx_parse_fibs (walk_fib == oracle/fib.c: stops at a FIG that runs past byte 30, FIG 0/0 needs length >= 5)
# reports another counter than the model: name -> (model, dabx_parse_fibs), -1 = none
STRICT_WALK_DIFFERS = {
    "fig00_length_0": (1770, -1), "fig00_length_1": (3557, -1), "fig00_length_2": (344, -1), "fig00_length_3": (2131, -1),
    "fig00_length_4": (3918, -1), "fig00_length_4_then_fig": (2316, -1), "fig00_runs_past_30": (2492, -1), "header_at_25": (2658, -1),
    "header_at_26": (6529, -1), "fig00_then_zeros": (4485, 1171), "all_zero": (5436, -1), "zeros_then_bytes": (1650, -1),
}


def _count(m):
    return -1 if m is None else m[0] * 250 + m[1]


def oracle_counters(fibs):
    """[(counter oracle/fic.c reads out of the FIB alone, -1 = none; its CRC verdict)].  Every FIB is the middle one of a block whose
    other two are fillers; three of them per frame, in blocks 0, 1 and 3, so that each is the only news of one ora_fic_process_block."""
    L = ol.oracle()
    f = fc.OraFic()
    L.ora_fic_init(C.byref(f))
    filler = fc.coded_block([fc.FILLER] * 3)
    out = []
    for i in range(0, len(fibs), 3):
        grp = list(fibs[i:i + 3]) + [fc.FILLER] * (3 - len(fibs[i:i + 3]))
        b = [fc.coded_block([fc.FILLER, g, fc.FILLER]) for g in grp]
        frame = np.concatenate([b[0], b[1], filler, b[2]])
        for sym, at in ((1, 1), (2, 4), (3, 10)):
            f.cif_count = -1
            L.ora_fic_process_block(C.byref(f), np.ascontiguousarray(frame[(sym - 1) * fc.K2:sym * fc.K2]), sym)
            out.append((f.cif_count, int(f.fib_crc[at])))
        assert all(f.fib_crc[k] for k in range(12) if k not in (1, 4, 10))      # the fillers around them
    return out[:len(fibs)]


def test_the_ctypes_picture_of_ora_fic_is_the_structs():
    f = fc.OraFic()
    assert C.sizeof(f) < 40000
    ol.oracle().ora_fic_init(C.byref(f))
    n_in, m = ol.ora_fic_map()
    prbs = np.zeros(768, np.uint8)
    ol.oracle().ora_prbs(prbs, 768)
    assert np.array_equal(np.frombuffer(f.map, np.int32), m) and np.array_equal(np.frombuffer(f.prbs, np.uint8), prbs)
    assert np.array_equal(np.frombuffer(f.punct, np.uint8), (m >= 0).astype(np.uint8)) and f.success_ratio == 0 and f.cif_count == 0


def test_the_model_is_the_oracle_and_the_library_fib_by_fib():
    """Model == library (csrc/fig00.h) on EVERY case; model == oracle/fic.c on every case whose walk meets no FIG 0/0 header at byte 27 or
    later: all crafted cases outside LATE_GROUP and at least 90 % of the 2000 random FIBs.  The late group is listed with both values."""
    crafted = fc.crafted_singles() + fc.NO_FIG00 + [("later_fib_wins_%d" % i, f) for i, f in enumerate(fc.later_fib_wins_blocks())]
    names = [n for n, _ in crafted] + ["random_%d" % i for i in range(2000)] + ["sparse_%d" % i for i in range(1000)]
    fibs = [f for _, f in crafted] + fc.random_fibs() + fc.sparse_fibs()
    assert len(fc.random_fibs()) == 2000 and len(set(names)) == len(names)
    bad = [fc.broken(f) for _, f in fc.crafted_singles()]
    ora = oracle_counters(fibs + bad)
    comparable = {"crafted": 0, "random": 0, "sparse": 0}
    late = []
    for name, fib, (cif, crc) in zip(names, fibs, ora):
        good = fc.crc_good(fib)
        assert crc == good, name
        m = fc.model_fig00(fib)
        assert dx.fib_cif_count(fib) == m, (name, m)                    # the library's walk is the model, late headers included
        if not good:                                                    # (the middle FIBs of the 'later FIB wins' blocks)
            assert cif == -1, name
            continue
        if fc.reaches_late_fig00(fib):
            late.append((name, _count(m), cif))
            continue
        assert cif == _count(m), (name, cif, m)
        comparable[name.split("_")[0] if name.split("_")[0] in ("random", "sparse") else "crafted"] += 1
    for (name, fib), (cif, crc) in zip(fc.crafted_singles(), ora[len(fibs):]):
        assert crc == 0 and cif == -1, name                             # a broken CRC changes nothing
    print("comparable with oracle/fic.c:", comparable, "of", len(crafted), "+ 2000 + 1000")
    print("FIG 0/0 header at byte 27 or later (name, model, oracle/fic.c with filler FIBs around it):")
    for row in late:
        if not row[0].startswith(("random", "sparse")):
            print("   ", row)
    print("    and %d of the random, %d of the thinned random FIBs" % (sum(r[0].startswith("random") for r in late), sum(r[0].startswith("sparse") for r in late)))
    assert {n for n, _, _ in late if not n.startswith(("random", "sparse"))} == LATE_GROUP
    assert comparable["crafted"] == len(crafted) - len(LATE_GROUP) - 2 and comparable["random"] >= 1800
    by = {n: (m, o) for n, m, o in late}
    for p in (27, 28, 29):                                              # the model ignores what the reference reads out of the next FIB
        assert by["header_at_%d" % p][0] == -1 and by["header_at_%d" % p][1] >= 0
    assert all(by[n][0] != by[n][1] for n in ("fig00_then_zeros", "all_zero", "zeros_then_bytes"))
    with_counter = sum(fc.model_fig00(f) is not None for f in fc.sparse_fibs())
    assert with_counter >= 500, with_counter


def test_where_the_strict_walk_of_dabx_parse_fibs_tells_another_counter():
    """walk_fib (dabx_fibdec, dabx_parse_fibs) and oracle/fib.c agree with each other everywhere and with the model on every well-formed
    case; the table names the crafted cases on which they do not follow the model."""
    one = np.ones(1, np.uint8)
    differs = {}
    for name, fib in fc.crafted_singles() + fc.NO_FIG00:
        strict = dx.parse_fibs(fib[None], one)[1]
        d = ol.OraFibDecoder()
        d.process(fib[None], one)
        assert d.info()["cif_count"] == strict, name
        d.close()
        if strict != _count(fc.model_fig00(fib)):
            differs[name] = (_count(fc.model_fig00(fib)), strict)
    print("dabx_parse_fibs differs from the model on (name: model, strict):", differs)
    assert differs == STRICT_WALK_DIFFERS


def test_every_class_meets_every_block_position_and_every_crafted_fib_is_carried():
    seen = set()
    for s in range(fc.N_STREAMS):
        n = fc.stream_frames_count(s)
        assert n >= 21
        for kinds in fc.block_kinds(s, n):
            seen |= {(k, b) for b, k in enumerate(kinds)}
        assert {(k, b) for k in fc.CLASS_NAMES for b in range(4)} == {(k, b) for kinds in fc.block_kinds(s, n) for b, k in enumerate(kinds)}
    assert seen == {(k, b) for k in fc.CLASS_NAMES for b in range(4)} and len(fc.CLASS_NAMES) == 11
    carried = [np.stack(fc.crafted_sequence(s)[:12 * len(range(0, fc.stream_frames_count(s), fc.CARRIER_EVERY))]) for s in range(fc.N_STREAMS)]
    good = np.concatenate(carried[:3])
    mixed = np.concatenate(carried[3:])
    for name, fib in fc.crafted_singles():
        assert (good == fib).all(1).any() and (mixed == fib).all(1).any(), name
        assert (mixed == fc.broken(fib)).all(1).any() and not (good == fc.broken(fib)).all(1).any(), name
    wins = np.stack(fc.later_fib_wins_blocks())
    assert np.array_equal(carried[0][:6], wins)                        # aligned to two blocks of stream 0's first frame
    assert all((carried[1][12:24] == f).all(1).any() for _, f in fc.NO_FIG00) and not any(fc.model_fig00(f) for f in carried[1][12:24])


def _blocks_differ(a, b, kinds, names=None):
    n = 0
    for f, (ra, rb) in enumerate(zip(a, b)):
        for blk in range(4):
            if (names is None or kinds[f][blk] in names) and not np.array_equal(ra["fibs"][3 * blk:3 * blk + 3], rb["fibs"][3 * blk:3 * blk + 3]):
                n += 1
    return n


def test_on_the_oracle_alone_the_inputs_decide_what_they_are_meant_to():
    differ01 = differ02_edges = ties = wrap_frames = edges_blocks = wrap_blocks = cif_frames = 0
    stops, longest = set(), {0: 0, 1: 0}
    mixed_blocks = 0
    for s in range(fc.N_STREAMS):
        soft, kinds = fc.stream_frames(s)
        r0, r1, r2 = (fc.oracle_stream(s, mode) for mode in (0, 1, 2))
        differ01 += _blocks_differ(r0, r1, kinds)
        differ02_edges += _blocks_differ(r0, r2, kinds, ("int16_edges",))
        # modes 1 and 2 convert alike (saturating) and these classes stay far from any metric saturation within 774 steps: a block that
        # differs between them holds a tie that their two tie rules decided differently
        ties += _blocks_differ(r1, r2, kinds, fc.TIE_MAKERS)
        edges_blocks += sum(k.count("int16_edges") for k in kinds)
        wrap_blocks += sum(r["wrap_blocks"] for r in fc.oracle_calls(fc.symbol_calls(soft), 0))
        wrap_frames += sum(r["ber"] != r["ber_wrap"] for r in r0)
        for mode, recs in enumerate((r0, r1, r2)):
            assert all(r["ber"] == r["ber_wrap"] for r in recs) or mode == 0
            assert recs[-1]["ber"][0] == ((40 * 2304 // 2 + 40 * 2304) // 2 + (4 * len(recs) - 80) * 2304)      # halved twice
        run = {0: 0, 1: 0}
        late_seen = False
        for f, r in enumerate(r0):
            stops.add(r["ratio"])
            for blk in range(4):
                v = r["crc"][3 * blk:3 * blk + 3]
                mixed_blocks += 0 < v.sum() < 3
            for fib, ok in zip(r["fibs"], r["crc"]):
                run[int(ok)] += 1
                run[1 - int(ok)] = 0
                longest[int(ok)] = max(longest[int(ok)], run[int(ok)])
                late_seen = late_seen or (bool(ok) and fc.reaches_late_fig00(fib))
            if not late_seen:                       # until the stream's first late header the oracle's counter IS the model's
                assert r["cif"] == r["cif_model"], (s, f)
                cif_frames += 1
    print("blocks that differ, modes 0/1:", differ01, " int16_edges blocks, modes 0/2:", differ02_edges, " tie-maker blocks, modes 1/2:", ties)
    print("int16_edges blocks:", edges_blocks, " frames whose BER pair the wrap changes:", wrap_frames, " mixed-verdict blocks:", mixed_blocks,
          " longest runs bad/good:", longest, " frames with counter == oracle's:", cif_frames)
    assert differ01 >= 1 and differ02_edges >= 1 and ties >= 1
    assert {0, 10} <= stops and longest[0] >= 11 and longest[1] >= 11 and mixed_blocks >= 1
    assert wrap_blocks == edges_blocks > 0 and wrap_frames >= 1
    assert cif_frames >= 21
