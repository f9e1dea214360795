"""The batched MSC decoder proper -- k_msc_prep + k_msc_vitT (vit_t.hip) as dabx_process launches them -- on adversarial soft bits,
against the oracle back end (oracle/msc.c), for every legal protection profile.

The soft bits go straight into the engine's time-de-interleaver ring (dx.msc_inject / dx.msc_decode: the library's internal test
entries, no IQ, no front end), so the decoder sees exact ties, saturated and out-of-range symbols, pure noise and codes it cannot
decode -- input on which a Viterbi decoder does NOT correct a fault in its own input path, unlike the >= 15 dB demapper output of
the engine tests.  Generators, layouts and the coverage facts: tests/msc_cases.py, proven on the CPU in tests/test_msc_cases.py.
Every comparison is np.array_equal on logical-frame bytes and on cifs_decoded; the oracle is the only reference."""
import numpy as np
import pytest

import msc_cases as mc
from dabstar_amd import lib as dx
from stage_driver import engine, kernel_launches

pytestmark = pytest.mark.gpu

H, B = mc.HISTORY, mc.BATCH
E_ARG = -2                          # DABX_E_ARG (include/dabx.h)


def _history_then_one_batch(eng, cifs):
    """16 CIFs of history for every stream (their batch decodes nothing: no logical frame exists yet), then one full batch."""
    S = len(cifs)
    for s in range(S):
        dx.msc_inject(eng, s, cifs[s][:H])
    dx.msc_decode(eng, [H] * S, H)
    for s in range(S):
        dx.msc_inject(eng, s, cifs[s][H:H + B])
    dx.msc_decode(eng, [B] * S, B)


def _compare(eng, s, layout, want, names, n=B, first=0):
    """Mismatches of stream s: its newest n logical frames of every slot against the oracle's frames first .. first + n."""
    bad = []
    eng.subch = list(layout)
    for j, sc in enumerate(layout):
        if sc.kbps == 0:
            continue
        got = eng.read_msc(s, j, n)
        st = eng.subch_stats(s, j)
        if st["cifs_decoded"] != first + n or got.shape[0] != n:
            bad.append((mc.profile_of(sc), s, "cifs_decoded", st["cifs_decoded"], got.shape[0]))
            continue
        for k in range(n):
            if not np.array_equal(got[k], want[j][first + k]):
                bad.append((mc.profile_of(sc), s, H + first + k, names.get((j, H + first + k))))
    return bad


def _run_layout(layout, n_streams, seed, tie_mode=0, expect_vitT=True):
    """One engine, the layout on every stream, every stream its own data: (mismatches, per stream the input-class names and
    the CIFs).  Asserts which decoder ran."""
    data = [mc.stream_cifs(layout, s, H + B, seed) for s in range(n_streams)]
    eng = engine(n_streams, len(layout), tie_mode=tie_mode)
    try:
        eng.set_subchannels(layout, dab_plus=False)
        _history_then_one_batch(eng, [d[0] for d in data])
        launches = kernel_launches(eng)
        if expect_vitT:      # every slot is a lane-per-trellis class: nothing may fall back to the wave-per-trellis kernel
            assert launches["k_msc_vitT"] == 2 and launches["k_msc_prep"] == 2 and launches["k_msc_frame"] == 0, launches
        else:                # the padded UEP rows: k_msc_frame is the only kernel that takes them
            assert launches["k_msc_vitT"] == 0 and launches["k_msc_prep"] == 0 and launches["k_msc_frame"] == 2, launches
        bad = []
        for s in range(n_streams):
            bad += _compare(eng, s, layout, mc.oracle_frames(layout, data[s][0], tie_mode), data[s][1])
        return bad, data
    finally:
        eng.close()


def test_every_legal_profile_on_adversarial_soft_bits_matches_the_oracle_back_end():
    """All 304 profiles, canonical arithmetic.  Three streams share a layout of at most 16 distinct profiles (one decoder class
    each), so every class has 3 x 28 = 84 jobs in the batch: a full wave and a partly filled one.  Per (stream, slot) the 28 logical
    frames walk through the ten input classes of msc_cases.CLASSES.  283 profiles are decoded by k_msc_prep + k_msc_vitT (asserted:
    k_msc_frame does not run); the 21 UEP rows with padding bits cannot be a lane-per-trellis class (build_msc_classes) and are
    checked on k_msc_frame, so that no legal profile is left out."""
    P = mc.legal_profiles()
    assert len(P) == 304
    fast = [p for p in P if mc.lane_per_trellis_capable(p)]
    padded = [p for p in P if not mc.lane_per_trellis_capable(p)]
    assert len(fast) == 283 and len(padded) == 21
    bad, seen, classes_seen = [], [], {}
    for part, vitT in ((fast, True), (padded, False)):
        for li, layout in enumerate(mc.pack_layouts(part)):
            b, data = _run_layout(layout, 3, seed=1000 + li + (0 if vitT else 500), expect_vitT=vitT)
            bad += b
            seen += [mc.profile_of(c) for c in layout]
            for _, names in data:
                for (j, _r), name in names.items():
                    classes_seen.setdefault(mc.profile_of(layout[j]), set()).add(name)
    assert sorted(seen) == sorted(P)
    assert all(classes_seen[p] == {c[0] for c in mc.CLASSES} for p in P)
    assert not bad, (len(bad), bad[:20])


def test_the_three_viterbi_arithmetics_on_every_byte_lane_pattern_and_chunk_residue():
    """viterbi_tie_mode 1 / 2 (k_msc_vitT_avx2 / _sse2) on a subset computed from the oracle's maps that still shows all 96 (step
    class, byte-lane pattern) combinations, all 16 residues of cu_size % 16 and the longest trellis (384 kbit/s: dozens of
    renormalisations).  Non-vacuity on the oracle side: on the tie-maker frames the AVX2 arithmetic (ties to the i + 32 path) differs
    from both others.  The SSE2 arithmetic keeps the scalar tie rule and differs from the canonical one only by its saturating symbol
    conversion and metric saturation: measured with the oracle on these very inputs, 0 tie-maker frames differ between modes 0 and 2
    (and 0 of 640 in-range random frames at 384 and 128 kbit/s), so for that pair the difference is demanded of the out-of-range int16
    frames (`int16_edges`), where the conversions differ."""
    fast = [p for p in mc.legal_profiles() if mc.lane_per_trellis_capable(p)]
    cover = mc.greedy_cover(fast)
    assert set().union(*[mc.lane_patterns(p) for p in cover]) == set().union(*[mc.lane_patterns(p) for p in fast])
    assert len(set().union(*[mc.lane_patterns(p) for p in cover])) == 96
    assert {mc.cu_size(p) % 16 for p in cover} == set(range(16)) and (384, 0, 0) in cover
    layouts = mc.pack_layouts(cover)
    differ = {(0, 1): 0, (0, 2): 0, (1, 2): 0}
    differ_edges = 0
    bad = []
    for mode in (1, 2):
        for li, layout in enumerate(layouts):
            b, data = _run_layout(layout, 3, seed=2000 + li, tie_mode=mode)
            bad += [(mode,) + x for x in b]
            if mode == 1:
                for cifs, names in data:
                    o = [mc.oracle_frames(layout, cifs, m) for m in range(3)]
                    for (j, r), name in names.items():
                        for a, c in differ:
                            ne = not np.array_equal(o[a][j][r - H], o[c][j][r - H])
                            if name in mc.TIE_MAKERS:
                                differ[(a, c)] += ne
                            elif name == "int16_edges" and (a, c) == (0, 2):
                                differ_edges += ne
    print("oracle: tie-maker frames that differ between the modes", differ, "; int16_edges frames, modes 0 / 2:", differ_edges)
    assert differ[(0, 1)] > 0 and differ[(1, 2)] > 0 and differ_edges > 0
    assert not bad, (len(bad), bad[:20])


def test_lanes_with_nothing_to_decode_leave_the_outputs_alone():
    """Per-stream CIF counts that differ inside one batch (0, a few, all), a stream with an inactive sub-channel slot, and a second
    batch behind the first (the other inT buffer and snapshot: batch_parity): the valid jobs equal the oracle, a stream that received
    nothing keeps its logical frames and cifs_decoded."""
    layout = mc.layout_of([(64, 2, 0), (8, 1, 0), (48, 5, 1), (32, 6, 0), (24, 3, 0)])
    assert {c.cu_size % 16 for c in layout} - {0} and all(mc.lane_per_trellis_capable(mc.profile_of(c)) for c in layout)
    gap = list(layout)
    gap[1] = mc.ds.SubCh(1, 0, 0, 0, dab_plus=0)                       # stream 4: slot 1 not configured
    S = 6
    lays = [gap if s == 4 else layout for s in range(S)]
    counts = [[B, 0, 5, B, 13, 27], [B, B, 23, 0, 15, 1]]
    total = [H + counts[0][s] + counts[1][s] for s in range(S)]
    data = [mc.stream_cifs(lays[s], s, total[s], 3000) for s in range(S)]
    want = [mc.oracle_frames(lays[s], data[s][0]) for s in range(S)]
    eng = engine(S, len(layout))
    try:
        for s in range(S):
            eng.set_subchannels(lays[s], stream=s, dab_plus=False)
        for s in range(S):
            dx.msc_inject(eng, s, data[s][0][:H])
        dx.msc_decode(eng, [H] * S, H)
        at = [H] * S
        snapshots = []
        for batch in range(2):
            for s in range(S):
                if counts[batch][s]:
                    dx.msc_inject(eng, s, data[s][0][at[s]:at[s] + counts[batch][s]])
            dx.msc_decode(eng, counts[batch], B)
            bad = []
            for s in range(S):
                at[s] += counts[batch][s]
                done = at[s] - H
                if done == 0:
                    eng.subch = list(lays[s])
                    for j, sc in enumerate(lays[s]):
                        if sc.kbps:
                            assert eng.read_msc(s, j, B).shape[0] == 0 and eng.subch_stats(s, j)["cifs_decoded"] == 0, (batch, s, j)
                else:
                    n = min(done, B)
                    bad += _compare(eng, s, lays[s], want[s], data[s][1], n=n, first=done - n)
            assert not bad, (batch, len(bad), bad[:20])
            eng.subch = list(layout)
            snapshots.append({(s, j): (eng.read_msc(s, j, B).copy(), eng.subch_stats(s, j)) for s in range(S) for j in range(len(layout))})
        # stream 3 received nothing in the second batch: byte for byte what it had
        for j in range(len(layout)):
            assert np.array_equal(snapshots[0][(3, j)][0], snapshots[1][(3, j)][0]) and snapshots[0][(3, j)][1] == snapshots[1][(3, j)][1]
        # the slot that is not configured stays empty
        assert eng.subch_stats(4, 1)["active"] == 0 and eng.subch_stats(4, 1)["cifs_decoded"] == 0
        launches = kernel_launches(eng)
        assert launches["k_msc_vitT"] == 3 and launches["k_msc_prep"] == 3 and launches["k_msc_frame"] == 0, launches
    finally:
        eng.close()


def test_more_than_one_round_of_decoder_groups():
    """150 streams x 16 small profiles x 28 CIFs = 16 classes of 66 groups each, 1056 decoder groups in one launch: the groups of the
    second round of 1024 are walked backwards (msc_vitT_body, ROUND).  Every job of every stream is compared."""
    fast = [p for p in mc.legal_profiles() if mc.lane_per_trellis_capable(p)]
    small = sorted(fast, key=lambda p: (p[0], mc.cu_size(p), p))[:mc.MAX_CLASSES]
    layout = mc.layout_of(small)
    S = 150
    per_class = -(-S * B // 64)
    assert len(layout) * per_class > 1024
    # stream s is lane (k * S + s) % 64 of group (k * S + s) // 64 of every class; all classes have per_class groups, so the last one
    # (whichever profile that is) starts at group 15 * per_class and its groups from 1024 on are the reversed round: every stream
    # has jobs on both sides
    for s in (0, S // 2, S - 1):
        rounds = {((len(layout) - 1) * per_class + (k * S + s) // 64) // 1024 for k in range(B)}
        assert rounds == {0, 1}
    eng = engine(S, len(layout))
    try:
        eng.set_subchannels(layout, dab_plus=False)
        keep = []
        for s in range(S):
            cifs, names = mc.stream_cifs(layout, s, H + B, 4000)
            dx.msc_inject(eng, s, cifs[:H])
            keep.append((cifs, names))
        dx.msc_decode(eng, [H] * S, H)
        for s in range(S):
            dx.msc_inject(eng, s, keep[s][0][H:])
        dx.msc_decode(eng, [B] * S, B)
        launches = kernel_launches(eng)
        assert launches["k_msc_vitT"] == 2 and launches["k_msc_frame"] == 0, launches
        bad = []
        for s in range(S):
            bad += _compare(eng, s, layout, mc.oracle_frames(layout, keep[s][0]), keep[s][1])
        assert not bad, (len(bad), bad[:20])
    finally:
        eng.close()


def test_both_decoders_share_a_batch_and_agree():
    """Six streams carry four profiles, stream 0 four more: with msc_class_min_jobs = 84 the classes of six pairs (168 jobs) go
    lane-per-trellis and the four of one pair (28 jobs) stay on k_msc_frame in the same batch.  Each of three engines -- mixed, all
    lane-per-trellis, all wave-per-trellis -- equals the oracle; then they equal each other."""
    common = [(64, 2, 0), (16, 0, 0), (32, 3, 1), (96, 5, 0)]
    extra = [(8, 3, 0), (40, 1, 0), (48, 4, 1), (32, 7, 0)]
    full = mc.layout_of(common + extra)
    part = [c if i < len(common) else mc.ds.SubCh(i, 0, 0, 0, dab_plus=0) for i, c in enumerate(full)]
    S = 6
    lays = [full if s == 0 else part for s in range(S)]
    data = [mc.stream_cifs(lays[s], s, H + B, 5000) for s in range(S)]
    want = [mc.oracle_frames(lays[s], data[s][0]) for s in range(S)]
    outputs = []
    for fast_min, class_min, vitT, frame in ((1, 84, True, True), (1, 1, True, False), (1 << 30, 1, False, True)):
        eng = engine(S, len(full), fast_min=fast_min, class_min=class_min)
        try:
            for s in range(S):
                eng.set_subchannels(lays[s], stream=s, dab_plus=False)
            _history_then_one_batch(eng, [d[0] for d in data])
            launches = kernel_launches(eng)
            assert (launches["k_msc_vitT"] > 0) == vitT and (launches["k_msc_frame"] > 0) == frame, launches
            bad = []
            for s in range(S):
                bad += _compare(eng, s, lays[s], want[s], data[s][1])
            assert not bad, ((fast_min, class_min), len(bad), bad[:20])
            eng.subch = list(full)
            outputs.append([eng.read_msc(s, j, B) for s in range(S) for j in range(len(full))])
        finally:
            eng.close()
    for other in outputs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outputs[0], other))


def test_the_injection_entries_refuse_what_would_leave_the_ring():
    eng = engine(2, 2)
    try:
        eng.set_subchannels(mc.layout_of([(8, 1, 0), (16, 2, 0)]), dab_plus=False)
        soft = np.zeros((B + 1, mc.CIF_BITS), np.int16)
        L = dx.load()
        bad_inject = [(2, B, 0), (-1, 1, 0), (0, B + 1, 0), (0, 0, 0), (0, -3, 0), (0, 1, B), (0, B, 1), (0, 2, -1), (0, 1, 1 << 30), (0, 1 << 30, 0)]
        for stream, n, first in bad_inject:
            assert L.dabx_internal_msc_inject(eng._h, stream, dx._p(soft), n, first) == E_ARG, (stream, n, first)
        assert L.dabx_internal_msc_inject(eng._h, 0, None, 1, 0) == E_ARG
        for counts, batch in (([1, 1], 0), ([1, 1], B + 1), ([B + 1, 0], B), ([0, -1], B), ([5, 4], 4), ([1, 1], -2)):
            c = np.asarray(counts, np.int32)
            assert L.dabx_internal_msc_decode(eng._h, dx._p(c), batch) == E_ARG, (counts, batch)
        assert L.dabx_internal_msc_decode(eng._h, None, B) == E_ARG
        # nothing of that moved a counter or produced a frame
        dx.msc_decode(eng, [0, 0], 1)
        assert eng.subch_stats(0, 0)["cifs_decoded"] == 0 and eng.stats(0)["cifs_decoded"] == 0
    finally:
        eng.close()
