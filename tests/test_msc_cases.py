"""No device needed: the ground test_gpu_msc_decoder.py stands on (tests/msc_cases.py).  The profile list, the layouts, the coverage
facts about the oracle's depuncture maps, and -- through the oracle back end alone -- that the generator, the puncturing and the
de-interleaver placement of the TEST are right before a GPU is involved."""
import numpy as np

import msc_cases as mc
import oracle_lib as ol


def test_the_profile_list_has_304_entries_and_21_padded_uep_rows():
    P = mc.legal_profiles()
    assert len(P) == 48 * 4 + 12 * 4 + 64 == 304 and len(set(P)) == 304
    padded = [p for p in P if not mc.lane_per_trellis_capable(p)]
    # the UEP rows whose coded bits leave 4 .. 20 padding bits in the last capacity unit: k_msc_prep cannot take them (whole 64-bit
    # units only), build_msc_classes leaves them to k_msc_frame -- 283 profiles can be a lane-per-trellis class
    assert len(padded) == 21 and all(p[2] == 1 for p in padded)
    assert all(4 <= 64 * mc.cu_size(p) - mc.oracle_map(p)[0] <= 20 for p in padded)
    assert sum(mc.oracle_map(p)[0] // 64 for p in P) == 48506 and sum(mc.cu_size(p) for p in P) == 48506 + 21


def test_layouts_are_legal_and_give_every_profile_a_class_slot():
    P = mc.legal_profiles()
    for part in ([p for p in P if mc.lane_per_trellis_capable(p)], [p for p in P if not mc.lane_per_trellis_capable(p)]):
        layouts = mc.pack_layouts(part)
        seen = []
        for lay in layouts:
            assert 1 <= len(lay) <= mc.MAX_CLASSES
            assert len({mc.profile_of(c) for c in lay}) == len(lay)               # distinct profiles: one class each
            at = 0
            for c in lay:
                assert c.cu_start == at and c.cu_size == mc.cu_size(mc.profile_of(c)) and c.dab_plus == 0
                assert c.cu_size * 64 >= mc.oracle_map(mc.profile_of(c))[0] > (c.cu_size - 1) * 64
                at += c.cu_size
            assert at <= 864
            seen += [mc.profile_of(c) for c in lay]
        assert sorted(seen) == sorted(part)
    assert len(mc.pack_layouts([p for p in P if mc.lane_per_trellis_capable(p)])) <= 60


def test_coverage_facts_of_the_oracles_depuncture_maps():
    """16 byte-lane patterns and 96 (step class, pattern) combinations, over all profiles and over those k_msc_vitT can take; every
    residue of cu_size % 16 (k_msc_prep's partial last chunk) among the latter; the identity map of dabx_internal_vitT shows 6."""
    P = mc.legal_profiles()
    fast = [p for p in P if mc.lane_per_trellis_capable(p)]
    for part in (P, fast):
        combos = set().union(*[mc.lane_patterns(p) for p in part])
        assert len(combos) == 96 and len({c for _, c in combos}) == 16
    assert {mc.cu_size(p) % 16 for p in fast} == set(range(16))
    identity = 0 + 5 * 1 + 25 * 2 + 125 * 3
    assert sum(1 for _, c in set().union(*[mc.lane_patterns(p) for p in fast]) if c == identity) == 6
    cover = mc.greedy_cover(fast)
    assert set().union(*[mc.lane_patterns(p) for p in cover]) == set().union(*[mc.lane_patterns(p) for p in fast])
    assert {mc.cu_size(p) % 16 for p in cover} == set(range(16)) and max(p[0] for p in cover) == 384
    assert len(cover) <= 2 * mc.MAX_CLASSES


def test_every_slot_sees_every_input_class_within_a_batch():
    for s in range(3):
        for j in range(mc.MAX_CLASSES):
            assert {mc.class_of(s, r, j) for r in range(mc.HISTORY, mc.HISTORY + mc.BATCH)} == set(range(len(mc.CLASSES)))


def test_coded_frames_come_back_from_the_oracle_back_end():
    """EEP 1-A and 2-A (rates 1/4 and 3/8) at amplitude 60, sigma 40: every frame of the coded class is the transmitted message, so
    conv_encode, the puncturing by the oracle's map, the energy dispersal and the placement into 16 CIFs are what the receiver undoes.
    (3-A and weaker lose frames at this noise; there the class gives the decoder a trellis it is losing, which is wanted.)"""
    rng = np.random.default_rng(20260)
    layout = mc.layout_of([(64, 0, 0), (64, 1, 0), (8, 0, 0), (24, 1, 0)])
    n_frames = 40
    n_cifs = mc.HISTORY + n_frames
    cifs = rng.integers(-127, 128, (n_cifs, mc.CIF_BITS)).astype(np.int16)
    msgs = {}
    for j, sc in enumerate(layout):
        for k in range(n_frames):
            soft, msgs[(j, k)] = mc.coded_frame(rng, mc.profile_of(sc))
            for m in range(16):
                cifs[k + mc.BITREV4[m], sc.cu_start * 64 + m:(sc.cu_start + sc.cu_size) * 64:16] = soft[m::16]
    out = mc.oracle_frames(layout, cifs)
    for j, sc in enumerate(layout):
        assert out[j].shape == (n_frames, 3 * sc.kbps)
        for k in range(n_frames):
            assert np.array_equal(np.unpackbits(out[j][k]), msgs[(j, k)]), (mc.profile_of(sc), k)


def test_stream_cifs_places_every_frame_where_the_de_interleaver_looks():
    """The class schedule of stream_cifs, read back through the oracle: the all-zero, +127 and -127 frames decode to what ora_deconvolve
    gives for that constant input, in exactly the frames the schedule names (any misplacement mixes noise into them)."""
    layout = mc.layout_of([(32, 2, 0), (48, 3, 1), (8, 1, 0)])
    cifs, names = mc.stream_cifs(layout, 1, mc.HISTORY + mc.BATCH, seed=7)
    out = mc.oracle_frames(layout, cifs)
    hits = 0
    for j, sc in enumerate(layout):
        n_in, m = mc.oracle_map(mc.profile_of(sc))
        prbs = np.zeros(24 * sc.kbps, np.uint8)
        ol.oracle().ora_prbs(prbs, 24 * sc.kbps)
        for name, v in (("zero", 0), ("plus127", 127), ("minus127", -127)):
            want = np.zeros(24 * sc.kbps, np.uint8)
            ol.oracle().ora_deconvolve(np.full(n_in, v, np.int16), m, sc.kbps, want)
            for r in range(mc.HISTORY, mc.HISTORY + mc.BATCH):
                if names[(j, r)] == name:
                    assert np.array_equal(np.unpackbits(out[j][r - mc.HISTORY]), want ^ prbs), (j, r, name)
                    hits += 1
    assert hits >= 3 * 3 * 2
