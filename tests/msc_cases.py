"""Shared by test_msc_cases.py (no device) and test_gpu_msc_decoder.py: the legal protection profiles, their packing into
sub-channel layouts, the adversarial soft-bit classes, and the placement of chosen logical frames into CIFs so that the
16-CIF time de-interleaver reassembles them.  Everything that is compared comes from the oracle (oracle/msc.c)."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as ol

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

CIF_BITS = 55296
HISTORY = 16                       # CIFs the de-interleaver needs before its first logical frame (backend.cpp:146-150)
BATCH = 28                         # CIFs of one full MSC batch (4 * MSC_BATCH_FRAMES)
MAX_CLASSES = 16                   # DABX_MSC_FAST_CLASSES
BITREV4 = [0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15]      # backend.cpp:129

_maps = {}


def legal_profiles():
    """(kbps, prot_level, short_form) of EN 300 401 11.3 exactly as test_deconvolve_every_legal_profile_matches_oracle lists them."""
    profiles = [(k, p, 0) for k in range(8, 385, 8) for p in range(8) if p < 4 or k % 32 == 0]
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_leaf_vectors.npz"))
    profiles += [(int(k), int(l), 1) for _, l, k in G["uep_table"].tolist()]
    return profiles


def oracle_map(profile):
    """(n_in, depuncture map of 4 * (24 kbps + 6) entries, -1 = punctured) from the oracle."""
    if profile not in _maps:
        kbps, prot, short = profile
        n_in, m = (ol.ora_uep_map if short else ol.ora_eep_map)(kbps, prot)
        assert n_in > 0, profile
        _maps[profile] = (n_in, m)
    return _maps[profile]


def cu_size(profile):
    """Capacity units of the sub-channel: 64 bits each; 21 UEP rows end in 4 .. 20 padding bits (EN 300 401 11.3.1)."""
    return -(-oracle_map(profile)[0] // 64)


def lane_per_trellis_capable(profile):
    """k_msc_prep moves whole 64-bit capacity units: a profile whose coded bits do not fill its last one (the padded UEP rows) never
    becomes a lane-per-trellis class (engine.cpp, build_msc_classes) and stays with k_msc_frame."""
    return oracle_map(profile)[0] % 64 == 0


def lane_patterns(profile):
    """The (step class t % 6, byte-lane pattern) pairs the profile's map makes k_msc_vitT's pick() / bm0..bm5 see: per trellis step the
    byte lane (index & 3) of each of its four symbols, 4 for a punctured one."""
    _, m = oracle_map(profile)
    q = m.reshape(-1, 4)
    lanes = np.where(q >= 0, q & 3, 4)
    code = lanes[:, 0] + 5 * lanes[:, 1] + 25 * lanes[:, 2] + 125 * lanes[:, 3]
    t6 = np.arange(len(q)) % 6
    return set(zip(t6.tolist(), code.tolist()))


def pack_layouts(profiles, max_per_layout=MAX_CLASSES, capacity=864):
    """First-fit decreasing: lists of ds.SubCh (dab_plus = 0, cu_size exactly n_in / 64), non-overlapping, <= 864 CU and at most
    max_per_layout distinct profiles each."""
    bins = []
    for p in sorted(profiles, key=lambda p: (-cu_size(p), p)):
        for b in bins:
            if len(b) < max_per_layout and sum(cu_size(q) for q in b) + cu_size(p) <= capacity:
                b.append(p)
                break
        else:
            bins.append([p])
    return [layout_of(b) for b in bins]


def layout_of(profiles):
    out, at = [], 0
    for i, p in enumerate(profiles):
        out.append(ds.SubCh(i, at, cu_size(p), p[0], p[1], p[2], dab_plus=0))
        at += cu_size(p)
    assert at <= 864
    return out


def profile_of(sc):
    return (sc.kbps, sc.prot_level, sc.short_form)


# ---- input classes: one logical frame's worth (n_in soft bits, as the de-interleaver hands them to the decoder) ---------------------
def coded_frame(rng, profile, msg=None):
    """A random message (returned), energy-dispersed, convolutionally encoded, punctured with the oracle's own map: amplitude 60,
    Gaussian sigma 40 (test_viterbi_encoded_noise's figures)."""
    kbps = profile[0]
    n_in, m = oracle_map(profile)
    nbits = 24 * kbps
    if msg is None:
        msg = rng.integers(0, 2, nbits).astype(np.uint8)
    prbs = np.zeros(nbits, np.uint8)
    ol.oracle().ora_prbs(prbs, nbits)
    code = ds.conv_encode(msg ^ prbs).astype(np.int16)
    soft = np.zeros(n_in, np.float64)
    tx = m >= 0
    soft[m[tx]] = (2 * code[tx] - 1) * 60
    return (soft + rng.normal(0, 40, n_in)).astype(np.int16), msg


def _padded(rng, v, n):
    """v followed by noise up to n soft bits (the padding bits of a UEP sub-channel's last capacity unit)."""
    return np.concatenate([v, rng.integers(-127, 128, n - len(v)).astype(np.int16)])


CLASSES = [
    ("noise", lambda rng, p, n: rng.integers(-127, 128, n)),
    ("coded", lambda rng, p, n: _padded(rng, coded_frame(rng, p)[0], n)),
    ("zero", lambda rng, p, n: np.zeros(n)),
    ("plus127", lambda rng, p, n: np.full(n, 127)),
    ("minus127", lambda rng, p, n: np.full(n, -127)),
    ("ternary", lambda rng, p, n: rng.choice([-1, 0, 1], n)),
    ("sign127", lambda rng, p, n: rng.choice([-127, 127], n)),
    ("int16_edges", lambda rng, p, n: rng.choice([-32768, -32767, 32767, 32640, 32641, -200, 200], n)),      # test_gpu_viterbi._cases
    ("byte_edges", lambda rng, p, n: rng.choice([-127, 0, 127, 128, -128, 1, -1], n)),
    ("wide", lambda rng, p, n: rng.integers(-200, 201, n)),
]
TIE_MAKERS = ("zero", "plus127", "minus127", "ternary", "sign127")


def class_of(s, r, j, n_classes=len(CLASSES)):
    """Input class of logical frame r of sub-channel slot j of stream s: 28 consecutive frames of any slot see every class."""
    return (r + 3 * s + 5 * j) % n_classes


def stream_cifs(layout, s, n_cifs, seed, classes=None):
    """[n_cifs, 55296] int16 for stream s: every logical frame r >= 16 of every sub-channel is a frame of class_of(s, r, slot), placed so
    that the de-interleaver reassembles it (frame r takes bit i from CIF r - 16 + bitrev4(i & 15)); everything else is uniform noise,
    different in every CIF.  Returns (cifs, {(slot, r): class name})."""
    rng = np.random.default_rng([seed, s])
    cifs = rng.integers(-127, 128, (n_cifs, CIF_BITS)).astype(np.int16)
    names = {}
    cls = CLASSES if classes is None else [c for c in CLASSES if c[0] in classes]
    for j, sc in enumerate(layout):
        if sc.kbps == 0:
            continue
        p, n_in, base = profile_of(sc), sc.cu_size * 64, sc.cu_start * 64
        nfr = n_cifs - HISTORY
        T = np.zeros((nfr, n_in), np.int16)
        for k in range(nfr):
            name, gen = cls[class_of(s, HISTORY + k, j, len(cls))]
            names[(j, HISTORY + k)] = name
            T[k] = np.asarray(gen(rng, p, n_in)).astype(np.int16)
        for m in range(16):
            cifs[BITREV4[m]:BITREV4[m] + nfr, base + m:base + n_in:16] = T[:, m::16]
    return cifs, names


def oracle_frames(layout, cifs, tie_mode=0, threads=8):
    """Per slot of the layout: the oracle back end's logical frames [n_cifs - 16, 3 kbps] for one stream's CIFs (None: empty slot)."""
    def one(sc):
        if sc.kbps == 0:
            return None
        b = ol.OraBackend(sc.cu_size, sc.kbps, sc.prot_level, sc.short_form, sc.cu_start, sc.subch_id)
        try:
            for c in range(cifs.shape[0]):
                b.push(cifs[c, sc.cu_start * 64:(sc.cu_start + sc.cu_size) * 64])
            out = b.msc_frames()
            assert b.stats()["cif_out"] == out.shape[0] == max(0, cifs.shape[0] - HISTORY)
            return out
        finally:
            b.close()
    ol.oracle().ora_set_viterbi_mode(tie_mode)
    try:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            return list(ex.map(one, layout))
    finally:
        ol.oracle().ora_set_viterbi_mode(0)


def greedy_cover(profiles):
    """Profiles that together show every (step class, byte-lane pattern) pair and every residue of cu_size % 16 the given ones show,
    plus the longest trellis; computed from the oracle's maps."""
    pats = {p: lane_patterns(p) for p in profiles}
    need = set().union(*pats.values())
    chosen = []
    while need:
        best = max(profiles, key=lambda p: (len(pats[p] & need), -cu_size(p)))
        chosen.append(best)
        need -= pats[best]
    res = {cu_size(p) % 16 for p in profiles} - {cu_size(p) % 16 for p in chosen}
    for r in sorted(res):
        chosen.append(min((p for p in profiles if cu_size(p) % 16 == r), key=lambda p: (cu_size(p), p)))
    longest = max(profiles, key=lambda p: (p[0], cu_size(p)))
    if not any(p[0] == longest[0] for p in chosen):
        chosen.append(longest)
    return chosen
