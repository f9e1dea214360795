"""Shared by test_dabplus_cases.py (no device) and test_gpu_dabplus_stage.py: adversarial DAB+ super frames for every bit rate, their
arrangement into logical-frame scenarios (junk in front, slips, a decoy header), noise-free coded soft bits for them, and the oracle
back end's verdicts (oracle/msc.c).  The role tests/msc_cases.py has for the Viterbi decoder, one stage further down: the soft bits
decode to exactly the intended bytes (proven in test_dabplus_cases.py), so everything here is aimed at k_dabplus -- the super-frame
sync state machine, RS(120,110), the fire code, the AU table and the AU CRCs."""
import binascii
import dataclasses
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import msc_cases as mc
import oracle_lib as ol
from msc_cases import BATCH, BITREV4, HISTORY, layout_of, oracle_map, pack_layouts  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from dabstar_amd.lib import SUPERFRAME_INFO  # noqa: E402

CIF_BITS = mc.CIF_BITS
PROT = 3                                    # EEP 4-A: the weakest A level packs densest (4 CU per 8 kbit/s), every rate 8 .. 384 is legal
RATES = list(range(8, 385, 8))              # R = kbps / 8 = 1 .. 48
N_BATCHES = 7
N_FRAMES = N_BATCHES * BATCH                # logical frames of one scenario: 196 = 39 super frames and the inserted ones
EDGE_LENGTHS = (0, 1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 959, 960, 961)
AU_HEAD = {2: 5, 3: 6, 4: 8, 6: 11}         # mp4processor.cpp:272-304: the first AU starts behind the header
AU_MODE = {4: (0, 0), 2: (0, 1), 6: (1, 0), 3: (1, 1)}      # (dac_rate, sbr_flag)


# ---- the independent check of one record (test_gpu_au_table.py imports it back) ---------------------------------------------------
def _crc16(b):
    crc = 0xFFFF
    for v in bytes(b):
        crc ^= v << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc ^ 0xFFFF


def _check_record_against_its_super_frame(r, sf, kbps):
    """What a host relies on: the record's table is the header's, the masks are the CRCs' (checked here once with a CRC of the test's own)."""
    end = 110 * kbps // 8
    n = int(r["num_aus"])
    dac, sbr = (sf[2] >> 6) & 1, (sf[2] >> 5) & 1
    assert n == {0: 4, 1: 2, 2: 6, 3: 3}[2 * dac + sbr] and r["stream_parms"] == sf[2] & 0x7F
    st = [int(v) for v in r["au_start"][:n + 1]]
    assert st[0] == {4: 8, 2: 5, 6: 11, 3: 6}[n] and st[n] == end and all(int(v) == 0 for v in r["au_start"][n + 1:])
    for a in range(n):
        ln = st[a + 1] - st[a] - 2
        bad_len = ln > 960 or ln < 0 or st[a] + ln + 2 > end
        assert bool(r["au_len_bad"] >> a & 1) == bad_len
        if bad_len:
            assert not (r["au_crc_ok"] >> a & 1)
            continue
        good = _crc16(sf[st[a]:st[a] + ln]) == (int(sf[st[a] + ln]) << 8 | int(sf[st[a] + ln + 1]))
        assert bool(r["au_crc_ok"] >> a & 1) == good, a
    assert r["au_crc_ok"] >> n == 0 and r["au_len_bad"] >> n == 0


# ---- fast equals of ds.crc16 / ds.rs_parity (test_dabplus_cases.py proves them equal) ----------------------------------------------
def crc16_fast(data):
    """ds.crc16: CCITT 0x1021, start 0xFFFF, complemented."""
    return binascii.crc_hqx(bytes(data), 0xFFFF) ^ 0xFFFF


_GF_MUL_G = None


def rs_parity_columns(data):
    """ds.rs_parity on every column of data [110, R] at once: [10, R] (the same LFSR, the feedback products from a 10 x 256 table)."""
    global _GF_MUL_G
    if _GF_MUL_G is None:
        _GF_MUL_G = np.array([[ds._gf_mul(fb, ds._RS_G[9 - j]) for fb in range(256)] for j in range(10)], np.uint8)
    rem = np.zeros((10, data.shape[1]), np.uint8)
    for d in data:
        fb = d ^ rem[0]
        rem = np.concatenate([rem[1:], np.zeros((1, data.shape[1]), np.uint8)])
        rem ^= _GF_MUL_G[:, fb]
    return rem


# ---- one super frame ------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Kind:
    n_au: int = 3                # 2, 3, 4, 6: the four header layouts
    table: str = "even"          # even | edge | sorted | unsorted
    bad_crc: float = 0.0         # fraction of AUs whose CRC is deliberately wrong
    header: str = ""             # "" | burst (inside one byte) | burst_any (any bit offset) | garbage -- before RS encoding
    k: int = 0                   # byte errors per hit code word -- after RS encoding
    hit: str = "all"             # all | first | last | random: which code words
    parity_only: bool = False    # the k errors in parity bytes only
    header_safe: bool = True     # k > 5: no error in a byte of the fire-coded header, so that the failed decode leaves an accepted super frame
    noise_frame: int = -1        # this logical frame of the five replaced by noise


def _au_starts(R, rng, n_au, table):
    end, h = 110 * R, AU_HEAD[n_au]
    if table == "even":            # as ds.build_superframe, every AU <= 960 bytes where the rate allows it, the last takes the rest
        step = max(2, min((end - h) // n_au, 962, (4095 - h) // (n_au - 1)))          # the starts are 12-bit fields
        return [h + i * step for i in range(1, n_au)]
    if table == "edge":
        out, at = [], h
        for _ in range(n_au - 1):
            at = (at + int(rng.choice(EDGE_LENGTHS)) + 2) & 0xFFF
            out.append(at)
        return out
    if table == "sorted":
        return sorted(int(v) for v in rng.integers(h, min(end, 4095) + 1, n_au - 1))
    assert table == "unsorted"
    return [int(v) for v in rng.integers(0, 4096, n_au - 1)]


def _burst(rng, inside_one_byte):
    """(bit offset 0 .. 87 counted from the MSB of byte 0, bit pattern of 1 .. 6 bits with both ends set)."""
    L = int(rng.integers(1, 7))
    pat = 1 if L == 1 else (1 << (L - 1)) | 1 | (int(rng.integers(0, 1 << (L - 2))) << 1 if L > 2 else 0)
    at = int(rng.integers(0, 11)) * 8 + int(rng.integers(0, 9 - L)) if inside_one_byte else int(rng.integers(0, 88 - L + 1))
    return at, L, pat


def build_super_frame(R, rng, kind):
    """(the 120 R bytes as transmitted, facts): facts["sf"] is the super frame a perfect decoder hands on (110 R bytes, header as
    encoded), facts["dirty"] the {code word: error positions} of the channel faults."""
    end, n_au = 110 * R, kind.n_au
    sf = rng.integers(0, 256, end).astype(np.uint8)
    dac, sbr = AU_MODE[n_au]
    sf[2] = (int(sf[2]) & 0x9F) | (dac << 6) | (sbr << 5)
    starts = _au_starts(R, rng, n_au, kind.table)
    nib = [v for f in starts for v in (f >> 8, (f >> 4) & 15, f & 15)]
    for i, v in enumerate(nib):                                 # 12-bit fields from byte 3 on; an odd last nibble stays random
        b = 3 + i // 2
        sf[b] = (int(sf[b]) & 0x0F) | (v << 4) if i % 2 == 0 else (int(sf[b]) & 0xF0) | v
    au = [AU_HEAD[n_au]] + starts + [end]
    for a in range(n_au):
        ln = au[a + 1] - au[a] - 2
        if ln < 0 or au[a + 1] > end or au[a] + ln < AU_HEAD[n_au]:      # nowhere to put a CRC (or it would land in the table itself)
            continue
        c = crc16_fast(sf[au[a]:au[a] + ln])
        if rng.random() < kind.bad_crc:
            c ^= int(rng.integers(1, 65536))
        sf[au[a] + ln], sf[au[a] + ln + 1] = c >> 8, c & 0xFF
    fc = ds.firecode_parity(bytes(sf[2:11]))
    sf[0], sf[1] = fc >> 8, fc & 0xFF
    good = sf.copy()
    if kind.header in ("burst", "burst_any"):
        at, L, pat = _burst(rng, kind.header == "burst")
        v = int.from_bytes(bytes(sf[:11]), "big") ^ (pat << (88 - at - L))
        sf[:11] = np.frombuffer(v.to_bytes(11, "big"), np.uint8)
    elif kind.header == "garbage":
        sf[:11] = rng.integers(0, 256, 11)
    full = np.zeros(120 * R, np.uint8)
    full[:end] = sf
    full[end:] = rs_parity_columns(sf.reshape(110, R)).reshape(-1)
    dirty = {}
    if kind.k:
        cws = {"all": range(R), "first": [0], "last": [R - 1],
               "random": sorted(set(rng.integers(0, R, max(1, R // 3)).tolist()))}[kind.hit]
        for j in cws:
            pool = np.arange(110, 120) if kind.parity_only else np.arange(120)
            if kind.k > 5 and kind.header_safe:
                pool = pool[j + pool * R >= 11]
            pos = rng.choice(pool, kind.k, replace=False)
            full[j + pos * R] ^= rng.integers(1, 256, kind.k).astype(np.uint8)
            dirty[int(j)] = sorted(int(p) for p in pos)
    if kind.noise_frame >= 0:
        f = kind.noise_frame
        full[f * 24 * R:(f + 1) * 24 * R] = rng.integers(0, 256, 24 * R)
    return full, {"kind": kind, "sf": good, "dirty": dirty}


def super_frame(R, rng, kind):
    """The 120 R bytes that are cut into five logical frames: random payload, header byte 2 (dac, sbr), the 12-bit AU starts, AU CRCs,
    fire-code parity, RS parity per column (ds.crc16, ds.firecode_parity, ds.rs_parity), then the faults `kind` names."""
    return build_super_frame(R, rng, kind)[0]


# ---- one sub-channel's logical frames ---------------------------------------------------------------------------------------------------
CLEAN = Kind()


def _kinds(R, rng):
    """The mix of one scenario: every header layout, every table, header and channel faults.  Three of them are (nearly) always rejected
    -- garbage header, first logical frame lost, 20 errors in every code word the header's bytes included -- and go one into each of the
    three blocks, away from the slips, so that no four windows in a row fail unplanned."""
    ks = [int(v) for v in rng.permutation(5) + 1]                        # every k of 1 .. 5 once, in an order of the seed's
    n = lambda: int(rng.choice([2, 3, 4, 6]))                            # noqa: E731
    mix = [Kind(2, "edge", 0.3), Kind(3, "edge", 0.3), Kind(4, "edge", 0.3), Kind(6, "edge", 0.3),
           Kind(n(), "sorted", 0.2), Kind(n(), "unsorted"), Kind(n(), "unsorted"),
           Kind(2, header="burst"), Kind(4, header="burst", k=2), Kind(n(), header="burst_any"),
           Kind(6, k=ks[0], hit="first"), Kind(3, k=ks[1], hit="last"), Kind(n(), k=ks[2], hit="all"), Kind(n(), k=ks[3], hit="random"),
           Kind(n(), k=ks[4], hit="first", parity_only=True), Kind(n(), "edge", 0.3, k=5, hit="all"),
           Kind(n(), k=6, hit="last"), Kind(n(), k=8, hit="random"), Kind(n(), k=20, hit="first"),
           Kind(n(), noise_frame=int(rng.integers(1, 5)))]
    mix = [mix[i] for i in rng.permutation(len(mix))]
    rejected = [Kind(n(), header="garbage"), Kind(n(), noise_frame=0), Kind(n(), k=20, hit="all", header_safe=False)]
    cut = [0, 6, 13, len(mix)]
    blocks = [mix[cut[b]:cut[b + 1]] for b in range(3)]
    for b in range(3):
        blocks[b].insert(2, rejected[b])
    return blocks


def decoy_header(rng):
    """Eleven bytes that pass the fire-code check."""
    h = rng.integers(0, 256, 11).astype(np.uint8)
    fc = ds.firecode_parity(bytes(h[2:11]))
    h[0], h[1] = fc >> 8, fc & 0xFF
    return h


def build_scenario(R, seed, n_frames=N_FRAMES):
    """(frames [n_frames, 24 R], facts).  facts["sf"][first logical frame] = the facts of the super frame that starts there,
    facts["junk"], facts["slips"] = [(frame, inserted)], facts["decoy"] = the logical frame that carries the decoy header.

    junk (0 .. 4 frames, (R + seed) % 5) | clean, block 0 | slip of 1 .. 4 frames | 3 super frames the four failed windows and the
    slide consume, clean, block 1 | slip of 2 .. 4 frames | 7 super frames: the windows fail, the slide reaches the decoy 16 frames
    behind the slip -- not a super-frame start, but its first 11 bytes pass the fire code -- the decoder locks there, fails four more
    windows and slides again | clean, block 2 | super frames of the mix until the frames run out, junk for the rest."""
    rng = np.random.default_rng([R, seed])
    nb = 24 * R
    out, facts = [], {"sf": {}, "slips": [], "R": R, "seed": seed}

    def junk(n):
        for _ in range(n):
            out.append(rng.integers(0, 256, nb).astype(np.uint8))

    def sf(kind):
        full, f = build_super_frame(R, rng, kind)
        facts["sf"][len(out)] = f
        out.extend(full.reshape(5, nb))

    facts["junk"] = (R + seed) % 5
    junk(facts["junk"])
    blocks = _kinds(R, rng)
    sf(CLEAN)
    for k in blocks[0]:
        sf(k)
    m1 = 1 + (R + 2 * seed) % 4
    facts["slips"].append((len(out), m1))
    junk(m1)
    for _ in range(3):
        sf(CLEAN)
    sf(CLEAN)
    for k in blocks[1]:
        sf(k)
    m2 = 2 + (R + seed) % 3
    at = len(out)
    facts["slips"].append((at, m2))
    junk(m2)
    for _ in range(7):
        sf(CLEAN)
    facts["decoy"] = at + 16                                     # the first frame the slide looks at (see oracle/msc.c mp4_add_to_frame)
    assert facts["decoy"] not in facts["sf"]
    out[facts["decoy"]][:11] = decoy_header(rng)
    sf(CLEAN)
    for k in blocks[2]:
        sf(k)
    fill = [k for b in blocks for k in b if k.header != "garbage" and k.noise_frame != 0 and k.header_safe]
    i = 0
    while len(out) + 5 <= n_frames:
        sf(fill[i % len(fill)])
        i += 1
    junk(n_frames - len(out))
    assert len(out) == n_frames
    return np.stack(out), facts


def scenario(R, seed):
    """The logical frames [N_FRAMES, 24 R] of one sub-channel."""
    return build_scenario(R, seed)[0]


# ---- soft bits ---------------------------------------------------------------------------------------------------------------------------
def dabplus_layout(profiles, dab_plus=None):
    """msc_cases.layout_of with the slots marked DAB+ (dab_plus: per-slot flags, default all 1)."""
    lay = layout_of(profiles)
    for i, c in enumerate(lay):
        c.dab_plus = 1 if dab_plus is None else int(dab_plus[i])
    return lay


def coded_frames(profile, frames):
    """Noise-free soft bits [n, n_in] of logical frames [n, 3 kbps]: energy dispersal, ds.conv_encode, the oracle's own puncturing map,
    amplitude +-127."""
    n_in, m = oracle_map(profile)
    nbits = 24 * profile[0]
    prbs = np.zeros(nbits, np.uint8)
    ol.oracle().ora_prbs(prbs, nbits)
    tx = m >= 0
    soft = np.zeros((len(frames), n_in), np.int16)
    for i, f in enumerate(frames):
        code = ds.conv_encode(np.unpackbits(f) ^ prbs).astype(np.int16)
        soft[i, m[tx]] = (2 * code[tx] - 1) * 127
    return soft


def cifs_of(layout, per_slot_frames, rng):
    """[16 + n, 55296] int16: logical frame k of slot j (per_slot_frames[j][k]; None: nothing placed) becomes frame 16 + k of the
    sub-channel, placed for the time de-interleaver the way msc_cases.stream_cifs places its frames; all else is uniform noise."""
    n = max(len(f) for f in per_slot_frames if f is not None)
    cifs = rng.integers(-127, 128, (HISTORY + n, CIF_BITS)).astype(np.int16)
    for sc, frames in zip(layout, per_slot_frames):
        if frames is None or sc.kbps == 0:
            continue
        assert len(frames) == n
        n_in, base = sc.cu_size * 64, sc.cu_start * 64
        T = coded_frames(mc.profile_of(sc), frames)
        assert T.shape[1] == n_in
        for m in range(16):
            cifs[BITREV4[m]:BITREV4[m] + n, base + m:base + n_in:16] = T[:, m::16]
    return cifs


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------
def oracle_results(layout, cifs, threads=8):
    """Per slot (None: not configured): {"frames" [n, 3 kbps], "sf" [n_sf, 110 R], "sfi" [n_sf] SUPERFRAME_INFO, "stats"} from
    OraBackend.  A slot with dab_plus = 0 has its logical frames only (the oracle back end has no such switch: its super-frame
    results are dropped here, the stage must not produce any)."""
    def one(sc):
        if sc.kbps == 0:
            return None
        b = ol.OraBackend(sc.cu_size, sc.kbps, sc.prot_level, sc.short_form, sc.cu_start, sc.subch_id)
        try:
            for c in range(cifs.shape[0]):
                b.push(cifs[c, sc.cu_start * 64:(sc.cu_start + sc.cu_size) * 64])
            st = b.stats()
            if not sc.dab_plus:
                return {"frames": b.msc_frames(), "sf": np.zeros((0, 110 * sc.kbps // 8), np.uint8), "sfi": np.zeros(0, SUPERFRAME_INFO),
                        "stats": dict(st, sf_ok=0, sf_fail=0, rs_corr=0, rs_fail=0, fc_corr=0, au_ok=0, au_bad=0)}
            return {"frames": b.msc_frames(), "sf": b.sf_bytes().reshape(-1, 110 * sc.kbps // 8), "sfi": b.sfi_bytes().view(SUPERFRAME_INFO),
                    "stats": st}
        finally:
            b.close()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(one, layout))


# ---- the sets both test files use -------------------------------------------------------------------------------------------------------
EVERY_RATE_STREAMS = 2
BOUNDARY_RATES = [8, 24, 64, 72, 136, 384]          # R = 1, 3, 8, 9, 17, 48
BOUNDARY_STREAMS = 5
BOUNDARY_COUNTS = [BATCH, 0, 1, 4, 5, 6, 27, 13]    # CIFs a stream receives in a batch: stream s starts the cycle at its own place (in this
                                                    # order every stream's batch ends fall on all five residues of frames % 5)


def every_rate_layouts():
    lays = pack_layouts([(k, PROT, 0) for k in RATES])
    for lay in lays:
        for c in lay:
            c.dab_plus = 1
    assert sorted(c.kbps for lay in lays for c in lay) == RATES
    assert all(mc.lane_per_trellis_capable(mc.profile_of(c)) for lay in lays for c in lay)
    return lays


def boundary_layout():
    return dabplus_layout([(k, PROT, 0) for k in BOUNDARY_RATES])


def seed_of(set_no, stream):
    """Scenario seed of a stream: set 0 = every rate, 1 = batch boundaries / both decoders, 2 = slots next to each other."""
    return 100 * set_no + stream


_cache = {}


def stream_case(set_no, layout, s):
    """(per-slot scenario facts, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296], per-slot oracle results) of stream s on
    `layout`: slot j carries scenario(R_j, seed_of(set_no, s)).  Cached: tests of one process share the arrays."""
    key = (set_no, s, tuple((c.kbps, c.cu_start, c.cu_size, c.dab_plus) for c in layout))
    if key not in _cache:
        built = [build_scenario(c.kbps // 8, seed_of(set_no, s)) if c.kbps else (None, None) for c in layout]
        cifs = cifs_of(layout, [b[0] for b in built], np.random.default_rng([7, set_no, s]))
        _cache[key] = ([b[1] for b in built], [b[0] for b in built], cifs, oracle_results(layout, cifs))
    return _cache[key]


def neighbour_layouts():
    """Stream 0: a DAB+ slot, a slot that is not configured, a slot that is NOT DAB+ (its data are a DAB+ scenario all the same: the stage
    would lock on it if it looked) and another DAB+ slot; stream 1: the same places, all four DAB+."""
    full = dabplus_layout([(64, PROT, 0), (16, PROT, 0), (40, PROT, 0), (24, PROT, 0)])
    part = dabplus_layout([(64, PROT, 0), (16, PROT, 0), (40, PROT, 0), (24, PROT, 0)], dab_plus=[1, 1, 0, 1])
    part[1] = ds.SubCh(1, 0, 0, 0, dab_plus=0)
    return [part, full]


def all_cases():
    """Every (set number, layout, stream) the GPU tests run: test_dabplus_cases.py proves the inputs on exactly these."""
    out = [(0, lay, s) for lay in every_rate_layouts() for s in range(EVERY_RATE_STREAMS)]
    out += [(1, boundary_layout(), s) for s in range(BOUNDARY_STREAMS)]
    out += [(2, lay, s) for s, lay in enumerate(neighbour_layouts())]
    return out


def boundary_schedule():
    """[batch][stream]: the CIFs every stream receives in each batch of the batch-boundary test, until all have had N_FRAMES: stream s
    walks through BOUNDARY_COUNTS from place s on (the last count is what is left)."""
    left, out, b = [N_FRAMES] * BOUNDARY_STREAMS, [], 0
    while any(left):
        row = [min(BOUNDARY_COUNTS[(b + s) % len(BOUNDARY_COUNTS)], left[s]) for s in range(BOUNDARY_STREAMS)]
        left = [a - c for a, c in zip(left, row)]
        out.append(row)
        b += 1
    return out
