"""Shared by test_aac_stream_cases.py (no device), test_gpu_aac_stream_stage.py, test_gpu_aac_stream_delivery.py and
tools/bench_aac_stream.py: a bit-serial model of the LOAS/LATM stream the reference makes of a DAB+ slot's access units, and the scenarios
that drive it.

The model restates, line by line, BitWriter (base/backend/audio/bit_writer.cpp:29-59), Mp4Processor::_build_aac_stream
(base/backend/audio/mp4processor.cpp:395-445) and the access-unit walk of _process_super_frame (:320-391) on a super frame's bytes and its
dabx_superframe_info record -- k_dabplus's verdicts; no CRC runs here.  It appends one bit at a time and knows nothing of templates or
shifts, which is what the device code is made of.

The scenarios are logical frames of DAB+ slots built with dabplus_cases' helpers: all four AU-table layouts, access units of every
edge length, length and CRC failures, all eight (dac, sbr, channel) combinations with psFlag / mpegSurround at random, rejected super
frames and, on one slot, a table out of order whose overlapping access units both pass their CRC."""
import os
import sys

import numpy as np

import dabplus_cases as dc
import mp2_audio_cases as mac
import oracle_lib as ol
import packet_cases as pkc
import pad_cases as pc

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from dabstar_amd import lib as dx  # noqa: E402

BATCH, HISTORY = dc.BATCH, dc.HISTORY
N_BATCHES = 7
N_FRAMES = N_BATCHES * BATCH                     # 196 logical frames = 39 super frames and a frame of junk
EDGE_L = (0, 1, 2, 254, 255, 256, 509, 510, 511, 764, 765, 766, 959, 960)
LOST_LEN, LOST_CRC = dx.AAC_LOST_LEN, dx.AAC_LOST_CRC
COUNTERS = ("superframes", "records", "frames", "frame_bytes", "lost_len", "lost_crc")
MUTATIONS = ("shift", "mod256", "size", "srindex")


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """bit_writer.cpp:29-59."""

    def __init__(self):
        self.data, self.byte_bits = [], 0

    def add_bits(self, data_new, count):                      # :29-46
        while count > 0:
            if self.byte_bits == 0:                           # :34-35
                self.data.append(0x00)
            copy_bits = min(count, 8 - self.byte_bits)        # :37
            copy_data = (data_new >> (count - copy_bits)) & (0xFF >> (8 - copy_bits))      # :38
            self.data[-1] |= copy_data << (8 - self.byte_bits - copy_bits)                 # :39
            self.byte_bits = (self.byte_bits + copy_bits) % 8                              # :43
            count -= copy_bits                                # :44

    def add_bytes(self, data):                                # :48-52
        for b in data:
            self.add_bits(int(b), 8)

    def write_audio_mux_length_bytes(self, mut=()):           # :54-59
        n = len(self.data) - (0 if "size" in mut else 3)      # :56
        self.data[1] |= (n >> 8) & 0x1F                       # :57
        self.data[2] = n & 0xFF                               # :58


def stream_parameters(parms, mut=()):
    """mp4processor.cpp:259-269 on mOutVec[2] & 0x7F."""
    dac, sbr, ch = (parms >> 6) & 1, (parms >> 5) & 1, (parms >> 4) & 1        # :259-261 (psFlag :262, mpegSurround :263 go nowhere)
    core_sr = ((6 if sbr else 3) if dac else (8 if sbr else 5))                # :266
    if "srindex" in mut:
        core_sr = ((6 if sbr else 3) if not dac else (8 if sbr else 5))
    return {"dac": dac, "sbr": sbr, "CoreSrIndex": core_sr, "CoreChConfig": 2 if ch else 1,      # :267
            "ExtensionSrIndex": 3 if dac else 5}                                                 # :269


def build_aac_stream(L, sp, data, mut=()):
    """_build_aac_stream, :395-445: the LOAS frame of an access unit of L bytes."""
    bw = BitWriter()                          # :397
    bw.add_bits(0x2B7, 11)                    # :399 syncword
    bw.add_bits(0, 13)                        # :400 audioMuxLengthBytes, written later
    bw.add_bits(0, 1)                         # :403 useSameStreamMux
    bw.add_bits(0, 1)                         # :406 audioMuxVersion
    bw.add_bits(1, 1)                         # :407 allStreamsSameTimeFraming
    bw.add_bits(0, 6)                         # :408 numSubFrames
    bw.add_bits(0, 4)                         # :409 numProgram
    bw.add_bits(0, 3)                         # :410 numLayer
    if bool(sp["sbr"]) != ("shift" in mut):   # :412
        bw.add_bits(0b00101, 5)               # :414 SBR
        bw.add_bits(sp["CoreSrIndex"], 4)     # :415
        bw.add_bits(sp["CoreChConfig"], 4)    # :416
        bw.add_bits(sp["ExtensionSrIndex"], 4)      # :417
        bw.add_bits(0b00010, 5)               # :418 AAC LC
        bw.add_bits(0b100, 3)                 # :419 GASpecificConfig() with 960 transform
    else:
        bw.add_bits(0b00010, 5)               # :423
        bw.add_bits(sp["CoreSrIndex"], 4)     # :424
        bw.add_bits(sp["CoreChConfig"], 4)    # :425
        bw.add_bits(0b100, 3)                 # :426
    bw.add_bits(0b000, 3)                     # :429 frameLengthType
    bw.add_bits(0xFF, 8)                      # :430 latmBufferFullness
    bw.add_bits(0, 1)                         # :431 otherDataPresent
    bw.add_bits(0, 1)                         # :432 crcCheckPresent
    for _ in range(L // 255):                 # :435-438
        bw.add_bits(0xFF, 8)
    bw.add_bits(L % (256 if "mod256" in mut else 255), 8)      # :439
    bw.add_bytes(data[:L])                    # :441
    bw.write_audio_mux_length_bytes(mut)      # :442
    return bytes(bw.data)                     # :444


class AacModel:
    """The slot's records, bytes and counters; snaps[n] = (records, bytes) after n super frames."""

    def __init__(self, mut=()):
        self.mut = mut
        self.rows, self.chunks, self.n_bytes = [], [], 0
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.snaps = [(0, 0, dict(self.counters))]
        self.sf_bytes = []                    # bytes every super frame emitted
        self.lines = set()                    # the branches of :320-382 taken

    def super_frame(self, sf, r):
        """:320-391 for one super frame (sf: its 110 R bytes, r: its SUPERFRAME_INFO record)."""
        sp = stream_parameters(int(r["stream_parms"]), self.mut)
        before = self.n_bytes
        n_au = int(r["num_aus"])
        for a in range(n_au):                                                  # :320
            L = int(r["au_start"][a + 1]) - int(r["au_start"][a]) - 2          # :322
            if int(r["au_len_bad"]) >> a & 1:                                  # :325 (k_dabplus's verdict)
                self.lines.add(325)
                self._row(r, a, 0, L, LOST_LEN)
                self.counters["lost_len"] += 1
            elif int(r["au_crc_ok"]) >> a & 1:                                 # :333
                self.lines.add(333)
                st = int(r["au_start"][a])
                frame = build_aac_stream(L, sp, sf[st:st + L], self.mut)       # :337
                self._row(r, a, len(frame), L, 0)
                self.chunks.append(frame)                                      # :341
                self.n_bytes += len(frame)
                self.counters["frames"] += 1
            else:                                                              # :377
                self.lines.add(377)
                self._row(r, a, 0, L, LOST_CRC)
                self.counters["lost_crc"] += 1
        self.counters["superframes"] += 1
        self.counters["records"] += n_au
        self.counters["frame_bytes"] = self.n_bytes
        self.sf_bytes.append(self.n_bytes - before)
        self.snaps.append((len(self.rows), self.n_bytes, dict(self.counters)))

    def _row(self, r, a, length, L, flags):
        self.rows.append((self.n_bytes, int(r["first_frame"]), length, L & 0xFFFF, a, int(r["num_aus"]), int(r["stream_parms"]), flags, [0] * 8))

    def records(self):
        out = np.zeros(len(self.rows), dx.AAC_FRAME)
        for i, row in enumerate(self.rows):
            out[i] = row
        return out

    def all_bytes(self):
        return np.frombuffer(b"".join(self.chunks), np.uint8)


def run_model(sfs, sfis, mut=()):
    m = AacModel(mut)
    for sf, r in zip(sfs, sfis):
        m.super_frame(np.asarray(sf), r)
    return m


def info_of(sf, kbps, first_frame=0):
    """The dabx_superframe_info of an accepted, error-free super frame, as k_dabplus fills it (mp4processor.cpp:256-333 and the engine's
    bound on the super frame; rs / fc fields 0)."""
    end = 110 * kbps // 8
    r = np.zeros(1, dx.SUPERFRAME_INFO)[0]
    dac, sbr = (int(sf[2]) >> 6) & 1, (int(sf[2]) >> 5) & 1
    n = {0: 4, 1: 2, 2: 6, 3: 3}[2 * dac + sbr]
    o = [int(v) for v in sf[:11]]
    tab = [o[3] * 16 + (o[4] >> 4), (o[4] & 15) * 256 + o[5], o[6] * 16 + (o[7] >> 4), (o[7] & 15) * 256 + o[8], o[9] * 16 + (o[10] >> 4)]
    st = [dc.AU_HEAD[n]] + tab[:n - 1] + [end]
    crc_ok = len_bad = 0
    for a in range(n):
        L = st[a + 1] - st[a] - 2
        if L > 960 or L < 0 or st[a] + L + 2 > end:
            len_bad |= 1 << a
        elif dc.crc16_fast(sf[st[a]:st[a] + L]) == (int(sf[st[a] + L]) << 8 | int(sf[st[a] + L + 1])):
            crc_ok |= 1 << a
    r["num_aus"], r["au_crc_ok"], r["au_len_bad"], r["stream_parms"] = n, crc_ok, len_bad, int(sf[2]) & 0x7F
    r["au_start"][:n + 1] = st
    r["first_frame"] = first_frame
    return r


# ---- an independent parser of the stream (used by the tests only) -----------------------------------------------------------------------------
class BitReader:
    def __init__(self, data):
        self.bits, self.at = np.unpackbits(np.frombuffer(bytes(data), np.uint8)), 0

    def get(self, n):
        v = 0
        for b in self.bits[self.at:self.at + n]:
            v = (v << 1) | int(b)
        assert self.at + n <= len(self.bits)
        self.at += n
        return v


def parse_loas(stream):
    """[(parameters, payload bytes)] of a sequence of LOAS AudioSyncStream frames holding one AudioMuxElement(1) each with its own
    StreamMuxConfig (ISO/IEC 14496-3, 1.7.2 / 1.7.3), as the reference writes them: whatever else the syntax allows is an AssertionError."""
    out, at = [], 0
    stream = bytes(stream)
    while at < len(stream):
        br = BitReader(stream[at:at + 3])
        assert br.get(11) == 0x2B7, "no sync word at %d" % at
        n = br.get(13)                                        # audioMuxLengthBytes
        br = BitReader(stream[at + 3:at + 3 + n])
        assert len(br.bits) == 8 * n
        assert br.get(1) == 0                                 # useSameStreamMux
        assert br.get(1) == 0                                 # audioMuxVersion
        assert br.get(1) == 1                                 # allStreamsSameTimeFraming
        assert (br.get(6), br.get(4), br.get(3)) == (0, 0, 0)       # numSubFrames, numProgram, numLayer
        aot = br.get(5)                                       # AudioSpecificConfig
        p = {"sr": br.get(4), "ch": br.get(4), "sbr": 0, "ext": None}
        if aot == 5:
            p["sbr"], p["ext"] = 1, br.get(4)
            aot = br.get(5)
        assert aot == 2                                       # AAC LC
        assert (br.get(1), br.get(1), br.get(1)) == (1, 0, 0)       # GASpecificConfig: frameLengthFlag (960), dependsOnCoreCoder, extensionFlag
        assert br.get(3) == 0 and br.get(8) == 0xFF           # frameLengthType, latmBufferFullness
        assert br.get(1) == 0 and br.get(1) == 0              # otherDataPresent, crcCheckPresent
        L = 0                                                 # PayloadLengthInfo
        while True:
            t = br.get(8)
            L += t
            if t != 255:
                break
        payload = bytes(br.get(8) for _ in range(L))
        rest = len(br.bits) - br.at
        assert 0 <= rest < 8 and br.get(rest) == 0            # byte alignment
        out.append((p, payload))
        at += 3 + n
    assert at == len(stream)
    return out


# ---- one super frame --------------------------------------------------------------------------------------------------------------------------
N_AU = {(0, 0): 4, (0, 1): 2, (1, 0): 6, (1, 1): 3}           # (dac, sbr): mp4processor.cpp:273-304


def make_super_frame(R, rng, dac, sbr, ch, starts, bad_crc=(), garbage=False, crc_order=None):
    """The 120 R bytes of a super frame with the AU starts `starts` (n_au - 1 of them), random payload, good AU CRCs but for the access units
    in bad_crc (crc_order: the order in which the CRCs are placed -- overlapping access units), fire code and RS parity.  garbage: the
    eleven header bytes replaced by noise afterwards, so that the fire code rejects the window.  Returns (bytes, the super frame)."""
    end, n_au = 110 * R, N_AU[(dac, sbr)]
    assert len(starts) == n_au - 1 and all(0 <= v < 4096 for v in starts)
    sf = rng.integers(0, 256, end).astype(np.uint8)
    sf[2] = (int(sf[2]) & 0x0F) | (dac << 6) | (sbr << 5) | (ch << 4)          # bit 7 unused, psFlag and mpegSurround random
    nib = [v for f in starts for v in (f >> 8, (f >> 4) & 15, f & 15)]
    for i, v in enumerate(nib):
        b = 3 + i // 2
        sf[b] = (int(sf[b]) & 0x0F) | (v << 4) if i % 2 == 0 else (int(sf[b]) & 0xF0) | v
    au = [dc.AU_HEAD[n_au]] + list(starts) + [end]
    for a in (range(n_au) if crc_order is None else crc_order):
        L = au[a + 1] - au[a] - 2
        if L < 0 or L > 960 or au[a] + L + 2 > end:
            continue
        c = dc.crc16_fast(sf[au[a]:au[a] + L])
        if a in bad_crc:
            c ^= int(rng.integers(1, 65536))
        sf[au[a] + L], sf[au[a] + L + 1] = c >> 8, c & 0xFF
    fc = ds.firecode_parity(bytes(sf[2:11]))
    sf[0], sf[1] = fc >> 8, fc & 0xFF
    good = sf.copy()
    if garbage:                               # noise the fire code neither passes nor "corrects" (check_and_correct_6bits mends one header in 25)
        while True:
            sf[:11] = rng.integers(0, 256, 11)
            probe = np.ascontiguousarray(sf[:11].copy())
            if not ol.oracle().ora_firecode_check_and_correct(probe):
                break
    full = np.zeros(120 * R, np.uint8)
    full[:end] = sf
    full[end:] = dc.rs_parity_columns(sf.reshape(110, R)).reshape(-1)
    return full, good


def _starts_for(R, n_au, want, rng):
    """AU starts such that the access units named in want = {a: L} have these lengths where the super frame has room; the others share the
    rest evenly (at a high rate some of them are longer than 960: LOST_LEN)."""
    end, h = 110 * R, dc.AU_HEAD[n_au]
    free = [a for a in range(n_au) if a not in want]
    room = end - h - sum(L + 2 for L in want.values())
    if not free or room < 2 * len(free):
        return None
    share = [room // len(free)] * len(free)
    share[-1] += room - sum(share)
    size = {a: (want[a] + 2 if a in want else share[free.index(a)]) for a in range(n_au)}
    st, at = [], h
    for a in range(n_au - 1):
        at += size[a]
        st.append(at)
    return st if all(v < 4096 for v in st) else None


def build_scenario(R, seed, overlap=False, n_frames=N_FRAMES):
    """(frames [n_frames, 24 R], facts): facts["sf"] = [(first logical frame, the super frame, accepted)] in order."""
    rng = np.random.default_rng([R, seed, 41])
    nb = 24 * R
    out, facts = [], {"sf": [], "R": R, "overlap": None}
    for _ in range((R + seed) % 3):
        out.append(rng.integers(0, 256, nb).astype(np.uint8))
    combos = [(dac, sbr, ch) for dac in (0, 1) for sbr in (0, 1) for ch in (0, 1)]
    edge = list(EDGE_L)
    k = 0
    while len(out) + 5 <= n_frames:
        dac, sbr, ch = combos[k % 8]
        n_au = N_AU[(dac, sbr)]
        kw = {}
        mode = k % 13
        starts = None
        if overlap and k == 9:                                # a table out of order: AU 0 and AU 2 overlap, both CRCs good (AU 0's placed first)
            dac, sbr = 1, 1
            n_au = 3
            end = 110 * R
            starts = [min(end - 60, 900), 100]
            kw["crc_order"] = (0, 2)
            facts["overlap"] = len(facts["sf"])
        elif mode == 5:                                       # L = 961 on the first access unit
            starts = _starts_for(R, n_au, {0: 961}, rng)
        elif mode == 8:                                       # a negative length (-1) on access unit 1, or 0 where there are only two
            starts = _starts_for(R, n_au, {min(1, n_au - 2): -1}, rng)
        elif mode == 11:
            kw["garbage"] = True
        if starts is None:                                    # the next edge lengths on all access units but one, where the super frame has room
            room = 110 * R - dc.AU_HEAD[n_au]
            for order in ([int(a) for a in rng.permutation(n_au)][:n_au - 1], list(range(n_au - 1))):
                want = {}
                for a in order:
                    L = edge[0]
                    if sum(v + 2 for v in want.values()) + L + 2 + 2 * (n_au - len(want) - 1) <= room:
                        want[a] = L
                    edge = edge[1:] + edge[:1]
                starts = _starts_for(R, n_au, want, rng)      # (None: a start beyond the 12-bit field; then the last access unit takes the rest)
                if starts is not None:
                    break
            if starts is None:
                starts = dc._au_starts(R, rng, n_au, "even")
        if "crc_order" not in kw:
            kw["bad_crc"] = {int(a) for a in range(n_au) if rng.random() < 0.2}
        full, good = make_super_frame(R, rng, dac, sbr, ch, starts, **kw)
        facts["sf"].append((len(out), good, not kw.get("garbage", False)))
        out.extend(full.reshape(5, nb))
        k += 1
    while len(out) < n_frames:
        out.append(rng.integers(0, 256, nb).astype(np.uint8))
    return np.stack(out), facts


_cache = {}


def scenario(kbps, seed, overlap=False, n_frames=N_FRAMES):
    key = (kbps, seed, overlap, n_frames)
    if key not in _cache:
        _cache[key] = build_scenario(kbps // 8, seed, overlap, n_frames)
    return _cache[key]


def accepted(facts, kbps):
    """(super frames, records) of a scenario's accepted super frames, the records from info_of."""
    rows = [(f, sf) for f, sf, ok in facts["sf"] if ok]
    return [sf for _, sf in rows], [info_of(sf, kbps, f) for f, sf in rows]


# ---- the sets the tests use -------------------------------------------------------------------------------------------------------------------
PROT = pc.PROT
PACKET_ADDRESS = pc.PACKET_ADDRESS
# (kbps, kind) per slot: "aac" a DAB+ slot with the AAC stream mode on, "aac+pad" one that also has PAD decoding (it carries a PAD scenario of
# tests/pad_cases.py), "pad" a DAB+ slot with PAD decoding only, "mp2" a DAB audio slot with the MP2 audio mode on, "pkt" a packet-mode slot
STAGE_LAYOUTS = [
    [(8, "aac"), (384, "aac"), (64, "aac+pad"), (32, "pad"), (48, "mp2"), (16, "pkt")],
    [(32, "aac"), (64, "aac"), (72, "aac"), (192, "aac"), (64, "pad")],
]
STAGE_STREAMS = [0, 1, 0, 1]                     # layout of stream s
MAX_SUBCH = 6
OVERLAP_SLOTS = {(1, 2), (3, 2)}                 # (stream, slot): the 72 kbit/s slots carry the table out of order


def kinds(s):
    return STAGE_LAYOUTS[STAGE_STREAMS[s]]


def is_aac(kind):
    return kind.startswith("aac")


def seed_of(s, j):
    return 10 * s + j


def stage_layout(lay):
    k = STAGE_LAYOUTS[lay]
    return dc.dabplus_layout([(kbps, PROT, 0) for kbps, _ in k], dab_plus=[int(kind in ("aac", "aac+pad", "pad")) for _, kind in k])


def slot_frames(s, j, kbps, kind, n_frames=N_FRAMES):
    if kind == "aac":
        return scenario(kbps, seed_of(s, j), (s, j) in OVERLAP_SLOTS, n_frames)[0]
    if kind in ("aac+pad", "pad"):
        return pc.scenario(kbps, seed_of(s, j), n_frames)[0]
    if kind == "mp2":
        return mac.scenario(kbps, seed_of(s, j), 5 + j, n_frames)[0]
    return pkc.scenario(kbps, seed_of(s, j), n_frames)


def all_scenarios():
    """(kbps, facts) of every scenario of this file the stage test runs."""
    return [(kbps, scenario(kbps, seed_of(s, j), (s, j) in OVERLAP_SLOTS)[1]) for s in range(len(STAGE_STREAMS))
            for j, (kbps, kind) in enumerate(kinds(s)) if kind == "aac"]


def boundary_schedule(n_streams):
    return pc.boundary_schedule(n_streams, N_FRAMES)


_stage_cache, _model_cache = {}, {}


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16, per-slot oracle results) of stream s.  Cached: the
    tests of one process share the arrays and leave them unchanged."""
    if s not in _stage_cache:
        layout = stage_layout(STAGE_STREAMS[s])
        frames = [slot_frames(s, j, kbps, kind) for j, (kbps, kind) in enumerate(kinds(s))]
        cifs = dc.cifs_of(layout, frames, np.random.default_rng([17, s]))
        _stage_cache[s] = (layout, frames, cifs, dc.oracle_results(layout, cifs))
    return _stage_cache[s]


def slot_model(s, j):
    """The model of slot (s, j) on the oracle back end's super frames and records, computed once."""
    if (s, j) not in _model_cache:
        o = stream_case(s)[3][j]
        _model_cache[(s, j)] = run_model(o["sf"], o["sfi"])
    return _model_cache[(s, j)]
