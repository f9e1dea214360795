"""Shared by test_packet_cases.py (no device) and the two GPU tests of the packet-mode stage (k_packet): DataProcessor restated in plain
Python -- the model every device result is compared with, exactly -- and generators that build the logical frames of a packet-mode data
sub-channel byte by byte.  The oracle (oracle/) has no DataProcessor and cannot be extended, so the model lives here; every branch cites the
line of the reference's base/backend/data/data_processor.cpp it restates.  Two guards go beyond the reference (include/dabx.h): a useful
length that reaches beyond the logical frame drops the packet (len_bad), and a series is bounded at DABX_DG_MAX_BYTES (dg_overflow)."""
import binascii
import collections
import os
import sys

import numpy as np

from dabplus_cases import BOUNDARY_COUNTS

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from dabstar_amd.lib import DATAGROUP_INFO, DG_MAX_BYTES, PACKET_COUNTERS  # noqa: E402

GRANULE = 24
ADDRESS_A, ADDRESS_B = 0x155, 0x2AA          # the two interleaved service components; 0 is padding (EN 300 401 5.3.2.3)
RATES = [8, 16, 32, 64, 128, 384]
N_BATCHES = 4
BATCH = 28
N_FRAMES = N_BATCHES * BATCH


def crc16(data):
    """calc_crc (crc.cpp:75-86): CCITT 0x1021, start 0xFFFF, complemented."""
    return binascii.crc_hqx(bytes(data), 0xFFFF) ^ 0xFFFF


def packet_crc_ok(pkt):
    """check_CRC_bits over the whole packet (crc.cpp:98-132): register all ones, the last 16 bits inverted, remainder zero -- the CRC of
    all but the last two bytes equals those two."""
    return crc16(pkt[:-2]) == (pkt[-2] << 8 | pkt[-1])


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class DataProcessorModel:
    """DataProcessor::add_to_frame -> _handle_packets -> _handle_packet for ONE packet address, on packed bytes.  records / groups: one
    DATAGROUP_INFO row and one bytes object per completed MSC data group (add_MSC_data_group calls); counters: dabx_packet_stats;
    branch: how often each path was taken (for test_packet_cases.py's "the scenarios reach everything")."""

    def __init__(self, address):
        self.address = address
        self.expected = 0                    # mExpectedIndex
        self.state = 0                       # mPacketState
        self.series = b""                    # mSeriesVec
        self.first_frame = 0
        self.broke = False
        self.counters = dict.fromkeys(PACKET_COUNTERS, 0)
        self.branch = collections.Counter()
        self.rows, self.groups = [], []

    def add_frame(self, data, frame):
        data = bytes(data)
        assert len(data) % GRANULE == 0
        self.counters["frames"] += 1
        at, left = 0, len(data)
        while True:                                              # :125
            plen = ((data[at] >> 6) + 1) * GRANULE                # :127
            if left < plen:                                      # :129-133 "be on the safe side"
                self.counters["walk_short"] += 1
                return
            self.counters["packets"] += 1
            self._packet(data, at, plen, frame)                  # :135
            left -= plen                                         # :137
            if left == 0:                                        # :139-146 (whole granules: never a bit left over)
                return
            at += plen                                           # :148

    def _packet(self, data, at, plen, frame):
        ci, fl = (data[at] >> 4) & 3, (data[at] >> 2) & 3        # :159-160
        address = (data[at] & 3) << 8 | data[at + 1]             # :161
        ulen = data[at + 2] & 0x7F                               # :163 (the command bit, :162, is not used)
        if address != self.address:                              # :165
            self.branch["padding" if address == 0 else "other_address"] += 1
            return
        self.counters["addr_match"] += 1
        if ci != self.expected:                                  # :170
            self.counters["continuity_err"] += 1
            self.expected = 0                                    # :176: to 0, not to ci + 1
            self.broke = True
            return
        if self.broke:
            self.branch["accepted_after_break_ci%d" % ci] += 1
        self.broke = False
        self.expected = (self.expected + 1) % 4                  # :181, before the CRC
        if not packet_crc_ok(data[at:at + plen]):                # :184
            self.counters["crc_bad"] += 1
            self.branch["crc_bad_fl%d" % fl] += 1
            return
        if at + 3 + ulen > len(data):                            # guard: :199 / :224 would read past the logical frame
            self.counters["len_bad"] += 1
            return
        if ulen > plen - 5:
            self.branch["beyond_packet_inside_frame"] += 1
        if ulen == 0:
            self.branch["ulen0"] += 1
        payload = data[at + 3:at + 3 + ulen]                     # :196-200: useful length bytes from byte 3, whatever follows
        if self.state == 0:                                      # :191 waiting for a start
            if fl == 2:                                          # :193 first
                self.state, self.series, self.first_frame = 1, payload, frame
                self.branch["first"] += 1
            elif fl == 3:                                        # :202 single
                self.series, self.first_frame = payload, frame
                self.branch["single"] += 1
                self._emit(frame)
            else:                                                # :211-214 cleared, state stays 0
                self.series = b""
                self.branch["orphan_fl%d" % fl] += 1
        else:                                                    # :216 within a series
            if fl in (0, 1):                                     # :218 intermediate, :227 last
                if len(self.series) + ulen > DG_MAX_BYTES:       # guard: mSeriesVec grows without limit
                    self.counters["dg_overflow"] += 1
                    self.state, self.series = 0, b""
                    return
                self.series += payload
                if len(self.series) == DG_MAX_BYTES:
                    self.branch["series_at_bound"] += 1
                if fl == 1:
                    self.branch["last"] += 1
                    self._emit(frame)                            # :236
                    self.state = 0                               # :237
                else:
                    self.branch["intermediate"] += 1
            elif fl == 2:                                        # :239 first, the previous series was erroneous
                self.series, self.first_frame = payload, frame
                self.branch["first_in_series"] += 1
            else:                                                # :248-252 single inside a series: abandoned, NOT emitted
                self.state, self.series = 0, b""
                self.branch["single_in_series"] += 1

    def _emit(self, frame):
        g = self.series
        flag = len(g) > 0 and bool(g[0] & 0x40)                  # ip_datahandler.cpp:48
        ok = flag and len(g) >= 2 and crc16(g[:-2]) == (g[-2] << 8 | g[-1])      # :59 check_crc_bytes(data, len - 2)
        c = self.counters
        self.rows.append((c["dg_bytes"], self.first_frame, frame, len(g), int(flag), int(ok), 0))
        self.groups.append(g)
        c["dg_count"] += 1
        c["dg_bytes"] += len(g)
        c["dg_crc_bad"] += int(flag and not ok)
        self.branch["dg_empty" if not g else "dg_flag_len1" if flag and len(g) == 1 else "dg_crc_ok" if ok else "dg_crc_bad" if flag else "dg_no_flag"] += 1
        if frame > self.first_frame:
            self.branch["dg_over_frames"] += 1
        if len(g) >= 4096:
            self.branch["dg_4096_and_more"] += 1
        self.series = b""

    def records(self):
        return np.array(self.rows, DATAGROUP_INFO) if self.rows else np.zeros(0, DATAGROUP_INFO)

    def all_bytes(self):
        return np.frombuffer(b"".join(self.groups), np.uint8)


def run_model(frames, address, first_frame=0):
    m = DataProcessorModel(address)
    for k, f in enumerate(frames):
        m.add_frame(f, first_frame + k)
    return m


# ---- generators --------------------------------------------------------------------------------------------------------------------------
def packet(code, ci, fl, address, payload, ulen=None, good=True, rng=None):
    """One packet of (code + 1) * 24 bytes (EN 300 401 5.3.2): header, payload from byte 3, filler, CRC.  ulen: the useful-length field
    when it is not to be the payload's length; good = False: a wrong CRC."""
    n = (code + 1) * GRANULE
    assert len(payload) <= n - 5
    b = bytearray(rng.integers(0, 256, n).astype(np.uint8).tobytes() if rng is not None else bytes(n))
    b[0] = code << 6 | ci << 4 | fl << 2 | address >> 8
    b[1] = address & 0xFF
    b[2] = (b[2] & 0x80) | (len(payload) if ulen is None else ulen)
    b[3:3 + len(payload)] = payload
    c = crc16(b[:n - 2]) ^ (0 if good else 0x0810)
    b[n - 2], b[n - 1] = c >> 8, c & 0xFF
    return bytes(b)


def data_group(rng, length, flag, good=True):
    """`length` bytes: bit 6 of byte 0 = the CRC flag; with the flag, the last two bytes are the CRC of the rest (good) or not."""
    g = bytearray(rng.integers(0, 256, length).astype(np.uint8).tobytes())
    if length:
        g[0] = (g[0] & 0xBF) | (0x40 if flag else 0)
    if flag and length >= 2:
        c = crc16(g[:-2]) ^ (0 if good else 0x0001)
        g[-2], g[-1] = c >> 8, c & 0xFF
    return bytes(g)


class Writer:
    """Packets into logical frames of kbps / 8 granules: a packet that does not fit into the rest of the frame is preceded by padding
    packets (address 0).  Keeps the continuity index per address; the scenario breaks it on purpose."""

    def __init__(self, kbps, rng):
        self.gran, self.rng = kbps // 8, rng
        self.frames, self.cur, self.ci = [], bytearray(), {}
        self.max_code = min(3, self.gran - 1)

    def room(self):
        return self.gran - len(self.cur) // GRANULE

    def raw(self, b):
        assert len(b) % GRANULE == 0 and len(b) // GRANULE <= self.room()
        self.cur += b
        if self.room() == 0:
            self.frames.append(bytes(self.cur))
            self.cur = bytearray()

    def pad(self, granules):
        while granules > 0:
            code = int(self.rng.integers(0, min(self.max_code, granules - 1) + 1))
            self.raw(packet(code, self.next_ci(0), 3, 0, b"", rng=self.rng))
            granules -= code + 1

    def pad_frame(self):
        if self.cur:
            self.pad(self.room())

    def until_room(self, g):
        """Pads until exactly g granules of the current frame are left."""
        assert g <= self.gran
        if self.room() < g:
            self.pad_frame()
        self.pad(self.room() - g)

    def next_ci(self, address):
        v = self.ci.get(address, 0)
        self.ci[address] = (v + 1) & 3
        return v

    def resync(self, address):
        """After a break the receiver expects index 0: the sender's next index happens to be 0."""
        self.ci[address] = 0

    def put(self, spec):
        """spec: dict(address, fl, payload, code, [ulen], [good], [drop], [repeat])."""
        ci = self.next_ci(spec["address"])
        if spec.get("drop"):
            return
        p = packet(spec["code"], ci, spec["fl"], spec["address"], spec["payload"], spec.get("ulen"), spec.get("good", True), self.rng)
        for _ in range(2 if spec.get("repeat") else 1):
            if len(p) // GRANULE > self.room():
                self.pad_frame()
            self.raw(p)

    def emit(self, specs):
        for s in specs:
            self.put(s)

    def cut(self, data, address, dense=False, min_packets=1):
        """A data group cut into packets: first (2), intermediate (0), last (1), or one single packet (3).  Packet lengths at random
        among those the frame holds (dense: the longest)."""
        parts, at = [], 0
        while True:
            code = self.max_code if dense else int(self.rng.integers(0, self.max_code + 1))
            cap = (code + 1) * GRANULE - 5
            left_after = min_packets - len(parts) - 1
            take = min(cap, len(data) - at)
            if left_after > 0:
                take = min(take, max(0, (len(data) - at) // (left_after + 1)))
            parts.append((code, data[at:at + take]))
            at += take
            if at >= len(data) and len(parts) >= min_packets:
                break
        out = []
        for i, (code, pl) in enumerate(parts):
            fl = 3 if len(parts) == 1 else 2 if i == 0 else 1 if i == len(parts) - 1 else 0
            out.append(dict(address=address, fl=fl, payload=pl, code=code))
        return out

    def group(self, length, flag, good=True, address=ADDRESS_A, dense=False, min_packets=1):
        return self.cut(data_group(self.rng, length, flag, good), address, dense, min_packets)

    def bytes_left(self, n_frames):
        return (n_frames - len(self.frames)) * self.gran * GRANULE - len(self.cur)


def build_scenario(kbps, seed, n_frames=N_FRAMES):
    """The logical frames [n_frames, 3 kbps] of one packet-mode sub-channel.  What does not fit the bit rate (packet lengths beyond the
    frame, the long groups, the series beyond the bound) is left out; test_packet_cases.py asserts that the committed set of scenarios
    reaches every branch."""
    rng = np.random.default_rng([kbps, seed, 77])
    w = Writer(kbps, rng)
    A, B = ADDRESS_A, ADDRESS_B
    g = w.group
    # good groups: one packet, CRC flag with a good and a bad CRC, one byte with the flag set, no byte at all
    w.emit(g(10, False))
    w.emit(g(1, True))
    w.emit(g(30, True, min_packets=2))
    w.emit(g(25, True, good=False, min_packets=2))
    w.emit(g(0, False))
    w.emit(g(26, False, min_packets=3))
    # last without first, intermediate without first
    w.emit(g(20, False, min_packets=2)[1:])
    w.emit(g(30, False, min_packets=3)[1:2])
    # first without last, then a complete group: its first arrives inside a series
    w.emit(g(30, True, min_packets=2)[:1])
    w.emit(g(28, True, min_packets=2))
    # single inside a series: the series is abandoned and the single packet is not emitted either
    w.emit(g(30, True, min_packets=2)[:1])
    w.emit(g(9, False))
    w.emit(g(8, False))
    # a bad packet CRC in a single, a first, an intermediate and a last packet
    for which, n in ((0, 1), (0, 3), (1, 3), (2, 3)):
        specs = g(36 if n > 1 else 12, True, min_packets=n)
        specs[which]["good"] = False
        w.emit(specs)
    w.emit(g(11, True))
    # a dropped packet; the sender's next index happens to be 0, what the receiver expects after the break
    specs = g(40, True, min_packets=4)
    specs[1]["drop"] = True
    w.emit(specs)
    w.resync(A)
    w.emit(g(21, True, min_packets=2))
    # a repeated packet: the copy breaks the continuity, the sender goes on counting -- packets are lost until its index comes round to 0
    specs = g(60, True, min_packets=6)
    specs[1]["repeat"] = True
    w.emit(specs)
    w.resync(A)
    w.emit(g(13, False))
    # two interleaved addresses and padding packets
    a, b = g(50, True, min_packets=4), g(45, True, address=B, min_packets=4)
    for i in range(max(len(a), len(b))):
        for lst in (a, b):
            if i < len(lst):
                w.put(lst[i])
        if i % 2 == 0:
            w.pad(1)
    # a length code that overruns the frame: the walk ends there
    w.until_room(1)
    junk = bytearray(rng.integers(0, 256, GRANULE).astype(np.uint8).tobytes())
    junk[0] = (junk[0] & 0x3F) | (int(rng.integers(1, 4)) << 6)
    w.raw(bytes(junk))
    # useful length beyond the packet: beyond the frame end (dropped), and inside the frame (delivered as the reference delivers it)
    w.until_room(1)
    w.put(dict(address=A, fl=3, payload=b"\x07" * 19, code=0, ulen=40))
    if w.gran >= 2:
        w.until_room(min(w.gran, 4))
        w.put(dict(address=A, fl=3, payload=b"\x47" * 19, code=0, ulen=min(127, w.room() * GRANULE - 5)))
        w.emit(g(12, True))
    # whole frames of random bytes
    w.pad_frame()
    for _ in range(2):
        w.raw(rng.integers(0, 256, w.gran * GRANULE).astype(np.uint8).tobytes())
    w.resync(A)
    w.emit(g(15, True))
    # long groups, as far as the frames hold them; every packet length the frame holds
    for length in (100, 700, 1000, 4095, 4096, 8191):
        if w.bytes_left(n_frames) > 1.1 * length * 24 / 19 + w.gran * GRANULE:
            w.emit(g(length, bool(length & 1), dense=length > 1000))
    # a series that reaches DABX_DG_MAX_BYTES exactly (kept) and one more byte (abandoned); the rest of it arrives in state 0
    if w.max_code == 3 and w.bytes_left(n_frames) > 1.1 * (DG_MAX_BYTES + 500) * 96 / 91:
        data = data_group(rng, DG_MAX_BYTES + 300, True)
        specs = [dict(address=A, fl=2 if i == 0 else 0, payload=data[91 * i:91 * i + 91], code=3) for i in range(180)]
        specs.append(dict(address=A, fl=0, payload=data[16380:16384], code=0))
        specs.append(dict(address=A, fl=0, payload=data[16384:16385], code=0))
        specs.append(dict(address=A, fl=0, payload=data[16385:16400], code=0))
        specs.append(dict(address=A, fl=1, payload=data[16400:16410], code=0))
        w.emit(specs)
    # groups of both addresses until the frames are full
    while len(w.frames) < n_frames:
        length = int(rng.choice([1, 2, 3, 18, 19, 20, 91, 92, 200, 333])) if rng.integers(0, 4) else int(rng.integers(1, 600))
        w.emit(g(length, bool(rng.integers(0, 2)), good=bool(rng.integers(0, 8)), address=A if rng.integers(0, 3) else B))
        if not rng.integers(0, 5):
            w.pad(1)
    out = np.frombuffer(b"".join(w.frames[:n_frames]), np.uint8).reshape(n_frames, 3 * kbps).copy()
    return out


_cache = {}


def scenario(kbps, seed, n_frames=N_FRAMES):
    key = (kbps, seed, n_frames)
    if key not in _cache:
        _cache[key] = build_scenario(kbps, seed, n_frames)
    return _cache[key]


# ---- a reader that comes late: scenarios that overrun a slot's rings before the first read --------------------------------------------------
# name: (kbps, data-group lengths [lo, hi], CRC flag).  Address A only, everything valid: the model's rows are simply all the groups.
LATE_READER = {
    "A": (8, (1, 19), False),                # one single-packet group per 24-byte frame: 112 groups against a record ring of 64
    "B": (64, (200, 400), True),             # ~17 KB in a byte ring of 32 768, of which DABX_DG_MAX_BYTES are the series' room
    "C": (256, (300, 900), False),           # ~76 KB through a byte ring of 65 536: the surviving window crosses the ring's end
}


def late_reader_scenario(name, n_frames=N_FRAMES):
    """(kbps, logical frames [n_frames, 3 kbps]) of LATE_READER[name]: dense groups until the frames are full (the last may stay open)."""
    key = ("late", name, n_frames)
    if key not in _cache:
        kbps, (lo, hi), flag = LATE_READER[name]
        w = Writer(kbps, np.random.default_rng([kbps, 4711]))
        while len(w.frames) < n_frames:
            w.emit(w.group(int(w.rng.integers(lo, hi + 1)), flag, dense=True))
        _cache[key] = np.frombuffer(b"".join(w.frames[:n_frames]), np.uint8).reshape(n_frames, 3 * kbps).copy()
    return LATE_READER[name][0], _cache[key]


def ring_sizes(kbps):
    """(records, bytes) of a packet-mode slot's rings (dabx_set_packet_mode): powers of two that hold two batches and the series' room."""
    pow2 = lambda v: 1 << (v - 1).bit_length()      # noqa: E731
    return pow2(2 * BATCH * (kbps // 8)), pow2(2 * BATCH * 3 * kbps + DG_MAX_BYTES)


def intact_window(byte_pos, n_bytes, ring_records, ring_bytes, asm_room=DG_MAX_BYTES):
    """The rule of a slot's output rings (dabstar_amd/csrc/out_ring.h), restated: of items with byte positions byte_pos and n_bytes bytes in
    all, (first by the record ring alone, first still intact).  An item is trusted while the record ring still holds its record and
    n_bytes + asm_room - byte_pos fits the byte ring -- the device may have written that far beyond n_bytes."""
    by_records = max(0, len(byte_pos) - ring_records)
    first = by_records
    while first < len(byte_pos) and n_bytes + asm_room - int(byte_pos[first]) > ring_bytes:
        first += 1
    return by_records, first


# ---- the sets the tests use --------------------------------------------------------------------------------------------------------------
PROT = 3                                     # EEP 4-A, as tests/dabplus_cases.py
# (kbps, kind) per slot: "pkt" a packet-mode slot, "dab+" a DAB+ slot, "plain" a slot left in plain logical frames that carries a packet
# scenario all the same (the stage must not look at it)
STAGE_LAYOUTS = [
    [(8, "pkt"), (64, "dab+"), (16, "pkt"), (32, "plain"), (128, "pkt")],
    [(384, "pkt"), (64, "pkt"), (32, "pkt"), (24, "dab+")],
]
STAGE_STREAMS = [(0, ADDRESS_A), (0, ADDRESS_B), (1, ADDRESS_A), (1, ADDRESS_B)]      # (layout, packet address of its packet slots)


def seed_of(stream, slot):
    return 10 * stream + slot


def all_scenarios():
    """Every (kbps, seed) the GPU stage test runs as a packet scenario, with the address it is read with."""
    out = []
    for s, (lay, address) in enumerate(STAGE_STREAMS):
        for j, (kbps, kind) in enumerate(STAGE_LAYOUTS[lay]):
            if kind == "pkt":
                out.append((kbps, seed_of(s, j), address))
    return out


def boundary_schedule(n_streams, n_frames=N_FRAMES):
    """[batch][stream] CIF counts: stream s walks through BOUNDARY_COUNTS from place s on until it has had n_frames."""
    left, out, b = [n_frames] * n_streams, [], 0
    while any(left):
        row = [min(BOUNDARY_COUNTS[(b + s) % len(BOUNDARY_COUNTS)], left[s]) for s in range(n_streams)]
        left = [a - c for a, c in zip(left, row)]
        out.append(row)
        b += 1
    return out


# ---- soft bits and the oracle's results for the GPU stage test (tests/dabplus_cases.py's tools, by import) -------------------------------
def stage_layout(lay):
    import dabplus_cases as dc
    kinds = STAGE_LAYOUTS[lay]
    return dc.dabplus_layout([(k, PROT, 0) for k, _ in kinds], dab_plus=[int(kind == "dab+") for _, kind in kinds])


def slot_frames(s, j, kbps, kind, n_frames=N_FRAMES):
    """The intended logical frames of slot j of stream s: a packet scenario ("pkt", "plain") or a DAB+ scenario of dabplus_cases."""
    if kind == "dab+":
        import dabplus_cases as dc
        return dc.build_scenario(kbps // 8, seed_of(s, j))[0][:n_frames]        # the beginning of its 196 frames
    return scenario(kbps, seed_of(s, j), n_frames)


_stage_cache = {}


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16, per-slot oracle results) of stream s of STAGE_STREAMS.
    Cached: the tests of one process share the arrays and leave them unchanged."""
    if s not in _stage_cache:
        import dabplus_cases as dc
        lay = STAGE_STREAMS[s][0]
        layout = stage_layout(lay)
        frames = [slot_frames(s, j, kbps, kind) for j, (kbps, kind) in enumerate(STAGE_LAYOUTS[lay])]
        cifs = dc.cifs_of(layout, frames, np.random.default_rng([9, s]))
        _stage_cache[s] = (layout, frames, cifs, dc.oracle_results(layout, cifs))
    return _stage_cache[s]
