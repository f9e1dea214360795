"""Shared by test_mot_cases.py (no device) and the GPU tests of the MOT stage (k_mot): the tail of PadHandler::_build_MSC_segment
(base/backend/data/pad_handler.cpp:539-622, cited as ph:) and the handler's one MotObject (base/backend/data/mot/mot_object.cpp:71-323,
cited as mo:; constructed at pad_handler.cpp:54 as a PAD element that is no directory element) restated in plain Python -- the model every
device result is compared with, exactly -- and builders that put crafted MSC data groups into the X-PADs of DAB+ access units with the
helpers of tests/pad_cases.py.  The oracle (oracle/) has no MotObject and mot_object.cpp cannot be compiled without the GUI's headers, so
the model lives here; every branch cites the line it restates and counts itself in `branch`.  Three guards go beyond the reference
(include/dabx.h, M1..M3)."""
import collections

import numpy as np

import dabplus_cases as dc
import pad_cases as pc
from pad_cases import Script, crc16_fast, group_fields, unit, var_ci  # noqa: F401
from dabstar_amd.lib import MOT_COUNTERS, MOT_OBJECT, PAD_DATAGROUP, PAD_ITEM, SUPERFRAME_INFO

import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

BATCH = dc.BATCH
N_BATCHES = 8
N_FRAMES = N_BATCHES * BATCH
NON_ADVANCING = (2, 3, 4, 5, 6, 7, 8, 0x0A, 0x0B, 0x0F)        # mo:191-200


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class MotModel:
    """_build_MSC_segment from ph:539 on and MotObject for ONE slot.  item() takes one PAD item (a PAD_ITEM row and its bytes) after the
    other; rows / payloads: one MOT_OBJECT row and one bytes object (body, then name) per signal_new_mot_object; counters: dabx_mot_stats;
    branch: how often each reference line / guard was reached."""

    def __init__(self, max_object_bytes=65536):
        self.max_object_bytes = max_object_bytes
        self.transport_id = -1                   # mTransportId, mot_object.h:82
        self.progress_pct = 0
        self.n = dict.fromkeys(MOT_COUNTERS, 0)
        self.branch = collections.Counter()
        self.rows, self.payloads, self.progress = [], [], []
        self.frame = self.au = 0
        self._clear()
        self.branch.clear()
        self.n["resets"] = 0

    def hit(self, line):
        self.branch[line] += 1

    @property
    def counters(self):
        c = dict(self.n)
        c.update(objects=len(self.rows), object_bytes=sum(len(p) for p in self.payloads), progress_pct=self.progress_pct,
                 transport_id=self.transport_id, segments_stored=len(self.map))
        return c

    def _clear(self):
        """reset(), mo:313-323"""
        self.num_segments, self.sum = -1, 0      # mNumOfSegments, mSumSegmentSize
        self.core = None                         # mHeaderCore: (bodySize, headerSize, contentType, contentSubType) once initialized
        self.name = b""                          # mName
        self.map = {}                            # mMotMap
        self.emits = 0
        self.n["resets"] += 1
        self.hit("mo:313 reset")

    # -- ph:522-622 --------------------------------------------------------------------------------------------------------------------------
    def item(self, rec, data):
        if int(rec["kind"]) != PAD_DATAGROUP:
            return
        self.frame, self.au = int(rec["frame"]), int(rec["au"])
        self.group(bytes(data), int(rec["crc_flag"]), int(rec["crc_ok"]))

    def _short(self, what):
        self.n["grp_short"] += 1
        self.hit("M1 " + what)

    def group(self, d, flag, ok):
        n = len(d)                                                              # ph:528 size
        self.n["groups"] += 1
        if flag and not ok:                                                     # ph:539-545
            self.n["crc_bad"] += 1
            self.hit("ph:543 bad CRC")
            return
        self.hit("ph:546 good CRC" if flag else "ph:550 no CRC flag")
        b0 = d[0]
        typ = b0 & 0x0F                                                         # ph:554
        if typ not in (3, 4):                                                   # ph:556-560
            self.n["type_other"] += 1
            self.hit("ph:558 type %d" % typ)
            return
        index = 4 if b0 & 0x80 else 2                                           # ph:564
        self.hit("ph:564 extension flag %d" % (b0 >> 7))
        number, last = -1, False                                                # ph:553, :565
        if b0 & 0x20:                                                           # ph:567
            if index + 2 > n:
                return self._short("segment field")
            last = bool(d[index] & 0x80)                                        # ph:569
            number = (d[index] & 0x7F) << 8 | d[index + 1]                      # ph:570
            index += 2
            self.hit("ph:567 segment field")
        else:
            self.hit("ph:567 no segment field")
        tid, tid_flag = 0, False                                                # ph:575-576
        if b0 & 0x10:                                                           # ph:579
            if index + 1 > n:
                return self._short("user access field")
            li = d[index] & 0x0F                                                # ph:582
            tid_flag = bool(d[index] & 0x10)                                    # ph:583
            if tid_flag:
                if index + 3 > n:
                    return self._short("transport id")
                tid = d[index + 1] << 8 | d[index + 2]                          # ph:587, whatever lengthIndicator says
                self.hit("ph:587 transport id, length indicator %s" % (li if li in (0, 1, 2, 15) else "other"))
            index += 1 + li                                                     # ph:589
        else:
            self.hit("ph:579 no user access field")
        if not tid_flag:                                                        # ph:593-597
            self.n["no_tid"] += 1
            self.hit("ph:595 no transport id")
            return
        if index + 2 > n:
            return self._short("segmentation header")
        segsize = (d[index] & 0x1F) << 8 | d[index + 1]                         # ph:605
        end = index + 2 + segsize
        if end > n:
            return self._short("segment one byte beyond length" if end == n + 1 else "segment beyond length")
        if end == n:
            self.hit("M1 segment ends exactly at length")
        seg = d[index + 2:end]
        if typ == 3:                                                            # ph:611-613
            self.set_header(seg, tid)
        else:                                                                   # ph:615-617
            self.add_body_segment(seg, number, last, tid)

    # -- mo:71-115, :177-238 -------------------------------------------------------------------------------------------------------------------
    def _bad(self, what):
        self.n["hdr_bad"] += 1
        self.hit("M2 " + what)

    def set_header(self, seg, tid):
        size = len(seg)
        if size < 7:                                                            # M2: no header core; state unchanged
            return self._bad("segment of %s bytes" % (size if size == 6 else "fewer than 6"))
        if size == 7:
            self.hit("M2 segment of 7 bytes")
        if self.transport_id != tid:                                            # mo:75-79
            self.hit("mo:75 transport id changes at a header" + (", object under way" if self.map or self.core else ""))
            self._clear()
        self.transport_id = tid                                                 # mo:81
        v = int.from_bytes(seg[:7], "big")
        self.core = (v >> 28, (v >> 15) & 0x1FFF, (v >> 9) & 0x3F, v & 0x1FF)   # mo:84-87
        self.n["headers"] += 1
        header_size = self.core[1]
        p = 7                                                                   # mo:99
        while p < header_size:                                                  # mo:101
            if p >= size:
                self._bad("parameter byte beyond the segment")
                break
            pli, pid = seg[p] >> 6, seg[p] & 0x3F                               # mo:212-213
            if pli < 3:                                                         # mo:219-221
                p += (1, 2, 5)[pli]
                self.hit("mo:219 PLI %d" % pli)
                continue
            if p + 1 >= size:
                self._bad("length byte beyond the segment")
                break
            if seg[p + 1] & 0x80:                                               # mo:223-227
                if p + 2 >= size:
                    self._bad("second length byte beyond the segment")
                    break
                length, q = (seg[p + 1] & 0x7F) << 8 | seg[p + 2], p + 3
                self.hit("mo:225 PLI 3, 15-bit length")
            else:                                                               # mo:228-232
                length, q = seg[p + 1] & 0x7F, p + 2
                self.hit("mo:230 PLI 3, 7-bit length")
            if pid == 0x0C:                                                     # mo:181-189
                if length >= 2 and q + length > size:
                    self._bad("name one byte beyond the segment" if q + length == size + 1 else "name beyond the segment")
                    break
                if length >= 2 and q + length == size:
                    self.hit("M2 name ends exactly at the segment's end")
                self.hit("mo:182 ContentName%s%s" % (" replaces a name" if self.name else "", ", empty" if length < 2 else ""))
                self.name = bytes(seg[q + 1:q + length]) if length >= 2 else b""
                p = q + length                                                  # mo:188
            elif pid in NON_ADVANCING:                                          # mo:191-201: the pointer stays in front of the value
                self.hit("mo:201 parameter whose value is walked")
                p = q
            else:                                                               # mo:203-206
                self.hit("mo:204 unknown parameter")
                p = q + length
        else:
            self.hit("mo:106 pointer %s headerSize" % ("==" if p == header_size else "!="))
        self.hit("mo:111 header")
        if self._check_if_complete():                                           # mo:111-114
            self._handle_complete()

    # -- mo:117-175 ----------------------------------------------------------------------------------------------------------------------------
    def add_body_segment(self, seg, number, last, tid):
        if number < 0 or number >= 8192:                                        # mo:119-123
            self.n["seg_number_bad"] += 1
            self.hit("mo:121 segment number %s" % ("-1" if number < 0 else "8192" if number == 8192 else "above 8192"))
            return
        if self.transport_id != tid:                                            # mo:125-130
            self.hit("mo:125 transport id changes at a body segment" + (", object under way" if self.map or self.core else ""))
            self._clear()
            self.transport_id = tid
        if number in self.map:                                                  # mo:139-143
            self.n["seg_duplicate"] += 1
            self.hit("mo:141 duplicate segment")
            return
        if self.sum + len(seg) > self.max_object_bytes:                         # M3
            self.hit("M3 one byte beyond max_object_bytes" if self.sum + len(seg) == self.max_object_bytes + 1 else "M3 beyond max_object_bytes")
            self._clear()                                                       # the transport id just set stays
            self.n["obj_overflow"] += 1
            return
        self.map[number] = bytes(seg)                                           # mo:135-137
        self.sum += len(seg)
        self.n["segments"] += 1
        if self.sum == self.max_object_bytes:
            self.hit("M3 exactly max_object_bytes")
        if number == 8191:
            self.hit("mo:119 segment number 8191")
        if last:                                                                # mo:145-148
            self.hit("mo:147 last flag" + (" moves" if self.num_segments >= 0 and self.num_segments != number + 1 else ""))
            self.num_segments = number + 1
        if self.core and self.core[0] > 0 and self.core[2] == 2:                # mo:160: base type image, ((contentType << 8) & 0x3f00) >> 8 == 2
            pct = 100 * self.sum // self.core[0]                                # mo:162
            if pct > 100:                                                       # mo:163-167
                pct = 100
                self.hit("mo:165 progress clamped")
            self.progress_pct = pct                                             # mo:168
            self.n["progress_events"] += 1
            self.progress.append(pct)
            self.hit("mo:168 progress")
        else:
            self.hit("mo:160 no progress: %s" % ("no header yet" if not self.core else "bodySize 0" if self.core[0] == 0 else "not an image"))
        if self._check_if_complete():                                           # mo:171-174
            self._handle_complete()

    def _check_if_complete(self):
        if not self.core:                                                       # mo:242
            self.hit("mo:244 no header core")
            return False
        if self.num_segments < 0:                                               # mo:248
            self.hit("mo:250 number of segments unknown")
            return False
        if len(self.map) < self.num_segments:                                   # mo:254
            self.hit("mo:256 fewer segments than needed")
            return False
        if any(i not in self.map for i in range(self.num_segments)):            # mo:262-275
            self.hit("mo:273 a segment below the last is missing")
            return False
        return True

    def _handle_complete(self):
        body = b"".join(self.map[k] for k in sorted(self.map))                  # mo:286-291: ALL stored segments in key order
        if any(k >= self.num_segments for k in self.map):
            self.hit("mo:288 a segment numbered beyond the last is emitted")
        self.hit("mo:300 emit, repeat %s" % (self.emits if self.emits < 3 else "3 and more"))
        self.hit("mo:293 no name" if not self.name else "mo:300 with a name")
        content = ((self.core[2] << 8) & 0x3F00) | (self.core[3] & 0xFF)        # mot_object.h:71-75
        self.rows.append((sum(len(p) for p in self.payloads), self.frame, len(body), self.core[0], self.transport_id & 0xFFFF, content,
                          len(self.name), self.au, min(self.emits, 255)))
        self.payloads.append(body + self.name)
        self.emits += 1                                                         # (nothing is cleared: mo:313 is reached by a new transport id only)

    def records(self):
        return np.array(self.rows, MOT_OBJECT) if self.rows else np.zeros(0, MOT_OBJECT)

    def all_bytes(self):
        return np.frombuffer(b"".join(self.payloads), np.uint8)


def run_model(rec, by, max_object_bytes=65536):
    """The model on PAD items: [n] PAD_ITEM (byte_pos counted from by[0]) and their bytes."""
    m = MotModel(max_object_bytes)
    by = bytes(np.asarray(by, np.uint8))
    for r in rec:
        m.item(r, by[int(r["byte_pos"]):int(r["byte_pos"]) + int(r["length"])])
    return m


def groups_only(groups):
    """(None in a scenario: an access unit that stays without PAD)"""
    return [g for g in groups if g is not None]


def items_of(groups):
    """PAD items as k_pad emits them for these groups (bytes objects), one per access unit of consecutive super frames."""
    rows, at = [], 0
    groups = groups_only(groups)
    for k, g in enumerate(groups):
        flag = (g[0] >> 6) & 1
        rows.append((at, 5 * (k // 3), len(g), PAD_DATAGROUP, k % 3, 0, flag, int(pc.check_crc_bytes(g, len(g) - 2)), [0] * 9))
        at += len(g)
    return np.array(rows, PAD_ITEM), np.frombuffer(b"".join(groups), np.uint8)


# ---- MSC data groups and MOT segments, as the reference reads them --------------------------------------------------------------------------
def msc_group(typ, segment, tid=None, number=None, last=False, ext=False, ua=True, li=2, crc=True, good=True, size=None, rng=None):
    """One MSC data group (EN 300 401 5.3.3): header, [extension], [segment field], [user access field with `li` bytes behind its length
    byte], the segmentation header (size: what it claims, default the segment's length), the segment and two CRC bytes."""
    rng = rng or np.random.default_rng(0)
    b0 = typ | (int(ua) << 4) | (int(number is not None) << 5) | (int(crc) << 6) | (int(ext) << 7)
    g = bytearray([b0, int(rng.integers(0, 256))])
    if ext:
        g += rng.integers(0, 256, 2).astype(np.uint8).tobytes()
    if number is not None:
        g += bytes([(0x80 if last else 0) | number >> 8, number & 0xFF])
    if ua:
        g.append((0x10 if tid is not None else 0) | li | int(rng.integers(0, 8)) << 5)
        t = bytes([tid >> 8, tid & 0xFF]) if tid is not None else b""
        g += (t + rng.integers(0, 256, 16).astype(np.uint8).tobytes())[:li]
    size = len(segment) if size is None else size
    g += bytes([int(rng.integers(0, 8)) << 5 | size >> 8, size & 0xFF]) + bytes(segment)
    c = crc16_fast(bytes(g)) ^ (0 if good else 0x0400)
    return bytes(g) + bytes([c >> 8, c & 0xFF])


def param(pid, data=b"", pli=3, long=False):
    """One header-extension parameter (EN 301 234 6.2): PLI 0 / 1 / 2 with 0 / 1 / 4 data bytes, PLI 3 with a 7- or 15-bit length."""
    if pli < 3:
        assert len(data) == (0, 1, 4)[pli]
        return bytes([pli << 6 | pid]) + bytes(data)
    n = len(data)
    return bytes([0xC0 | pid]) + (bytes([0x80 | n >> 8, n & 0xFF]) if long or n > 127 else bytes([n])) + bytes(data)


def name_param(name, long=False):
    return param(0x0C, b"\x04" + name, long=long)              # the character-set byte, then the name (mo:183-186 skips the first byte)


def mot_header(body_size, params=(), content_type=2, subtype=1, header_size=None, cut=None):
    """A MOT header segment: the 7-byte core and the extension; header_size: what the core claims (default: what there is); cut: the segment
    ends after that many bytes."""
    ext = b"".join(params)
    hs = 7 + len(ext) if header_size is None else header_size
    seg = (body_size << 28 | hs << 15 | content_type << 9 | subtype).to_bytes(7, "big") + ext
    return seg if cut is None else seg[:cut]


# ---- the scenarios: groups in order ----------------------------------------------------------------------------------------------------------
class Groups:
    def __init__(self, seed):
        self.rng = np.random.default_rng([seed, 815])
        self.out = []

    def rand(self, n):
        return self.rng.integers(0, 256, n).astype(np.uint8).tobytes()

    def hdr(self, tid, body_size, params=(), **kw):
        g = {k: kw.pop(k) for k in ("content_type", "subtype", "header_size", "cut") if k in kw}
        self.out.append(msc_group(3, mot_header(body_size, params, **g), tid, rng=self.rng, **kw))

    def body(self, tid, number, n, last=False, **kw):
        self.out.append(msc_group(4, self.rand(n), tid, number, last, rng=self.rng, **kw))

    def obj(self, tid, lengths, params=(), **kw):
        """A complete object: header, then its segments in order."""
        self.hdr(tid, sum(lengths), params, **kw)
        for k, n in enumerate(lengths):
            self.body(tid, k, n, last=k == len(lengths) - 1)

    def raw(self, g):
        self.out.append(bytes(g))


def placement_groups(seed):
    """Transport ids, segment placement, the forms of the group header, guard M1, progress; and one object of 3 000 bytes (64 kbit/s slot)."""
    s = Groups(seed)
    r = s.rng
    s.body(1, 0, 40)                                            # a first body segment: no header core yet (mo:244), id -1 -> 1
    s.hdr(1, 100, [name_param(b"one.jpg")])                     # the header between the body segments
    s.body(1, 1, 60, last=True)
    s.hdr(1, 100, [name_param(b"one.jpg")])                     # a repeated header of a complete object emits it again: repeat 1, 2, 3
    s.hdr(1, 100, [name_param(b"one.jpg")])
    s.hdr(1, 100)
    s.body(2, 0, 25)                                            # the header after the body segments; the id changes at a body segment
    s.body(2, 1, 200, last=True)
    s.hdr(2, 225)                                               # no name: the host's trid_2
    s.obj(3, [20, 30, 50], [name_param(b"three.png")])          # the header before
    s.hdr(4, 180, content_type=0)                               # out of order, a duplicate, not an image: no progress
    s.body(4, 2, 70, last=True)
    s.body(4, 0, 50)
    s.body(4, 0, 51)
    s.body(4, 1, 60)
    s.hdr(5, 90)                                                # segment 1 never comes: as many segments as needed, no object (mo:273) ...
    s.body(5, 0, 30)
    s.body(5, 3, 30)
    s.body(5, 2, 30, last=True)
    s.hdr(6, 0)                                                 # ... and a header with another id resets it.  bodySize 0: no progress
    s.body(6, 3, 33)                                            # numbered beyond the last: emitted with the rest
    s.body(6, 0, 20)
    s.body(6, 1, 21, last=True)
    s.hdr(7, 100)                                               # a last flag that moves: 1, then 3
    s.body(7, 1, 25, last=True)
    s.body(7, 3, 25, last=True)
    s.body(7, 0, 25)
    s.body(7, 2, 25)
    s.hdr(8, 50)                                                # the id changes in the middle of an object, at a body segment
    s.body(8, 0, 30)
    s.body(9, 0, 30)
    s.body(9, 1, 30, last=True)
    s.hdr(9, 60)
    s.hdr(10, 40)                                               # progress beyond 100 %: more bytes than bodySize
    s.body(10, 0, 30)
    s.body(10, 1, 30)
    s.body(10, 2, 30, last=True)
    # the forms of the group header
    s.hdr(11, 24, ext=True)
    s.body(11, 0, 24, last=True, ext=True)
    s.out.append(msc_group(3, mot_header(30), 12, rng=r))       # a header without segment field
    s.out.append(msc_group(4, s.rand(30), 12, rng=r))           # a body segment without: number -1
    s.body(12, 0, 30, last=True)
    s.out.append(msc_group(4, s.rand(20), None, 0, True, ua=False, rng=r))      # no user access field
    s.out.append(msc_group(4, s.rand(20), None, 0, True, li=2, rng=r))          # a user access field without transport id
    for li in (0, 1, 15, 7):                                    # the id is read from the two bytes behind the length byte whatever li says
        s.hdr(20 + li, 22, li=li)
        s.out.append(msc_group(4, s.rand(22), 20 + li, 0, True, li=li, rng=r))
    s.obj(13, [20, 21], crc=False)                              # without CRC flag: taken as it is
    s.body(13, 5, 20, good=False)                               # a bad CRC: dropped
    s.out.append(msc_group(0, s.rand(20), 13, 6, rng=r))        # types 0 and 6
    s.out.append(msc_group(6, s.rand(20), 13, 6, rng=r))
    s.body(14, 8191, 20)                                        # the largest segment number, and the first that is refused
    s.body(14, 8192, 20)
    s.body(14, 0x7FFF, 20)
    # M1
    s.body(15, 0, 40)
    g = msc_group(4, s.rand(38), 15, 1, True, size=40, crc=False, rng=r)        # the segment takes the two CRC bytes: ends exactly at length
    s.raw(g)
    s.hdr(15, 80)
    g = msc_group(4, s.rand(38), 15, 2, size=41, crc=False, rng=r)              # one byte beyond
    s.raw(g)
    s.raw(msc_group(4, s.rand(20), 15, 2, size=4000, crc=False, rng=r))         # far beyond
    s.raw(bytes([0xB4, 0x00, 0x01]))                            # extension + segment flag: the segment field lies beyond 3 bytes
    s.raw(bytes([0x14, 0x00]))                                  # user access flag: its length byte lies beyond
    s.raw(bytes([0x14, 0x00, 0x12, 0x00]))                      # ... the transport id does
    s.raw(bytes([0x14, 0x00, 0x12, 0x00, 0x09]))                # ... the segmentation header does
    # one object of 3 000 bytes in 25 segments, its header in the middle, an access unit without PAD behind every segment (None): it
    # takes some 90 logical frames, three batches
    for k in range(25):
        if k == 9:
            s.hdr(30, 3000, [name_param(b"slide-30.jpg")])
        s.body(30, k, 120, last=k == 24)
        s.out.append(None)
    s.hdr(30, 3000, [name_param(b"slide-30.jpg")])
    return s.out


def header_groups(seed):
    """The header extension walk, guard M2 and guard M3 with max_object_bytes = 4 096 (192 kbit/s slot)."""
    s = Groups(seed)
    r = s.rng
    four = s.rand(4)
    s.obj(40, [50, 60], [param(0x21, pli=0), param(0x25, b"\x07", pli=1), param(0x29, four, pli=2), name_param(b"every-pli.jpg")])
    s.obj(41, [40], [name_param(b"long-form", long=True), param(0x30, s.rand(9))])                    # 15-bit length; an unknown parameter
    s.obj(42, [40], [name_param(b"first"), name_param(b"second.jpg")])                                # a second name replaces the first
    s.obj(43, [40], [name_param(b"gone"), name_param(b"")])                                           # ... an empty one too
    s.obj(44, [40], [param(0x0C, b"")])                                                               # length 0: mo:183 loops to -1
    # triggerTime's value is walked as parameters: its first byte reads as ContentName with length 4
    s.obj(45, [40], [param(0x05, bytes([0xCC, 0x04, 0x04]) + b"tri")])
    s.obj(46, [40], [param(0x0F, bytes([0x01, 0x41, 0x00]))])                                         # ... here as PLI 0 and PLI 1
    s.obj(47, [40], [name_param(b"short-claim")], header_size=9)                                      # headerSize inside a parameter: the walk ends beyond it
    s.obj(48, [40], [name_param(b"never-read")], header_size=7)                                       # no extension as far as the core says
    s.obj(49, [40], [name_param(b"segmented")], header_size=200)                                      # a header longer than its segment (M2)
    # M2
    s.hdr(50, 40, cut=6)
    s.hdr(50, 40, cut=5)
    s.hdr(50, 40, [param(0x21, pli=0)], cut=7)                                                        # the core alone: the parameter byte is beyond
    s.body(50, 0, 40, last=True)
    s.hdr(51, 40, [name_param(b"exact")])                                                             # a name that ends exactly at the segment's end
    s.hdr(51, 40, [name_param(b"beyond")], cut=7 + 2 + 1 + 5)                                         # ... one byte beyond: not applied
    s.hdr(51, 40, [name_param(b"far-beyond")], cut=7 + 2 + 1 + 2)
    s.hdr(51, 40, [name_param(b"x")], cut=8)                                                          # the length byte is beyond
    s.hdr(51, 40, [name_param(b"y", long=True)], cut=9)                                               # the second length byte is
    s.body(51, 0, 40, last=True)
    # M3: exactly max_object_bytes, one byte beyond, far beyond
    s.hdr(60, 4096, [name_param(b"full.jpg")])
    for k in range(4):
        s.body(60, k, 1024, last=k == 3)
    s.body(60, 4, 1)
    s.body(60, 0, 1000)                                                                               # the table is empty again: no duplicate
    s.body(60, 1, 3000)
    s.body(60, 2, 1000)
    s.obj(61, [100, 100], [name_param(b"after.jpg")])
    # traffic nobody crafted: random bytes behind a plausible first byte, good CRCs
    for _ in range(40):
        n = int(r.integers(3, 120))
        g = bytearray(s.rand(n))
        g[0] = (g[0] & 0xB0) | 0x40 | int(r.choice([3, 4]))
        c = crc16_fast(bytes(g))
        s.raw(bytes(g) + bytes([c >> 8, c & 0xFF]))
    s.obj(62, [30, 31, 32], [name_param(b"last.jpg")])
    return s.out


# ---- super frames whose access units carry the groups ------------------------------------------------------------------------------------------
LAYOUTS = {64: (3, 4, 2), 192: (6,)}              # access units per super frame, cycled: each holds an X-PAD of 196 bytes
ROOM = 196


def units_of(groups, seed, size=48, per_unit=1):
    """The access units' PADs: every group behind its length indicator in sub-fields of `size` bytes, four contents indicators per X-PAD;
    per_unit: the sub-fields of that many groups are packed together (two groups of at most `size` bytes share an X-PAD)."""
    s = Script(np.random.default_rng([seed, 4712]), ROOM)
    fs, k = [], 0
    for g in groups:
        if g is None:
            s.units.append(None)                 # an access unit that stays without PAD
            continue
        fs += group_fields(s.rng, g, [size])
        k += 1
        if k % per_unit == 0:
            s.fields(fs)
            fs = []
    if fs:
        s.fields(fs)
    return s.units


def overrun_groups(seed, repeats):
    """One object of 250 bytes and `repeats` repeated headers: each emits it again (mo:111-114), far more bytes than small rings hold."""
    s = Groups(seed)
    s.obj(77, [125, 125], content_type=0)
    for _ in range(repeats):
        s.hdr(77, 250, content_type=0)
    return s.out


def build_frames(kbps, units, seed, n_frames=N_FRAMES):
    """(frames [n_frames, 3 kbps], super frames, SUPERFRAME_INFO records): clean super frames, one unit per access unit that holds it, in
    order; all units must find their place."""
    R = kbps // 8
    rng = np.random.default_rng([kbps, seed, 98])
    end, nb = 110 * R, 24 * R
    out, sfs, sfi = [], [], np.zeros(n_frames // 5, SUPERFRAME_INFO)
    at = 0
    for n_sf in range(n_frames // 5):
        n_au = LAYOUTS[kbps][n_sf % len(LAYOUTS[kbps])]
        sf = rng.integers(0, 256, end).astype(np.uint8)
        dac, sbr = dc.AU_MODE[n_au]
        sf[2] = (int(sf[2]) & 0x9F) | (dac << 6) | (sbr << 5)
        starts = dc._au_starts(R, rng, n_au, "even")
        nib = [v for f in starts for v in (f >> 8, (f >> 4) & 15, f & 15)]
        for i, v in enumerate(nib):
            b = 3 + i // 2
            sf[b] = (int(sf[b]) & 0x0F) | (v << 4) if i % 2 == 0 else (int(sf[b]) & 0xF0) | v
        au = [dc.AU_HEAD[n_au]] + starts + [end]
        for a in range(n_au):
            st, ln = au[a], au[a + 1] - au[a] - 2
            sf[st] = (int(sf[st]) & 0x1F) | (int(rng.choice([0, 1, 2, 3, 5, 6, 7])) << 5)       # no PAD unless a unit is placed
            if at < len(units) and units[at] is None:
                at += 1
            elif at < len(units) and 2 + units[at]["count"] <= ln:
                u = units[at]
                at += 1
                sf[st] = (int(sf[st]) & 0x1F) | (4 << 5)
                sf[st + 1] = u["count"]
                sf[st + 2:st + 2 + u["count"]] = np.frombuffer(u["body"], np.uint8)
            c = crc16_fast(sf[st:st + ln])
            sf[st + ln], sf[st + ln + 1] = c >> 8, c & 0xFF
        fc = ds.firecode_parity(bytes(sf[2:11]))
        sf[0], sf[1] = fc >> 8, fc & 0xFF
        full = np.zeros(120 * R, np.uint8)
        full[:end] = sf
        full[end:] = pc.rs_parity_columns(sf.reshape(110, R)).reshape(-1)
        out.extend(full.reshape(5, nb))
        sfs.append(sf.copy())
        rec = sfi[n_sf]
        rec["num_aus"], rec["au_crc_ok"], rec["stream_parms"], rec["first_frame"] = n_au, (1 << n_au) - 1, int(sf[2]) & 0x7F, 5 * n_sf
        rec["au_start"][:n_au + 1] = au
    assert at == len(units), "%d of %d units placed in %d frames at %d kbit/s" % (at, len(units), n_frames, kbps)
    while len(out) < n_frames:
        out.append(rng.integers(0, 256, nb).astype(np.uint8))
    return np.stack(out), np.stack(sfs), sfi


# ---- the sets the tests use ------------------------------------------------------------------------------------------------------------------
PROT = pc.PROT
# (kbps, kind) per slot: "mot" a DAB+ PAD slot with MOT decoding, "pad" a DAB+ PAD slot without (tests/pad_cases.py's scenario), "dab+" a
# plain DAB+ slot, "pkt" a packet-mode slot (tests/packet_cases.py)
STAGE_LAYOUT = [(64, "mot"), (192, "mot"), (32, "pad"), (32, "dab+"), (16, "pkt")]
N_STREAMS = 2
MAX_OBJECT_BYTES = {0: 0, 1: 4096}               # per "mot" slot: dabx_mot_config.max_object_bytes (0 = 65 536)
PACKET_ADDRESS = pc.PACKET_ADDRESS


def max_bytes_of(j):
    return MAX_OBJECT_BYTES[j] or 65536


def slot_groups(s, j):
    return placement_groups(100 + s) if j == 0 else header_groups(200 + s)


_cache = {}


def mot_frames(s, j):
    """(frames, super frames, records) of MOT slot j of stream s."""
    if (s, j) not in _cache:
        _cache[(s, j)] = build_frames(STAGE_LAYOUT[j][0], units_of(slot_groups(s, j), 10 * s + j), 10 * s + j)
    return _cache[(s, j)]


def stage_layout():
    return pc.dabplus_layout([(k, PROT, 0) for k, _ in STAGE_LAYOUT], dab_plus=[int(kind != "pkt") for _, kind in STAGE_LAYOUT])


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16, per-slot oracle results) of stream s.  Cached: the
    tests of one process share the arrays and leave them unchanged."""
    if ("case", s) not in _cache:
        import packet_cases as pkc
        layout = stage_layout()
        frames = []
        for j, (kbps, kind) in enumerate(STAGE_LAYOUT):
            frames.append(mot_frames(s, j)[0] if kind == "mot" else pkc.scenario(kbps, 10 * s + j, N_FRAMES) if kind == "pkt"
                          else pc.scenario(kbps, 10 * s + j, N_FRAMES)[0])
        cifs = pc.cifs_of(layout, frames, np.random.default_rng([12, s]))
        _cache[("case", s)] = (layout, frames, cifs, pc.oracle_results(layout, cifs))
    return _cache[("case", s)]


def pad_model_of(sfs, sfi):
    return pc.run_model(sfs, sfi)


def mot_model_of(pad_model, max_object_bytes):
    """MotModel on the items of a PadModel."""
    m = MotModel(max_object_bytes)
    for row, data in zip(pad_model.records(), pad_model.payloads):
        m.item(row, data)
    return m
