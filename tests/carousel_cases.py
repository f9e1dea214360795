"""Shared by test_carousel_cases.py (no device) and the GPU tests of the carousel stage (k_carousel): MotHandler::add_MSC_data_group with its
cache (base/backend/data/mot/mot_handler.cpp:69-259, cited as mh:) and MotDirectory (base/backend/data/mot/mot_dir.cpp:28-156, md:) restated
in plain Python around the MotObject of tests/mot_cases.py (mo:) -- the model every device result is compared with, exactly -- and builders
that put crafted MSC data groups into the packets of a packet-mode sub-channel with the helpers of tests/packet_cases.py.  The model keeps a
dict of objects, each a dict of bytes joined in sorted key order; nothing of it follows the kernel's stores, tables or ballots.
mot_handler.cpp cannot be compiled without the GUI's headers, so the model lives here; every branch cites the line it restates and counts
itself in `branch`.  The guards C1..C3 and D1..D4 go beyond the reference (include/dabx.h)."""
import collections

import numpy as np

import mot_cases as mc
import packet_cases as pkc
from mot_cases import mot_header, msc_group, name_param, param  # noqa: F401
from packet_cases import Writer
from dabstar_amd.lib import CAROUSEL_COUNTERS, DATAGROUP_INFO, MOT_FLAG_DIR_ELEMENT, MOT_OBJECT

BATCH = pkc.BATCH
N_BATCHES = 8
N_FRAMES = N_BATCHES * BATCH
ADDRESS = pkc.ADDRESS_A
CACHE = 15                                       # mot_handler.h:60
DIR_SEGMENTS = 512                               # mot_dir.h:56
NAME_ROOM = 8192


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class _Object(mc.MotModel):
    """One MotObject of the handler: mot_cases.MotModel's set_header and completeness check as they are, add_body_segment without the
    progress signal (mIsPadElement is false, mo:160); counters, branches and emitted objects are the handler's.  The X-PAD model's guard
    names M2 / M3 are this stage's C2 / C3."""

    def __init__(self, handler, dir_element):
        self.handler, self.dir_element = handler, dir_element
        self.max_object_bytes = handler.max_object_bytes
        self.transport_id, self.progress_pct, self.progress = -1, 0, []      # mot_object.h:82: a fresh object, reset by its first set_header
        self.n, self.branch, self.rows, self.payloads = handler.n, handler.branch, handler.rows, handler.payloads
        self.num_segments, self.sum, self.core, self.name, self.map, self.emits = -1, 0, None, b"", {}, 0

    def hit(self, line):
        self.branch[("C" + line[1:]) if line[:3] in ("M2 ", "M3 ") else line] += 1

    def add_body_segment(self, seg, number, last, tid):
        if number < 0 or number >= 8192:                                        # mo:119-123
            self.n["seg_number_bad"] += 1
            self.hit("mo:121 segment number %s" % ("8192" if number == 8192 else "above 8192"))
            return
        if self.transport_id != tid:                                            # mo:125-130 (a handle is found by its id: never here)
            self.hit("mo:125 transport id changes at a body segment")
            self._clear()
            self.transport_id = tid
        if number in self.map:                                                  # mo:139-143
            self.n["seg_duplicate"] += 1
            self.hit("mo:141 duplicate segment")
            return
        if self.sum + len(seg) > self.max_object_bytes:                         # C3
            self.hit("C3 one byte beyond max_object_bytes" if self.sum + len(seg) == self.max_object_bytes + 1 else "C3 beyond max_object_bytes")
            self._clear()
            self.n["obj_overflow"] += 1
            return
        self.map[number] = bytes(seg)                                           # mo:135-137
        self.sum += len(seg)
        self.n["segments"] += 1
        if self.sum == self.max_object_bytes:
            self.hit("C3 exactly max_object_bytes")
        if number == 8191:
            self.hit("mo:119 segment number 8191")
        if last:                                                                # mo:145-148
            self.hit("mo:147 last flag")
            self.num_segments = number + 1
        self.hit("mo:160 no PAD element: no progress")
        if self._check_if_complete():                                           # mo:171-174
            self._handle_complete()

    def _handle_complete(self):
        self.frame = self.handler.frame
        self.au = MOT_FLAG_DIR_ELEMENT if self.dir_element else 0               # the dirElement argument of mo:300
        self.hit("mo:300 dirElement %d" % int(self.dir_element))
        self.handler.emissions.append(self.handler.frame)
        super()._handle_complete()


class MotHandlerModel:
    """MotHandler for ONE slot.  item() takes one data group (a DATAGROUP_INFO row and its bytes) after the other; rows / payloads: one
    MOT_OBJECT row and one bytes object (body, then name) per signal_new_mot_object; counters: dabx_carousel_stats; branch: how often each
    reference line / guard was reached; emissions: the frame of every emission."""

    def __init__(self, max_object_bytes=65536, max_dir_objects=49, max_dir_bytes=65536):
        self.max_object_bytes, self.max_dir_objects, self.max_dir_bytes = max_object_bytes or 65536, max_dir_objects or 49, max_dir_bytes or 65536
        self.n = dict.fromkeys(CAROUSEL_COUNTERS, 0)
        self.branch = collections.Counter()
        self.rows, self.payloads, self.emissions = [], [], []
        self.cache = {}                              # place -> [order number, transport id, object] (mMotTable, mh:42-46: all free)
        self.order = 0                               # mOrderNumber
        self.dir = None                              # mpDirectory
        self.frame = 0

    def hit(self, line):
        self.branch[line] += 1

    @property
    def counters(self):
        c = dict(self.n)
        c.update(objects=len(self.rows), object_bytes=sum(len(p) for p in self.payloads))
        return c

    def records(self):
        return np.array(self.rows, MOT_OBJECT) if self.rows else np.zeros(0, MOT_OBJECT)

    def all_bytes(self):
        return np.frombuffer(b"".join(self.payloads), np.uint8)

    # -- mh:211-259 ---------------------------------------------------------------------------------------------------------------------------
    def get_handle(self, tid):
        for place in sorted(self.cache):                                        # mh:213-220
            if self.cache[place][1] == tid:
                self.hit("mh:218 handle in the cache" + (", and in the directory" if self.dir and any(c and c[0] == tid for c in self.dir["comps"]) else ""))
                return self.cache[place][2]
        if self.dir:                                                            # mh:222-225, md:68-76
            for c in self.dir["comps"]:
                if c and c[0] == tid:
                    self.hit("md:73 handle in the directory")
                    return c[1]
        self.hit("mh:226 no handle")
        return None

    def set_handle(self, obj, tid):
        free = [p for p in range(CACHE) if p not in self.cache]
        if free:                                                                # mh:231-240
            place = free[0]
            self.hit("mh:233 a free entry")
        else:                                                                   # mh:243-258
            place = min(self.cache, key=lambda p: self.cache[p][0])
            self.n["evictions"] += 1
            self.hit("mh:255 the oldest entry is evicted")
        self.cache[place] = [self.order, tid, obj]
        self.order += 1

    # -- mh:69-209 ----------------------------------------------------------------------------------------------------------------------------
    def item(self, rec, data):
        self.frame = int(rec["last_frame"])
        self.group(bytes(data), int(rec["crc_flag"]), int(rec["crc_ok"]))

    def _short(self, what):
        self.n["grp_short"] += 1
        self.hit("C1 " + what)

    def group(self, d, flag, ok):
        n = len(d)
        self.n["groups"] += 1
        if n == 0:                                                              # mh:86-89
            self.n["grp_short"] += 1
            return self.hit("mh:88 empty group")
        if flag and not ok:                                                     # mh:91-94
            self.n["crc_bad"] += 1
            return self.hit("mh:93 bad CRC")
        self.hit("mh:91 good CRC" if flag else "mh:91 no CRC flag")
        b0 = d[0]
        typ = b0 & 0x0F                                                         # mh:76
        nxt = 4 if b0 & 0x80 else 2                                             # mh:78, :96-99
        self.hit("mh:96 extension flag %d" % (b0 >> 7))
        number, last = 0, False                                                 # mh:79-80
        if b0 & 0x20:                                                           # mh:101-106
            if nxt + 2 > n:
                return self._short("segment field")
            last, number = bool(d[nxt] & 0x80), (d[nxt] & 0x7F) << 8 | d[nxt + 1]
            nxt += 2
            self.hit("mh:101 segment field")
        else:
            self.hit("mh:101 no segment field")
        tid, tid_flag = 0, False
        if b0 & 0x10:                                                           # mh:108-118
            if nxt + 1 > n:
                return self._short("user access field")
            tid_flag, li = bool(d[nxt] & 0x10), d[nxt] & 0x0F                   # mh:110-111
            nxt += 1                                                            # mh:112
            if tid_flag:
                if nxt + 2 > n:
                    return self._short("transport id")
                tid = d[nxt] << 8 | d[nxt + 1]                                  # mh:115, whatever lengthInd says
                self.hit("mh:115 transport id, length indicator %s" % (li if li in (0, 2, 15) else "other"))
            nxt += li                                                           # mh:117
        else:
            self.hit("mh:108 no user access field")
        size = n - nxt - (2 if flag else 0)                                     # mh:120
        if not tid_flag:                                                        # mh:122-125
            self.n["no_tid"] += 1
            return self.hit("mh:124 no transport id")
        if size < 2:                                                            # C1: motVector[0], [1] of mh:139
            return self._short("payload of %s" % ("1 byte" if size == 1 else "no byte" if size == 0 else "less than no byte"))
        segsize = (d[nxt] & 0x1F) << 8 | d[nxt + 1]                             # mh:139
        if 2 + segsize > size:
            return self._short("segment one byte beyond the payload" if 2 + segsize == size + 1 else "segment beyond the payload")
        if 2 + segsize == size:
            self.hit("C1 segment ends exactly at the payload's end")
        seg = d[nxt + 2:nxt + 2 + segsize]
        if typ == 3:                                                            # mh:142-154
            if number != 0:
                self.n["hdr_not_first"] += 1
                return self.hit("mh:143 header segment %d" % number)
            if self.get_handle(tid) is not None:                                # mh:145-149
                self.n["hdr_known"] += 1
                return self.hit("mh:148 header for a known id")
            obj = self._new_object(seg, tid, False)                             # mh:150-152
            if obj:
                self.set_handle(obj, tid)
        elif typ == 4:                                                          # mh:156-170
            obj = self.get_handle(tid)
            if obj is None:                                                     # mh:159-164
                obj = self._new_object(seg, tid, False)
                if obj is None:
                    return
                self.set_handle(obj, tid)
                self.n["from_body"] += 1
                self.hit("mh:161 object made from a body segment")
            obj.add_body_segment(seg, number, last, tid)                        # mh:167
        elif typ == 6:                                                          # mh:172-204
            if number == 0:
                self._directory(seg, tid)
            elif not self.dir or self.dir["tid"] != tid:                        # mh:198-201
                self.hit("mh:200 directory segment without its directory")
            else:
                self._directory_segment(seg, number, last)                      # mh:202
        else:                                                                   # mh:206-207
            self.n["type_other"] += 1
            self.hit("mh:206 type %d" % typ)

    def _new_object(self, seg, tid, dir_element):
        """new MotObject (mo:45-57); C2 in front: no header core, no object"""
        if len(seg) < 7:
            self.n["hdr_bad"] += 1
            self.hit("C2 segment of %s bytes" % (len(seg) if len(seg) == 6 else "fewer than 6"))
            return None
        obj = _Object(self, dir_element)
        obj.set_header(seg, tid)
        return obj

    # -- md:28-156 ----------------------------------------------------------------------------------------------------------------------------
    def _directory(self, seg, tid):
        if self.dir and self.dir["tid"] == tid:                                 # mh:175-181
            self.n["dirs_repeated"] += 1
            return self.hit("mh:179 segment 0 of the directory there is")
        if len(seg) < 13:                                                       # D1
            self.n["dir_short"] += 1
            return self.hit("D1 segment 0 of %s bytes" % (12 if len(seg) == 12 else "fewer than 12"))
        if len(seg) == 13:
            self.hit("D1 segment 0 of 13 bytes")
        if self.dir:
            self.hit("mh:184 the old directory is deleted")
        self.dir = None                                                         # mh:183-184
        size = (seg[0] & 0x3F) << 24 | seg[1] << 16 | seg[2] << 8 | seg[3]      # mh:188
        objects = seg[4] << 8 | seg[5]                                          # mh:189
        if size > self.max_dir_bytes or objects > self.max_dir_objects:         # D2
            self.n["dirs_refused"] += 1
            return self.hit("D2 dirSize beyond max_dir_bytes" if size > self.max_dir_bytes else "D2 numObjects beyond max_dir_objects")
        if size == self.max_dir_bytes:
            self.hit("D2 dirSize exactly max_dir_bytes")
        if objects == self.max_dir_objects:
            self.hit("D2 numObjects exactly max_dir_objects")
        buf = bytearray(size)                                                   # md:46
        buf[:min(len(seg), size)] = seg[:size]                                  # md:52, clipped to dirSize (D3)
        if len(seg) > size:
            self.hit("D3 segment 0 clipped to dirSize")
        self.dir = dict(tid=tid, size=size, objects=objects, seg_size=len(seg), num=-1, marked={0}, buf=buf, comps=[None] * objects)     # md:36-53
        self.n["dirs_begun"] += 1
        self.n["dir_segments"] += 1
        if len(seg) >= size:                                                    # md:54-55
            self.hit("md:55 analysed at construction")
            self._analyse()

    def _directory_segment(self, seg, number, last):
        d = self.dir
        if number >= DIR_SEGMENTS:                                              # D3: marked[512]
            self.n["dir_seg_bad"] += 1
            return self.hit("D3 directory segment 512" if number == 512 else "D3 directory segment above 512")
        if number in d["marked"]:                                               # md:102-103
            return self.hit("md:103 directory segment already marked")
        at = number * d["seg_size"]                                             # md:107
        if at + len(seg) > d["size"]:                                           # D3
            self.n["dir_seg_bad"] += 1
            return self.hit("D3 copy one byte beyond dirSize" if at + len(seg) == d["size"] + 1 else "D3 copy beyond dirSize")
        if at + len(seg) == d["size"]:
            self.hit("D3 copy ends exactly at dirSize")
        if number == DIR_SEGMENTS - 1:
            self.hit("D3 directory segment 511")
        if last:                                                                # md:104-105
            d["num"] = number + 1
        d["marked"].add(number)                                                 # md:106
        d["buf"][at:at + len(seg)] = seg                                        # md:107-108
        self.n["dir_segments"] += 1
        if d["num"] != -1:                                                      # md:112-118
            if all(i in d["marked"] for i in range(d["num"])):
                self.hit("md:117 all segments in: analysed" + (" again" if d.get("analysed") else ""))
                self._analyse()
            else:
                self.hit("md:115 a directory segment is missing")
        else:
            self.hit("md:112 number of directory segments unknown")

    def _cut(self, what):
        self.n["dir_cut"] += 1
        self.hit("D4 " + what)

    def _analyse(self):
        d = self.dir
        d["analysed"] = True
        buf, size = d["buf"], d["size"]
        if size < 13:                                                           # D4: md:127 reads bytes 11 and 12
            return self._cut("extension length beyond dirSize")
        base = 11 + 2 + (buf[11] << 8 | buf[12])                                # md:125-130
        for i in range(d["objects"]):                                           # md:132
            if base + 2 > size:
                return self._cut("entry id beyond dirSize")
            tid = buf[base] << 8 | buf[base + 1]                                # md:133
            if tid == 0:                                                        # md:135
                return self.hit("md:136 a zero id ends the walk")
            if base + 2 + 7 > size:
                return self._cut("header core beyond dirSize")
            if base + 2 + 7 == size:
                self.hit("D4 header core ends exactly at dirSize")
            if None not in d["comps"]:                                          # md:81-87 finds no place: the object is never seen again
                self.hit("md:87 no component free: not registered")
                base += 2 + ((buf[base + 5] & 0x0F) << 9 | buf[base + 6] << 1 | buf[base + 7] >> 7)
                continue
            obj = _Object(self, True)                                           # md:140-146
            obj.set_header(bytes(buf[base + 2:min(size, base + 2 + NAME_ROOM)]), tid)      # C2: the directory's end bounds the walk
            base += 2 + obj.core[1]                                             # md:149
            d["comps"][d["comps"].index(None)] = (tid, obj)                     # md:83-85
            self.n["dir_objects"] += 1
            self.hit("md:150 directory object registered")
        self.hit("md:132 the walk ends at numObjects")


def run_model(rec, by, **cfg):
    """The model on data groups: [n] DATAGROUP_INFO (byte_pos counted from by[0]) and their bytes."""
    m = MotHandlerModel(**cfg)
    by = bytes(np.asarray(by, np.uint8))
    for r in rec:
        m.item(r, by[int(r["byte_pos"]):int(r["byte_pos"]) + int(r["length"])])
    return m


def model_of(packet_model, **cfg):
    """MotHandlerModel on the groups of a DataProcessorModel."""
    m = MotHandlerModel(**cfg)
    for row, data in zip(packet_model.records(), packet_model.groups):
        m.item(row, data)
    return m


def items_of(groups):
    """Data groups as k_packet records them (bytes objects), one per logical frame."""
    rows, at = [], 0
    for k, g in enumerate(groups):
        flag = len(g) > 0 and bool(g[0] & 0x40)
        ok = flag and len(g) >= 2 and pkc.crc16(g[:-2]) == (g[-2] << 8 | g[-1])
        rows.append((at, k, k, len(g), int(flag), int(ok), 0))
        at += len(g)
    return np.array(rows, DATAGROUP_INFO), np.frombuffer(b"".join(groups), np.uint8)


# ---- directories, as the reference reads them ---------------------------------------------------------------------------------------------
def directory(entries, objects=None, size=None, ext=b"", tail=b""):
    """The bytes of a MOT directory (EN 301 234 7.2): dirSize (30 bits), numObjects, period, segment size, the extension behind its
    length, then per entry the transport id and a MOT header; objects / size: what the fields claim (default: what there is)."""
    body = b"".join(bytes([tid >> 8, tid & 0xFF]) + hdr for tid, hdr in entries) + tail
    n = 13 + len(ext) + len(body)
    size = n if size is None else size
    objects = len(entries) if objects is None else objects
    return size.to_bytes(4, "big") + bytes([objects >> 8, objects & 0xFF]) + bytes(5) + bytes([len(ext) >> 8, len(ext) & 0xFF]) + ext + body


class Groups(mc.Groups):
    """mot_cases.Groups (hdr, body, obj, raw) and directory segments"""

    def dir_seg(self, tid, number, seg, last=False, **kw):
        self.out.append(msc_group(6, seg, tid, number, last, rng=self.rng, **kw))

    def dir(self, tid, data, n_segments=1, order=None):
        """A directory in n_segments segments of equal size (the last may be shorter), sent in `order`."""
        k = -(-len(data) // n_segments)
        for i in (order if order is not None else range(n_segments)):
            self.dir_seg(tid, i, data[k * i:k * i + k], last=i == n_segments - 1)
        return k


def header_mode_groups(seed):
    """(a) header mode, max_object_bytes 4 096: the cache, the quirks of mh:142-170, the forms of the group header, C1..C3."""
    s = Groups(seed)
    r = s.rng
    s.hdr(1, 100, [name_param(b"one.jpg")])                     # two objects whose segments interleave; both complete
    s.hdr(2, 90, [name_param(b"two.png")])
    s.body(1, 0, 40)
    s.body(2, 0, 45)
    s.body(1, 1, 60, last=True)
    s.body(2, 1, 45, last=True)
    cycle = list(s.out)
    s.out += cycle                                              # the carousel's next cycle: known headers, duplicate segments, no emission
    s.body(3, 0, 30)                                            # body before header: the object is made from the body segment's bytes ...
    s.body(3, 1, 30, last=True)                                 # ... and emitted with what set_header read there
    s.hdr(3, 60, [name_param(b"three.jpg")])                    # a header for a known id: ignored
    seg = mot_header(50, [name_param(b"from-body.jpg")]) + s.rand(20)
    s.out.append(msc_group(4, seg, 4, 0, True, rng=r))          # a body segment that reads as a header with a name
    s.out.append(msc_group(3, mot_header(40), 5, 1, rng=r))     # a type-3 group with segment number 1: not looked at
    s.out.append(msc_group(3, mot_header(40), 5, rng=r))        # ... without segment field: number 0
    s.body(5, 0, 40, last=True)
    s.body(5, 1, 10)                                            # a segment behind the last flag, after completion: repeat 1
    for tid in range(6, 18):                                    # ids 1 .. 17: the cache holds 15, ids 1 and 2 are evicted
        s.hdr(tid, 20, [name_param(b"n%d" % tid)])
    s.body(1, 2, 25)                                            # a segment for an evicted id: made from the body again (3 is evicted)
    s.body(17, 0, 20, last=True)
    s.body(16, 0, 20, last=True, ext=True)                      # the extension flag
    s.hdr(20, 22, ext=True)
    s.body(20, 0, 22, last=True, crc=False)                     # without CRC flag: taken as it is
    s.body(20, 5, 20, good=False)                               # a bad CRC
    s.out.append(msc_group(0, s.rand(20), 20, 6, rng=r))        # type 0
    s.dir_seg(20, 3, s.rand(20))                                # type 6 without a directory
    s.out.append(msc_group(4, s.rand(20), None, 0, True, ua=False, rng=r))      # no user access field
    s.out.append(msc_group(4, s.rand(20), None, 0, True, li=2, rng=r))          # a user access field without transport id
    for li in (0, 15, 7):                                       # the id is read behind the length byte whatever li says
        s.out.append(msc_group(4, s.rand(22), 30 + li, 0, True, li=li, rng=r))
    s.raw(b"")                                                  # an empty group
    # C1
    s.hdr(40, 80)
    s.body(40, 0, 40)
    s.raw(msc_group(4, s.rand(38), 40, 1, True, size=40, crc=False, rng=r))     # the segment takes the two trailing bytes: ends exactly at the end
    s.raw(msc_group(4, s.rand(38), 40, 2, size=41, crc=False, rng=r))           # one byte beyond
    s.raw(msc_group(4, s.rand(20), 40, 2, size=4000, rng=r))                    # far beyond
    s.raw(msc_group(4, s.rand(30), 40, 2, size=31, rng=r))                      # with the CRC flag: one byte into the CRC
    s.raw(bytes([0xB4, 0x00, 0x01]))                            # extension + segment flag: the segment field lies beyond 3 bytes
    s.raw(bytes([0x14, 0x00]))                                  # user access flag: its length byte lies beyond
    s.raw(bytes([0x14, 0x00, 0x12, 0x00]))                      # ... the transport id does
    s.raw(bytes([0x14, 0x00, 0x12, 0x00, 0x09]))                # the payload has no byte
    s.raw(bytes([0x14, 0x00, 0x12, 0x00, 0x09, 0x00]))          # ... one byte
    s.raw(bytes([0x14, 0x00, 0x1F, 0x00, 0x09, 0x00]))          # the length indicator points beyond the group
    # C2
    s.hdr(41, 40, cut=6)
    s.hdr(41, 40, cut=5)
    s.hdr(41, 40, [param(0x21, pli=0)], cut=7)                  # the core alone: the parameter byte is beyond
    s.body(41, 0, 40, last=True)
    s.body(42, 0, 6, last=True)                                 # made from a body segment of 6 bytes: no object
    s.body(42, 0, 7, last=True)                                 # ... of 7
    s.hdr(43, 40, [name_param(b"beyond")], cut=7 + 2 + 1 + 5)   # a name one byte beyond the segment
    s.hdr(44, 40, [name_param(b"y", long=True)], cut=9)         # the second length byte is beyond
    s.hdr(47, 40, [name_param(b"x")], cut=8)                    # the length byte is
    s.hdr(48, 40, [name_param(b"far-beyond")], cut=7 + 2 + 1 + 2)
    # C3 at 4 096: exactly, one byte beyond, far beyond
    s.hdr(60, 4096, [name_param(b"full.jpg")])
    for k in range(4):
        s.body(60, k, 1024, last=k == 3)
    s.body(60, 4, 1)
    s.body(60, 0, 1000)
    s.body(60, 1, 3200)
    s.body(61, 8191, 20)                                        # the largest segment number, and the first that is refused
    s.body(61, 8192, 20)
    s.body(62, 0x7FFF, 20)
    s.obj(63, [30, 31, 32], [name_param(b"last.jpg")])
    return s.out


DIR_MODE = dict(max_object_bytes=0, max_dir_objects=8, max_dir_bytes=8192)


def directory_mode_groups(seed):
    """(b) directory mode, max_dir_objects 8, max_dir_bytes 8 192: MotDirectory and D1..D4."""
    s = Groups(seed)
    entry = lambda tid, size, name: (tid, mot_header(size, [name_param(name)]))      # noqa: E731
    s.hdr(301, 50, [name_param(b"cache-301")])                  # an object of the cache; its id comes back in a directory
    d100 = directory([entry(201, 60, b"d201.jpg"), entry(202, 40, b"d202.jpg"), entry(203, 30, b"d203")])
    s.dir(100, d100)                                            # one segment: analysed at construction
    s.body(201, 0, 30)
    s.body(201, 1, 30, last=True)                               # completes a directory object: flag bit 0
    s.hdr(202, 40, [name_param(b"not-this")])                   # a header for a directory id: ignored
    s.body(202, 0, 20)
    d101 = directory([entry(301, 50, b"dir-301"), entry(302, 44, b"d302.png")], objects=5, tail=bytes(9))       # a zero id ends the walk
    k = -(-len(d101) // 3)
    s.dir_seg(101, 1, d101[k:2 * k])                            # before its segment 0: no directory of that id, dropped
    s.dir_seg(101, 0, d101[:k])                                 # the directory is replaced, the objects of 100 are gone
    s.body(202, 1, 20, last=True)                               # a body for an old id makes an object of the cache
    s.dir_seg(101, 0, d101[:k])                                 # segment 0 again
    s.dir_seg(101, 2, d101[2 * k:], last=True)
    s.dir_seg(101, 2, d101[2 * k:], last=True)                  # a duplicate
    s.dir_seg(101, 1, d101[k:2 * k])                            # 0, 2, 1: now it is analysed
    s.body(301, 0, 50, last=True)                               # in the cache AND in the directory: the cache wins, flag 0
    s.body(302, 0, 44, last=True)
    d102 = directory([entry(401, 25, b"d401"), entry(402, 26, b"d402")])
    k = -(-len(d102) // 2)
    d102 = directory([entry(401, 25, b"d401"), entry(402, 26, b"d402")], size=3 * k)
    s.dir_seg(102, 0, d102[:k])
    s.dir_seg(102, 1, d102[k:2 * k], last=True)                 # analysed: both components in use
    s.dir_seg(102, 2, bytes(k))                                 # ends exactly at dirSize; the second analysis registers nothing
    s.body(401, 0, 25, last=True)
    s.dir(103, directory([entry(501, 20, b"d501"), entry(502, 21, b"d502")], objects=4))       # numObjects above the entries: D4 at the id
    s.body(502, 0, 21, last=True)
    s.dir(104, directory([entry(511, 20, b"d511")], objects=2, tail=bytes([0x02, 0x00]) + bytes(6)))    # ... at a header core one byte short
    s.dir(105, directory([entry(521, 20, b"d521")], objects=2, tail=bytes([0x02, 0x01]) + mot_header(10)))      # a core that ends exactly at dirSize
    s.dir_seg(106, 0, directory([])[:12])                       # D1: 12 bytes; the directory 105 stays
    s.body(521, 0, 20, last=True)
    s.dir_seg(106, 0, directory([]))                            # ... 13 bytes: a directory without objects
    s.dir_seg(107, 0, directory([], size=12) + bytes(3))        # dirSize below 13: segment 0 is clipped, D4 at the extension length
    s.dir_seg(108, 0, directory([entry(531, 9, b"x")], objects=9))              # D2: numObjects 9
    s.body(521, 1, 5)                                           # the old directory was deleted all the same: an object of the cache
    s.dir_seg(109, 0, directory([entry(531, 9, b"x")], size=8193))              # D2: dirSize 8 193
    s.dir_seg(110, 0, directory([entry(531, 9, b"x")], size=8192))              # exactly 8 192: taken, never complete
    s.dir(111, directory([entry(540 + i, 10 + i, b"e%d" % i) for i in range(8)]))         # exactly 8 objects
    s.body(547, 0, 17, last=True)
    d112 = directory([], size=512 * 13)                         # D3: segments of 13 bytes, dirSize 6 656
    s.dir_seg(112, 0, d112)
    s.dir_seg(112, 511, bytes(13))                              # ends exactly at dirSize
    s.dir_seg(112, 512, bytes(13))                              # marked[512]
    s.dir_seg(112, 600, bytes(13))
    s.dir_seg(113, 0, directory([], size=3 * 13 - 1))
    s.dir_seg(113, 2, bytes(13), last=True)                     # one byte beyond dirSize: dropped, its last flag too
    s.dir_seg(113, 1, bytes(13))
    s.dir_seg(113, 5, bytes(13))                                # far beyond
    s.obj(600, [40, 41], [name_param(b"after.jpg")])
    return s.out


# ---- logical frames whose packets carry the groups -----------------------------------------------------------------------------------------
SCENARIOS = {"header": (64, header_mode_groups, dict(max_object_bytes=4096, max_dir_objects=0, max_dir_bytes=0)),
             "directory": (384, directory_mode_groups, DIR_MODE)}
WINDOW = 32                                      # logical frames a chunk of the bulk delivery may cover: 28 and a margin
CHUNK_OBJECTS = 16


def build_frames(kbps, groups, seed, cfg, n_frames=N_FRAMES):
    """The logical frames [n_frames, 3 kbps] of a packet-mode sub-channel at ADDRESS that carries the groups in order.  The model runs along:
    when the objects emitted within the last WINDOW frames come near what a chunk of the delivery holds (16 objects, 2 * max_object_bytes
    bytes), padding frames follow until the window is empty."""
    w = Writer(kbps, np.random.default_rng([kbps, seed, 4713]))
    m = MotHandlerModel(**cfg)
    room = 2 * m.max_object_bytes
    for g in groups:
        w.emit(w.cut(g, ADDRESS, dense=len(g) > 100))
        m.frame = len(w.frames)
        flag = len(g) > 0 and bool(g[0] & 0x40)
        m.group(g, int(flag), int(flag and len(g) >= 2 and pkc.crc16(g[:-2]) == (g[-2] << 8 | g[-1])))
        recent = [len(p) for f, p in zip(m.emissions, m.payloads) if f > len(w.frames) - WINDOW]
        if len(recent) >= CHUNK_OBJECTS // 2 or sum(recent) > room // 3:
            w.pad_frame()
            for _ in range(WINDOW):
                w.pad(w.gran)
    w.pad_frame()
    assert len(w.frames) <= n_frames, "%d frames for %d" % (len(w.frames), n_frames)
    while len(w.frames) < n_frames:
        w.pad(w.gran)
    return np.frombuffer(b"".join(w.frames), np.uint8).reshape(n_frames, 3 * kbps).copy()


_cache = {}


def scenario(name, s=0):
    """(kbps, groups, logical frames, configuration) of scenario `name` for stream s."""
    if (name, s) not in _cache:
        kbps, make, cfg = SCENARIOS[name]
        groups = make(300 + s)
        _cache[(name, s)] = (kbps, groups, build_frames(kbps, groups, s, cfg), cfg)
    return _cache[(name, s)]


def overrun_groups(seed, repeats):
    """One object of 250 bytes and `repeats` further segments behind its last flag, 1 byte each: every one emits the object again, longer
    by a byte (mo:171-174), far more bytes than small rings hold."""
    s = Groups(seed)
    s.obj(77, [125, 125], content_type=0)
    for k in range(repeats):
        s.body(77, 2 + k, 1)
    return s.out


# ---- the sets the GPU tests use --------------------------------------------------------------------------------------------------------------
PROT = pkc.PROT
# (kbps, kind) per slot: "car" a carousel slot (scenario by bit rate), "pkt" a packet-mode slot without carousel decoding, "mot" a DAB+ PAD
# slot with MOT decoding (tests/mot_cases.py's first scenario), "plain" a slot left in plain logical frames
STAGE_LAYOUT = [(64, "car"), (384, "car"), (16, "pkt"), (64, "mot"), (32, "plain")]
N_STREAMS = 2
NAME_OF = {0: "header", 1: "directory"}


def stage_layout():
    import dabplus_cases as dc
    return dc.dabplus_layout([(k, PROT, 0) for k, _ in STAGE_LAYOUT], dab_plus=[int(kind == "mot") for _, kind in STAGE_LAYOUT])


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16, per-slot oracle results) of stream s.  Cached: the
    tests of one process share the arrays and leave them unchanged."""
    if ("case", s) not in _cache:
        import dabplus_cases as dc
        layout = stage_layout()
        frames = []
        for j, (kbps, kind) in enumerate(STAGE_LAYOUT):
            frames.append(scenario(NAME_OF[j], s)[2] if kind == "car" else mc.mot_frames(s, 0)[0] if kind == "mot"
                          else pkc.scenario(kbps, 10 * s + j, N_FRAMES))
        cifs = dc.cifs_of(layout, frames, np.random.default_rng([14, s]))
        _cache[("case", s)] = (layout, frames, cifs, dc.oracle_results(layout, cifs))
    return _cache[("case", s)]
