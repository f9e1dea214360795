"""Shared by test_data_handler_cases.py (no device) and test_gpu_data_handler_stage.py: the three data handlers DataProcessor hands the MSC
data groups of a packet-mode sub-channel to beside MotHandler (data_processor.cpp:53-101), restated in plain Python -- the models every
device result is compared with, exactly -- and builders of crafted groups on packet_cases.Writer.  The oracle (oracle/) has no DataProcessor
and the handlers cannot be compiled without the GUI's headers, so parity with the reference's object code is unpinned, as for every
DataProcessor path: the models live here and every branch cites the line it restates --
    tdc:  base/backend/data/tdc_datahandler.cpp          ip:  base/backend/data/ip_datahandler.cpp
    dg:   base/backend/data/journaline/dabdgdec_impl.c   jl:  base/backend/data/journaline_datahandler.cpp    nml: .../journaline/NML.cpp
The models walk byte by byte and keep a dict; the device tests 64 sync positions per pass, folds CRCs from 64 slices and keeps a 64 KiB
table.  The guards T1..T3, I1, J1 go beyond the reference (include/dabx.h "The data handlers of a packet-mode slot").  model.reached holds a
key per branch taken; REQUIRED lists every key there is."""
import os
import sys

import numpy as np

import packet_cases as pkc
from packet_cases import crc16

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from dabstar_amd.lib import (DATA_COUNTERS, DATA_CRC_OK, DATA_ITEM, DATA_NEW_REVISION, DATA_NML, DATA_TDC_0, DATA_TDC_1, DATA_UDP,  # noqa: E402
                             DATAGROUP_INFO)

ADDRESS = pkc.ADDRESS_A
HANDLERS = ("tdc", "ip", "journaline")


# ---- the models --------------------------------------------------------------------------------------------------------------------------
class HandlerModel:
    """One handler object: add(group bytes, crc_flag, crc_ok, last_frame) per add_MSC_data_group call, in the slot's order."""

    def __init__(self, only_new_revisions=False, first_group=0):
        self.only_new = only_new_revisions
        self.counters = dict.fromkeys(DATA_COUNTERS, 0)
        self.reached = set()
        self.rows, self.payloads = [], []
        self.index = first_group
        self.filed = {}                                          # Journaline: mDataMap, object id -> revision_index

    def add(self, g, crc_flag, crc_ok, frame):
        self.counters["groups"] += 1
        self.group(bytes(g), bool(crc_flag), bool(crc_ok), int(frame))
        self.index += 1

    def hit(self, key, counter=None):
        self.reached.add(key)
        if counter:
            self.counters[counter] += 1

    def emit(self, payload, kind, flags, a, b, frame):
        c = self.counters
        self.rows.append((c["bytes"], frame, len(payload), kind, flags, a & 0xFFFF, b & 0xFFFF, self.index & 0xFFFFFFFF, 0))
        self.payloads.append(bytes(payload))
        c["items"] += 1
        c["bytes"] += len(payload)

    def records(self):
        return np.array(self.rows, DATA_ITEM) if self.rows else np.zeros(0, DATA_ITEM)

    def all_bytes(self):
        return np.frombuffer(b"".join(self.payloads), np.uint8)


class TdcModel(HandlerModel):
    """tdc_dataHandler::add_MSC_data_group (tdc:52-128) with handleFrame_type_0 / _1 (tdc:130-193)."""

    def group(self, g, crc_flag, crc_ok, frame):
        n, o, frames = len(g), 0, 0
        while o < n:                                             # tdc:60
            while o + 2 < n and not (g[o] == 0xFF and g[o + 1] == 0x0F):       # tdc:62-72
                o += 1
            if o + 2 >= n:                                       # tdc:73-76
                return self.hit("tdc:73-76 no sync" if not frames else "tdc:73-76 no further sync", "walk_end")
            if o + 7 > n:
                return self.hit("T1", "tdc_cut")
            length = int.from_bytes(g[o + 2:o + 4], "big", signed=True)      # tdc:80: an i16
            if length < 0:                                       # tdc:85
                return self.hit("tdc:85-88 negative", "tdc_len_bad")
            if length >= n - o:
                return self.hit("tdc:85-88 beyond", "tdc_len_bad")
            if o + 7 + length > n:
                return self.hit("T2", "tdc_cut")
            s = min(length, 11)                                  # tdc:102
            self.hit("tdc:102 eleven" if length >= 11 else "tdc:102 all")
            vec = g[o:o + 4] + g[o + 6:o + 7] + g[o + 7:o + 7 + s]            # tdc:94-106
            if crc16(vec) != (g[o + 4] << 8 | g[o + 5]):          # tdc:107-113
                return self.hit("tdc:109-113", "tdc_hdr_crc_bad")
            kind, body = g[o + 6], g[o + 7:o + 7 + length]
            if kind == 0:                                        # tdc:115-118, :130-151
                flags = 0
                if length < 2:
                    self.hit("T3", "tdc_crc0_short")
                elif crc16(body[:-2]) == (body[-2] << 8 | body[-1]):             # tdc:140
                    flags = DATA_CRC_OK
                    self.hit("tdc:140 good")
                else:
                    self.hit("tdc:140-143 bad", "tdc_crc0_bad")
                self.emit(body, DATA_TDC_0, flags, o, 0, frame)  # tdc:148-149
            elif kind == 1:                                      # tdc:119-122, :153-193
                self.hit("tdc:153-193")
                self.emit(body, DATA_TDC_1, 0, o, 0, frame)      # tdc:170, :191
            else:                                                # tdc:123-126
                return self.hit("tdc:123-126", "tdc_type_other")
            o += 7 + length                                      # tdc:150, :192
            frames += 1
            if o == n:
                self.hit("tdc:60 ends at N")
            if frames == 2:
                self.hit("tdc:60 second frame")
        if n == 0:
            self.hit("tdc:60 empty")


class IpModel(HandlerModel):
    """IpDataHandler::add_MSC_data_group, process_ipVector, process_udpVector (ip:44-148)."""

    def group(self, g, crc_flag, crc_ok, frame):
        n = len(g)
        if crc_flag and not crc_ok:                              # ip:59
            return self.hit("ip:59", "ip_dg_crc_bad")
        if n < 1:
            return self.hit("I1 flags", "ip_short")
        nxt = 2                                                  # ip:51
        if g[0] & 0x80:                                          # ip:64-67
            nxt += 2
            self.hit("ip:64-67")
        if g[0] & 0x20:                                          # ip:69-74
            nxt += 2
            self.hit("ip:69-74")
        if g[0] & 0x10:                                          # ip:78-88
            if nxt >= n:
                return self.hit("I1 lengthInd", "ip_short")
            nxt += 1 + (g[nxt] & 0x0F)
            self.hit("ip:78-88")
        if nxt + 4 > n:
            return self.hit("I1 length word", "ip_short")
        ip_len = g[nxt + 2] << 8 | g[nxt + 3]                    # ip:94
        if not ip_len < n:                                       # ip:95
            return self.hit("ip:95", "ip_len_bad")
        if ip_len < 10:
            return self.hit("I1 below 10", "ip_short")
        if nxt + ip_len > n:
            return self.hit("I1 copy", "ip_short")
        v = g[nxt:nxt + ip_len]                                  # ip:97-102
        if v[0] >> 4 != 4:                                       # ip:103
            return self.hit("ip:103", "ip_not_v4")
        h = v[0] & 0x0F                                          # ip:114
        if 4 * h > ip_len:
            return self.hit("I1 header", "ip_short")
        total = 0
        for i in range(2 * h):                                   # ip:121-124
            total += v[2 * i] << 8 | v[2 * i + 1]
        if total > 0xFFFF:
            self.hit("ip:125 carries")
        total = (total >> 16) + (total & 0xFFFF)                 # ip:125, once
        if ~total & 0xFFFF:                                      # ip:126-129
            return self.hit("ip:126-129", "ip_checksum_bad")
        if v[9] != 17:                                           # ip:131-137
            return self.hit("ip:136", "ip_proto_other")
        length = ip_len - 4 * h - 8                              # ip:134, :146
        if length < 0:
            return self.hit("I1 payload", "ip_short")
        self.hit("ip:145-147 empty" if length == 0 else "ip:145-147")
        u = v[4 * h:]
        self.emit(u[8:8 + length], DATA_UDP, 0, u[0] << 8 | u[1], u[2] << 8 | u[3], frame)


class JournalineModel(HandlerModel):
    """DAB_DATAGROUP_DECODER_putData (dg:130-241) with its header extraction (dg:248-296), callback_func and add_to_dataBase (jl:38-54,
    :101-132) around the head of NMLFactory::CreateNML (nml:363-385).  Stated deviation: every object that passes the head is filed."""

    def group(self, g, crc_flag, crc_ok, frame):
        n = len(g)
        if n < 2:                                                # dg:251-258
            return self.hit("dg:251-258", "jl_hdr_short")
        ext = g[0] >> 7
        if ext and n < 4:                                        # dg:271-280
            return self.hit("dg:271-280", "jl_hdr_short")
        if g[0] & 0x20:                                          # dg:170-177
            return self.hit("dg:170-177", "jl_segmented")
        hl = 2 + 2 * ext                                         # dg:179
        self.hit("dg:179 extension" if ext else "dg:179 plain")
        length = n - hl                                          # dg:181
        if length == 0:                                          # dg:183-190
            return self.hit("dg:183-190", "jl_empty")
        if g[0] & 0x40:                                          # dg:192
            if length < 2:                                       # dg:194-201
                return self.hit("dg:194-201", "jl_len_bad")
            length -= 2                                          # dg:202
            if not crc_ok:                                       # dg:209-216
                return self.hit("dg:209-216", "jl_crc_bad")
        else:                                                    # dg:218-225
            return self.hit("dg:218-225", "jl_no_crc")
        if g[0] & 0x0F:                                          # dg:227-235
            return self.hit("dg:227-235", "jl_type_other")
        if g[0] & 0x10:
            self.hit("dg:238 user access kept")
        nml = g[hl:hl + length]                                  # dg:238
        if length > 4096:
            return self.hit("J1", "nml_too_long")
        if length < 4:                                           # nml:363-368
            return self.hit("nml:363-368", "nml_short")
        oid = nml[0] << 8 | nml[1]                               # nml:371
        if nml[2] >> 5 == 0 or nml[2] >> 5 > 4:                  # nml:374-379, jl:105-106
            return self.hit("nml:374-379", "nml_type_bad")
        rev = nml[2] & 7                                         # nml:385
        if oid not in self.filed:                                # jl:114-116
            fresh = True
            self.hit("jl:116 new id")
        else:
            fresh = self.filed[oid] != rev                       # jl:118
            self.hit("jl:118 new revision" if fresh else "jl:118 same revision")
        self.filed[oid] = rev                                    # jl:120-122 (and the deviation)
        if not fresh and self.only_new:
            return self.hit("only_new_revisions", "nml_repeat")
        self.emit(nml, DATA_NML, DATA_NEW_REVISION if fresh else 0, oid, nml[2] | g[1] << 8, frame)


MODELS = {"tdc": TdcModel, "ip": IpModel, "journaline": JournalineModel}
REQUIRED = {
    "tdc": {"tdc:60 empty", "tdc:73-76 no sync", "tdc:73-76 no further sync", "T1", "tdc:85-88 negative", "tdc:85-88 beyond", "T2", "tdc:102 eleven", "tdc:102 all",
            "tdc:109-113", "T3", "tdc:140 good", "tdc:140-143 bad", "tdc:153-193", "tdc:123-126", "tdc:60 ends at N", "tdc:60 second frame"},
    "ip": {"ip:59", "I1 flags", "ip:64-67", "ip:69-74", "I1 lengthInd", "ip:78-88", "I1 length word", "ip:95", "I1 below 10", "I1 copy", "ip:103", "I1 header",
           "ip:125 carries", "ip:126-129", "ip:136", "I1 payload", "ip:145-147 empty", "ip:145-147"},
    "journaline": {"dg:251-258", "dg:271-280", "dg:170-177", "dg:179 extension", "dg:179 plain", "dg:183-190", "dg:194-201", "dg:209-216", "dg:218-225",
                   "dg:227-235", "dg:238 user access kept", "J1", "nml:363-368", "nml:374-379", "jl:116 new id", "jl:118 new revision", "jl:118 same revision",
                   "only_new_revisions"},
}


def record_of(g, frame, byte_pos=0):
    """The dabx_datagroup_info of a completed group as DataProcessorModel._emit writes it."""
    flag = len(g) > 0 and bool(g[0] & 0x40)
    ok = flag and len(g) >= 2 and crc16(g[:-2]) == (g[-2] << 8 | g[-1])
    return (byte_pos, frame, frame, len(g), int(flag), int(ok), 0)


def records_of(groups):
    """(DATAGROUP_INFO [n], bytes) of a list of groups, group i completed in logical frame i // 3."""
    rows, at = [], 0
    for i, g in enumerate(groups):
        rows.append(record_of(g, i // 3, at))
        at += len(g)
    return (np.array(rows, DATAGROUP_INFO) if rows else np.zeros(0, DATAGROUP_INFO)), np.frombuffer(b"".join(groups), np.uint8)


def run_model(handler, rec, by, only_new_revisions=False, first_group=0):
    """The handler's model on data groups as dabx_read_datagroups returns them (records with byte_pos into by)."""
    m = MODELS[handler](only_new_revisions, first_group)
    by = bytes(np.asarray(by, np.uint8))
    for r in rec:
        p = int(r["byte_pos"])
        m.add(by[p:p + int(r["length"])], r["crc_flag"], r["crc_ok"], r["last_frame"])
    return m


def model_of(handler, dm, only_new_revisions=False):
    """... and on the groups of a packet_cases.DataProcessorModel."""
    return run_model(handler, dm.records(), dm.all_bytes(), only_new_revisions)


# ---- builders ----------------------------------------------------------------------------------------------------------------------------
def junk(rng, n):
    """n bytes without 0xFF: no sync word"""
    return rng.integers(0, 255, n).astype(np.uint8).tobytes()


def with_crc(b):
    c = crc16(b)
    return bytes(b) + bytes([c >> 8, c & 0xFF])


def tdc_frame(rng, length, kind=0, hdr_good=True, body_good=True, claim=None):
    """FF 0F, the length (claim: the field when it is not to be the body's), the header CRC over the vector of tdc:91-108, the type, the body
    -- of a type-0 frame with its own CRC in the last two bytes."""
    body = junk(rng, length)
    if kind == 0 and length >= 2:
        body = with_crc(body[:-2]) if body_good else body[:-2] + bytes(2 * [crc16(body[:-2]) >> 8 ^ 0x55])
    field = (length if claim is None else claim) & 0xFFFF
    head = bytes([0xFF, 0x0F, field >> 8, field & 0xFF])
    c = crc16(head + bytes([kind]) + body[:11]) ^ (0 if hdr_good else 0x0100)
    return head + bytes([c >> 8, c & 0xFF, kind]) + body


def tdc_groups(rng):
    g = [b"", b"\x00", b"\xFF\x0F", b"\xFF\x0F\x00", junk(rng, 3), junk(rng, 8), tdc_frame(rng, 1)]              # N = 0, 1, 2, 3, 8
    g.append(junk(rng, 20) + b"\xFF\x0F\x00")                                                # sync at N - 3: found, T1
    g.append(junk(rng, 21) + b"\xFF\x0F")                                                    # sync at N - 2: never found
    for at in (63, 64, 65, 127, 128):                                                        # sync at every side of a pass of 64 positions
        f = tdc_frame(rng, 20, kind=at & 1)
        g.append(junk(rng, at) + f + junk(rng, 200 - at - len(f)))
    g.append(b"\xFF" + tdc_frame(rng, 5))                                                    # FF FF 0F
    for length in (0, 1, 2, 10, 11, 12):
        g.append(tdc_frame(rng, length, 0))
        g.append(tdc_frame(rng, length, 1) + junk(rng, 4))
    g.append(junk(rng, 9) + tdc_frame(rng, 30))                                              # length = N - o - 7: the frame ends the group
    for claim in (36, 37, 0x8000, 0xFFFF):                                                   # N - o = 37: N - o - 1 (T2), N - o, negative
        g.append(tdc_frame(rng, 30, claim=claim))
    g.append(tdc_frame(rng, 25) + tdc_frame(rng, 40, 1) + tdc_frame(rng, 3))                 # back to back
    g.append(tdc_frame(rng, 25, 1) + junk(rng, 70) + tdc_frame(rng, 12) + junk(rng, 2))      # junk between two frames
    g.append(tdc_frame(rng, 8, 2))
    g.append(junk(rng, 3) + tdc_frame(rng, 16, hdr_good=False) + tdc_frame(rng, 16))         # header CRC bad: the walk ends there
    g.append(tdc_frame(rng, 16, body_good=False) + tdc_frame(rng, 500))                      # body CRC bad: emitted, the walk goes on
    g.append(tdc_frame(rng, 6, 1) + b"\xFF\x0F\x00\x01")                                     # T1 behind a frame
    return g


def tdc_long_group(rng):
    return tdc_frame(rng, pkc.DG_MAX_BYTES - 7)              # one 16 384-byte group holding one frame


def ip_datagram(rng, payload, h=5, version=4, proto=17, checksum="good", ip_len=None, ports=(0x1234, 8888), fill=None):
    """An IPv4 header of 4 h bytes, a UDP header and the payload.  checksum: "good", "bad", or "carry": good, with header words that make
    the 32-bit sum pass 0xFFFF, so that only the fold of ip:125 accepts it."""
    udp = bytes([ports[0] >> 8, ports[0] & 0xFF, ports[1] >> 8, ports[1] & 0xFF]) + junk(rng, 4) + bytes(payload)
    total = 4 * h + len(udp) if ip_len is None else ip_len
    hdr = bytearray(junk(rng, max(4 * h, 12)) if fill is None else bytes([fill]) * max(4 * h, 12))
    hdr[0] = version << 4 | h
    hdr[2], hdr[3] = total >> 8 & 0xFF, total & 0xFF
    hdr[9] = proto
    if checksum == "carry":
        hdr[4:8] = b"\xFE\xFE\xFD\xFD"
    if h >= 3:
        hdr[10] = hdr[11] = 0
        s = sum(hdr[2 * i] << 8 | hdr[2 * i + 1] for i in range(2 * h))
        while s > 0xFFFF:
            s = (s >> 16) + (s & 0xFFFF)
        c = ~s & 0xFFFF ^ (0x0400 if checksum == "bad" else 0)
        hdr[10], hdr[11] = c >> 8, c & 0xFF
    return (bytes(hdr[:4 * h]) + udp) if h >= 3 else (bytes(hdr[:max(4 * h, 12)]) + udp)


def dg_header(rng, ext=0, crc=1, seg=0, ua=0, gtype=0, length_ind=0):
    b = bytes([ext << 7 | crc << 6 | seg << 5 | ua << 4 | gtype, int(rng.integers(0, 256))])
    b += junk(rng, 2 * ext) + junk(rng, 2 * seg)
    if ua:
        b += bytes([int(rng.integers(0, 16)) << 4 | length_ind]) + junk(rng, length_ind)
    return b


def dg_close(b, crc=1, good=True):
    if not crc:
        return b
    c = crc16(b) ^ (0 if good else 0x8001)
    return b + bytes([c >> 8, c & 0xFF])


def ip_group(rng, dgram, good=True, tail=0, **hdr):
    return dg_close(dg_header(rng, **hdr) + dgram + junk(rng, tail), hdr.get("crc", 1), good)


def ip_groups(rng):
    pay = lambda n: junk(rng, n)      # noqa: E731
    g = [b"", b"\x00", junk(rng, 2), junk(rng, 3), b"\x10\x00", b"\x90\x00\x00", junk(rng, 5)]       # I1: flags, lengthInd, the length word
    for nib in range(16):                                                                    # all 16 flag nibbles
        g.append(ip_group(rng, ip_datagram(rng, pay(20 + nib)), ext=nib >> 3, crc=nib >> 2 & 1, seg=nib >> 1 & 1, ua=nib & 1, length_ind=2))
    for li in (0, 1, 15):
        g.append(ip_group(rng, ip_datagram(rng, pay(30)), ua=1, length_ind=li))
    d = ip_datagram(rng, pay(30))
    for want in (0, 9, 10, "N-1", "N"):                                                     # the length word: N = 2 + 58 + 2 = 62
        n = 2 + len(d) + 2
        v = bytearray(d)
        k = n - 1 if want == "N-1" else n if want == "N" else want
        v[2], v[3] = k >> 8, k & 0xFF
        g.append(ip_group(rng, bytes(v)))
    g.append(ip_group(rng, ip_datagram(rng, pay(12), h=2, ip_len=10), tail=3))               # ipLength 10 with a header inside it: the checksum decides
    g.append(ip_group(rng, ip_datagram(rng, pay(30), version=6)))
    for h in (0, 1, 5, 15):
        g.append(ip_group(rng, ip_datagram(rng, pay(17), h=h)))
    g.append(ip_group(rng, ip_datagram(rng, pay(40), h=15, ip_len=20), crc=0))               # 4 h > ipLength
    g.append(ip_group(rng, ip_datagram(rng, pay(30), checksum="bad")))
    g.append(ip_group(rng, ip_datagram(rng, pay(30), checksum="carry", fill=0xEE)))          # accepted only because the sum is folded
    g.append(ip_group(rng, ip_datagram(rng, pay(30), proto=6)))
    g.append(ip_group(rng, ip_datagram(rng, b"")))                                           # payload of 0 bytes
    g.append(ip_group(rng, ip_datagram(rng, pay(1)), crc=0, tail=1))                         # ... and of 1
    g.append(ip_group(rng, ip_datagram(rng, b"", ip_len=27)[:27], tail=4))                   # ipLength - 4 h - 8 = -1
    g.append(ip_group(rng, ip_datagram(rng, pay(25)), good=False))                           # the group's CRC fails
    g.append(ip_group(rng, ip_datagram(rng, pay(1400)), ext=1))
    return g


def nml_object(rng, oid, kind, rev, length, static=0, compressed=0):
    b = bytes([oid >> 8, oid & 0xFF, kind << 5 | static << 4 | compressed << 3 | rev]) + junk(rng, max(0, length - 3))
    return b[:length]


def jl_group(rng, obj, good=True, **hdr):
    return dg_close(dg_header(rng, **hdr) + obj, hdr.get("crc", 1), good)


def journaline_groups(rng):
    g = []
    for n in range(6):                                                                       # N = 0 .. 5, extension off and on, CRC flag set
        for ext in (0, 1):
            b = bytearray(junk(rng, n))
            if n:
                b[0] = ext << 7 | 0x40
            g.append(bytes(b))
    obj = lambda oid, kind, rev, n=40, **kw: nml_object(rng, oid, kind, rev, n, **kw)      # noqa: E731
    g.append(jl_group(rng, obj(1, 1, 0), seg=1))
    g.append(jl_group(rng, obj(1, 1, 0), crc=0))
    g.append(jl_group(rng, obj(1, 1, 0), good=False))
    for gtype in (0, 4, 6):
        g.append(jl_group(rng, obj(2, 2, 1), gtype=gtype))
    for n in (0, 1, 2, 3, 4, 4096, 4097):                                                    # data_len 2 (an object of 0 bytes), 3, .. after the CRC: 4096, 4097
        g.append(jl_group(rng, obj(3, 3, 2, n), ext=n & 1))
    for kind in (0, 1, 4, 5, 7):
        g.append(jl_group(rng, obj(0x100 + kind, kind, 3)))
    g.append(jl_group(rng, obj(0xBEEF, 2, 5), ua=1, length_ind=3))                           # the user-access field stays in the object
    for oid, rev in ((7, 1), (7, 1), (7, 2), (8, 2), (7, 2), (8, 2), (7, 1), (0xFFFF, 7), (0, 0), (0xFFFF, 7), (0, 0)):
        g.append(jl_group(rng, obj(oid, 1 + (oid & 3), rev, 30 + rev, static=oid & 1, compressed=rev & 1)))
    return g


_cache = {}


def sequence(handler):
    """The crafted groups of a handler, in order; cached, and left unchanged by every test."""
    if handler not in _cache:
        rng = np.random.default_rng([5, HANDLERS.index(handler)])
        _cache[handler] = {"tdc": tdc_groups, "ip": ip_groups, "journaline": journaline_groups}[handler](rng)
    return _cache[handler]


def random_groups(handler, n=300):
    """Random bytes and thinned random bytes behind plausible heads: what no builder thought of."""
    key = ("random", handler, n)
    if key not in _cache:
        rng = np.random.default_rng([6, HANDLERS.index(handler)])
        out = []
        for i in range(n):
            b = bytearray(rng.integers(0, 256, int(rng.integers(0, 90))).astype(np.uint8).tobytes())
            if handler == "tdc" and len(b) > 8 and i % 2:
                at = int(rng.integers(0, len(b) - 7))
                b[at:at + 4] = bytes([0xFF, 0x0F, 0, int(rng.integers(0, 24))])
                if i % 4 == 1:
                    c = crc16(bytes(b[at:at + 4]) + bytes(b[at + 6:at + 7]) + bytes(b[at + 7:at + 7 + min(11, b[at + 3])]))
                    b[at + 4], b[at + 5] = c >> 8, c & 0xFF
            if handler == "ip" and len(b) > 12 and i % 2:
                b[0] &= 0x9F if i % 4 == 1 else 0xDF
                b[2] = 0x40 | int(rng.integers(0, 8))
                b[4], b[5] = 0, int(rng.integers(0, len(b) + 2))
            if handler == "journaline" and len(b) > 4:
                b[0] = (b[0] & 0xD0 if i % 8 else b[0]) | 0x40
                b = bytearray(with_crc(bytes(b[:-2]))) if i % 3 else b
            out.append(bytes(b))
        _cache[key] = out
    return _cache[key]


# ---- the slots of the engine tests -------------------------------------------------------------------------------------------------------
N_STREAMS = 2
N_BATCHES = pkc.N_BATCHES
N_FRAMES = pkc.N_FRAMES
# (kbps, kind): one slot per handler beside a plain packet slot, a carousel slot and a DAB+ slot
STAGE_LAYOUT = [(128, "tdc"), (64, "ip"), (128, "journaline"), (64, "pkt"), (64, "car"), (48, "dab+")]
ONLY_NEW = {0: False, 1: True}                               # per stream: only_new_revisions of its Journaline slot


def slot_groups(s, kind):
    """The groups of slot `kind` of stream s: the crafted sequence (stream 1: reversed but for Journaline, whose order matters) and random ones."""
    seq = list(sequence(kind))
    if s == 1 and kind != "journaline":
        seq.reverse()
    if kind == "tdc" and s == 0:
        seq.insert(5, tdc_long_group(np.random.default_rng(55)))
    return seq + random_groups(kind, 60)


def slot_frames(s, j):
    """The logical frames [N_FRAMES, 3 kbps] of slot j of stream s: its groups cut into packets at ADDRESS between padding and packets of
    another address, padded to the end."""
    key = ("frames", s, j)
    if key not in _cache:
        kbps, kind = STAGE_LAYOUT[j]
        if kind == "dab+":
            import dabplus_cases as dc
            _cache[key] = dc.build_scenario(kbps // 8, pkc.seed_of(s, j))[0][:N_FRAMES]
        elif kind in ("pkt", "car"):
            _cache[key] = pkc.scenario(kbps, pkc.seed_of(s, j), N_FRAMES)
        else:
            _cache[key] = frames_of(kbps, slot_groups(s, kind), [8, s, j])
    return _cache[key]


def frames_of(kbps, groups, seed):
    """The logical frames [N_FRAMES, 3 kbps] that carry `groups` at ADDRESS, in order."""
    rng = np.random.default_rng(seed)
    w = pkc.Writer(kbps, rng)
    for i, g in enumerate(groups):
        w.emit(w.cut(g, ADDRESS, dense=len(g) > 300))
        if i % 7 == 0:
            w.emit(w.group(int(rng.integers(1, 40)), True, address=pkc.ADDRESS_B))
        if i % 5 == 0:
            w.pad(1)
    assert len(w.frames) < N_FRAMES, len(w.frames)
    while len(w.frames) < N_FRAMES:
        w.pad_frame()
        w.pad(w.gran)
    return np.frombuffer(b"".join(w.frames[:N_FRAMES]), np.uint8).reshape(N_FRAMES, 3 * kbps).copy()


def stage_layout():
    import dabplus_cases as dc
    return dc.dabplus_layout([(k, pkc.PROT, 0) for k, _ in STAGE_LAYOUT], dab_plus=[int(kind == "dab+") for _, kind in STAGE_LAYOUT])


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16, per-slot oracle results) of stream s.  Cached."""
    key = ("case", s)
    if key not in _cache:
        import dabplus_cases as dc
        layout = stage_layout()
        frames = [slot_frames(s, j) for j in range(len(STAGE_LAYOUT))]
        cifs = dc.cifs_of(layout, frames, np.random.default_rng([10, s]))
        _cache[key] = (layout, frames, cifs, dc.oracle_results(layout, cifs))
    return _cache[key]


def overrun_group(rng, n=300):
    """More TDC frames of length 0 than the record ring holds, in one group"""
    return b"".join(tdc_frame(rng, 0, i & 1) for i in range(n))
