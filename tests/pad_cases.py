"""Shared by test_pad_cases.py (no device) and the two GPU tests of the PAD stage (k_pad): the data stream element of a DAB+ access unit
(mp4processor.cpp:345-353) and PadHandler (base/backend/data/pad_handler.cpp:67-547) restated in plain Python -- the model every device
result is compared with, exactly -- and a builder that puts PAD into the access units of super frames byte by byte.  The oracle (oracle/)
has no PadHandler and is not extended, so the model lives here; every branch cites the reference line it restates (mp4: mp4processor.cpp,
everything else pad_handler.cpp) and counts itself in `branch`.  Four guards go beyond the reference (include/dabx.h, G1..G4)."""
import collections
import os
import sys

import numpy as np

import dabplus_cases as dc
from dabplus_cases import BOUNDARY_COUNTS, cifs_of, crc16_fast, dabplus_layout, oracle_results, rs_parity_columns  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from dabstar_amd.lib import DL_MAX_BYTES, PAD_COUNTERS, PAD_DATAGROUP, PAD_ITEM, PAD_LABEL  # noqa: E402

CI_LENGTHS = (4, 6, 8, 12, 16, 24, 32, 48)       # ContInd::cLengthTable, :48
BATCH = dc.BATCH
N_BATCHES = 7
N_FRAMES = N_BATCHES * BATCH                     # 196 logical frames = 39 super frames and a frame of junk
RATES = [8, 32, 64, 192]


def check_crc_bytes(msg, n):
    """crc.cpp:89-96: calc_crc over msg[0 .. n) against the two bytes behind it."""
    return crc16_fast(msg[:n]) == (msg[n] << 8 | msg[n + 1])


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class PadModel:
    """Mp4Processor's PAD hand-over and PadHandler for ONE slot.  rows / payloads: one PAD_ITEM row and one bytes object per item;
    counters: dabx_pad_stats; branch: how often each reference line / guard was reached; crc_calls: every (message, n) handed to
    check_crc_bytes (compared with the reference's own function in test_pad_cases.py)."""

    def __init__(self):
        self.text = bytearray()                  # mDynamicLabelTextUnConverted
        self.charset = 0                         # mCharSet = EbuLatin
        self.last_app_type = 0                   # mLastAppType
        self.msc_group_element = False           # mMscGroupElement
        self.xpad_length = -1                    # mXPadLength
        self.still_to_go = 0                     # mStillToGo
        self.short = bytearray()                 # mShortPadData
        self.last_segment = self.first_segment = False
        self.segment_number = -1                 # mSegmentNumber
        self.dg_length = 0                       # mDataGroupLength
        self.msc = bytearray()                   # mMscDataGroupBuffer
        self.segment_no = -1                     # mSegmentNo
        self.remain = 0                          # mRemainDataLength
        self.is_last_segment = self.more_xpad = False
        self.counters = dict.fromkeys(PAD_COUNTERS, 0)
        self.branch = collections.Counter()
        self.rows, self.payloads, self.crc_calls = [], [], []
        self.frame = self.au = 0
        self.max_msc = 0

    def hit(self, line):
        self.branch[line] += 1

    def _crc(self, msg, n):
        self.crc_calls.append((bytes(msg[:n + 2]), n))
        return check_crc_bytes(msg, n)

    def _item(self, kind, data, charset=0, flag=0, ok=0):
        c = self.counters
        self.rows.append((c["label_bytes"] + c["group_bytes"], self.frame, len(data), kind, self.au, charset, flag, ok, [0] * 9))
        self.payloads.append(bytes(data))

    # -- mp4processor.cpp:320-353 ---------------------------------------------------------------------------------------------------------
    def super_frame(self, sf, rec):
        sf = bytes(sf)
        end = len(sf)
        self.counters["superframes"] += 1
        self.frame = int(rec["first_frame"])
        for a in range(int(rec["num_aus"])):                                   # mp4:320
            if rec["au_len_bad"] >> a & 1:                                      # mp4:325
                self.hit("mp4:325 impossible length")
                continue
            if not rec["au_crc_ok"] >> a & 1:                                   # mp4:333, :377
                self.hit("mp4:377 wrong AU CRC")
                continue
            self.counters["aus"] += 1
            self.au = a
            st, nxt = int(rec["au_start"][a]), int(rec["au_start"][a + 1])
            if (sf[st] >> 5) & 7 != 4:                                          # mp4:345
                self.hit("mp4:345 element id != 4")
                continue
            self.counters["pad_aus"] += 1
            if st + 2 > end:                                                    # G1 (a taken AU has st + 2 <= its end: never)
                self.counters["pad_bad"] += 1
                self.hit("G1 no count byte")
                continue
            count = sf[st + 1]                                                  # mp4:347
            if count < 2:                                                       # G1: buffer[count - 2] (mp4:351)
                self.counters["pad_bad"] += 1
                self.hit("G1 count %d" % count)
                continue
            if st + 2 + count > end:                                            # G1: mp4:349 would read beyond the super frame
                self.counters["pad_bad"] += 1
                self.hit("G1 beyond the super frame" if st + 2 + count > end + 1 else "G1 one byte beyond the super frame")
                continue
            if st + 2 + count == end:
                self.hit("G1 ends at the super frame's end")
            elif st + 2 + count > nxt - 2:
                self.hit("G1 beyond the AU, inside the super frame")
            self.hit("G1 count %d" % count if count <= 6 else "G1 count > 6")
            buf = sf[st + 2:st + 2 + count]                                     # mp4:348-349
            self.process_pad(buf, count - 3, buf[count - 2], buf[count - 1])    # mp4:350-352

    # -- process_PAD :67-97 ---------------------------------------------------------------------------------------------------------------
    def process_pad(self, buf, last, l1, l0):
        if (l1 >> 6) & 3 != 0:                                                  # :69-75
            self.counters["fpad_other"] += 1
            self.hit(":71 F-PAD type != 0")
            return
        x_pad_ind, ci_flag = (l1 >> 4) & 3, bool(l0 & 2)                        # :77-78
        if x_pad_ind == 1:                                                      # :87
            self.counters["xpad_short"] += 1
            if last < 3:                                                        # G2: :119-122, :151 index below 0
                self.counters["pad_bad"] += 1
                self.hit("G2 short X-PAD, iLast %d" % last)
                return
            if last == 3:
                self.hit("G2 short X-PAD, iLast 3")
            self.short_pad(buf, last, ci_flag)
        elif x_pad_ind == 2:                                                    # :92
            self.counters["xpad_variable"] += 1
            self.variable_pad(buf, last, ci_flag)
        else:                                                                   # :83
            self.counters["xpad_other"] += 1
            self.hit(":83 X-PAD indicator %d" % x_pad_ind)

    def append(self, data, line):
        """mDynamicLabelTextUnConverted.append with guard G4."""
        if len(self.text) + len(data) > DL_MAX_BYTES:
            self.counters["dl_overflow"] += 1
            self.hit("G4 dropped at %s" % line)
            return
        self.text += data
        self.hit(line + " append")
        if len(self.text) == DL_MAX_BYTES:
            self.hit("G4 text at the bound")

    def show_label(self, line):
        self._item(PAD_LABEL, self.text, charset=self.charset)
        self.counters["labels"] += 1
        self.counters["label_bytes"] += len(self.text)
        self.hit(line + " signal_show_label")
        if self.msc:
            self.hit("label while a group is under assembly")

    # -- _handle_short_PAD :111-200 -------------------------------------------------------------------------------------------------------
    def short_pad(self, b, last, ci_flag):
        if ci_flag:                                                             # :115
            ci = b[last]                                                        # :119
            self.first_segment = bool(b[last - 1] & 0x40)                       # :120
            self.last_segment = bool(b[last - 1] & 0x20)                        # :121
            new_charset = b[last - 2] & 0x0F                                    # :122
            if new_charset != self.charset:
                self.hit(":122 charset change")
            self.charset = new_charset
            if self.first_segment:                                              # :124-128
                self.text = bytearray()
                self.hit(":126 first segment clears")
            appl = ci & 0x1F
            if appl == 2:                                                       # :137
                self.hit(":137 short, start of fragment")
                if self.first_segment and not self.last_segment:                # :138
                    self.segment_number = b[last - 2] >> 4                      # :140
                    if self.text:                                               # :141 (cleared at :126: never)
                        self.show_label(":144")
                    self.text = bytearray()                                     # :146
                    self.hit(":138 first and not last")
                self.still_to_go = b[last - 1] & 0x0F                           # :149
                self.short = bytearray([b[last - 3]])                           # :150-151
            elif appl == 3:                                                     # :154
                self.hit(":154 short, continuation")
                i = 0
                while i < 3 and self.still_to_go > 0:                           # :155-159
                    self.still_to_go -= 1
                    self.short.append(b[last - 1 - i])
                    i += 1
                if self.still_to_go <= 0 and len(self.short) > 1:               # :161
                    self.append(self.short, ":163")
                    self.short = bytearray()                                    # :165
            elif appl == 0:
                self.hit(":134 short, end marker")
            else:
                self.hit(":132 short, other application type")
        else:                                                                   # :170
            i = 0
            while i < 4 and self.still_to_go > 0:                               # :173-177
                self.short.append(b[last - i])
                self.still_to_go -= 1
                i += 1
            self.hit(":173 short without CI, %s" % ("data taken" if i else "nothing to take"))
            if self.still_to_go <= 0 and len(self.short) > 0:                   # :180
                if i == 0:
                    self.hit(":183 unsolicited append")
                self.append(self.short, ":183")
                self.short = bytearray()                                        # :185
                if not self.first_segment and self.last_segment:                # :188
                    if self.text:                                               # :190
                        self.show_label(":193")
                    self.text = bytearray()                                     # :195
                    self.hit(":188 end of the last segment")

    # -- _handle_variable_PAD :208-330 ----------------------------------------------------------------------------------------------------
    def variable_pad(self, b, last, ci_flag):
        if not ci_flag:                                                         # :215
            if self.xpad_length > 0:                                            # :217
                if last < self.xpad_length - 1:                                 # :219
                    self.hit(":219 no-CI X-PAD shorter than mXPadLength")
                    return
                data = bytes(b[last - j] for j in range(self.xpad_length))      # :224-228
                if self.last_app_type in (2, 3):                                # :232-235
                    self.hit(":234 no-CI continuation of a label")
                    self.dynamic_label(data, 3)
                elif self.last_app_type in (12, 13):                            # :237-241
                    if self.msc_group_element:
                        self.hit(":240 no-CI continuation of a group")
                        self.add_msc(data)
                    else:
                        self.hit(":239 no-CI continuation without mMscGroupElement")
                else:
                    self.hit(":242 no-CI, other last application type")
            else:
                self.hit(":217 no-CI, mXPadLength not set")
            return                                                              # :245
        base, cis = last, []
        while True:                                                             # :254-262
            if base < 0:                                                        # G3: the CI list would be read below index 0
                self.counters["pad_bad"] += 1
                self.hit("G3 CI list below index 0")
                return
            v = b[base]
            base -= 1                                                           # :256
            cis.append(v)
            if v & 0x1F == 0:                                                   # :259
                cis.pop()
                self.hit(":259 end marker")
                break
            if len(cis) == 4:                                                   # :262
                self.hit(":262 four CIs, no end marker")
                break
        if base == -1:
            self.hit("G3 CI list ends at index 0")
        n_ci = len(cis)
        self.xpad_length = sum(CI_LENGTHS[v >> 5] for v in cis) + (4 if n_ci == 4 else n_ci + 1)      # :268-273
        for k, v in enumerate(cis):                                             # :277
            appl, length = v & 0x1F, CI_LENGTHS[v >> 5]                         # :279-280
            if base - (length - 1) < 0:                                         # G3: :284-287 would read below index 0
                self.counters["pad_bad"] += 1
                self.hit("G3 sub-field below index 0")
                return
            if base - (length - 1) == 0:
                self.hit("G3 sub-field ends at index 0")
            data = bytes(b[base - j] for j in range(length))                    # :283-287
            self.hit("sub-field of %d bytes" % length)
            if appl == 1:                                                       # :291
                if length == 4 and self._crc(data, 2):                          # :292
                    self.dg_length = (data[0] & 0x3F) << 8 | data[1]            # :294
                    self.hit(":294 data group length")
                else:                                                           # :296-299
                    self.counters["li_bad"] += 1
                    self.hit(":298 length indicator, %s" % ("bad CRC" if length == 4 else "length != 4"))
            elif appl in (2, 3):                                                # :302-306
                self.dynamic_label(data, appl)
            elif appl == 12:                                                    # :308-311
                self.new_msc(data)
            elif appl == 13:                                                    # :313-316
                self.add_msc(data)
            else:                                                               # :318
                self.hit(":318 unknown application type, %s" % ("last of the list" if k == n_ci - 1 else "in the middle of the list"))
                return
            self.last_app_type = appl                                           # :321
            base -= length                                                      # :322
            assert base >= -1                                                   # :324 cannot happen behind G3

    # -- _dynamic_label :335-455 ----------------------------------------------------------------------------------------------------------
    def dynamic_label(self, data, appl):
        n = len(data)
        if appl == 2:                                                           # :339
            prefix = data[0] << 8 | data[1]                                     # :342
            field_1, cflag = (prefix >> 8) & 15, (prefix >> 12) & 1             # :343-344
            first, last = (prefix >> 14) & 1, (prefix >> 13) & 1                # :345-346
            if first:                                                           # :350-356
                self.segment_no = 1
                new_charset = (prefix >> 4) & 15
                if new_charset != self.charset:
                    self.hit(":353 charset change")
                self.charset = new_charset
                self.text = bytearray()
                self.hit(":350 first segment")
            else:
                test = ((prefix >> 4) & 7) + 1                                  # :359
                if test != self.segment_no + 1:                                 # :361-366
                    self.hit(":361 segment number mismatch, %s" % ("no first before" if self.segment_no == -1 else
                                                                  "repeated" if test == self.segment_no else "missing or other"))
                    self.segment_no = -1
                    return
                self.segment_no = test                                          # :367
                self.hit(":367 segment %d" % test)
            if cflag:                                                           # :371
                if field_1 == 1:                                                # :375-381
                    self.text = bytearray()
                    self.segment_no = -1
                    self.hit(":375 clear command")
                else:
                    self.hit(":382 other command")
                return
            total = field_1 + 1                                                 # :394
            if n - 2 < total:                                                   # :396-400
                length, self.more_xpad = n - 2, True
                self.hit(":396 segment continues")
            else:                                                               # :401-405
                length, self.more_xpad = total, False
            self.append(data[2:2 + length], ":407")
            self.hit("label segment of %d bytes" % total)
            if last:                                                            # :411
                if not self.more_xpad:                                          # :413-419
                    self.show_label(":416")
                    self.segment_no = -1
                else:
                    self.is_last_segment = True                                 # :422
            else:
                self.is_last_segment = False                                    # :427
            self.remain = total - length                                        # :430
        elif appl == 3 and self.more_xpad:                                      # :433
            if self.remain > n:                                                 # :435-439
                length = n
                self.remain -= n
                self.hit(":435 continuation, more to come")
            else:                                                               # :440-444
                length, self.more_xpad = self.remain, False
                self.hit(":440 continuation, complete")
            self.append(data[:length], ":446")
            if not self.more_xpad and self.is_last_segment:                     # :449
                self.show_label(":452")
        else:
            self.hit(":433 continuation without mMoreXPad")

    # -- _new_MSC_element :460-487, _add_MSC_element :490-519, _build_MSC_segment :522-547 --------------------------------------------------
    def new_msc(self, data):
        self.msc = bytearray()                                                  # :473
        if len(data) >= self.dg_length:                                         # :475
            self.hit(":475 single item")
            self.build_msc(data)
            self.msc_group_element = False
            return
        self.msc_group_element = True                                           # :484
        self.msc = bytearray(data)                                              # :485
        self.hit(":484 start of a group")

    def add_msc(self, data):
        if not self.msc:                                                        # :494
            self.hit(":494 type 13 without type 12")
            return
        self.msc += data                                                        # :507
        self.max_msc = max(self.max_msc, len(self.msc))
        if len(self.msc) >= self.dg_length:                                     # :512
            self.hit(":512 group complete")
            self.build_msc(self.msc)
            self.msc = bytearray()                                              # :515
        else:
            self.hit(":507 group continues")

    def build_msc(self, data):
        size = min(len(data), self.dg_length)                                   # :528
        if size < len(data) - 48:
            self.hit(":528 mDataGroupLength well below the buffer")
        if size < 2:                                                            # :530-534
            self.counters["dg_small"] += 1
            self.hit(":530 size < 2")
            return
        flag = (data[0] >> 6) & 1                                               # :524, :539 CrcFlag
        ok = self._crc(data, size - 2)                                          # :541
        self._item(PAD_DATAGROUP, data[:size], flag=flag, ok=int(ok))
        c = self.counters
        c["groups"] += 1
        c["group_bytes"] += size
        c["dg_crc_bad"] += int(flag and not ok)
        self.hit(":541 group with %s" % ("a good CRC" if flag and ok else "a bad CRC" if flag else "no CRC flag"))
        self.hit("group of %s bytes" % ("2" if size == 2 else "16383" if size == 16383 else "3 .. 255" if size < 256 else "256 .. 4095" if size < 4096
                                       else "4096 and more"))

    def records(self):
        return np.array(self.rows, PAD_ITEM) if self.rows else np.zeros(0, PAD_ITEM)

    def all_bytes(self):
        return np.frombuffer(b"".join(self.payloads), np.uint8)


def run_model(sfs, sfis):
    """The model on super frames [n, 110 R] and their SUPERFRAME_INFO records (the oracle back end's, or the device's)."""
    m = PadModel()
    for sf, rec in zip(sfs, sfis):
        m.super_frame(sf, rec)
    return m


# ---- X-PAD, as the reference reads it ----------------------------------------------------------------------------------------------------
def pad_of(xp, l1, l0):
    """The `count` bytes behind the count byte: the X-PAD reversed (iBuffer[iLast - k] = xp[k]), then the F-PAD L1, L0."""
    return bytes(reversed(bytes(xp))) + bytes([l1, l0])


def var_ci(fields, end_marker=True, filler=b""):
    """Variable X-PAD with contents indicators: fields = [(application type, data of a CI length)], at most four."""
    assert len(fields) <= 4 and all(len(d) in CI_LENGTHS for _, d in fields)
    cis = bytes(CI_LENGTHS.index(len(d)) << 5 | t for t, d in fields)
    if len(fields) < 4 and end_marker:
        cis += b"\x00"
    return pad_of(cis + b"".join(d for _, d in fields) + filler, 0x20, 0x02)


def var_noci(data):
    return pad_of(data, 0x20, 0x00)


def short_ci(appl, first, last, still, charset, segment, byte):
    """Short X-PAD with CI as :119-151 reads it: CI, flags + mStillToGo, segment number + charset, one data byte."""
    return pad_of(bytes([appl, first << 6 | last << 5 | still, segment << 4 | charset, byte]), 0x10, 0x02)


def short_ci3(three):
    return pad_of(bytes([3]) + bytes(three), 0x10, 0x02)


def short_noci(four):
    return pad_of(four, 0x10, 0x00)


def fit(data, rng, sizes=CI_LENGTHS):
    """data padded with random bytes to the smallest CI length that holds it."""
    n = min(s for s in sizes if s >= len(data))
    return bytes(data) + rng.integers(0, 256, n - len(data)).astype(np.uint8).tobytes()


def label_fields(rng, text, first, last, segment=0, charset=0, size=None, cont_size=None):
    """One label segment (1 .. 16 bytes) as a type-2 sub-field of `size` bytes and, when that does not hold it, type-3 sub-fields of
    cont_size bytes for the rest."""
    assert 1 <= len(text) <= 16
    size = size or min(s for s in CI_LENGTHS if s >= len(text) + 2)
    prefix = int(rng.integers(0, 2)) << 15 | first << 14 | last << 13 | (len(text) - 1) << 8 | (charset if first else segment) << 4 | int(rng.integers(0, 16))
    head = bytes([prefix >> 8, prefix & 0xFF]) + text[:size - 2]
    out, at = [(2, fit(head, rng, (size,)))], size - 2
    while at < len(text):
        n = cont_size or 4
        out.append((3, fit(text[at:at + n], rng, (n,))))
        at += n
    return out


def command_field(rng, first, command, segment=0):
    prefix = first << 14 | 1 << 12 | command << 8 | segment << 4
    return (2, fit(bytes([prefix >> 8, prefix & 0xFF]), rng, (4,)))


def length_indicator(rng, length, good=True, size=4):
    d = bytes([int(rng.integers(0, 4)) << 6 | length >> 8, length & 0xFF])
    c = crc16_fast(d) ^ (0 if good else 0x0100)
    return (1, fit(d + bytes([c >> 8, c & 0xFF]), rng, (size,)))


def data_group(rng, length, flag, good=True):
    """`length` >= 2 bytes: bit 6 of byte 0 = the CRC flag; the last two bytes are the CRC of the rest (good) or not."""
    g = bytearray(rng.integers(0, 256, length).astype(np.uint8).tobytes())
    g[0] = (g[0] & 0xBF) | (0x40 if flag else 0)
    if length >= 3 and (flag or good):
        c = crc16_fast(g[:-2]) ^ (0 if good else 0x0001)
        g[-2], g[-1] = c >> 8, c & 0xFF
    return bytes(g)


def group_fields(rng, group, sizes, indicator=True, first_type=12):
    """A data group cut into a type-12 sub-field and type-13 sub-fields of the given sizes (cycled), the last one padded."""
    out = [length_indicator(rng, len(group))] if indicator else []
    at, k = 0, 0
    while at < len(group) or k == 0:
        n = sizes[k % len(sizes)]
        out.append((first_type if k == 0 else 13, fit(group[at:at + n], rng, (n,))))
        at += n
        k += 1
    return out


# ---- the script of one scenario: what the access units carry, in order ---------------------------------------------------------------------
def unit(pad, **kw):
    """One access unit's PAD: element id, count byte and the bytes behind it."""
    return dict(dict(id=4, count=len(pad), body=bytes(pad), crc_bad=False, kind="pad"), **kw)


class Script:
    def __init__(self, rng, room):
        self.rng, self.room, self.units, self.pending = rng, room, [], []

    def fields(self, fs, per_pad=4):
        """Sub-fields into variable X-PADs of at most per_pad CIs that fit `room` bytes of X-PAD (CIs, end marker and data)."""
        cur = []
        for f in fs:
            assert 2 + len(f[1]) <= self.room, (len(f[1]), self.room)
            n = len(cur) + 1
            if cur and (len(cur) == per_pad or n + (1 if n < 4 else 0) + sum(len(d) for _, d in cur) + len(f[1]) > self.room):
                self.units.append(unit(var_ci(cur)))
                cur = []
            cur.append(f)
        if cur:
            self.units.append(unit(var_ci(cur)))

    def pad(self, p, **kw):
        self.units.append(unit(p, **kw))

    def rand(self, n):
        return self.rng.integers(0, 256, n).astype(np.uint8).tobytes()


def _labels(s, rng, room, sizes):
    """Labels of 1 .. 8 segments with 1 .. 16 bytes each, in sub-fields of every CI length the room allows."""
    lengths = list(range(1, 17))
    k = 0
    for n_seg in range(1, 9):
        fs = []
        for seg in range(n_seg):
            ln = lengths[k % 16]
            size = sizes[k % len(sizes)]
            k += 1
            fs += label_fields(rng, s.rand(ln), seg == 0, seg == n_seg - 1, seg, charset=k % 16, size=size if size <= room - 2 else None,
                               cont_size=sizes[(k + 3) % len(sizes)] if sizes[(k + 3) % len(sizes)] <= room - 2 else 4)
        s.fields(fs, per_pad=1 + k % 4)


def build_script(kbps, seed, room):
    """The units of one scenario.  room: X-PAD bytes the scenario's access units hold (the builder waits for an AU that is large enough).
    What belongs to which rate is listed in the issue of this stage: guards and short X-PADs at 8, labels at 32, groups and faults at 64,
    the long groups and the text bound at 192 kbit/s; test_pad_cases.py asserts that together they reach every branch."""
    rng = np.random.default_rng([kbps, seed, 4711])
    s = Script(rng, room)
    sizes = [n for n in CI_LENGTHS if n + 2 <= room]
    F = s.fields
    r = s.rand
    if kbps == 8:
        s.pad(var_noci(r(6)))                                          # before any X-PAD with CIs: mXPadLength is -1 (:217)
    # a first complete label, a first small group: every scenario has them
    F(label_fields(rng, b"DABX" + r(3), 1, 1, charset=4))
    F(group_fields(rng, data_group(rng, 9, True), [4, 6]))
    if kbps == 8:
        # G1: count 0, 1, 2 (variable: G3 before the first CI), 5 (short: G2), 6 (short: the smallest that is walked)
        s.pad(b"", kind="raw")
        s.pad(r(1), kind="raw")
        s.pad(pad_of(b"", 0x20, 0x02))
        s.pad(pad_of(b"", 0x20, 0x00))
        s.pad(pad_of(r(3), 0x10, 0x02))
        s.pad(short_ci(2, 1, 0, 5, 1, 0, 65))
        # G3: CI list that ends exactly at index 0 (its sub-field then lies below), one that would be read below 0
        s.pad(pad_of(bytes([2, 0]), 0x20, 0x02))
        s.pad(pad_of(bytes([2]), 0x20, 0x02))
        s.pad(pad_of(bytes([0x22, 0x23, 0x2C, 0x2D]), 0x20, 0x02))
        s.pad(pad_of(bytes([0x22, 0x23, 0x2C]), 0x20, 0x02))
        # G3: a sub-field that ends exactly at index 0, one byte below, and one below behind a sub-field that was walked
        f = label_fields(rng, b"ab", 1, 1)
        s.pad(var_ci(f))
        s.pad(var_ci(f)[1:])
        f2 = label_fields(rng, b"cd", 1, 0) + label_fields(rng, b"ef", 0, 1, 1)
        s.pad(var_ci(f2)[1:])
        s.pad(var_noci(r(4)))                                          # mXPadLength 11 from the X-PAD in front: too short (:219)
        # short X-PAD labels: CI form (types 2 and 3), the no-CI form, the unsolicited append, end marker and another type
        s.pad(short_ci(2, 1, 0, 7, 2, 3, 72))                          # first, not last: 1 + 7 bytes
        s.pad(short_ci3(b"ell"))
        s.pad(short_ci3(b"o w"))
        s.pad(short_ci3(b"o!!"))                                       # takes one byte, appends 8
        s.pad(short_ci(2, 0, 1, 6, 2, 0, 32))                          # not first, last: 1 + 6 bytes through the no-CI form
        s.pad(short_noci(b"DAB+"))
        s.pad(short_noci(b"!!xx"))                                     # takes two, appends, shows the label (:188-197)
        s.pad(short_noci(b"none"))                                     # nothing to take, nothing held
        s.pad(short_ci(2, 0, 1, 0, 2, 0, 90))                          # mStillToGo 0 with one byte held ...
        s.pad(short_noci(b"uns."))                                     # ... the unsolicited append of :180-198
        s.pad(short_ci(0, 0, 0, 0, 3, 0, 0))
        s.pad(short_ci(7, 1, 1, 0, 3, 0, 0))
        s.pad(short_ci3(b"xyz"))                                       # continuation with nothing to go and nothing held
        # F-PAD type != 0, X-PAD indicators 0 and 3, another element id
        s.pad(pad_of(r(6), 0x60, 0x02))
        s.pad(pad_of(r(6), 0xA0, 0x00))
        s.pad(pad_of(r(6), 0x00, 0x02))
        s.pad(pad_of(r(6), 0x30, 0x02))
        s.pad(var_ci(label_fields(rng, b"never", 1, 1)), id=3)
        s.pad(var_ci(label_fields(rng, b"never", 1, 1)), id=0)
        s.pad(b"", kind="at_end")
        s.pad(b"", kind="past_end")
        s.pad(b"", kind="overhang")
    if kbps == 32:
        _labels(s, rng, room, sizes)
        # a full 196-byte X-PAD: four sub-fields of 48 bytes, a label in them
        text = r(16)
        F(label_fields(rng, text, 1, 0, size=48) + label_fields(rng, r(16), 0, 0, 1, size=48) + label_fields(rng, r(16), 0, 0, 2, size=48) +
          label_fields(rng, r(16), 0, 1, 3, size=48))
        # continued through application type 3 over three X-PADs, and through no-CI X-PADs
        F(label_fields(rng, r(16), 1, 1, size=6, cont_size=4), per_pad=1)
        fs = label_fields(rng, r(15), 1, 1, size=6, cont_size=6)
        s.pad(var_ci(fs[:1]))
        s.pad(var_noci(fs[1][1] + r(2)))                                # mXPadLength = 6 + 2: eight bytes are taken, six are the sub-field's
        s.pad(var_noci(fs[2][1][:5] + r(3)))
        # a missing segment, a repeated segment, a segment without a first
        F(label_fields(rng, b"one ", 1, 0) + label_fields(rng, b"three", 0, 1, 2))
        F(label_fields(rng, b"uno ", 1, 0) + label_fields(rng, b"dos ", 0, 0, 1) + label_fields(rng, b"dos ", 0, 0, 1) + label_fields(rng, b"tres", 0, 1, 2))
        F(label_fields(rng, b"late", 0, 1, 1))
        # the clear command (first and not first), another command, a charset change inside a label (first segment in another charset)
        F(label_fields(rng, b"to be cleared", 1, 0, charset=1) + [command_field(rng, 1, 1)])
        F(label_fields(rng, b"again", 1, 0, charset=1) + [command_field(rng, 0, 1, 1), command_field(rng, 1, 2)])
        F(label_fields(rng, b"EBU ", 1, 0, charset=0) + label_fields(rng, b"UTF8", 0, 1, 1))
        F(label_fields(rng, b"utf8 ", 1, 0, charset=15) + label_fields(rng, b"more", 0, 1, 1))
        s.pad(short_ci(2, 0, 0, 0, 6, 0, 66))                          # the short form changes mCharSet under a variable label
        # a continuation without mMoreXPad, an unknown type at the end and in the middle of a list, four CIs without an end marker
        F([(3, r(4))])
        F(label_fields(rng, b"seen", 1, 1) + [(9, r(4))])
        F(label_fields(rng, b"seen", 1, 1) + [(9, r(4))] + label_fields(rng, b"not seen", 1, 1))
        F(label_fields(rng, b"a", 1, 0) + label_fields(rng, b"b", 0, 0, 1) + label_fields(rng, b"c", 0, 0, 2) + label_fields(rng, b"d", 0, 1, 3))
        # an AU with a wrong CRC and one with an impossible length between the AUs of one label: neither is looked at
        F(label_fields(rng, b"part one, ", 1, 0))
        s.pad(var_ci(label_fields(rng, b"decoy", 1, 1)), crc_bad=True)
        F(label_fields(rng, b"part two, ", 0, 0, 1))
        s.pad(b"", kind="len_bad")
        F(label_fields(rng, b"part three", 0, 1, 2))
        s.pad(b"", kind="at_end")
        s.pad(b"", kind="past_end")
    if kbps == 64:
        g = lambda n, flag=True, good=True: data_group(rng, n, flag, good)      # noqa: E731
        # groups of 2 .. 2000 bytes with a good, a bad and no CRC; a single item; sub-fields of every length
        for n, flag, good in ((2, False, True), (3, True, True), (47, True, False), (48, True, True), (49, False, True), (300, True, True), (2000, True, True)):
            F(group_fields(rng, g(n, flag, good), sizes[-3:] if n > 100 else sizes))
        F(group_fields(rng, g(20, True), [24]))                         # :475 single item
        F(group_fields(rng, g(4, True), [4]))
        # type 13 without type 12; no-CI continuation with and without mMscGroupElement
        F([(13, r(8))])
        grp = g(40, True)
        F(group_fields(rng, grp[:16] + grp[16:], [16])[:2], per_pad=2)  # length indicator + type 12 with 16 bytes: mXPadLength = 4 + 16 + 3
        s.pad(var_noci(grp[16:39] + r(1)))                              # 23 bytes are taken
        s.pad(var_noci(grp[39:] + r(22)))                               # completes the group
        s.pad(var_noci(r(23)))                                          # the buffer is empty: _add_MSC_element returns (:494)
        F(group_fields(rng, g(12, True), [12]))                         # single item: mMscGroupElement false ...
        s.pad(var_noci(r(19)))                                          # ... the no-CI X-PAD behind it is not taken (:239)
        F(label_fields(rng, b"between", 1, 1))
        F([length_indicator(rng, 25)])                                  # a length indicator alone: mLastAppType 1, mXPadLength 4 + 2 ...
        s.pad(var_noci(r(6)))                                           # ... the no-CI X-PAD behind it goes nowhere (:242)
        # a length indicator with a bad CRC, one of length != 4: mDataGroupLength stays
        F([length_indicator(rng, 30)] + [length_indicator(rng, 5, good=False), length_indicator(rng, 6, size=6)] + group_fields(rng, g(30, True), [12, 8], indicator=False))
        # mDataGroupLength changed between type 12 and type 13: shorter (the group is cut, :528) and longer
        grp = g(120, True)
        fs = group_fields(rng, grp, [48])
        F(fs[:3] + [length_indicator(rng, 20)] + fs[3:4])
        cut = g(20, True)
        fs = group_fields(rng, cut + r(60), [32])
        F([length_indicator(rng, 90)] + fs[1:3] + [length_indicator(rng, 20)] + fs[3:4])
        fs = group_fields(rng, g(60, True), [16], indicator=False)
        F([length_indicator(rng, 33)] + fs[:2] + [length_indicator(rng, 60)] + fs[2:])
        # size < 2: mDataGroupLength 0 and 1
        F([length_indicator(rng, 0), (12, r(4))])
        F([length_indicator(rng, 1), (12, r(6))])
        # a label while a group is under assembly, four CIs without an end marker, an unknown type in the middle
        grp = g(70, True)
        fs = group_fields(rng, grp, [24])
        F(fs[:2] + label_fields(rng, b"mid-group", 1, 1) + fs[2:])
        F(group_fields(rng, g(30, False), [8]), per_pad=4)
        F(fs[:2] + [(17, r(4))] + fs[2:3])
        F(group_fields(rng, g(33, True), [16]))
        # an AU with a wrong CRC, one with an impossible length and a lost super frame in the middle of one group
        grp = g(400, True)
        fs = group_fields(rng, grp, [32, 48])
        F(fs[:4])
        s.pad(var_ci(group_fields(rng, g(8, True), [8])), crc_bad=True)
        F(fs[4:6])
        s.pad(b"", kind="len_bad")
        F(fs[6:8])
        s.pad(b"", kind="lost_sf")
        F(fs[8:])
        _labels(s, rng, room, sizes[:5])
    if kbps == 192:
        # the text bound: 128 bytes through eight variable segments, 8 x 16 through the short form to 256 exactly, one more append is dropped
        fs = []
        for seg in range(8):
            fs += label_fields(rng, r(16), seg == 0, 0, seg)
        F(fs)
        for k in range(9):
            s.pad(short_ci(2, 0, 0, 15, 0, 0, 65 + k))
            for _ in range(5):
                s.pad(short_ci3(bytes(v & 0xBF for v in r(3))))         # (bit 6 of the first byte is read as "first segment", :120, and would clear the text)
        s.pad(short_ci(2, 0, 1, 2, 0, 0, 33))                           # three more bytes: dropped too, then the 256 bytes are shown
        s.pad(short_noci(r(4)))
        # the long groups, one of them well over a batch
        for n in (16383, 4095):
            F(group_fields(rng, data_group(rng, n, True, n != 4095), [48]))
        F(label_fields(rng, b"after the groups", 1, 0) + label_fields(rng, r(5), 0, 1, 1))
    n_scripted = len(s.units)
    # until the access units run out: labels, groups and AUs of random bytes
    for k in range(400):
        what = int(rng.integers(0, 6))
        if what == 0:
            s.pad(r(int(rng.integers(2, min(room, 60)))), kind="random")
        elif what < 3:
            F(label_fields(rng, r(int(rng.integers(1, 17))), 1, 1))
        else:
            F(group_fields(rng, data_group(rng, int(rng.integers(2, 3 * room)), bool(rng.integers(0, 4)), bool(rng.integers(0, 6))), sizes[-3:]))
    return s.units, n_scripted


# ---- super frames ------------------------------------------------------------------------------------------------------------------------
# AUs per super frame, cycled.  192 kbit/s has the 6-AU layout only: its 39 super frames are all needed for the text bound and the long
# groups (16 383 bytes take 86 AUs), and two AUs of at most 960 bytes cannot cover its 2 640-byte super frame anyway
LAYOUTS = {8: (2, 3, 4, 2, 6), 32: (2, 3, 2, 4, 6), 64: (3, 4, 2, 6), 192: (6,)}
ROOM = {8: 46, 32: 196, 64: 196, 192: 196}                                              # 8 kbit/s: a 2-AU super frame's AU holds 50 bytes


def _solve_crc(msg, at, want):
    """Two bytes at msg[at], msg[at + 1] for which calc_crc(msg) == want."""
    msg = bytearray(msg)
    for v in range(65536):
        msg[at], msg[at + 1] = v >> 8, v & 0xFF
        if crc16_fast(msg) == want:
            return bytes(msg)
    raise AssertionError("no solution")


def build_scenario(kbps, seed, n_frames=N_FRAMES):
    """(frames [n_frames, 3 kbps], facts).  facts["sf"]: the super frames a perfect decoder hands on, in order; facts["lost"]: indices, in
    the sequence of all super frames built, of those that are corrupted beyond repair; facts["placed"]: units that went into an AU."""
    R = kbps // 8
    rng = np.random.default_rng([kbps, seed, 99])
    units, n_scripted = build_script(kbps, seed, ROOM[kbps])
    end, nb = 110 * R, 24 * R
    out, facts = [], {"sf": [], "lost": [], "placed": collections.Counter()}
    at, n_sf = 0, 0
    while (n_sf + 1) * 5 <= n_frames:
        n_au = LAYOUTS[kbps][n_sf % len(LAYOUTS[kbps])]
        nxt = units[at] if at < len(units) else None
        len_bad = nxt is not None and nxt["kind"] == "len_bad"
        lost = nxt is not None and nxt["kind"] == "lost_sf"
        if len_bad:
            n_au = 4
            at += 1
        if lost:
            at += 1
        sf = rng.integers(0, 256, end).astype(np.uint8)
        dac, sbr = dc.AU_MODE[n_au]
        sf[2] = (int(sf[2]) & 0x9F) | (dac << 6) | (sbr << 5)
        starts = dc._au_starts(R, rng, n_au, "even")
        if len_bad:
            starts[1] = starts[0] + 1                                   # AU 1 is one byte long: its length is -1 (mp4:325)
        nib = [v for f in starts for v in (f >> 8, (f >> 4) & 15, f & 15)]
        for i, v in enumerate(nib):
            b = 3 + i // 2
            sf[b] = (int(sf[b]) & 0x0F) | (v << 4) if i % 2 == 0 else (int(sf[b]) & 0xF0) | v
        au = [dc.AU_HEAD[n_au]] + starts + [end]
        for a in range(n_au):
            st, ln = au[a], au[a + 1] - au[a] - 2
            if ln < 0:
                continue
            sf[st] = (int(sf[st]) & 0x1F) | (int(rng.choice([0, 1, 2, 3, 5, 6, 7])) << 5)       # no PAD unless a unit is placed
            u = units[at] if at < len(units) and not lost else None
            crc_fix = None
            if lost:
                u = unit(var_ci(group_fields(rng, data_group(rng, 8, True), [8])))              # would restart the group if it were seen
            if u is not None:
                k = u["kind"]
                is_last = a == n_au - 1
                if k in ("pad", "raw", "random") and 2 + u["count"] <= ln:
                    body, count = u["body"], u["count"]
                elif k == "at_end" and is_last and 16 <= ln <= 255:
                    # the PAD's last two bytes are the AU's CRC: count = ln, F-PAD = the CRC bytes, two free bytes make it come out as 0x20 0x02
                    xp = var_ci(label_fields(rng, b"at the end", 1, 1, size=12))[:-2]
                    body, count = rng.integers(0, 256, ln - 2 - len(xp)).astype(np.uint8).tobytes() + xp, ln
                    crc_fix = 0x2002
                elif k == "past_end" and is_last and ln <= 254:
                    body, count = rng.integers(0, 256, ln - 2).astype(np.uint8).tobytes(), ln + 1
                elif k == "overhang" and not is_last and ln <= 200 and au[a + 2] - au[a + 1] >= 8:
                    body, count = rng.integers(0, 256, ln - 2).astype(np.uint8).tobytes(), ln + 4      # reads the CRC and two bytes of the next AU
                else:
                    u = None
            if u is not None:
                sf[st] = (int(sf[st]) & 0x1F) | (u["id"] << 5)
                sf[st + 1] = count
                sf[st + 2:st + 2 + len(body)] = np.frombuffer(body, np.uint8)
                if crc_fix is not None:
                    sf[st:st + ln] = np.frombuffer(_solve_crc(bytes(sf[st:st + ln]), 2, crc_fix), np.uint8)
                if not lost:
                    facts["placed"][u["kind"] + (" crc_bad" if u["crc_bad"] else "") + ("" if u["id"] == 4 else " other id")] += 1
                    at += 1
            c = crc16_fast(sf[st:st + ln]) ^ (0x5A5A if u is not None and u["crc_bad"] else 0)
            sf[st + ln], sf[st + ln + 1] = c >> 8, c & 0xFF
        fc = ds.firecode_parity(bytes(sf[2:11]))
        sf[0], sf[1] = fc >> 8, fc & 0xFF
        full = np.zeros(120 * R, np.uint8)
        full[:end] = sf
        full[end:] = rs_parity_columns(sf.reshape(110, R)).reshape(-1)
        if lost:
            full[:nb] = rng.integers(0, 256, nb)                        # the first logical frame is noise: 24 errors in every code word
            facts["lost"].append(n_sf)
        else:
            facts["sf"].append(sf.copy())
        out.extend(full.reshape(5, nb))
        n_sf += 1
    facts["scripted_left"] = max(0, n_scripted - at)
    while len(out) < n_frames:
        out.append(rng.integers(0, 256, nb).astype(np.uint8))
    return np.stack(out), facts


_cache = {}


def scenario(kbps, seed, n_frames=N_FRAMES):
    key = (kbps, seed, n_frames)
    if key not in _cache:
        _cache[key] = build_scenario(kbps, seed, n_frames)
    return _cache[key]


# ---- the sets the tests use --------------------------------------------------------------------------------------------------------------
PROT = 3                                         # EEP 4-A, as tests/dabplus_cases.py
# (kbps, kind) per slot: "pad" a DAB+ slot with PAD decoding, "dab+" a DAB+ slot without (it carries a PAD scenario all the same: the stage
# must not look at it), "pkt" a packet-mode slot (tests/packet_cases.py), "plain" a slot in plain logical frames
STAGE_LAYOUTS = [
    [(8, "pad"), (64, "pad"), (32, "dab+"), (16, "pkt"), (32, "pad")],
    [(192, "pad"), (24, "plain"), (64, "pad"), (32, "pad"), (8, "dab+")],
]
STAGE_STREAMS = [0, 1, 0, 1]                     # layout of stream s
PACKET_ADDRESS = 0x155


def seed_of(stream, slot):
    return 10 * stream + slot


def all_scenarios():
    """Every (kbps, seed) the GPU stage test runs with PAD decoding on."""
    return [(kbps, seed_of(s, j)) for s, lay in enumerate(STAGE_STREAMS) for j, (kbps, kind) in enumerate(STAGE_LAYOUTS[lay]) if kind == "pad"]


def boundary_schedule(n_streams, n_frames=N_FRAMES):
    """[batch][stream] CIF counts: stream s walks through BOUNDARY_COUNTS from place s on until it has had n_frames."""
    left, out, b = [n_frames] * n_streams, [], 0
    while any(left):
        row = [min(BOUNDARY_COUNTS[(b + s) % len(BOUNDARY_COUNTS)], left[s]) for s in range(n_streams)]
        left = [a - c for a, c in zip(left, row)]
        out.append(row)
        b += 1
    return out


def stage_layout(lay):
    kinds = STAGE_LAYOUTS[lay]
    return dabplus_layout([(k, PROT, 0) for k, _ in kinds], dab_plus=[int(kind in ("pad", "dab+")) for _, kind in kinds])


def slot_frames(s, j, kbps, kind, n_frames=N_FRAMES):
    """The intended logical frames of slot j of stream s."""
    if kind in ("pad", "dab+"):
        return scenario(kbps, seed_of(s, j), n_frames)[0]
    import packet_cases as pc
    return pc.scenario(kbps, seed_of(s, j), n_frames)


_stage_cache = {}


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16, per-slot oracle results) of stream s of STAGE_STREAMS.
    Cached: the tests of one process share the arrays and leave them unchanged."""
    if s not in _stage_cache:
        lay = STAGE_STREAMS[s]
        layout = stage_layout(lay)
        frames = [slot_frames(s, j, kbps, kind) for j, (kbps, kind) in enumerate(STAGE_LAYOUTS[lay])]
        cifs = cifs_of(layout, frames, np.random.default_rng([11, s]))
        _stage_cache[s] = (layout, frames, cifs, oracle_results(layout, cifs))
    return _stage_cache[s]


def slot_model(s, j):
    """The model of PAD slot (s, j) on the oracle back end's super frames and records."""
    o = stream_case(s)[3][j]
    return run_model(o["sf"], o["sfi"])
