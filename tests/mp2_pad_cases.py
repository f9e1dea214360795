"""Shared by test_mp2_pad_cases.py (no device) and the two GPU tests of the PAD stage's MP2 source (k_pad_mp2): Mp2Processor's frame sync
and PAD hand-over (base/backend/audio/mp2processor.cpp:250-285 and :611-747) restated bit-serially in plain Python -- the model every
device result is compared with, exactly -- on top of PadModel (tests/pad_cases.py), and a builder that writes logical frames of a DAB
audio sub-channel: an MP2 header wherever a scenario wants one, audio bytes, the X-PAD reversed in front of the ScF-CRC bytes and the
F-PAD.  mp2processor.cpp cannot be compiled without the GUI's headers, so parity with the reference's object code is unpinned; every branch
of the restatement cites its line (mp2: mp2processor.cpp) and counts itself in `branch`."""
import collections
import copy

import numpy as np

import pad_cases as pc
from dabplus_cases import BOUNDARY_COUNTS, cifs_of, dabplus_layout, oracle_results  # noqa: F401
from dabstar_amd.lib import MP2_GET_DATA, MP2_GET_RATE, MP2_SEARCHING, MP2_SYNC_STATS, PAD_COUNTERS  # noqa: F401

BATCH = pc.BATCH
N_BATCHES = pc.N_BATCHES
N_FRAMES = pc.N_FRAMES
RATES = [8, 48, 56, 128, 384]                    # vLen 20; the largest rate with a 2-byte ScF-CRC; the smallest with 4; a mid rate; 1152 bytes
SAMPLE_RATES = (44100, 48000, 32000, 0, 22050, 24000, 16000, 0)       # mp2:61-64
SYNC_FIELDS = tuple(k for k in MP2_SYNC_STATS.names if k != "reserved")


def v_len(kbps):
    """mp2:613-621: the bytes of a logical frame in front of the ScF-CRC and the F-PAD."""
    return 3 * kbps - (4 if kbps * 1000 >= 56000 else 2) - 2


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Mp2PadModel:
    """Mp2Processor::add_to_frame and _process_pad_data for ONE slot, one bit at a time, feeding PadModel.process_pad.  limit: how many
    of the X-PAD bytes next to the F-PAD are handed on (None: all vLen of them, as the reference does; 254: as the device stages them).
    snaps[k]: (items, item bytes, dabx_pad_stats counters, dabx_mp2_sync_stats fields) after k logical frames."""

    def __init__(self, kbps, limit=None, first=0):
        self.kbps, self.limit = kbps, limit
        self.framesize = 24 * kbps               # mp2:236 MP2framesize
        self.state = MP2_SEARCHING               # mp2:238
        self.header_count = self.bit_count = 0   # mp2:239-240
        self.sample_rate = 48000                 # mp2processor.h: sampleRate
        self.mp2frame = bytearray(3)             # MP2frame: only bytes 0 .. 2 are read for our purpose (mp2:271-285)
        self.pad = pc.PadModel()
        self.stats = dict(syncs=0, frames=0, hdr_refused=0, rate_unsupported=0, last_sync_bit=-1)
        self.branch = collections.Counter()
        self.n_frames = first                    # index of the next logical frame in the slot's sequence
        self.snaps = [self.snap()]

    def hit(self, line):
        self.branch[line] += 1

    def sync_stats(self):
        return dict(self.stats, sample_rate=self.sample_rate, state=self.state, bit_count=self.bit_count, header_count=self.header_count, active=1)

    def snap(self):
        c = self.pad.counters
        return (len(self.pad.rows), c["label_bytes"] + c["group_bytes"], dict(c), self.sync_stats())

    # -- mp2:250-264 ----------------------------------------------------------------------------------------------------------------------
    def set_sample_rate(self, rate):
        if self.sample_rate == rate:                                            # mp2:252
            self.hit("mp2:252 rate unchanged")
            return
        if rate != 48000 and rate != 24000:                                     # mp2:257-261
            self.hit("mp2:257 unsupported rate %d" % rate)
            return
        self.hit("mp2:263 rate %d -> %d" % (self.sample_rate, rate))
        self.sample_rate = rate                                                 # mp2:263

    # -- mp2:271-285 ----------------------------------------------------------------------------------------------------------------------
    def get_mp2_sample_rate(self):
        f = self.mp2frame
        if f[0] != 0xFF:                                                        # mp2:277 (the 12 ones of :725: never)
            self.hit("mp2:277 no sync word")
            self.stats["hdr_refused"] += 1
            return 0
        if (f[1] & 0xF6) != 0xF4:                                               # mp2:278
            self.hit("mp2:278 not layer II, layer bits %d" % ((f[1] >> 1) & 3))
            self.stats["hdr_refused"] += 1
            return 0
        if (f[2] - 0x10) >= 0xE0:                                               # mp2:279, in int: only index 15 is refused
            self.hit("mp2:279 bit-rate index 15")
            self.stats["hdr_refused"] += 1
            return 0
        if f[2] < 0x10:
            self.hit("mp2:279 bit-rate index 0 passes")
        rate = SAMPLE_RATES[(((f[1] & 0x08) >> 1) ^ 4) + ((f[2] >> 2) & 3)]     # mp2:283-284
        self.hit("mp2:283 rate index %d, ID %d" % ((f[2] >> 2) & 3, (f[1] >> 3) & 1))
        if rate not in (48000, 24000):
            self.stats["rate_unsupported"] += 1
        return rate

    def add_bit_to_mp2(self, bit, nm):                                          # mp2:749-763, bytes 0 .. 2 only
        if nm < 24:
            mask = 1 << (7 - (nm & 7))
            self.mp2frame[nm >> 3] = (self.mp2frame[nm >> 3] | mask) if bit else (self.mp2frame[nm >> 3] & ~mask)

    # -- mp2:611-674 ----------------------------------------------------------------------------------------------------------------------
    def process_pad_data(self, frame):
        n = len(frame)                                                          # iBits.size() / 8
        vlen = 24 * self.kbps // 8                                              # mp2:613
        assert vlen == n                                                        # mp2:615
        vlen -= (4 if self.kbps * 1000 >= 56000 else 2) + 2                     # mp2:620-621
        l0, l1 = frame[n - 1], frame[n - 2]                                     # mp2:623-624
        c = self.pad.counters
        c["aus"] += 1
        c["pad_aus"] += 1
        self.pad.frame, self.pad.au = self.n_frames, 0
        if (l1 >> 6) & 3 != 0:                                                  # mp2:629
            c["fpad_other"] += 1
            self.hit("mp2:629 F-PAD type != 0")
            return
        ind = (l1 >> 4) & 3
        if ind == 0:                                                            # mp2:635
            c["xpad_other"] += 1
            self.hit("mp2:635 no X-PAD")
            return
        if ind == 3:                                                            # mp2:641
            c["xpad_other"] += 1
            self.hit("mp2:641 X-PAD indicator 3")
            return
        if ind == 1:                                                            # mp2:649-653
            data = bytes(frame[vlen - 4:vlen])
            self.hit("mp2:649 short X-PAD")
        else:                                                                   # mp2:654-657
            data = bytes(frame[:vlen])
            self.hit("mp2:654 variable X-PAD")
            if self.limit is not None:
                data = data[-self.limit:]
        self.pad.process_pad(data, len(data) - 1, l1, l0)                       # mp2:673

    # -- mp2:678-747 ----------------------------------------------------------------------------------------------------------------------
    def add_to_frame(self, frame):
        frame = bytes(frame)
        bits = np.unpackbits(np.frombuffer(frame, np.uint8)).tolist()
        amount = self.framesize                                                 # mp2:681
        assert amount == len(bits)                                              # mp2:682
        lf = self.framesize if self.sample_rate == 48000 else 2 * self.framesize        # mp2:680
        self.pad.counters["superframes"] += 1
        for i in range(amount):                                                 # mp2:685
            if self.state == MP2_GET_DATA:                                      # mp2:687
                self.add_bit_to_mp2(bits[i], self.bit_count)                    # mp2:689
                self.bit_count += 1
                if self.bit_count >= lf:                                        # mp2:691
                    self.hit("mp2:691 frame complete, %s, %d Hz" % ("at the last bit" if i == amount - 1 else "in mid-frame", self.sample_rate))
                    self.stats["frames"] += 1
                    self.process_pad_data(frame)                                # mp2:695
                    self.state = MP2_SEARCHING                                  # mp2:710-712
                    self.header_count = 0
                    self.bit_count = 0
            elif self.state == MP2_SEARCHING:                                   # mp2:715
                if bits[i] == 1:                                                # mp2:718
                    self.header_count += 1
                    if self.header_count == 12:                                 # mp2:720
                        if i < 11:
                            self.hit("mp2:720 sync word across the frame boundary")
                        self.hit("mp2:720 sync word")
                        self.stats["syncs"] += 1
                        self.stats["last_sync_bit"] = i
                        self.bit_count = 0                                      # mp2:722-726
                        while self.bit_count < 12:
                            self.add_bit_to_mp2(1, self.bit_count)
                            self.bit_count += 1
                        self.state = MP2_GET_RATE                               # mp2:727
                else:                                                           # mp2:730-733
                    if self.header_count == 11:
                        self.hit("mp2:732 eleven ones, then a zero")
                    self.header_count = 0
            else:                                                               # mp2:735 GetSampleRate
                if i == 0 and self.bit_count > 12:
                    self.hit("mp2:737 header across the frame boundary")
                self.add_bit_to_mp2(bits[i], self.bit_count)                    # mp2:737
                self.bit_count += 1
                if self.bit_count == 24:                                        # mp2:738
                    self.set_sample_rate(self.get_mp2_sample_rate())            # mp2:740
                    lf = self.framesize if self.sample_rate == 48000 else 2 * self.framesize    # mp2:741
                    self.state = MP2_GET_DATA                                   # mp2:742
        if self.state == MP2_SEARCHING and self.header_count > 0:
            self.hit("mp2:718 ones at the end of the frame")
        self.n_frames += 1
        self.snaps.append(self.snap())


def run_model(kbps, frames, limit=None, first=0):
    m = Mp2PadModel(kbps, limit, first)
    for f in frames:
        m.add_to_frame(f)
    return m


# ---- a second, word-at-a-time walk of the sync alone: the builder asks it which logical frames will have their PAD taken -------------------
class SyncWalk:
    """add_to_frame's state without the bit loop (str.find on the frame's bits); step() returns whether an MP2 frame completed in the
    frame.  test_mp2_pad_cases.py holds it against the model on every scenario."""

    def __init__(self, kbps):
        self.A = 24 * kbps
        self.state, self.hc, self.bc, self.rate = MP2_SEARCHING, 0, 0, 48000
        self.hdr = ""

    def step(self, frame):
        s = "".join(format(b, "08b") for b in bytes(frame))
        A, pos, done = self.A, 0, False
        while pos < A:
            if self.state == MP2_GET_DATA:
                need = (A if self.rate == 48000 else 2 * A) - self.bc
                if need > A - pos:
                    self.bc += A - pos
                    break
                pos += need
                done = True
                self.state, self.hc, self.bc = MP2_SEARCHING, 0, 0
            elif self.state == MP2_SEARCHING:
                at = ("1" * self.hc + s[pos:]).find("1" * 12)
                if at < 0:
                    tail = s[pos:]
                    run = len(tail) - len(tail.rstrip("1"))
                    self.hc = run + (self.hc if run == len(tail) else 0)
                    break
                pos += at + 12 - self.hc
                self.state, self.hc, self.bc, self.hdr = MP2_GET_RATE, 12, 12, ""
            else:
                k = min(24 - self.bc, A - pos)
                self.hdr += s[pos:pos + k]
                self.bc += k
                pos += k
                if self.bc == 24:
                    b1, b2 = 0xF0 | int(self.hdr[:4], 2), int(self.hdr[4:], 2)
                    rate = 0 if (b1 & 0xF6) != 0xF4 or b2 - 0x10 >= 0xE0 else SAMPLE_RATES[(((b1 & 8) >> 1) ^ 4) + ((b2 >> 2) & 3)]
                    if rate in (48000, 24000):
                        self.rate = rate
                    self.state = MP2_GET_DATA
        return done


# ---- the builder -------------------------------------------------------------------------------------------------------------------------
def header(mpeg1=1, layer=2, prot=1, bitrate=8, rate=1, padding=0, private=0):
    """The 24 header bits the sync reads: 12 ones, ID, layer (2 = '10', Layer II), protection, bit-rate index, rate index, padding, private."""
    return 0xFFF << 12 | mpeg1 << 11 | layer << 9 | prot << 8 | bitrate << 4 | rate << 2 | padding << 1 | private


H48 = dict(mpeg1=1, rate=1)                      # sample_rates[1] = 48 000
H24 = dict(mpeg1=0, rate=1)                      # sample_rates[5] = 24 000


def frame_plan(kbps, variant):
    """One entry per logical frame: (style of the audio bytes, bit offset of an MP2 header that starts in this frame or None, its fields).
    variant 0: the header at bit 0 throughout -- both rates, every header the check refuses or the rate switch ignores, the switch
    48 -> 24 -> 48 kHz.  variant 1: what the search can meet -- all-zero and all-ones frames, 11 ones then a zero, 20 ones, the bit stream
    shifted so that the sync word or the header straddles a frame boundary and frames complete in mid-frame, frames of random bytes."""
    A = 24 * kbps
    plan = []

    def seg(n, offset=0, style="low", step=1, **h):
        for k in range(n):
            plan.append((style, offset if offset is not None and k % step == 0 else None, dict(H48, **h)))
    if variant == 0:
        seg(30)
        seg(1, layer=1); seg(1, layer=3); seg(1, layer=0)                       # not Layer II
        seg(1, bitrate=15); seg(1, bitrate=0); seg(2)
        for mpeg1, rate in ((1, 0), (1, 2), (1, 3), (0, 0), (0, 2), (0, 3)):    # 44.1, 32 kHz, reserved, 22.05, 16 kHz, reserved
            seg(1, mpeg1=mpeg1, rate=rate)
        seg(3)
        seg(20, step=2, **H24)                                                  # 24 kHz: an MP2 frame is two logical frames
        seg(2, step=2, mpeg1=1, rate=0); seg(2, step=2, mpeg1=0, rate=3); seg(2, step=2, bitrate=15, **H24)      # ... and stays so
        seg(6, step=2, **H24)
        seg(N_FRAMES - len(plan))                                               # back to 48 kHz
    else:
        seg(2, None, "zeros"); seg(1, None, "ones"); seg(1, None, "zeros")
        seg(1, None, "ones11"); seg(1, None, "ones20"); seg(2, None, "zeros")
        seg(8)
        for off in (A - 1, A - 7, A - 8, A - 13, 1, 7, 8, 13, A // 2 + 3):       # sync word / header across the boundary; completion in mid-frame
            seg(7, off)
        seg(2, None, "zeros")
        seg(12, A - 5, step=2, **H24)                                           # 24 kHz, shifted
        seg(3, None, "zeros")
        seg(10, None, "random")
        seg(2, None, "zeros")
        seg(8, 0, step=2, **H24)
        seg(N_FRAMES - len(plan))
    assert len(plan) == N_FRAMES, len(plan)
    return plan


SCRIPT_OF = {48: 32, 56: 64, 64: 64, 128: 64, 384: 192}      # which of pad_cases.build_script's scripts a rate carries (at the room it allows; 8 kbit/s has its own, 64 is the delivery test's)


def mp2_units(kbps, seed):
    """The PADs of a scenario, in order: what only an MP2 slot can meet first (8 kbit/s: vLen is 20, so guard G3 and the check of
    pad_handler.cpp:219 bite), then build_script's labels and groups; units that only make sense inside an access unit are left out."""
    room = min(196, v_len(kbps))
    rng = np.random.default_rng([kbps, seed, 1789])
    r = lambda n: rng.integers(0, 256, n).astype(np.uint8).tobytes()           # noqa: E731
    own = []
    if kbps == 8:
        L = lambda t, first, last, seg=0, **kw: pc.label_fields(rng, t, first, last, seg, **kw)    # noqa: E731
        four = L(b"ab", 1, 0) + L(b"cd", 0, 0, 1) + L(b"ef", 0, 0, 2) + L(b"gh", 0, 1, 3)
        own.append(pc.var_ci(four))                                             # 4 CIs + 4 x 4 bytes = 20: the last sub-field ends at index 0
        own.append(pc.var_noci(r(20)))                                          # mXPadLength 20, iLast 19: taken (:219), goes to the label path
        own.append(pc.var_ci(L(b"0123456789", 1, 0, size=12) + L(b"abcd", 0, 1, 1, size=6)))     # 3 + 12 + 6 = 21: one byte below index 0 (G3)
        own.append(pc.var_noci(r(20)))                                          # mXPadLength 21 > 20: too short (:219)
        own.append(pc.var_ci(L(b"ij", 1, 0) + L(b"kl", 0, 0, 1) + L(b"mn", 0, 0, 2) + L(b"op", 0, 1, 3, size=6)))     # 4 + 18 = 22: G3 behind three walked
    if kbps == 48:
        # pad_handler.cpp:219 at vLen 140: mXPadLength 148 from a full X-PAD that itself is cut short by G3, then a no-CI X-PAD
        fs = [(12, r(48)), (13, r(48)), (13, r(48))]
        own.append(pc.var_ci(fs))                                               # 4 + 144 = 148 > 140: the third sub-field lies below index 0
        own.append(pc.var_noci(r(60)))
        fs = [pc.length_indicator(rng, 400), (12, r(48)), (13, r(48)), (13, r(32))]
        own.append(pc.var_ci(fs))                                               # 4 + 132 = 136 <= 140 ...
        own.append(pc.var_noci(r(136)))                                         # ... and the no-CI X-PAD of 136 bytes behind it continues the group
    # the short X-PAD in both forms at every rate: the four bytes in front of the ScF-CRC, iLast 3 (mp2:649-653)
    own += [pc.short_ci(2, 1, 0, 3, 1, 0, 77), pc.short_ci3(b"P2!"), pc.short_ci(2, 0, 1, 2, 1, 0, 33), pc.short_noci(b"ok..")]
    own = [pc.unit(p) for p in own]
    # F-PAD type != 0 and the X-PAD indicators 0 and 3 at every rate
    own += [pc.unit(pc.pad_of(r(6), l1, l0)) for l1, l0 in ((0x60, 0x02), (0xA0, 0x00), (0x00, 0x02), (0x30, 0x02))]
    if kbps == 8:
        # build_script's labels and groups need 26 bytes of X-PAD and more; here are 20: segments of up to 10 bytes, sub-fields of up to 16
        sc = pc.Script(rng, room)
        sizes = [4, 6, 8, 12, 16]
        sc.fields(pc.label_fields(rng, b"DABX" + r(3), 1, 1, charset=4))
        sc.fields(pc.group_fields(rng, pc.data_group(rng, 9, True), [4, 6]))
        for n_seg in range(1, 9):
            fs = []
            for seg in range(n_seg):
                fs += pc.label_fields(rng, r(1 + (3 * n_seg + seg) % 10), seg == 0, seg == n_seg - 1, seg, charset=n_seg, cont_size=4)
            sc.fields(fs, per_pad=1 + n_seg % 3)
        for n, flag, good in ((2, False, True), (3, True, True), (47, True, False), (48, True, True), (300, True, True)):
            sc.fields(pc.group_fields(rng, pc.data_group(rng, n, flag, good), sizes[-3:] if n > 40 else sizes))
        n_scripted = len(sc.units)
        for k in range(200):
            what = int(rng.integers(0, 6))
            if what == 0:
                sc.pad(r(int(rng.integers(2, room))), kind="random")
            elif what < 3:
                sc.fields(pc.label_fields(rng, r(int(rng.integers(1, 11))), 1, 1))
            else:
                sc.fields(pc.group_fields(rng, pc.data_group(rng, int(rng.integers(2, 3 * room)), bool(rng.integers(0, 4)), bool(rng.integers(0, 6))), sizes[-3:]))
        units = sc.units
    else:
        units, n_scripted = pc.build_script(SCRIPT_OF[kbps], seed, room)
    fits = lambda u: u["kind"] in ("pad", "random") and u["id"] == 4 and not u["crc_bad"] and 2 <= u["count"] <= room + 2      # noqa: E731
    return own + [u for u in units if fits(u)], len(own) + sum(1 for u in units[:n_scripted] if fits(u))


def _stamp(frame, base, at, value):
    """The 24 bits of `value` at absolute bit `at` of the stream, as far as they lie in the frame that starts at bit `base`."""
    n = 8 * len(frame)
    for k in range(24):
        i = at + k - base
        if 0 <= i < n:
            mask = 1 << (7 - (i & 7))
            frame[i >> 3] = (frame[i >> 3] | mask) if (value >> (23 - k)) & 1 else (frame[i >> 3] & ~mask)


def build_scenario(kbps, seed, variant, n_frames=N_FRAMES):
    """(frames [n_frames, 3 kbps] uint8, facts).  facts["placed"]: units that went into a frame whose PAD the reference takes,
    facts["scripted_left"]: scripted units that found no such frame, facts["taken"]: per frame, whether its PAD is taken."""
    rng = np.random.default_rng([kbps, seed, variant, 1848])
    nb, A, vl = 3 * kbps, 24 * kbps, v_len(kbps)
    plan = frame_plan(kbps, variant)[:n_frames]
    units, n_scripted = mp2_units(kbps, seed)
    stamps = [(f * A + off, header(**h)) for f, (_, off, h) in enumerate(plan) if off is not None]
    decoy = pc.var_ci(pc.label_fields(rng, b"never", 1, 1))
    walk = SyncWalk(kbps)
    out, taken, at = [], [], 0
    for f, (style, _, _) in enumerate(plan):
        if style == "zeros":
            fr = bytearray(nb)
        elif style == "ones":
            fr = bytearray(b"\xff" * nb)
        elif style == "ones11":
            fr = bytearray(nb)
            _stamp(fr, 0, 5, 0xFFE000)                                          # 11 ones from bit 5, then zeros
        elif style == "ones20":
            fr = bytearray(nb)
            _stamp(fr, 0, 40, 0xFFFFF0)                                         # 20 ones from bit 40
        elif style == "random":
            fr = bytearray(rng.integers(0, 256, nb).astype(np.uint8).tobytes())
        else:
            fr = bytearray((rng.integers(0, 256, nb) & 0x7F).astype(np.uint8).tobytes())       # audio without a run of 12 ones

        def finish(pad):
            g = bytearray(fr)
            if pad is not None and style in ("low",):
                xp = pad[:-2][-vl:]                                             # (an X-PAD longer than vLen: what is nearest to the F-PAD)
                g[vl - len(xp):vl] = xp                                         # the X-PAD, reversed, in front of the ScF-CRC bytes
                g[nb - 2:] = pad[-2:]                                           # L1, L0
            for a, v in stamps:
                if a + 24 > f * A and a < (f + 1) * A:
                    _stamp(g, f * A, a, v)
            return g
        trial = copy.copy(walk)
        done = trial.step(finish(decoy))
        pad = decoy
        if done and style == "low" and at < len(units):
            pad = units[at]["body"]
            at += 1
        g = finish(pad)
        assert walk.step(g) == done                                             # (the PAD bytes lie behind the completion or inside the frame's data)
        taken.append(done)
        out.append(np.frombuffer(bytes(g), np.uint8))
    return np.stack(out), {"placed": at, "scripted_left": max(0, n_scripted - at), "taken": taken}


_cache = {}


def scenario(kbps, seed, variant, n_frames=N_FRAMES):
    key = (kbps, seed, variant, n_frames)
    if key not in _cache:
        _cache[key] = build_scenario(kbps, seed, variant, n_frames)
    return _cache[key]


# ---- the sets the tests use --------------------------------------------------------------------------------------------------------------
PROT = pc.PROT
# (kbps, kind) per slot: "mp2" a DAB audio slot with PAD decoding from its MP2 frames, "pad" / "dab+" / "pkt" / "plain" as tests/pad_cases.py
STAGE_LAYOUTS = [
    [(8, "mp2"), (384, "mp2"), (64, "pad"), (16, "pkt"), (56, "mp2")],
    [(48, "mp2"), (24, "plain"), (128, "mp2"), (32, "pad"), (8, "mp2")],
]
STAGE_STREAMS = [0, 1, 0, 1]                     # layout of stream s; streams 0-1 carry variant 0 of frame_plan, streams 2-3 variant 1
PACKET_ADDRESS = pc.PACKET_ADDRESS
seed_of = pc.seed_of


def variant_of(s):
    return s // 2


def kinds(s):
    return STAGE_LAYOUTS[STAGE_STREAMS[s]]


def mp2_slots():
    return [(s, j, kbps) for s in range(len(STAGE_STREAMS)) for j, (kbps, kind) in enumerate(kinds(s)) if kind == "mp2"]


def stage_layout(lay):
    k = STAGE_LAYOUTS[lay]
    return dabplus_layout([(kbps, PROT, 0) for kbps, _ in k], dab_plus=[int(kind in ("pad", "dab+")) for _, kind in k])


def slot_frames(s, j, kbps, kind, n_frames=N_FRAMES):
    if kind == "mp2":
        return scenario(kbps, seed_of(s, j), variant_of(s), n_frames)[0]
    if kind == "plain":
        return np.random.default_rng([s, j, 7]).integers(0, 256, (n_frames, 3 * kbps)).astype(np.uint8)
    return pc.slot_frames(s, j, kbps, kind, n_frames)


boundary_schedule = pc.boundary_schedule
_stage_cache, _model_cache = {}, {}


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16, per-slot oracle results) of stream s.  Cached: the
    tests of one process share the arrays and leave them unchanged."""
    if s not in _stage_cache:
        layout = stage_layout(STAGE_STREAMS[s])
        frames = [slot_frames(s, j, kbps, kind) for j, (kbps, kind) in enumerate(kinds(s))]
        cifs = cifs_of(layout, frames, np.random.default_rng([12, s]))
        _stage_cache[s] = (layout, frames, cifs, oracle_results(layout, cifs))
    return _stage_cache[s]


def slot_model(s, j, limit=None, frames=None):
    """The model of MP2 slot (s, j) on its intended logical frames (the oracle back end decodes the coded frames back to exactly these:
    test_mp2_pad_cases.py)."""
    key = (s, j, limit)
    if frames is not None:
        return run_model(kinds(s)[j][0], frames, limit)
    if key not in _model_cache:
        kbps = kinds(s)[j][0]
        _model_cache[key] = run_model(kbps, scenario(kbps, seed_of(s, j), variant_of(s))[0], limit)
    return _model_cache[key]
