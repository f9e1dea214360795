"""Shared by test_mp2_audio_cases.py (no device) and the GPU tests of the MP2 audio stage (k_mp2_audio): Mp2Processor's frame assembly and
its MP2 decoder (base/backend/audio/mp2processor.cpp:197-243, :292-609 and :678-763, kjmp2) restated bit-serially, line by line, in Python
with every 32-bit operation wrapped as two's complement -- the model every device result is compared with, exactly -- a bitstream builder
that makes an MP2 frame from a chosen header, allocation, scfsi, scale factors and sample codes, and the scenarios, placed in logical
frames at bit offsets that are not multiples of 8.  mp2processor.cpp cannot be compiled without the GUI's headers, so parity with the
reference's object code is unpinned; every branch of the restatement cites its line (mp2: mp2processor.cpp) and counts itself in `branch`."""
import collections
import math

import numpy as np

import dabplus_cases as dc
import packet_cases as pkc
import pad_cases as pc
from dabstar_amd.lib import MP2_AUDIO_FRAME, MP2_AUDIO_STATS, MP2_GET_DATA, MP2_GET_RATE, MP2_SEARCHING

BATCH = dc.BATCH
N_BATCHES = 6
N_FRAMES = N_BATCHES * BATCH                     # 168 logical frames
PCM_BYTES = 4608                                 # 1152 stereo int16 samples (KJMP2_SAMPLES_PER_FRAME * 2)
STAT_FIELDS = tuple(k for k in MP2_AUDIO_STATS.names if k not in ("launches", "frames_lost"))      # what the model knows

# ---- tables (mp2:61-189); test_mp2_audio_cases.py compares them with csrc/mp2_core.h and, where the reference tree is present, with its
# initialisers ------------------------------------------------------------------------------------------------------------------------------
STEREO, JOINT_STEREO, DUAL_CHANNEL, MONO = 0, 1, 2, 3                                               # mp2:55-58
SAMPLE_RATES = (44100, 48000, 32000, 0, 22050, 24000, 16000, 0)                                     # mp2:61-64
BITRATES = (32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384,                         # mp2:67-70
            8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160)
SCF_BASE = (0x02000000, 0x01965FEA, 0x01428A30)                                                     # mp2:73
D = [                                                                                               # mp2:76-113
    0, 0, 0, 0, 0, 0, 0, -1, -1, -1, -1, -2, -2, -3, -3, -4,
    -4, -5, -6, -6, -7, -8, -9, -10, -12, -13, -15, -16, -18, -20, -23, -25,
    -28, -30, -34, -37, -40, -44, -48, -52, -57, -62, -67, -72, -78, -84, -90, -96,
    -103, -110, -116, -124, -131, -138, -146, -153, -160, -168, -175, -182, -189, -195, -201, -207,
    213, 218, 222, 225, 227, 228, 228, 227, 224, 221, 215, 208, 200, 189, 177, 163,
    146, 127, 106, 83, 57, 29, -1, -35, -71, -110, -152, -196, -243, -293, -346, -400,
    -458, -518, -580, -644, -710, -778, -847, -918, -990, -1063, -1136, -1209, -1282, -1355, -1427, -1497,
    -1566, -1633, -1697, -1758, -1816, -1869, -1918, -1961, -2000, -2031, -2056, -2074, -2084, -2086, -2079, -2062,
    2037, 2000, 1952, 1893, 1822, 1739, 1644, 1535, 1414, 1280, 1131, 970, 794, 605, 402, 185,
    -44, -287, -544, -813, -1094, -1387, -1691, -2005, -2329, -2662, -3003, -3350, -3704, -4062, -4424, -4787,
    -5152, -5516, -5878, -6236, -6588, -6934, -7270, -7596, -7909, -8208, -8490, -8754, -8997, -9218, -9415, -9584,
    -9726, -9837, -9915, -9958, -9965, -9934, -9862, -9749, -9591, -9388, -9138, -8839, -8491, -8091, -7639, -7133,
    6574, 5959, 5288, 4561, 3776, 2935, 2037, 1082, 70, -997, -2121, -3299, -4532, -5817, -7153, -8539,
    -9974, -11454, -12979, -14547, -16154, -17798, -19477, -21188, -22928, -24693, -26481, -28288, -30111, -31946, -33790, -35639,
    -37488, -39335, -41175, -43005, -44820, -46616, -48389, -50136, -51852, -53533, -55177, -56777, -58332, -59837, -61288, -62683,
    -64018, -65289, -66493, -67628, -68691, -69678, -70589, -71419, -72168, -72834, -73414, -73907, -74312, -74629, -74855, -74991,
    75038, 74992, 74856, 74630, 74313, 73908, 73415, 72835, 72169, 71420, 70590, 69679, 68692, 67629, 66494, 65290,
    64019, 62684, 61289, 59838, 58333, 56778, 55178, 53534, 51853, 50137, 48390, 46617, 44821, 43006, 41176, 39336,
    37489, 35640, 33791, 31947, 30112, 28289, 26482, 24694, 22929, 21189, 19478, 17799, 16155, 14548, 12980, 11455,
    9975, 8540, 7154, 5818, 4533, 3300, 2122, 998, -69, -1081, -2036, -2934, -3775, -4560, -5287, -5958,
    6574, 7134, 7640, 8092, 8492, 8840, 9139, 9389, 9592, 9750, 9863, 9935, 9966, 9959, 9916, 9838,
    9727, 9585, 9416, 9219, 8998, 8755, 8491, 8209, 7910, 7597, 7271, 6935, 6589, 6237, 5879, 5517,
    5153, 4788, 4425, 4063, 3705, 3351, 3004, 2663, 2330, 2006, 1692, 1388, 1095, 814, 545, 288,
    45, -184, -401, -604, -793, -969, -1130, -1279, -1413, -1534, -1643, -1738, -1821, -1892, -1951, -1999,
    2037, 2063, 2080, 2087, 2085, 2075, 2057, 2032, 2001, 1962, 1919, 1870, 1817, 1759, 1698, 1634,
    1567, 1498, 1428, 1356, 1283, 1210, 1137, 1064, 991, 919, 848, 779, 711, 645, 581, 519,
    459, 401, 347, 294, 244, 197, 153, 111, 72, 36, 2, -28, -56, -82, -105, -126,
    -145, -162, -176, -188, -199, -207, -214, -220, -223, -226, -227, -227, -226, -224, -221, -217,
    213, 208, 202, 196, 190, 183, 176, 169, 161, 154, 147, 139, 132, 125, 117, 111,
    104, 97, 91, 85, 79, 73, 68, 63, 58, 53, 49, 45, 41, 38, 35, 31,
    29, 26, 24, 21, 19, 17, 16, 14, 13, 11, 10, 9, 8, 7, 7, 6,
    5, 5, 4, 4, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1,
]
QUANT_LUT_STEP1 = ((0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2),                                      # mp2:119-124 mono / stereo
                   (0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2))
TAB_A, TAB_B, TAB_C, TAB_D = 27 | 64, 30 | 64, 8, 12                                                # mp2:127-130
QUANT_LUT_STEP2 = ((TAB_C, TAB_C, TAB_D), (TAB_A, TAB_A, TAB_A), (TAB_B, TAB_A, TAB_B))             # mp2:132-137
QUANT_LUT_STEP3 = (                                                                                 # mp2:141-161, rows padded with zeros to 32 as the C arrays are
    (0x44,) * 2 + (0x34,) * 10 + (0,) * 20,
    (0x43,) * 3 + (0x42,) * 8 + (0x31,) * 12 + (0x20,) * 7 + (0,) * 2,
    (0x45,) * 4 + (0x34,) * 7 + (0x24,) * 19 + (0,) * 2,
)
QUANT_LUT_STEP4 = (                                                                                 # mp2:164-169 (rows padded with zeros to 16)
    (0, 1, 2, 17) + (0,) * 12,
    (0, 1, 2, 3, 4, 5, 6, 17) + (0,) * 8,
    (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 17),
    (0, 1, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17),
    (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17),
    (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
)
QUANTIZER_TABLE = ((3, 1, 5), (5, 1, 7), (7, 0, 3), (9, 1, 10), (15, 0, 4), (31, 0, 5), (63, 0, 6), (127, 0, 7), (255, 0, 8),      # mp2:172-189
                   (511, 0, 9), (1023, 0, 10), (2047, 0, 11), (4095, 0, 12), (8191, 0, 13), (16383, 0, 14), (32767, 0, 15), (65535, 0, 16))


def n_table():
    """mp2:206-212, N[64][32] as the constructor computes it."""
    return [[int(256.0 * math.cos(((16 + i) * ((j << 1) + 1)) * 0.0490873852123405)) for j in range(32)] for i in range(64)]


N = n_table()
_N64 = np.array(N, np.int64)
_D64 = np.array(D, np.int64)
# mp2:578-583 U[(i << 6) + j] = V[(t + (i << 7) + j) & 1023], U[(i << 6) + j + 32] = V[(t + (i << 7) + j + 96) & 1023]: the offsets from t
_U_OFFS = np.zeros(512, np.int64)
for _i in range(8):
    for _j in range(32):
        _U_OFFS[(_i << 6) + _j] = (_i << 7) + _j
        _U_OFFS[(_i << 6) + _j + 32] = (_i << 7) + _j + 96


def w32(x):
    """two's-complement wrap of an int (or int64 array) to 32 bits: what the reference's i32 arithmetic does on every target it runs on"""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def header_layout(b1, b2, b3):
    """What mp2:411-479 derive from header bytes 1-3 of a frame that passes the checks: dict(table, sblimit, bound, nch, mode, crc,
    frame_size), or None where the decoder returns 0.  Shared by the builder and the tests; the model walks the lines itself."""
    if (b1 & 0xF6) != 0xF4 or b2 - 0x10 >= 0xE0:
        return None
    bri = (b2 >> 4) - 1
    sf = (b2 >> 2) & 3
    if bri < 0 or bri > 13 or sf == 3:
        return None
    if not b1 & 8:
        sf += 4
        bri += 14
    mode = b3 >> 6
    bound = (((b3 >> 4) & 3) + 1) << 2 if mode == JOINT_STEREO else 0 if mode == MONO else 32
    if sf & 4:
        table, sblimit = 2, 30
    else:
        t = QUANT_LUT_STEP2[QUANT_LUT_STEP1[0 if mode == MONO else 1][bri]][sf]
        table, sblimit = t >> 6, t & 63
    return dict(table=table, sblimit=sblimit, bound=min(bound, sblimit), nch=1 if mode == MONO else 2, mode=mode, crc=not b1 & 1,
                frame_size=144000 * BITRATES[bri] // SAMPLE_RATES[sf] + ((b2 >> 1) & 1))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Mp2AudioModel:
    """Mp2Processor for ONE slot without its PAD and signals: add_to_frame one bit at a time into MP2frame, _mp2_decode_frame on every
    completed frame.  mut: single-line mutations (test_mp2_audio_cases.py shows that each changes the PCM of some scenario).
    snaps[k] = (records so far, dabx_mp2_audio_stats fields) after k logical frames; pcm[r] = the 2304 int16 of record r."""

    def __init__(self, kbps, first=0, mut=()):
        self.kbps, self.mut = kbps, frozenset(mut)
        self.framesize = 24 * kbps                                              # mp2:236 MP2framesize
        self.mp2frame = bytearray(2 * self.framesize)                           # mp2:237
        self.state = MP2_SEARCHING                                              # mp2:238
        self.header_count = self.bit_count = 0                                  # mp2:239-240
        self.number_of_frames = self.error_frames = 0                           # mp2:241-242
        self.voffs = 0                                                          # mp2:234
        self.sample_rate = 48000                                                # mp2:235
        self.V = np.zeros((2, 2048), np.int64)                                  # mp2:215-221 V[2][1024]; the upper half is only ever read by the "& 1023" mutation
        self.allocation = [[None] * 32, [None] * 32]                            # members of the class: they keep their values from frame to frame
        self.scfsi = [[0] * 32, [0] * 32]
        self.scalefactor = [[[0] * 3 for _ in range(32)] for _ in range(2)]
        self.sample = [[[0] * 3 for _ in range(32)] for _ in range(2)]
        self.stats = dict(decode_calls=0, frames_out=0, bad_header=0, refused=0, overread=0)
        self.branch = collections.Counter()
        self.rows, self.pcm = [], []
        self.max_product = 0                                                    # the largest |U[i] * D[i] + 32| met (mp2:587), before the wrap
        self.wraps = 0                                                          # ... and how many went past 2^31
        self.n_frames = first
        self.snaps = [self.snap()]

    def hit(self, line):
        self.branch[line] += 1

    def all_stats(self):
        return dict(self.stats, number_of_frames=self.number_of_frames, error_frames=self.error_frames, voffs=self.voffs,
                    sample_rate=self.sample_rate, active=1)

    def snap(self):
        return (len(self.rows), self.all_stats())

    def records(self):
        r = np.zeros(len(self.rows), MP2_AUDIO_FRAME)
        for k, (frame, rate, size, hdr, stereo, flags) in enumerate(self.rows):
            r[k]["byte_pos"], r[k]["frame"], r[k]["sample_rate"], r[k]["frame_size"] = k * PCM_BYTES, frame, rate, size
            r[k]["header"], r[k]["stereo"], r[k]["flags"] = hdr, stereo, flags
        return r

    def all_pcm(self):
        return np.concatenate(self.pcm).view(np.uint8) if self.pcm else np.zeros(0, np.uint8)

    # -- mp2:250-285 ----------------------------------------------------------------------------------------------------------------------
    def set_sample_rate(self, rate):
        if self.sample_rate == rate:                                            # mp2:252
            return
        if rate != 48000 and rate != 24000:                                     # mp2:257-261
            self.hit("mp2:257 unsupported rate %d" % rate)
            return
        self.hit("mp2:263 rate %d -> %d" % (self.sample_rate, rate))
        self.sample_rate = rate                                                 # mp2:263

    def get_mp2_sample_rate(self):
        f = self.mp2frame
        if f[0] != 0xFF or (f[1] & 0xF6) != 0xF4 or (f[2] - 0x10) >= 0xE0:      # mp2:277-282
            return 0
        return SAMPLE_RATES[(((f[1] & 0x08) >> 1) ^ 4) + ((f[2] >> 2) & 3)]     # mp2:283-284

    def add_bit_to_mp2(self, bit, nm):                                          # mp2:749-763
        mask = 1 << (7 - (nm & 7))
        self.mp2frame[nm >> 3] = (self.mp2frame[nm >> 3] | mask) if bit else (self.mp2frame[nm >> 3] & ~mask)

    # -- mp2:354-370 ----------------------------------------------------------------------------------------------------------------------
    def get_bits(self, n):
        result = self.bit_window >> (24 - n)                                    # mp2:358
        self.bit_window = (self.bit_window << n) & 0xFFFFFF                     # mp2:360
        self.bits_in_window -= n                                                # mp2:361
        while self.bits_in_window < 16:                                         # mp2:363
            if self.frame_pos >= len(self.mp2frame):                            # guard G1: past MP2frame the device reads zeros and flags the frame
                self.over = True
                byte = 0
            else:
                byte = self.mp2frame[self.frame_pos]
            self.frame_pos += 1
            self.bit_window |= byte << (16 - self.bits_in_window)               # mp2:365
            self.bits_in_window += 8                                            # mp2:366
        return result

    # -- mp2:292-297 ----------------------------------------------------------------------------------------------------------------------
    def read_allocation(self, sb, b2_table):
        table_idx = QUANT_LUT_STEP3[b2_table][sb]                               # mp2:294
        table_idx = QUANT_LUT_STEP4[table_idx & 15][self.get_bits(table_idx >> 4)]      # mp2:295
        return QUANTIZER_TABLE[table_idx - 1] if table_idx else None            # mp2:296

    # -- mp2:299-351 ----------------------------------------------------------------------------------------------------------------------
    def read_samples(self, q, scalefactor, out):
        if not q:                                                               # mp2:303-308
            out[0] = out[1] = out[2] = 0
            return
        if scalefactor == 63:                                                   # mp2:311-314
            self.hit("mp2:311 scale factor 63")
            scalefactor = 0
        else:
            adj = scalefactor // 3                                              # mp2:317
            scalefactor = (SCF_BASE[scalefactor % 3] + ((1 << adj) >> 1)) >> adj        # mp2:318
        adj = q[0]                                                              # mp2:322 nlevels
        if q[1]:                                                                # mp2:323-330 grouped
            val = self.get_bits(q[2])
            if val >= adj * adj * adj:
                self.hit("mp2:325 grouped code word beyond nlevels^3")
            out[0] = val % adj
            val //= adj
            out[1] = val % adj
            out[2] = val // adj
        else:                                                                   # mp2:331-337
            for idx in range(3):
                out[idx] = self.get_bits(q[2])
        scale = 65536 // (adj + 1)                                              # mp2:340
        adj = ((adj + 1) >> 1) - 1                                              # mp2:341
        for idx in range(3):
            val = w32((adj - out[idx]) * scale)                                 # mp2:345
            out[idx] = w32(w32(w32(val * (scalefactor >> 12)) + (w32(w32(val * (scalefactor & 4095)) + 2048) >> 12)) >> 12)     # mp2:347-349

    # -- mp2:377-609 ----------------------------------------------------------------------------------------------------------------------
    def decode_frame(self, pcm):
        f = self.mp2frame
        self.stats["decode_calls"] += 1
        self.number_of_frames += 1                                              # mp2:388
        if self.number_of_frames >= 25:                                         # mp2:389-394
            self.hit("mp2:389 the window of 25 frames closes")
            self.number_of_frames = 0
            self.error_frames = 0
        if f[0] != 0xFF or (f[1] & 0xF6) != 0xF4 or (f[2] - 0x10) >= 0xE0:      # mp2:397-403
            self.hit("mp2:397 bad header: layer bits %d, bit-rate index %d" % ((f[1] >> 1) & 3, f[2] >> 4))
            self.error_frames += 1
            self.stats["bad_header"] += 1
            return 0
        self.bit_window = f[2] << 16                                            # mp2:406-408
        self.bits_in_window = 8
        self.frame_pos = 3
        self.over = False
        bit_rate_index_minus1 = (self.get_bits(4) - 1) & 0xFFFFFFFF             # mp2:411
        if bit_rate_index_minus1 > 13:                                          # mp2:412-415
            self.hit("mp2:412 free format (bit-rate index 0)")
            self.stats["refused"] += 1
            return 0
        sampling_frequency = self.get_bits(2)                                   # mp2:417
        if sampling_frequency == 3:                                             # mp2:418-421
            self.hit("mp2:418 reserved sampling frequency")
            self.stats["refused"] += 1
            return 0
        if (f[1] & 0x08) == 0:                                                  # mp2:423-427
            sampling_frequency += 4
            bit_rate_index_minus1 += 14
        padding_bit = self.get_bits(1)                                          # mp2:429
        self.get_bits(1)                                                        # mp2:430
        mode = self.get_bits(2)                                                 # mp2:431
        if mode == JOINT_STEREO:                                                # mp2:434-442
            bound = (self.get_bits(2) + 1) << 2
            self.hit("mp2:436 joint stereo, bound %d" % bound)
        else:
            self.get_bits(2)
            bound = 0 if mode == MONO else 32
            self.hit("mp2:441 mode %d" % mode)
        stereo = int(mode == JOINT_STEREO or mode == STEREO)                    # mp2:444
        self.get_bits(4)                                                        # mp2:447
        if (f[1] & 1) == 0:                                                     # mp2:448-451
            self.hit("mp2:448 CRC present")
            self.get_bits(16)
        else:
            self.hit("mp2:448 no CRC")
        frame_size = 144000 * BITRATES[bit_rate_index_minus1] // SAMPLE_RATES[sampling_frequency] + padding_bit       # mp2:454
        if sampling_frequency & 4:                                              # mp2:462-467
            table_idx, sblimit = 2, 30
            self.hit("mp2:462 LSR table")
        else:                                                                   # mp2:468-476
            table_idx = 0 if mode == MONO else 1
            table_idx = QUANT_LUT_STEP1[table_idx][bit_rate_index_minus1]
            table_idx = QUANT_LUT_STEP2[table_idx][sampling_frequency]
            sblimit = table_idx & 63
            self.hit("mp2:473 table %s%s" % ({TAB_A: "A", TAB_B: "B", TAB_C: "C", TAB_D: "D"}[table_idx],
                                             "" if sampling_frequency == 1 else " from a %d Hz header" % SAMPLE_RATES[sampling_frequency]))
            table_idx >>= 6
        if bound > sblimit:                                                     # mp2:478-479
            if mode == JOINT_STEREO:
                self.hit("mp2:478 joint-stereo bound above sblimit")
            bound = sblimit
        al, sc, sf, sm = self.allocation, self.scfsi, self.scalefactor, self.sample
        for sb in range(bound):                                                 # mp2:482-484
            for ch in range(2):
                al[ch][sb] = self.read_allocation(sb, table_idx)
        for sb in range(bound, sblimit):                                        # mp2:486-487
            al[0][sb] = al[1][sb] = self.read_allocation(sb, table_idx)
        nch = 1 if mode == MONO else 2                                          # mp2:490
        for sb in range(sblimit):                                               # mp2:491-499
            for ch in range(nch):
                if al[ch][sb]:
                    sc[ch][sb] = self.get_bits(2)
            if mode == MONO:
                sc[1][sb] = sc[0][sb]
        for sb in range(sblimit):                                               # mp2:502-535
            for ch in range(nch):
                if al[ch][sb]:
                    s = sf[ch][sb]
                    k = sc[ch][sb]
                    self.hit("mp2:508 scfsi %d" % k)
                    if k == 0:
                        s[0] = self.get_bits(6); s[1] = self.get_bits(6); s[2] = self.get_bits(6)
                    elif k == 1:
                        s[0] = s[1] = self.get_bits(6); s[2] = self.get_bits(6)
                    elif k == 2:
                        s[0] = s[1] = s[2] = self.get_bits(6)
                    else:
                        s[0] = self.get_bits(6); s[1] = s[2] = self.get_bits(6)
            if mode == MONO:
                for part in range(3):
                    sf[1][sb][part] = sf[0][sb][part]
        smp = np.zeros((2, 36, 32), np.int64)                                   # sample[ch][sb][idx] of every granule, for the synthesis below
        for part in range(3):                                                   # mp2:538-556
            for gr in range(4):
                for sb in range(bound):
                    for ch in range(2):
                        self.read_samples(al[ch][sb], sf[ch][sb][part], sm[ch][sb])
                for sb in range(bound, sblimit):
                    self.read_samples(al[0][sb], sf[0][sb][part], sm[0][sb])
                    for idx in range(3):
                        sm[1][sb][idx] = sm[0][sb][idx]
                for ch in range(2):
                    for sb in range(sblimit, 32):
                        for idx in range(3):
                            sm[ch][sb][idx] = 0
                g = 4 * part + gr
                for ch in range(2):
                    for sb in range(32):
                        for idx in range(3):
                            smp[ch, 3 * g + idx, sb] = sm[ch][sb][idx]
        self.synthesis(smp, pcm)                                                # mp2:558-606
        if self.over:
            self.hit("G1 the refill ran past MP2frame")
            self.stats["overread"] += 1
        self.rows.append((self.n_frames, self.sample_rate, frame_size, (f[1], f[2], f[3]), stereo, 1 if self.over else 0))
        self.pcm.append(pcm.copy())
        self.stats["frames_out"] += 1
        return frame_size                                                       # mp2:608

    def synthesis(self, smp, pcm):
        """mp2:558-603 for the 36 sub-blocks of a frame (k = 3 * granule + idx); pcm[(k << 6) | (j << 1) | ch] as opPcm advances (:600, :605)."""
        mut = self.mut
        mask = 2047 if "and1023" in mut else 1023
        for k in range(36):
            self.voffs = t = (self.voffs - 64) & 1023                           # mp2:562
            for ch in range(2):
                s = w32(_N64 @ smp[ch, k])                                      # mp2:567-571
                self.V[ch, t:t + 64] = w32(s + (0 if "round574" in mut else 8192)) >> 14        # mp2:574
                u = self.V[ch, (t + _U_OFFS) & mask]                            # mp2:578-583
                p = u * _D64 + (0 if "round587" in mut else 32)                 # mp2:587
                big = int(np.abs(p).max())
                if big > self.max_product:
                    self.max_product = big
                n_wrap = int(np.count_nonzero((p >= 1 << 31) | (p < -(1 << 31))))
                if n_wrap:
                    self.hit("mp2:587 U[i] * D[i] wraps")
                    self.wraps += n_wrap
                u = w32(p) >> 6
                acc = u.reshape(16, 32).sum(axis=0)                             # mp2:592-594 (16 terms below 2^26 each: no wrap)
                acc = acc if "sign594" in mut else -acc
                acc = (acc + 8) >> 4                                            # mp2:595
                if "clamp" not in mut:                                          # mp2:596-599
                    if (acc < -32768).any() or (acc > 32767).any():
                        self.hit("mp2:596 clamp")
                    acc = np.clip(acc, -32768, 32767)
                pcm[(k << 6) + 2 * np.arange(32) + ch] = (acc & 0xFFFF).astype(np.uint16).view(np.int16)      # mp2:600

    # -- mp2:678-747 ----------------------------------------------------------------------------------------------------------------------
    def add_to_frame(self, frame):
        bits = np.unpackbits(np.frombuffer(bytes(frame), np.uint8)).tolist()
        amount = self.framesize                                                 # mp2:681
        assert amount == len(bits)                                              # mp2:682
        lf = self.framesize if self.sample_rate == 48000 else 2 * self.framesize        # mp2:680
        for i in range(amount):                                                 # mp2:685
            if self.state == MP2_GET_DATA:                                      # mp2:687
                self.add_bit_to_mp2(bits[i], self.bit_count)                    # mp2:689
                self.bit_count += 1
                if self.bit_count >= lf:                                        # mp2:691
                    self.hit("mp2:691 frame complete %s, %d Hz" % ("at a byte boundary" if i % 8 == 7 else "inside a byte", self.sample_rate))
                    pcm = np.zeros(PCM_BYTES // 2, np.int16)                    # mp2:693 (a frame that is refused emits nothing: its content does not matter)
                    self.decode_frame(pcm)                                      # mp2:696
                    self.state = MP2_SEARCHING                                  # mp2:710-712
                    self.header_count = 0
                    self.bit_count = 0
            elif self.state == MP2_SEARCHING:                                   # mp2:715
                if bits[i] == 1:                                                # mp2:718
                    self.header_count += 1
                    if self.header_count == 12:                                 # mp2:720
                        self.bit_count = 0                                      # mp2:722-726
                        while self.bit_count < 12:
                            self.add_bit_to_mp2(1, self.bit_count)
                            self.bit_count += 1
                        self.state = MP2_GET_RATE                               # mp2:727
                else:                                                           # mp2:730-733
                    self.header_count = 0
            else:                                                               # mp2:735 GetSampleRate
                self.add_bit_to_mp2(bits[i], self.bit_count)                    # mp2:737
                self.bit_count += 1
                if self.bit_count == 24:                                        # mp2:738
                    self.set_sample_rate(self.get_mp2_sample_rate())            # mp2:740
                    lf = self.framesize if self.sample_rate == 48000 else 2 * self.framesize    # mp2:741
                    self.state = MP2_GET_DATA                                   # mp2:742
        self.n_frames += 1
        self.snaps.append(self.snap())


def run_model(kbps, frames, first=0, mut=()):
    m = Mp2AudioModel(kbps, first, mut)
    for f in frames:
        m.add_to_frame(f)
    return m


# ---- the builder -------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits.extend((value >> (n - 1 - k)) & 1 for k in range(n))


def build_frame(n_bytes, rng, mpeg1=1, layer=2, prot=1, bitrate=10, rate=1, padding=0, private=0, mode=STEREO, mode_ext=0, tail=0, crc=0xBEEF,
                alloc="random", scfsi="random", scf="random", code="random", fill="random"):
    """One MP2 frame of n_bytes bytes: the 32 header bits, the CRC word when prot == 0, then -- as far as header_layout knows the header
    -- allocation, scfsi, scale factors and the 12 granules of sample codes in the order mp2:482-551 read them.  alloc / scfsi / scf / code:
    "random", or a function (sb, ch[, part / granule]) -> the field's value (allocation: the raw index of nbal bits; code: the raw code word,
    or per sample).  What does not fit n_bytes is cut off (the decoder then reads what lies behind the frame); what is left is `fill`."""
    w = BitWriter()
    w.put(0xFFF, 12); w.put(mpeg1, 1); w.put(layer, 2); w.put(prot, 1)
    w.put(bitrate, 4); w.put(rate, 2); w.put(padding, 1); w.put(private, 1)
    w.put(mode, 2); w.put(mode_ext, 2); w.put(tail, 4)
    b = np.packbits(np.array(w.bits, np.uint8))
    lay = header_layout(int(b[1]), int(b[2]), int(b[3]))
    if prot == 0:
        w.put(crc, 16)
    if lay is not None:
        pick = lambda f, hi, *a: int(rng.integers(0, hi)) if f == "random" else int(f(*a))      # noqa: E731
        tab, sblimit, bound, nch = lay["table"], lay["sblimit"], lay["bound"], lay["nch"]
        q = [[0] * 32, [0] * 32]
        for sb in range(sblimit):
            step3 = QUANT_LUT_STEP3[tab][sb]
            for ch in range(2 if sb < bound else 1):
                a = pick(alloc, 1 << (step3 >> 4), sb, ch) & ((1 << (step3 >> 4)) - 1)
                w.put(a, step3 >> 4)
                q[ch][sb] = QUANT_LUT_STEP4[step3 & 15][a]
            if sb >= bound:
                q[1][sb] = q[0][sb]
        sel = [[0] * 32, [0] * 32]
        for sb in range(sblimit):
            for ch in range(nch):
                if q[ch][sb]:
                    sel[ch][sb] = pick(scfsi, 4, sb, ch)
                    w.put(sel[ch][sb], 2)
        for sb in range(sblimit):
            for ch in range(nch):
                if q[ch][sb]:
                    for part in range((3, 2, 1, 2)[sel[ch][sb]]):
                        w.put(pick(scf, 64, sb, ch, part), 6)
        for g in range(12):
            for sb in range(sblimit):
                for ch in range(2 if sb < bound else 1):
                    if q[ch][sb]:
                        nlevels, grouping, cw = QUANTIZER_TABLE[q[ch][sb] - 1]
                        for _ in range(1 if grouping else 3):
                            w.put(pick(code, 1 << cw, sb, ch, g), cw)
    bits = w.bits[:8 * n_bytes]
    n_fill = 8 * n_bytes - len(bits)
    if fill == "random":
        bits = bits + rng.integers(0, 2, n_fill).tolist()
    else:
        bits = bits + [fill] * n_fill
    return np.packbits(np.array(bits, np.uint8)), len(w.bits)


def max_alloc(sb, ch):
    return 15                                    # put() keeps the low nbal bits: the last entry of the subband's row, 16-bit samples in tables A and B


def _alloc_for(want_q):
    """allocation function that asks for quantiser `want_q` wherever the subband's row has it, 0 elsewhere (needs the table: built per frame)"""
    def make(tab):
        def f(sb, ch):
            row = QUANT_LUT_STEP4[QUANT_LUT_STEP3[tab][sb] & 15][:1 << (QUANT_LUT_STEP3[tab][sb] >> 4)]
            return row.index(want_q) if want_q in row else 0
        return f
    return make


# One template per kind of frame the issue lists.  h: header fields; the other keys go to build_frame (a key that names a function of the
# table is resolved by frame_of).  rate = None: the slot's sticky rate decides how long the frame is, as in the decoder.
TEMPLATES = [
    ("A stereo", dict(bitrate=10)),
    ("A stereo CRC", dict(bitrate=12, prot=0)),
    ("A mono", dict(bitrate=6, mode=MONO)),
    ("C stereo", dict(bitrate=4)),
    ("C mono CRC", dict(bitrate=1, mode=MONO, prot=0)),
    ("A dual", dict(bitrate=9, mode=DUAL_CHANNEL, padding=1)),
    ("A joint 4", dict(bitrate=11, mode=JOINT_STEREO, mode_ext=0)),
    ("A joint 8", dict(bitrate=11, mode=JOINT_STEREO, mode_ext=1, private=1)),
    ("A joint 12", dict(bitrate=8, mode=JOINT_STEREO, mode_ext=2)),
    ("A joint 16", dict(bitrate=14, mode=JOINT_STEREO, mode_ext=3)),
    ("C joint 12 above sblimit", dict(bitrate=3, mode=JOINT_STEREO, mode_ext=2)),
    ("B from 44.1 kHz", dict(bitrate=13, rate=0)),
    ("D from 32 kHz joint 16", dict(bitrate=2, rate=2, mode=JOINT_STEREO, mode_ext=3)),
    ("B from 32 kHz mono", dict(bitrate=10, rate=2, mode=MONO)),
    ("silence", dict(bitrate=10, alloc=lambda sb, ch: 0)),
    ("scale factor 63", dict(bitrate=7, scf=lambda sb, ch, part: 63 if (sb + part) % 2 else 0)),
    ("grouped codes beyond nlevels^3", dict(bitrate=4, alloc_q=1, code=lambda sb, ch, g: 31 - (g & 3))),
    ("grouped codes of 3 and 5 levels, all ones", dict(bitrate=10, alloc=lambda sb, ch: 1 + (sb & 1) * 2 if sb < 3 else 2 - (sb & 1), code=lambda sb, ch, g: (1 << 10) - 1 - g)),
    ("index 0", dict(bitrate=0)),
    ("index 15", dict(bitrate=15)),
    ("layer I bits", dict(bitrate=10, layer=3)),
    ("layer III bits", dict(bitrate=10, layer=1)),
    ("layer 0 bits", dict(bitrate=10, layer=0)),
    ("reserved rate", dict(bitrate=10, rate=3)),
    ("reserved rate, MPEG-2", dict(bitrate=10, rate=3, mpeg1=0)),
    ("over-reading header", dict(bitrate=13, rate=0, alloc=max_alloc, scfsi=lambda sb, ch: 0)),
    ("in-range full scale DC", dict(bitrate=14, alloc=max_alloc, scfsi=lambda sb, ch: 2, scf=lambda sb, ch, part: 0, code=lambda sb, ch, g: 0)),
    ("LSR stereo", dict(mpeg1=0, bitrate=8)),
    ("LSR mono", dict(mpeg1=0, bitrate=3, mode=MONO)),
    ("LSR joint 8 CRC", dict(mpeg1=0, bitrate=12, mode=JOINT_STEREO, mode_ext=1, prot=0)),
    ("LSR 22.05 kHz", dict(mpeg1=0, bitrate=5, rate=0)),
    # every subband at 9 levels, the code word 1023 = (6, 5, 12): the third sample is 8 steps below the lowest level, -104 848 at scale factor 0;
    # row 48 of N (all -256) times 30 of them is V = 49 147, times D[240] = -64 018 is -3.1e9: past -2^31 (mp2:587)
    ("DC beyond full scale: the wrap", dict(mpeg1=0, bitrate=14, mode=MONO, alloc_q=4, scfsi=lambda sb, ch: 2, scf=lambda sb, ch, part: 0, code=lambda sb, ch, g: 1023)),
    ("LSR to 48 kHz: stale bytes", dict(bitrate=13, alloc=max_alloc, scfsi=lambda sb, ch: 3)),
    ("A stereo again", dict(bitrate=9, padding=1)),
]


def frame_of(kbps, rng, sticky, name, spec):
    """(bytes of the frame, sticky rate behind its header, bits the fields asked for)"""
    spec = dict(spec)
    h = {k: spec[k] for k in ("mpeg1", "layer", "bitrate", "rate") if k in spec}
    mpeg1, layer, bitrate, rate = h.get("mpeg1", 1), h.get("layer", 2), h.get("bitrate", 10), h.get("rate", 1)
    if layer == 2 and bitrate != 15:                                            # mp2:277-284 with :252-263: what the header does to the sticky rate
        r = SAMPLE_RATES[(0 if mpeg1 else 4) + rate]
        if r in (48000, 24000):
            sticky = r
    n_bytes = 3 * kbps if sticky == 48000 else 6 * kbps
    if "alloc_q" in spec:
        want = spec.pop("alloc_q")
        b1, b2 = 0xF0 | mpeg1 << 3 | layer << 1 | spec.get("prot", 1), bitrate << 4 | rate << 2
        lay = header_layout(b1, b2, spec.get("mode", STEREO) << 6 | spec.get("mode_ext", 0) << 4)
        spec["alloc"] = _alloc_for(want)(lay["table"]) if lay else "random"
    data, asked = build_frame(n_bytes, rng, **spec)
    return data, sticky, asked


def build_scenario(kbps, seed, offset, n_frames=N_FRAMES):
    """(frames [n_frames, 3 kbps] uint8, facts): the MP2 frames of TEMPLATES one behind the other, again and again with fresh random fields,
    from bit `offset` of the slot's first logical frame on (zeros in front); facts["names"]: the template of every MP2 frame placed whole."""
    rng = np.random.default_rng([kbps, seed, offset, 1877])
    total = n_frames * 3 * kbps
    stream = np.zeros(8 * total + 8 * 6 * kbps, np.uint8)
    at, sticky, names, k = offset, 48000, [], 0
    while at < 8 * total:
        name, spec = TEMPLATES[k % len(TEMPLATES)]
        data, sticky, _ = frame_of(kbps, rng, sticky, name, spec)
        stream[at:at + 8 * len(data)] = np.unpackbits(data)
        at += 8 * len(data)
        if at <= 8 * total:
            names.append(name)
        k += 1
    return np.packbits(stream[:8 * total]).reshape(n_frames, 3 * kbps), {"names": names}


_cache = {}


def scenario(kbps, seed, offset, n_frames=N_FRAMES):
    key = (kbps, seed, offset, n_frames)
    if key not in _cache:
        _cache[key] = build_scenario(kbps, seed, offset, n_frames)
    return _cache[key]


# ---- the sets the tests use --------------------------------------------------------------------------------------------------------------
PROT = pc.PROT
PACKET_ADDRESS = pc.PACKET_ADDRESS
# (kbps, kind) per slot: "aud" a DAB audio slot with the MP2 audio mode on, "aud+pad" one that also has PAD decoding from its MP2 frames,
# "pad" a DAB+ slot with PAD decoding, "pkt" a packet-mode slot, "plain" a slot in plain logical frames
STAGE_LAYOUTS = [
    [(8, "aud"), (384, "aud"), (64, "pad"), (16, "pkt"), (56, "aud+pad")],
    [(48, "aud"), (96, "aud"), (128, "aud+pad"), (32, "pad"), (24, "plain")],
]
STAGE_STREAMS = [0, 1, 0, 1]                     # layout of stream s
OFFSETS = [13, 6, 8 * 7 + 3, 1]                  # bit offset of stream s's MP2 streams in their first logical frame, + the slot's index (one is a multiple of 8)


def kinds(s):
    return STAGE_LAYOUTS[STAGE_STREAMS[s]]


def is_audio(kind):
    return kind.startswith("aud")


def seed_of(s, j):
    return 10 * s + j


def audio_slots():
    return [(s, j, kbps) for s in range(len(STAGE_STREAMS)) for j, (kbps, kind) in enumerate(kinds(s)) if is_audio(kind)]


def stage_layout(lay):
    k = STAGE_LAYOUTS[lay]
    return dc.dabplus_layout([(kbps, PROT, 0) for kbps, _ in k], dab_plus=[int(kind == "pad") for _, kind in k])


def slot_frames(s, j, kbps, kind, n_frames=N_FRAMES):
    if is_audio(kind):
        return scenario(kbps, seed_of(s, j), OFFSETS[s] + j, n_frames)[0]
    if kind == "plain":
        return np.random.default_rng([s, j, 7]).integers(0, 256, (n_frames, 3 * kbps)).astype(np.uint8)
    return pc.slot_frames(s, j, kbps, kind, n_frames)


def boundary_schedule(n_streams):
    return pc.boundary_schedule(n_streams, N_FRAMES)


_stage_cache, _model_cache = {}, {}


def stream_case(s):
    """(layout, per-slot intended logical frames, CIFs [16 + N_FRAMES, 55296] int16) of stream s.  Cached: the tests of one process share
    the arrays and leave them unchanged."""
    if s not in _stage_cache:
        layout = stage_layout(STAGE_STREAMS[s])
        frames = [slot_frames(s, j, kbps, kind) for j, (kbps, kind) in enumerate(kinds(s))]
        _stage_cache[s] = (layout, frames, dc.cifs_of(layout, frames, np.random.default_rng([14, s])))
    return _stage_cache[s]


def slot_model(s, j):
    """The model of audio slot (s, j) on its intended logical frames, computed once."""
    if (s, j) not in _model_cache:
        kbps = kinds(s)[j][0]
        _model_cache[(s, j)] = run_model(kbps, slot_frames(s, j, kbps, kinds(s)[j][1]))
    return _model_cache[(s, j)]


def longest_parse_bits(table):
    """The most bits mp2:396-551 can read with quantiser table 0 (C / D), 1 (A / B) or 2 (LSR): CRC present, stereo, every subband of the
    largest sblimit at the widest quantiser of its row, scfsi 0."""
    sblimit = {0: 12, 1: 30, 2: 30}[table]
    bits = 32 + 16
    for sb in range(sblimit):
        step3 = QUANT_LUT_STEP3[table][sb]
        nbal = step3 >> 4
        widest = 0
        for a in range(1 << nbal):
            q = QUANT_LUT_STEP4[step3 & 15][a]
            if q:
                nlevels, grouping, cw = QUANTIZER_TABLE[q - 1]
                widest = max(widest, cw if grouping else 3 * cw)
        bits += 2 * (nbal + 2 + 18 + 12 * widest)
    return bits
