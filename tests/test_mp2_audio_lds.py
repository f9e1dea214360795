"""CPU: the LDS layout of k_mp2_audio (msc_stages.hip, Mp2AudioLds) and its bank behaviour under the gfx950 rules (tools/lds_conflicts.py,
after MI355X_MICROARCH.md "LDS"), access by access, in the manner of test_lds_layouts.py.

  frm   1152 B   the logical frame being walked
  mp2f  2320 B   MP2frame (6 kbps bytes kept, zeros behind)
  smp   2 x (36 x 32 + 16) int32   sample[ch][sub-block][sb]
  v     2 x 52 x 64 int32          V rows of a channel, oldest first: 16 of history, the frame's 36

39 440 bytes a block: four blocks fit a CU's 160 KiB, and a block's 165 VGPRs allow three waves per SIMD, so LDS is not what bounds occupancy."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import lds_conflicts as lc  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SMP_CH = 36 * 32 + 16                 # ints per channel of smp
V_CH = 52 * 64                        # ints per channel of v
FRM, MP2F = 1152, 2320
SMP0 = FRM + MP2F                     # byte offsets in the block's LDS (all members are 16-byte aligned)
V0 = SMP0 + 2 * SMP_CH * 4


def test_the_sizes_are_the_kernels():
    src = open(os.path.join(ROOT, "dabstar_amd", "csrc", "msc_stages.hip")).read()
    core = open(os.path.join(ROOT, "dabstar_amd", "csrc", "mp2_core.h")).read()
    assert "uint8_t frm[3 * MP2A_MAX_KBPS];" in src and "uint8_t mp2f[MP2A_FRAME_ROOM + 16];" in src
    assert "int smp[2][MP2A_SUBBLOCKS * 32 + 16];" in src and "int v[2][(MP2A_HIST_ROWS + MP2A_SUBBLOCKS) * 64];" in src
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (MP2A_MAX_KBPS|MP2A_HIST_ROWS|MP2A_SUBBLOCKS) = (\d+);", core)}
    assert consts == dict(MP2A_MAX_KBPS=384, MP2A_HIST_ROWS=16, MP2A_SUBBLOCKS=36) and "MP2A_FRAME_ROOM = 6 * MP2A_MAX_KBPS" in core
    assert V0 + 2 * V_CH * 4 == 39440 and SMP0 % 16 == 0 and V0 % 16 == 0
    assert 4 * 39440 <= 160 * 1024


def test_the_sample_stores_need_the_sixteen_ints_between_the_channels():
    """parse: lane 2 sb + ch stores sample[ch][k][sb] (ds_write_b32: two groups of 32 lanes, bank = dword mod 32).  A half wave holds 16
    subbands of both channels: with the channels 36 x 32 ints apart (= 0 mod 32) every bank would be hit twice."""
    for k in (0, 17, 35):
        addr = [SMP0 + 4 * ((l & 1) * SMP_CH + k * 32 + (l >> 1)) for l in range(64)]
        assert lc.extra_cycles(addr, 4, "w")[0] == 0, k
        flat = [SMP0 + 4 * ((l & 1) * 36 * 32 + k * 32 + (l >> 1)) for l in range(64)]
        assert lc.extra_cycles(flat, 4, "w")[0] == 2, k            # one extra cycle in each half


def test_matrixing_reads_broadcasts_and_stores_rows():
    """matrix: every lane of a wave reads the same 32 samples (16-byte reads of one address: broadcasts) and lane i stores V[ch][row][i]."""
    for c in range(2):
        for k in (0, 35):
            for q in range(8):
                addr = [SMP0 + 4 * (c * SMP_CH + k * 32 + 4 * q)] * 64
                assert lc.extra_cycles(addr, 16, "r")[0] == 0
            addr = [V0 + 4 * (c * V_CH + (16 + k) * 64 + i) for i in range(64)]
            assert lc.extra_cycles(addr, 4, "w")[0] == 0


def test_the_window_reads_are_conflict_free():
    """window: lane (ch << 5 | j) reads V[ch][row - 2 i][j] and V[ch][row - 2 i - 1][32 + j] (ds_read_b32): each half wave reads 32
    consecutive ints of its own channel."""
    for k in (0, 1, 35):
        for i in range(8):
            a = [V0 + 4 * ((l >> 5) * V_CH + (16 + k - 2 * i) * 64 + (l & 31)) for l in range(64)]
            b = [V0 + 4 * ((l >> 5) * V_CH + (16 + k - 2 * i - 1) * 64 + 32 + (l & 31)) for l in range(64)]
            assert lc.extra_cycles(a, 4, "r")[0] == 0 and lc.extra_cycles(b, 4, "r")[0] == 0
            assert min(16 + k - 2 * i - 1 for i in range(8)) >= 0
    # the newest 16 rows become the history: thread t moves ints t + 256 i of both channels' 1024
    for w in range(4):
        for i in range(8):
            e = [64 * w + l + 256 * i for l in range(64)]
            rd = [V0 + 4 * ((x >> 10) * V_CH + 36 * 64 + (x & 1023)) for x in e]
            wr = [V0 + 4 * ((x >> 10) * V_CH + (x & 1023)) for x in e]
            assert lc.extra_cycles(rd, 4, "r")[0] == 0 and lc.extra_cycles(wr, 4, "w")[0] == 0


def test_the_bit_fields_are_read_with_at_most_a_two_way_conflict():
    """parse: lane l reads the bytes of its field at a bit position that is a prefix sum (ds_read_u8, bank = dword mod 32 per half wave).
    Allocation, scfsi and scale factors of a half wave lie within 32 dwords: no conflict.  The sample code words of a granule can span up
    to 32 x 6 bytes per half wave: where they pass 128 bytes two lanes meet on a bank (one extra cycle), never more."""
    for bits in (2, 4, 6, 18):
        for start in (32, 48, 333):
            for byte in range(3):
                addr = [FRM + ((start + bits * l) >> 3) + byte for l in range(64)]
                assert lc.extra_cycles(addr, 1, "r")[0] == 0, (bits, start, byte)
    worst = 0
    for bits in (5, 9, 15, 21, 30, 48):
        for start in (500, 5003):
            for byte in range(3):
                for idx in range(3):
                    addr = [FRM + ((start + bits * l + idx * (bits // 3)) >> 3) + byte for l in range(64)]
                    worst = max(worst, lc.extra_cycles(addr, 1, "r")[0])
    assert worst == 2                                                  # one extra cycle per half wave at 48 bits a lane


def test_the_funnel_shift_reads_and_writes_consecutive_bytes():
    """frame assembly: thread t merges destination byte first + t of MP2frame from source bytes sb, sb + 1 of the logical frame, sb = t + a
    constant: four lanes to a dword, 16 dwords a wave."""
    for first in (0, 3, 1151):
        for shift in (-1, 0, 77):
            dst = [FRM + first + l for l in range(64)]
            src = [max(0, first + l + shift) for l in range(64)]
            assert lc.extra_cycles(dst, 1, "r")[0] == 0 and lc.extra_cycles(dst, 1, "w")[0] == 0 and lc.extra_cycles(src, 1, "r")[0] == 0
