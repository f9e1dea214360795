"""No device: the MP2 sync and PAD model and the scenarios of tests/mp2_pad_cases.py on their own -- that the committed scenarios reach
every branch of mp2processor.cpp:250-285 and :611-747 (a coverage table keyed by reference line) and, through it, PadHandler's guards at
the sizes an MP2 logical frame has; that handing PadHandler only the 254 X-PAD bytes next to the F-PAD, as k_pad_mp2 stages them, changes
nothing; that the oracle back end (oracle/msc.c) decodes the builder's coded frames back to the same bytes; that the model's
check_crc_bytes is the reference's; and that the new declarations exist.  The GPU tests compare the device with this model on exactly
these scenarios."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp2_pad_cases as mc
import oracle_lib as ol
import pad_cases as pc
from dabstar_amd import lib as dx

NEW_SYMBOLS = ("dabx_get_mp2_sync_stats",)

# every branch of the restatement by reference line ("mp2:277 no sync word" cannot be reached: :725 writes the 12 ones itself)
COVERAGE = (
    "mp2:252 rate unchanged", "mp2:257 unsupported rate 0", "mp2:257 unsupported rate 44100", "mp2:257 unsupported rate 32000",
    "mp2:257 unsupported rate 22050", "mp2:257 unsupported rate 16000", "mp2:263 rate 48000 -> 24000", "mp2:263 rate 24000 -> 48000",
    "mp2:278 not layer II, layer bits 0", "mp2:278 not layer II, layer bits 1", "mp2:278 not layer II, layer bits 3",
    "mp2:279 bit-rate index 15", "mp2:279 bit-rate index 0 passes",
    "mp2:629 F-PAD type != 0", "mp2:635 no X-PAD", "mp2:641 X-PAD indicator 3", "mp2:649 short X-PAD", "mp2:654 variable X-PAD",
    "mp2:691 frame complete, at the last bit, 48000 Hz", "mp2:691 frame complete, at the last bit, 24000 Hz",
    "mp2:691 frame complete, in mid-frame, 48000 Hz", "mp2:691 frame complete, in mid-frame, 24000 Hz",
    "mp2:718 ones at the end of the frame", "mp2:720 sync word", "mp2:720 sync word across the frame boundary",
    "mp2:732 eleven ones, then a zero", "mp2:737 header across the frame boundary",
) + tuple("mp2:283 rate index %d, ID %d" % (r, i) for r in range(4) for i in range(2))

# PadHandler's lines that an MP2 logical frame reaches differently from an access unit (the rest is test_pad_cases.py's table): guard G3
# and the check of :219 each side of their boundary at vLen 20, G4 at 256 exactly and beyond, both short forms, the long group.  A CI list
# that ends at or below index 0 cannot exist here: vLen >= 20 and the list has at most four bytes.
PAD_COVERAGE = (
    "G3 sub-field ends at index 0", "G3 sub-field below index 0", ":219 no-CI X-PAD shorter than mXPadLength", ":234 no-CI continuation of a label",
    ":240 no-CI continuation of a group", "G4 text at the bound", "G4 dropped at :163", "G4 dropped at :183", ":137 short, start of fragment",
    ":154 short, continuation", ":173 short without CI, data taken", ":193 signal_show_label", ":416 signal_show_label", ":452 signal_show_label",
    ":262 four CIs, no end marker", ":259 end marker", "group of 16383 bytes", "group of 2 bytes", ":541 group with a bad CRC",
    "label while a group is under assembly", ":298 length indicator, bad CRC",
)


def test_new_declarations_enum_values_and_the_size_of_the_sync_stats(tmp_path):
    assert set(NEW_SYMBOLS) <= set(dx.declared_symbols())
    assert dx.MP2_SYNC_STATS.itemsize == 64 and C.sizeof(dx.PadConfig) == 32 and dx.PadConfig.source.offset == 4
    assert dx.PAD_SOURCES == {"dabplus": 0, "mp2": 1} and dx.Engine.mp2_sync_stats and (dx.MP2_SEARCHING, dx.MP2_GET_RATE, dx.MP2_GET_DATA) == (0, 1, 2)
    L = dx.load()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    so = os.path.join(os.path.dirname(os.path.abspath(dx.__file__)), "hipmodule", "libdabx.so")
    if not os.path.exists(so):
        from dabstar_amd import build as b
        b.build_hipmodule()
    assert all(hasattr(C.CDLL(so), n) for n in NEW_SYMBOLS)
    src = tmp_path / "t.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(dabx_mp2_sync_stats), offsetof(dabx_mp2_sync_stats, sample_rate),
         offsetof(dabx_mp2_sync_stats, last_sync_bit), offsetof(dabx_mp2_sync_stats, active), sizeof(dabx_pad_config), offsetof(dabx_pad_config, source),
         sizeof(dabx_pad_stats), DABX_PAD_SOURCE_DABPLUS, DABX_PAD_SOURCE_MP2, DABX_ABI_VERSION);
  return 0;
}
""")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    f = dx.MP2_SYNC_STATS.fields
    assert got == [64, f["sample_rate"][1], f["last_sync_bit"][1], f["active"][1], 32, 4, 128, 0, 1, 6], got


def test_the_model_on_hand_made_frames():
    """The rules that are easy to get wrong, on frames small enough to check by eye (8 kbit/s: 24 bytes, vLen 20)."""
    rng = np.random.default_rng(8)
    nb = 24

    def frame(hdr_at=0, pad=None, **h):
        f = bytearray((rng.integers(0, 256, nb) & 0x7F).astype(np.uint8).tobytes())
        if pad is not None:
            f[20 - (len(pad) - 2):20] = pad[:-2]
            f[22:] = pad[-2:]
        if hdr_at is not None:
            mc._stamp(f, 0, hdr_at, mc.header(**dict(mc.H48, **h)))
        return bytes(f)
    lab = pc.var_ci(pc.label_fields(rng, b"hi", 1, 1))
    # aligned, 48 kHz: every frame gives its PAD; the item carries the logical frame's index and au 0
    m = mc.run_model(8, [frame(pad=lab), frame(pad=lab)])
    assert m.pad.payloads == [b"hi", b"hi"] and [r[1] for r in m.pad.rows] == [0, 1] and [r[4] for r in m.pad.rows] == [0, 0]
    assert m.sync_stats() == dict(syncs=2, frames=2, hdr_refused=0, rate_unsupported=0, last_sync_bit=11, sample_rate=48000, state=0, bit_count=0,
                                  header_count=0, active=1)
    # 24 kHz: the PAD of every second logical frame; the first one's is not looked at
    m = mc.run_model(8, [frame(pad=lab, **mc.H24), frame(None, pad=lab), frame(pad=lab, **mc.H24)])
    assert [r[1] for r in m.pad.rows] == [1] and m.sample_rate == 24000 and m.state == mc.MP2_GET_DATA and m.bit_count == 192
    # bit-rate index 15 is refused, index 0 passes; 44.1 kHz is unsupported; all three leave 48 kHz and the frame completes
    m = mc.run_model(8, [frame(bitrate=15), frame(bitrate=0), frame(rate=0)])
    assert (m.stats["hdr_refused"], m.stats["rate_unsupported"], m.stats["frames"], m.sample_rate) == (1, 1, 3, 48000)
    # the sync word 5 bits in front of the frame's end: 5 ones there, 7 and the header in the next frame; an MP2 frame completes at bit 186
    # of each of the next two frames and takes THAT frame's PAD (its L0 has the next sync word's first ones in it)
    fr = [bytearray(frame(None)), bytearray(frame(None, pad=lab)), bytearray(frame(None, pad=lab))]
    for k in range(2):
        for q in (k, k + 1):
            mc._stamp(fr[q], q * 192, k * 192 + 187, mc.header(**mc.H48))
    m = mc.run_model(8, fr)
    assert m.stats["syncs"] == 2 and m.stats["frames"] == 2 and m.stats["last_sync_bit"] == 6 and [r[1] for r in m.pad.rows] == [1, 2]
    assert m.branch["mp2:720 sync word across the frame boundary"] == 2 and m.branch["mp2:691 frame complete, in mid-frame, 48000 Hz"] == 2
    # eleven ones and a zero are no sync word; twelve are
    z = bytearray(nb)
    mc._stamp(z, 0, 3, 0xFFE000)
    m = mc.run_model(8, [z])
    assert m.stats["syncs"] == 0 and m.header_count == 0 and m.branch["mp2:732 eleven ones, then a zero"] == 1
    mc._stamp(z, 0, 3, 0xFFF000)
    assert mc.run_model(8, [z]).stats["last_sync_bit"] == 14


def _all_models(limit=None):
    return [(s, j, kbps, mc.slot_model(s, j, limit)) for s, j, kbps in mc.mp2_slots()]


def test_the_scenarios_reach_every_line_of_the_restatement_at_all_five_rates():
    branch, pbranch, counters = collections.Counter(), collections.Counter(), collections.Counter()
    per_rate = collections.defaultdict(collections.Counter)
    for s, j, kbps, m in _all_models():
        branch.update(m.branch); pbranch.update(m.pad.branch); counters.update(m.pad.counters)
        per_rate[kbps].update(m.branch)
        per_rate[kbps].update(m.pad.branch)
        facts = mc.scenario(kbps, mc.seed_of(s, j), mc.variant_of(s))[1]
        # everything scripted went into a frame whose PAD is taken; the shifted 384 kbit/s scenario has too few such frames for all of the
        # 192 kbit/s script, but its 16 383-byte group is complete
        assert facts["scripted_left"] == 0 or (kbps, mc.variant_of(s)) == (384, 1), (s, j, kbps, facts["scripted_left"])
        assert sum(facts["taken"]) == m.pad.counters["aus"] == m.pad.counters["pad_aus"] == m.stats["frames"] and m.pad.counters["superframes"] == mc.N_FRAMES
        assert m.pad.counters["labels"] > 0 and m.pad.counters["groups"] > 0 and m.pad.max_msc <= 16382 + 196
        assert max(b - a for a, b in zip([q[0] for q in m.snaps[:-1]], [q[0] for q in m.snaps[1:]])) <= 4          # pad_core.h: at most 4 items per logical frame
    print(sorted(branch.items()), dict(counters))
    assert sorted(per_rate) == mc.RATES
    missing = [k for k in COVERAGE if branch[k] == 0] + [k for k in PAD_COVERAGE if pbranch[k] == 0]
    assert not missing, missing
    extra = sorted(set(branch) - set(COVERAGE))
    assert not extra, extra                                        # no line of the model that is not in the table
    # what each rate is there for
    assert per_rate[8]["G3 sub-field ends at index 0"] and per_rate[8]["G3 sub-field below index 0"] and per_rate[8][":219 no-CI X-PAD shorter than mXPadLength"]
    assert per_rate[48][":219 no-CI X-PAD shorter than mXPadLength"] and per_rate[48][":240 no-CI continuation of a group"]
    assert per_rate[384]["group of 16383 bytes"] >= 2 and per_rate[384]["G4 text at the bound"] and per_rate[384]["G4 dropped at :163"]
    for kbps in mc.RATES:
        for k in ("mp2:720 sync word across the frame boundary", "mp2:737 header across the frame boundary", "mp2:263 rate 48000 -> 24000",
                  "mp2:691 frame complete, in mid-frame, 24000 Hz", "mp2:629 F-PAD type != 0", "mp2:649 short X-PAD"):
            assert per_rate[kbps][k], (kbps, k)
    for k in pc.PAD_COUNTERS:
        assert counters[k] > 0, k


def test_the_last_254_xpad_bytes_decide_everything():
    """The bound k_pad_mp2 relies on: the model fed the whole X-PAD field (vLen bytes, as the reference) and the model fed its last 254
    bytes give identical items, bytes, counters and branches, frame by frame, on every scenario."""
    n = 0
    for (s, j, kbps, full), (_, _, _, cut) in zip(_all_models(), _all_models(254)):
        assert full.pad.records().tobytes() == cut.pad.records().tobytes() and full.pad.payloads == cut.pad.payloads, (s, j, kbps)
        assert full.snaps == cut.snaps and full.pad.branch == cut.pad.branch and full.branch == cut.branch, (s, j, kbps)
        n += mc.v_len(kbps) > 254
    assert n >= 4                                                  # 128 and 384 kbit/s: the field is longer than what is staged


def test_the_builders_sync_walk_is_the_models():
    """SyncWalk (the builder's way to know which frames have their PAD taken) against the bit-serial model, state by state."""
    for s, j, kbps in mc.mp2_slots():
        frames = mc.scenario(kbps, mc.seed_of(s, j), mc.variant_of(s))[0]
        m, w = mc.slot_model(s, j), mc.SyncWalk(kbps)
        for k, f in enumerate(frames):
            done = w.step(f)
            st = m.snaps[k + 1][3]
            assert (w.state, w.hc, w.bc, w.rate, int(done)) == (st["state"], st["header_count"], st["bit_count"], st["sample_rate"],
                                                                st["frames"] - m.snaps[k][3]["frames"]), (s, j, kbps, k)


def test_the_oracle_decodes_the_coded_frames_back_to_the_builders_bytes():
    for s in range(len(mc.STAGE_STREAMS)):
        layout, frames, _, want = mc.stream_case(s)
        for j, (kbps, kind) in enumerate(mc.kinds(s)):
            assert np.array_equal(want[j]["frames"], frames[j]), (s, j, kbps, kind)
            assert layout[j].dab_plus == int(kind == "pad")
    sched = mc.boundary_schedule(len(mc.STAGE_STREAMS))
    assert {c for row in sched for c in row} >= {0, 1, 4, 5, 6, 13, 27, 28}
    assert {kbps for _, _, kbps in mc.mp2_slots()} == set(mc.RATES)


def test_check_crc_bytes_of_the_model_is_the_references_on_every_length_indicator_and_group():
    if not ol.have_ref():
        pytest.skip("oracle/_ref is not built")
    R = ol.ref()
    n = bad = 0
    for s, j, kbps, m in _all_models():
        for msg, ln in m.pad.crc_calls:
            want = bool(R.ref_check_crc_bytes(np.frombuffer(msg, np.uint8).copy(), ln))
            assert pc.check_crc_bytes(msg, ln) == want, (s, j, n, ln)
            n += 1
            bad += not want
    assert n > 200 and 0 < bad < n
