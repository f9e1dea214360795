"""CPU: the model of the MP2 audio stage (tests/mp2_audio_cases.py) and what it stands on.  The scenarios reach every line the stage
restates; the tables are what the formula and -- where its tree is present -- the reference's initialisers say, and csrc/mp2_core.h holds
the same numbers; single-line mutations of the model change the PCM, so a device that made them would be noticed; and the kernel's own
pieces (mp2_core.h, run lane after lane on the host through dabx_internal_mp2_decode_host) give the model's PCM on every frame of every
scenario, bit for bit."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mp2_audio_cases as ac
from dabstar_amd import lib as dx

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = "/root/reference/src/base/backend/audio/mp2processor.cpp"


def _models():
    return {(s, j): ac.slot_model(s, j) for s, j, _ in ac.audio_slots()}


def test_the_scenarios_reach_every_line_of_the_restatement():
    total = sum((m.branch for m in _models().values()), ac.collections.Counter())
    want = ["mp2:263 rate 48000 -> 24000", "mp2:263 rate 24000 -> 48000", "mp2:257 unsupported rate 44100", "mp2:257 unsupported rate 32000",
            "mp2:257 unsupported rate 22050", "mp2:257 unsupported rate 0", "mp2:311 scale factor 63", "mp2:325 grouped code word beyond nlevels^3",
            "mp2:389 the window of 25 frames closes", "mp2:397 bad header: layer bits 3, bit-rate index 10", "mp2:397 bad header: layer bits 1, bit-rate index 10",
            "mp2:397 bad header: layer bits 0, bit-rate index 10", "mp2:397 bad header: layer bits 2, bit-rate index 15", "mp2:412 free format (bit-rate index 0)",
            "mp2:418 reserved sampling frequency", "mp2:436 joint stereo, bound 4", "mp2:436 joint stereo, bound 8", "mp2:436 joint stereo, bound 12",
            "mp2:436 joint stereo, bound 16", "mp2:441 mode 0", "mp2:441 mode 2", "mp2:441 mode 3", "mp2:448 CRC present", "mp2:448 no CRC",
            "mp2:462 LSR table", "mp2:473 table A", "mp2:473 table C", "mp2:473 table B from a 44100 Hz header", "mp2:473 table D from a 32000 Hz header",
            "mp2:473 table B from a 32000 Hz header", "mp2:478 joint-stereo bound above sblimit", "mp2:508 scfsi 0", "mp2:508 scfsi 1", "mp2:508 scfsi 2",
            "mp2:508 scfsi 3", "mp2:587 U[i] * D[i] wraps", "mp2:596 clamp", "mp2:691 frame complete inside a byte, 48000 Hz",
            "mp2:691 frame complete inside a byte, 24000 Hz", "mp2:691 frame complete at a byte boundary, 48000 Hz", "G1 the refill ran past MP2frame"]
    missing = [k for k in want if not total[k]]
    assert not missing, (missing, sorted(total))


def test_what_the_scenarios_do_to_every_slot():
    """Per slot: every template was placed whole several times, frames of all three outcomes; over-reading happens at 8 and 56 kbit/s and
    never at 96 and above (48 kbps >= 4608 > the longest parse + 2), although the same headers are there; the wrap needs codes beyond the
    quantiser's range: the in-range full-scale frame stays below 2^31, the one beyond it does not."""
    for (s, j), m in _models().items():
        kbps, kind = ac.kinds(s)[j]
        names = ac.scenario(kbps, ac.seed_of(s, j), ac.OFFSETS[s] + j)[1]["names"]
        st = m.all_stats()
        assert set(names) == {n for n, _ in ac.TEMPLATES}, (s, j)
        assert st["decode_calls"] == len(names) and st["frames_out"] + st["bad_header"] + st["refused"] == st["decode_calls"], (s, j, st)
        assert st["bad_header"] > 0 and st["refused"] > 0 and st["frames_out"] > 50, (s, j, st)
        assert (st["overread"] > 0) == (kbps < 96), (s, j, kbps, st)
        assert names.count("over-reading header") >= 3
        assert len({r[1] for r in m.rows}) == 2                       # records at both sticky rates
        if kbps >= 96:
            assert m.wraps > 0 and m.max_product > 1 << 31, (s, j, m.max_product)
    # the in-range full-scale frame alone, from silence: 65 534 in each of table A's 27 subbands makes V[48] = (27 * 256 * 65 534 + 8192) >> 14
    # = 27 647, times D[240] = -64 018; table B's 30 subbands would make 30 719: still below 2^31
    assert (30 * 256 * 65534 + 8192) >> 14 == 30719 and 30719 * 64018 + 32 < 1 << 31 and ac.D[240] == -64018
    rng = np.random.default_rng(1)
    data, _, _ = ac.frame_of(384, rng, 48000, *[t for t in ac.TEMPLATES if t[0] == "in-range full scale DC"][0])
    m = ac.Mp2AudioModel(384)
    m.mp2frame[:len(data)] = data.tobytes()
    assert m.decode_frame(np.zeros(2304, np.int16)) > 0
    assert m.wraps == 0 and m.max_product == 27647 * 64018 + 32, m.max_product


def test_n_is_the_formula_in_python_and_in_c(tmp_path):
    N = ac.N
    assert N == [[int(256.0 * math.cos(((16 + i) * ((j << 1) + 1)) * 0.0490873852123405)) for j in range(32)] for i in range(64)]
    src = tmp_path / "n.c"
    src.write_text("#include <stdio.h>\n#include <math.h>\nint main(void) { for (int i = 0; i < 64; i++) for (int j = 0; j < 32; ++j) "
                   "printf(\"%d\\n\", (int)(short)(256.0 * cos(((16 + i) * ((j << 1) + 1)) * 0.0490873852123405))); return 0; }\n")
    exe = tmp_path / "n"
    subprocess.check_call(["gcc", "-O0", "-o", str(exe), str(src), "-lm"])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [v for row in N for v in row]
    # the products of rows 16 and 48 are the 64 that lie next to an integer: they come out 0 and -256; every other is >= 0.019 from one
    far = 1.0
    for i in range(64):
        for j in range(32):
            x = 256.0 * math.cos(((16 + i) * ((j << 1) + 1)) * 0.0490873852123405)
            if i in (16, 48):
                assert abs(x - round(x)) < 1e-9 and N[i][j] == (0 if i == 16 else -256), (i, j, x)
            else:
                far = min(far, abs(x - round(x)))
    assert far >= 0.019, far
    # the symmetries: 32 rows would do
    for i in range(33):
        assert N[i] == [-v for v in N[32 - i]], i
    for i in range(33, 64):
        assert N[i] == N[96 - i], i


def test_the_longest_parse_per_table():
    assert (ac.longest_parse_bits(1) + 7) // 8 == 4500 and (ac.longest_parse_bits(2) + 7) // 8 == 1690
    assert ac.longest_parse_bits(0) < ac.longest_parse_bits(2)
    # ... and the window's refill reads at most two bytes more (mp2:363-367): 4502 < 4608 = 48 * 96
    assert (ac.longest_parse_bits(1) + 23) // 8 == 4502 < 48 * 96 and (ac.longest_parse_bits(1) + 23) // 8 > 48 * 88
    # the builder agrees: a frame with every field at its widest asks for exactly as many bits
    rng = np.random.default_rng(0)
    _, asked = ac.build_frame(6000, rng, bitrate=13, rate=0, prot=0, alloc=ac.max_alloc, scfsi=lambda sb, ch: 0)
    assert asked == ac.longest_parse_bits(1)
    _, asked = ac.build_frame(6000, rng, mpeg1=0, bitrate=8, prot=0, alloc=lambda sb, ch: 15 if sb < 4 else 7 if sb < 11 else 3, scfsi=lambda sb, ch: 0)
    assert asked == ac.longest_parse_bits(2)


def _c_arrays(text):
    """name -> flat list of the integers of every `constexpr T name[..] = {...};` of a C source, as data"""
    out = {}
    for name, body in re.findall(r"(\w+)\s*(?:\[[^\]]*\])+\s*=\s*\{(.*?)\};", text, re.S):
        body = re.sub(r"//[^\n]*", "", body)
        out[name] = [int(x, 0) for x in re.findall(r"-?0x[0-9A-Fa-f]+|-?\d+", body)]
    return out


def _padded(rows, width):
    return [v for r in rows for v in list(r) + [0] * (width - len(r))]


def test_the_tables_of_the_kernel_are_the_models():
    t = _c_arrays(re.sub(r"\b27 \| 64\b", "91", re.sub(r"\b30 \| 64\b", "94", open(os.path.join(ROOT, "dabstar_amd", "csrc", "mp2_core.h")).read())))
    assert t["MP2_D"] == ac.D and t["MP2_N"] == [v for row in ac.N for v in row]
    assert t["MP2_SAMPLE_RATES"] == list(ac.SAMPLE_RATES) and t["MP2_BITRATES"] == list(ac.BITRATES) and t["MP2_SCF_BASE"] == list(ac.SCF_BASE)
    assert t["MP2_STEP1"] == [v for r in ac.QUANT_LUT_STEP1 for v in r]
    assert t["MP2_STEP2"] == [v for r in ac.QUANT_LUT_STEP2 for v in r]
    assert _padded([[v for v in r] for r in (t["MP2_STEP3"][:12], t["MP2_STEP3"][12:42], t["MP2_STEP3"][42:])], 32) == [v for r in ac.QUANT_LUT_STEP3 for v in r]
    assert t["MP2_QUANT"] == [v for r in ac.QUANTIZER_TABLE for v in r]
    rows, at = [], 0
    for n in (4, 8, 16, 16, 16, 16):
        rows.append(t["MP2_STEP4"][at:at + n]); at += n
    assert _padded(rows, 16) == [v for r in ac.QUANT_LUT_STEP4 for v in r]


def test_the_tables_are_the_reference_initialisers():
    """D, the quantiser tables, scf_base, the bit rates and the sample rates parsed out of the reference's source as data."""
    if not os.path.exists(REFERENCE):
        pytest.skip("the reference tree is not on this machine")
    text = open(REFERENCE).read()
    text = text.replace("QUANT_TAB_A", "91").replace("QUANT_TAB_B", "94").replace("QUANT_TAB_C", "8").replace("QUANT_TAB_D", "12")
    t = _c_arrays(text)
    assert t["D"] == ac.D and t["scf_base"] == list(ac.SCF_BASE) and t["bitrates"] == list(ac.BITRATES) and t["sample_rates"] == list(ac.SAMPLE_RATES)
    assert t["quant_lut_step1"] == [v for r in ac.QUANT_LUT_STEP1 for v in r] and t["quant_lut_step2"] == [v for r in ac.QUANT_LUT_STEP2 for v in r]
    assert t["quantizer_table"] == [v for r in ac.QUANTIZER_TABLE for v in r]
    strip = lambda rows: [v for r in rows for v in list(r)[:max(k + 1 for k, x in enumerate(r) if x)]]      # noqa: E731  (the C rows are shorter than their arrays)
    assert t["quant_lut_step3"] == strip(ac.QUANT_LUT_STEP3)
    assert t["quant_lut_step4"] == [v for r, n in zip(ac.QUANT_LUT_STEP4, (4, 8, 16, 16, 16, 16)) for v in r[:n]]


def test_every_mutation_of_a_single_line_changes_the_pcm():
    kbps = 96
    frames = ac.scenario(kbps, 1, 13, 2 * ac.BATCH)[0]
    good = ac.run_model(kbps, frames)
    assert good.wraps > 0 and good.branch["mp2:596 clamp"] > 0
    for mut in ("round574", "round587", "sign594", "clamp", "and1023"):
        bad = ac.run_model(kbps, frames, mut=(mut,))
        assert bad.records().tobytes() == good.records().tobytes(), mut
        assert not np.array_equal(bad.all_pcm(), good.all_pcm()), mut


def test_the_kernels_pieces_on_the_host_give_the_models_pcm_on_every_frame():
    """dabx_internal_mp2_decode_host runs mp2_core.h's functions -- the header, the field widths and positions, the requantisation, the
    matrixing and the window of k_mp2_audio -- lane after lane on the host.  Every completed MP2 frame of every scenario, with the MP2frame
    and the V history the model has at that point: frame size, refusal, guard G1 and all 2304 samples equal the model's."""
    L = dx.load()
    L.dabx_internal_mp2_decode_host.argtypes = [C.c_void_p] + [C.c_int] + [C.c_void_p] * 4
    n_frames = n_out = 0
    for s, j, kbps in ac.audio_slots():
        if (s, j) not in ((0, 0), (0, 4), (1, 1), (2, 1), (3, 0), (3, 2)):      # every rate once
            continue
        frames = ac.slot_frames(s, j, kbps, ac.kinds(s)[j][1])
        hist = np.zeros((2, 16, 64), np.int32)
        seen = []

        class Tapped(ac.Mp2AudioModel):
            def decode_frame(self, pcm):
                frame = np.frombuffer(bytes(self.mp2frame[:6 * kbps]), np.uint8).copy()
                got = np.zeros(2304, np.int16)
                status, over = C.c_int32(0), C.c_int32(0)
                size = L.dabx_internal_mp2_decode_host(frame.ctypes.data, kbps, hist.ctypes.data, got.ctypes.data, C.byref(status), C.byref(over))
                before = dict(self.stats)
                want = super().decode_frame(pcm)
                kind = 1 if self.stats["bad_header"] > before["bad_header"] else 2 if self.stats["refused"] > before["refused"] else 0
                seen.append((size == want, status.value == kind, want == 0 or over.value == int(self.over), want == 0 or np.array_equal(got, pcm)))
                return want
        m = Tapped(kbps)
        for f in frames:
            m.add_to_frame(f)
        assert len(seen) == m.stats["decode_calls"] and all(all(x) for x in seen), (s, j, kbps, [k for k, x in enumerate(seen) if not all(x)][:5])
        # the history the host pieces keep is the model's V, oldest sub-block first
        for ch in range(2):
            rows = [m.V[ch, ((m.voffs + 64 * (15 - r)) & 1023):((m.voffs + 64 * (15 - r)) & 1023) + 64] for r in range(16)]
            assert np.array_equal(hist[ch], np.array(rows)), (s, j, ch)
        n_frames += len(seen)
        n_out += m.stats["frames_out"]
    assert n_frames > 600 and n_out > 400
