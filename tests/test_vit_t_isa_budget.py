"""CPU: the instruction budget of the lane-per-trellis Viterbi decoder (vit_t.hip, vit_t_gen.h from tools/gen_vit_t.py).

k_msc_vitT is VALU-issue bound, so its cost is the number of VALU instructions per trellis step.  This cross-compiles
vit_t.hip for gfx950 with the library's own flags, finds the forward main loop (two 6-step cycles, the loop with the most
v_pk_min_i16) and the chain-back loop of every decoder kernel, and checks both against the formulation's count, so that a
change of the generator or of the compiler that costs instructions or a wave of occupancy shows up here and not only in a
profile.  Counts are static (instructions in the loop body)."""
import os
import re
import subprocess
import tempfile
from collections import Counter

import pytest

from dabstar_amd import build as B

SRC = os.path.join(B.CSRC, "vit_t.hip")
KERNELS = {"k_msc_vitT": 0, "k_msc_vitT_avx2": 1, "k_msc_vitT_sse2": 2}

# forward main loop, VALU per trellis step.  Tie mode 0: 12 steps, one step body.  Tie modes 1 / 2: the loop holds both the plain
# and the saturating cycle bodies and the renormalisation, so this is the loop's whole static count / 12 (a drift guard only).
FWD_BUDGET = {0: 179.0, 1: 475.0, 2: 475.0}
# chain-back loop, VALU per decoded bit (3 on the chain, the rest: addresses of the prefetched words, the per-word store)
BACK_BUDGET = 7.5


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "vit_t.s")
        flags = [f for f in B.FLAGS if not f.startswith("-W")] + ["-w"]
        subprocess.run([B.HIPCC] + flags + ["-x", "hip", "--cuda-device-only", "-S", SRC, "-o", out], check=True, capture_output=True)
        return open(out).read().split("\n")


def _mangled(name):
    return "_ZN4dabx%d%sENS_9EngineDev" % (len(name), name)


def _function(lines, name):
    m = _mangled(name)
    i0 = next(i for i, ln in enumerate(lines) if ln.startswith(m) and re.match(r"^\S+:", ln))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[i0:i1]


def _vgprs(lines, name):
    m = _mangled(name)
    for i, ln in enumerate(lines):
        if re.match(r"^\s+\.name:\s+" + re.escape(m), ln):
            j = i + 1                                       # the kernel's metadata map continues until the next "- .args" entry
            while j < len(lines) and not re.match(r"^\s+- \.", lines[j]) and not lines[j].startswith("..."):
                g = re.match(r"^\s+\.vgpr_count:\s+(\d+)", lines[j])
                if g:
                    return int(g.group(1))
                j += 1
    raise AssertionError("no .vgpr_count for " + name)


def _loops(body):
    """(first line, last line, Counter of mnemonics) of every loop closed by a backward branch."""
    labels = {}
    for i, ln in enumerate(body):
        g = re.match(r"^(\.LBB\d+_\d+):", ln)
        if g:
            labels[g.group(1)] = i
    out = []
    for i, ln in enumerate(body):
        g = re.match(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", ln)
        if g and labels[g.group(2)] < i:
            a = labels[g.group(2)]
            ins = [x.split()[0] for x in body[a:i + 1] if x.strip() and not x.strip().startswith((";", ".")) and not x.strip().endswith(":")]
            out.append((a, i, Counter(ins)))
    return out


def _valu(c):
    return sum(n for k, n in c.items() if k.startswith("v_") and not k.startswith(("v_readfirstlane", "v_readlane", "v_writelane")))


def _counts(lines, name):
    loops = _loops(_function(lines, name))
    fwd = max(loops, key=lambda lp: lp[2]["v_pk_min_i16"])
    # chain-back: the innermost loop that loads decision words (global_load_dwordx2) and picks bits (v_alignbit_b32)
    back = [lp for lp in loops if lp[2]["v_alignbit_b32"] and lp[2]["global_load_dwordx2"]]
    back = min(back, key=lambda lp: lp[1] - lp[0])
    return fwd[2], back[2]


@pytest.mark.parametrize("name", list(KERNELS))
def test_forward_loop_valu_per_step(asm, name):
    fwd, _ = _counts(asm, name)
    tie = KERNELS[name]
    if tie == 0:
        assert fwd["global_store_dwordx2"] == 12, fwd["global_store_dwordx2"]            # one decision store per trellis step
    per_step = _valu(fwd) / 12
    print("%s: forward loop %d VALU, %.1f per step" % (name, _valu(fwd), per_step))
    assert per_step <= FWD_BUDGET[tie], (name, per_step)


@pytest.mark.parametrize("name", list(KERNELS))
def test_chain_back_valu_per_bit(asm, name):
    _, back = _counts(asm, name)
    bits = back["v_alignbit_b32"]                                                        # one per decoded bit
    assert bits % 6 == 0, bits
    per_bit = _valu(back) / bits
    print("%s: chain-back loop %d VALU over %d bits, %.2f per bit" % (name, _valu(back), bits, per_bit))
    assert per_bit <= BACK_BUDGET, (name, per_bit)


def test_tie0_keeps_four_waves_per_simd(asm):
    # 512 VGPRs per SIMD lane, allocated in granules of 8: 4 waves need <= 128
    v = _vgprs(asm, "k_msc_vitT")
    print("k_msc_vitT: %d VGPRs" % v)
    assert v <= 128, v
