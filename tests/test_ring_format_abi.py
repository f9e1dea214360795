"""CPU-only: the native IQ ring (dabx_create_ex, DABX_RING_S16 / DABX_RING_U8) at the interface and in the compiler's output.

The ABI half: the two new entry points are declared and exported by both library forms, the ABI version and dabx_config
are what they were, dabx_create_ext has its documented size in C and in the binding.  The device half: each of the five
kernels that read the ring exists once per ring element, and no instantiation costs scratch or a wave of occupancy that
the kernel did not cost before it became a template (figures of the commit before the feature, same compiler flags)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from dabstar_amd import build as B
from dabstar_amd import lib as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dabx_create_ex", "dabx_get_ring_format")


def test_new_entry_points_are_declared_and_exported_and_the_abi_version_stays():
    L = dx.load()
    names = dx.declared_symbols()
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    assert L.dabx_abi_version() == 6


def test_hipmodule_form_exports_them_too():
    mod = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "hipmodule")
    so = os.path.join(mod, "libdabx.so")
    if not os.path.exists(so):
        if not shutil.which(B.HIPCC):
            pytest.skip("no hipcc and no prebuilt hipmodule/libdabx.so")
        B.build_hipmodule()
    L = C.CDLL(so)
    for n in NEW:
        assert hasattr(L, n), n
    assert L.dabx_abi_version() == 6
    # the ring formats brought no translation unit of their own: one code object per .hip file of csrc/
    assert len([f for f in os.listdir(mod) if f.startswith("dabx_gfx950_") and f.endswith(".hsaco")]) == 8


def test_config_keeps_its_size_and_the_extension_record_has_its_own(tmp_path):
    src = tmp_path / "t.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void) {
  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(dabx_config), sizeof(dabx_create_ext), offsetof(dabx_create_ext, ring_format),
         offsetof(dabx_create_ext, reserved), DABX_RING_CF32, DABX_RING_S16, DABX_RING_U8);
  return 0;
}
""")
    exe = tmp_path / "t"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64, 32, 4, 8, 0, 1, 2], got
    assert C.sizeof(dx.Config) == 64 and C.sizeof(dx.CreateExt) == 32
    assert dx.CreateExt.ring_format.offset == 4 and dx.CreateExt.reserved.offset == 8
    assert (dx.RING_CF32, dx.RING_S16, dx.RING_U8) == (0, 1, 2) and dx.RING_FORMATS == {"cf32": 0, "s16": 1, "u8": 2}


# VGPRs / scratch bytes per lane / waves per SIMD of the ring-reading kernels on the commit before they became templates
PARENT = {"k_acquire": (256, 204, 2), "k_frame_head": (126, 0, 4), "k_symbols_persistent": (166, 0, 3), "k_frame_tail": (68, 0, 7),
          "k_level_exact": (234, 0, 2)}


@pytest.fixture(scope="module")
def resources():
    """{(kernel, ring format): (VGPRs, scratch, occupancy)} from the compiler's kernel-resource-usage remarks for pipeline.hip."""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    flags = [f for f in B.FLAGS if not f.startswith("-W")] + ["-w"]
    p = subprocess.run([B.HIPCC] + flags + ["-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                            os.path.join(B.CSRC, "pipeline.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    out, cur = {}, None
    for ln in p.stderr.split("\n"):
        g = re.search(r"remark: +Function Name: (\S+)", ln)
        if g:
            m = re.match(r"_ZN4dabx\d+(k_[a-z_]+)ILi(\d)EEEvNS_9EngineDev", g.group(1))
            cur = (m.group(1), int(m.group(2))) if m else None
            if cur:
                out[cur] = {}
            continue
        if cur:
            for key, pat in (("vgpr", r"remark: +VGPRs: (\d+)"), ("scratch", r"remark: +ScratchSize \[bytes/lane\]: (\d+)"),
                             ("occ", r"remark: +Occupancy \[waves/SIMD\]: (\d+)")):
                g = re.search(pat, ln)
                if g:
                    out[cur][key] = int(g.group(1))
    return {k: (v["vgpr"], v["scratch"], v["occ"]) for k, v in out.items()}


@pytest.mark.parametrize("kernel", sorted(PARENT))
def test_ring_kernels_exist_per_ring_format_and_cost_no_scratch_or_occupancy(resources, kernel):
    vg0, sc0, oc0 = PARENT[kernel]
    for rf in (0, 1, 2):
        assert (kernel, rf) in resources, (kernel, rf, sorted(resources))
        vg, sc, oc = resources[(kernel, rf)]
        print("%s<%d>: %d VGPRs, %d bytes of scratch per lane, %d waves per SIMD (before: %d / %d / %d)" % (kernel, rf, vg, sc, oc, vg0, sc0, oc0))
        assert sc <= sc0 and oc >= oc0, (kernel, rf, vg, sc, oc)
        if rf == 0:
            assert vg <= vg0, (kernel, vg, vg0)             # the cf32 instantiation is the kernel as it was
