"""The declarations of the MP2 audio stage (include/dabx.h: dabx_set_mp2_audio_mode, dabx_mp2_audio_frame, dabx_mp2_audio_stats,
DABX_DELIVER_MP2_AUDIO, dabx_chunk_header_ext.off_mp2_audio, dabx_chunk_mp2_audio) as a C compiler sees them, against the Python mirror
(dabstar_amd/lib.py) and both forms of the built library.  No device."""
import ctypes
import os
import subprocess

import pytest

from dabstar_amd import lib as dx

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STRUCTS = {
    "dabx_mp2_audio_frame": (dx.MP2_AUDIO_FRAME, 32),
    "dabx_mp2_audio_stats": (dx.MP2_AUDIO_STATS, 64),
    "dabx_chunk_mp2_audio": (dx.CHUNK_MP2_AUDIO, 128),
    "dabx_chunk_header_ext": (dx.CHUNK_HEADER_EXT, 64),
}
NEW_SYMBOLS = ("dabx_set_mp2_audio_mode", "dabx_read_mp2_audio", "dabx_get_mp2_audio_stats")


def test_sizes_offsets_and_constants(tmp_path):
    fields = [(s, k) for s, (dt, _) in STRUCTS.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void)
{
  printf("%%zu %%zu %%zu %%zu %%zu %%zu ", sizeof(dabx_mp2_audio_frame), sizeof(dabx_mp2_audio_stats), sizeof(dabx_chunk_mp2_audio), sizeof(dabx_chunk_header_ext),
         sizeof(dabx_mp2_audio_config), sizeof(dabx_chunk_header));
  printf("%%d %%d %%d %%d %%d ", DABX_DELIVER_MP2_AUDIO, DABX_MP2_PCM_BYTES, DABX_MAX_KERNELS, DABX_ABI_VERSION, DABX_CHUNK_FRAMES);
%s
  printf("\\n");
  return 0;
}
""" % "\n".join('  printf("%%zu ", offsetof(%s, %s));' % f for f in fields))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:6] == [32, 64, 128, 64, 32, 128]                     # the header's extension stays 64 bytes, the header 128
    assert got[6:11] == [512, 4608, 16, 6, 7]                         # DABX_MAX_KERNELS stays 16, the ABI version does not move (as for ETI and TII)
    assert [dt.itemsize for dt, _ in STRUCTS.values()] == [n for _, n in STRUCTS.values()]
    assert got[11:] == [STRUCTS[s][0].fields[k][1] for s, k in fields]
    assert dx.CHUNK_HEADER_EXT.fields["off_tii"][1] == 8 and dx.CHUNK_HEADER_EXT.fields["off_mp2_audio"][1] == 16       # out of the reserved room
    assert dx.MP2_AUDIO_FRAME.names[0] == "byte_pos"                  # what the output ring's records share (out_ring.h)
    assert ctypes.sizeof(dx.Mp2AudioConfig) == 32
    assert dx.DELIVER_MP2_AUDIO == 512 and dx.MP2_PCM_BYTES == 4608 == 1152 * 2 * 2
    # the bit is beside the others, not one of them: what == 0 ("everything") is made of these
    assert dx.DELIVER_MP2_AUDIO & (dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF | dx.DELIVER_MSC_NOT_DABPLUS | dx.DELIVER_DG | dx.DELIVER_PAD |
                                   dx.DELIVER_MOT | dx.DELIVER_ETI | dx.DELIVER_TII) == 0


def test_the_library_exports_the_new_entries_and_declares_them():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert hasattr(L, "dabx_internal_mp2_decode_host") and "dabx_internal_mp2_decode_host" not in declared
    assert L.dabx_abi_version() == 6


def test_the_hipmodule_form_exports_the_same_entries_and_has_the_kernel():
    """hipmodule/libdabx.so (the same sources, kernels in code objects next to it): the same C ABI, and k_mp2_audio in the code object of
    msc_stages.hip.  Skipped where the form was not built (its build is optional: __graft_entry__.build says why)."""
    lib = os.path.join(ROOT, "dabstar_amd", "hipmodule", "libdabx.so")
    co = os.path.join(ROOT, "dabstar_amd", "hipmodule", "dabx_gfx950_msc_stages.hsaco")
    if not os.path.exists(lib) or not os.path.exists(co):
        pytest.skip("the hipModule form is not built")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert " T %s\n" % name in exported, name
    blob = open(co, "rb").read()
    assert b"k_mp2_audio" in blob and b"k_deliver_mp2_audio" in open(os.path.join(ROOT, "dabstar_amd", "hipmodule", "dabx_gfx950_deliver.hsaco"), "rb").read()
