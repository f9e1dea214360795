"""The declarations of the AAC stream stage (include/dabx.h: dabx_set_aac_stream_mode, dabx_aac_frame, dabx_aac_stream_stats,
DABX_DELIVER_AAC, dabx_chunk_header_ext.off_aac, dabx_chunk_aac) as a C compiler sees them, against the Python mirror
(dabstar_amd/lib.py) and both forms of the built library.  No device."""
import ctypes
import os
import subprocess

import pytest

from dabstar_amd import lib as dx

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STRUCTS = {
    "dabx_aac_frame": (dx.AAC_FRAME, 32),
    "dabx_aac_stream_stats": (dx.AAC_STREAM_STATS, 64),
    "dabx_chunk_aac": (dx.CHUNK_AAC, 128),
    "dabx_chunk_header_ext": (dx.CHUNK_HEADER_EXT, 64),
}
NEW_SYMBOLS = ("dabx_set_aac_stream_mode", "dabx_read_aac_frames", "dabx_get_aac_stream_stats")


def test_sizes_offsets_and_constants(tmp_path):
    fields = [(s, k) for s, (dt, _) in STRUCTS.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void)
{
  printf("%%zu %%zu %%zu %%zu %%zu %%zu ", sizeof(dabx_aac_frame), sizeof(dabx_aac_stream_stats), sizeof(dabx_chunk_aac), sizeof(dabx_chunk_header_ext),
         sizeof(dabx_aac_stream_config), sizeof(dabx_chunk_header));
  printf("%%d %%d %%d %%d %%d %%d %%d ", DABX_DELIVER_AAC, DABX_AAC_MAX_FRAME_BYTES, DABX_MAX_KERNELS, DABX_ABI_VERSION, DABX_CHUNK_FRAMES, DABX_AAC_LOST_LEN,
         DABX_AAC_LOST_CRC);
%s
  printf("\\n");
  return 0;
}
""" % "\n".join('  printf("%%zu ", offsetof(%s, %s));' % f for f in fields))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:6] == [32, 64, 128, 64, 32, 128]                     # the header's extension stays 64 bytes, the header 128
    assert got[6:13] == [2048, 974, 16, 6, 7, 1, 2]                   # DABX_MAX_KERNELS stays 16, the ABI version does not move
    assert [dt.itemsize for dt, _ in STRUCTS.values()] == [n for _, n in STRUCTS.values()]
    assert got[13:] == [STRUCTS[s][0].fields[k][1] for s, k in fields]
    ext = dx.CHUNK_HEADER_EXT.fields
    assert (ext["off_tii"][1], ext["off_mp2_audio"][1], ext["off_aac"][1]) == (8, 16, 24)        # out of the reserved room
    assert dx.AAC_FRAME.names[0] == "byte_pos"                        # what the output ring's records share (out_ring.h)
    f = dx.AAC_FRAME.fields
    assert [f[k][1] for k in ("byte_pos", "first_frame", "length", "au_len", "au", "num_aus", "stream_parms", "flags", "reserved")] == [0, 8, 16, 18, 20, 21, 22, 23, 24]
    assert dx.AAC_STREAM_STATS.names == ("superframes", "records", "frames", "frame_bytes", "lost_len", "lost_crc", "launches", "lost")
    assert ctypes.sizeof(dx.AacStreamConfig) == 32
    assert dx.DELIVER_AAC == 2048 and dx.AAC_MAX_FRAME_BYTES == 974 == 11 + 960 // 255 + 960 and (dx.AAC_LOST_LEN, dx.AAC_LOST_CRC) == (1, 2)
    # the bit is beside the others, not one of them, and it is not the 1024 that stays refused
    assert dx.DELIVER_AAC & (1024 | dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF | dx.DELIVER_MSC_NOT_DABPLUS | dx.DELIVER_DG | dx.DELIVER_PAD |
                             dx.DELIVER_MOT | dx.DELIVER_ETI | dx.DELIVER_TII | dx.DELIVER_MP2_AUDIO) == 0


def test_the_library_exports_the_new_entries_and_declares_them():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert hasattr(L, "dabx_internal_aac_frame_host") and "dabx_internal_aac_frame_host" not in declared
    assert L.dabx_abi_version() == 6


def test_the_hipmodule_form_exports_the_same_entries_and_has_the_kernel():
    """hipmodule/libdabx.so (the same sources, kernels in code objects next to it): the same C ABI, and k_aac_stream in the code object of
    msc_stages.hip.  Skipped where the form was not built (its build is optional: __graft_entry__.build says why)."""
    lib = os.path.join(ROOT, "dabstar_amd", "hipmodule", "libdabx.so")
    co = os.path.join(ROOT, "dabstar_amd", "hipmodule", "dabx_gfx950_msc_stages.hsaco")
    if not os.path.exists(lib) or not os.path.exists(co):
        pytest.skip("the hipModule form is not built")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS + ("dabx_internal_aac_frame_host",):
        assert " T %s\n" % name in exported, name
    blob = open(co, "rb").read()
    assert b"k_aac_stream" in blob and b"k_deliver_aac" in open(os.path.join(ROOT, "dabstar_amd", "hipmodule", "dabx_gfx950_deliver.hsaco"), "rb").read()
