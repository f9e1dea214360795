"""The declarations of the TII detector on the device (include/dabx.h: dabx_set_tii_mode, dabx_tii_event, dabx_tii_stats, DABX_DELIVER_TII,
dabx_chunk_header_ext, dabx_chunk_tii, dabx_tii_process_device) as a C compiler sees them, against the Python mirror (dabstar_amd/lib.py) and
the built library.  No device."""
import os
import subprocess

from dabstar_amd import lib as dx

STRUCTS = {
    "dabx_tii_event": (dx.TII_EVENT, 32),
    "dabx_chunk_tii": (dx.CHUNK_TII, 32),
    "dabx_chunk_header_ext": (dx.CHUNK_HEADER_EXT, 64),
    "dabx_tii_stats": (dx.TII_STATS, 64),
    "dabx_tii_result": (dx.TII_RESULT, 16),
}
NEW_SYMBOLS = ("dabx_set_tii_mode", "dabx_read_tii_events", "dabx_get_tii_stats", "dabx_tii_process_device")


def test_sizes_offsets_and_constants(tmp_path):
    fields = [(s, k) for s, (dt, _) in STRUCTS.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void)
{
  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu ", sizeof(dabx_tii_event), sizeof(dabx_chunk_tii), sizeof(dabx_chunk_header_ext), sizeof(dabx_tii_stats),
         sizeof(dabx_tii_result), sizeof(dabx_tii_config), sizeof(dabx_chunk_header));
  printf("%%d %%d %%d %%d %%d %%u ", DABX_DELIVER_TII, DABX_TII_MAX_RESULTS, DABX_MAX_KERNELS, DABX_ABI_VERSION, DABX_TII_EVENT_SLOT_BYTES, DABX_CHUNK_EXT_MAGIC);
%s
  printf("\\n");
  return 0;
}
""" % "\n".join('  printf("%%zu ", offsetof(%s, %s));' % f for f in fields))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:7] == [32, 32, 64, 64, 16, 32, 128]
    assert got[7:13] == [256, 32, 16, 6, 32 + 32 * 16, int.from_bytes(b"DBXE", "little")]
    assert [dt.itemsize for dt, _ in STRUCTS.values()] == [n for _, n in STRUCTS.values()]
    assert got[13:] == [STRUCTS[s][0].fields[k][1] for s, k in fields]
    assert C_sizeof(dx.TiiConfig) == 32 and C_sizeof(dx.TiiResult) == 16
    assert dx.DELIVER_TII == 256 and dx.TII_MAX_RESULTS == 32 and dx.CHUNK_EXT_MAGIC == got[12] and dx.TII_EVENT_SLOT_BYTES == got[11]
    assert dx.CHUNK_HEADER.itemsize == 128
    # the bit is beside the others, not one of them: what == 0 ("everything") is made of these
    assert dx.DELIVER_TII & (dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF | dx.DELIVER_MSC_NOT_DABPLUS | dx.DELIVER_DG | dx.DELIVER_PAD |
                             dx.DELIVER_MOT | dx.DELIVER_ETI) == 0


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_the_library_exports_the_new_entries_and_declares_them():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.dabx_abi_version() == 6
