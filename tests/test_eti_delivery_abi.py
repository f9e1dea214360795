"""The declarations of the delivery's ETI stage (include/dabx.h: DABX_DELIVER_ETI, dabx_chunk_header.off_eti, dabx_chunk_eti,
dabx_eti_frames_device) as a C compiler sees them, against the Python mirror (dabstar_amd/lib.py) and the built library.  No device."""
import os
import subprocess

from dabstar_amd import lib as dx

ETI_FIELDS = ("first_cif", "n_eti", "cifs_lost", "cifs_waiting", "cifs_refused", "cif_hi", "cif_lo", "rows_off", "fib_frames", "reserved")


def test_sizes_offsets_and_constants_of_the_eti_section(tmp_path):
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void)
{
  printf("%%zu %%zu %%zu %%zu %%d %%d %%d %%d %%d ", sizeof(dabx_chunk_header), offsetof(dabx_chunk_header, off_eti), offsetof(dabx_chunk_header, off_mot),
         sizeof(dabx_chunk_eti), DABX_DELIVER_ETI, DABX_MAX_KERNELS, DABX_ABI_VERSION, DABX_ETI_FRAME_BYTES, DABX_CHUNK_FRAMES);
%s
  printf("\\n");
  return 0;
}
""" % "\n".join('  printf("%%zu ", offsetof(dabx_chunk_eti, %s));' % k for k in ETI_FIELDS))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:9] == [128, 120, 112, 64, 128, 16, 6, 6144, 7]
    assert dx.CHUNK_HEADER.itemsize == 128 and dx.CHUNK_HEADER.fields["off_eti"][1] == 120 and dx.CHUNK_HEADER.fields["off_mot"][1] == 112
    assert dx.CHUNK_ETI.itemsize == 64 and dx.CHUNK_ETI.names == ETI_FIELDS
    assert got[9:] == [dx.CHUNK_ETI.fields[k][1] for k in ETI_FIELDS]
    assert dx.DELIVER_ETI == 128 and dx.ETI_FRAME_BYTES == 6144 and dx.CHUNK_FRAMES == 7
    # the bit is beside the others, not one of them: what == 0 ("everything") is made of these
    assert dx.DELIVER_ETI & (dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF | dx.DELIVER_MSC_NOT_DABPLUS | dx.DELIVER_DG | dx.DELIVER_PAD | dx.DELIVER_MOT) == 0


def test_the_library_exports_the_new_entry_and_declares_it():
    L = dx.load()
    assert "dabx_eti_frames_device" in dx.declared_symbols()
    for name in ("dabx_eti_frames_device", "dabx_eti_frame", "dabx_read_eti", "dabx_delivery_open"):
        assert hasattr(L, name), name
    assert L.dabx_abi_version() == 6
