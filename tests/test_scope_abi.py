"""The declarations of the IQ scope and the carrier plots (include/dabx.h: dabx_set_scope_mode, dabx_read_scope, dabx_get_scope_stats,
dabx_scope_cadence_frame, dabx_scope_config, dabx_scope_record, dabx_scope_stats, DABX_DELIVER_SCOPE, dabx_chunk_scope) as a C compiler sees
them, against the Python mirror (dabstar_amd/lib.py) and the built library; and the library's own counters against the test model.  No device."""
import ctypes
import os
import subprocess

import numpy as np

import scope_cases as sc
from dabstar_amd import lib as dx

STRUCTS = {
    "dabx_scope_record": (dx.SCOPE_RECORD, 32),
    "dabx_scope_stats": (dx.SCOPE_STATS, 64),
    "dabx_chunk_scope": (dx.CHUNK_SCOPE, 32),
    "dabx_chunk_header_ext": (dx.CHUNK_HEADER_EXT, 64),
}
NEW_SYMBOLS = ("dabx_set_scope_mode", "dabx_read_scope", "dabx_get_scope_stats", "dabx_scope_cadence_frame")


def test_sizes_offsets_and_constants(tmp_path):
    fields = [(s, k) for s, (dt, _) in STRUCTS.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void)
{
  printf("%%zu %%zu %%zu %%zu %%zu ", sizeof(dabx_scope_config), sizeof(dabx_scope_record), sizeof(dabx_scope_stats), sizeof(dabx_chunk_scope),
         sizeof(dabx_chunk_header_ext));
  printf("%%d %%d %%d %%d %%d ", DABX_DELIVER_SCOPE, DABX_SCOPE_CARRIERS, DABX_SCOPE_SLOT_BYTES, DABX_ABI_VERSION, DABX_CHUNK_FRAMES);
%s
  printf("\\n");
  return 0;
}
""" % "\n".join('  printf("%%zu ", offsetof(%s, %s));' % f for f in fields))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:5] == [32, 32, 64, 32, 64]                    # both structs of the mode are 32 bytes
    assert got[5:10] == [8192, 1536, 32 + 1536 * 8 + 1536 * 4, 6, dx.CHUNK_FRAMES]
    assert [dt.itemsize for dt, _ in STRUCTS.values()] == [n for _, n in STRUCTS.values()]
    assert got[10:] == [STRUCTS[s][0].fields[k][1] for s, k in fields]
    assert ctypes.sizeof(dx.ScopeConfig) == 32
    assert dx.DELIVER_SCOPE == 8192 and dx.SCOPE_SLOT_BYTES == got[7] and dx.SCOPE_CARRIERS == 1536
    assert "off_scope" in dx.CHUNK_HEADER_EXT.names
    # the bit is beside the others, not one of them
    assert dx.DELIVER_SCOPE & (dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF | dx.DELIVER_MSC_NOT_DABPLUS | dx.DELIVER_DG | dx.DELIVER_PAD |
                               dx.DELIVER_MOT | dx.DELIVER_ETI | dx.DELIVER_TII | dx.DELIVER_MP2_AUDIO | dx.DELIVER_AAC | 1024 | 4096) == 0
    assert set(dx.SCOPE_CARRIER_TYPES.values()) == set(sc.CARRIER_TYPES) and set(dx.SCOPE_IQ_TYPES.values()) == set(sc.IQ_TYPES)


def test_the_library_exports_the_new_entries_and_declares_them():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.dabx_abi_version() == 6


def test_the_librarys_counters_are_the_models():
    """scope_counters_frame (csrc/scope_core.h), the function k_scope runs, through its host entry: 700 decoded frames from a fresh decoder
    against scope_cases.Counters, counters and shown symbol after every frame -- once round the 75 symbols and on."""
    L = dx.load()
    L.dabx_scope_cadence_frame.argtypes = [ctypes.c_void_p]
    st = np.array([0, 0, 1], np.int32)
    m, shown = sc.Counters(), []
    for f in range(700):
        got, want = L.dabx_scope_cadence_frame(dx._p(st)), m.frame()
        assert got == want and st.tolist() == [m.cnt_iq, m.cnt_stat, m.next_sym], f
        if got:
            shown.append((f, got))
    assert shown[:4] == [(2, 1), (4, 1), (6, 1), (8, 2)]
    assert max(l for _, l in shown) == 75 and shown[-1][1] < 75          # the symbol has wrapped 75 -> 1
    for bad in ([0, 0, 0], [0, 0, 76]):
        assert L.dabx_scope_cadence_frame(dx._p(np.array(bad, np.int32))) == -2
    assert L.dabx_scope_cadence_frame(None) == -2
