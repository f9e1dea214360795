"""The declarations of the channel impulse response and correlation plot stage (include/dabx.h: dabx_set_cir_mode, dabx_read_cir,
dabx_get_cir_stats, dabx_cir_rows_device, dabx_cir_rows_due, dabx_cir_row_trusted, dabx_cir_config, dabx_cir_record, dabx_cir_stats,
DABX_DELIVER_CIR, dabx_chunk_cir, dabx_chunk_header_ext.off_cir) as a C compiler sees them, against the Python mirror (dabstar_amd/lib.py)
and the built library; and the library's own window walk and trust rule, through their host entries, against the test models on
exhaustive small tables.  No device."""
import ctypes
import os
import subprocess

import numpy as np

import cir_cases as cc
from dabstar_amd import lib as dx

STRUCTS = {
    "dabx_cir_record": (dx.CIR_RECORD, 32),
    "dabx_cir_stats": (dx.CIR_STATS, 64),
    "dabx_chunk_cir": (dx.CHUNK_CIR, 32),
    "dabx_chunk_header_ext": (dx.CHUNK_HEADER_EXT, 64),
}
NEW_SYMBOLS = ("dabx_set_cir_mode", "dabx_read_cir", "dabx_get_cir_stats", "dabx_cir_rows_device", "dabx_cir_rows_due", "dabx_cir_row_trusted")
CONSTANTS = ("DABX_DELIVER_CIR", "DABX_CIR_ROWS", "DABX_CIR_WINDOW", "DABX_CIR_PERIOD", "DABX_CIR_CORR_LAGS", "DABX_CIR_MAX_INDICES",
             "DABX_CIR_INDEX_ROOM", "DABX_CIR_SLOT_BYTES", "DABX_CIR_CHUNK_RECORDS", "DABX_CIR_KIND_CIR", "DABX_CIR_KIND_CORRELATION",
             "DABX_ABI_VERSION", "DABX_CHUNK_FRAMES")


def test_sizes_offsets_and_constants(tmp_path):
    fields = [(s, k) for s, (dt, _) in STRUCTS.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void)
{
  printf("%%zu %%zu %%zu %%zu %%zu ", sizeof(dabx_cir_config), sizeof(dabx_cir_record), sizeof(dabx_cir_stats), sizeof(dabx_chunk_cir),
         sizeof(dabx_chunk_header_ext));
%s
%s
  printf("\\n");
  return 0;
}
""" % ("\n".join('  printf("%%d ", (int)%s);' % c for c in CONSTANTS), "\n".join('  printf("%%zu ", offsetof(%s, %s));' % f for f in fields)))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(os.path.dirname(__file__), "..", "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:5] == [32, 32, 64, 32, 64]                    # the ext struct is still 64 bytes
    c = dict(zip(CONSTANTS, got[5:5 + len(CONSTANTS)]))
    assert c == dict(DABX_DELIVER_CIR=32768, DABX_CIR_ROWS=385, DABX_CIR_WINDOW=97 * 2048, DABX_CIR_PERIOD=6 * 196608, DABX_CIR_CORR_LAGS=2048,
                     DABX_CIR_MAX_INDICES=69, DABX_CIR_INDEX_ROOM=72, DABX_CIR_SLOT_BYTES=32 + 2048 * 4 + 72 * 2, DABX_CIR_CHUNK_RECORDS=4,
                     DABX_CIR_KIND_CIR=0, DABX_CIR_KIND_CORRELATION=1, DABX_ABI_VERSION=6, DABX_CHUNK_FRAMES=dx.CHUNK_FRAMES)
    assert [dt.itemsize for dt, _ in STRUCTS.values()] == [n for _, n in STRUCTS.values()]
    assert got[5 + len(CONSTANTS):] == [STRUCTS[s][0].fields[k][1] for s, k in fields]
    assert ctypes.sizeof(dx.CirConfig) == 32
    assert (dx.DELIVER_CIR, dx.CIR_ROWS, dx.CIR_WINDOW, dx.CIR_PERIOD, dx.CIR_CORR_LAGS, dx.CIR_MAX_INDICES, dx.CIR_INDEX_ROOM, dx.CIR_SLOT_BYTES,
            dx.CIR_CHUNK_RECORDS, dx.CIR_KIND_CIR, dx.CIR_KIND_CORRELATION) == tuple(c[k] for k in CONSTANTS[:11])
    assert (cc.ROWS, cc.WINDOW, cc.PERIOD, cc.MAX_INDICES) == (dx.CIR_ROWS, dx.CIR_WINDOW, dx.CIR_PERIOD, dx.CIR_MAX_INDICES)
    # the section is announced by the first of the three words that were reserved
    assert dx.CHUNK_HEADER_EXT.fields["off_cir"][1] == 40 and dx.CHUNK_HEADER_EXT.fields["off_scope"][1] == 32
    # the index list's bound: 750 positions, an accepted peak moves the walk on by 11
    assert -(-(cc.I1 - cc.I0) // (cc.GAP + 1)) == c["DABX_CIR_MAX_INDICES"] <= c["DABX_CIR_INDEX_ROOM"]
    # the bit is beside the others, not one of them, and none of the three masks that stay refused
    assert dx.DELIVER_CIR & (dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF | dx.DELIVER_MSC_NOT_DABPLUS | dx.DELIVER_DG | dx.DELIVER_PAD |
                             dx.DELIVER_MOT | dx.DELIVER_ETI | dx.DELIVER_TII | dx.DELIVER_MP2_AUDIO | dx.DELIVER_AAC | dx.DELIVER_SCOPE |
                             1024 | 4096 | 16384) == 0


def test_the_library_exports_the_new_entries_and_declares_them():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.dabx_abi_version() == 6


def _walk_entry():
    L = dx.load()
    L.dabx_cir_rows_due.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.dabx_cir_rows_due.restype = ctypes.c_int

    def call(base, win, rows_done, wr, cap):
        w = np.array([base, win, rows_done], np.int64)
        first, done = ctypes.c_int64(-1), ctypes.c_int32(-1)
        n = L.dabx_cir_rows_due(dx._p(w), wr, cap, ctypes.byref(first), ctypes.byref(done))
        return n, first.value, done.value, w.tolist()
    return L, call


def test_the_librarys_window_walk_is_the_models_on_the_table():
    """cir_rows_due / cir_rows_advance (csrc/cir_core.h), the functions k_cir and k_cir_finish run, through their host entry: every row
    boundary +-1 sample around wr, the last row, the hand-over to window n + 1, caps that bind."""
    L, call = _walk_entry()
    table = cc.walk_table()
    assert len(table) > 80000 and {(wr - base - win * cc.PERIOD - cc.TU) // cc.ROW_STEP for base, win, _, wr, _ in table} >= set(range(cc.ROWS))
    seen = set()
    for base, win, rows_done, wr, cap in table:
        m = cc.Walk(base, win, rows_done)
        want = m.step(wr, cap)
        n, first, done, w = call(base, win, rows_done, wr, cap)
        assert (n, first, done) == want and w == [m.base, m.win, m.rows_done], (base, win, rows_done, wr, cap)
        seen.add(("none" if n == 0 else "some", "done" if done else "open", "capped" if n == cap and cap < cc.ROWS else "free"))
    assert {("none", "open", "free"), ("some", "open", "free"), ("some", "done", "free"), ("some", "open", "capped"), ("some", "done", "capped")} <= seen
    # a whole stream of steps: a frame's worth of samples per step from a base that is no multiple of 512, two windows and on
    m, w = cc.Walk(4243), [4243, 0, 0]
    completed = []
    for step in range(1, 16):
        wr = step * cc.TF
        want = m.step(wr)
        n, first, done, w = call(*w, wr, cc.ROWS)
        assert (n, first, done) == want and w == [m.base, m.win, m.rows_done], step
        if done:
            completed.append(step)
    assert completed == [2, 8, 14]                            # window n ends at 4243 + n * 6 T_F + 198 656: in frames 2, 8, 14
    for bad in ([-1, 0, 0], [0, -1, 0], [0, 0, 385]):
        assert L.dabx_cir_rows_due(dx._p(np.array(bad, np.int64)), 0, 1, None, None) == -2
    assert L.dabx_cir_rows_due(None, 0, 1, None, None) == -2


def test_the_librarys_trust_rule_is_the_models_on_the_table():
    """cir_row_trusted (csrc/cir_core.h), the function k_cir runs: first == rd, first == horizon - ring_len +- 1, horizon = ~0"""
    L = dx.load()
    L.dabx_cir_row_trusted.argtypes = [ctypes.c_uint64] * 4
    table = cc.trust_table()
    assert len(table) > 300 and {t[4] for t in table} == {True, False}
    for first, rd, horizon, ring_len, want in table:
        assert bool(L.dabx_cir_row_trusted(first, rd, horizon, ring_len)) == want, (first, rd, horizon, ring_len)
    # the cases by name
    assert L.dabx_cir_row_trusted(1000, 1000, cc.U64, 4096) == 1                    # first == rd: not read yet
    assert L.dabx_cir_row_trusted(999, 1000, cc.U64, 4096) == 0                     # read, and a zero-copy producer may be anywhere
    assert L.dabx_cir_row_trusted(999, 1000, 999 + 4096, 4096) == 1                 # first == horizon - ring_len
    assert L.dabx_cir_row_trusted(999, 1000, 999 + 4096 + 1, 4096) == 0             # ... one sample further: its slot may be being written
    assert L.dabx_cir_row_trusted(999, 1000, 999 + 4096 - 1, 4096) == 1
    assert L.dabx_cir_row_trusted(0, 5, 100, 4096) == 1                             # nothing has been round the ring yet
