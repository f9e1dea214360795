"""The declarations of the RF spectrum and waterfall stage (include/dabx.h: dabx_set_spectrum_mode, dabx_read_spectrum,
dabx_get_spectrum_stats, dabx_spectrum_rows_device, dabx_spectrum_limits, dabx_spectrum_waterfall_row, dabx_spectrum_next_show,
dabx_spectrum_config, dabx_spectrum_record, dabx_spectrum_limits_rec, dabx_spectrum_stats, DABX_DELIVER_SPECTRUM, dabx_chunk_spectrum,
dabx_chunk_header_ext.off_spectrum) as a C compiler sees them, against the Python mirror (dabstar_amd/lib.py) and the built library; and
the library's own display limits and capture schedule, through their host entries, EXACTLY against the test models on tables that reach
every branch.  No device."""
import ctypes
import os
import subprocess

import numpy as np

import spectrum_cases as sp
from dabstar_amd import lib as dx

STRUCTS = {
    "dabx_spectrum_record": (dx.SPECTRUM_RECORD, 32),
    "dabx_spectrum_limits_rec": (dx.SPECTRUM_LIMITS, 32),
    "dabx_spectrum_stats": (dx.SPECTRUM_STATS, 64),
    "dabx_chunk_spectrum": (dx.CHUNK_SPECTRUM, 32),
    "dabx_chunk_header_ext": (dx.CHUNK_HEADER_EXT, 64),
}
NEW_SYMBOLS = ("dabx_set_spectrum_mode", "dabx_read_spectrum", "dabx_get_spectrum_stats", "dabx_spectrum_rows_device", "dabx_spectrum_limits",
               "dabx_spectrum_waterfall_row", "dabx_spectrum_next_show", "dabx_spectrum_look")
CONSTANTS = ("DABX_DELIVER_SPECTRUM", "DABX_SPECTRUM_BINS", "DABX_SPECTRUM_SIZE", "DABX_SPECTRUM_PERIOD", "DABX_SPECTRUM_RING",
             "DABX_SPECTRUM_SLOT_BYTES", "DABX_SPECTRUM_CHUNK_RECORDS", "DABX_SPECTRUM_AVR_SLOW", "DABX_SPECTRUM_AVR_MEDIUM",
             "DABX_SPECTRUM_AVR_FAST", "DABX_ABI_VERSION", "DABX_CHUNK_FRAMES")


def test_sizes_offsets_and_constants(tmp_path):
    fields = [(s, k) for s, (dt, _) in STRUCTS.items() for k in dt.names]
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "dabx.h"
int main(void)
{
  printf("%%zu %%zu %%zu %%zu %%zu %%zu ", sizeof(dabx_spectrum_config), sizeof(dabx_spectrum_record), sizeof(dabx_spectrum_limits_rec),
         sizeof(dabx_spectrum_stats), sizeof(dabx_chunk_spectrum), sizeof(dabx_chunk_header_ext));
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
    assert got[:6] == [32, 32, 32, 64, 32, 64]                # the ext struct is still 64 bytes
    c = dict(zip(CONSTANTS, got[6:6 + len(CONSTANTS)]))
    assert c == dict(DABX_DELIVER_SPECTRUM=65536, DABX_SPECTRUM_BINS=512, DABX_SPECTRUM_SIZE=2048, DABX_SPECTRUM_PERIOD=512000, DABX_SPECTRUM_RING=8,
                     DABX_SPECTRUM_SLOT_BYTES=32 + 32 + 512 * 4 + 512, DABX_SPECTRUM_CHUNK_RECORDS=6, DABX_SPECTRUM_AVR_SLOW=0,
                     DABX_SPECTRUM_AVR_MEDIUM=1, DABX_SPECTRUM_AVR_FAST=2, DABX_ABI_VERSION=6, DABX_CHUNK_FRAMES=dx.CHUNK_FRAMES)
    assert [dt.itemsize for dt, _ in STRUCTS.values()] == [n for _, n in STRUCTS.values()]
    assert got[6 + len(CONSTANTS):] == [STRUCTS[s][0].fields[k][1] for s, k in fields]
    assert ctypes.sizeof(dx.SpectrumConfig) == 32
    assert (dx.DELIVER_SPECTRUM, dx.SPECTRUM_BINS, dx.SPECTRUM_SIZE, dx.SPECTRUM_PERIOD, dx.SPECTRUM_RING, dx.SPECTRUM_SLOT_BYTES,
            dx.SPECTRUM_CHUNK_RECORDS) == tuple(c[k] for k in CONSTANTS[:7])
    assert dx.SPECTRUM_AVERAGING == dict(slow=0, medium=1, fast=2)
    assert (sp.BINS, sp.SIZE, sp.PERIOD) == (dx.SPECTRUM_BINS, dx.SPECTRUM_SIZE, dx.SPECTRUM_PERIOD)
    # the section is announced by the second of the three words that were reserved; the words in front of it stay where they were
    f = dx.CHUNK_HEADER_EXT.fields
    assert f["off_spectrum"][1] == 48 and f["off_cir"][1] == 40 and f["off_scope"][1] == 32 and f["reserved"][1] == 56
    # the bit is beside the others, not one of them, and none of the three masks that stay refused
    assert dx.DELIVER_SPECTRUM & (dx.DELIVER_FIB | dx.DELIVER_MSC | dx.DELIVER_SF | dx.DELIVER_MSC_NOT_DABPLUS | dx.DELIVER_DG | dx.DELIVER_PAD |
                                  dx.DELIVER_MOT | dx.DELIVER_ETI | dx.DELIVER_TII | dx.DELIVER_MP2_AUDIO | dx.DELIVER_AAC | dx.DELIVER_SCOPE |
                                  dx.DELIVER_CIR | 1024 | 4096 | 16384) == 0


def test_the_library_exports_the_new_entries_and_declares_them():
    L = dx.load()
    declared = dx.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.dabx_abi_version() == 6


def test_the_librarys_limits_are_the_models_exactly_on_every_branch():
    """spectrum_limits (csrc/spectrum_core.h), the function k_spectrum runs, through dabx_spectrum_limits, bit for bit the float32
    transcription of spectrum_viewer.cpp:220-230, :112-139 and waterfall_scope.cpp:57-60 -- for all three alphas and five zooms."""
    reached = set()
    n = 0
    for ext, lim, what in sp.limits_table():
        for avr in ("slow", "medium", "fast"):
            for zoom in (0, 1, 37, 99, 100):
                want_l, want_ymin, want_ymax, want_valid, br = sp.limits32(ext, lim, sp.ALPHA[avr], zoom)
                got_l, (ymin, ymax), valid = dx.spectrum_limits(ext, lim, avr, zoom)
                assert got_l.tobytes() == np.array(want_l, np.float32).tobytes(), (what, avr, zoom, got_l, want_l)
                assert np.float32(ymin).tobytes() == np.float32(want_ymin).tobytes() and np.float32(ymax).tobytes() == np.float32(want_ymax).tobytes()
                assert valid == want_valid, (what, avr, zoom)
                reached |= set(br)
                n += 1
    assert n == 9 * 15
    assert reached >= {"glob_min_below", "glob_range_under_20", "glob_second_shift", "glob_unchanged", "loc_looked_at", "loc_min_below",
                       "loc_range_under_20", "loc_second_shift"}, reached
    # by name: Glob unchanged, so Loc keeps a range of 5; one step of the medium filter from the initial limits
    l, y, valid = dx.spectrum_limits((-30.0, -90.0, -40.0, -45.0), (-30.0, -90.0, -40.0, -45.0), "fast", 100)
    assert l.tolist() == [-30.0, -90.0, -40.0, -45.0] and y == (-45.0, -40.0) and valid
    l, y, valid = dx.spectrum_limits((-20.0, -80.0, -25.0, -60.0), sp.LIMITS0, "medium", 0)
    assert np.allclose(l, [-29.0, -89.0, -30.4, -51.0], atol=1e-5) and valid and abs(y[1] - (-24.0)) < 1e-5
    # a range that is not positive: no row (yMax = Glob.Max + 5 at zoom 0 is never below Glob.Min + 25, so only the local pair can)
    assert dx.spectrum_limits((-30.0, -90.0, -45.0, -40.0), (-30.0, -90.0, -45.0, -40.0), "fast", 100)[2] is False
    L = dx.load()
    for bad in ((3, 0), (-1, 0), (1, 101), (1, -1)):
        assert L.dabx_spectrum_limits(dx._p(np.zeros(4, np.float32)), dx._p(np.zeros(4, np.float32)), bad[0], bad[1], dx._p(np.zeros(2, np.float32))) == -2


def test_the_librarys_waterfall_row_is_the_models():
    """spectrum_pixel through dabx_spectrum_waterfall_row against waterfall_scope.cpp:73-74 in float32: below, inside, above, the ends, a NaN"""
    db = np.array([-200.0, -90.0, -89.9, -60.0, -30.000002, -30.0, -25.0, 0.0, np.nan, -60.00001, -42.5], np.float32)
    for y in ((-90.0, -25.0), (-50.0, -31.0), (-89.0, -24.0)):
        want, _ = sp.pixels(db, y[0], y[1], np.float32)
        got = dx.spectrum_waterfall_row(db, y)
        assert got.tolist() == want.tolist(), (y, got, want)
    assert dx.spectrum_waterfall_row(db, (-90.0, -25.0))[[0, 1, 6, 7, 8]].tolist() == [0, 0, 255, 255, 0]


def _first_show(W, pieces):
    """the library's schedule over the pieces of a receiver's walk, in order -> E or None"""
    for kind, a, b in pieces:
        E = dx.spectrum_next_show(W, kind, a, b)
        if E is not None:
            return E
    return None


def _model(W, calls):
    """the Reader over the same walk, call by call -> E or None"""
    r = sp.Reader(W)
    for what, n in calls:
        if what == "search":
            r.search(n)
        elif what == "frame":
            r.frame(n)
        else:
            r.get_samples(n, False)
        if r.shows:
            return r.shows[0][1]
    return None


def test_the_librarys_schedule_is_the_models_on_the_table():
    """spectrum_next_show (csrc/spectrum_core.h), the function k_spectrum runs, through dabx_spectrum_next_show, against the call-by-call
    Reader (sample_reader.cpp:285-296)."""
    P, TU, TS, TN = sp.PERIOD, sp.TU, sp.TS, sp.TN
    W = 4243
    # W + 512 001 inside a search
    assert _first_show(W, [(0, W, W + 700000)]) == W + P + 1 == _model(W, [("search", 700000)])
    # ... the search ends exactly there, or one call earlier
    assert _first_show(W, [(0, W, W + P + 1)]) == W + P + 1 == _model(W, [("search", P + 1)])
    assert _first_show(W, [(0, W, W + P)]) is None and _model(W, [("search", P)]) is None
    # sample W + 512 000 inside the block read after a dip end: the correlation fails -> the first call of the search behind the block
    for into in (0, 1, 1000, TU - 1):
        D = W + P - into
        want = _model(W, [("search", D - W), ("block", TU), ("search", 5000)])
        assert want == D + TU + 1
        assert _first_show(W, [(0, W, D), (0, D + TU, D + TU + 5000)]) == want, into
        # ... the correlation succeeds -> the end of the frame's first symbol (the rest of symbol 0 does not show either)
        for start in (0, 300, 504, 700):
            want = _model(W, [("search", D - W), ("block", TU), ("frame", start)])
            assert want == D + TU + start + TS
            assert _first_show(W, [(0, W, D), (1, D + TU + start, 0)]) == want, (into, start)
    # every j = 1..75 reached by some W, in lock; and the frames that follow: E in the next frame and in the frame after next
    sym0_end = 10 * sp.TF + 777
    seen = set()
    for j in range(1, 76):
        for d in (0, 1, TS - 1):
            Wj = sym0_end + j * TS - P - 1 - d                 # the smallest E with E - W > P is symbol end j, for TS values of W
            E = dx.spectrum_next_show(Wj, 1, sym0_end, 0)
            r = sp.Reader(Wj)
            r.get_samples(sym0_end - Wj, False)
            r.frame(0)
            assert E == r.shows[0][1] == sym0_end + j * TS, (j, d)
            seen.add((E - sym0_end) // TS)
    assert seen == set(range(1, 76))
    # W so late that no symbol end of this frame is far enough: not in here; the gap across the null symbol and the next frame's symbol 0
    Wl = sym0_end + 75 * TS - P
    assert dx.spectrum_next_show(Wl, 1, sym0_end, 0) is None
    nxt = sym0_end + 75 * TS + TN + TU + 499                   # the next frame's symbol 0 ends 2656 + 2048 + start behind this frame's last symbol
    assert _first_show(Wl, [(1, sym0_end, 0), (1, nxt, 0)]) == nxt + TS == _model(Wl, [("block", sym0_end - Wl), ("frame", 0), ("block", TU), ("frame", 499)])
    # a window shown at a frame's symbol end is shown again in the frame after next (3 frames are 589 824 samples)
    f1, f2, f3 = sym0_end, sym0_end + sp.TF, sym0_end + 2 * sp.TF + 3
    W0 = f1 + 10 * TS
    E = _first_show(W0, [(1, f1, 0), (1, f2, 0), (1, f3, 0)])
    rd = sp.Reader(W0)
    for _ in range(65):
        rd.get_samples(TS, True)
    rd.get_samples(TN, False)
    rd.get_samples(f2 - TU - rd.pos, False)                    # (whatever lies between the frames is not shown)
    rd.get_samples(TU, False)
    rd.frame(0)
    rd.get_samples(f3 - TU - rd.pos, False)
    rd.get_samples(TU, False)
    rd.frame(0)
    assert E == rd.shows[0][1] and f3 < E <= f3 + 75 * TS
    # E - W > 512 000 strictly: a symbol end exactly 512 000 behind W does not show, the next one does
    Ws = sym0_end + 20 * TS - P
    assert dx.spectrum_next_show(Ws, 1, sym0_end, 0) == sym0_end + 21 * TS
    assert dx.spectrum_next_show(Ws - 1, 1, sym0_end, 0) == sym0_end + 20 * TS
    # an empty range, a range in front of the target, a bad kind
    assert dx.spectrum_next_show(W, 0, W + 10, W + 10) is None and dx.spectrum_next_show(W, 0, W, W + 100) is None
    assert dx.spectrum_next_show(W, 0, W + P + 5000, W + P + 6000) == W + P + 5001
    L = dx.load()
    L.dabx_spectrum_next_show.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
    L.dabx_spectrum_next_show.restype = ctypes.c_int64
    assert L.dabx_spectrum_next_show(0, 2, 0, 0) == -2
