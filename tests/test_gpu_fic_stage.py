"""The FIC stage (k_fic_frame) on soft bits a Viterbi decoder cannot repair and on crafted FIBs, against oracle/fic.c -- exactly.

The soft bits go straight into the engine's FIC symbols (dx.fic_inject / dx.fic_decode_frame: the library's internal test entries, no
IQ, no front end), so the decoder sees exact ties, saturated and out-of-range symbols, pure noise, and FIBs with a good CRC that no
multiplexer would send.  tests/fic_cases.py builds the schedules and runs the oracle; tests/test_fic_cases.py proves, without a device,
that they cover what they claim and that the CIF-counter model is oracle/fic.c wherever the reference stays inside the FIB."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fic_cases as fc
from dabstar_amd import lib as dx
from oracle_lib import FicBer

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STATS = ("frames", "fib_ok", "fib_total", "fic_ratio_percent", "cif_count", "fic_ber_bits", "fic_ber_errors")


def _expected_stats(recs, n, mode):
    """dabx_stats of a stream after its first n frames."""
    if n == 0:
        return dict.fromkeys(STATS, 0)
    r = recs[n - 1]
    ber = r["ber_wrap"] if mode == 0 else r["ber"]
    return dict(frames=n, fib_ok=sum(int(q["crc"].sum()) for q in recs[:n]), fib_total=12 * n, fic_ratio_percent=10 * r["ratio"],
                cif_count=r["cif_model"], fic_ber_bits=ber[0], fic_ber_errors=ber[1])


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["tie_mode_0", "tie_mode_1", "tie_mode_2"])
def test_engine_fic_stage_equals_the_oracle_frame_by_frame(mode):
    """Six streams, 24 steps, every stream its own rotation of classes and crafted FIBs; streams 4 and 5 have no frame in three steps
    each (fresh soft bits are injected all the same: nothing of theirs may move).  After every step, per stream: the newest frame's
    FIBs and CRC verdicts and the six counters of dabx_stats.  Mode 0: behind an int16_edges block the BER pair is the oracle's with
    every soft bit >= 32641 taken as negative (the reference's `soft + 127` wraps before the hard decision; include/dabx.h)."""
    S = fc.N_STREAMS
    exp = [fc.oracle_stream(s, mode) for s in range(S)]
    soft = [fc.stream_frames(s)[0] for s in range(S)]
    eng = dx.Engine(n_streams=S, max_subch=0, fic_only=True, out_frames=4, ring_frames=2, viterbi_tie_mode=mode)
    try:
        at = [0] * S
        for step in range(fc.N_STEPS):
            present = [0 if step in fc.ABSENT.get(s, ()) else 1 for s in range(S)]
            for s in range(S):
                # an absent stream gets its NEXT frame negated: decoding it would show in every output
                dx.fic_inject(eng, s, soft[s][at[s]] if present[s] else -(soft[s][at[s]] // 2) - 1)
            dx.fic_decode_frame(eng, present)
            for s in range(S):
                at[s] += present[s]
                fibs, crc = eng.read_fibs(s, 1)
                if at[s] == 0:
                    assert fibs.shape[0] == 0, (step, s)
                else:
                    r = exp[s][at[s] - 1]
                    assert np.array_equal(fibs[0], r["fibs"]) and np.array_equal(crc[0], r["crc"]), (step, s)
                st = eng.stats(s)
                want = _expected_stats(exp[s], at[s], mode)
                assert {k: st[k] for k in STATS} == want, (step, s, present[s])
        for s in range(S):
            assert at[s] == fc.stream_frames_count(s)
            fibs, crc = eng.read_fibs(s, 4)
            assert np.array_equal(fibs, np.stack([r["fibs"] for r in exp[s][-4:]])), s
            assert np.array_equal(crc, np.stack([r["crc"] for r in exp[s][-4:]])), s
    finally:
        eng.close()
    if mode == 0:      # the wrap rule was in play: as many blocks as the schedules have int16_edges blocks, and it moved the expected pair
        edges = sum(k.count("int16_edges") for s in range(S) for k in fc.stream_frames(s)[1])
        wrapped = sum(r["wrap_blocks"] for s in range(S) for r in fc.oracle_calls(fc.symbol_calls(soft[s]), 0))
        assert wrapped == edges == 38
        assert sum(r["ber"] != r["ber_wrap"] for s in range(S) for r in exp[s]) >= S
    else:
        assert all(r["ber"] == r["ber_wrap"] for s in range(S) for r in exp[s])


def test_batch_entry_decodes_the_same_frames():
    """dabx_fic_decode (tie mode 0, one fresh stream per row): every frame of every schedule at once."""
    soft = np.concatenate([fc.stream_frames(s)[0] for s in range(fc.N_STREAMS)])
    recs = [r for s in range(fc.N_STREAMS) for r in fc.oracle_stream(s, 0)]
    fibs, crc = dx.fic_decode(soft)
    assert len(recs) == soft.shape[0] == 138
    assert np.array_equal(fibs, np.stack([r["fibs"] for r in recs]))
    assert np.array_equal(crc, np.stack([r["crc"] for r in recs]))


@pytest.mark.parametrize("s", range(fc.N_STREAMS))
def test_per_symbol_handle_follows_the_oracle_through_a_frame_cut_short(s):
    """The dabx_fic_* handle, symbol by symbol, on a whole schedule with one extra frame that ends after its symbol 1: its block 0 is
    decoded and counted, the next symbol 1 starts over.  The 40th block is then the first of the count = 2 launch of a symbol 3, and
    the BER pair is halved between the two blocks of one launch."""
    soft = fc.stream_frames(s)[0]
    calls = fc.symbol_calls(soft, short_after=5)
    recs = fc.oracle_calls(calls, 0)
    blocks_before = np.cumsum([0] + [len(r["completed"]) for r in recs])
    k40 = int(np.searchsorted(blocks_before, 40, side="left")) - 1           # the call that completes the 40th block
    assert blocks_before[k40] == 39 and recs[k40]["completed"] == [2, 3] and recs[k40]["blocks"] == 1
    L = dx.load()
    h = C.c_void_p()
    dx.check(L.dabx_fic_create(C.byref(h)))
    try:
        dx.check(L.dabx_fic_restart(h))
        cif = 0
        for i, ((sym_soft, sym), r) in enumerate(zip(calls, recs)):
            first = C.c_int(-1)
            done = dx.check(L.dabx_fic_process_block(h, dx._p(sym_soft), sym, C.byref(first)))
            assert done == len(r["completed"]) and (done == 0 or first.value == r["completed"][0]), i
            for b in r["completed"]:
                fibs, crc = np.zeros((3, 32), np.uint8), np.zeros(3, np.uint8)
                dx.check(L.dabx_fic_get_fibs(h, b, dx._p(fibs), dx._p(crc)))
                assert np.array_equal(fibs, r["fibs"][3 * b:3 * b + 3]) and np.array_equal(crc, r["crc"][3 * b:3 * b + 3]), (i, b)
                cif = fc.model_track(cif, fibs, crc)
            assert L.dabx_fic_get_cif_count(h) == cif, i
            assert L.dabx_fic_get_decode_ratio_percent(h) == 10 * r["ratio"], i
            ber = FicBer()
            dx.check(L.dabx_fic_get_ber(h, C.byref(ber)))
            assert (ber.bits, ber.errors, ber.blocks) == (r["ber_wrap"][0], r["ber_wrap"][1], r["blocks"]), i
    finally:
        L.dabx_fic_destroy(h)


def test_eti_frames_carry_the_counter_dabx_stats_shows_on_a_non_conformant_fib():
    """One walk for both (csrc/fig00.h): a FIG 0/0 of length 4, and one whose header lies at byte 26, set dabx_stats.cif_count AND the
    counter of the ETI frames of their CIFs (FCT = (lo + minor) % 250, FP = counter % 8; eti_generator.cpp:212-231).  The ETI reader used
    to walk with length checks of its own and wrote no frame for such a FIB."""
    cases = dict(fc.crafted_singles())
    for name in ("fig00_length_4", "header_at_26"):
        fib = cases[name]
        hi, lo = fc.model_fig00(fib)
        assert dx.parse_fibs(fib[None], np.ones(1, np.uint8))[1] == -1            # the strict walk of dabx_fibdec sees none here
        blocks = [fc.coded_block([fib, fc.FILLER, fc.FILLER])] + [fc.coded_block([fc.FILLER] * 3)] * 3
        eng = dx.Engine(n_streams=1, max_subch=1, out_frames=4, ring_frames=2)
        try:
            dx.fic_inject(eng, 0, np.concatenate(blocks))
            dx.fic_decode_frame(eng, [1])
            dx.msc_decode(eng, [4], 4)                                           # the frame's four CIFs exist (no sub-channel is active)
            assert eng.stats(0)["cif_count"] == hi * 250 + lo, name
            eti, lost = eng.read_eti(0, 8)
            assert eti.shape[0] == 4 and lost == 0, name
            for minor in range(4):
                l2 = (lo + minor) % 250
                h2 = min(hi + (lo + minor) // 250, 20)
                assert eti[minor, 4] == l2 and eti[minor, 6] >> 5 == (h2 * 250 + l2) % 8, (name, minor)
                assert np.array_equal(eti[minor, 8 + 4:8 + 4 + 96], np.concatenate(([fib, fc.FILLER, fc.FILLER] if minor == 0 else [fc.FILLER] * 3))), (name, minor)
        finally:
            eng.close()


def test_the_test_entries_refuse_what_they_cannot_do():
    eng = dx.Engine(n_streams=2, max_subch=0, fic_only=True, out_frames=2, ring_frames=2)
    try:
        L = dx.load()
        soft = np.zeros(9216, np.int16)
        E_ARG = -2                                                          # DABX_E_ARG (include/dabx.h)
        for stream in (-1, 2):
            assert L.dabx_internal_fic_inject(eng._h, stream, dx._p(soft)) == E_ARG
        assert L.dabx_internal_fic_inject(eng._h, 0, None) == E_ARG and L.dabx_internal_fic_decode(eng._h, None) == E_ARG
        for present in ([2, 0], [0, -1]):
            assert L.dabx_internal_fic_decode(eng._h, dx._p(np.array(present, np.int32))) == E_ARG
        with pytest.raises(ValueError):
            dx.fic_decode_frame(eng, [1])
        dx.fic_decode_frame(eng, [0, 0])                                   # nobody has a frame: nothing moves
        assert eng.stats(0)["frames"] == 0 and eng.stats(1)["fib_total"] == 0
    finally:
        eng.close()


def test_the_entries_work_in_the_hipmodule_form():
    """The same engine test (tie mode 1) with the binding pointed at hipmodule/libdabx.so: k_fic_inject and its companions are found in
    the code objects and launched through hipModuleLaunchKernel."""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_fic_stage.py", "-k", "tie_mode_1 or refuse"], cwd=ROOT, env=hipmodule_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
