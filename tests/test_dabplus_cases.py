"""No device: the inputs of test_gpu_dabplus_stage.py are what they claim to be, shown on the oracle back end alone (oracle/msc.c) for
the very seeds, layouts and scenarios the GPU test runs (dabplus_cases.all_cases).

  * the noise-free soft bits decode to exactly the intended logical frames, so the Viterbi decoder and the puncturing map add nothing
    to what k_dabplus sees;
  * every record the oracle writes passes a check that shares no code with it (_check_record_against_its_super_frame);
  * the coverage conditions -- which branches of the super-frame stage the scenarios reach -- are asserted per bit rate and over the
    whole set, from the oracle's records and counters over accepted super frames.  A seed that misses one is a reason to change the
    seed or the generator, never the condition."""
import collections

import numpy as np
import pytest

import dabplus_cases as dc
from tools import dab_synth as ds


@pytest.fixture(scope="module")
def cases():
    """[(set number, layout, stream, per-slot facts, per-slot intended frames, per-slot oracle results)]"""
    out = []
    for set_no, lay, s in dc.all_cases():
        facts, frames, _cifs, ora = dc.stream_case(set_no, lay, s)
        out.append((set_no, lay, s, facts, frames, ora))
    return out


def _slots(cases, set_no=None, dab_plus_only=True):
    for n, lay, s, facts, frames, ora in cases:
        if set_no is not None and n != set_no:
            continue
        for j, c in enumerate(lay):
            if c.kbps and (c.dab_plus or not dab_plus_only):
                yield c, s, facts[j], frames[j], ora[j]


def test_the_fast_crc_and_rs_encoders_are_the_synthesiser_s():
    rng = np.random.default_rng(1)
    d = rng.integers(0, 256, (110, 7)).astype(np.uint8)
    p = dc.rs_parity_columns(d)
    assert all(np.array_equal(p[:, j], ds.rs_parity(d[:, j])) for j in range(7))
    for n in (0, 1, 2, 3, 64, 960):
        b = bytes(rng.integers(0, 256, n).astype(np.uint8))
        assert dc.crc16_fast(b) == ds.crc16(b) == dc._crc16(b)


def test_a_clean_super_frame_is_what_the_synthesiser_builds():
    """The generator's clean 3-AU frame passes the same checks as ds.build_superframe's: fire code, RS, AU CRCs, all by the oracle."""
    import oracle_lib as ol
    for R in (1, 3, 8, 48):
        full = dc.super_frame(R, np.random.default_rng(R), dc.CLEAN)
        assert full.shape == (120 * R,) and ol.oracle().ora_firecode_check(np.ascontiguousarray(full[:11])) == 1
        for j in range(R):
            out = np.zeros(110, np.uint8)
            assert ol.oracle().ora_rs_dec(np.ascontiguousarray(full[j::R]), out) == 0
        for st, en in zip([6, 6 + (110 * R - 6) // 3], [6 + (110 * R - 6) // 3, 6 + 2 * ((110 * R - 6) // 3)]):
            if en - st <= 962:
                assert ds.crc16(bytes(full[st:en - 2])) == (int(full[en - 2]) << 8 | int(full[en - 1]))


def test_the_sets_hold_what_the_gpu_tests_are_told_to_run(cases):
    assert sorted(c.kbps for n, lay, s, *_ in cases if n == 0 and s == 0 for c in lay) == dc.RATES and len(dc.RATES) == 48
    assert dc.EVERY_RATE_STREAMS >= 2 and dc.BOUNDARY_STREAMS >= 5
    R = [k // 8 for k in dc.BOUNDARY_RATES]
    assert 1 in R and 8 in R and 48 in R and any(r % 2 for r in R if r > 1)
    assert sorted(dc.BOUNDARY_COUNTS) == [0, 1, 4, 5, 6, 13, 27, 28]
    sched = dc.boundary_schedule()
    for s in range(dc.BOUNDARY_STREAMS):
        col = [c[s] for c in sched]
        assert sum(col) == dc.N_FRAMES and set(dc.BOUNDARY_COUNTS) <= set(col)
        assert {int(v) % 5 for v in np.cumsum(col)} == {0, 1, 2, 3, 4}          # the batch ends cut the five-frame windows at every place


def test_noise_free_soft_bits_decode_to_exactly_the_intended_logical_frames(cases):
    bad = [(c.kbps, s) for c, s, _f, frames, o in _slots(cases, dab_plus_only=False) if not np.array_equal(o["frames"], frames)]
    assert not bad, bad
    assert all(o["stats"]["cif_out"] == dc.N_FRAMES for *_x, o in _slots(cases, dab_plus_only=False))


def test_every_oracle_record_passes_the_independent_check(cases):
    n = 0
    for c, s, _f, _frames, o in _slots(cases):
        assert len(o["sfi"]) == len(o["sf"]) == o["stats"]["sf_ok"] >= 16, (c.kbps, s)      # >= 16: the device's ring of 16 wraps
        for r, sf in zip(o["sfi"], o["sf"]):
            dc._check_record_against_its_super_frame(r, sf, c.kbps)
            n += 1
        st = o["stats"]
        assert int(o["sfi"]["rs_corrected"].astype(np.int64).sum()) <= st["rs_corr"] and int(o["sfi"]["rs_failed"].astype(np.int64).sum()) <= st["rs_fail"]
        assert sum(bin(int(v)).count("1") for v in o["sfi"]["au_crc_ok"]) == st["au_ok"]
        assert int(o["sfi"]["num_aus"].astype(np.int64).sum()) == st["au_ok"] + st["au_bad"]
        assert int(o["sfi"]["fc_corrected"].astype(np.int64).sum()) == st["fc_corr"]
    print("records checked:", n)


def _aus(r):
    n = int(r["num_aus"])
    st = [int(v) for v in r["au_start"][:n + 1]]
    for a in range(n):
        yield st[a + 1] - st[a] - 2, bool(r["au_len_bad"] >> a & 1), bool(r["au_crc_ok"] >> a & 1)


def test_coverage_conditions_of_every_bit_rate(cases):
    """Per rate, over its streams' accepted super frames: all four header layouts; a fire-code correction; a frame with corrected code
    words and none failed; one with failed code words; a loss of sync (four failed windows, sf_fail) with an accepted super frame
    behind it; a changed phase."""
    per = collections.defaultdict(list)
    for c, s, _f, _frames, o in _slots(cases, set_no=0):
        per[c.kbps].append(o)
    assert sorted(per) == dc.RATES
    for kbps in dc.RATES:
        recs = np.concatenate([o["sfi"] for o in per[kbps]])
        assert set(recs["num_aus"].tolist()) == {2, 3, 4, 6}, kbps
        assert (recs["fc_corrected"] == 1).any(), kbps
        assert ((recs["rs_corrected"] > 0) & (recs["rs_failed"] == 0)).any(), kbps
        assert (recs["rs_failed"] > 0).any(), kbps
        resync = False
        for o in per[kbps]:
            ff = o["sfi"]["first_frame"].astype(np.int64)
            # more than 20 frames between two accepted super frames: four windows in a row failed in between (oracle/msc.c mp4_add_to_frame)
            resync = resync or (o["stats"]["sf_fail"] >= 1 and bool((np.diff(ff) > 20).any()))
            assert len(set((ff % 5).tolist())) >= 2, kbps
        assert resync, kbps


def test_coverage_conditions_of_the_whole_set(cases):
    judged, marked_bad, guard_only = set(), set(), 0
    exact_k, parity_only_k, all_dirty, last_only_odd, first_only = set(), set(), 0, 0, 0
    phases, decoys, n_au_hist = set(), 0, collections.Counter()
    totals = collections.Counter()
    for c, s, facts, _frames, o in _slots(cases, set_no=0):
        R = c.kbps // 8
        totals.update(o["stats"])
        phases |= set(((o["sfi"]["first_frame"].astype(np.int64) - facts["junk"]) % 5).tolist()) | set()
        decoys += facts["decoy"] in o["sfi"]["first_frame"].tolist()
        for r, sf in zip(o["sfi"], o["sf"]):
            n_au_hist[int(r["num_aus"])] += 1
            for ln, len_bad, crc_ok in _aus(r):
                if len_bad:
                    marked_bad.add(ln if ln > 0 else -1)
                    guard_only += 0 <= ln <= 960
                else:
                    judged.add((ln, crc_ok))
            f = facts["sf"].get(int(r["first_frame"]))
            if f is None or f["kind"].noise_frame >= 0 or not f["dirty"] or f["kind"].k > 5:
                continue
            k, d = f["kind"].k, f["dirty"]
            # the decoder counts the corrections it makes in data bytes; an error it locates in a parity byte is not one (reed_solomon.cpp:223-227,
            # oracle/fec.c rs_decode255), so errors in parity bytes only leave a record like a clean frame's -- after the whole decoder ran
            in_data = sum(p < 110 for pos in d.values() for p in pos)
            corrected = int(r["rs_corrected"]) == in_data and int(r["rs_failed"]) == 0 and np.array_equal(sf[11:], f["sf"][11:])
            if not corrected:
                continue
            if len(d) == 1 and in_data == k:
                exact_k.add(k)                      # one code word, k errors, all in data bytes, and the record counts k
            if len(d) == 1 and in_data == 0:
                parity_only_k.add(k)
            all_dirty += len(d) == R and R > 1
            last_only_odd += list(d) == [R - 1] and R % 2 == 1 and R > 1
            first_only += list(d) == [0] and R > 1
    print("accepted super frames by number of AUs:", dict(sorted(n_au_hist.items())), "; oracle counters summed:", dict(totals))
    print("AU lengths judged by CRC (length, verdict):", len(judged), "; lengths marked bad:", len(marked_bad), "; by the end-of-frame guard alone:", guard_only)
    print("exactly-k corrections seen:", sorted(exact_k), "; in parity bytes only:", sorted(parity_only_k), "; all code words dirty:", all_dirty,
          "; only the last at odd R:", last_only_odd, "; only code word 0:", first_only, "; decoy headers locked on:", decoys, "of", sum(1 for _ in _slots(cases, set_no=0)))
    for ln in dc.EDGE_LENGTHS:
        if ln <= 960:
            assert (ln, True) in judged and (ln, False) in judged, ln
    assert 961 in marked_bad and -1 in marked_bad
    assert guard_only >= 1
    assert exact_k == {1, 2, 3, 4, 5} and parity_only_k
    assert all_dirty and last_only_odd and first_only
    # the super-frame start relative to the first decoded frame: where the oracle found them, and where the generator put them
    found = set()
    for c, s, facts, _frames, o in _slots(cases, set_no=0):
        found |= set((o["sfi"]["first_frame"].astype(np.int64) % 5).tolist())
    assert found == {0, 1, 2, 3, 4}
    assert decoys >= 1
    assert all(totals[k] > 0 for k in ("sf_ok", "sf_fail", "rs_corr", "rs_fail", "fc_corr", "au_ok", "au_bad"))
