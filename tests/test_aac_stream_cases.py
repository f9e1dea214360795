"""No device.  The model of tests/aac_stream_cases.py and its scenarios: the scenarios reach every cited branch and every L / 255 value in
both SBR modes; a LOAS parser written for this test recovers every access unit from the model's output; the frame sizes and the two hex
strings of the format; the kernel's own header and copy pieces (aac_core.h, run lane after lane on the host through
dabx_internal_aac_frame_host) give the model's bytes for every L and every parameter combination; each single-line mutation of the model
changes its output; the in-order byte bound."""
import numpy as np
import pytest

import aac_stream_cases as ac
import dabplus_cases as dc
from dabstar_amd import lib as dx

_models = {}


def _all():
    """[(kbps, facts, super frames, records, model)] of every scenario of the stage test, computed once."""
    if not _models:
        rows = []
        for kbps, facts in ac.all_scenarios():
            sfs, sfis = ac.accepted(facts, kbps)
            rows.append((kbps, facts, sfs, sfis, ac.run_model(sfs, sfis)))
        _models["all"] = rows
    return _models["all"]


def test_the_records_of_info_of_pass_the_check_a_host_relies_on():
    """info_of is the test's stand-in for k_dabplus's record: it passes the independent check of tests/dabplus_cases.py on every accepted
    super frame (the GPU tests take the records of the oracle back end and of the device instead)."""
    for kbps, facts, sfs, sfis, m in _all():
        for sf, r in zip(sfs, sfis):
            dc._check_record_against_its_super_frame(r, sf, kbps)


def test_the_oracles_super_frames_are_the_scenarios_accepted_ones():
    """What k_aac_stream is given in the GPU tests: the oracle back end (oracle/msc.c), fed the coded soft bits of the stage test's four
    streams, accepts exactly the super frames the scenarios mean to be accepted and fills their records as info_of does, so the models of
    the GPU tests (on the oracle's super frames and records) are the models this file examines."""
    for s in range(len(ac.STAGE_STREAMS)):
        case = ac.stream_case(s)
        for j, (kbps, kind) in enumerate(ac.kinds(s)):
            if kind != "aac":
                continue
            sfs, sfis = ac.accepted(ac.scenario(kbps, ac.seed_of(s, j), (s, j) in ac.OVERLAP_SLOTS)[1], kbps)
            o = case[3][j]
            assert np.array_equal(o["sf"], np.stack(sfs)), (s, j)
            for a, b in zip(o["sfi"], sfis):
                assert all(a[k].tobytes() == b[k].tobytes() for k in ("num_aus", "au_crc_ok", "au_len_bad", "stream_parms", "au_start", "first_frame")), (s, j, a, b)


def test_the_scenarios_reach_every_branch_every_length_byte_count_and_every_parameter_combination():
    rows = _all()
    assert sorted(kbps for kbps, *_ in rows) == [8, 8, 32, 32, 64, 64, 72, 72, 192, 192, 384, 384]
    lines, seen_L, combos, n_aus, neg, over = set(), set(), set(), set(), 0, 0
    for kbps, facts, sfs, sfis, m in rows:
        lines |= m.lines
        rec = m.records()
        assert sum(1 for _, _, ok in facts["sf"] if not ok) >= 2 and len(sfs) == m.counters["superframes"]      # rejected super frames: nothing of them
        for r in rec:
            sbr = (int(r["stream_parms"]) >> 5) & 1
            if r["flags"] == 0:
                seen_L.add((int(r["au_len"]), sbr))
                combos.add(int(r["stream_parms"]) >> 4)
            n_aus.add(int(r["num_aus"]))
            if r["flags"] == ac.LOST_LEN:
                L = int(r["au_len"]) - (65536 if r["au_len"] >= 32768 else 0)
                neg += L < 0
                over += L == 961
        assert len({int(r["stream_parms"]) & 0x0F for r in rec}) > 8             # psFlag / mpegSurround vary
    assert lines == {325, 333, 377}
    assert n_aus == {2, 3, 4, 6} and combos == set(range(8))
    assert neg > 0 and over > 0
    for sbr in (0, 1):
        assert {L for L, s in seen_L if s == sbr} >= set(ac.EDGE_L), (sbr, sorted(set(ac.EDGE_L) - {L for L, s in seen_L if s == sbr}))
        assert {L // 255 for L, s in seen_L if s == sbr} == {0, 1, 2, 3}


def test_an_independent_parser_recovers_every_access_unit_and_its_parameters():
    for kbps, facts, sfs, sfis, m in _all():
        parsed = ac.parse_loas(m.all_bytes())
        good = [(sf, r, a) for sf, r in zip(sfs, sfis) for a in range(int(r["num_aus"])) if (int(r["au_crc_ok"]) & ~int(r["au_len_bad"])) >> a & 1]
        assert len(parsed) == len(good) == m.counters["frames"]
        for (p, payload), (sf, r, a) in zip(parsed, good):
            st, L = int(r["au_start"][a]), int(r["au_start"][a + 1]) - int(r["au_start"][a]) - 2
            assert payload == bytes(sf[st:st + L])
            dac, sbr, ch = int(r["stream_parms"]) >> 6 & 1, int(r["stream_parms"]) >> 5 & 1, int(r["stream_parms"]) >> 4 & 1
            assert p == {"sr": {(0, 0): 5, (0, 1): 8, (1, 0): 3, (1, 1): 6}[(dac, sbr)], "ch": 2 if ch else 1, "sbr": sbr, "ext": ({0: 5, 1: 3}[dac] if sbr else None)}
        # the records slice the stream
        rec, by = m.records(), m.all_bytes()
        at = 0
        for r in rec:
            assert r["byte_pos"] == at and (r["length"] > 0) == (r["flags"] == 0)
            at += int(r["length"])
        assert at == len(by)


def test_frame_sizes_and_the_two_frames_of_the_format():
    for parms, want in ((0x50, "56e007200011941fe000"), (0x70, "56e00820002b118a0ff000")):
        sp = ac.stream_parameters(parms)
        assert ac.build_aac_stream(0, sp, b"").hex() == want
        assert dx.aac_frame_host(np.zeros(0, np.uint8), parms).tobytes().hex() == want
    rng = np.random.default_rng(5)
    for sbr in (0, 1):
        for L in range(0, 961):
            data = rng.integers(0, 256, L).astype(np.uint8)
            f = ac.build_aac_stream(L, ac.stream_parameters(0x40 | sbr << 5), data)
            assert len(f) == (11 if sbr else 10) + L // 255 + L
            assert f[-1] & (3 if sbr else 7) == 0                      # the last byte's zero bits
            assert (f[1] & 0x1F) << 8 | f[2] == len(f) - 3
            # the payload is the input shifted right by 6 / 5 bits
            s = 6 if sbr else 5
            tail = np.unpackbits(np.frombuffer(f, np.uint8))[8 * (len(f) - L - 1) + s:8 * len(f) - (8 - s)]
            assert np.array_equal(np.packbits(tail), data)


def test_the_kernels_pieces_on_the_host_equal_the_model_for_every_length_and_parameter_combination():
    """dabx_internal_aac_frame_host runs aac_core.h's functions -- the header template, the length bytes, the shifted copy -- byte after
    byte as k_aac_stream's lanes do: for every L in 0 .. 960 and all eight (dac, sbr, channel) combinations, psFlag and mpegSurround at
    random, on random payloads (0xFF and 0x00 runs among them) the bytes are the model's."""
    rng = np.random.default_rng(11)
    n = 0
    for L in range(0, 961):
        for combo in range(8):
            parms = combo << 4 | int(rng.integers(0, 16))
            data = rng.integers(0, 256, L).astype(np.uint8)
            if L and combo == L % 8:
                data[:] = 0xFF if L % 2 else 0x00
            want = ac.build_aac_stream(L, ac.stream_parameters(parms), data)
            got = dx.aac_frame_host(data, parms)
            assert got.tobytes() == want, (L, parms)
            n += 1
    assert n == 961 * 8
    L = dx.load()
    out = np.zeros(dx.AAC_MAX_FRAME_BYTES, np.uint8)
    for bad in ((961, 0), (-1, 0), (0, 0x80), (0, -1)):
        assert L.dabx_internal_aac_frame_host(out.ctypes.data, bad[0], bad[1], out.ctypes.data) == -2


@pytest.mark.parametrize("mut", ac.MUTATIONS)
def test_every_single_line_mutation_of_the_model_changes_its_output(mut):
    """shift 5 <-> 6 (the branch of :412), L % 255 -> L % 256 (:439), size - 3 -> size (bit_writer.cpp:56), the CoreSrIndex table (:266)."""
    for kbps, facts, sfs, sfis, m in _all():
        w = ac.run_model(sfs, sfis, mut=(mut,))
        assert w.records()["flags"].tobytes() == m.records()["flags"].tobytes()
        # (L % 255 and L % 256 differ from L = 255 on: a super frame of 110 bytes holds no such access unit)
        assert (w.all_bytes().tobytes() != m.all_bytes().tobytes()) == (mut != "mod256" or kbps > 8), (mut, kbps)


def test_the_in_order_byte_bound_holds_and_the_overlapping_super_frame_exceeds_it():
    n_over = 0
    for kbps, facts, sfs, sfis, m in _all():
        bound = 110 * (kbps // 8) + 72
        idx = [i for i, (_, _, ok) in enumerate(facts["sf"]) if ok]
        for k, (r, emitted) in enumerate(zip(sfis, m.sf_bytes)):
            st = [int(v) for v in r["au_start"][:int(r["num_aus"]) + 1]]
            in_order = all(b >= a for a, b in zip(st, st[1:]))
            if facts["overlap"] is not None and idx[k] == facts["overlap"]:
                assert not in_order and emitted > bound and int(r["au_crc_ok"]) == 0b101 and int(r["au_len_bad"]) == 0b010, (kbps, st, emitted)
                n_over += 1
                # a batch that holds it still fits the byte ring (the newest six super frames around it)
                assert max(sum(m.sf_bytes[i:i + 6]) for i in range(max(0, k - 5), k + 1)) + dx.AAC_MAX_FRAME_BYTES <= dx.aac_ring_bytes(kbps)
            elif in_order:
                assert emitted <= bound, (kbps, st, emitted)
        assert 2 * 6 * bound <= dx.aac_ring_bytes(kbps) < 4 * 6 * bound
    assert n_over == 2
