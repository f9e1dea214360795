"""The comparisons of tests/stage_driver.py are what fails a test of the MSC slot stages, and they run only behind a device.  Here, without
one: fed what a perfect device would have produced -- frames, super frames and records from the cases' oracle results, items, bytes and
counters from the models -- each returns no line; with one thing wrong at a time each returns at least one, and every line names the stream,
the slot, the bit rate and the kind.  The first stream of packet_cases, pad_cases and mp2_pad_cases (cached there for test_*_cases.py)."""
import copy

import numpy as np
import pytest

import mp2_pad_cases as mc
import packet_cases as pkc
import pad_cases as pc
import stage_driver as sd

B = sd.B


def _oracle_part(o):
    stats = {mine: o["stats"][theirs] for mine, theirs in sd.SF_COUNTERS}
    return {"frames": o["frames"], "sf": o["sf"], "sfi": o["sfi"], "stats": dict(stats, sf_count=len(o["sfi"]))}


def _ring_part(g, model, counters, **fixed):
    """The items, bytes and counters of `model`, or of a slot whose mode is off (None): nothing, and all-zero stats."""
    if model is None:
        g.update(rec=np.zeros(0, np.uint8), bytes=np.zeros(0, np.uint8), pstats=dict.fromkeys(list(counters) + list(fixed), 0))
    else:
        g.update(rec=model.records(), bytes=model.all_bytes(), pstats=dict({k: model.counters[k] for k in counters}, **fixed))
    return g


def _packet():
    case = pkc.stream_case(0)
    lay, address = pkc.STAGE_STREAMS[0]
    got = {}
    for j, (kbps, kind) in enumerate(pkc.STAGE_LAYOUTS[lay]):
        m = pkc.run_model(case[1][j], address) if kind == "pkt" else None
        got[(0, j)] = _ring_part(_oracle_part(case[3][j]), m, pkc.PACKET_COUNTERS, dg_lost=0, active=1, packet_address=address)
    return got, pkc.STAGE_LAYOUTS[lay], lambda g: sd.packet_mismatches(g, [case], [0]), ("pkt",), pkc.PACKET_COUNTERS, "dg_lost"


def _pad():
    case = pc.stream_case(0)
    got = {}
    for j, (kbps, kind) in enumerate(pc.STAGE_LAYOUTS[pc.STAGE_STREAMS[0]]):
        o = case[3][j]
        m = pc.run_model(o["sf"], o["sfi"]) if kind == "pad" else None
        got[(0, j)] = _ring_part(_oracle_part(o), m, pc.PAD_COUNTERS, items_lost=0, active=1)
    return got, pc.STAGE_LAYOUTS[pc.STAGE_STREAMS[0]], lambda g: sd.pad_mismatches(g, [case], [0]), ("pad",), pc.PAD_COUNTERS, "items_lost"


def _mp2():
    """The MP2 file's whole-run comparison: the MP2 slots' items are the MP2 model's, the DAB+ PAD slot's those of pad_cases' model."""
    case = mc.stream_case(0)
    got = {}
    for j, (kbps, kind) in enumerate(mc.kinds(0)):
        o = case[3][j]
        m = mc.slot_model(0, j) if kind == "mp2" else pc.run_model(o["sf"], o["sfi"]) if kind == "pad" else None
        g = _ring_part(_oracle_part(o), m.pad if kind == "mp2" else m, pc.PAD_COUNTERS, items_lost=0, active=1)
        g["sync"] = m.sync_stats() if kind == "mp2" else dict.fromkeys(mc.SYNC_FIELDS, 0)
        got[(0, j)] = g
    return got, mc.kinds(0), lambda g: sd.mp2_final_mismatches(g, [case], [0]), ("mp2", "pad"), pc.PAD_COUNTERS, "items_lost"


_FILES = {"packet": _packet, "pad": _pad, "mp2": _mp2}


def _tampered(got, key, field, change):
    g = copy.deepcopy(got)
    value = g[key][field]
    g[key][field] = change(value.copy() if isinstance(value, np.ndarray) else dict(value))
    return g


def _flip(at):
    def change(a):
        a.reshape(-1)[at] ^= 1
        return a
    return change


def _bump(field, to=None):
    def change(a):
        a[field] = to if to is not None else a[field] + 1
        return a
    return change


def _record_field(row, field):
    def change(a):
        a[field][row] += 1
        return a
    return change


@pytest.mark.parametrize("which", sorted(_FILES))
def test_a_perfect_device_gives_no_line_and_every_single_fault_gives_one_that_names_its_slot(which):
    got, kinds, mismatches, followed, counters, lost = _FILES[which]()
    assert mismatches(got) == []
    rings = [next(j for j, (_, k) in enumerate(kinds) if k == kind and len(got[(0, j)]["rec"]) > 1) for kind in followed]      # a slot of every kind whose ring the file follows
    dabplus = next(j for j in range(len(kinds)) if len(got[(0, j)]["sfi"]))       # a slot with super frames
    off = next(j for j, (_, k) in enumerate(kinds) if k in ("plain", "dab+", "pkt") and k not in followed)
    assert not len(got[(0, off)]["rec"])
    faults = [("a byte of a super frame", dabplus, "sf", _flip(-7)), ("a field of a super-frame record", dabplus, "sfi", _record_field(0, "first_frame"))]
    faults += [("counter " + k, dabplus, "stats", _bump(k)) for k, _ in sd.SF_COUNTERS]
    for ring in rings:
        faults += [("a byte of a logical frame", ring, "frames", _flip(100)),
                   ("a byte of an item's payload", ring, "bytes", _flip(len(got[(0, ring)]["bytes"]) // 2)),
                   ("a field of an item record", ring, "rec", _record_field(1, "length")),
                   ("the lost count", ring, "pstats", _bump(lost, 1))]
        faults += [("counter " + k, ring, "pstats", _bump(k)) for k in counters]
    for what, j, field, change in faults:
        bad = mismatches(_tampered(got, (0, j), field, change))
        tag = "stream 0 slot %d (%d kbit/s, %s): " % (j, kinds[j][0], kinds[j][1])
        assert bad and all(line.startswith(tag) for line in bad), (what, tag, bad)
    # a slot whose mode is off shows one record
    shows = _tampered(got, (0, off), "rec", lambda a: np.zeros(1, got[(0, rings[0])]["rec"].dtype))
    bad = mismatches(shows)
    assert len(bad) == 1 and bad[0].startswith("stream 0 slot %d (%d kbit/s, %s): " % ((off,) + tuple(kinds[off]))) and " and shows " in bad[0], bad


def test_the_mp2_slots_comparison_after_every_batch_notices_every_single_fault():
    """stage_driver.mp2_batch_mismatches on what a follower would have taken from a perfect device after every batch of 28 frames, then
    with one counter, one sync field, the lost count, one record field and one byte wrong."""
    j, kbps = next((j, kbps) for j, (kbps, kind) in enumerate(mc.kinds(0)) if kind == "mp2" and kbps >= 48)
    m = mc.slot_model(0, j)
    tag = "stream 0 slot %d (%d kbit/s, mp2): " % (j, kbps)
    first = first_byte = 0
    tampered = 0
    for n in range(B, mc.N_FRAMES + 1, B):
        items, n_bytes, counters, sync = m.snaps[n]
        st = dict({k: counters[k] for k in pc.PAD_COUNTERS}, items_lost=0, active=1)
        rec = m.pad.records()[first:items].copy() if items > first else None
        by = m.pad.all_bytes()[first_byte:n_bytes].copy()
        sy = {k: sync[k] for k in mc.SYNC_FIELDS}
        assert sd.mp2_batch_mismatches(tag, m, n, (st, rec, by, first, first_byte), sy) == []
        faults = [(dict(st, **{k: st[k] + 1}), rec, by, sy) for k in pc.PAD_COUNTERS]
        faults += [(st, rec, by, dict(sy, **{k: sy[k] + 1})) for k in mc.SYNC_FIELDS]
        faults += [(dict(st, items_lost=1), rec, by, sy), (dict(st, active=0), rec, by, sy)]
        if rec is not None and len(by):
            wrong, wrong_byte = rec.copy(), by.copy()
            wrong["frame"][-1] += 1
            wrong_byte[len(by) // 2] ^= 1 << (n % 8)
            faults += [(st, wrong, by, sy), (st, rec, wrong_byte, sy), (st, rec[:-1], by, sy), (st, rec, by[:-1], sy)]
        for f_st, f_rec, f_by, f_sy in faults:
            bad = sd.mp2_batch_mismatches(tag, m, n, (f_st, f_rec, f_by, first, first_byte), f_sy)
            assert bad and all(line.startswith(tag + "after %d frames " % n) for line in bad), (n, bad)
        tampered += len(faults)
        first, first_byte = items, n_bytes
    assert first == len(m.pad.rows) > 0 and tampered > mc.N_BATCHES * (len(pc.PAD_COUNTERS) + len(mc.SYNC_FIELDS) + 2)      # some batches had items


def test_the_follower_rebases_and_bounds_what_it_takes():
    """stage_driver.Follower on a stand-in for the engine that serves a model's ring batch by batch: result() is the model's whole
    sequence; a batch with more new items than the bound, a reader that returns fewer than the counters say, and bytes that do not add up
    each stop it."""
    m = pc.slot_model(0, 1)
    rows, data = m.records(), m.all_bytes()
    assert len(rows) > 8

    class Served:
        def __init__(self, short=0, cut=0):
            self.n, self.short, self.cut = 0, short, cut

        def pad_stats(self, i, j):
            end = int(rows["byte_pos"][self.n - 1]) + int(rows["length"][self.n - 1]) if self.n else 0
            return dict(labels=self.n, groups=0, label_bytes=end, group_bytes=0)

        def read_pad_items(self, i, j, n, max_bytes=None):
            r = rows[self.n - n + self.short:self.n].copy()
            lo, hi = int(r["byte_pos"][0]), int(r["byte_pos"][-1]) + int(r["length"][-1])
            r["byte_pos"] -= lo
            return r, data[lo:hi - self.cut]

    eng, f = Served(), sd.Follower(sd.PAD_ITEMS, 4)
    for n in list(range(0, len(rows), 3)) + [len(rows), len(rows)]:
        eng.n = n
        st, rec, by, first, first_byte = f.take(eng, 0, 1)
        assert (rec is None) == (n == first) and f.seen == n
    rec, by = f.result()
    assert rec.tobytes() == rows.tobytes() and np.array_equal(by, data)
    for eng, bound in ((Served(), 4), (Served(short=1), 8), (Served(cut=1), 8)):
        eng.n = 5
        with pytest.raises(AssertionError):
            sd.Follower(sd.PAD_ITEMS, bound).take(eng, 0, 1)
