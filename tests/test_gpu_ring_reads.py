"""The output rings of the packet-mode and the PAD slots as a reader sees them (dabx_read_datagroups, dabx_read_pad_items): what is left for
a reader that comes late, and the argument paths of the two read calls -- n, max_bytes, bytes = NULL.  Built like
test_gpu_packet_stage.py / test_gpu_pad_stage.py: one stream, one slot, noise-free soft bits through dx.msc_inject / dx.msc_decode, every
result compared EXACTLY with the model of packet_cases.py / pad_cases.py and the rule of the rings (dabstar_amd/csrc/out_ring.h): an item is trusted
while its record is still in the record ring and n_bytes + the assembly room - byte_pos still fits the byte ring; of those a call returns
the newest n, and of these the longest newest run whose bytes fit max_bytes; what was never returned and is no longer intact is lost.

test_packet_cases.py proves on the model that the three late-reader scenarios overrun the rings the way each is meant to.  The PAD rings
(512 items, 128 KiB) cannot be overrun by a scenario of test size: the window code both stages run is the one the packet scenarios reach."""
import numpy as np
import pytest

import dabplus_cases as dc
import packet_cases as pkc
import pad_cases as pdc
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu

H, B = dc.HISTORY, dc.BATCH


def _run(layout, cifs, n_batches, switch_on):
    """One stream on an engine of its own: 16 CIFs of history, then n_batches full batches with NOTHING read in between."""
    eng = dx.Engine(n_streams=1, ring_frames=2, max_subch=len(layout), out_frames=1, msc_fast_min_jobs=1, msc_class_min_jobs=1)
    try:
        eng.set_subchannels(layout, stream=0)
        switch_on(eng)
        dx.msc_inject(eng, 0, cifs[:H])
        dx.msc_decode(eng, [H], H)
        for b in range(n_batches):
            dx.msc_inject(eng, 0, cifs[H + B * b:H + B * (b + 1)])
            dx.msc_decode(eng, [B], B)
    except BaseException:
        eng.close()
        raise
    return eng


def _expected(want, data, n, max_bytes=None, lo=0):
    """What a read call returns of the model's rows `want` (byte_pos counted from the slot's first byte) and bytes `data` when the items
    from `lo` on are intact: the newest n of those, of these the longest newest run that fits max_bytes; byte_pos counted from the first."""
    first = max(lo, len(want) - n)
    while max_bytes is not None and first < len(want) and len(data) - int(want["byte_pos"][first]) > max_bytes:
        first += 1
    rec = want[first:].copy()
    base = int(rec["byte_pos"][0]) if len(rec) else len(data)
    rec["byte_pos"] -= base
    return rec, data[base:]


def _same(got, want):
    return len(got[0]) == len(want[0]) and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


# ---- packet mode: a reader that comes late ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pkc.LATE_READER))
def test_a_late_reader_gets_exactly_the_groups_that_are_still_intact_and_the_rest_is_counted_lost(name):
    kbps, frames = pkc.late_reader_scenario(name)
    m = pkc.run_model(frames, pkc.ADDRESS_A)
    want, data = m.records(), m.all_bytes()
    n_rec, n_ring = pkc.ring_sizes(kbps)
    _, first = pkc.intact_window(want["byte_pos"], len(data), n_rec, n_ring)
    layout = dc.dabplus_layout([(kbps, pkc.PROT, 0)], dab_plus=[0])
    cifs = dc.cifs_of(layout, [frames], np.random.default_rng([21, kbps]))
    eng = _run(layout, cifs, pkc.N_BATCHES, lambda e: e.set_packet_mode(0, 0, pkc.ADDRESS_A))
    try:
        eng.subch = list(layout)
        last = eng.read_msc(0, 0, B)
        one = eng.read_datagroups(0, 0, 4096, max_bytes=dx.DG_RING_MAX_BYTES)
        st1 = eng.packet_stats(0, 0)
        two = eng.read_datagroups(0, 0, 4096, max_bytes=dx.DG_RING_MAX_BYTES)
        st2 = eng.packet_stats(0, 0)
    finally:
        eng.close()
    print(name, kbps, "groups", len(want), "bytes", len(data), "rings", n_rec, n_ring, "first intact", first, "returned", len(one[0]), "dg_lost", st1["dg_lost"])
    assert np.array_equal(last, frames[-B:])
    assert 0 < first < len(want)
    exp = _expected(want, data, 4096, lo=first)
    assert len(one[0]) == len(want) - first and one[0].tobytes() == exp[0].tobytes()
    assert np.array_equal(one[1], data[int(want["byte_pos"][first]):])
    assert st1["dg_lost"] == first, (st1, first)
    assert all(st1[k] == m.counters[k] for k in pkc.PACKET_COUNTERS), (st1, m.counters)
    assert _same(two, one) and st2 == st1, (st2, st1)


# ---- both stages: the argument paths ---------------------------------------------------------------------------------------------------------
def _argument_paths(read, read_records_only, lost, want, data):
    """read(n, max_bytes) -> (records, bytes); read_records_only(n) -> records, the C call with bytes = NULL; lost() -> the lost counter."""
    total = len(want)
    assert total > 12 and int(want["length"][-1]) > 0 and int(want["length"][-6:].sum()) > int(want["length"][-1])
    # n smaller than what is there: the newest n.  The older ones were behind the returned ones: a following full read still has them all
    assert _same(read(5, None), _expected(want, data, 5)) and lost() == 0
    full = read(total + 7, None)
    assert _same(full, _expected(want, data, total + 7)) and len(full[0]) == total and len(full[1]) == len(data) and lost() == 0
    # max_bytes one short of the newest six items' bytes, and of every shorter run's: the longest newest run that fits, from the model's lengths
    for k in (6, 3, 2):
        room = int(want["length"][-k:].sum()) - 1
        got, exp = read(k, room), _expected(want, data, k, room)
        assert _same(got, exp) and len(got[0]) < k and len(got[1]) <= room, (k, room, len(got[0]), len(exp[0]))
    # ... smaller than the newest item alone: nothing
    got = read(4, int(want["length"][-1]) - 1)
    assert len(got[0]) == 0 and len(got[1]) == 0
    # bytes = NULL: the same records, byte_pos counted from the first all the same, whatever max_bytes says
    for n in (total + 7, 5):
        assert read_records_only(n).tobytes() == _expected(want, data, n)[0].tobytes(), n
    assert lost() == 0


def _records_only(call, eng, dtype):
    def read(n):
        info = np.zeros(n, dtype)
        k = dx.check(call(eng._h, 0, 0, n, dx._p(info), None, 0))
        return info[:k]
    return read


def _packet_run():
    """(engine, model) behind the 64 kbit/s scenario() of packet_cases with nothing read."""
    kbps, seed = 64, pkc.seed_of(2, 1)
    frames = pkc.scenario(kbps, seed)
    m = pkc.run_model(frames, pkc.ADDRESS_A)
    assert pkc.intact_window(m.records()["byte_pos"], len(m.all_bytes()), *pkc.ring_sizes(kbps)) == (0, 0)          # nothing read, nothing overrun
    layout = dc.dabplus_layout([(kbps, pkc.PROT, 0)], dab_plus=[0])
    cifs = dc.cifs_of(layout, [frames], np.random.default_rng([22, kbps]))
    return _run(layout, cifs, pkc.N_BATCHES, lambda e: e.set_packet_mode(0, 0, pkc.ADDRESS_A)), m


def _pad_run():
    """(engine, model) behind the 64 kbit/s script of pad_cases with nothing read."""
    kbps, seed = 64, pdc.seed_of(0, 1)
    frames = pdc.scenario(kbps, seed)[0]
    layout = dc.dabplus_layout([(kbps, pdc.PROT, 0)], dab_plus=[1])
    cifs = dc.cifs_of(layout, [frames], np.random.default_rng([23, kbps]))
    o = dc.oracle_results(layout, cifs)[0]
    m = pdc.run_model(o["sf"], o["sfi"])
    assert pkc.intact_window(m.records()["byte_pos"], len(m.all_bytes()), 512, dx.PAD_RING_BYTES, asm_room=16896) == (0, 0)
    return _run(layout, cifs, pdc.N_BATCHES, lambda e: e.set_pad_mode(0, 0)), m


def test_read_datagroups_n_max_bytes_and_no_bytes_return_what_the_rule_says():
    eng, m = _packet_run()
    try:
        _argument_paths(lambda n, mb: eng.read_datagroups(0, 0, n, max_bytes=mb), _records_only(dx.load().dabx_read_datagroups, eng, dx.DATAGROUP_INFO),
                        lambda: eng.packet_stats(0, 0)["dg_lost"], m.records(), m.all_bytes())
        st = eng.packet_stats(0, 0)
    finally:
        eng.close()
    assert all(st[k] == m.counters[k] for k in pkc.PACKET_COUNTERS), (st, m.counters)


def test_read_pad_items_n_max_bytes_and_no_bytes_return_what_the_rule_says():
    eng, m = _pad_run()
    try:
        _argument_paths(lambda n, mb: eng.read_pad_items(0, 0, n, max_bytes=mb), _records_only(dx.load().dabx_read_pad_items, eng, dx.PAD_ITEM),
                        lambda: eng.pad_stats(0, 0)["items_lost"], m.records(), m.all_bytes())
        st = eng.pad_stats(0, 0)
    finally:
        eng.close()
    assert all(st[k] == m.counters[k] for k in pdc.PAD_COUNTERS), (st, m.counters)


def test_the_python_readers_return_the_records_alone_on_request():
    """Engine.read_datagroups / read_pad_items with with_bytes = False (bytes = NULL in the C call): every record, no bytes, nothing lost."""
    for run, read, lost in ((_packet_run, lambda e: e.read_datagroups(0, 0, 4096, with_bytes=False), lambda e: e.packet_stats(0, 0)["dg_lost"]),
                            (_pad_run, lambda e: e.read_pad_items(0, 0, 512, with_bytes=False), lambda e: e.pad_stats(0, 0)["items_lost"])):
        eng, m = run()
        try:
            rec, by = read(eng)
            n_lost = lost(eng)
        finally:
            eng.close()
        assert rec.tobytes() == m.records().tobytes() and len(by) == 0 and n_lost == 0
