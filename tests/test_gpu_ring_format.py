"""GPU: an engine whose IQ ring keeps the recording's own codes (dabx_create_ex, DABX_RING_S16 / DABX_RING_U8) computes, bit for
bit, what a cf32 engine computes that is fed the same codes (which expands them on ingest), and what the oracle receiver computes
on the values those codes stand for.  Every comparison here is for equality: both maps -- c / 32768 and (c - 127.38) / 128 -- are
exact in float, so there is nothing to tolerate."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

import oracle_lib as ol
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from tools import iq_files as iqf  # noqa: E402

pytestmark = pytest.mark.gpu
TF = ds.TF
KINDS = ["s16", "u8"]
DTYPE = {"s16": np.int16, "u8": np.uint8}


def quantise(x, kind, gain):
    """interleaved I, Q codes of the recording a front end of that sample type would have made"""
    return iqf.to_u8(x, gain) if kind == "u8" else iqf.to_int(x, 16, gain).astype(np.int16)


def values(codes, kind):
    """what the codes stand for: the reference's maps (raw_reader.cpp:66-70, wav_reader.cpp:164), in numpy float32"""
    c = codes.astype(np.float32)
    v = (c - np.float32(127.38)) / np.float32(128) if kind == "u8" else c / np.float32(32768)
    return np.ascontiguousarray(v).view(np.complex64)


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0] if isinstance(v, float) else v


def stats_bits(st):
    return {k: bits(v) for k, v in st.items()}


def oracle_run(x, subch):
    L = ol.oracle()
    rx = L.ora_rx_create(ol.make_descs(subch), len(subch))
    L.ora_rx_enable_soft_capture(rx, 0)
    n = L.ora_rx_run(rx, x, len(x), 10000)
    cap = L.ora_rx_get_capture(rx).contents
    res = dict(n=n, fibs=np.ctypeslib.as_array(cap.fibs, (n, 12, 32)).copy(), crc=np.ctypeslib.as_array(cap.fib_crc, (n, 12)).copy(),
               start=np.ctypeslib.as_array(cap.start_idx, (n,)).copy(),
               msc=[ol.backend_bytes(rx, i, "msc") for i in range(len(subch))], sf=[ol.backend_bytes(rx, i, "sf") for i in range(len(subch))])
    L.ora_rx_destroy(rx)
    return res


def walk(codes, subch, ring_format, **kw):
    """One ensemble, all of it in the ring, one step at a time: everything the engine reports after every frame, and everything it holds
    at the end."""
    n = len(codes) // 2
    eng = dx.Engine(n_streams=1, ring_frames=n // TF + 1, max_subch=max(1, len(subch)), out_frames=4, ring_format=ring_format, **kw)
    if subch:
        eng.set_subchannels(subch)
    eng.set_lcd_statistics(1)
    eng.push_iq(0, codes)
    r = dict(fibs=[], crc=[], start=[], level=[], peak=[], stats=[], info=[])
    idle, steps = 0, 0
    while idle < 4 and steps < 400:
        before = eng.stats(0)
        eng.process(1)
        st = eng.stats(0)
        steps += 1
        idle = idle + 1 if st["samples_consumed"] == before["samples_consumed"] else 0
        if st["frames"] > before["frames"]:
            f, c = eng.read_fibs(0, 1)
            r["fibs"].append(f[0]); r["crc"].append(c[0]); r["start"].append(st["last_start_index"])
            r["level"].append(bits(st["signal_level"])); r["peak"].append(bits(st["peak_level"]))
            r["stats"].append(stats_bits(st))
            r["info"].append(tuple(np.asarray(a).tolist() for a in eng.read_frame_info(0, 1)))
    r["final"] = stats_bits(eng.stats(0))
    r["counters"] = eng.counters()
    if kw.get("capture_soft"):
        r["soft"] = eng.read_soft(0)
    r["msc"] = [eng.read_msc(0, j, 32) for j in range(len(subch))]
    r["sf"] = [eng.read_superframes(0, j, 4) for j in range(len(subch))]
    r["sfi"] = [eng.read_superframe_info(0, j, 4).tobytes() for j in range(len(subch))]
    r["sub"] = [eng.subch_stats(0, j) for j in range(len(subch))]
    for k in ("fibs", "crc", "start"):
        r[k] = np.array(r[k])
    eng.close()
    return r


def same_walk(a, b):
    """native engine == cf32 engine: every frame, every field"""
    assert len(a["fibs"]) == len(b["fibs"])
    for k in ("fibs", "crc", "start"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("level", "peak", "stats", "info", "final", "counters", "sfi", "sub"):
        assert a[k] == b[k], k
    for k in ("msc", "sf"):
        assert len(a[k]) == len(b[k]) and all(np.array_equal(p, q) for p, q in zip(a[k], b[k])), k
    if "soft" in a:
        assert np.array_equal(a["soft"], b["soft"])


# ------------------------------------------------------------------------------------------------------ 1. ring contents
@pytest.mark.parametrize("kind", KINDS)
def test_ring_contents_are_the_codes_and_read_back_as_their_values(kind):
    rng = np.random.default_rng(3)
    n = 3 * TF + 12345
    if kind == "u8":
        codes = rng.integers(0, 256, 2 * n).astype(np.uint8)
        codes[:256] = np.arange(256)                              # every value
    else:
        codes = rng.integers(-32768, 32768, 2 * n).astype(np.int16)
        codes[:4] = [-32768, 32767, 32767, -32768]
    want = values(codes, kind)
    nat = dx.Engine(n_streams=2, ring_frames=2, max_subch=0, fic_only=1, ring_format=kind)
    ref = dx.Engine(n_streams=2, ring_frames=2, max_subch=0, fic_only=1)
    assert nat.ring_format() == ({"s16": 1, "u8": 2}[kind], {"s16": 4, "u8": 2}[kind]) and ref.ring_format() == (0, 8)
    pos, piece, wrapped = 0, 50001, False
    while pos < n:
        m = min(piece, n - pos)
        for e in (nat, ref):
            for attempt in range(20):                            # the search reads the (noise) samples away: room for the next piece
                try:
                    e.push_iq(1, codes[2 * pos:2 * (pos + m)])
                    break
                except dx.DabxError:
                    e.process(1)
            else:
                raise AssertionError("no room in the ring")
        a, b = nat.read_iq(1, pos, m), ref.read_iq(1, pos, m)
        assert np.array_equal(a.view(np.uint32), want[pos:pos + m].view(np.uint32)), pos
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), pos
        wrapped = wrapped or (pos // (2 * TF) != (pos + m - 1) // (2 * TF))
        pos += m
        piece += 1002                                             # odd and even piece sizes
    assert wrapped and pos > 2 * TF
    back = min(n, 2 * TF) - 7                                     # and the newest ring's worth at once, across the wrap
    assert np.array_equal(nat.read_iq(1, n - back, back).view(np.uint32), want[n - back:].view(np.uint32))
    nat.close(); ref.close()


# ------------------------------------------------------------------------------------------------------ 2. one ensemble, whole path
_CASE2 = {}


def _case2(kind):
    if kind not in _CASE2:
        subch = ds.default_subchannels(18, 64)
        ens = ds.build_ensemble(10, subch, seed=55)
        x = ds.channel(ens.iq, snr_db=14.0, cfo_hz=-640.0, timing_offset=41000, seed=12, n_out=16 * TF)
        g = 0.25 / np.sqrt(np.mean(np.abs(x) ** 2))
        _CASE2[kind] = (subch, ens, x, g, quantise(x, kind, g))
    return _CASE2[kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("soft_bit_type,tie", [(1, 0), (2, 0), (3, 0), (1, 1), (1, 2), (2, 1), (3, 2)])
def test_whole_path_equals_the_cf32_engine_and_the_oracle(kind, soft_bit_type, tie):
    subch, ens, _, _, codes = _case2(kind)
    kw = dict(soft_bit_type=soft_bit_type, viterbi_tie_mode=tie, capture_soft=True)
    nat, ref = walk(codes, subch, kind, **kw), walk(codes, subch, 0, **kw)
    same_walk(nat, ref)
    assert len(nat["fibs"]) >= 13
    if (soft_bit_type, tie) != (1, 0):
        return
    ora = oracle_run(values(codes, kind), subch)
    k = len(nat["fibs"])
    assert ora["n"] - 1 <= k <= ora["n"]
    assert np.array_equal(nat["crc"], ora["crc"][:k]) and np.array_equal(nat["fibs"], ora["fibs"][:k])
    assert ora["crc"][6:k].all() and np.array_equal(nat["start"], ora["start"][:k])
    n_lf = 4 * k - 16
    for j in range(len(subch)):
        assert nat["sub"][j]["cifs_decoded"] == n_lf
        m = min(n_lf, 32)
        assert np.array_equal(nat["msc"][j], ora["msc"][j].reshape(-1, 192)[n_lf - m:n_lf]), j
        ok = nat["sub"][j]["sf_ok"]
        q = min(4, ok)
        assert ok >= 5 and np.array_equal(nat["sf"][j], ora["sf"][j].reshape(-1, 880)[ok - q:ok]), j
        assert any(np.array_equal(nat["sf"][j][-1], t) for t in ens.superframes[j])


# ------------------------------------------------------------------------------------------------------ 3. losing and finding the lock
_CASE3 = {}


def _case3(kind, gap_kind):
    key = (kind, gap_kind)
    if key not in _CASE3:
        subch = ds.default_subchannels(18, 64)
        ens = ds.build_ensemble(10, subch, seed=71)
        x = ds.channel(ens.iq, snr_db=18.0, cfo_hz=-1333.0, timing_offset=5555, seed=7, n_out=34 * TF).copy()
        g = 0.25 / np.sqrt(np.mean(np.abs(x) ** 2))                # (of the signal before the gap goes in: the recorder's gain does not know of it)
        rng = np.random.default_rng(5)
        a, b = int(11.3 * TF), int(13.1 * TF)
        if gap_kind == "silence":
            x[a:b] = 0                                            # (code 127 in a u8 recording: -0.003 after the map, not zero)
        elif gap_kind == "noise":
            x[a:b] = ((rng.standard_normal(b - a) + 1j * rng.standard_normal(b - a)) * 0.2).astype(np.complex64)
        else:
            x = np.concatenate([x[:a], x[a + int(0.37 * TF):]])
        codes = quantise(x, kind, g)
        _CASE3[key] = (subch, codes, oracle_run(values(codes, kind), subch))
    return _CASE3[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("exact_level_tracker", [0, 1, 2])
@pytest.mark.parametrize("acquire_mode", [1, 2])
@pytest.mark.parametrize("gap_kind", ["silence", "noise", "shifted"])
def test_loss_of_lock_and_reacquisition_equal_the_cf32_engine_and_the_oracle(kind, gap_kind, acquire_mode, exact_level_tracker):
    subch, codes, ora = _case3(kind, gap_kind)
    kw = dict(acquire_mode=acquire_mode, exact_level_tracker=exact_level_tracker)
    nat, ref = walk(codes, subch, kind, **kw), walk(codes, subch, 0, **kw)
    same_walk(nat, ref)                                           # start indices, FIBs, CRCs, level bit patterns, level_*_events, sync_lost: every frame
    assert nat["counters"]["sync_lost"] >= 1
    n = min(len(nat["fibs"]), ora["n"])
    print(kind, gap_kind, acquire_mode, exact_level_tracker, "frames", len(nat["fibs"]), "oracle", ora["n"], "failed CRC frames", int((~ora["crc"][:n].all(axis=1)).sum()))
    assert n >= ora["n"] - 1 and n >= 24
    assert np.array_equal(nat["start"][:n].astype(int), ora["start"][:n].astype(int))
    assert np.array_equal(nat["crc"][:n], ora["crc"][:n]) and np.array_equal(nat["fibs"][:n], ora["fibs"][:n])
    assert nat["crc"][n - 6:n].all() and not nat["crc"][:n].all()


# ------------------------------------------------------------------------------------------------------ 4. many streams, fast MSC path, bulk ingest
@pytest.mark.parametrize("kind", KINDS)
def test_many_streams_bulk_ingest_and_pushes_equal_the_cf32_engine(kind):
    S, chunk, n_chunks = 64, 3, 4
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=91)
    x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=210.0, timing_offset=3001, seed=9, n_out=(chunk * n_chunks + 1) * TF)
    g = 0.25 / np.sqrt(np.mean(np.abs(x) ** 2))
    codes = quantise(x, kind, g)
    offs = [17 * s + (s % 3) for s in range(S)]                   # odd and even: symbol starts on every alignment of a 2- or 4-byte element
    assert {o % 2 for o in offs} == {0, 1} and {o % 4 for o in offs} == {0, 1, 2, 3}
    n = chunk * n_chunks * TF
    xs = [codes[2 * o:2 * (o + n)] for o in offs]
    per = 2 * chunk * TF
    mk = lambda rf: dx.Engine(n_streams=S, ring_frames=3 * chunk, max_subch=18, out_frames=8, msc_fast_min_jobs=1, ring_format=rf)   # noqa: E731
    engines = {"ingest0": mk(kind), "ingest1": mk(kind), "push": mk(kind), "cf32": mk(0)}
    for e in engines.values():
        e.set_subchannels(subch)
    slabs = {k: engines[k].ingest_open(DTYPE[kind], slabs=2, max_frames=chunk, copy_engine=int(k[-1])) for k in ("ingest0", "ingest1")}
    for c in range(n_chunks):
        for k in ("ingest0", "ingest1"):
            for s in range(S):
                slabs[k][c % 2][s * per:(s + 1) * per] = xs[s][c * per:(c + 1) * per]
            engines[k].ingest_submit(c % 2, chunk * TF)
            engines[k].ingest_commit(c % 2)
            engines[k].process(chunk, sync=False)
        for k in ("push", "cf32"):
            for s in range(S):
                engines[k].push_iq(s, xs[s][c * per:(c + 1) * per])
            engines[k].process(chunk, sync=False)
    for e in engines.values():
        e.process(2)
    ref = engines["cf32"]
    cr = ref.counters()
    assert cr["frames"] >= S * (chunk * n_chunks - 2) and cr["sf_ok"] > 0 and cr["sf_fail"] == 0
    fr = [ref.read_fibs(s, 8) for s in range(S)]
    for k in ("ingest0", "ingest1", "push"):
        e = engines[k]
        assert e.counters() == cr, k
        for s in range(S):
            f, c = e.read_fibs(s, 8)
            assert np.array_equal(f, fr[s][0]) and np.array_equal(c, fr[s][1]), (k, s)
            assert stats_bits(e.stats(s)) == stats_bits(ref.stats(s)), (k, s)
    for s in range(S):
        for j in range(18):
            m, q = ref.read_msc(s, j, 8), ref.read_superframes(s, j, 2)
            for k in ("ingest0", "ingest1", "push"):
                assert np.array_equal(engines[k].read_msc(s, j, 8), m) and np.array_equal(engines[k].read_superframes(s, j, 2), q), (k, s, j)
    for k in ("ingest0", "ingest1"):
        engines[k].ingest_close()
    for e in engines.values():
        e.close()


@pytest.mark.parametrize("kind", KINDS)
def test_bulk_delivery_slabs_equal_the_cf32_engines(kind):
    """Chunk for chunk: FIB, CRC, frame-record, logical-frame, super-frame and super-frame-record regions and every integer field of the
    stream and slot tables.  (snr_db_est / mer_db_est of a chunk are documented as that frame's or the previous one's from 48 streams up:
    they are compared in the one-ensemble case.)"""
    S, n_frames = 64, 21
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=92)
    x = ds.channel(ens.iq, snr_db=21.0, cfo_hz=-95.0, timing_offset=777, seed=4, n_out=(n_frames + 1) * TF)
    codes = quantise(x, kind, 0.25 / np.sqrt(np.mean(np.abs(x) ** 2)))
    xs = [codes[2 * (13 * s + s % 2):][:2 * n_frames * TF] for s in range(S)]
    chunks = {}
    for name, rf in (("nat", kind), ("cf32", 0)):
        e = dx.Engine(n_streams=S, ring_frames=n_frames + 1, max_subch=18, out_frames=8, msc_fast_min_jobs=1, ring_format=rf)
        e.set_subchannels(subch)
        e.delivery_open(slots=4)
        for s in range(S):
            e.push_iq(s, xs[s])
        got = []
        for _ in range(n_frames // 7):
            e.process(7, sync=False)
            while True:
                ch = e.delivery_next(wait=True)
                if ch is None:
                    break
                got.append(ch)
        nf = lambda c, s: int(c.streams[s]["n_frames"])       # noqa: E731
        chunks[name] = [dict(fibs=[c.fibs[s, :nf(c, s)].copy() for s in range(S)], crc=[c.crc[s, :nf(c, s)].copy() for s in range(S)],
                             frames=[c.frames[s, :nf(c, s)].tobytes() for s in range(S)], streams=c.streams.copy(), subch=c.subch.copy(),
                             msc=[[c.msc(s, j).copy() for j in range(18)] for s in range(S)],
                             sf=[[c.superframes(s, j).copy() for j in range(18)] for s in range(S)],
                             sfi=[[c.superframe_info(s, j).tobytes() for j in range(18)] for s in range(S)]) for c in got]
        for c in got:
            c.release()
        e.delivery_close()
        e.close()
    a, b = chunks["nat"], chunks["cf32"]
    assert len(a) == len(b) >= 2
    assert sum(int(c["streams"]["n_frames"].sum()) for c in a) >= S * (n_frames - 8)
    for ca, cb in zip(a, b):
        for k in ("fibs", "crc"):
            assert all(np.array_equal(p, q) for p, q in zip(ca[k], cb[k])), k
        assert ca["frames"] == cb["frames"]
        for tab in ("streams", "subch"):
            for name in ca[tab].dtype.names:
                if np.issubdtype(ca[tab].dtype[name].base, np.integer):
                    assert np.array_equal(ca[tab][name], cb[tab][name]), (tab, name)
        for k in ("msc", "sf"):
            assert all(np.array_equal(p, q) for ra, rb in zip(ca[k], cb[k]) for p, q in zip(ra, rb)), k
        assert ca["sfi"] == cb["sfi"]


# ------------------------------------------------------------------------------------------------------ 5. files
def _write(tmp_path, which, x, g, rate=2048000):
    path = str(tmp_path / ("rec_%s.%s" % (which, {"raw": "iq", "sdr": "sdr"}.get(which, "uff"))))
    if which == "raw":
        iqf.write_raw(path, x, g)
    elif which == "sdr":
        iqf.write_sdr(path, x, rate, g)
    elif which == "uff_i16_msb_qi":
        v = iqf.to_int(x, 16, g).reshape(-1, 2)[:, ::-1].reshape(-1)
        iqf.write_uff(path, iqf.pack_int(v, 2, True), rate, 16, "int16", "MSB", order="QI")
    elif which == "uff_f32":
        iqf.write_uff(path, (x * g).astype(np.complex64).view(np.uint8), rate, 32, "float32", "LSB")
    elif which == "uff_i24":
        iqf.write_uff(path, iqf.pack_int(iqf.to_int(x, 24, g), 3, False), rate, 24, "int24", "LSB")
    return path


def _played(path, subch, ring_format):
    eng = dx.Engine(n_streams=1, ring_frames=10, max_subch=18, ring_format=ring_format)
    eng.set_subchannels(subch)
    frames = dx.play_file(eng, 0, path, block_frames=3)
    out = (frames, stats_bits(eng.stats(0)), eng.read_fibs(0, 4), [eng.read_msc(0, j, 16) for j in range(18)], [eng.read_superframes(0, j, 3) for j in range(18)])
    eng.close()
    return out


def _same_play(a, b):
    assert a[0] == b[0] >= 12 and a[1] == b[1]
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1]) and a[2][1].all()
    for k in (3, 4):
        assert all(np.array_equal(p, q) for p, q in zip(a[k], b[k]))


@pytest.mark.parametrize("which,kind", [("raw", "u8"), ("sdr", "s16"), ("uff_i16_msb_qi", "s16")])
def test_recorded_files_play_into_the_ring_of_their_sample_type(tmp_path, which, kind):
    subch, _, x, g, _ = _case2(kind)
    path = _write(tmp_path, which, x, g)
    fmt = dx.probe_iq_file(path)
    if which == "uff_i16_msb_qi":
        assert (fmt.family, fmt.container, fmt.big_endian, fmt.swap_iq, fmt.bits) == (2, 2, 1, 1, 16)
    _same_play(_played(path, subch, kind), _played(path, subch, 0))
    # the bulk ingest's general form: two streams, the second recording shorter
    with open(path, "rb") as fh:
        fh.seek(fmt.data_offset)
        payload = np.frombuffer(fh.read(fmt.data_bytes), np.uint8)
    sb = fmt.sample_bytes()
    lens = [14 * TF * sb, 9 * TF * sb + 5 * sb]
    res = {}
    for name, rf in (("nat", kind), ("cf32", 0)):
        e = dx.Engine(n_streams=2, ring_frames=12, max_subch=18, ring_format=rf)
        e.set_subchannels(subch)
        slabs, pitch = e.ingest_open_formats([fmt, fmt], slabs=2, max_frames=4)
        per, pos, k = 3 * TF * sb + 7 * sb, [0, 0], 0
        while any(pos[s] < lens[s] for s in range(2)):
            nb = []
            for s in range(2):
                take = min(per, lens[s] - pos[s])
                slabs[k % 2][s, :take] = payload[pos[s]:pos[s] + take]
                nb.append(take); pos[s] += take
            e.ingest_submit_bytes(k % 2, nb)
            e.ingest_commit(k % 2)
            e.process(4)
            k += 1
        e.process(3)
        res[name] = [(stats_bits(e.stats(s)), e.read_fibs(s, 4), [e.read_msc(s, j, 16) for j in range(18)], [e.read_superframes(s, j, 3) for j in range(18)]) for s in range(2)]
        e.ingest_close()
        e.close()
    for s in range(2):
        a, b = res["nat"][s], res["cf32"][s]
        assert a[0] == b[0] and a[0]["frames"] >= (12, 7)[s]
        assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])
        for k in (2, 3):
            assert all(np.array_equal(p, q) for p, q in zip(a[k], b[k]))


@pytest.mark.parametrize("which,kind,rate,good", [("sdr", "s16", 2500000, "sdr"), ("uff_f32", "s16", 2048000, "sdr"), ("uff_i24", "s16", 2048000, "sdr"),
                                                  ("raw", "s16", 2048000, "sdr"), ("sdr", "u8", 2500000, "raw"), ("uff_f32", "u8", 2048000, "raw"),
                                                  ("uff_i24", "u8", 2048000, "raw"), ("sdr", "u8", 2048000, "raw")])
def test_files_whose_samples_are_not_the_rings_codes_are_refused_and_leave_the_engine_usable(tmp_path, which, kind, rate, good):
    subch, _, x, g, _ = _case2(kind)
    bad = _write(tmp_path, which, x[:3 * TF], g, rate)
    eng = dx.Engine(n_streams=1, ring_frames=10, max_subch=18, ring_format=kind)
    eng.set_subchannels(subch)
    with pytest.raises(dx.DabxError, match="DABX_RING_" + kind.upper()):
        dx.play_file(eng, 0, bad, block_frames=3)
    with pytest.raises(dx.DabxError, match="DABX_RING_" + kind.upper()):
        eng.ingest_open_formats([dx.probe_iq_file(bad)], slabs=2, max_frames=3)
    assert eng.stats(0)["samples_consumed"] == 0 and eng.stats(0)["frames"] == 0
    with pytest.raises(dx.DabxError, match="not in the ring"):    # the write position has not moved: there is no sample 0
        eng.read_iq(0, 0, 1)
    path = _write(tmp_path, good, x, g)
    frames = dx.play_file(eng, 0, path, block_frames=3)
    got = (frames, stats_bits(eng.stats(0)), eng.read_fibs(0, 4), [eng.read_msc(0, j, 16) for j in range(18)], [eng.read_superframes(0, j, 3) for j in range(18)])
    eng.close()
    _same_play(got, _played(path, subch, 0))


# ------------------------------------------------------------------------------------------------------ 6. refusals at the interface
def test_create_ex_refuses_what_the_header_says_it_refuses():
    L = dx.load()
    for rf in (3, -1):
        with pytest.raises(dx.DabxError, match="ring_format"):
            dx.Engine(n_streams=1, max_subch=0, fic_only=1, ring_format=rf)
    for kind in KINDS:
        with pytest.raises(dx.DabxError, match="dc_iq_correction"):
            dx.Engine(n_streams=1, max_subch=0, fic_only=1, ring_format=kind, dc_iq_correction=1)
    cfg = dx.Config()
    L.dabx_default_config(C.byref(cfg))
    cfg.max_subch, cfg.fic_only = 0, 1
    h = C.c_void_p()
    for size in (0, 4, 7):                                        # smaller than the first two fields
        ext = dx.CreateExt(size=size, ring_format=1)
        assert L.dabx_create_ex(C.byref(cfg), C.byref(ext), C.byref(h)) == -2 and not h.value
    ext = dx.CreateExt(size=8, ring_format=2)                     # a caller that knows the first two fields only
    assert L.dabx_create_ex(C.byref(cfg), C.byref(ext), C.byref(h)) == 0 and h.value
    fmt, bps = C.c_int32(-1), C.c_int32(-1)
    assert L.dabx_get_ring_format(h, C.byref(fmt), C.byref(bps)) == 0 and (fmt.value, bps.value) == (2, 2)
    L.dabx_destroy(h)
    h = C.c_void_p()
    assert L.dabx_create_ex(C.byref(cfg), None, C.byref(h)) == 0 and h.value          # NULL: exactly dabx_create
    assert L.dabx_get_ring_format(h, C.byref(fmt), None) == 0 and fmt.value == 0
    assert L.dabx_get_ring_format(h, None, C.byref(bps)) == 0 and bps.value == 8
    x = (np.arange(64) / 64).astype(np.complex64)
    assert L.dabx_push_iq(h, 0, x.ctypes.data_as(C.c_void_p), 0, 64) == 0             # ... which takes every fmt
    L.dabx_destroy(h)
    assert L.dabx_get_ring_format(None, C.byref(fmt), C.byref(bps)) == -2


@pytest.mark.parametrize("kind", KINDS)
def test_a_native_ring_takes_its_own_codes_only(kind):
    other = "u8" if kind == "s16" else "s16"
    rng = np.random.default_rng(8)
    own = rng.integers(0, 200, 2 * 5000).astype(DTYPE[kind])
    eng = dx.Engine(n_streams=1, ring_frames=2, max_subch=0, fic_only=1, ring_format=kind)
    eng.push_iq(0, own)
    for bad in (np.zeros(100, np.complex64), np.zeros(200, DTYPE[other])):
        for push in (eng.push_iq, eng.push_iq_async):
            with pytest.raises(dx.DabxError, match="DABX_RING_" + kind.upper()):
                push(0, bad)
    for bad in (np.complex64, DTYPE[other]):
        with pytest.raises(dx.DabxError, match="DABX_RING_" + kind.upper()):
            eng.ingest_open(bad, slabs=2, max_frames=1)
    with pytest.raises(dx.DabxError, match="not in the ring"):    # the write position is where it was
        eng.read_iq(0, 0, 5001)
    assert np.array_equal(eng.read_iq(0, 0, 5000).view(np.uint32), values(own, kind).view(np.uint32))
    assert eng.stats(0)["samples_consumed"] == 0
    eng.push_iq_async(0, own)                                     # and the engine goes on taking its own
    eng.push_wait()
    assert np.array_equal(eng.read_iq(0, 5000, 5000).view(np.uint32), values(own, kind).view(np.uint32))
    eng.close()


# ------------------------------------------------------------------------------------------------------ 7. zero-copy producer
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("announce", [False, True])
def test_zero_copy_producers_write_codes_into_the_ring(kind, announce):
    hip = C.CDLL("libamdhip64.so")
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=171)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=911.0, timing_offset=77777, gain=0.25, seed=17, n_out=30 * TF).copy()
    x[int(10.6 * TF):int(14.4 * TF)] = 0
    codes = np.ascontiguousarray(quantise(x, kind, 1.0))
    n = len(x)
    out = {}
    for name, rf in (("nat", kind), ("cf32", 0)):
        eng = dx.Engine(n_streams=1, ring_frames=n // TF + 1, max_subch=4, out_frames=4, ring_format=rf)
        eng.set_subchannels(subch)
        ptr, cap = eng.ring_ptr(0)
        bps = eng.ring_format()[1]
        assert cap >= n                                           # (in samples, whatever the element)
        if announce:
            eng.announce_write(n)
        src = codes if rf else values(codes, kind)
        assert src.nbytes == bps * n
        assert hip.hipMemcpy(C.c_void_p(ptr), C.c_void_p(src.ctypes.data), C.c_size_t(bps * n), 1) == 0      # host to device
        eng.commit(n)
        r = dict(start=[], level=[], fibs=[])
        idle = 0
        for _ in range(400):
            before = eng.stats(0)
            eng.process(1)
            st = eng.stats(0)
            idle = idle + 1 if st["samples_consumed"] == before["samples_consumed"] else 0
            r["level"].append((st["samples_consumed"], bits(st["signal_level"]), bits(st["peak_level"])))
            if st["frames"] > before["frames"]:
                r["start"].append(st["last_start_index"]); r["fibs"].append(eng.read_fibs(0, 1)[0].tobytes())
            if idle >= 4:
                break
        r["final"] = stats_bits(eng.stats(0))
        eng.close()
        out[name] = r
    assert out["nat"] == out["cf32"]
    st = out["nat"]["final"]
    assert len(out["nat"]["start"]) >= 20
    if announce:
        assert st["level_rewalk_events"] >= 1 and st["level_unanchored_events"] == 0, st
    else:
        assert st["level_unanchored_events"] >= 1 and st["level_rewalk_events"] == 0, st
