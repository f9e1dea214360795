"""The FIG section of the bulk delivery (DABX_DELIVER_FIG, dabx_chunk_header_ext.off_fig, dabx_chunk_fig; deliver.hip k_deliver_records) through
IQ: four streams of one FIC-only engine, each with a crafted FIC of 15 frames (tests/fig_cases.py: the 18-sub-channel ensemble with its
labels, restarts between labels, an announced reconfiguration, and a flood of labels that makes more events per chunk than a chunk has
room for), two dabx_process calls of 7 frames = 2 chunks.  Chunk.fig equals dabx_read_fig_events of the same frames and the Python model
fed with the chunk's own FIBs; what does not fit is counted and the database is still complete; without the bit nothing of a slab changes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fic_cases as fc
import fig_cases as fg
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S, F, N_FRAMES = 4, 7, 15
FLOOD = 2
CALLS = (7, 7)


def flood_fibs():
    """180 FIBs, a label with a key of its own in each: 12 events per frame, 84 per chunk"""
    out = []
    for i in range(12 * N_FRAMES):
        k = i // 3
        out.append(fg.one_fib((fg.fig1s1(0x5000 + k, "svc %d" % k), fg.fig1s5(0x70000000 + k, "data %d" % k), fg.fig1s4(k & 1, k % 16, 0x6000 + k, "comp %d" % k))[i % 3]))
    return np.stack(out)


def iq_of(fibs, seed):
    """[12 n, 32] FIBs -> n frames of IQ whose FIC they are (no sub-channel: the MSC symbols carry random bits), as tools/dab_synth.py codes an ensemble's"""
    frames = fibs.reshape(-1, 12, 32)
    n = len(frames)
    rng = np.random.default_rng(seed)
    tx = rng.integers(0, 2, (n, 75, 3072), dtype=np.uint8)
    fmask, fdisp = ds.fic_mask().astype(bool), ds.prbs(768)
    for f in range(n):
        tx[f, :3] = np.concatenate([ds.conv_encode(np.unpackbits(frames[f, 3 * g:3 * g + 3].reshape(-1)) ^ fdisp)[fmask] for g in range(4)]).reshape(3, 3072)
    iq = ds._ofdm_frames(tx, n, False, 0, None).reshape(-1)
    return ds.channel(iq, snr_db=30.0, cfo_hz=30.0 * seed, timing_offset=3000 + 500 * seed, seed=seed, cyclic=False).copy()


def signals():
    pad = np.stack([fc.FILLER] * 12 * N_FRAMES)
    seqs = [fg.sequences()["ensemble18"][0], fg.sequences()["restart_labels"][0], flood_fibs(), fg.sequences()["reconf_flags_3_fig00_first"][0]]
    return [iq_of(np.concatenate([q, pad])[:12 * N_FRAMES], s) for s, q in enumerate(seqs)]


def run(xs, what, mode):
    """-> (chunks as dicts, per stream what read_fig_events gave after every call, slab bytes, per stream the database at the end)"""
    eng = dx.Engine(n_streams=S, ring_frames=N_FRAMES + 2, max_subch=1, out_frames=8, fic_only=True, acquire_mode=1, schedule=1)
    try:
        for s, x in enumerate(xs):
            eng.push_iq(s, x)
        if mode:
            eng.set_fig_mode(-1)
        eng.delivery_open(slots=4, what=what)
        slab = eng.delivery_slab_bytes()
        chunks, read = [], [[] for _ in range(S)]
        for m in CALLS:
            eng.process(m)
            ch = eng.delivery_next(wait=True)
            assert ch is not None and ch.seq == len(chunks)
            chunks.append(dict(raw=ch.raw.copy(), header=ch.header.copy(), ext=None if ch.header_ext is None else ch.header_ext.copy(),
                               table=None if ch.fig_table is None else ch.fig_table.copy(), fig=[ch.fig(s) for s in range(S)],
                               n_frames=[int(ch.streams[s]["n_frames"]) for s in range(S)],
                               fibs=[ch.fibs[s, :int(ch.streams[s]["n_frames"])].copy() for s in range(S)],
                               crc=[ch.crc[s, :int(ch.streams[s]["n_frames"])].copy() for s in range(S)]))
            ch.release()
            assert eng.delivery_next(wait=False) is None
            if mode:
                for s in range(S):
                    ev, lost = eng.read_fig_events(s)
                    assert lost == 0
                    read[s].append(ev)
        db = None
        if mode:
            db = [dict(info=eng.fig_info(s), subch=[dx._subch_dict(q) for q in eng.fig_subchannels(s)], labels=eng.fig_labels(s), stats=eng.fig_stats(s))
                  for s in range(S)]
            for bad in (dx.DELIVER_FIG, dx.DELIVER_FIG | dx.DELIVER_TII, 131072, 131072 | 256, 131072 | dx.DELIVER_FIB, 1024 | dx.DELIVER_FIB, 4096 | dx.DELIVER_FIB, 16384 | dx.DELIVER_FIB):
                with pytest.raises(dx.DabxError, match="error -2"):           # DABX_E_ARG, before "already open" is looked at
                    eng.delivery_open(slots=4, what=bad)
        eng.delivery_close()
    finally:
        eng.close()
    return chunks, read, slab, db


@pytest.fixture(scope="module")
def world():
    xs = signals()
    return dict(fig=run(xs, dx.DELIVER_FIB | dx.DELIVER_FIG, True), fib=run(xs, dx.DELIVER_FIB, False), fib_mode=run(xs, dx.DELIVER_FIB, True))


def test_the_chunk_events_are_read_fig_events_of_the_same_frames_and_the_models(world):
    chunks, read, _, db = world["fig"]
    assert len(chunks) == 2
    for s in range(S):
        m = fg.Model()
        total = 0
        for q, r in zip(chunks, read[s]):
            assert q["n_frames"][s] >= 6
            before = len(m.events)
            m.feed(q["fibs"][s].reshape(-1, 32), q["crc"][s].reshape(-1))
            new = m.events[before:]
            assert r == new, s                                             # read_fig_events after the call: the events of the chunk's frames
            row = q["table"][s]
            total += len(new)
            keep = min(len(new), dx.FIG_CHUNK_RECORDS)
            assert q["fig"][s] == (new[-keep:] if keep else []), s         # the chunk: the newest that fit, oldest first
            assert (int(row["n_records"]), int(row["records_lost"]), int(row["records_total"])) == (keep, len(new) - keep, total), s
            assert int(row["first_record"]) == total - keep
        # the database is the truth, complete whatever the chunks lost
        assert db[s]["info"] == m.info() and db[s]["subch"] == m.subch(0) and db[s]["labels"] == m.row()["labels"], s
        assert {k: db[s]["stats"][k] for k in fg.COUNTERS} == m.row()["stats"], s
    lost = [int(q["table"][FLOOD]["records_lost"]) for q in chunks]
    assert all(v >= 12 * 6 - dx.FIG_CHUNK_RECORDS for v in lost), lost      # 12 labels per frame: more than the room of 32
    assert len(db[FLOOD]["labels"]) == sum(q["n_frames"][FLOOD] for q in chunks) * 12
    assert all(int(q["table"][s]["records_lost"]) == 0 for q in chunks for s in range(S) if s != FLOOD)
    assert len(db[0]["subch"]) == 18 and len(db[0]["labels"]) >= 19 and db[1]["info"]["n_restarts"] == 2 and db[3]["info"]["n_changes"] == 1


def test_with_the_bit_the_extension_announces_the_section(world):
    chunks, _, slab, _ = world["fig"]
    plain, _, slab0, _ = world["fib"]
    off_fig = int(chunks[0]["ext"]["off_fig"])
    assert off_fig % 16 == 0 and slab == (off_fig + S * (32 + dx.FIG_CHUNK_RECORDS * 64) + 255) // 256 * 256
    for q, p in zip(chunks, plain):
        h, x = q["header"], q["ext"]
        assert int(h["off_stream"]) == 192 and int(h["what"]) == dx.DELIVER_FIB | dx.DELIVER_FIG and int(h["bytes"]) == slab
        assert int(x["magic"]) == dx.CHUNK_EXT_MAGIC and int(x["bytes"]) == 64 and int(x["off_fig"]) == off_fig == int(x["reserved"][0])
        assert not any(int(x[k]) for k in ("off_tii", "off_mp2_audio", "off_aac", "off_scope", "off_cir", "off_spectrum"))
        for s in range(S):
            assert int(q["table"][s]["rec_off"]) == off_fig + S * 32 + s * dx.FIG_CHUNK_RECORDS * 64
        for k, n in (("off_fib", S * F * 384), ("off_crc", S * F * 12), ("off_frame", S * F * 16), ("off_stream", S * 72)):
            a, b = int(h[k]), int(p["header"][k])
            assert a == b + 64 and q["raw"][a:a + n].tobytes() == p["raw"][b:b + n].tobytes(), k


def test_without_the_bit_a_slab_is_what_it_was(world):
    chunks, _, slab, _ = world["fib"]
    chunks2, read2, slab2, db2 = world["fib_mode"]
    assert slab == slab2 and len(chunks) == len(chunks2) == 2
    for q, q2 in zip(chunks, chunks2):
        assert q["ext"] is None and q["table"] is None and int(q["header"]["off_stream"]) == 128 and not int(q["header"]["what"]) & dx.DELIVER_FIG
        assert len(q["raw"]) == slab and q["raw"].tobytes() == q2["raw"].tobytes()        # the stage beside it changes no delivered byte
        assert q2["fig"] == [[] for _ in range(S)]
    # ... while the engine with the mode on made the very events of the delivery with the bit
    assert read2 == world["fig"][1] and db2[0]["labels"] == world["fig"][3][0]["labels"]


def test_the_section_works_in_the_hipmodule_form():
    """the first test again with the binding pointed at hipmodule/libdabx.so: k_fig and the section's gather are found in the code objects"""
    from hipmodule_env import hipmodule_env
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_fig_delivery.py", "-k", "chunk_events"],
                       cwd=ROOT, env=hipmodule_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "1 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-500:]
