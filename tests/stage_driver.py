"""What the tests of the MSC slot stages share (test_gpu_dabplus_stage.py, test_gpu_packet_stage.py, test_gpu_pad_stage.py,
test_gpu_mp2_pad_stage.py, and the engine of test_gpu_msc_decoder.py): the engine with profiling on, the batch loop over dx.msc_inject /
dx.msc_decode, the follower of a slot's output ring, and the comparisons with the oracle back end and the models that decide whether a
stage test passes.  The comparisons need no device: tests/test_stage_driver.py shows on the CPU that each notices one wrong byte."""
import collections
import ctypes as C

import numpy as np

import dabplus_cases as dc
import mp2_pad_cases as mc
import packet_cases as pkc
import pad_cases as pc
from dabstar_amd import lib as dx

H, B = dc.HISTORY, dc.BATCH
SF_COUNTERS = (("cifs_decoded", "cif_out"), ("sf_ok", "sf_ok"), ("sf_fail", "sf_fail"), ("rs_corrected", "rs_corr"), ("rs_failed", "rs_fail"),
               ("fc_corrected", "fc_corr"), ("au_ok", "au_ok"), ("au_bad", "au_bad"))


def engine(n_streams, max_subch, fast_min=1, class_min=1, tie_mode=0):
    eng = dx.Engine(n_streams=n_streams, ring_frames=2, max_subch=max_subch, out_frames=1, viterbi_tie_mode=tie_mode,
                    msc_fast_min_jobs=fast_min, msc_class_min_jobs=class_min)
    dx.check(dx.load().dabx_set_profiling(eng._h, 1))
    return eng


def kernel_launches(eng):
    ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)(); names = (C.c_char_p * 16)()
    nk = dx.check(dx.load().dabx_get_profile(eng._h, ms, cnt, names))
    return {names[i].decode(): int(cnt[i]) for i in range(nk)}


# ---- a slot's output ring (out_ring.h): data groups of a packet-mode slot, PAD items of a PAD slot -----------------------------------------
Ring = collections.namedtuple("Ring", "stats count bytes read dtype")
DATAGROUPS = Ring("packet_stats", ("dg_count",), ("dg_bytes",), "read_datagroups", dx.DATAGROUP_INFO)
PAD_ITEMS = Ring("pad_stats", ("labels", "groups"), ("label_bytes", "group_bytes"), "read_pad_items", dx.PAD_ITEM)


def packet_follower(kbps):
    """A packet slot completes at most one group per 24-byte packet of a batch; max_bytes: the batch's bytes and a group under assembly."""
    return Follower(DATAGROUPS, B * (kbps // 8), max_bytes=B * (kbps // 8) * 127 + dx.DG_MAX_BYTES)


class Follower:
    """Follows one slot's ring from batch to batch: take() reads what the counters say is new -- at most `bound` records per batch -- and
    appends it with byte_pos counted from the slot's first byte, so that result() is the slot's whole sequence."""

    def __init__(self, ring, bound, max_bytes=None):
        self.ring, self.bound, self.max_bytes = ring, bound, max_bytes
        self.seen = self.byte_seen = 0
        self.rec, self.by = [], []

    def take(self, eng, i, j):
        """(the slot's stats, the new records or None, their bytes, how many records and bytes the slot had before)."""
        st = getattr(eng, self.ring.stats)(i, j)
        first, first_byte = self.seen, self.byte_seen
        new, total = sum(st[k] for k in self.ring.count) - first, sum(st[k] for k in self.ring.bytes)
        assert 0 <= new <= self.bound, (i, j, new)
        rec = by = None
        if new:
            rec, by = getattr(eng, self.ring.read)(i, j, new, max_bytes=self.max_bytes)
            assert len(rec) == new and rec["byte_pos"][0] == 0 and len(by) == total - first_byte, (i, j, new, len(rec), len(by))
            rec = rec.copy()
            rec["byte_pos"] += first_byte
            self.rec.append(rec); self.by.append(by)
        self.seen, self.byte_seen = first + new, total
        return st, rec, by, first, first_byte

    def result(self):
        return (np.concatenate(self.rec) if self.rec else np.zeros(0, self.ring.dtype)), (np.concatenate(self.by) if self.by else np.zeros(0, np.uint8))


def drive(eng, cases, schedule, switch_on, followers, idle_state, after_batch=None):
    """cases[i] = (layout, intended frames, CIFs, ...) of stream i.  Configures the streams (switch_on(eng, i) sets the slots' modes), 16
    CIFs of history, then one MSC batch per row of `schedule` ([batch][stream] CIF counts).  After every batch the new logical frames,
    super frames and records of every configured slot are read and appended, then followers[(i, j)] takes its slot's new ring items, then
    after_batch(i, logical frames so far, {j: what take() returned}) runs; a stream that received nothing must hold byte for byte what it
    held (idle_state(eng, i)).  Returns {(i, j): {"frames", "sf", "sfi", "sf_new" (per batch of the stream), "stats", "rec", "bytes"}}."""
    S = len(cases)
    got = {}
    for i, case in enumerate(cases):
        eng.set_subchannels(case[0], stream=i)                   # SubCh.dab_plus of every slot decides
        switch_on(eng, i)
        dx.msc_inject(eng, i, case[2][:H])
        for j, sc in enumerate(case[0]):
            if sc.kbps:
                got[(i, j)] = {"frames": [], "sf": [], "sfi": [], "sf_new": [], "seen": 0}
    dx.msc_decode(eng, [H] * S, H)
    at = [H] * S
    for counts in schedule:
        before = {i: idle_state(eng, i) for i in range(S) if counts[i] == 0}
        for i in range(S):
            if counts[i]:
                dx.msc_inject(eng, i, cases[i][2][at[i]:at[i] + counts[i]])
        dx.msc_decode(eng, counts, B)
        for i in range(S):
            if counts[i] == 0:
                assert idle_state(eng, i) == before[i], "stream %d received nothing in this batch and changed" % i
                continue
            at[i] += counts[i]
            eng.subch = list(cases[i][0])                        # Engine.read_msc sizes its buffer from it
            taken = {}
            for j, sc in enumerate(cases[i][0]):
                if not sc.kbps:
                    continue
                g = got[(i, j)]
                fr = eng.read_msc(i, j, counts[i])
                assert fr.shape[0] == counts[i], (sc.kbps, i, j, fr.shape)
                g["frames"].append(fr)
                new = eng.subch_stats(i, j)["sf_count"] - g["seen"]
                assert 0 <= new <= 6, (sc.kbps, i, j, new)       # 28 + 4 frames hold at most 6 windows: nothing left the ring of 16 unread
                if new:
                    sf, sfi = eng.read_superframes(i, j, new), eng.read_superframe_info(i, j, new)
                    assert sf.shape[0] == new == len(sfi), (sc.kbps, i, j, new)
                    g["sf"].append(sf); g["sfi"].append(sfi)
                g["seen"] += new
                g["sf_new"].append(new)
                if (i, j) in followers:
                    taken[j] = followers[(i, j)].take(eng, i, j)
            if after_batch:
                after_batch(i, at[i] - H, taken)
    for (i, j), g in got.items():
        g["frames"] = np.concatenate(g["frames"])
        g["sf"] = np.concatenate(g["sf"]) if g["sf"] else np.zeros((0, 110 * cases[i][0][j].kbps // 8), np.uint8)
        g["sfi"] = np.concatenate(g["sfi"]) if g["sfi"] else np.zeros(0, dx.SUPERFRAME_INFO)
        g["stats"] = eng.subch_stats(i, j)
        g["rec"], g["bytes"] = followers[(i, j)].result() if (i, j) in followers else (np.zeros(0, np.uint8),) * 2
    return got


# ---- the comparisons: every difference as a line that names the stream, the slot, the bit rate and the kind -------------------------------
def oracle_mismatches(tag, g, o, frames):
    """Logical frames, super frames, their records and the counters of one slot against the oracle back end's (o) and the intended frames."""
    bad = []
    if not np.array_equal(o["frames"], frames):
        bad.append(tag + "the oracle's logical frames are not the intended ones")
    if not np.array_equal(g["frames"], o["frames"]):
        bad.append(tag + "logical frames differ from the oracle's")
    if g["sfi"].tobytes() != o["sfi"].tobytes() or not np.array_equal(g["sf"], o["sf"]):
        bad.append(tag + "super frames or their records differ from the oracle's (%d, the oracle has %d)" % (len(g["sfi"]), len(o["sfi"])))
    for mine, theirs in SF_COUNTERS:
        if g["stats"][mine] != o["stats"][theirs]:
            bad.append(tag + "%s = %d, the oracle's %d" % (mine, g["stats"][mine], o["stats"][theirs]))
    return bad


def ring_mismatches(tag, g, model, counters, noun):
    """The ring items of one slot (g["rec"], g["bytes"], g["pstats"]) against a model's: records by .tobytes(), bytes by np.array_equal,
    every counter by ==."""
    bad = []
    want, want_bytes = model.records(), model.all_bytes()
    if g["rec"].tobytes() != want.tobytes():
        d = [k for k in range(min(len(g["rec"]), len(want))) if g["rec"][k].tobytes() != want[k].tobytes()][:3]
        bad.append(tag + "%d %ss, the model has %d; first differences %s" % (len(g["rec"]), noun, len(want), [(k, g["rec"][k].tolist(), want[k].tolist()) for k in d]))
    if not np.array_equal(g["bytes"], want_bytes):
        n = min(len(g["bytes"]), len(want_bytes))
        d = np.flatnonzero(g["bytes"][:n] != want_bytes[:n])
        bad.append(tag + "%s bytes differ (%d, the model has %d; first difference at %d)" % (noun, len(g["bytes"]), len(want_bytes), d[0] if len(d) else n))
    for k in counters:
        if g["pstats"][k] != model.counters[k]:
            bad.append(tag + "%s = %d, the model's %d" % (k, g["pstats"][k], model.counters[k]))
    return bad


def _tag(i, j, kbps, kind):
    return "stream %d slot %d (%d kbit/s, %s): " % (i, j, kbps, kind)


def packet_mismatches(got, cases, streams):
    """test_gpu_packet_stage.py: every slot against the oracle, the packet slots against packet_cases' model at the stream's address."""
    bad = []
    for (i, j), g in sorted(got.items()):
        lay, address = pkc.STAGE_STREAMS[streams[i]]
        kbps, kind = pkc.STAGE_LAYOUTS[lay][j]
        tag = _tag(i, j, kbps, kind)
        # the soft bits decode to the intended frames, on the oracle and on the device; DAB+ results equal the oracle back end's
        bad += oracle_mismatches(tag, g, cases[i][3][j], cases[i][1][j])
        if kind != "pkt":
            if g["pstats"]["active"] or any(g["pstats"].values()) or len(g["rec"]):
                bad.append(tag + "not in packet mode and shows packet results: %s" % g["pstats"])
            continue
        bad += ring_mismatches(tag, g, pkc.run_model(cases[i][1][j], address), pkc.PACKET_COUNTERS, "data group")
        if g["pstats"]["dg_lost"] != 0 or g["pstats"]["active"] != 1 or g["pstats"]["packet_address"] != address:
            bad.append(tag + "dg_lost / active / packet_address: %s" % g["pstats"])
    return bad


def pad_mismatches(got, cases, streams):
    """test_gpu_pad_stage.py: every slot against the oracle, the PAD slots against pad_cases' model on the oracle's super frames."""
    bad = []
    for (i, j), g in sorted(got.items()):
        kbps, kind = pc.STAGE_LAYOUTS[pc.STAGE_STREAMS[streams[i]]][j]
        tag = _tag(i, j, kbps, kind)
        o = cases[i][3][j]
        bad += oracle_mismatches(tag, g, o, cases[i][1][j])
        if kind != "pad":
            if any(g["pstats"].values()) or len(g["rec"]):
                bad.append(tag + "no PAD decoding and shows PAD results: %s" % g["pstats"])
            continue
        bad += ring_mismatches(tag, g, pc.run_model(o["sf"], o["sfi"]), pc.PAD_COUNTERS, "item")
        if g["pstats"]["items_lost"] != 0 or g["pstats"]["active"] != 1:
            bad.append(tag + "items_lost / active: %s" % g["pstats"])
    return bad


def mp2_batch_mismatches(tag, m, n, taken, sy):
    """An MP2 slot after n logical frames against the model's snapshot: what its follower took (the new items and bytes, dabx_pad_stats)
    and dabx_mp2_sync_stats (sy)."""
    bad = []
    items, n_bytes, counters, sync = m.snaps[n]
    st, rec, by, first, first_byte = taken
    for k in pc.PAD_COUNTERS:
        if st[k] != counters[k]:
            bad.append(tag + "after %d frames %s = %d, the model's %d" % (n, k, st[k], counters[k]))
    if st["items_lost"] != 0 or st["active"] != 1:
        bad.append(tag + "after %d frames items_lost / active: %s" % (n, st))
    for k in mc.SYNC_FIELDS:
        if sy[k] != sync[k]:
            bad.append(tag + "after %d frames sync %s = %d, the model's %d" % (n, k, sy[k], sync[k]))
    if rec is not None:
        want = m.pad.records()[first:items]
        if rec.tobytes() != want.tobytes():
            d = [k for k in range(min(len(rec), len(want))) if rec[k].tobytes() != want[k].tobytes()][:3]
            bad.append(tag + "after %d frames %d new items, the model has %d; first differences %s" % (n, len(rec), len(want), [(k, rec[k].tolist(), want[k].tolist()) for k in d]))
        if not np.array_equal(by, m.pad.all_bytes()[first_byte:n_bytes]):
            bad.append(tag + "after %d frames the new items' bytes differ (%d, the model has %d)" % (n, len(by), n_bytes - first_byte))
    return bad


def mp2_final_mismatches(got, cases, streams, mp2=True):
    """test_gpu_mp2_pad_stage.py, the whole run of every slot: every slot against the oracle back end, MP2 slots against the model,
    DAB+ PAD slots against pad_cases' model on the oracle's super frames, the other slots show no PAD results."""
    bad = []
    for (i, j), g in sorted(got.items()):
        s = streams[i]
        kbps, kind = mc.kinds(s)[j]
        tag = _tag(i, j, kbps, kind)
        o = cases[i][3][j]
        bad += oracle_mismatches(tag, g, o, cases[i][1][j])
        if kind == "mp2" and mp2:
            m = mc.slot_model(s, j)
            bad += ring_mismatches(tag, g, m.pad, pc.PAD_COUNTERS, "item")
            if g["sync"] != m.sync_stats():
                bad.append(tag + "sync stats %s, the model's %s" % (g["sync"], m.sync_stats()))
        elif kind == "pad":
            bad += ring_mismatches(tag, g, pc.run_model(o["sf"], o["sfi"]), pc.PAD_COUNTERS, "item")
            if any(g["sync"].values()):
                bad.append(tag + "a DAB+ PAD slot shows MP2 sync stats: %s" % g["sync"])
        elif any(g["pstats"].values()) or any(g["sync"].values()) or len(g["rec"]):
            bad.append(tag + "no PAD decoding and shows PAD results: %s %s" % (g["pstats"], g["sync"]))
        if kind in ("mp2", "pad") and (kind == "pad" or mp2) and (g["pstats"]["items_lost"] != 0 or g["pstats"]["active"] != 1):
            bad.append(tag + "items_lost / active: %s" % g["pstats"])
    return bad
