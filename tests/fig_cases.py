"""Inputs and models of the FIG walk on the device (csrc/fig_core.h; include/dabx.h "The FIC followed on the device").

Models.  For the configuration (FIG 0/0 .. 0/3, both swap rules) the model is the library's own host decoder, dabx_fibdec (dx.FibDecoder) fed
the same FIBs: fibdec_row() presents it like a row of dx.fig_walk_device.  For the labels, the events, the guards and the counters it is
Model below: a Python restatement of the walk -- FibDecoder::process_FIB (fib_decoder.cpp:59-106), the library's walk_fib for FIG 0
(csrc/fib.cpp:66-179, cited by line), _process_Fig1 / _extract_character_set_label for the labels (fib_decoder_fig1.cpp:18-152,
fib_decoder.cpp:744-778, charsets.h:50-55) and the event rules of include/dabx.h.  Model also notes every branch it takes (Model.reached), so
that a test can prove the inputs reach them all.

Inputs.  sequences() -> {name: (fibs [n, 32] uint8, crc_ok [n] uint8)}; PARITY names the ones that stay below every cap, for which dabx_fibdec
alone is a complete model of the configuration; STEPWISE the reconfiguration and restart cases that the GPU test checks after every FIB."""
import copy
import functools
import os
import sys

import numpy as np

import fic_cases as fc
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
from test_fib_reconfig import _layouts  # noqa: E402

MAX_SUB, MAX_COMP, MAX_PKT, MAX_LAB, RING = 64, dx.FIG_MAX_COMPONENTS, dx.FIG_MAX_PACKETS, dx.FIG_MAX_LABELS, dx.FIG_MAX_EVENTS
VALID_CHARSETS = (0, 6, 15)                          # charsets.h:45-55: EbuLatin, UnicodeUcs2, UnicodeUtf8
UEP = [(32, 5, 16), (32, 4, 21), (32, 3, 24), (32, 2, 29), (32, 1, 35), (48, 5, 24), (48, 4, 29), (48, 3, 35), (48, 2, 42), (48, 1, 52), (56, 5, 29),
       (56, 4, 35), (56, 3, 42), (56, 2, 52), (64, 5, 32), (64, 4, 42), (64, 3, 48), (64, 2, 58), (64, 1, 70), (80, 5, 40), (80, 4, 52), (80, 3, 58),
       (80, 2, 70), (80, 1, 84), (96, 5, 48), (96, 4, 58), (96, 3, 70), (96, 2, 84), (96, 1, 104), (112, 5, 58), (112, 4, 70), (112, 3, 84),
       (112, 2, 104), (128, 5, 64), (128, 4, 84), (128, 3, 96), (128, 2, 116), (128, 1, 140), (160, 5, 80), (160, 4, 104), (160, 3, 116),
       (160, 2, 140), (160, 1, 168), (192, 5, 96), (192, 4, 116), (192, 3, 140), (192, 2, 168), (192, 1, 208), (224, 5, 116), (224, 4, 140),
       (224, 3, 168), (224, 2, 208), (224, 1, 232), (256, 5, 128), (256, 4, 168), (256, 3, 192), (256, 2, 232), (256, 1, 280), (320, 5, 160),
       (320, 4, 208), (320, 2, 280), (384, 5, 192), (384, 3, 280), (384, 1, 416)]       # EN 300 401 table 8 (fib_table.h:44-117)
COUNTERS = tuple(k for k in dx.FIG_COUNTERS if k != "launches")


def bits(d, off, n):
    v = 0
    for i in range(n):
        v = (v << 1) | ((d[(off + i) >> 3] >> (7 - ((off + i) & 7))) & 1)
    return v


def cif_of_fib(i):
    return 4 * (i // 12) + (i % 12) // 3


class _Cfg:
    def __init__(self):
        self.sub, self.comp, self.pkt, self.gained = [], [], [], False

    def reset(self):
        self.sub, self.comp, self.pkt, self.gained = [], [], [], False

    def sizes(self):
        return [len(self.sub), len(self.comp), len(self.pkt)]


class Model:
    def __init__(self, reference_quirks=False):
        self.strict = bool(reference_quirks)
        self.cfg, self.cur = [_Cfg(), _Cfg()], 0
        self.cif_count = self.cif_hi = self.cif_lo = -1
        self.change_flags = self.occurrence = self.prev_change_flag = 0
        self.fibs, self.fig00_fib, self.last_change_fib = 0, -1, -1
        self.n_changes = self.n_restarts = 0
        self.labels, self.n_kind = [], {0: 0, 1: 0, 4: 0, 5: 0}
        self.events = []
        self.cnt = dict.fromkeys(COUNTERS, 0)
        self.reached = set()

    # ---- events (include/dabx.h: the record's head by the FIB being walked) -----------------------------------------------------------------
    def emit(self, kind, **payload):
        self.events.append(dict(kind=kind, epoch=self.n_restarts, frame=self.fibs // 12, fib=self.fibs, cif=cif_of_fib(self.fibs), **payload))
        self.cnt["events"] += 1

    def restart(self, why):                          # _restart_fib_decoding, fib_decoder.cpp:131-141: both configurations, the labels, _reset
        self.reached.add("restart_" + why)
        self.cfg[0].reset(); self.cfg[1].reset()
        self.labels, self.n_kind = [], {0: 0, 1: 0, 4: 0, 5: 0}
        self.cif_count = self.cif_hi = self.cif_lo = -1
        self.change_flags = self.occurrence = self.prev_change_flag = 0
        self.fig00_fib = -1
        self.n_restarts += 1
        self.cnt["restarts"] += 1
        self.emit(dx.FIG_RESTART)

    # ---- FIG 0 (csrc/fib.cpp, walk_fib) -----------------------------------------------------------------------------------------------------
    def fig0s0(self, d, ln):                         # fib.cpp:78-102
        flags = bits(d, 32, 2)
        self.cif_hi, self.cif_lo = bits(d, 35, 5), bits(d, 40, 8)
        self.cif_count = self.cif_hi * 250 + self.cif_lo
        self.occurrence = bits(d, 48, 8) if ln >= 6 else 0
        self.change_flags = flags
        self.fig00_fib = self.fibs
        self.cnt["fig00"] += 1
        if flags != 0 and self.prev_change_flag == 0:                                     # DABX_FIG_ANNOUNCE: 0 -> non-zero
            ahead = (self.occurrence - self.cif_lo) % 250 or 250                          # engine.cpp, dabx_follow_fic
            self.cnt["announces"] += 1
            self.reached.add("announce_flags_%d" % flags)
            self.emit(dx.FIG_ANNOUNCE, flags=flags, occurrence_change=self.occurrence, at_cif=cif_of_fib(self.fibs) + ahead)
        if flags == 0 and self.prev_change_flag != 0 and (self.prev_change_flag == 3 or not self.strict):   # fib.cpp:90
            cu, nx = self.cfg[self.cur], self.cfg[self.cur ^ 1]
            if not self.strict:                                                           # fib.cpp:91-96: carried over
                for tab in ("sub", "comp", "pkt"):
                    if not getattr(nx, tab):
                        setattr(nx, tab, list(getattr(cu, tab)))
                        if getattr(cu, tab):
                            self.reached.add("carry_over_" + tab)
            self.cur ^= 1
            self.cfg[self.cur ^ 1].reset()
            self.n_changes += 1
            self.cnt["swaps"] += 1
            self.last_change_fib = self.fibs
            self.reached.add("swap_after_flags_%d%s" % (self.prev_change_flag, "_strict" if self.strict else ""))
            n = self.cfg[self.cur].sizes()
            self.emit(dx.FIG_SWAP, n_changes=self.n_changes, n_subch=n[0], n_components=n[1], n_packets=n[2])
        elif flags == 0 and self.prev_change_flag != 0:
            self.reached.add("no_swap_after_flags_%d_strict" % self.prev_change_flag)
        self.prev_change_flag = flags

    def fig0s1(self, cfg, d, ln):                    # fib.cpp:103-137; True: restarted
        used = 2
        while used <= ln:
            o = used * 8
            if used + 3 > ln + 1:
                break
            sid = bits(d, o, 6)
            known = next((q for q in cfg.sub if q["subch_id"] == sid), None)
            if known:                                                                     # :110-113, by the STORED entry's form
                used += 3 if known["short_form"] else 4
                self.cnt["subch_known"] += 1
                self.reached.add("subch_known")
                continue
            q = dict(subch_id=sid, cu_start=bits(d, o + 6, 10))
            if bits(d, o + 16, 1) == 0:
                kbps, lvl, cus = UEP[bits(d, o + 18, 6)]
                q.update(short_form=1, kbps=kbps, prot_level=lvl, cu_size=cus)
                used += 3
                self.reached.add("subch_short_form")
            else:
                if used + 4 > ln + 1:
                    break
                option, lvl = bits(d, o + 17, 3), bits(d, o + 20, 2)
                q.update(cu_size=bits(d, o + 22, 10), short_form=0, prot_level=lvl)
                if option == 0:
                    q["kbps"] = q["cu_size"] // (12, 8, 6, 4)[lvl] * 8
                elif option == 1:
                    q["kbps"] = q["cu_size"] // (27, 21, 18, 15)[lvl] * 32
                    q["prot_level"] += 4
                else:
                    q["kbps"] = 0
                used += 4
                self.reached.add("subch_long_form")
            if q["cu_start"] + q["cu_size"] > 864:                                        # :131
                self.restart("beyond_864")
                return True
            if any(q["cu_start"] < k["cu_start"] + k["cu_size"] and k["cu_start"] < q["cu_start"] + q["cu_size"] for k in cfg.sub):     # :132-135
                self.restart("overlap")
                return True
            cfg.sub.append(q)
            cfg.gained = True
            self.cnt["subch_new"] += 1
        return False

    def fig0s2(self, cfg, d, ln, pd):                # fib.cpp:138-159
        used = 2
        while used <= ln:
            o = used * 8
            if (o + (32 if pd else 16)) // 8 + 1 > ln + 1:
                break
            sid = bits(d, o, 32 if pd else 16)
            o += 32 if pd else 16
            ncomp = bits(d, o + 4, 4)
            o += 8
            for c in range(ncomp):
                if (o + 16) // 8 > ln + 1:
                    break
                if any(k["sid"] == sid and k["idx"] == c for k in cfg.comp):
                    self.cnt["comp_known"] += 1
                    self.reached.add("comp_known")
                elif len(cfg.comp) >= MAX_COMP:                                           # guard (include/dabx.h)
                    self.cnt["over_components"] += 1
                    self.reached.add("over_components")
                else:
                    k = dict(sid=sid, idx=c, tmid=bits(d, o, 2), ascty=-1, subch_id=-1, scid=-1)
                    if k["tmid"] == 0:
                        k["ascty"], k["subch_id"] = bits(d, o + 2, 6), bits(d, o + 8, 6)
                    elif k["tmid"] == 1:
                        k["subch_id"] = bits(d, o + 8, 6)
                    elif k["tmid"] == 3:
                        k["scid"] = bits(d, o + 2, 12)
                    cfg.comp.append(k)
                    cfg.gained = True
                    self.cnt["comp_new"] += 1
                    self.reached.add("comp_tmid_%d" % k["tmid"])
                o += 16
            used = o // 8

    def fig0s3(self, cfg, d, ln):                    # fib.cpp:160-173
        used = 2
        while used + 5 <= ln + 1:
            o = used * 8
            scid = bits(d, o, 12)
            known = next((q for q in cfg.pkt if q["scid"] == scid), None)
            if known:
                used += 5 + (2 if known["caorg"] else 0)
                self.cnt["packet_known"] += 1
                self.reached.add("packet_known")
                continue
            k = dict(scid=scid, caorg=bits(d, o + 15, 1), dg_flag=bits(d, o + 16, 1), dscty=bits(d, o + 18, 6), subch_id=bits(d, o + 24, 6),
                     address=bits(d, o + 30, 10))
            used += 5 + (2 if k["caorg"] else 0)
            if used > ln + 1:
                break
            if len(cfg.pkt) >= MAX_PKT:                                                   # guard (include/dabx.h)
                self.cnt["over_packets"] += 1
                self.reached.add("over_packets")
                continue
            cfg.pkt.append(k)
            cfg.gained = True
            self.cnt["packet_new"] += 1
            self.reached.add("packet_caorg_%d" % k["caorg"])

    # ---- FIG 1 (fib_decoder_fig1.cpp) --------------------------------------------------------------------------------------------------------
    def fig1(self, d, ln):
        def short(why):
            self.cnt["label_short"] += 1
            self.reached.add("label_short_" + why)
        if ln < 1:
            return short("no_second_byte")
        charset, ext = d[1] >> 4, d[1] & 7                                                # fib_decoder.cpp:746, fib_decoder_fig1.cpp:20
        pd = scids = 0
        if ext in (0, 1):                                                                 # :49-96: identifier bits 16..31, label from bit 32
            if ln < 3:
                return short("no_identifier")
            ident, off = bits(d, 16, 16), 4
            key = (0, 0, 0, 0) if ext == 0 else (1, ident, 0, 0)                          # :59: the one ensemble label; :83 SId
        elif ext == 4:                                                                    # :99-125
            if ln < 2:
                return short("no_identifier")
            pd, scids = d[2] >> 7, d[2] & 15                                              # :102-103
            off = 7 if pd else 5                                                          # :105
            if ln < off - 1:
                return short("no_identifier")
            ident = bits(d, 24, 32 if pd else 16)                                         # :104
            key = (4, ident, pd, scids)                                                   # :107 (SId, SCIdS) + P/D
        elif ext == 5:                                                                    # :128-152
            if ln < 5:
                return short("no_identifier")
            ident, off = bits(d, 16, 32), 6
            key = (5, ident, 0, 0)
        else:                                                                             # :38-44
            self.cnt["label_other_ext"] += 1
            self.reached.add("label_other_ext")
            return
        if off + 18 > ln + 1:                                                             # guard: 16 bytes + CharFlagField inside the FIG
            return short("cut_by_length")
        if any(r["_key"] == key for r in self.labels):
            self.cnt["label_known"] += 1
            self.reached.add("label_known_1s%d" % ext)
            return
        if charset not in VALID_CHARSETS:                                                 # fib_decoder.cpp:748-752
            self.cnt["label_charset"] += 1
            self.reached.add("label_charset_%d" % charset)
            return
        if self.n_kind[ext] >= (1 if ext == 0 else MAX_LAB):                              # guard (include/dabx.h)
            self.cnt["over_labels"] += 1
            self.reached.add("over_labels_1s%d" % ext)
            return
        rec = dict(id=ident, char_flags=d[off + 16] << 8 | d[off + 17], kind=ext, charset=charset, label=bytes(d[off:off + 16]), pd=pd, scids=scids)
        self.labels.append(dict(rec, _key=key))
        self.n_kind[ext] += 1
        self.cnt["label_new"] += 1
        self.reached.add("label_new_1s%d_charset_%d%s" % (ext, charset, "_pd_%d" % pd if ext == 4 else ""))
        if self.n_restarts:
            self.reached.add("label_new_after_restart")
        self.emit(dx.FIG_LABEL_EVENT, label=rec)

    # ---- one FIB (fib_decoder.cpp:59-106; fib.cpp:66-179, dabx_fibdec_process) -----------------------------------------------------------------
    def walk(self, fib, crc_ok):
        fib = bytes(bytearray(fib))
        if not crc_ok:
            self.cnt["fibs_bad"] += 1
            self.reached.add("fib_bad_crc")
        else:
            self.cnt["fibs_good"] += 1
            p = 0
            while p < 30:
                typ, ln = fib[p] >> 5, fib[p] & 0x1F
                if typ == 7 and ln == 0x1F:
                    self.cnt["end_markers"] += 1
                    self.reached.add("end_marker_at_%s" % (p if p in (0, 29) else "middle"))
                    break
                if p + 1 + ln > 30:
                    self.cnt["fig_overrun"] += 1
                    self.reached.add("fig_overrun_type_%d" % typ)
                    break
                self.cnt["figs"] += 1
                d = fib[p:]
                restarted = False
                if typ == 0 and ln >= 1:
                    ext, pd, cn = d[1] & 0x1F, (d[1] >> 5) & 1, (d[1] >> 7) & 1
                    cfg = self.cfg[self.cur if cn == 0 else self.cur ^ 1]
                    if ext == 0 and ln >= 5:
                        self.reached.add("fig00_%s" % ("first" if p == 0 else "last" if p + 1 + ln == 30 or fib[p + 1 + ln] == 0xFF else "inside"))
                        self.fig0s0(d, ln)
                    elif ext == 1:
                        self.reached.add("fig01_cn_%d" % cn)
                        restarted = self.fig0s1(cfg, d, ln)
                    elif ext == 2:
                        self.reached.add("fig02_cn_%d_pd_%d" % (cn, pd))
                        self.fig0s2(cfg, d, ln, pd)
                    elif ext == 3:
                        self.reached.add("fig03_cn_%d" % cn)
                        self.fig0s3(cfg, d, ln)
                    else:
                        self.cnt["fig0_other_ext"] += 1
                        self.reached.add("fig0_other_ext")
                elif typ == 1:
                    self.fig1(d, ln)
                elif typ != 0:
                    self.cnt["fig_other_type"] += 1
                    self.reached.add("fig_type_%d" % typ)
                else:
                    self.cnt["fig0_other_ext"] += 1
                if restarted:
                    break
                p += ln + 1
            else:
                self.reached.add("fib_full")
        if self.fibs % 12 == 11:                                                          # DABX_FIG_TABLE: per frame and configuration that gained
            for k in range(2):
                c = self.cfg[self.cur ^ k]
                if c.gained:
                    n = c.sizes()
                    self.reached.add("table_event_%s" % ("next" if k else "current"))
                    self.emit(dx.FIG_TABLE, next=k, n_subch=n[0], n_components=n[1], n_packets=n[2])
                    c.gained = False
        self.fibs += 1

    def feed(self, fibs, crc):
        for f, ok in zip(fibs, crc):
            self.walk(f, ok)
        return self

    # ---- presented like a row of dx.fig_walk_device ---------------------------------------------------------------------------------------------
    def info(self):
        return dict(fibs_processed=self.fibs, fig00_fib=self.fig00_fib, last_change_fib=self.last_change_fib, cif_count=self.cif_count,
                    cif_count_hi=self.cif_hi, cif_count_lo=self.cif_lo, change_flags=self.change_flags, occurrence_change=self.occurrence,
                    n_changes=self.n_changes, n_restarts=self.n_restarts)

    def subch(self, k):                              # fib.cpp:181-192, table_out: the dab_plus join
        c = self.cfg[self.cur ^ k]
        out = []
        for q in c.sub:
            hit = next((x for x in c.comp if x["tmid"] == 0 and x["subch_id"] == q["subch_id"]), None)
            out.append(dict(q, dab_plus=-1 if hit is None else int(hit["ascty"] == 63)))
        return out

    def packets(self, k):                            # fib.cpp:259-271: the sid join
        c = self.cfg[self.cur ^ k]
        return [(q["scid"], q["subch_id"], q["address"], q["dscty"], q["dg_flag"],
                 next((x["sid"] for x in c.comp if x["tmid"] == 3 and x["scid"] == q["scid"]), 0)) for q in c.pkt]

    def follow(self, frames_fed):                    # engine.cpp, dabx_follow_fic
        out = dict(pending=0, n_changes=self.n_changes, frames_missed=0, at_cif=-1, last_change_cif=-1, frames_fed=frames_fed)
        if self.last_change_fib >= 0:
            out["last_change_cif"] = cif_of_fib(self.last_change_fib)
        if self.change_flags != 0 and self.fig00_fib >= 0:
            out["pending"] = 1
            out["at_cif"] = cif_of_fib(self.fig00_fib) + ((self.occurrence - self.cif_lo) % 250 or 250)
        return out

    def row(self):
        return dict(info=self.info(), n_tab=[self.cfg[self.cur].sizes(), self.cfg[self.cur ^ 1].sizes()], subch=[self.subch(0), self.subch(1)],
                    packets=[self.packets(0), self.packets(1)], labels=[{k: v for k, v in r.items() if k != "_key"} for r in self.labels],
                    stats=dict(self.cnt), n_events=len(self.events), events=copy.deepcopy(self.events[-RING:]))


def plain(row):
    """a row of dx.fig_walk_device / dx.FigHostDecoder.read as Model.row gives one"""
    return dict(info=row["info"], n_tab=row["n_tab"], subch=row["subch"], packets=[[tuple(int(v) for v in q) for q in p] for p in row["packets"]],
                labels=row["labels"], stats={k: row["stats"][k] for k in COUNTERS}, n_events=row["n_events"], events=row["events"])


def fibdec_row(d):
    """a dx.FibDecoder as the configuration part of a row: info, the sub-channel tables with their join, the packet components with theirs"""
    return dict(info=d.info(), subch=[[dx._subch_dict(q) for q in d.subchannels(next=bool(k))] for k in range(2)],
                packets=[[tuple(int(v) for v in q) for q in d.packet_components(next=bool(k))] for k in range(2)])


def config_part(row):
    return dict(info=row["info"], subch=row["subch"], packets=row["packets"])


# ---- FIGs ---------------------------------------------------------------------------------------------------------------------------------------
def label16(text):
    return text.encode("latin-1").ljust(16)[:16]


def fig1(ext, ident, text, charset=0, flags=0xFF00, length=None, oe=0):
    """FIG 1/ext with its identifier field (bytes) in front of the 16 label bytes and the flag field; length: the header's, when it lies"""
    body = bytes([(charset << 4) | (oe << 3) | ext]) + bytes(ident) + label16(text) + flags.to_bytes(2, "big")
    return bytes([0x20 | (len(body) if length is None else length)]) + body


def fig1s0(eid, text, **kw):
    return fig1(0, eid.to_bytes(2, "big"), text, **kw)


def fig1s1(sid, text, **kw):
    return fig1(1, sid.to_bytes(2, "big"), text, **kw)


def fig1s4(pd, scids, sid, text, **kw):
    return fig1(4, bytes([(pd << 7) | scids]) + sid.to_bytes(4 if pd else 2, "big"), text, **kw)


def fig1s5(sid, text, **kw):
    return fig1(5, sid.to_bytes(4, "big"), text, **kw)


def fibs_of(cifs):
    """[[FIG bytes, ...] per CIF] -> (fibs [3 n, 32], crc_ok all good): ds.pack_fibs puts a CIF's FIGs into its three FIBs, in order"""
    fibs = np.concatenate([ds.pack_fibs(list(figs)).reshape(3, 32) for figs in cifs])
    return fibs, np.ones(len(fibs), np.uint8)


def one_fib(*figs, fill=0x00):
    return fc.make_fib(b"".join(figs), fill=fill)


def _chunks(items, first, rest):
    out, k = [], first
    items = list(items)
    while items:
        out.append(items[:k]); items = items[k:]; k = rest
    return out


# ---- sequences --------------------------------------------------------------------------------------------------------------------------------
ENSEMBLE_LABEL = "Graft Ensemble"
PACKET_SERVICE = (0xE1D31234, [0x123, 0x456])


def ensemble18_cifs(n_cifs=40, cif_start=100):
    """18 sub-channels (17 audio services, one of them described in the short form; the last sub-channel carries a packet-mode data service
    of two components) with every label: FIG 0/1 on CIF 0 of four, FIG 0/2 on CIFs 1 and 3, FIG 0/3 and the labels on CIFs 2 and 3."""
    sub = ds.default_subchannels(18, 32)
    sub[16] = ds.SubCh(16, 16 * 24, 24, 32, 3, 1)   # UEP 32 kbit/s level 3: 24 CU
    audio = sub[:17]
    labels = [fig1s0(0x10F2, ENSEMBLE_LABEL)] + [fig1s1(0x1000 + c.subch_id, "Service %02d" % c.subch_id, charset=(0, 15, 6)[c.subch_id % 3]) for c in audio]
    labels += [fig1s5(PACKET_SERVICE[0], "Data service"), fig1s4(1, 1, PACKET_SERVICE[0], "Data comp 1"), fig1s4(0, 2, 0x1003, "Audio comp 2")]
    f03 = ds.fig03_bytes([(0x123, 17, 5, 60, 0, None), (0x456, 17, 9, 5, 1, 0xBEEF)])
    cifs, nl = [], 0
    for q in range(n_cifs):
        f00 = ds.fig00_bytes(cif_start + q)
        ph = q % 4
        if ph == 0:
            figs = [f00] + [ds.fig01_bytes(ch) for ch in _chunks(sub, 5, 7)]
        elif ph == 1:
            figs = [f00] + [ds.fig02_bytes(ch) for ch in _chunks(audio[:14], 4, 5)]
        elif ph == 2:
            figs = [f00, f03, labels[nl % len(labels)], labels[(nl + 1) % len(labels)]]
            nl += 2
        else:
            figs = [f00, ds.fig02_bytes(audio[14:]), labels[nl % len(labels)], ds.fig02_packet_bytes([PACKET_SERVICE], pd=1)]
            nl += 1
        cifs.append(figs)
    return cifs


def reconf_cifs(flags, clear_first, n_cifs=40, switch=28, announce=8, cif_start=4990):
    """Layout a, an announcement with the given change flags from CIF `announce` (the next configuration's FIG 0/1 with flags 1 and 3, its
    FIG 0/2 with flags 2 and 3), layout b from CIF `switch` on.  clear_first: the FIG 0/0 of every CIF is the first FIG of its FIB, otherwise
    the last one (behind that CIF's first table FIG)."""
    a, b = _layouts()
    cifs = []
    for q in range(n_cifs):
        ann = announce <= q < switch
        cur = a if q < switch else b
        f00 = ds.fig00_bytes(cif_start + q, change_flags=flags if ann else 0, occurrence=(cif_start + switch) % 250)
        ph = q % 4
        nxt = ann and ph >= 2
        if ph % 2 == 0:
            tabs = [ds.fig01_bytes(ch, 1 if nxt and flags & 1 else 0) for ch in _chunks(b if nxt and flags & 1 else cur, 4, 7)]
        else:
            tabs = [ds.fig02_bytes(ch, 1 if nxt and flags & 2 else 0) for ch in _chunks(b if nxt and flags & 2 else cur, 4, 5)]
        cifs.append([f00] + tabs if clear_first else tabs[:1] + [f00] + tabs[1:])
    return cifs


def restart_cifs():
    """a label, a restart (a sub-channel that overlaps a known one), another label, then the first label again: filed and reported twice;
    later a restart through a sub-channel beyond 864 CU while an announcement is pending"""
    a, _ = _layouts()
    la, lb = fig1s1(0x1001, "First label"), fig1s1(0x1002, "Second label")
    clash = ds.SubCh(9, 40, 48, 64, 2, 0)           # overlaps sub-channels 0 and 1 of layout a
    beyond = ds.SubCh(10, 840, 48, 64, 2, 0)        # 840 + 48 > 864
    cifs = []
    for q in range(40):
        f00 = ds.fig00_bytes(200 + q, change_flags=1 if 14 <= q < 18 else 0, occurrence=240)
        figs = [f00, ds.fig01_bytes(a[:4]), ds.fig01_bytes(a[4:])] if q % 2 == 0 else [f00, ds.fig02_bytes(a[:4]), ds.fig02_bytes(a[4:])]
        if q == 2:
            figs = [f00, la]
        if q == 5:
            figs = [ds.fig01_bytes([clash]), lb, f00]                       # the label behind the restart, in the same FIB, is not evaluated
        if q == 6:
            figs = [f00, lb]
        if q == 7:
            figs = [f00, la, fig1s0(0x10F2, ENSEMBLE_LABEL)]
        if q == 16:
            figs = [f00, ds.fig01_bytes([beyond], 1), lb]
        if q == 20:
            figs = [f00, la, lb]
        cifs.append(figs)
    return cifs


def label_fibs():
    """single FIBs around FIG 1: every charset verdict, every way a label can be cut, keys sent twice, the other extensions"""
    out = [one_fib(fig1s0(0x1234, "Ensemble one")), one_fib(fig1s0(0x4321, "Ensemble two"))]                       # the second is "known"
    for cs in (0, 6, 15, 1, 4, 14):
        out.append(one_fib(fig1s1(0x2000 + cs, "charset %d" % cs, charset=cs)))
    out.append(one_fib(fig1s1(0x2001, "again, invalid")))                                                          # charset 1 was not filed: filed now
    out.append(one_fib(fig1s1(0x2000, "same key, new text")))                                                      # known
    out.append(one_fib(fig1s1(0x2000, "bad charset known", charset=4)))                                            # known comes first
    out += [one_fib(fig1s4(0, 3, 0x3000, "comp pd 0")), one_fib(fig1s4(1, 3, 0x3000, "comp pd 1")), one_fib(fig1s4(0, 4, 0x3000, "comp scids 4")),
            one_fib(fig1s4(1, 3, 0x3000, "comp pd 1 again")), one_fib(fig1s5(0x3000, "data service")), one_fib(fig1s5(0x3000, "data again"))]
    out.append(one_fib(fig1s1(0x2100, "two in one", oe=1)[:22], bytes([0x42, 0xA5, 0xA5])))                        # a label and a FIG to step over
    # cut by the FIG's own length: the header says less than the label needs (what follows is walked as FIGs: 0xFF ends that)
    for ln in (0, 1, 2, 3, 20):
        out.append(one_fib(fig1s1(0x2200 + ln, "cut by length", length=ln)[:1 + ln], fill=0xFF))
    out.append(one_fib(fig1s4(1, 1, 0x2300, "cut pd 1", length=23)[:24], fill=0xFF))                                 # 1/4 P/D 1 needs 24
    out.append(one_fib(fig1s4(1, 1, 0x2300, "cut pd 1", length=4)[:5], fill=0xFF))
    out.append(one_fib(fig1s4(0, 1, 0x2301, "cut pd 0", length=21)[:22], fill=0xFF))
    out.append(one_fib(fig1s5(0x2302, "cut 1/5", length=22)[:23], fill=0xFF))
    out.append(one_fib(fig1s5(0x2302, "cut 1/5", length=4)[:5], fill=0xFF))
    out.append(one_fib(fig1s0(0x2303, "cut 1/0", length=20)[:21], fill=0xFF))
    out.append(one_fib(fig1s1(0x2304, "exactly fits", length=21)))                                                  # the shortest that holds one
    # cut by byte 30: the FIG starts so late that its length runs past the data field
    out.append(one_fib(fc._skip(9), fig1s1(0x2400, "cut by byte 30")[:21]))
    out.append(one_fib(fc._skip(8), fig1s1(0x2401, "ends at byte 30")))                                             # 8 + 22 = 30: filed
    for ext in (2, 3, 6, 7):
        out.append(one_fib(fig1(ext, b"\x12\x34", "other extension")))
    fibs = np.stack(out)
    return fibs, np.ones(len(fibs), np.uint8)


def marker_fibs():
    """end markers at byte 0, 29 and in the middle, FIGs of types 2..6 to step over, FIGs running past byte 30, FIG 0 of other extensions"""
    out = [fc.FILLER, one_fib(fc._skip(29)), fc.make_fib(fc._skip(29) + b"\xFF"), one_fib(fc._skip(11), fc._skip(7, 5))]
    out += [one_fib(fc._skip(4, t), ds.fig00_bytes(300 + t)) for t in range(2, 8)]
    out += [one_fib(bytes([0x03, 0x05, 1, 2]), bytes([0x02, 0x0D, 7])), fc.make_fib(bytes([0x00] * 30), pad=False)]   # FIG 0/5, 0/13; 30 FIGs of length 0
    out += [one_fib(fc._skip(20), bytes([0x0C, 0x01]) + bytes(8)), one_fib(fc._skip(25), bytes([0x25, 0x01])), fc.make_fib(fc._skip(30))]
    out += [f for _, f in fc.crafted_singles()]
    fibs = np.stack(out)
    return fibs, np.ones(len(fibs), np.uint8)


def cap_cifs():
    """every table one entry past its cap: 257 service components, 65 packet components, 65 labels of each kind (and a second ensemble label)"""
    cifs, q = [], 0
    comps = [(0x4000 + i, [0x800 + i]) for i in range(MAX_COMP + 1)]
    for ch in _chunks(comps, 5, 5):
        cifs.append([ds.fig00_bytes(q), ds.fig02_packet_bytes(ch)]); q += 1
    pk = [(0x800 + i, i % 64, i, 60, 0, None if i % 3 else 0x1111) for i in range(MAX_PKT + 1)]
    for ch in _chunks(pk, 3, 3):
        cifs.append([ds.fig00_bytes(q), ds.fig03_bytes(ch)]); q += 1
    labs = [fig1s0(1, "one"), fig1s0(2, "two")]
    for i in range(MAX_LAB + 1):
        labs += [fig1s1(0x5000 + i, "s%d" % i), fig1s4(i & 1, i % 16, 0x6000 + i, "c%d" % i), fig1s5(0x70000000 + i, "d%d" % i)]
    for ch in _chunks(labs, 3, 3):
        cifs.append(ch); q += 1
    cifs.append([ds.fig02_packet_bytes(comps[-2:]), ds.fig03_bytes(pk[-2:]), labs[-1]])       # the dropped ones again: dropped again, not "known"
    return cifs


@functools.lru_cache(maxsize=None)
def sequences():
    out = {"ensemble18": fibs_of(ensemble18_cifs())}
    for flags in (1, 2, 3):
        for first in (True, False):
            out["reconf_flags_%d_fig00_%s" % (flags, "first" if first else "last")] = fibs_of(reconf_cifs(flags, first))
    out["restart_labels"] = fibs_of(restart_cifs())
    out["labels"] = label_fibs()
    out["markers"] = marker_fibs()
    out["caps"] = fibs_of(cap_cifs())
    # bad CRCs between good ones: the 18-sub-channel ensemble with every fifth FIB failing (some of them damaged as well)
    fibs, crc = (a.copy() for a in out["ensemble18"])
    crc[::5] = 0
    fibs[::10, 7] ^= 0x40
    out["bad_crc"] = (fibs, crc)
    rnd = np.stack(fc.random_fibs() + fc.sparse_fibs())                                     # 2 000 random-byte FIBs + 1 000 thinned ones, CRC flag forced good
    out["random"] = (rnd, np.ones(len(rnd), np.uint8))
    return out


PARITY = ("ensemble18", "reconf_flags_1_fig00_first", "reconf_flags_1_fig00_last", "reconf_flags_2_fig00_first", "reconf_flags_2_fig00_last",
          "reconf_flags_3_fig00_first", "reconf_flags_3_fig00_last", "restart_labels", "labels", "markers", "bad_crc", "random")
STEPWISE = PARITY[1:8] + ("bad_crc",)                # 8 sequences: one launch of 8 decoders per prefix length

# every branch and guard the issue names, by Model.reached
REQUIRED = {
    "fib_bad_crc", "end_marker_at_0", "end_marker_at_29", "end_marker_at_middle", "fib_full", "fig_overrun_type_1", "fig_overrun_type_0",
    "fig_type_2", "fig_type_3", "fig_type_4", "fig_type_5", "fig_type_6", "fig_type_7", "fig0_other_ext",
    "fig00_first", "fig00_last", "fig01_cn_0", "fig01_cn_1", "fig02_cn_0_pd_0", "fig02_cn_1_pd_0", "fig02_cn_0_pd_1", "fig03_cn_0",
    "subch_known", "subch_long_form", "subch_short_form", "comp_known", "comp_tmid_0", "comp_tmid_3", "packet_known", "packet_caorg_0", "packet_caorg_1",
    "restart_overlap", "restart_beyond_864",
    "announce_flags_1", "announce_flags_2", "announce_flags_3", "swap_after_flags_1", "swap_after_flags_2", "swap_after_flags_3",
    "swap_after_flags_3_strict", "no_swap_after_flags_1_strict", "no_swap_after_flags_2_strict", "carry_over_sub", "carry_over_comp",
    "table_event_current", "table_event_next",
    "label_new_1s0_charset_0", "label_new_1s1_charset_0", "label_new_1s1_charset_6", "label_new_1s1_charset_15", "label_new_1s4_charset_0_pd_0",
    "label_new_1s4_charset_0_pd_1", "label_new_1s5_charset_0", "label_charset_1", "label_charset_4", "label_charset_14",
    "label_known_1s0", "label_known_1s1", "label_known_1s4", "label_known_1s5", "label_other_ext", "label_short_cut_by_length",
    "label_short_no_identifier", "label_short_no_second_byte", "label_new_after_restart",
    "over_components", "over_packets", "over_labels_1s1", "over_labels_1s4", "over_labels_1s5",
}


@functools.lru_cache(maxsize=None)
def model_rows(name, reference_quirks, stepwise=False):
    """the model's row after the whole sequence, or (stepwise) after every FIB; and what the model reached on the way"""
    fibs, crc = sequences()[name]
    m = Model(reference_quirks)
    if not stepwise:
        m.feed(fibs, crc)
        return m.row(), frozenset(m.reached)
    rows = []
    for f, ok in zip(fibs, crc):
        m.walk(f, ok)
        rows.append(m.row())
    return rows, frozenset(m.reached)
