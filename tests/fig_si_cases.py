"""Inputs and the model of the service information the device follows (csrc/fig_si_core.h; include/dabx.h "Service information").

Model.  SiModel extends the model of tests/fig_cases.py -- which decides cur, the swap and the restart -- by a Python restatement of the
reference's FIG 0/5, 0/7, 0/8, 0/9, 0/10, 0/13, 0/14, 0/17, 0/18 and 0/19 (fib_decoder_fig0.cpp:333-720, cited by line; _set_cluster and
_get_cluster fib_decoder.cpp:693-742), with unbounded tables but for the caps include/dabx.h states, the SI events, and the join of the service
directory (fib_decoder.cpp:219-290, :351-460).  It notes every branch it takes (reached).  row() presents it like a row of
dx.fig_si_walk_device.

Inputs.  sequences() -> {name: (fibs [n, 32], crc_ok [n])}; PARITY names the ones that stay below every cap."""
import copy
import functools

import numpy as np

import fic_cases as fc
import fig_cases as fg
from dabstar_amd import lib as dx
from fig_cases import bits, ds

MAX_GD, MAX_UA, MAX_LANG, MAX_PTY, MAX_CL, MAX_CM, LIST = (dx.FIG_MAX_GLOBAL_DEFS, dx.FIG_MAX_USER_APPS, dx.FIG_MAX_LANGUAGES, dx.FIG_MAX_PTYS,
                                                          dx.FIG_MAX_CLUSTERS, dx.FIG_MAX_CLUSTER_SIDS, dx.FIG_CLUSTER_LIST)
HAS, JOIN = dx.FIG_SI_HAS, dx.FIG_JOIN


class _SiCfg:
    def __init__(self):
        self.reset()

    def reset(self):                                 # FibConfigFig0::reset, fib_config_fig0.cpp:35-47 (+ the cluster table: include/dabx.h)
        self.gd, self.ua, self.fec, self.cl, self.cfg7, self.gained, self.n_cm = [], [], [], [], None, 0, 0


class SiModel(fg.Model):
    def __init__(self, reference_quirks=False):
        super().__init__(reference_quirks)
        self.si = [_SiCfg(), _SiCfg()]               # indexed like self.cfg
        self.lang, self.pty, self.lto, self.time = [], [], None, None
        self.sc = dict.fromkeys(dx.FIG_SI_COUNTERS, 0)

    # ---- what the walk of fig_cases decides -----------------------------------------------------------------------------------------------
    def restart(self, why):
        super().restart(why)
        self.si[0].reset(); self.si[1].reset()
        self.lang, self.pty, self.lto, self.time = [], [], None, None
        self.reached.add("si_restart")

    def fig0s0(self, d, ln):
        cur, n = self.cur, self.n_changes
        super().fig0s0(d, ln)
        if self.n_changes == n:
            return
        cu, nx = self.si[cur], self.si[cur ^ 1]                                          # fib_decoder_fig0.cpp:103-110
        if self.strict:                                                                  # the object that becomes current never had one filed
            if self.lang or self.pty or self.lto:
                self.reached.add("si_swap_strict_drops_current_tables")
            self.lang, self.pty, self.lto = [], [], None
        else:
            for tab in ("gd", "ua", "fec"):
                if not getattr(nx, tab):
                    setattr(nx, tab, copy.deepcopy(getattr(cu, tab)))
                    if getattr(cu, tab):
                        self.reached.add("si_carry_over_" + tab)
                else:
                    self.reached.add("si_next_brings_" + tab)
            if not nx.cl:
                nx.cl, nx.n_cm = copy.deepcopy(cu.cl), cu.n_cm
                if cu.cl:
                    self.reached.add("si_carry_over_cl")
            if nx.cfg7 is None:
                nx.cfg7 = cu.cfg7
            nx.gained |= cu.gained & (HAS["language"] | HAS["lto"] | HAS["pty"])
        cu.reset()

    def fig0s2(self, cfg, d, ln, pd):                # fig_cases' with P/S, P/D and the DSCTy of TMId 1 kept (csrc/fig_core.h, comp_info)
        n = len(cfg.comp)
        super().fig0s2(cfg, d, ln, pd)
        used = 2
        while used <= ln:                            # the same cursor again, for the fields the model of fig_cases does not keep
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
                for k in cfg.comp[n:]:
                    if k["sid"] == sid and k["idx"] == c and "ps" not in k:
                        k.update(ps=bits(d, o + 14, 1), pd=pd)
                        if k["tmid"] == 1:
                            k["ascty"] = bits(d, o + 2, 6)
                o += 16
            used = o // 8

    # ---- FIG 0/5 .. 0/19 ----------------------------------------------------------------------------------------------------------------------
    def outside(self, what):
        self.sc["outside"] += 1
        self.reached.add("outside_" + what)

    def s5(self, cur, d, ln):                        # :333-383
        used = 2
        while used <= ln:
            o = used * 8
            ls = bits(d, o, 1)
            size = 3 if ls else 2
            if used + size > ln + 1:
                return self.outside("0s5")
            if not ls:
                ident = probe = bits(d, o + 2, 6); language = bits(d, o + 8, 8)           # :343-346
            else:
                ident = bits(d, o + 4, 12); probe = ident & 0xFF; language = bits(d, o + 16, 8)     # :363-366, fib_config_fig0.h:242
            used += size
            if any(q[0] == ls and q[1] == probe for q in self.lang):
                self.sc["language_known"] += 1
                self.reached.add("language_known_ls_%d" % ls)
            elif len(self.lang) >= MAX_LANG:
                self.sc["over_languages"] += 1
                self.reached.add("over_languages")
            else:
                self.lang.append((ls, ident, language))
                cur.gained |= HAS["language"]
                self.sc["language_new"] += 1
                self.reached.add("language_new_ls_%d%s" % (ls, "_scid_above_255" if ls and ident > 255 else ""))

    def s7(self, cfg, d, ln, cn):                    # :386-406
        if 4 > ln + 1:
            return self.outside("0s7")
        if cfg.cfg7 is not None:
            self.sc["config_known"] += 1
            self.reached.add("config_known")
            return
        cfg.cfg7 = (bits(d, 16, 6), bits(d, 22, 10))
        cfg.gained |= HAS["config"]
        self.sc["config_new"] += 1
        self.reached.add("config_new_cn_%d" % cn)

    def s8(self, cfg, d, ln, pd, cn):                # :409-449
        used, sidb = 2, 4 if pd else 2
        while used <= ln:
            o = used * 8
            if used + sidb + 2 > ln + 1:
                return self.outside("0s8")
            sid = bits(d, o, 8 * sidb)
            o += 8 * sidb
            ext, scids, ls = bits(d, o, 1), bits(d, o + 4, 4), bits(d, o + 8, 1)
            size = sidb + (3 if ls else 2) + (1 if ext else 0)
            if used + size > ln + 1:
                return self.outside("0s8")
            q = dict(sid=sid, scids=scids, pd=pd, ls=ls, ext=ext, subch_id=-1 if ls else bits(d, o + 10, 6), scid=bits(d, o + 12, 12) if ls else -1)
            used += size
            if any(k["sid"] == sid and k["scids"] == scids for k in cfg.gd):             # :435
                self.sc["global_def_known"] += 1
                self.reached.add("global_def_known")
            elif len(cfg.gd) >= MAX_GD:
                self.sc["over_global_defs"] += 1
                self.reached.add("over_global_defs")
            else:
                cfg.gd.append(q)
                cfg.gained |= HAS["global_def"]
                self.sc["global_def_new"] += 1
                self.reached.add("global_def_new_ls_%d_ext_%d_pd_%d_cn_%d" % (ls, ext, pd, cn))

    def s9(self, cur, d, ln):                        # :452-479
        if self.lto is not None:
            self.sc["lto_known"] += 1
            self.reached.add("lto_known")
            return
        if 5 > ln + 1:
            return self.outside("0s9")
        lto = bits(d, 19, 5)
        self.lto = dict(lto_ext=bits(d, 16, 1), lto_minutes=(-lto if bits(d, 18, 1) else lto) * 30, ecc=bits(d, 24, 8), inter_table=bits(d, 32, 8))
        cur.gained |= HAS["lto"]
        self.sc["lto_new"] += 1
        self.reached.add("lto_new_%s" % ("negative" if bits(d, 18, 1) else "positive"))

    def s10(self, d, ln):                            # :481-514
        if 5 > ln + 1:
            return self.outside("0s10")
        flag = bits(d, 36, 1)
        if (8 if flag else 6) > ln + 1:
            return self.outside("0s10")
        utc = bits(d, 37, 27 if flag else 11)
        t = dict(mjd=bits(d, 17, 17), lsi=bits(d, 34, 1), utc_flag=flag)
        if flag:
            t.update(hour=utc >> 22 & 31, minute=utc >> 16 & 63, second=utc >> 10 & 63)   # fib_config_fig0.h:179
        else:
            t.update(hour=utc >> 6 & 31, minute=utc & 63, second=-1)                     # :178, :505
        self.time = t
        self.sc["time_set"] += 1
        self.reached.add("time_%s_form_%s_0s9" % ("long" if flag else "short", "after" if self.lto else "before"))
        if self.lto:                                                                     # :508-513
            self.emit(dx.FIG_TIME, mjd=t["mjd"], hour=t["hour"], minute=t["minute"], second=t["second"], lto_minutes=self.lto["lto_minutes"],
                      utc_flag=flag, lsi=t["lsi"])

    def s13(self, cur, cfg, d, ln, pd, cn):          # :517-560
        used, sidb = 2, 4 if pd else 2
        while used <= ln:
            o = used * 8
            if used + sidb + 1 > ln + 1:
                return self.outside("0s13")
            sid = bits(d, o, 8 * sidb)
            o += 8 * sidb
            scids = bits(d, o, 4)
            known = next((k for k in cur.ua if k["sid"] == sid and k["scids"] == scids), None)     # :525: the CURRENT configuration
            if known:
                used += known["size_bits"] // 8                                           # :554
                self.sc["user_apps_known"] += 1
                self.reached.add("user_apps_known")
                continue
            n = bits(d, o + 4, 4)
            o += 8
            if n > 6:                                                                     # :532-536
                n = 6
                self.sc["user_apps_clamped"] += 1
                self.reached.add("user_apps_clamped")
            apps = []
            for _ in range(n):
                if o // 8 + 2 > ln + 1:
                    return self.outside("0s13")
                typ, alen = bits(d, o, 11), bits(d, o + 11, 5)
                if o // 8 + 2 + alen > ln + 1:
                    return self.outside("0s13")
                apps.append((typ, alen, bytes(d[o // 8 + 2:o // 8 + 2 + min(alen, 4)]).ljust(4, b"\0")))
                o += 16 + 8 * alen
            q = dict(sid=sid, scids=scids, pd=pd, size_bits=o - used * 8, apps=apps)      # :546
            used = o // 8
            if len(cfg.ua) >= MAX_UA:
                self.sc["over_user_apps"] += 1
                self.reached.add("over_user_apps")
                continue
            cfg.ua.append(q)                                                              # :547: the C/N configuration
            cfg.gained |= HAS["user_apps"]
            self.sc["user_apps_new"] += 1
            self.reached.add("user_apps_new_%d_apps_pd_%d_cn_%d" % (n, pd, cn))

    def s14(self, cfg, d, ln, cn):                   # :563-583
        for used in range(2, ln + 1):
            ident = bits(d, used * 8, 6)
            if any(q[0] == ident for q in cfg.fec):
                self.sc["fec_known"] += 1
                self.reached.add("fec_known")
            else:
                cfg.fec.append((ident, bits(d, used * 8 + 6, 2)))
                cfg.gained |= HAS["fec"]
                self.sc["fec_new"] += 1
                self.reached.add("fec_new_cn_%d" % cn)

    def s17(self, cur, d, ln):                       # :585-613
        for off in range(16, ln * 8, 32):
            if off // 8 + 4 > ln + 1:
                return self.outside("0s17")
            sid = bits(d, off, 16)
            if any(q[0] == sid for q in self.pty):
                self.sc["pty_known"] += 1
                self.reached.add("pty_known")
            elif len(self.pty) >= MAX_PTY:
                self.sc["over_ptys"] += 1
                self.reached.add("over_ptys")
            else:
                self.pty.append((sid, bits(d, off + 16, 1), bits(d, off + 27, 5)))
                cur.gained |= HAS["pty"]
                self.sc["pty_new"] += 1
                self.reached.add("pty_new")

    def cluster(self, cfg, ident):                   # _get_cluster, fib_decoder.cpp:722-742 -> (slot, made now)
        for i, c in enumerate(cfg.cl):
            if c["cluster_id"] == ident:
                return i, False
        if len(cfg.cl) >= MAX_CL:
            self.sc["cluster_fallback"] += 1
            self.reached.add("cluster_fallback")
            return 0, False
        cfg.cl.append(dict(cluster_id=ident, flags=0, announcing=0, sids=[]))
        cfg.gained |= HAS["cluster"]
        self.sc["cluster_new"] += 1
        return len(cfg.cl) - 1, True

    def s18(self, cfg, d, ln, cn):                   # :616-647, _set_cluster fib_decoder.cpp:693-720
        bo = 16
        while bo <= ln * 8:
            by = bo // 8
            if by + 5 > ln + 1:
                return self.outside("0s18")
            sid, asu, nr = bits(d, bo, 16), bits(d, bo + 16, 16), bits(d, bo + 37, 3)
            if by + 5 + nr > ln + 1:
                return self.outside("0s18")
            for i in range(nr):
                ident = d[by + 5 + i]
                if ident == 0:                                                            # :635
                    self.sc["cluster_zero"] += 1
                    self.reached.add("cluster_zero")
                    continue
                slot, _ = self.cluster(cfg, ident)
                c = cfg.cl[slot]
                c["flags"] = asu                                                          # :707-710
                if sid in c["sids"]:
                    self.sc["cluster_sid_known"] += 1
                    self.reached.add("cluster_sid_known")
                elif cfg.n_cm >= MAX_CM:
                    self.sc["over_cluster_sids"] += 1
                    self.reached.add("over_cluster_sids")
                else:
                    c["sids"].append(sid)
                    cfg.n_cm += 1
                    cfg.gained |= HAS["cluster"]
                    self.sc["cluster_sid_new"] += 1
                    self.reached.add("cluster_sid_new_cn_%d" % cn)
            bo += 40 + 8 * nr

    def s19(self, cfg, d, ln, cn):                   # :650-720
        bo = 16
        while bo <= ln * 8:
            by = bo // 8
            if by + 4 > ln + 1:
                return self.outside("0s19")
            ident, asw, region, subch = bits(d, bo, 8), bits(d, bo + 8, 16), bits(d, bo + 25, 1), bits(d, bo + 26, 6)
            bo += 32
            if region:                                                                    # :671-677
                if by + 5 > ln + 1:
                    return self.outside("0s19")
                bo += 8
                self.reached.add("asw_region")
            slot, fresh = self.cluster(cfg, ident)                                        # :684
            if fresh:
                self.sc["asw_unknown"] += 1
                self.reached.add("asw_unknown_cluster")
            c = cfg.cl[slot]
            payload = dict(cluster=ident, flags=asw, subch_id=subch, n_services=len(c["sids"]), next=cn)
            if c["flags"] & asw:                                                          # :691-704
                c["announcing"] += 1
                self.sc["asw_count"] += 1
                if c["announcing"] == 5:
                    self.sc["asw_start"] += 1
                    self.reached.add("asw_start")
                    self.emit(dx.FIG_ANNOUNCE_START, **payload)
                elif c["announcing"] > 5:
                    self.reached.add("asw_goes_on")
            elif c["announcing"] > 0:                                                     # :705-717
                self.reached.add("asw_stop_%s" % ("announced" if c["announcing"] >= 5 else "early"))
                c["announcing"] = 0
                self.sc["asw_stop"] += 1
                self.emit(dx.FIG_ANNOUNCE_STOP, **payload)
            else:
                self.reached.add("asw_idle")

    def si_walk(self, d, ln, ext, pd, cn):           # _process_Fig0, :20-67
        cur, cfg = self.si[self.cur], self.si[self.cur if cn == 0 else self.cur ^ 1]
        if ext == 5: self.s5(cur, d, ln)
        elif ext == 7: self.s7(cfg, d, ln, cn)
        elif ext == 8: self.s8(cfg, d, ln, pd, cn)
        elif ext == 9: self.s9(cur, d, ln)
        elif ext == 10: self.s10(d, ln)
        elif ext == 13: self.s13(cur, cfg, d, ln, pd, cn)
        elif ext == 14: self.s14(cfg, d, ln, cn)
        elif ext == 17: self.s17(cur, d, ln)
        elif ext == 18: self.s18(cfg, d, ln, cn)
        elif ext == 19: self.s19(cfg, d, ln, cn)
        else:
            self.reached.add("fig0_ext_not_followed")
            return
        self.sc["si_figs"] += 1

    # ---- one FIB: fig_cases' walk with the SI walk where it counts fig0_other_ext, and the SI_TABLE events behind the TABLE events -----------------
    def walk(self, fib, crc_ok):
        fib = bytes(bytearray(fib))
        if not crc_ok:
            self.cnt["fibs_bad"] += 1
        else:
            self.cnt["fibs_good"] += 1
            p = 0
            while p < 30:
                typ, ln = fib[p] >> 5, fib[p] & 0x1F
                if typ == 7 and ln == 0x1F:
                    self.cnt["end_markers"] += 1
                    break
                if p + 1 + ln > 30:
                    self.cnt["fig_overrun"] += 1
                    break
                self.cnt["figs"] += 1
                d = fib[p:]
                restarted = False
                if typ == 0 and ln >= 1:
                    ext, pd, cn = d[1] & 0x1F, (d[1] >> 5) & 1, (d[1] >> 7) & 1
                    cfg = self.cfg[self.cur if cn == 0 else self.cur ^ 1]
                    if ext == 0 and ln >= 5:
                        self.fig0s0(d, ln)
                    elif ext == 1:
                        restarted = self.fig0s1(cfg, d, ln)
                    elif ext == 2:
                        self.fig0s2(cfg, d, ln, pd)
                    elif ext == 3:
                        self.fig0s3(cfg, d, ln)
                    else:
                        self.cnt["fig0_other_ext"] += 1
                        self.si_walk(d, ln, ext, pd, cn)
                elif typ == 1:
                    self.fig1(d, ln)
                elif typ != 0:
                    self.cnt["fig_other_type"] += 1
                else:
                    self.cnt["fig0_other_ext"] += 1
                if restarted:
                    break
                p += ln + 1
        if self.fibs % 12 == 11:
            for k in range(2):
                c = self.cfg[self.cur ^ k]
                if c.gained:
                    n = c.sizes()
                    self.emit(dx.FIG_TABLE, next=k, n_subch=n[0], n_components=n[1], n_packets=n[2])
                    c.gained = False
            for k in range(2):
                c = self.si[self.cur ^ k]
                if c.gained:
                    self.reached.add("si_table_event_%s" % ("next" if k else "current"))
                    self.emit(dx.FIG_SI_TABLE, next=k, mask=c.gained, n_global_defs=len(c.gd), n_user_apps=len(c.ua), n_fec=len(c.fec), n_clusters=len(c.cl),
                              n_cluster_sids=c.n_cm, n_languages=0 if k else len(self.lang), n_ptys=0 if k else len(self.pty))
                    c.gained = 0
        self.fibs += 1

    # ---- the service directory (fib_decoder.cpp:219-290, :351-460) --------------------------------------------------------------------------------
    def label_of(self, kind, sid, scids=0):
        for r in self.labels:
            if r["kind"] == kind and r["id"] == sid and (kind != 4 or r["scids"] == scids):
                return {k: v for k, v in r.items() if k != "_key"}
        return None

    def directory(self, k):
        c, q = self.cfg[self.cur ^ k], self.si[self.cur ^ k]
        out = []
        for x in c.comp:
            sid, tmid, ps, pd = x["sid"], x["tmid"], x["ps"], x["pd"]
            r = dict(sid=sid, comp_idx=x["idx"], ps=ps, tmid=tmid, ty=-1, scids=-1, subch_id=-1, prot_level=-1, short_form=-1, cu_start=-1, cu_size=-1, kbps=-1,
                     packet_address=-1, scid=-1, language=-1, pty=-1, fec_scheme=0, dg_flag=-1, pd=pd, joined=0, reference_defined=0, apps=[], label=None)
            subch, pkt, gd = -1, None, None
            if tmid in (0, 1):
                subch, r["ty"] = x["subch_id"], x["ascty"]
                gd = next((g for g in q.gd if g["sid"] == sid and not g["ls"] and g["subch_id"] == subch), None)      # (extension, include/dabx.h)
            elif tmid == 3:
                r["scid"] = x["scid"]
                pkt = next((p for p in c.pkt if p["scid"] == x["scid"]), None)            # :362
                if pkt:
                    r["joined"] |= JOIN["packet"]
                    subch = pkt["subch_id"]
                    r.update(ty=pkt["dscty"], dg_flag=pkt["dg_flag"], packet_address=pkt["address"])
                gd = next((g for g in q.gd if g["sid"] == sid and g["ls"]), None)         # :379, fib_config_fig0.cpp:180-190: whatever its SCId
            if gd:
                r["joined"] |= JOIN["global_def"]
                r["scids"] = gd["scids"]
            sub = None
            if subch >= 0:
                r["subch_id"] = subch
                sub = next((s for s in c.sub if s["subch_id"] == subch), None)            # :234, :370
            if sub:
                r["joined"] |= JOIN["subch"]
                r.update(cu_start=sub["cu_start"], cu_size=sub["cu_size"], kbps=sub["kbps"], prot_level=sub["prot_level"], short_form=sub["short_form"])
            ua = next((u for u in q.ua if u["sid"] == sid and u["scids"] == gd["scids"]), None) if gd else None      # :387
            if ua:
                r["joined"] |= JOIN["user_apps"]
                r["apps"] = list(ua["apps"])
            if tmid == 3 and subch >= 0:
                f = next((f for f in q.fec if f[0] == subch), None)                       # :395, :408
                if f:
                    r["joined"] |= JOIN["fec"]
                    r["fec_scheme"] = f[1]
            lang = None
            if tmid == 3:
                lang = next((g for g in self.lang if g[0] == 1 and g[1] == (x["scid"] & 0xFF)), None)               # :396 through a u8
            elif subch >= 0:
                lang = next((g for g in self.lang if g[0] == 0 and g[1] == subch), None)  # :283
            if lang:
                r["joined"] |= JOIN["language"]
                r["language"] = lang[2]
            if tmid == 0:
                p = next((p for p in self.pty if p[0] == (sid & 0xFFFF)), None)           # :284
                if p:
                    r["joined"] |= JOIN["pty"]
                    r["pty"] = p[2]
            if ps:
                lab = self.label_of(1 if tmid == 0 else 5, sid)                           # :241, :443
            else:
                lab = self.label_of(4, sid, gd["scids"]) if gd else None                  # :426
            if lab:
                r["joined"] |= JOIN["label"]
                r["label"] = lab
            if tmid == 0:
                r["reference_defined"] = int(pd == 0 and sub is not None)                 # :224-228, :236-239
            elif tmid == 3:
                r["reference_defined"] = int(bool(pkt and sub and gd and ua and len(ua["apps"]) >= 1 and lab))      # :364-393, :436-456
            out.append(r)
        return out

    # ---- presented like a row of dx.fig_si_walk_device ------------------------------------------------------------------------------------------------
    def si_row(self):
        cf = [self.si[self.cur], self.si[self.cur ^ 1]]
        lto = self.lto or dict(lto_ext=0, lto_minutes=0, ecc=0, inter_table=0)
        t = self.time or dict(mjd=0, hour=0, minute=0, second=0, lsi=0, utc_flag=0)
        info = dict(has_config=[int(c.cfg7 is not None) for c in cf], n_services=[c.cfg7[0] if c.cfg7 else 0 for c in cf],
                    count=[c.cfg7[1] if c.cfg7 else 0 for c in cf], has_lto=int(self.lto is not None), lto_minutes=lto["lto_minutes"], ecc=lto["ecc"],
                    inter_table=lto["inter_table"], lto_ext=lto["lto_ext"], time_set=int(self.time is not None), mjd=t["mjd"], hour=t["hour"],
                    minute=t["minute"], second=t["second"], lsi=t["lsi"], utc_flag=t["utc_flag"], n_global_defs=[len(c.gd) for c in cf],
                    n_user_apps=[len(c.ua) for c in cf], n_fec=[len(c.fec) for c in cf], n_clusters=[len(c.cl) for c in cf],
                    n_cluster_sids=[c.n_cm for c in cf], n_languages=len(self.lang), n_ptys=len(self.pty))
        return dict(info=info, stats=dict(self.sc), global_defs=[copy.deepcopy(c.gd) for c in cf], user_apps=[copy.deepcopy(c.ua) for c in cf],
                    fec=[list(c.fec) for c in cf],
                    clusters=[[dict(cluster_id=x["cluster_id"], flags=x["flags"], announcing=x["announcing"], n_services=len(x["sids"]), sids=x["sids"][:LIST])
                               for x in c.cl] for c in cf],
                    languages=list(self.lang), ptys=list(self.pty))

    def row(self):
        return dict(super().row(), si=self.si_row(), dir=[self.directory(0), self.directory(1)])


def plain(row):
    """a row of dx.fig_si_walk_device / dx.FigSiHostDecoder.read as SiModel.row gives one"""
    return dict(fg.plain(row), si=row["si"], dir=row["dir"])


# ---- FIGs -----------------------------------------------------------------------------------------------------------------------------------------
def fig0(ext, body, cn=0, pd=0, oe=0, length=None):
    body = bytes([cn << 7 | oe << 6 | pd << 5 | ext]) + bytes(body)
    return bytes([len(body) if length is None else length]) + body


def e05(ident, language, long_form=False):
    return bytes([0x80 | 0x50 | ident >> 8, ident & 0xFF, language]) if long_form else bytes([ident, language])


def e08(sid, scids, subch=None, scid=None, ext=0, pd=0):
    out = sid.to_bytes(4 if pd else 2, "big") + bytes([ext << 7 | scids])
    out += bytes([subch]) if scid is None else bytes([0x80 | scid >> 8, scid & 0xFF])
    return out + (b"\x5A" if ext else b"")


def f09(half_hours, ecc, table, ext=0, **kw):
    return fig0(9, bytes([ext << 7 | (0x20 if half_hours < 0 else 0) | abs(half_hours), ecc, table]), **kw)


def f10(mjd, hour, minute, second=None, ms=0, lsi=0, **kw):
    if second is None:
        v = mjd << 14 | lsi << 13 | 0 << 11 | hour << 6 | minute                         # Rfu, MJD 17, LSI, Rfa, UTC flag 0, 11 bits
        return fig0(10, v.to_bytes(4, "big"), **kw)
    v = mjd << 30 | lsi << 29 | 1 << 27 | hour << 22 | minute << 16 | second << 10 | ms
    return fig0(10, v.to_bytes(6, "big"), **kw)


def e13(sid, scids, apps, pd=0, n=None):
    out = sid.to_bytes(4 if pd else 2, "big") + bytes([scids << 4 | (len(apps) if n is None else n)])
    for typ, data in apps:
        out += (typ << 5 | len(data)).to_bytes(2, "big") + bytes(data)
    return out


def e17(sid, code, sd=0):
    return sid.to_bytes(2, "big") + bytes([sd << 7, code])


def e18(sid, asu, clusters):
    return sid.to_bytes(2, "big") + asu.to_bytes(2, "big") + bytes([len(clusters)]) + bytes(clusters)


def e19(cluster, asw, subch, region=None, new=1):
    return bytes([cluster]) + asw.to_bytes(2, "big") + bytes([new << 7 | (0x40 if region is not None else 0) | subch]) + (bytes([region]) if region is not None else b"")


SLS, JOURNALINE, TPEG, SPI = 0x002, 0x44A, 0x004, 0x007       # TS 101 756 table 16


# ---- sequences --------------------------------------------------------------------------------------------------------------------------------------
def si_figs_ensemble18():
    """the service information of fig_cases' 18-sub-channel ensemble, every FIG type in both forms: one list of FIGs per SI CIF"""
    psid = fg.PACKET_SERVICE[0]
    audio = [0x1000 + i for i in range(17)]
    return [
        [fig0(7, bytes([18 << 2 | 0, 7])), f10(60000, 12, 34), f09(2, 0xE1, 1), f10(60000, 12, 35, 56, 789, lsi=1)],           # 0/10 before and after 0/9
        [fig0(5, b"".join(e05(i, 8 + i % 3) for i in range(9))), fig0(5, e05(0x023, 15, True) + e05(0x156, 9, True))],
        [fig0(8, b"".join(e08(s, 0, subch=s - 0x1000) for s in audio[:6])), fig0(8, e08(0x1003, 2, subch=3, ext=1) + e08(0x1002, 1, scid=0x456))],
        [fig0(8, e08(psid, 0, scid=0x123, pd=1) + e08(psid, 1, scid=0x456, ext=1, pd=1), pd=1), fig0(8, e08(0x1006, 0, subch=6), cn=1)],
        [fig0(13, e13(0x1000, 0, [(SLS, b"\x0C\x3C"), (SPI, b"")]) + e13(0x1001, 0, [])),
         fig0(13, e13(psid, 0, [(JOURNALINE, b"\x00\x00")], pd=1) + e13(psid, 1, [(TPEG, b"\x01\x02\x03\x04\x05\x06")], pd=1), pd=1)],
        [fig0(13, e13(0x1002, 0, [(SLS, b"\x0C\x3C"), (2, b"\x01"), (3, b""), (4, b"\x07\x08"), (5, b""), (6, b"\x09")])),
         fig0(14, bytes([17 << 2 | 1, 3 << 2 | 0])), fig0(14, bytes([17 << 2 | 2, 9 << 2 | 3]), cn=1)],
        [fig0(17, b"".join(e17(s, 1 + (s & 15), sd=s & 1) for s in audio[:6])), fig0(17, e17(0x1000, 31) + e17(0x1006, 10))],
        [fig0(18, e18(0x1000, 0x0003, [1, 2]) + e18(0x1001, 0x0002, [2, 0, 3])), fig0(18, e18(0x1002, 0x0002, [2]), pd=1), fig0(18, e18(0x1003, 0x0010, [9]), cn=1)],
        [fig0(7, bytes([19 << 2 | 1, 0x23]), cn=1), fig0(7, bytes([1, 2])), f09(-3, 0xE2, 2)],                                   # known 0/7, 0/9 read once
    ]


def announcement_cifs():
    """FIG 0/19 on cluster 2 (flags 0x0002 from 0/18): four matching FIGs, a pause, then five and more (start at the 5th), the stop, an early
    stop, a FIG with the region field, an unknown cluster (it gets an entry: asw_unknown) and a cluster the ASw flags do not meet"""
    on, off = fig0(19, e19(2, 0x0002, 5)), fig0(19, e19(2, 0x0000, 5))
    seq = [on] * 4 + [off] + [on] * 7 + [off, off] + [on, on, off] + [fig0(19, e19(2, 0x0002, 5, region=9) + e19(1, 0x0001, 6))] * 5
    seq += [fig0(19, e19(77, 0xFFFF, 1)), fig0(19, e19(77, 0xFFFF, 1)), fig0(19, e19(1, 0x0100, 6)), fig0(19, e19(9, 0x0010, 2), cn=1)]
    return [[g] for g in seq]


def si_ensemble_cifs(n=72):
    """fig_cases' ensemble with an SI CIF behind every MCI / label CIF; the announcements of announcement_cifs() from the second round on"""
    base, si, ann = fg.ensemble18_cifs(n_cifs=n // 2), si_figs_ensemble18(), announcement_cifs()
    cifs = []
    for q in range(n // 2):
        cifs.append(base[q])
        extra = ann[q - len(si)] if len(si) <= q < len(si) + len(ann) else []
        cifs.append([ds.fig00_bytes(5000 + q)] + si[q % len(si)] + extra)
    return cifs


def si_reconf_cifs(flags, n_cifs=40, switch=28, announce=8, cif_start=4990):
    """fig_cases' reconfiguration (layout a -> b) with SI in both configurations: the current one's 0/5, 0/7, 0/8, 0/9, 0/13, 0/14, 0/17 and
    0/18 throughout; while the change is announced the next one's 0/7 and 0/8 (so 0/13, 0/14 and the clusters are carried over under the
    default rule, and gone under the reference's)"""
    base = fg.reconf_cifs(flags, True, n_cifs, switch, announce, cif_start)
    cur = [fig0(7, bytes([8 << 2, 1])), fig0(8, e08(0x1000, 0, subch=0) + e08(0x1001, 0, subch=1)), fig0(13, e13(0x1000, 0, [(SLS, b"\x0C\x3C")])),
           fig0(14, bytes([5 << 2 | 1])), fig0(5, e05(0, 8)), f09(2, 0xE1, 1), fig0(17, e17(0x1000, 10)), fig0(18, e18(0x1000, 1, [4])), f10(60001, 1, 2)]
    nxt = [fig0(7, bytes([9 << 2, 2]), cn=1)] + ([fig0(8, e08(0x1002, 0, subch=2), cn=1)] if flags == 3 else [])
    cifs = []
    for q, figs in enumerate(base):                  # an SI CIF (without a FIG 0/0) behind every CIF of the reconfiguration
        cifs += [figs, (nxt if announce <= q < switch else []) + cur]
    return cifs


def si_restart_cifs():
    """SI filed, a restart mid-frame (an overlapping sub-channel in the frame's second CIF), the same SI again: filed and reported again"""
    a, _ = fg._layouts()
    si = [fig0(7, bytes([8 << 2, 1])), f09(2, 0xE1, 1), f10(60002, 3, 4, 5), fig0(5, e05(1, 8)), fig0(17, e17(0x1001, 3)), fig0(18, e18(0x1001, 1, [4]))]
    clash = ds.SubCh(9, 40, 48, 64, 2, 0)
    cifs = []
    for q in range(16):
        figs = [ds.fig00_bytes(300 + q)] + ([ds.fig01_bytes(a[:4])] if q % 2 == 0 else [ds.fig02_bytes(a[:4])]) + si[:3 + q % 4]
        if q == 5:
            figs = [ds.fig00_bytes(300 + q), si[3], ds.fig01_bytes([clash]), si[4]]       # the FIG behind the restart, in the same FIB, is not evaluated
        cifs.append(figs)
    return cifs


def edge_fibs():
    """single FIBs: every FIG cut by its own length (an entry outside its FIG, for every type), 0/13 with 0, 6 and 7 applications, the SCId
    above 255 that is never known, 0/13 with C/N 1 filed twice, a FIG 0 extension nobody follows"""
    one = fg.one_fib
    out = [one(fig0(5, e05(3, 8) + e05(4, 9)[:1])), one(fig0(5, e05(0x123, 8, True)[:2])),                                     # 0/5 short / long cut
           one(fig0(7, b"\x10")), one(fig0(8, e08(0x1000, 0, subch=1)[:3])), one(fig0(8, e08(0x1000, 0, scid=0x111)[:4])),
           one(fig0(8, e08(0x1000, 1, subch=1, ext=1)[:4])), one(fig0(8, e08(0xE1000000, 0, subch=1, pd=1)[:5], pd=1)),
           one(fig0(9, b"\x01\x02")), one(fig0(10, f10(60000, 1, 2)[2:4])), one(fig0(10, f10(60000, 1, 2, 3)[2:7])), one(fig0(10, f10(60000, 1, 2)[2:5])),
           one(f09(-5, 0xE0, 4, ext=1)),
           one(fig0(13, e13(0x2000, 0, [(1, b"\x01\x02\x03")])[:2])), one(fig0(13, e13(0x2000, 0, [(1, b"\x01\x02\x03")])[:4])),
           one(fig0(13, e13(0x2000, 0, [(1, b"\x01\x02\x03")])[:6])),
           one(fig0(17, e17(0x2000, 1) + e17(0x2001, 2)[:3])), one(fig0(17, e17(0x2002, 1)[:3])),
           one(fig0(18, e18(0x2000, 1, [1, 2])[:4])), one(fig0(18, e18(0x2000, 1, [1, 2])[:6])),
           one(fig0(19, e19(1, 1, 1)[:3])), one(fig0(19, e19(1, 1, 1, region=3)[:4]))]
    out += [one(fig0(13, e13(0x2100, 0, []))), one(fig0(13, e13(0x2101, 1, [(i + 1, bytes([i])) for i in range(6)]))),
            # 7 applications announced: 6 are read, the cursor stands on the 7th, whose bytes are the next entry's SId
            one(fig0(13, e13(0x2102, 2, [(i + 1, b"") for i in range(7)], n=7) + e13(0x2103, 3, [(9, b"\xAA")]))),
            one(fig0(13, e13(0x2100, 0, [(1, b"\x55")])[:3] + e13(0x2104, 0, [(2, b"\x01\x02")]))),     # known: stepped over by its SizeBits, whatever it says now
            one(fig0(13, e13(0x2200, 0, [(SLS, b"")]), cn=1)), one(fig0(13, e13(0x2200, 0, [(SLS, b"")]), cn=1)),            # filed twice (:525 / :547)
            one(fig0(5, e05(0x323, 8, True))), one(fig0(5, e05(0x323, 8, True))), one(fig0(5, e05(0x023, 8, True))), one(fig0(5, e05(0x423, 8, True))),
            one(fig0(6, b"\x12\x34\x56")), one(fig0(21, b"\x12\x34")), one(fig0(14, b"")), one(fig0(18, e18(0x2000, 1, []))),
            one(fig0(8, e08(0xE1000000, 5, scid=0x7FF, pd=1), pd=1, cn=1)), one(fig0(5, e05(63, 255), cn=1))]
    fibs = np.stack(out)
    return fibs, np.ones(len(fibs), np.uint8)


def gd_fibs(n):
    """a FIG 0/8 table of n entries (short form, 16-bit SIds), 5 to a FIB, then every 7th again (known, across the ballot's 64-entry rounds) and
    a 0/13 per 16th (SId, SCIdS), and the components they belong to: a directory of n components"""
    ent = [(0x3000 + i, i % 16, i % 64) for i in range(n)]
    out = []
    for at in range(0, n, 5):
        out.append(fg.one_fib(fig0(8, b"".join(e08(s, c, subch=u) for s, c, u in ent[at:at + 5]))))
    for at in range(0, n, 5):
        body = bytearray([0x02])
        for s, c, u in ent[at:at + 5]:
            body += bytes([s >> 8, s & 0xFF, 0x01, 63, u << 2])                            # TMId 0, ASCTy 63, SubChId u, secondary
        out.append(fg.one_fib(bytes([len(body)]) + bytes(body)))
    out += [fg.one_fib(fig0(8, e08(s, c, subch=u))) for s, c, u in ent[::7]]
    out += [fg.one_fib(fig0(13, e13(s, c, [(SLS, bytes([c]))]))) for s, c, u in ent[::16]]
    out += [fg.one_fib(fg.fig1s4(0, c, s, "comp %d" % c)) for s, c, u in ent[::16]]
    out.append(fg.one_fib(ds.fig01_bytes([ds.SubCh(u, 12 * u, 12, 16, 2, 0) for u in range(5)])))
    fibs = np.stack(out)
    return fibs, np.ones(len(fibs), np.uint8)


def cluster_fibs():
    """the cluster table filled (64 ids), then more ids (they fall back to entry 0), and entry 0's flags met by a FIG 0/19"""
    out = []
    for at in range(1, 73, 6):
        out.append(fg.one_fib(fig0(18, e18(0x4000 + at, 0x0004, list(range(at, at + 6))))))
    out.append(fg.one_fib(fig0(18, e18(0x4100, 0x0008, [200, 1]))))
    out += [fg.one_fib(fig0(19, e19(201, 0x0008, 3)))] * 6
    fibs = np.stack(out)
    return fibs, np.ones(len(fibs), np.uint8)


def cap_fibs():
    """every bounded table one past its cap, the dropped ones again (dropped again, never "known"), and a directory of the cap's components"""
    out = []
    for at in range(0, MAX_GD + 1, 5):
        out.append(fg.one_fib(fig0(8, b"".join(e08(0x5000 + i, i % 16, subch=i % 64) for i in range(at, min(at + 5, MAX_GD + 1))))))
    for at in range(0, MAX_UA + 1, 4):
        out.append(fg.one_fib(fig0(13, b"".join(e13(0x5000 + i, i % 16, [(1, b"\x01")]) for i in range(at, min(at + 4, MAX_UA + 1))))))
    for at in range(0, MAX_LANG + 1, 8):
        out.append(fg.one_fib(fig0(5, b"".join(e05(0x100 + i, 1, True) for i in range(at, min(at + 8, MAX_LANG + 1))))))      # SCIds above 255: never known
    for at in range(0, MAX_PTY + 1, 6):
        out.append(fg.one_fib(fig0(17, b"".join(e17(0x5000 + i, 1) for i in range(at, min(at + 6, MAX_PTY + 1))))))
    for i in range(MAX_CM // 7 + 1):
        out.append(fg.one_fib(fig0(18, e18(0x5000 + i, 1, [1 + (7 * i + k) % 60 for k in range(7)]))))
    out += [fg.one_fib(fig0(8, e08(0x5000 + MAX_GD, 0, subch=0))), fg.one_fib(fig0(13, e13(0x5000 + MAX_UA, 0, [(1, b"\x01")]))),
            fg.one_fib(fig0(5, e05(0x100 + MAX_LANG, 1, True))), fg.one_fib(fig0(17, e17(0x5000 + MAX_PTY, 1)))]
    comps = [(0x5000 + i, [0x800 + i]) for i in range(fg.MAX_COMP)]
    out += [fg.one_fib(ds.fig02_packet_bytes(ch)) for ch in fg._chunks(comps, 5, 5)]
    fibs = np.stack(out)
    return fibs, np.ones(len(fibs), np.uint8)


def _with_si_headers(fibs, seed):
    """random FIBs of fic_cases with the second byte of their first FIG forced to an SI extension, so that hostile bytes reach every SI walk"""
    rng = np.random.default_rng(seed)
    out = fibs.copy()
    exts = np.array([5, 7, 8, 9, 10, 13, 14, 17, 18, 19])
    pick = rng.integers(0, len(exts), len(out))
    out[:, 0] &= 0x1F                                                                     # type 0, the length as it fell
    out[:, 1] = (out[:, 1] & 0xE0) | exts[pick]
    return out


@functools.lru_cache(maxsize=None)
def sequences():
    out = {"si_ensemble": fg.fibs_of(si_ensemble_cifs())}
    for flags in (1, 3):
        out["si_reconf_flags_%d" % flags] = fg.fibs_of(si_reconf_cifs(flags))
    out["si_restart"] = fg.fibs_of(si_restart_cifs())
    out["si_edges"] = edge_fibs()
    for n in (63, 64, 65, 129):
        out["si_gd_%d" % n] = gd_fibs(n)
    out["si_clusters"] = cluster_fibs()
    one = np.stack([fg.one_fib(ds.fig02_bytes([ds.SubCh(3, 0, 48, 64)]), ds.fig01_bytes([ds.SubCh(3, 0, 48, 64)]))])
    out["si_dir_1"] = (one, np.ones(1, np.uint8))
    out["si_caps"] = cap_fibs()
    fibs, crc = (a.copy() for a in out["si_ensemble"])
    crc[::5] = 0
    out["si_bad_crc"] = (fibs, crc)
    rnd = np.stack(fc.random_fibs() + fc.sparse_fibs())
    rnd = np.concatenate([rnd, _with_si_headers(rnd[:1500], 11)])
    out["si_random"] = (rnd, np.ones(len(rnd), np.uint8))
    return out


PARITY = ("si_dir_1", "si_ensemble", "si_reconf_flags_1", "si_reconf_flags_3", "si_restart", "si_edges", "si_gd_63", "si_gd_64", "si_gd_65", "si_gd_129", "si_bad_crc")

REQUIRED = {
    "language_new_ls_0", "language_new_ls_1", "language_new_ls_1_scid_above_255", "language_known_ls_0", "language_known_ls_1",
    "config_new_cn_0", "config_new_cn_1", "config_known",
    "global_def_new_ls_0_ext_0_pd_0_cn_0", "global_def_new_ls_0_ext_1_pd_0_cn_0", "global_def_new_ls_1_ext_0_pd_0_cn_0", "global_def_new_ls_1_ext_0_pd_1_cn_0",
    "global_def_new_ls_1_ext_1_pd_1_cn_0", "global_def_new_ls_0_ext_0_pd_0_cn_1", "global_def_known",
    "lto_new_positive", "lto_new_negative", "lto_known",
    "time_short_form_before_0s9", "time_long_form_after_0s9", "time_short_form_after_0s9",
    "user_apps_new_0_apps_pd_0_cn_0", "user_apps_new_6_apps_pd_0_cn_0", "user_apps_new_1_apps_pd_1_cn_0", "user_apps_new_1_apps_pd_0_cn_1", "user_apps_known",
    "user_apps_clamped", "fec_new_cn_0", "fec_new_cn_1", "fec_known", "pty_new", "pty_known",
    "cluster_zero", "cluster_sid_new_cn_0", "cluster_sid_new_cn_1", "cluster_sid_known", "cluster_fallback",
    "asw_start", "asw_goes_on", "asw_stop_announced", "asw_stop_early", "asw_idle", "asw_region", "asw_unknown_cluster",
    "outside_0s5", "outside_0s7", "outside_0s8", "outside_0s9", "outside_0s10", "outside_0s13", "outside_0s17", "outside_0s18", "outside_0s19",
    "over_global_defs", "over_user_apps", "over_languages", "over_ptys", "over_cluster_sids",
    "si_restart", "si_swap_strict_drops_current_tables", "si_carry_over_gd", "si_carry_over_ua", "si_carry_over_fec", "si_carry_over_cl", "si_next_brings_gd",
    "si_table_event_current", "si_table_event_next", "fig0_ext_not_followed",
}


@functools.lru_cache(maxsize=None)
def model_rows(name, reference_quirks, stepwise=False):
    """the model's row after the whole sequence, or (stepwise) after every FIB; and what the model reached on the way"""
    fibs, crc = sequences()[name]
    m = SiModel(reference_quirks)
    if not stepwise:
        m.feed(fibs, crc)
        return m.row(), frozenset(m.reached)
    rows = []
    for f, ok in zip(fibs, crc):
        m.walk(f, ok)
        rows.append(m.row())
    return rows, frozenset(m.reached)
