// fig_si_core.h -- the service information of FIG 0 for the walk of fig_core.h (which declares the four hooks it calls and includes this file at its end): FIG 0/5,
// 0/7, 0/8, 0/9, 0/10, 0/13, 0/14, 0/17, 0/18 and 0/19 with the reference's decisions line for line (fib_decoder_fig0.cpp:333-720, cited below;
// _set_cluster / _get_cluster fib_decoder.cpp:693-742), the SI events of include/dabx.h, and the join of every table into one record per
// service component (fig_dir_record: fib_decoder.cpp:219-290, :351-460).  Like fig_core.h one source serves the wave (FIG_LANES 64) and the host
// (FIG_LANES 1): cursor and fields come out of fig_u, "is this key known" is fig_first over key arrays, every lane stores the same value and a
// store is followed by fig_sync.  fig_walk_fib calls fig_si_walk where it counts fig0_other_ext, fig_0s0 calls fig_si_swap where it swaps and
// fig_restart calls fig_si_restart: cur, the swap and the restart are the ones the walk decides.  Where this departs from the reference is
// stated in include/dabx.h ("Service information").
#pragma once
#include "fig_core.h"

namespace dabx {

constexpr int SI_MAX_GD = DABX_FIG_MAX_GLOBAL_DEFS, SI_MAX_UA = DABX_FIG_MAX_USER_APPS, SI_MAX_FEC = 64, SI_MAX_CL = DABX_FIG_MAX_CLUSTERS;
constexpr int SI_MAX_CM = DABX_FIG_MAX_CLUSTER_SIDS, SI_MAX_LANG = DABX_FIG_MAX_LANGUAGES, SI_MAX_PTY = DABX_FIG_MAX_PTYS, SI_UA_WORDS = 12;
static_assert(sizeof(dabx_fig_si_stats) == 256 && sizeof(dabx_fig_si_scalars) == 128 && sizeof(dabx_fig_service) == 128 && sizeof(dabx_fig_cluster) == 128 &&
              sizeof(dabx_fig_user_apps_entry) == 64 && sizeof(dabx_fig_global_def) == 12, "record sizes of include/dabx.h");

// The SI tables of one multiplex configuration (the SI vectors and mClusterTable of FibConfigFig0).  Keys and values, 64 to a coalesced load.
struct FigSiCfg {
  int32_t n_gd, n_ua, n_fec, n_cl, n_cm, has7, cfg7, gained;   // cfg7: NumServices | Count << 8; gained: DABX_FIG_SI_HAS_* of the frame being walked
  uint32_t gd_sid[SI_MAX_GD];
  uint32_t gd_info[SI_MAX_GD];                   // scids | ls << 4 | ext << 5 | pd << 6 | subch_id << 8 (short form) | scid << 16 (long form)
  uint32_t ua_sid[SI_MAX_UA];
  uint32_t ua_info[SI_MAX_UA];                   // scids | pd << 4 | n_apps << 8 | size_bits << 16
  uint32_t ua_app[SI_MAX_UA * SI_UA_WORDS];      // per application: type | data length << 11, then the first four data bytes, first byte on top
  uint32_t fec[SI_MAX_FEC];                      // subch_id | scheme << 8
  uint32_t cl_id[SI_MAX_CL], cl_flags[SI_MAX_CL], cl_ann[SI_MAX_CL], cl_n[SI_MAX_CL];     // cluster id, ASu flags, announcing, SIds filed
  uint32_t cm[SI_MAX_CM];                        // the clusters' SIds, all clusters in order of filing: slot << 16 | SId
};
struct FigSiState {
  int32_t n_lang, n_pty, has9, lto_minutes, ecc, inter_table, lto_ext, time_set;          // 0/5, 0/17 and 0/9 belong to the current configuration
  int32_t mjd, hour, minute, second, lsi, utc_flag, pad_[2];
  dabx_fig_si_stats cnt;
  FigSiCfg cfg[2];                               // indexed like FigState::cfg: cfg[cur] = current
  uint32_t lang[SI_MAX_LANG];                    // language | id << 8 | ls << 31
  uint32_t pty[SI_MAX_PTY];                      // sid | sd << 16 | code << 17
};
static_assert(sizeof(FigSiState) % 8 == 0, "FigSiState is copied as dwords");

FIG_HD inline void fig_si_cfg_reset(FigSiCfg &c) { c.n_gd = c.n_ua = c.n_fec = c.n_cl = c.n_cm = c.has7 = c.cfg7 = c.gained = 0; }
FIG_HD inline void fig_si_state_init(FigSiState &s) { memset(&s, 0, sizeof(s)); }

// _restart_fib_decoding: both configurations' reset() and _reset() (fib_decoder.cpp:112-141): every table and the time
FIG_HD inline void fig_si_restart(FigSiState &s)
{
  fig_si_cfg_reset(s.cfg[0]); fig_si_cfg_reset(s.cfg[1]);
  s.n_lang = s.n_pty = s.has9 = s.lto_minutes = s.ecc = s.inter_table = s.lto_ext = s.time_set = 0;
  s.mjd = s.hour = s.minute = s.second = s.lsi = s.utc_flag = 0;
}

// The swap (fib_decoder_fig0.cpp:103-110), called in front of the flip of `cur`.  strict: the object that becomes current brings what was filed
// into it, and nobody files a 0/5, 0/9 or 0/17 there.  Otherwise every table the announcement never filled is carried over, as fig_0s0 does.
FIG_HD inline void fig_si_swap(FigSiState &s, int cur, int strict, int lane)
{
  FigSiCfg &cu = s.cfg[cur], &nx = s.cfg[cur ^ 1];
  if (strict) { s.n_lang = s.n_pty = s.has9 = s.lto_minutes = s.ecc = s.inter_table = s.lto_ext = 0; }
  else {
    if (nx.n_gd == 0) { fig_copy(nx.gd_sid, cu.gd_sid, cu.n_gd, lane); fig_copy(nx.gd_info, cu.gd_info, cu.n_gd, lane); nx.n_gd = cu.n_gd; }
    if (nx.n_ua == 0) {
      fig_copy(nx.ua_sid, cu.ua_sid, cu.n_ua, lane); fig_copy(nx.ua_info, cu.ua_info, cu.n_ua, lane); fig_copy(nx.ua_app, cu.ua_app, cu.n_ua * SI_UA_WORDS, lane);
      nx.n_ua = cu.n_ua;
    }
    if (nx.n_fec == 0) { fig_copy(nx.fec, cu.fec, cu.n_fec, lane); nx.n_fec = cu.n_fec; }
    if (nx.n_cl == 0) {
      fig_copy(nx.cl_id, cu.cl_id, cu.n_cl, lane); fig_copy(nx.cl_flags, cu.cl_flags, cu.n_cl, lane); fig_copy(nx.cl_ann, cu.cl_ann, cu.n_cl, lane);
      fig_copy(nx.cl_n, cu.cl_n, cu.n_cl, lane); fig_copy(nx.cm, cu.cm, cu.n_cm, lane);
      nx.n_cl = cu.n_cl; nx.n_cm = cu.n_cm;
    }
    if (!nx.has7) { nx.has7 = cu.has7; nx.cfg7 = cu.cfg7; }
    nx.gained |= cu.gained & (DABX_FIG_SI_HAS_LANGUAGE | DABX_FIG_SI_HAS_LTO | DABX_FIG_SI_HAS_PTY);      // what the current tables gained in this frame
    fig_sync();
  }
  fig_si_cfg_reset(cu);                                                  // :107: the one that becomes next
}

#define SI_BITS(off, n) ((unsigned)fig_u((int)fig_bits(d, (off), (n))))
#define SI_OUTSIDE(end) ((end) > len + 1)                                // the FIG is bytes 0 .. len of d

// _subprocess_Fig0s5 (:333-383), in the current configuration
FIG_HD inline void fig_si_0s5(FigSiState &s, FigSiCfg &cur, const uint8_t *d, int len, int lane)
{
  int used = 2;
  while (used <= len) {                                                  // _process_fig0_loop, :79
    const int ob = used * 8;
    const unsigned ls = SI_BITS(ob, 1);
    const int size = ls ? 3 : 2;
    if (SI_OUTSIDE(used + size)) { s.cnt.outside++; return; }
    unsigned id, probe, language;
    if (!ls) { id = probe = SI_BITS(ob + 2, 6); language = SI_BITS(ob + 8, 8); }                  // :343-346
    else { id = SI_BITS(ob + 4, 12); probe = id & 0xFF; language = SI_BITS(ob + 16, 8); }         // :363-366; the getter takes a u8 (fib_config_fig0.h:242)
    const unsigned key = ls << 31 | probe << 8;
    const int known = fig_first(s.n_lang, lane, [&](int i) { return (s.lang[i] & 0xFFFFFF00u) == key; });
    used += size;
    if (known >= 0) { s.cnt.language_known++; continue; }
    if (s.n_lang >= SI_MAX_LANG) { s.cnt.over_languages++; continue; }   // guard: the table is full
    s.lang[s.n_lang] = language | id << 8 | ls << 31;
    s.n_lang++; cur.gained |= DABX_FIG_SI_HAS_LANGUAGE;
    s.cnt.language_new++;
    fig_sync();
  }
}

// _process_Fig0s7 (:386-406), in the C/N configuration
FIG_HD inline void fig_si_0s7(FigSiState &s, FigSiCfg &cfg, const uint8_t *d, int len)
{
  if (SI_OUTSIDE(4)) { s.cnt.outside++; return; }
  if (cfg.has7) { s.cnt.config_known++; return; }
  cfg.cfg7 = (int)(SI_BITS(16, 6) | SI_BITS(22, 10) << 8);
  cfg.has7 = 1; cfg.gained |= DABX_FIG_SI_HAS_CONFIG;
  s.cnt.config_new++;
  fig_sync();
}

// _subprocess_Fig0s8 (:409-449), in the C/N configuration
FIG_HD inline void fig_si_0s8(FigSiState &s, FigSiCfg &cfg, const uint8_t *d, int len, int pd, int lane)
{
  int used = 2;
  const int sidb = pd ? 4 : 2;
  while (used <= len) {
    int ob = used * 8;
    if (SI_OUTSIDE(used + sidb + 2)) { s.cnt.outside++; return; }
    const unsigned sid = SI_BITS(ob, pd ? 32 : 16);                      // :412
    ob += sidb * 8;
    const unsigned ext = SI_BITS(ob, 1), scids = SI_BITS(ob + 4, 4), ls = SI_BITS(ob + 8, 1);     // :418-420
    const int size = sidb + (ls ? 3 : 2) + (ext ? 1 : 0);                // :425, :430
    if (SI_OUTSIDE(used + size)) { s.cnt.outside++; return; }
    const unsigned info = scids | ls << 4 | ext << 5 | (unsigned)pd << 6 | (ls ? SI_BITS(ob + 12, 12) << 16 : SI_BITS(ob + 10, 6) << 8);
    const int known = fig_first(cfg.n_gd, lane, [&](int i) { return cfg.gd_sid[i] == sid && (cfg.gd_info[i] & 15) == scids; });     // :435
    used += size;
    if (known >= 0) { s.cnt.global_def_known++; continue; }
    if (cfg.n_gd >= SI_MAX_GD) { s.cnt.over_global_defs++; continue; }   // guard: the table is full
    cfg.gd_sid[cfg.n_gd] = sid; cfg.gd_info[cfg.n_gd] = info;
    cfg.n_gd++; cfg.gained |= DABX_FIG_SI_HAS_GLOBAL_DEF;
    s.cnt.global_def_new++;
    fig_sync();
  }
}

// _process_Fig0s9 (:452-479): read once, into the current configuration
FIG_HD inline void fig_si_0s9(FigSiState &s, FigSiCfg &cur, const uint8_t *d, int len)
{
  if (s.has9) { s.cnt.lto_known++; return; }                             // :456-460
  if (SI_OUTSIDE(5)) { s.cnt.outside++; return; }
  const int lto = (int)SI_BITS(19, 5);                                   // :464-467
  s.lto_ext = (int)SI_BITS(16, 1);
  s.lto_minutes = (SI_BITS(18, 1) ? -lto : lto) * 30;
  s.ecc = (int)SI_BITS(24, 8); s.inter_table = (int)SI_BITS(32, 8);
  s.has9 = 1; cur.gained |= DABX_FIG_SI_HAS_LTO;
  s.cnt.lto_new++;
  fig_sync();
}

// _process_Fig0s10 (:481-514): the time is overwritten by every FIG, and reported while a FIG 0/9 is filed
FIG_HD inline void fig_si_0s10(FigState &t, FigSiState &s, const uint8_t *d, int len, const FigOut &o, int lane)
{
  if (SI_OUTSIDE(5)) { s.cnt.outside++; return; }
  const int utc_flag = (int)SI_BITS(36, 1);                              // :488
  if (SI_OUTSIDE(utc_flag ? 8 : 6)) { s.cnt.outside++; return; }
  s.mjd = (int)SI_BITS(17, 17); s.lsi = (int)SI_BITS(34, 1); s.utc_flag = utc_flag;
  const unsigned utc = SI_BITS(37, utc_flag ? 27 : 11);                  // :489; the bit fields of fib_config_fig0.h:178-179
  if (utc_flag) { s.hour = (int)(utc >> 22 & 31); s.minute = (int)(utc >> 16 & 63); s.second = (int)(utc >> 10 & 63); }
  else { s.hour = (int)(utc >> 6 & 31); s.minute = (int)(utc & 63); s.second = -1; }
  s.time_set = 1;
  s.cnt.time_set++;
  fig_sync();
  if (s.has9) {                                                          // :508-513
    const int32_t w[8] = {s.mjd, s.hour, s.minute, s.second, s.lto_minutes, s.utc_flag, s.lsi, 0};
    fig_emit(t, o, DABX_FIG_TIME, w, lane);
  }
}

// _subprocess_Fig0s13 (:517-560): looked up in the CURRENT configuration (:525), filed into the C/N one (:547)
FIG_HD inline void fig_si_0s13(FigSiState &s, FigSiCfg &cur, FigSiCfg &cfg, const uint8_t *d, int len, int pd, int lane)
{
  int used = 2;
  const int sidb = pd ? 4 : 2;
  while (used <= len) {
    int ob = used * 8;
    if (SI_OUTSIDE(used + sidb + 1)) { s.cnt.outside++; return; }
    const unsigned sid = SI_BITS(ob, pd ? 32 : 16);
    ob += sidb * 8;
    const unsigned scids = SI_BITS(ob, 4);
    const int known = fig_first(cur.n_ua, lane, [&](int i) { return cur.ua_sid[i] == sid && (cur.ua_info[i] & 15) == scids; });
    if (known >= 0) { used += (int)(cur.ua_info[known] >> 16) / 8; s.cnt.user_apps_known++; continue; }        // :554: by the stored SizeBits
    int n_apps = (int)SI_BITS(ob + 4, 4);
    ob += 8;
    if (n_apps > 6) { n_apps = 6; s.cnt.user_apps_clamped++; }           // :532-536; the cursor will stand inside the 7th application
    const bool room = cfg.n_ua < SI_MAX_UA;
    uint32_t *app = cfg.ua_app + (room ? cfg.n_ua : 0) * SI_UA_WORDS;
    for (int i = 0; i < 6; i++) {
      uint32_t head = 0, data = 0;
      if (i < n_apps) {
        if (SI_OUTSIDE(ob / 8 + 2)) { s.cnt.outside++; return; }
        const unsigned type = SI_BITS(ob, 11), alen = SI_BITS(ob + 11, 5);                         // :541-542
        if (SI_OUTSIDE(ob / 8 + 2 + (int)alen)) { s.cnt.outside++; return; }
        for (unsigned k = 0; k < 4; k++) data = data << 8 | (k < alen ? (unsigned)d[ob / 8 + 2 + k] : 0u);
        head = type | alen << 11;
        ob += 16 + 8 * (int)alen;                                        // :543
      }
      if (room) { app[2 * i] = head; app[2 * i + 1] = (uint32_t)fig_u((int)data); }
    }
    const int size_bits = ob - used * 8;                                 // :546
    used = ob / 8;
    if (!room) { s.cnt.over_user_apps++; fig_sync(); continue; }         // guard: the table is full
    cfg.ua_sid[cfg.n_ua] = sid; cfg.ua_info[cfg.n_ua] = scids | (unsigned)pd << 4 | (unsigned)n_apps << 8 | (unsigned)size_bits << 16;
    cfg.n_ua++; cfg.gained |= DABX_FIG_SI_HAS_USER_APPS;
    s.cnt.user_apps_new++;
    fig_sync();
  }
}

// _subprocess_Fig0s14 (:563-583), in the C/N configuration.  (64 ids, first wins: the table cannot overflow)
FIG_HD inline void fig_si_0s14(FigSiState &s, FigSiCfg &cfg, const uint8_t *d, int len, int lane)
{
  for (int used = 2; used <= len; used++) {
    const unsigned id = SI_BITS(used * 8, 6);
    const int known = fig_first(cfg.n_fec, lane, [&](int i) { return (cfg.fec[i] & 63) == id; });
    if (known >= 0) { s.cnt.fec_known++; continue; }
    cfg.fec[cfg.n_fec] = id | SI_BITS(used * 8 + 6, 2) << 8;
    cfg.n_fec++; cfg.gained |= DABX_FIG_SI_HAS_FEC;
    s.cnt.fec_new++;
    fig_sync();
  }
}

// _process_Fig0s17 (:585-613): 32 bits a step whatever the entry's flags say, in the current configuration
FIG_HD inline void fig_si_0s17(FigSiState &s, FigSiCfg &cur, const uint8_t *d, int len, int lane)
{
  for (int off = 16; off < len * 8; off += 32) {                         // :590, :611
    if (SI_OUTSIDE(off / 8 + 4)) { s.cnt.outside++; return; }
    const unsigned sid = SI_BITS(off, 16);
    const int known = fig_first(s.n_pty, lane, [&](int i) { return (s.pty[i] & 0xFFFF) == sid; });          // :596
    if (known >= 0) { s.cnt.pty_known++; continue; }
    if (s.n_pty >= SI_MAX_PTY) { s.cnt.over_ptys++; continue; }          // guard: the table is full
    s.pty[s.n_pty] = sid | SI_BITS(off + 16, 1) << 16 | SI_BITS(off + 27, 5) << 17;                // :599-600
    s.n_pty++; cur.gained |= DABX_FIG_SI_HAS_PTY;
    s.cnt.pty_new++;
    fig_sync();
  }
}

// _get_cluster (fib_decoder.cpp:722-742): the entry of the id, else the first free one, else entry 0.  *fresh: the entry was made now.
FIG_HD inline int fig_si_cluster(FigSiState &s, FigSiCfg &cfg, unsigned id, bool *fresh, int lane)
{
  *fresh = false;
  const int known = fig_first(cfg.n_cl, lane, [&](int i) { return cfg.cl_id[i] == id; });
  if (known >= 0) return known;
  if (cfg.n_cl >= SI_MAX_CL) { s.cnt.cluster_fallback++; return 0; }     // :741
  const int n = cfg.n_cl;
  cfg.cl_id[n] = id; cfg.cl_flags[n] = 0; cfg.cl_ann[n] = 0; cfg.cl_n[n] = 0;
  cfg.n_cl = n + 1; cfg.gained |= DABX_FIG_SI_HAS_CLUSTER;
  s.cnt.cluster_new++;
  *fresh = true;
  fig_sync();
  return n;
}

// _process_Fig0s18 (:616-647) with _set_cluster (fib_decoder.cpp:693-720), in the C/N configuration
FIG_HD inline void fig_si_0s18(FigSiState &s, FigSiCfg &cfg, const uint8_t *d, int len, int lane)
{
  int bo = 16;
  while (bo <= len * 8) {                                                // :624
    const int by = bo / 8;
    if (SI_OUTSIDE(by + 5)) { s.cnt.outside++; return; }
    const unsigned sid = SI_BITS(bo, 16), asu = SI_BITS(bo + 16, 16);    // :626-628: 16 bits whatever P/D says
    const int nr = (int)SI_BITS(bo + 37, 3);                             // :630
    if (SI_OUTSIDE(by + 5 + nr)) { s.cnt.outside++; return; }
    for (int i = 0; i < nr; i++) {
      const unsigned id = SI_BITS(bo + 40 + 8 * i, 8);
      if (id == 0) { s.cnt.cluster_zero++; continue; }                   // :635
      bool fresh;
      const int slot = fig_si_cluster(s, cfg, id, &fresh, lane);
      cfg.cl_flags[slot] = asu;                                          // :707-710
      const unsigned key = (unsigned)slot << 16 | sid;
      const int listed = fig_first(cfg.n_cm, lane, [&](int k) { return cfg.cm[k] == key; });       // :712-718
      if (listed >= 0) s.cnt.cluster_sid_known++;
      else if (cfg.n_cm >= SI_MAX_CM) s.cnt.over_cluster_sids++;         // guard: the table is full
      else {
        cfg.cm[cfg.n_cm] = key;
        cfg.n_cm++; cfg.cl_n[slot]++; cfg.gained |= DABX_FIG_SI_HAS_CLUSTER;
        s.cnt.cluster_sid_new++;
      }
      fig_sync();
    }
    bo += 40 + 8 * nr;
  }
}

// _process_Fig0s19 (:650-720), in the C/N configuration
FIG_HD inline void fig_si_0s19(FigState &t, FigSiState &s, FigSiCfg &cfg, const uint8_t *d, int len, int cn, const FigOut &o, int lane)
{
  int bo = 16;
  while (bo <= len * 8) {                                                // :658
    const int by = bo / 8;
    if (SI_OUTSIDE(by + 4)) { s.cnt.outside++; return; }
    const unsigned id = SI_BITS(bo, 8), asw = SI_BITS(bo + 8, 16), region = SI_BITS(bo + 25, 1), subch = SI_BITS(bo + 26, 6);
    bo += 32;
    if (region) {                                                        // :671-677
      if (SI_OUTSIDE(by + 5)) { s.cnt.outside++; return; }
      bo += 8;
    }
    bool fresh;
    const int slot = fig_si_cluster(s, cfg, id, &fresh, lane);           // :684: an unknown id gets an entry (flags 0) here too
    if (fresh) s.cnt.asw_unknown++;
    const int32_t w[8] = {(int32_t)id, (int32_t)asw, (int32_t)subch, (int32_t)cfg.cl_n[slot], cn, 0, 0, 0};
    if (cfg.cl_flags[slot] & asw) {                                      // :691-704
      cfg.cl_ann[slot]++;
      s.cnt.asw_count++;
      fig_sync();
      if (cfg.cl_ann[slot] == 5) { s.cnt.asw_start++; fig_emit(t, o, DABX_FIG_ANNOUNCE_START, w, lane); }
    } else if (cfg.cl_ann[slot] > 0) {                                   // :705-717
      cfg.cl_ann[slot] = 0;
      s.cnt.asw_stop++;
      fig_sync();
      fig_emit(t, o, DABX_FIG_ANNOUNCE_STOP, w, lane);
    }
  }
}

// _process_Fig0 (:20-67) for the extensions behind 0/3; cur: FigState::cur
FIG_HD inline void fig_si_walk(FigState &t, FigSiState &s, const uint8_t *d, int len, int ext, int pd, int cn, const FigOut &o, int lane)
{
  FigSiCfg &cur = s.cfg[t.cur], &cfg = s.cfg[cn == 0 ? t.cur : t.cur ^ 1];                       // _get_config_ptr
  switch (ext) {
    case 5: fig_si_0s5(s, cur, d, len, lane); break;
    case 7: fig_si_0s7(s, cfg, d, len); break;
    case 8: fig_si_0s8(s, cfg, d, len, pd, lane); break;
    case 9: fig_si_0s9(s, cur, d, len); break;
    case 10: fig_si_0s10(t, s, d, len, o, lane); break;
    case 13: fig_si_0s13(s, cur, cfg, d, len, pd, lane); break;
    case 14: fig_si_0s14(s, cfg, d, len, lane); break;
    case 17: fig_si_0s17(s, cur, d, len, lane); break;
    case 18: fig_si_0s18(s, cfg, d, len, lane); break;
    case 19: fig_si_0s19(t, s, cfg, d, len, cn, o, lane); break;
    default: return;
  }
  s.cnt.si_figs++;
}

// the frame is through: one DABX_FIG_SI_TABLE per configuration that gained an SI entry
FIG_HD inline void fig_si_frame_end(FigState &t, FigSiState &s, const FigOut &o, int lane)
{
  for (int k = 0; k < 2; k++) {
    FigSiCfg &c = s.cfg[t.cur ^ k];
    if (!c.gained) continue;
    const int32_t w[8] = {k, c.gained, c.n_gd, c.n_ua, c.n_fec, c.n_cl, c.n_cm, k == 0 ? s.n_lang | s.n_pty << 16 : 0};
    fig_emit(t, o, DABX_FIG_SI_TABLE, w, lane);
    c.gained = 0;
  }
}
#undef SI_BITS
#undef SI_OUTSIDE

// ---- the service directory: component i of the chosen configuration with everything the tables say about it ---------------------------------
// Plain loops over the tables, one component per caller (a lane of k_fig_directory; the host).  lab: the decoder's label records.
FIG_HD inline const dabx_fig_label *fig_dir_label(const FigState &t, const dabx_fig_label *lab, unsigned kind, unsigned sid, int scids)
{
  for (int i = 0; i < t.n_labels; i++) {
    const unsigned sel = t.lab_sel[i];
    if ((sel & 15) != kind || t.lab_id[i] != sid) continue;
    if (kind == 4 && (int)(sel >> 8) != scids) continue;                 // get_Fig1s4_ServiceComponentLabel_of_SId_SCIdS: SId and SCIdS, not P/D
    return lab + i;
  }
  return nullptr;
}
FIG_HD inline void fig_dir_record(const FigState &t, const FigSiState &s, const dabx_fig_label *lab, int next, int i, dabx_fig_service *out)
{
  const FigCfg &c = t.cfg[next ? t.cur ^ 1 : t.cur];
  const FigSiCfg &q = s.cfg[next ? t.cur ^ 1 : t.cur];
  dabx_fig_service r;
  memset(&r, 0, sizeof(r));
  const unsigned info = c.comp_info[i], sid = c.comp_sid[i];
  const int tmid = (int)(info >> 4 & 3), ps = (int)(info >> 30 & 1), pd = (int)(info >> 31);
  r.sid = sid; r.comp_idx = (int8_t)(info & 15); r.ps = (int8_t)ps; r.tmid = (int8_t)tmid; r.pd = (int8_t)pd;
  r.ty = r.scids = r.subch_id = r.prot_level = r.short_form = r.pty = r.dg_flag = -1;
  r.cu_start = r.cu_size = r.kbps = r.packet_address = r.scid = r.language = -1;
  r.label.kind = 0xFF;
  int subch = -1, scids = -1, pkt = -1, gd = -1;
  unsigned joined = 0;
  if (tmid == 0 || tmid == 1) {                                          // stream mode: the sub-channel and the type are FIG 0/2's
    subch = (int)(info >> 12 & 63);
    r.ty = (int8_t)(info >> 6 & 63);
    for (int k = 0; k < q.n_gd; k++)                                     // (extension) the short-form FIG 0/8 of (SId, SubChId)
      if (q.gd_sid[k] == sid && !(q.gd_info[k] >> 4 & 1) && (int)(q.gd_info[k] >> 8 & 63) == subch) { gd = k; break; }
  } else if (tmid == 3) {
    r.scid = (int16_t)(info >> 18 & 4095);
    for (int k = 0; k < c.n_pkt; k++) if ((int)c.pkt_scid[k] == r.scid) { pkt = k; break; }       // fib_decoder.cpp:362
    if (pkt >= 0) {
      const unsigned f = c.pkt_info[pkt];
      joined |= DABX_FIG_JOIN_PACKET;
      subch = (int)(f >> 8 & 63); r.ty = (int8_t)(f >> 2 & 63); r.dg_flag = (int8_t)(f >> 1 & 1); r.packet_address = (int16_t)(f >> 14 & 1023);
    }
    for (int k = 0; k < q.n_gd; k++) if (q.gd_sid[k] == sid && (q.gd_info[k] >> 4 & 1)) { gd = k; break; }     // :379: the first long form of the SId
  }
  if (gd >= 0) { joined |= DABX_FIG_JOIN_GLOBAL_DEF; scids = (int)(q.gd_info[gd] & 15); r.scids = (int8_t)scids; }
  int sub = -1;
  if (subch >= 0) {
    r.subch_id = (int8_t)subch;
    for (int k = 0; k < c.n_sub; k++) if ((int)c.sub_id[k] == subch) { sub = k; break; }          // :234, :370
  }
  if (sub >= 0) {
    joined |= DABX_FIG_JOIN_SUBCH;
    r.cu_start = (int16_t)(c.sub_span[sub] & 0xFFFF); r.cu_size = (int16_t)(c.sub_span[sub] >> 16);
    r.kbps = (int16_t)(c.sub_desc[sub] & 0xFFF); r.prot_level = (int8_t)(c.sub_desc[sub] >> 12 & 15); r.short_form = (int8_t)(c.sub_desc[sub] >> 16 & 1);
  }
  int ua = -1;
  if (scids >= 0)
    for (int k = 0; k < q.n_ua; k++) if (q.ua_sid[k] == sid && (int)(q.ua_info[k] & 15) == scids) { ua = k; break; }      // :387
  if (ua >= 0) {
    joined |= DABX_FIG_JOIN_USER_APPS;
    r.n_apps = (uint8_t)(q.ua_info[ua] >> 8 & 15);
    for (int k = 0; k < 6; k++) {
      const unsigned head = q.ua_app[ua * SI_UA_WORDS + 2 * k], data = q.ua_app[ua * SI_UA_WORDS + 2 * k + 1];
      r.app_type[k] = (uint16_t)(head & 2047); r.app_len[k] = (uint8_t)(head >> 11);
      r.app_data[k][0] = (uint8_t)(data >> 24); r.app_data[k][1] = (uint8_t)(data >> 16); r.app_data[k][2] = (uint8_t)(data >> 8); r.app_data[k][3] = (uint8_t)data;
    }
  }
  if (subch >= 0 && tmid == 3)
    for (int k = 0; k < q.n_fec; k++) if ((int)(q.fec[k] & 63) == subch) { joined |= DABX_FIG_JOIN_FEC; r.fec_scheme = (int8_t)(q.fec[k] >> 8); break; }   // :395, :408
  // the language: by sub-channel (:283) or, in packet mode, by SCId through the 8-bit getter (:396)
  const unsigned lkey = tmid == 3 ? 1u << 31 | (unsigned)(r.scid & 0xFF) << 8 : (unsigned)subch << 8;
  if (tmid == 3 || subch >= 0)
    for (int k = 0; k < s.n_lang; k++) if ((s.lang[k] & 0xFFFFFF00u) == lkey) { joined |= DABX_FIG_JOIN_LANGUAGE; r.language = (int16_t)(s.lang[k] & 0xFF); break; }
  if (tmid == 0)
    for (int k = 0; k < s.n_pty; k++) if ((s.pty[k] & 0xFFFF) == (sid & 0xFFFF)) { joined |= DABX_FIG_JOIN_PTY; r.pty = (int8_t)(s.pty[k] >> 17 & 31); break; }   // :284
  // the label: a primary component's is its service's (1/1 audio :241, 1/5 data :443), a secondary one's FIG 1/4 of (SId, SCIdS) (:426)
  const dabx_fig_label *l = nullptr;
  if (ps) l = fig_dir_label(t, lab, tmid == 0 ? 1u : 5u, sid, 0);
  else if (scids >= 0) l = fig_dir_label(t, lab, 4u, sid, scids);
  if (l) { joined |= DABX_FIG_JOIN_LABEL; r.label = *l; }
  r.joined = joined;
  if (tmid == 0) r.reference_defined = pd == 0 && sub >= 0;              // :224-228, :236-239
  else if (tmid == 3) r.reference_defined = pkt >= 0 && sub >= 0 && gd >= 0 && ua >= 0 && r.n_apps >= 1 && l != nullptr;     // :364-393, :436-456
  *out = r;
}

// ---- the getters' side (host) ------------------------------------------------------------------------------------------------------------------
inline void fig_si_info(const FigState &t, const FigSiState &s, dabx_fig_si_scalars *out)
{
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < 2; k++) {
    const FigSiCfg &c = s.cfg[t.cur ^ k];
    out->has_config[k] = c.has7; out->n_services[k] = c.cfg7 & 63; out->count[k] = c.cfg7 >> 8;
    out->n_global_defs[k] = c.n_gd; out->n_user_apps[k] = c.n_ua; out->n_fec[k] = c.n_fec; out->n_clusters[k] = c.n_cl; out->n_cluster_sids[k] = c.n_cm;
  }
  out->has_lto = s.has9; out->lto_minutes = s.lto_minutes; out->ecc = s.ecc; out->inter_table = s.inter_table; out->lto_ext = s.lto_ext;
  out->time_set = s.time_set; out->mjd = s.mjd; out->hour = s.hour; out->minute = s.minute; out->second = s.second; out->lsi = s.lsi; out->utc_flag = s.utc_flag;
  out->n_languages = s.n_lang; out->n_ptys = s.n_pty;
}
inline int fig_si_global_defs(const FigState &t, const FigSiState &s, int next, dabx_fig_global_def *out, int max_out)
{
  const FigSiCfg &c = s.cfg[next ? t.cur ^ 1 : t.cur];
  int n = 0;
  for (; n < c.n_gd && n < max_out; n++) {
    const unsigned f = c.gd_info[n];
    const int ls = (int)(f >> 4 & 1);
    out[n] = dabx_fig_global_def{c.gd_sid[n], (int8_t)(f & 15), (int8_t)(f >> 6 & 1), (int8_t)ls, (int8_t)(f >> 5 & 1), (int16_t)(ls ? -1 : (int)(f >> 8 & 63)),
                                 (int16_t)(ls ? (int)(f >> 16 & 4095) : -1)};
  }
  return n;
}
inline int fig_si_user_apps(const FigState &t, const FigSiState &s, int next, dabx_fig_user_apps_entry *out, int max_out)
{
  const FigSiCfg &c = s.cfg[next ? t.cur ^ 1 : t.cur];
  int n = 0;
  for (; n < c.n_ua && n < max_out; n++) {
    dabx_fig_user_apps_entry q;
    memset(&q, 0, sizeof(q));
    const unsigned f = c.ua_info[n];
    q.sid = c.ua_sid[n]; q.size_bits = (uint16_t)(f >> 16); q.scids = (uint8_t)(f & 15); q.pd = (uint8_t)(f >> 4 & 1); q.n_apps = (uint8_t)(f >> 8 & 15);
    for (int k = 0; k < 6; k++) {
      const unsigned head = c.ua_app[n * SI_UA_WORDS + 2 * k], data = c.ua_app[n * SI_UA_WORDS + 2 * k + 1];
      q.type[k] = (uint16_t)(head & 2047); q.len[k] = (uint8_t)(head >> 11);
      for (int b = 0; b < 4; b++) q.data[k][b] = (uint8_t)(data >> (24 - 8 * b));
    }
    out[n] = q;
  }
  return n;
}
inline int fig_si_fec(const FigState &t, const FigSiState &s, int next, dabx_fig_fec_scheme *out, int max_out)
{
  const FigSiCfg &c = s.cfg[next ? t.cur ^ 1 : t.cur];
  int n = 0;
  for (; n < c.n_fec && n < max_out; n++) out[n] = dabx_fig_fec_scheme{(int32_t)(c.fec[n] & 63), (int32_t)(c.fec[n] >> 8)};
  return n;
}
inline int fig_si_clusters(const FigState &t, const FigSiState &s, int next, dabx_fig_cluster *out, int max_out)
{
  const FigSiCfg &c = s.cfg[next ? t.cur ^ 1 : t.cur];
  int n = 0;
  for (; n < c.n_cl && n < max_out; n++) {
    dabx_fig_cluster q;
    memset(&q, 0, sizeof(q));
    q.cluster_id = (int32_t)c.cl_id[n]; q.flags = (int32_t)c.cl_flags[n]; q.announcing = (int32_t)c.cl_ann[n]; q.n_services = (int32_t)c.cl_n[n];
    int m = 0;
    for (int k = 0; k < c.n_cm && m < DABX_FIG_CLUSTER_LIST; k++) if ((int)(c.cm[k] >> 16) == n) q.sid[m++] = c.cm[k] & 0xFFFF;
    out[n] = q;
  }
  return n;
}
inline int fig_si_languages(const FigSiState &s, dabx_fig_language *out, int max_out)
{
  int n = 0;
  for (; n < s.n_lang && n < max_out; n++) out[n] = dabx_fig_language{(int32_t)(s.lang[n] >> 31), (int32_t)(s.lang[n] >> 8 & 4095), (int32_t)(s.lang[n] & 0xFF), 0};
  return n;
}
inline int fig_si_ptys(const FigSiState &s, dabx_fig_programme_type *out, int max_out)
{
  int n = 0;
  for (; n < s.n_pty && n < max_out; n++) out[n] = dabx_fig_programme_type{s.pty[n] & 0xFFFF, (int32_t)(s.pty[n] >> 16 & 1), (int32_t)(s.pty[n] >> 17 & 31), 0};
  return n;
}

}  // namespace dabx
