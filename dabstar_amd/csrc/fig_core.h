// fig_core.h -- the FIG walk of one FIB for the device (deliver.hip: k_fig behind k_fic_frame, k_fig_batch for dabx_fig_walk_device) and for the
// host (dabx_internal_fig_walk_host, tests/cxx/fig_core_check.cpp): FibDecoder::process_FIB (fib_decoder.cpp:59-106) with the FIG types the
// library knows -- FIG 0/0 .. 0/3 with walk_fib's decisions (fib.cpp:66-179) bit for bit -- plus the labels of FIG 1/0, 1/1, 1/4 and 1/5
// (fib_decoder_fig1.cpp:49-152, fib_decoder.cpp:744-778), and the change events of include/dabx.h.  The walk exists once: the code below.
//
// On the device one wave walks one decoder.  The FIG chain of a FIB is serial and the same for all 64 lanes: the cursor and the fields come
// out of fig_u (a readfirstlane) and every lane takes every branch together.  The decoder's state (FigState: scalars, the key and value
// arrays of both configurations, the label keys) lies in LDS while a frame is walked; every lane stores the same value where it is
// changed.  The wave is used for what is parallel: "is this key known" and "does this sub-channel overlap" are one compare per lane over
// arrays of 64 keys, decided with a ballot (fig_find*, fig_overlaps), and the carry-over of a swap copies lane-strided (fig_copy).  The swap
// itself flips FigState::cur.  For the host the same functions are loops (FIG_LANES = 1, lane 0).  Label records and events go to global
// memory from lane 0.
//
// The service information of FIG 0 behind 0/3 and the service directory's join are fig_si_core.h, included at the end of this file: a decoder follows them when
// FigOut::si points at its FigSiState (k_fig_si, k_fig_si_batch; the host walk of the tests), and a walk whose FigOut::si is the constant
// nullptr (k_fig, k_fig_batch) is compiled without them.
//
// Plain C++ but for those few functions: a host compiler takes it without HIP.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/dabx.h"

#if defined(__HIPCC__)
#define FIG_HD __host__ __device__
#else
#define FIG_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define FIG_LANES 64
#else
#define FIG_LANES 1
#endif

namespace dabx {

constexpr int FIG_MAX_SUB = 64, FIG_MAX_COMP = DABX_FIG_MAX_COMPONENTS, FIG_MAX_PKT = DABX_FIG_MAX_PACKETS, FIG_MAX_LAB = DABX_FIG_MAX_LABELS;
constexpr int FIG_LAB_SLOTS = 4 * FIG_MAX_LAB;   // label records of a decoder, all kinds, in order of filing (1 + 3 * FIG_MAX_LAB are the most)
constexpr int FIG_RING = DABX_FIG_MAX_EVENTS;    // event slots per decoder (rec_ring.h)
constexpr int FIG_SLOT_BYTES = 64;
static_assert(sizeof(dabx_fig_event) == FIG_SLOT_BYTES && sizeof(dabx_fig_label) == 32 && sizeof(dabx_fig_stats) == 256, "record sizes of include/dabx.h");

// One multiplex configuration (FibConfig of fib.cpp).  Every array is keys or values of one kind, 64 to a coalesced load.
struct FigCfg {
  int32_t n_sub, n_comp, n_pkt, gained;          // gained: a table gained an entry in the frame being walked (DABX_FIG_TABLE)
  uint32_t sub_id[FIG_MAX_SUB];
  uint32_t sub_span[FIG_MAX_SUB];                // cu_start | cu_size << 16
  uint32_t sub_desc[FIG_MAX_SUB];                // kbps | prot_level << 12 | short_form << 16
  uint32_t comp_sid[FIG_MAX_COMP];
  uint32_t comp_info[FIG_MAX_COMP];              // idx | tmid << 4 | ascty or dscty << 6 | subch_id << 12 | scid << 18 (what the TMId does not define: 0) | P/S << 30 | P/D << 31
  uint32_t pkt_scid[FIG_MAX_PKT];
  uint32_t pkt_info[FIG_MAX_PKT];                // caorg | dg << 1 | dscty << 2 | subch_id << 8 | address << 14
};
struct FigState {
  int32_t cur, strict;                           // cfg[cur] = current, cfg[cur ^ 1] = next; strict: the reference's swap rule
  int32_t cif_count, cif_hi, cif_lo, change_flags, occurrence, prev_change_flag;
  int32_t n_changes, n_restarts, n_labels, pad_;
  int32_t n_kind[4];                             // labels filed per kind (1/0, 1/1, 1/4, 1/5)
  long long fibs, fig00_fib, last_change_fib;
  dabx_fig_stats cnt;                            // cnt.events = events written: event k lies in slot k % FIG_RING
  FigCfg cfg[2];
  uint32_t lab_id[FIG_LAB_SLOTS];                // label keys: the identifier (1/0: 0) ...
  uint32_t lab_sel[FIG_LAB_SLOTS];               // ... and kind | pd << 4 | scids << 8
};
static_assert(sizeof(FigState) % 8 == 0, "FigState is copied as dwords");

// where a walk leaves what does not live in FigState
struct FigSiState;
struct FigOut {
  dabx_fig_label *labels;                        // [FIG_LAB_SLOTS]
  dabx_fig_event *ring;                          // [FIG_RING]
  FigSiState *si = nullptr;                      // the decoder's service information (fig_si_core.h); nullptr: not followed
};

FIG_HD inline void fig_state_init(FigState &t, int strict, long long fibs)      // a fresh dabx_fibdec (fib.cpp) that has skipped `fibs` FIBs
{
  memset(&t, 0, sizeof(t));
  t.strict = strict; t.cif_count = t.cif_hi = t.cif_lo = -1; t.fig00_fib = t.last_change_fib = -1; t.fibs = fibs;
}

// ---- the few functions that differ between the wave and the host ---------------------------------------------------------------------------
FIG_HD inline int fig_u(int v)                  // a value every lane holds: into a scalar
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}
FIG_HD inline void fig_sync()                   // what the wave has stored is what its lanes load next
{
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}
// the first i < n for which hit(i) holds, -1: none.  One compare per lane and 64 entries, a ballot decides.
template <class Hit> FIG_HD inline int fig_first(int n, int lane, Hit hit)
{
#if defined(__HIP_DEVICE_COMPILE__)
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const unsigned long long m = __ballot(i < n && hit(i));
    if (m) return base + __ffsll((long long)m) - 1;
  }
  return -1;
#else
  (void)lane;
  for (int i = 0; i < n; i++) if (hit(i)) return i;
  return -1;
#endif
}
FIG_HD inline void fig_copy(uint32_t *dst, const uint32_t *src, int n, int lane)
{
  for (int i = lane; i < n; i += FIG_LANES) dst[i] = src[i];
}

// ---- pieces ------------------------------------------------------------------------------------------------------------------------------------
FIG_HD inline unsigned fig_bits(const uint8_t *b, int off, int n)   // MSB-first bit field of n <= 32 bits (fib.cpp, bits): the bytes it touches, no other
{
  const int first = off >> 3, nb = ((off & 7) + n + 7) >> 3;        // <= 5 bytes
  unsigned long long v = 0;
  for (int i = 0; i < nb; i++) v = v << 8 | b[first + i];
  return (unsigned)((v >> (8 * nb - (off & 7) - n)) & (n >= 32 ? 0xFFFFFFFFull : (1ull << n) - 1));
}
// EN 300 401 table 8, the rows of fib.cpp's kUepIndex: kbps | level << 10 | CUs << 14
FIG_HD inline unsigned fig_uep(int idx)
{
#define U(k, l, c) ((unsigned)(k) | (unsigned)(l) << 10 | (unsigned)(c) << 14)
  static constexpr unsigned tab[64] = {
      U(32, 5, 16), U(32, 4, 21), U(32, 3, 24), U(32, 2, 29), U(32, 1, 35), U(48, 5, 24), U(48, 4, 29), U(48, 3, 35),
      U(48, 2, 42), U(48, 1, 52), U(56, 5, 29), U(56, 4, 35), U(56, 3, 42), U(56, 2, 52), U(64, 5, 32), U(64, 4, 42),
      U(64, 3, 48), U(64, 2, 58), U(64, 1, 70), U(80, 5, 40), U(80, 4, 52), U(80, 3, 58), U(80, 2, 70), U(80, 1, 84),
      U(96, 5, 48), U(96, 4, 58), U(96, 3, 70), U(96, 2, 84), U(96, 1, 104), U(112, 5, 58), U(112, 4, 70), U(112, 3, 84),
      U(112, 2, 104), U(128, 5, 64), U(128, 4, 84), U(128, 3, 96), U(128, 2, 116), U(128, 1, 140), U(160, 5, 80), U(160, 4, 104),
      U(160, 3, 116), U(160, 2, 140), U(160, 1, 168), U(192, 5, 96), U(192, 4, 116), U(192, 3, 140), U(192, 2, 168), U(192, 1, 208),
      U(224, 5, 116), U(224, 4, 140), U(224, 3, 168), U(224, 2, 208), U(224, 1, 232), U(256, 5, 128), U(256, 4, 168), U(256, 3, 192),
      U(256, 2, 232), U(256, 1, 280), U(320, 5, 160), U(320, 4, 208), U(320, 2, 280), U(384, 5, 192), U(384, 3, 280), U(384, 1, 416)};
#undef U
  return tab[idx & 63];
}

FIG_HD inline void fig_cfg_reset(FigCfg &c) { c.n_sub = c.n_comp = c.n_pkt = 0; c.gained = 0; }

// one event into the ring: head by the FIB being walked, payload by the caller's 8 words
FIG_HD inline void fig_emit(FigState &t, const FigOut &o, int kind, const int32_t *words, int lane)
{
  if (lane == 0 && o.ring) {
    dabx_fig_event ev;
    ev.kind = kind; ev.epoch = t.n_restarts; ev.frame = t.fibs / 12; ev.fib = t.fibs; ev.cif = 4 * (t.fibs / 12) + (t.fibs % 12) / 3;
    for (int i = 0; i < 8; i++) ev.u.words[i] = words ? words[i] : 0;
    o.ring[t.cnt.events % FIG_RING] = ev;
  }
  fig_sync();
  t.cnt.events++;
}

// The service information's side of the walk (fig_si_core.h, included at the end of this file): what the functions below call
struct FigSiState;
FIG_HD inline void fig_si_restart(FigSiState &s);
FIG_HD inline void fig_si_swap(FigSiState &s, int cur, int strict, int lane);
FIG_HD inline void fig_si_walk(FigState &t, FigSiState &s, const uint8_t *d, int len, int ext, int pd, int cn, const FigOut &o, int lane);
FIG_HD inline void fig_si_frame_end(FigState &t, FigSiState &s, const FigOut &o, int lane);

// _restart_fib_decoding (fib_decoder.cpp:131-141; dabx_fibdec::restart_decoding): both configurations, the labels and the FIG 0/0 scalars
FIG_HD inline void fig_restart(FigState &t, const FigOut &o, int lane)
{
  fig_cfg_reset(t.cfg[0]); fig_cfg_reset(t.cfg[1]);
  t.n_labels = 0; t.n_kind[0] = t.n_kind[1] = t.n_kind[2] = t.n_kind[3] = 0;
  t.cif_count = t.cif_hi = t.cif_lo = -1; t.change_flags = t.occurrence = t.prev_change_flag = 0; t.fig00_fib = -1;
  t.n_restarts++; t.cnt.restarts++;
  if (o.si) fig_si_restart(*o.si);
  fig_emit(t, o, DABX_FIG_RESTART, nullptr, lane);
}

// _process_Fig0s0 (fib_decoder_fig0.cpp:89-112; fib.cpp:78-102)
FIG_HD inline void fig_0s0(FigState &t, const uint8_t *d, int len, const FigOut &o, int lane)
{
  const int flags = fig_u((int)fig_bits(d, 32, 2));
  t.cif_hi = fig_u((int)fig_bits(d, 35, 5)); t.cif_lo = fig_u((int)fig_bits(d, 40, 8));
  t.cif_count = t.cif_hi * 250 + t.cif_lo;
  t.occurrence = len >= 6 ? fig_u((int)fig_bits(d, 48, 8)) : 0;
  t.change_flags = flags;
  t.fig00_fib = t.fibs;
  t.cnt.fig00++;
  if (flags != 0 && t.prev_change_flag == 0) {                         // an announcement begins: at_cif as dabx_follow_fic computes it
    int ahead = ((t.occurrence - t.cif_lo) % 250 + 250) % 250;
    if (ahead == 0) ahead = 250;
    const long long at = 4 * (t.fibs / 12) + (t.fibs % 12) / 3 + ahead;
    const int32_t w[8] = {flags, t.occurrence, (int32_t)(at & 0xFFFFFFFFll), (int32_t)(at >> 32), 0, 0, 0, 0};
    t.cnt.announces++;
    fig_emit(t, o, DABX_FIG_ANNOUNCE, w, lane);
  }
  if (flags == 0 && t.prev_change_flag != 0 && (t.prev_change_flag == 3 || !t.strict)) {
    FigCfg &cu = t.cfg[t.cur], &nx = t.cfg[t.cur ^ 1];
    if (!t.strict) {                                                   // a table the announcement never filled is carried over
      if (nx.n_sub == 0) {
        fig_copy(nx.sub_id, cu.sub_id, cu.n_sub, lane); fig_copy(nx.sub_span, cu.sub_span, cu.n_sub, lane); fig_copy(nx.sub_desc, cu.sub_desc, cu.n_sub, lane);
        nx.n_sub = cu.n_sub;
      }
      if (nx.n_comp == 0) { fig_copy(nx.comp_sid, cu.comp_sid, cu.n_comp, lane); fig_copy(nx.comp_info, cu.comp_info, cu.n_comp, lane); nx.n_comp = cu.n_comp; }
      if (nx.n_pkt == 0) { fig_copy(nx.pkt_scid, cu.pkt_scid, cu.n_pkt, lane); fig_copy(nx.pkt_info, cu.pkt_info, cu.n_pkt, lane); nx.n_pkt = cu.n_pkt; }
      fig_sync();
    }
    if (o.si) fig_si_swap(*o.si, t.cur, t.strict, lane);
    t.cur ^= 1;                                                        // the swap: an index, no table moves
    fig_cfg_reset(t.cfg[t.cur ^ 1]);
    t.n_changes++; t.cnt.swaps++;
    t.last_change_fib = t.fibs;
    const FigCfg &now = t.cfg[t.cur];
    const int32_t w[8] = {t.n_changes, now.n_sub, now.n_comp, now.n_pkt, 0, 0, 0, 0};
    fig_emit(t, o, DABX_FIG_SWAP, w, lane);
  }
  t.prev_change_flag = flags;
}

// _subprocess_Fig0s1 (fib_decoder_fig0.cpp:142-224; fib.cpp:103-137).  Returns true when the decoder restarted.
FIG_HD inline bool fig_0s1(FigState &t, FigCfg &cfg, const uint8_t *d, int len, const FigOut &o, int lane)
{
  int used = 2;
  while (used <= len) {
    const int ob = used * 8;
    if (used + 3 > len + 1) break;
    const unsigned id = (unsigned)fig_u((int)fig_bits(d, ob, 6));
    const int known = fig_first(cfg.n_sub, lane, [&](int i) { return cfg.sub_id[i] == id; });
    if (known >= 0) {                                                  // stepped over by the STORED entry's form
      used += (cfg.sub_desc[known] >> 16) & 1 ? 3 : 4;
      t.cnt.subch_known++;
      continue;
    }
    const int cu_start = fig_u((int)fig_bits(d, ob + 6, 10));
    const bool short_form = fig_bits(d, ob + 16, 1) == 0;
    int cu_size, kbps, level;
    if (short_form) {
      const unsigned u = fig_uep(fig_u((int)fig_bits(d, ob + 18, 6)));
      kbps = (int)(u & 1023); level = (int)((u >> 10) & 15); cu_size = (int)(u >> 14);
      used += 3;
    } else {
      if (used + 4 > len + 1) break;
      const int option = fig_u((int)fig_bits(d, ob + 17, 3)), lvl = fig_u((int)fig_bits(d, ob + 20, 2));
      cu_size = fig_u((int)fig_bits(d, ob + 22, 10));
      level = lvl;
      const int ta[4] = {12, 8, 6, 4}, tb[4] = {27, 21, 18, 15};
      if (option == 0) kbps = cu_size / ta[lvl] * 8;
      else if (option == 1) { kbps = cu_size / tb[lvl] * 32; level += 4; }
      else kbps = 0;
      used += 4;
    }
    if (cu_start + cu_size > 864) { fig_restart(t, o, lane); return true; }
    const int hit = fig_first(cfg.n_sub, lane, [&](int i) {
      const int ks = (int)(cfg.sub_span[i] & 0xFFFF), kz = (int)(cfg.sub_span[i] >> 16);
      return cu_start < ks + kz && ks < cu_start + cu_size;
    });
    if (hit >= 0) { fig_restart(t, o, lane); return true; }
    // (64 ids, unknown: n_sub < 64)
    const int n = cfg.n_sub;
    cfg.sub_id[n] = id; cfg.sub_span[n] = (unsigned)cu_start | (unsigned)cu_size << 16;
    cfg.sub_desc[n] = (unsigned)kbps | (unsigned)level << 12 | (short_form ? 1u : 0u) << 16;
    cfg.n_sub = n + 1; cfg.gained = 1;
    t.cnt.subch_new++;
    fig_sync();
  }
  return false;
}

// _subprocess_Fig0s2 (fib_decoder_fig0.cpp:230-293; fib.cpp:138-159)
FIG_HD inline void fig_0s2(FigState &t, FigCfg &cfg, const uint8_t *d, int len, int pd, int lane)
{
  int used = 2;
  while (used <= len) {
    int ob = used * 8;
    if ((ob + (pd ? 32 : 16)) / 8 + 1 > len + 1) break;
    const unsigned sid = (unsigned)fig_u((int)fig_bits(d, ob, pd ? 32 : 16));
    ob += pd ? 32 : 16;
    const int ncomp = fig_u((int)fig_bits(d, ob + 4, 4));
    ob += 8;
    for (int c = 0; c < ncomp; c++, ob += 16) {
      if ((ob + 16) / 8 > len + 1) break;
      const int known = fig_first(cfg.n_comp, lane, [&](int i) { return cfg.comp_sid[i] == sid && (int)(cfg.comp_info[i] & 15) == c; });
      if (known >= 0) { t.cnt.comp_known++; continue; }
      if (cfg.n_comp >= FIG_MAX_COMP) { t.cnt.over_components++; continue; }     // guard: the table is full
      const unsigned tmid = (unsigned)fig_u((int)fig_bits(d, ob, 2));
      unsigned info = (unsigned)c | tmid << 4 | fig_bits(d, ob + 14, 1) << 30 | (unsigned)pd << 31;
      if (tmid == 0 || tmid == 1) info |= fig_bits(d, ob + 2, 6) << 6 | fig_bits(d, ob + 8, 6) << 12;
      else if (tmid == 3) info |= fig_bits(d, ob + 2, 12) << 18;
      const int n = cfg.n_comp;
      cfg.comp_sid[n] = sid; cfg.comp_info[n] = (unsigned)fig_u((int)info);
      cfg.n_comp = n + 1; cfg.gained = 1;
      t.cnt.comp_new++;
      fig_sync();
    }
    used = ob / 8;
  }
}

// _subprocess_Fig0s3 (fib_decoder_fig0.cpp:294-330; fib.cpp:160-173)
FIG_HD inline void fig_0s3(FigState &t, FigCfg &cfg, const uint8_t *d, int len, int lane)
{
  int used = 2;
  while (used + 5 <= len + 1) {
    const int ob = used * 8;
    const unsigned scid = (unsigned)fig_u((int)fig_bits(d, ob, 12));
    const int known = fig_first(cfg.n_pkt, lane, [&](int i) { return cfg.pkt_scid[i] == scid; });
    if (known >= 0) { used += 5 + ((cfg.pkt_info[known] & 1) ? 2 : 0); t.cnt.packet_known++; continue; }
    const unsigned caorg = fig_bits(d, ob + 15, 1);
    const unsigned info = (unsigned)fig_u((int)(caorg | fig_bits(d, ob + 16, 1) << 1 | fig_bits(d, ob + 18, 6) << 2 | fig_bits(d, ob + 24, 6) << 8 | fig_bits(d, ob + 30, 10) << 14));
    used += 5 + ((info & 1) ? 2 : 0);
    if (used > len + 1) break;
    if (cfg.n_pkt >= FIG_MAX_PKT) { t.cnt.over_packets++; continue; }            // guard: the table is full
    const int n = cfg.n_pkt;
    cfg.pkt_scid[n] = scid; cfg.pkt_info[n] = info;
    cfg.n_pkt = n + 1; cfg.gained = 1;
    t.cnt.packet_new++;
    fig_sync();
  }
}

// _process_Fig1 (fib_decoder_fig1.cpp:18-152) with _extract_character_set_label (fib_decoder.cpp:744-778) as far as the device follows it
FIG_HD inline void fig_1(FigState &t, const uint8_t *d, int len, const FigOut &o, int lane)
{
  if (len < 1) { t.cnt.label_short++; return; }
  const int charset = d[1] >> 4, ext = d[1] & 7;
  int kind, off;                                                       // off: the label's first byte, counted from the FIG header
  unsigned id = 0, key = 0, sel;
  if (ext == 0 || ext == 1) {
    if (len < 3) { t.cnt.label_short++; return; }
    kind = ext; off = 4; id = fig_bits(d, 16, 16); key = ext == 0 ? 0u : id; sel = (unsigned)ext;
  } else if (ext == 4) {
    if (len < 2) { t.cnt.label_short++; return; }
    const unsigned pd = d[2] >> 7, scids = d[2] & 15u;
    off = pd ? 7 : 5;
    if (len < off - 1) { t.cnt.label_short++; return; }
    kind = 2; id = key = pd ? fig_bits(d, 24, 32) : fig_bits(d, 24, 16); sel = 4u | pd << 4 | scids << 8;
  } else if (ext == 5) {
    if (len < 5) { t.cnt.label_short++; return; }
    kind = 3; off = 6; id = key = fig_bits(d, 16, 32); sel = 5u;
  } else { t.cnt.label_other_ext++; return; }
  if (off + 18 > len + 1) { t.cnt.label_short++; return; }             // guard: the label field does not lie inside its own FIG
  key = (unsigned)fig_u((int)key); sel = (unsigned)fig_u((int)sel);
  const int known = fig_first(t.n_labels, lane, [&](int i) { return t.lab_id[i] == key && t.lab_sel[i] == sel; });
  if (known >= 0) { t.cnt.label_known++; return; }
  if (charset != 0 && charset != 6 && charset != 15) { t.cnt.label_charset++; return; }       // is_charset_valid, charsets.h:50-55
  if (t.n_kind[kind] >= (kind == 0 ? 1 : FIG_MAX_LAB)) { t.cnt.over_labels++; return; }       // guard: the kind's table is full
  dabx_fig_label r;
  memset(&r, 0, sizeof(r));
  r.id = id; r.char_flags = (uint16_t)(d[off + 16] << 8 | d[off + 17]); r.kind = (uint8_t)ext; r.charset = (uint8_t)charset;
  for (int i = 0; i < 16; i++) r.label[i] = d[off + i];
  if (ext == 4) { r.pd = (uint8_t)((sel >> 4) & 1); r.scids = (uint8_t)(sel >> 8); }
  const int n = t.n_labels;
  if (lane == 0 && o.labels) o.labels[n] = r;
  t.lab_id[n] = key; t.lab_sel[n] = sel;
  t.n_labels = n + 1; t.n_kind[kind]++;
  t.cnt.label_new++;
  int32_t w[8];
  memcpy(w, &r, sizeof(w));
  fig_emit(t, o, DABX_FIG_LABEL, w, lane);
}

// One FIB of 32 bytes (30 data + CRC) with its CRC verdict: dabx_fibdec_process's step.  After FIB 11 of a frame the frame's DABX_FIG_TABLE
// events are written.
FIG_HD inline void fig_walk_fib(FigState &t, const uint8_t *fib, bool crc_ok, const FigOut &o, int lane)
{
  if (!crc_ok) t.cnt.fibs_bad++;
  else {
    t.cnt.fibs_good++;
    int p = 0;
    while (p < 30) {
      const int type = fig_u(fib[p] >> 5), len = fig_u(fib[p] & 0x1F);
      if (type == 7 && len == 0x1F) { t.cnt.end_markers++; break; }
      if (p + 1 + len > 30) { t.cnt.fig_overrun++; break; }            // the FIG runs past the FIB's data field
      t.cnt.figs++;
      const uint8_t *d = fib + p;
      bool restarted = false;
      if (type == 0 && len >= 1) {
        const int ext = fig_u(d[1] & 0x1F), pd = fig_u((d[1] >> 5) & 1), cn = fig_u((d[1] >> 7) & 1);
        FigCfg &cfg = t.cfg[cn == 0 ? t.cur : t.cur ^ 1];
        if (ext == 0 && len >= 5) fig_0s0(t, d, len, o, lane);
        else if (ext == 1) restarted = fig_0s1(t, cfg, d, len, o, lane);
        else if (ext == 2) fig_0s2(t, cfg, d, len, pd, lane);
        else if (ext == 3) fig_0s3(t, cfg, d, len, lane);
        else {
          t.cnt.fig0_other_ext++;
          if (o.si) fig_si_walk(t, *o.si, d, len, ext, pd, cn, o, lane);
        }
      } else if (type == 1) fig_1(t, d, len, o, lane);
      else if (type != 0) t.cnt.fig_other_type++;
      else t.cnt.fig0_other_ext++;
      if (restarted) break;
      p += len + 1;
    }
  }
  if (t.fibs % 12 == 11) {                                             // the frame is through: one event per configuration that gained an entry
    for (int k = 0; k < 2; k++) {
      FigCfg &c = t.cfg[t.cur ^ k];
      if (!c.gained) continue;
      const int32_t w[8] = {k, c.n_sub, c.n_comp, c.n_pkt, 0, 0, 0, 0};
      fig_emit(t, o, DABX_FIG_TABLE, w, lane);
      c.gained = 0;
    }
    if (o.si) fig_si_frame_end(t, *o.si, o, lane);
  }
  t.fibs++;
}

// ---- the getters' side: FigState as the dabx_fibdec_* entries present a decoder (fib.cpp) ----------------------------------------------------
inline void fig_info(const FigState &t, dabx_fibdec_info *out)
{
  memset(out, 0, sizeof(*out));
  out->fibs_processed = t.fibs; out->cif_count = t.cif_count; out->change_flags = t.change_flags; out->occurrence_change = t.occurrence;
  out->fig00_fib = t.fig00_fib; out->n_changes = t.n_changes; out->last_change_fib = t.last_change_fib; out->n_restarts = t.n_restarts;
  out->cif_count_hi = t.cif_hi; out->cif_count_lo = t.cif_lo;
}
inline int fig_subchannels(const FigState &t, int next, dabx_subch_desc *out, int max_out)      // table_out
{
  const FigCfg &c = t.cfg[next ? t.cur ^ 1 : t.cur];
  int n = 0;
  for (; n < c.n_sub && n < max_out; n++) {
    dabx_subch_desc q{};
    q.subch_id = (int)c.sub_id[n]; q.cu_start = (int)(c.sub_span[n] & 0xFFFF); q.cu_size = (int)(c.sub_span[n] >> 16);
    q.kbps = (int)(c.sub_desc[n] & 0xFFF); q.prot_level = (int)((c.sub_desc[n] >> 12) & 15); q.short_form = (int)((c.sub_desc[n] >> 16) & 1);
    q.dab_plus = -1;
    for (int i = 0; i < c.n_comp; i++) {
      const unsigned f = c.comp_info[i];
      if (((f >> 4) & 3) == 0 && (int)((f >> 12) & 63) == q.subch_id) { q.dab_plus = ((f >> 6) & 63) == 63 ? 1 : 0; break; }
    }
    out[n] = q;
  }
  return n;
}
inline int fig_packet_components(const FigState &t, int next, dabx_packet_component *out, int max_out)
{
  const FigCfg &c = t.cfg[next ? t.cur ^ 1 : t.cur];
  int n = 0;
  for (; n < c.n_pkt && n < max_out; n++) {
    const unsigned f = c.pkt_info[n];
    dabx_packet_component q{(int)c.pkt_scid[n], (int)((f >> 8) & 63), (int)((f >> 14) & 1023), (int)((f >> 2) & 63), (int)((f >> 1) & 1), 0u};
    for (int i = 0; i < c.n_comp; i++)
      if (((c.comp_info[i] >> 4) & 3) == 3 && (int)((c.comp_info[i] >> 18) & 4095) == q.scid) { q.sid = c.comp_sid[i]; break; }
    out[n] = q;
  }
  return n;
}
// dabx_follow_fic's answer from a decoder's state (engine.cpp)
inline void fig_follow(const FigState &t, dabx_reconf *out)
{
  memset(out, 0, sizeof(*out));
  out->at_cif = out->last_change_cif = -1;
  out->frames_fed = t.fibs / 12;
  out->n_changes = t.n_changes;
  auto cif_of_fib = [](long long i) { return 4 * (i / 12) + (i % 12) / 3; };
  if (t.last_change_fib >= 0) out->last_change_cif = cif_of_fib(t.last_change_fib);
  if (t.change_flags != 0 && t.fig00_fib >= 0) {
    out->pending = 1;
    int ahead = ((t.occurrence - t.cif_lo) % 250 + 250) % 250;
    if (ahead == 0) ahead = 250;
    out->at_cif = cif_of_fib(t.fig00_fib) + ahead;
  }
}

// A decoder with everything it writes, as the host holds one (the host walk's decoder; a device decoder downloaded)
struct FigDecoder {
  FigState st;
  dabx_fig_label labels[FIG_LAB_SLOTS];
  dabx_fig_event ring[FIG_RING];
};
// ... and presented as dabx_fig_walk_device returns a decoder (include/dabx.h): every output optional, one decoder's row each
inline void fig_present(const FigDecoder &d, dabx_fibdec_info *info, int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets,
                        int32_t *n_labels, dabx_fig_label *labels, dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events)
{
  const FigState &t = d.st;
  if (info) fig_info(t, info);
  for (int k = 0; k < 2; k++) {
    const FigCfg &c = t.cfg[t.cur ^ k];
    if (n_tab) { n_tab[3 * k] = c.n_sub; n_tab[3 * k + 1] = c.n_comp; n_tab[3 * k + 2] = c.n_pkt; }
    if (subch) fig_subchannels(t, k, subch + (size_t)k * FIG_MAX_SUB, FIG_MAX_SUB);
    if (packets) fig_packet_components(t, k, packets + (size_t)k * FIG_MAX_PKT, FIG_MAX_PKT);
  }
  if (n_labels) *n_labels = t.n_labels;
  if (labels) memcpy(labels, d.labels, sizeof(dabx_fig_label) * (size_t)t.n_labels);
  if (stats) *stats = t.cnt;
  if (n_events) *n_events = t.cnt.events;
  if (events) {
    const long long total = t.cnt.events, n = total < FIG_RING ? total : FIG_RING;
    for (long long i = 0; i < n; i++) events[i] = d.ring[(total - n + i) % FIG_RING];
  }
}

// The engine's stage (k_fig): nothing of it exists until dabx_set_fig_mode first switches a stream on.
struct FigDev {
  FigState *st;                                  // [S]
  dabx_fig_label *labels;                        // [S][FIG_LAB_SLOTS]
  dabx_fig_event *ring;                          // [S][FIG_RING]
  int32_t *on;                                   // [S] the stream has the mode on
  FigSiState *si;                                // [S] the service information; nullptr until a stream first asks for it (dabx_fig_config.service_info)
  int32_t *si_on;                                // [S] the stream follows it
};

#ifdef __HIPCC__
// deliver.hip
struct EngineDev;
int launch_fig(const EngineDev &e, const FigDev &f, hipStream_t st);
int launch_fig_batch(const uint8_t *fibs, const uint8_t *crc_ok, int n_decoders, int n_fibs, FigState *st, FigSiState *si /* nullptr: without */,
                     dabx_fig_label *labels, dabx_fig_event *ring, hipStream_t stream);
int launch_fig_directory(const FigState *st, const FigSiState *si, const dabx_fig_label *labels, const int32_t *on, int first, int n, int next,
                         dabx_fig_service *out, long long out_stride, int max_per, int32_t *n_out, int n_stride, hipStream_t stream);
#endif

}  // namespace dabx

#include "fig_si_core.h"
