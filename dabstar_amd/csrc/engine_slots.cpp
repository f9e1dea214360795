// engine_slots.cpp -- the slots with output rings, packet mode, PAD and the MOT objects of the X-PAD and of a carousel: what their entry points share and
// dabx_set_*_mode, dabx_read_*, dabx_get_*_stats.
#include "engine.h"
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <type_traits>

namespace dabx {

// PadDev::n_mp2 follows the table: called behind every e->pad.upload()
void pad_count_sources(dabx_engine *e)
{
  int n = 0;
  for (const auto &h : e->pad.host) n += h.on && h.st.source == DABX_PAD_SOURCE_MP2 ? 1 : 0;
  e->pad.dev.n_mp2 = n;
}

// The MOT job table follows the PAD job table: called behind every e->pad.upload() that may have changed the PAD slots, with a fresh mirror
// of the MOT table (download with the engine drained).  A MOT slot whose PAD decoding is gone leaves the stage; the others learn their PAD
// slot's place in the rebuilt table.
int mot_follow_pad(dabx_engine *e)
{
  auto &tab = e->mot;
  if (tab.host.empty()) return 0;
  for (size_t sj = 0; sj < tab.host.size(); sj++) {
    if (!tab.host[sj].on) continue;
    if (!e->pad.on(sj)) tab.drop(sj);
    else tab.host[sj].st.pad_index = e->pad.index[sj];
  }
  return tab.upload();
}

// ... and the carousel job table the packet job table, in the same way (behind every e->pkt.upload())
int carousel_follow_packet(dabx_engine *e)
{
  auto &tab = e->car;
  if (tab.host.empty()) return 0;
  for (size_t sj = 0; sj < tab.host.size(); sj++) {
    if (!tab.host[sj].on) continue;
    if (!e->pkt.on(sj)) tab.drop(sj);
    else tab.host[sj].st.pkt_index = e->pkt.index[sj];
  }
  return tab.upload();
}

// ... and the data-handler job table, likewise
int data_follow_packet(dabx_engine *e)
{
  auto &tab = e->dat;
  if (tab.host.empty()) return 0;
  for (size_t sj = 0; sj < tab.host.size(); sj++) {
    if (!tab.host[sj].on) continue;
    if (!e->pkt.on(sj)) tab.drop(sj);
    else tab.host[sj].st.pkt_index = e->pkt.index[sj];
  }
  return tab.upload();
}

}  // namespace dabx

// ---- slots with output rings (out_ring.h): what the packet-mode and the PAD entry points below share -------------------------------------
static uint32_t pow2_at_least(size_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

// The rings of a slot that is switched on (n_bytes, n_rec: powers of two) and what one chunk of the bulk delivery has room for
// (extra: bytes the stage keeps behind the byte ring in the same allocation, freed with it)
template <class Rec> static bool out_ring_create(OutRing<Rec> *r, uint32_t n_bytes, uint32_t n_rec, uint32_t asm_room, uint32_t dl_rec_cap, uint32_t dl_bytes_cap,
                                                 size_t extra = 0)
{
  void *b = nullptr, *q = nullptr;
  if (hipMalloc(&b, (size_t)n_bytes + extra) != hipSuccess || hipMalloc(&q, sizeof(Rec) * (size_t)n_rec) != hipSuccess) {
    if (b) (void)hipFree(b);
    return false;
  }
  r->bytes = static_cast<uint8_t *>(b); r->recs = static_cast<Rec *>(q);
  r->bytes_mask = n_bytes - 1; r->rec_mask = n_rec - 1; r->asm_room = asm_room;
  r->dl_rec_cap = dl_rec_cap; r->dl_bytes_cap = dl_bytes_cap;
  return true;
}

// The tail of dabx_set_packet_mode / dabx_set_pad_mode / dabx_set_mot_mode (engine drained): the slab of an open delivery follows the
// stage's slots.  delivery_layout writes ALL job tables back from their mirrors, so the other stages' are refreshed first.
template <class... Tabs> static int relayout_open_delivery(dabx_engine *e, size_t sj, const SubchDev &sc, Tabs &...others)
{
  if (!e->dl.open) return 0;
  e->subch_host[sj] = sc;
  int rc_dl = 0;
  ((rc_dl = rc_dl ? rc_dl : others.download(e->dev.max_subch)), ...);
  if (rc_dl) return rc_dl;
  if (int rc = e->delivery_layout()) {
    const std::string why = dabx::last_error();
    delivery_free(e);
    set_error("%s -- the delivery has been closed", why.c_str());
    return rc;
  }
  return 0;
}

// The slot's table entry as the device holds it and the items [*lo, count) whose record and bytes are still intact (out_ring.h); older ones
// that no call has returned yet are counted as lost.  Reads the entry and, as a rule, ONE record (the oldest candidate's).
template <class Slot, class Dev> static int ring_window(dabx_engine *e, JobTable<Slot, Dev> &tab, size_t sj, Slot *st, long long *lo)
{
  if (int rc = sync_all(e)) return rc;
  DABX_HIP(hipMemcpy(st, tab.dev.slots + tab.index[sj], sizeof(Slot), hipMemcpyDeviceToHost));
  const auto &r = st->out;
  long long first = out_ring_oldest(r);
  while (first < r.count) {
    std::remove_reference_t<decltype(*r.recs)> q;
    DABX_HIP(hipMemcpy(&q, r.recs + (size_t)(first & r.rec_mask), sizeof(q), hipMemcpyDeviceToHost));
    if (out_ring_intact(r, q.byte_pos)) break;
    first++;
  }
  auto &h = tab.host[sj];
  if (first > h.seen) { h.lost += first - h.seen; h.seen = first; }
  *lo = first;
  return 0;
}

// dabx_read_datagroups / dabx_read_pad_items behind their argument checks: the newest n intact items, of these the newest that fit max_bytes
template <class Slot, class Dev, class Rec> static int ring_read(dabx_engine *e, JobTable<Slot, Dev> &tab, size_t sj, int n, Rec *info, uint8_t *bytes, size_t max_bytes)
{
  if (!tab.on(sj)) return 0;
  Slot st;
  long long lo = 0;
  if (int rc = ring_window(e, tab, sj, &st, &lo)) return rc;
  const OutRing<Rec> &r = st.out;
  long long from = std::max(lo, r.count - n);
  int have = (int)(r.count - from);
  if (have > 0) {                                             // the records [from, count): one or two runs of the ring
    const size_t ring = (size_t)r.rec_mask + 1, at = (size_t)(from & r.rec_mask), head = std::min<size_t>((size_t)have, ring - at);
    DABX_HIP(hipMemcpy(info, r.recs + at, sizeof(Rec) * head, hipMemcpyDeviceToHost));
    if ((size_t)have > head) DABX_HIP(hipMemcpy(info + head, r.recs, sizeof(Rec) * ((size_t)have - head), hipMemcpyDeviceToHost));
    int skip = 0;                                             // the newest items that fit
    if (bytes) while (skip < have && (unsigned long long)(r.n_bytes - info[skip].byte_pos) > max_bytes) skip++;
    if (skip) { memmove(info, info + skip, sizeof(Rec) * (size_t)(have - skip)); have -= skip; }
  }
  if (have > 0) {
    const long long base = info[0].byte_pos, total = r.n_bytes - base;
    for (int i = 0; i < have; i++) info[i].byte_pos -= base;
    if (bytes && total > 0) {
      const size_t ring = (size_t)r.bytes_mask + 1, at = (size_t)((unsigned long long)base & r.bytes_mask);
      const size_t head = std::min<size_t>((size_t)total, ring - at);
      DABX_HIP(hipMemcpy(bytes, r.bytes + at, head, hipMemcpyDeviceToHost));
      if ((size_t)total > head) DABX_HIP(hipMemcpy(bytes + head, r.bytes, (size_t)total - head, hipMemcpyDeviceToHost));
    }
  }
  tab.host[sj].seen = std::max(tab.host[sj].seen, r.count);
  return have;
}

// ---- slots with output rings: packet-mode data sub-channels (packet_core.h, k_packet) and programme-associated data (pad_core.h, k_pad) ----
static_assert(sizeof(dabx_chunk_dg) == 128 && sizeof(dabx_datagroup_info) == 32 && sizeof(dabx_packet_stats) == 128 && sizeof(dabx_packet_config) == 32, "include/dabx.h: packet-mode records");
static_assert(sizeof(dabx_chunk_pad) == 128 && sizeof(dabx_pad_item) == 32 && sizeof(dabx_pad_stats) == 128 && sizeof(dabx_pad_config) == 32, "include/dabx.h: PAD records");
static_assert(sizeof(dabx_chunk_mot) == 128 && sizeof(dabx_mot_object) == 32 && sizeof(dabx_mot_stats) == 128 && sizeof(dabx_mot_config) == 32, "include/dabx.h: MOT records");
static_assert(sizeof(dabx_carousel_stats) == 128 && sizeof(dabx_carousel_config) == 32, "include/dabx.h: carousel records");
static_assert(sizeof(dabx_data_item) == 32 && sizeof(dabx_data_stats) == 256 && sizeof(dabx_data_config) == 32 && offsetof(dabx_data_item, group) == 24 &&
              offsetof(dabx_data_stats, launches) == 232, "include/dabx.h: data-handler records");
static_assert(sizeof(dabx_mp2_sync_stats) == 64 && offsetof(dabx_pad_config, source) == 4, "include/dabx.h: PAD of MP2 frames");
static_assert(sizeof(dabx_mp2_audio_frame) == 32 && sizeof(dabx_mp2_audio_stats) == 64 && sizeof(dabx_mp2_audio_config) == 32 && offsetof(dabx_mp2_audio_frame, flags) == 28,
              "include/dabx.h: MP2 audio records");
static_assert(sizeof(dabx_aac_frame) == 32 && sizeof(dabx_aac_stream_stats) == 64 && sizeof(dabx_aac_stream_config) == 32 && offsetof(dabx_aac_frame, flags) == 23 &&
              offsetof(dabx_aac_frame, length) == 16, "include/dabx.h: AAC stream records");

extern "C" {

int dabx_set_packet_mode(dabx_engine *e, int stream, int j, const dabx_packet_config *cfg)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch) { set_error("dabx_set_packet_mode: bad argument"); return DABX_E_ARG; }
  if (cfg && (cfg->size < 2 * sizeof(int32_t) || cfg->packet_address < 0 || cfg->packet_address > 1023)) {
    set_error("dabx_set_packet_mode: bad configuration (size %u, packet address %d)", cfg->size, (int)cfg->packet_address);
    return DABX_E_ARG;
  }
  int rc;
  if ((rc = sync_all(e))) return rc;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  SubchDev sc;
  DABX_HIP(hipMemcpy(&sc, e->dev.subch + sj, sizeof(SubchDev), hipMemcpyDeviceToHost));
  if (!sc.active || sc.dab_plus || sc.kbps % 8 != 0 || sc.kbps > PKT_MAX_KBPS) {
    set_error("dabx_set_packet_mode: stream %d slot %d is %s", stream, j, !sc.active ? "not active" : sc.dab_plus ? "a DAB+ slot" : "not at a multiple of 8 kbit/s up to 384");
    return DABX_E_ARG;
  }
  if (cfg && e->pad.on(sj)) { set_error("dabx_set_packet_mode: stream %d slot %d has PAD decoding on", stream, j); return DABX_E_ARG; }
  if (cfg && e->mpa.on(sj)) { set_error("dabx_set_packet_mode: stream %d slot %d has MP2 audio decoding on", stream, j); return DABX_E_ARG; }
  if (cfg && e->aac.on(sj)) { set_error("dabx_set_packet_mode: stream %d slot %d has the AAC stream mode on", stream, j); return DABX_E_ARG; }
  auto &tab = e->pkt;
  if (tab.host.empty()) {
    if (!cfg) return 0;
    tab.host.resize((size_t)e->dev.n_streams * e->dev.max_subch);
    tab.index.assign(tab.host.size(), -1);
  }
  if ((rc = tab.download(e->dev.max_subch)) || (rc = e->car.download(e->dev.max_subch)) || (rc = e->dat.download(e->dev.max_subch))) return rc;
  tab.drop(sj);
  e->car.drop(sj);                                                     // the packet stage restarts with empty rings: nothing for k_carousel to follow
  e->dat.drop(sj);                                                     // ... or for k_data_handler
  if (cfg) {
    // two full batches (56 logical frames) of single-packet groups: a record per 24-byte packet, their payloads, and room for the series
    // under assembly, which lives in the byte ring in front of the completed groups (packet_core.h); a chunk: one batch of them
    decltype(e->pkt)::Host h;
    h.on = true;
    h.st.s = stream; h.st.j = j; h.st.address = cfg->packet_address; h.st.first_byte = -1; h.st.run_crc = 0xFFFFu;
    const size_t recs = (size_t)4 * MSC_BATCH_FRAMES * (sc.kbps / 8), bytes = (size_t)4 * MSC_BATCH_FRAMES * 3 * sc.kbps;
    if (!out_ring_create(&h.st.out, pow2_at_least(2 * bytes + DABX_DG_MAX_BYTES), pow2_at_least(2 * recs), DABX_DG_MAX_BYTES, (uint32_t)recs,
                         (uint32_t)(bytes + DABX_DG_MAX_BYTES))) {
      set_error("dabx_set_packet_mode: out of device memory");
      (void)tab.upload();
      (void)carousel_follow_packet(e);
      (void)data_follow_packet(e);
      return DABX_E_NOMEM;
    }
    tab.host[sj] = h;
  }
  if ((rc = tab.upload())) return rc;
  if ((rc = carousel_follow_packet(e))) return rc;
  if ((rc = data_follow_packet(e))) return rc;
  return relayout_open_delivery(e, sj, sc, e->pad, e->mot, e->car, e->mpa, e->aac, e->dat);
}

int dabx_read_datagroups(dabx_engine *e, int stream, int j, int n, dabx_datagroup_info *info, uint8_t *bytes, size_t max_bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || !info) { set_error("dabx_read_datagroups: bad argument"); return DABX_E_ARG; }
  return ring_read(e, e->pkt, (size_t)stream * e->dev.max_subch + j, n, info, bytes, max_bytes);
}

int dabx_get_packet_stats(dabx_engine *e, int stream, int j, dabx_packet_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_packet_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->pkt.on(sj)) return sync_all(e);
  PacketSlot st;
  long long lo = 0;
  if (int rc = ring_window(e, e->pkt, sj, &st, &lo)) return rc;
  out->frames = st.frames; out->packets = st.packets; out->addr_match = st.addr_match; out->continuity_err = st.continuity_err;
  out->crc_bad = st.crc_bad; out->len_bad = st.len_bad; out->walk_short = st.walk_short; out->dg_count = st.out.count;
  out->dg_bytes = st.out.n_bytes; out->dg_crc_bad = st.dg_crc_bad; out->dg_overflow = st.dg_overflow; out->dg_lost = e->pkt.host[sj].lost;
  out->active = 1; out->packet_address = st.address;
  return 0;
}

int dabx_set_pad_mode(dabx_engine *e, int stream, int j, const dabx_pad_config *cfg)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch) { set_error("dabx_set_pad_mode: bad argument"); return DABX_E_ARG; }
  if (cfg && cfg->size < sizeof(uint32_t)) { set_error("dabx_set_pad_mode: bad configuration (size %u)", cfg->size); return DABX_E_ARG; }
  int rc;
  if ((rc = sync_all(e))) return rc;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  SubchDev sc;
  DABX_HIP(hipMemcpy(&sc, e->dev.subch + sj, sizeof(SubchDev), hipMemcpyDeviceToHost));
  const int source = cfg && cfg->size >= 2 * sizeof(uint32_t) ? cfg->source : DABX_PAD_SOURCE_DABPLUS;
  if (source != DABX_PAD_SOURCE_DABPLUS && source != DABX_PAD_SOURCE_MP2) { set_error("dabx_set_pad_mode: unknown source %d", source); return DABX_E_ARG; }
  if (source == DABX_PAD_SOURCE_MP2) {
    if (!sc.active || sc.dab_plus || e->pkt.on(sj) || sc.kbps % 8 != 0 || sc.kbps > PKT_MAX_KBPS) {
      set_error("dabx_set_pad_mode: source MP2: stream %d slot %d is %s", stream, j, !sc.active ? "not active" : sc.dab_plus ? "a DAB+ slot" :
                e->pkt.on(sj) ? "in packet mode" : "not at a multiple of 8 kbit/s up to 384");
      return DABX_E_ARG;
    }
  } else if (!(cfg == nullptr && e->pad.on(sj)) && (!sc.active || sc.dab_plus != 1 || !e->dev.sf_info)) {      // (NULL also switches an MP2 source slot off)
    set_error("dabx_set_pad_mode: stream %d slot %d is %s", stream, j, !sc.active ? "not active" : "not a DAB+ slot");
    return DABX_E_ARG;
  }
  auto &tab = e->pad;
  if (tab.host.empty()) {
    if (!cfg) return 0;
    tab.host.resize((size_t)e->dev.n_streams * e->dev.max_subch);
    tab.index.assign(tab.host.size(), -1);
  }
  if ((rc = tab.download(e->dev.max_subch)) || (rc = e->mot.download(e->dev.max_subch))) return rc;
  tab.drop(sj);
  e->mot.drop(sj);                                                     // PAD restarts with empty rings: nothing for k_mot to follow
  if (cfg) {
    decltype(e->pad)::Host h;
    h.on = true;
    h.st.s = stream; h.st.j = j; h.st.sf_seen = sc.sf_count;           // the walk starts with the next super frame completed
    h.st.h.xpad_length = -1; h.st.h.segment_number = -1; h.st.h.segment_no = -1;       // pad_handler.h:74, :79, :83
    h.st.source = source;
    h.st.m.sample_rate = 48000; h.st.m.last_sync_bit = -1;             // mp2processor.cpp:236-240: SearchingForSync, both counts 0
    if (!out_ring_create(&h.st.out, PAD_BYTE_RING, PAD_ITEM_RING, PAD_ASM_ROOM, PAD_DL_ITEM_CAP, PAD_DL_BYTES_CAP)) {      // (pad_core.h has the derivations)
      set_error("dabx_set_pad_mode: out of device memory");
      (void)tab.upload();
      pad_count_sources(e);
      (void)mot_follow_pad(e);
      return DABX_E_NOMEM;
    }
    tab.host[sj] = h;
  }
  if ((rc = tab.upload())) return rc;
  pad_count_sources(e);
  if ((rc = mot_follow_pad(e))) return rc;
  return relayout_open_delivery(e, sj, sc, e->pkt, e->mot, e->car, e->mpa, e->aac, e->dat);
}

int dabx_get_mp2_sync_stats(dabx_engine *e, int stream, int j, dabx_mp2_sync_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_mp2_sync_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->pad.on(sj) || e->pad.host[sj].st.source != DABX_PAD_SOURCE_MP2) return sync_all(e);
  if (int rc = sync_all(e)) return rc;
  PadSlot st;
  DABX_HIP(hipMemcpy(&st, e->pad.dev.slots + e->pad.index[sj], sizeof(PadSlot), hipMemcpyDeviceToHost));
  const Mp2State &m = st.m;
  out->syncs = m.syncs; out->frames = m.frames; out->hdr_refused = m.hdr_refused; out->rate_unsupported = m.rate_unsupported;
  out->sample_rate = m.sample_rate; out->state = m.state; out->bit_count = m.bit_count; out->header_count = m.header_count;
  out->last_sync_bit = m.last_sync_bit; out->active = 1;
  return 0;
}

int dabx_read_pad_items(dabx_engine *e, int stream, int j, int n, dabx_pad_item *info, uint8_t *bytes, size_t max_bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || !info) { set_error("dabx_read_pad_items: bad argument"); return DABX_E_ARG; }
  return ring_read(e, e->pad, (size_t)stream * e->dev.max_subch + j, n, info, bytes, max_bytes);
}

int dabx_get_pad_stats(dabx_engine *e, int stream, int j, dabx_pad_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_pad_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->pad.on(sj)) return sync_all(e);
  PadSlot st;
  long long lo = 0;
  if (int rc = ring_window(e, e->pad, sj, &st, &lo)) return rc;
  const PadCounters &c = st.c;
  auto i32 = [](long long v) { return (int32_t)std::min<long long>(v, INT32_MAX); };
  out->superframes = c.superframes; out->aus = c.aus; out->pad_aus = c.pad_aus; out->fpad_other = c.fpad_other; out->xpad_short = c.xpad_short;
  out->xpad_variable = c.xpad_variable; out->xpad_other = c.xpad_other; out->pad_bad = c.pad_bad; out->labels = c.labels;
  out->label_bytes = c.label_bytes; out->groups = c.groups; out->group_bytes = c.group_bytes; out->items_lost = e->pad.host[sj].lost;
  out->li_bad = i32(c.li_bad); out->dl_overflow = i32(c.dl_overflow); out->dg_crc_bad = i32(c.dg_crc_bad); out->dg_small = i32(c.dg_small);
  out->active = 1;
  return 0;
}

// ---- MP2 audio (mp2_core.h, k_mp2_audio) -------------------------------------------------------------------------------------------------
int dabx_set_mp2_audio_mode(dabx_engine *e, int stream, int j, const dabx_mp2_audio_config *cfg)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch) { set_error("dabx_set_mp2_audio_mode: bad argument"); return DABX_E_ARG; }
  if (cfg && cfg->size < sizeof(uint32_t)) { set_error("dabx_set_mp2_audio_mode: bad configuration (size %u)", cfg->size); return DABX_E_ARG; }
  int rc;
  if ((rc = sync_all(e))) return rc;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  SubchDev sc;
  DABX_HIP(hipMemcpy(&sc, e->dev.subch + sj, sizeof(SubchDev), hipMemcpyDeviceToHost));
  if (!(cfg == nullptr && e->mpa.on(sj)) && (!sc.active || sc.dab_plus || e->pkt.on(sj) || sc.kbps % 8 != 0 || sc.kbps > MP2A_MAX_KBPS)) {      // the rules of DABX_PAD_SOURCE_MP2
    set_error("dabx_set_mp2_audio_mode: stream %d slot %d is %s", stream, j, !sc.active ? "not active" : sc.dab_plus ? "a DAB+ slot" :
              e->pkt.on(sj) ? "in packet mode" : "not at a multiple of 8 kbit/s up to 384");
    return DABX_E_ARG;
  }
  auto &tab = e->mpa;
  if (tab.host.empty()) {
    if (!cfg) return 0;
    tab.host.resize((size_t)e->dev.n_streams * e->dev.max_subch);
    tab.index.assign(tab.host.size(), -1);
  }
  if ((rc = tab.download(e->dev.max_subch))) return rc;
  tab.drop(sj);
  if (cfg) {
    decltype(e->mpa)::Host h;
    h.on = true;
    h.st.s = stream; h.st.j = j;
    h.st.m.sample_rate = 48000; h.st.m.last_sync_bit = -1;             // mp2processor.cpp:234-242: SearchingForSync, every count and Voffs 0
    if (!out_ring_create(&h.st.out, MP2A_BYTE_RING, MP2A_REC_RING, MP2A_PCM_BYTES, MP2A_DL_REC_CAP, MP2A_DL_BYTES_CAP, MP2A_EXTRA_BYTES)) {      // (mp2_core.h has the derivations)
      set_error("dabx_set_mp2_audio_mode: out of device memory");
      (void)tab.upload();
      return DABX_E_NOMEM;
    }
    h.st.hist = reinterpret_cast<int32_t *>(h.st.out.bytes + MP2A_BYTE_RING);
    h.st.mp2frame = reinterpret_cast<uint8_t *>(h.st.hist + 2 * MP2A_HIST_ROWS * 64);
    tab.host[sj] = h;
    if (hipMemset(h.st.hist, 0, MP2A_EXTRA_BYTES) != hipSuccess) {     // V and MP2frame zero (:215-221, :237)
      tab.drop(sj);
      (void)tab.upload();
      set_error("dabx_set_mp2_audio_mode: clearing the decoder state failed");
      return DABX_E_HIP;
    }
  }
  if ((rc = tab.upload())) return rc;
  return relayout_open_delivery(e, sj, sc, e->pkt, e->pad, e->mot, e->car, e->aac, e->dat);
}

int dabx_read_mp2_audio(dabx_engine *e, int stream, int j, int n, dabx_mp2_audio_frame *recs, uint8_t *pcm, size_t max_bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || !recs) { set_error("dabx_read_mp2_audio: bad argument"); return DABX_E_ARG; }
  return ring_read(e, e->mpa, (size_t)stream * e->dev.max_subch + j, n, recs, pcm, max_bytes);
}

int dabx_get_mp2_audio_stats(dabx_engine *e, int stream, int j, dabx_mp2_audio_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_mp2_audio_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  out->launches = e->mpa_launches;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->mpa.on(sj)) return sync_all(e);
  Mp2AudioSlot st;
  long long lo = 0;
  if (int rc = ring_window(e, e->mpa, sj, &st, &lo)) return rc;
  const Mp2AudioState &a = st.a;
  out->decode_calls = a.decode_calls; out->frames_out = a.frames_out; out->bad_header = a.bad_header; out->refused = a.refused; out->overread = a.overread;
  out->sample_rate = st.m.sample_rate; out->frames_lost = (int32_t)std::min<long long>(e->mpa.host[sj].lost, INT32_MAX);
  out->number_of_frames = (int16_t)a.number_of_frames; out->error_frames = (int16_t)a.error_frames; out->voffs = (int16_t)a.voffs; out->active = 1;
  return 0;
}

// ---- AAC stream (aac_core.h, k_aac_stream) ------------------------------------------------------------------------------------------------
int dabx_set_aac_stream_mode(dabx_engine *e, int stream, int j, const dabx_aac_stream_config *cfg)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch) { set_error("dabx_set_aac_stream_mode: bad argument"); return DABX_E_ARG; }
  if (cfg && cfg->size < sizeof(dabx_aac_stream_config)) { set_error("dabx_set_aac_stream_mode: bad configuration (size %u)", cfg->size); return DABX_E_ARG; }
  if (cfg && cfg->format != 0) { set_error("dabx_set_aac_stream_mode: unknown format %d (0 = LOAS)", cfg->format); return DABX_E_ARG; }
  if (cfg) for (int r : cfg->reserved) if (r) { set_error("dabx_set_aac_stream_mode: a reserved word is not 0"); return DABX_E_ARG; }
  int rc;
  if ((rc = sync_all(e))) return rc;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  SubchDev sc;
  DABX_HIP(hipMemcpy(&sc, e->dev.subch + sj, sizeof(SubchDev), hipMemcpyDeviceToHost));
  if (!(cfg == nullptr && e->aac.on(sj)) && (!sc.active || sc.dab_plus != 1 || e->pkt.on(sj) || !e->dev.sf_info)) {
    set_error("dabx_set_aac_stream_mode: stream %d slot %d is %s", stream, j, !sc.active ? "not active" : e->pkt.on(sj) ? "in packet mode" : "not a DAB+ slot");
    return DABX_E_ARG;
  }
  auto &tab = e->aac;
  if (tab.host.empty()) {
    if (!cfg) return 0;
    tab.host.resize((size_t)e->dev.n_streams * e->dev.max_subch);
    tab.index.assign(tab.host.size(), -1);
  }
  if ((rc = tab.download(e->dev.max_subch))) return rc;
  tab.drop(sj);
  if (cfg) {
    decltype(e->aac)::Host h;
    h.on = true;
    h.st.s = stream; h.st.j = j; h.st.sf_seen = sc.sf_count;           // the walk starts with the next super frame completed
    const uint32_t batch = aac_batch_bytes(sc.kbps);                   // (aac_core.h has the derivation)
    if (!out_ring_create(&h.st.out, pow2_at_least(2 * (size_t)batch), AAC_REC_RING, AAC_MAX_FRAME_BYTES, AAC_DL_REC_CAP, batch)) {
      set_error("dabx_set_aac_stream_mode: out of device memory");
      (void)tab.upload();
      return DABX_E_NOMEM;
    }
    tab.host[sj] = h;
  }
  if ((rc = tab.upload())) return rc;
  return relayout_open_delivery(e, sj, sc, e->pkt, e->pad, e->mot, e->car, e->mpa, e->dat);
}

int dabx_read_aac_frames(dabx_engine *e, int stream, int j, int n, dabx_aac_frame *recs, uint8_t *bytes, size_t max_bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || !recs) { set_error("dabx_read_aac_frames: bad argument"); return DABX_E_ARG; }
  return ring_read(e, e->aac, (size_t)stream * e->dev.max_subch + j, n, recs, bytes, max_bytes);
}

int dabx_get_aac_stream_stats(dabx_engine *e, int stream, int j, dabx_aac_stream_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_aac_stream_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  out->launches = e->aac_launches;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->aac.on(sj)) return sync_all(e);
  AacStreamSlot st;
  long long lo = 0;
  if (int rc = ring_window(e, e->aac, sj, &st, &lo)) return rc;
  out->superframes = st.superframes; out->records = st.records; out->frames = st.frames; out->frame_bytes = st.frame_bytes;
  out->lost_len = st.lost_len; out->lost_crc = st.lost_crc; out->lost = e->aac.host[sj].lost;
  return 0;
}

// ---- MOT objects of the X-PAD (mot_core.h, k_mot) ----------------------------------------------------------------------------------------
int dabx_set_mot_mode(dabx_engine *e, int stream, int j, const dabx_mot_config *cfg)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch) { set_error("dabx_set_mot_mode: bad argument"); return DABX_E_ARG; }
  if (cfg && cfg->size < sizeof(uint32_t)) { set_error("dabx_set_mot_mode: bad configuration (size %u)", cfg->size); return DABX_E_ARG; }
  const uint32_t max_bytes = cfg && cfg->size >= 2 * sizeof(uint32_t) && cfg->max_object_bytes ? cfg->max_object_bytes : MOT_OBJECT_BYTES_DEFAULT;
  if (max_bytes < MOT_OBJECT_BYTES_MIN || max_bytes > MOT_OBJECT_BYTES_MAX) {
    set_error("dabx_set_mot_mode: max_object_bytes %u is not within %u .. %u", max_bytes, MOT_OBJECT_BYTES_MIN, MOT_OBJECT_BYTES_MAX);
    return DABX_E_ARG;
  }
  int rc;
  if ((rc = sync_all(e))) return rc;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (cfg && !e->pad.on(sj)) { set_error("dabx_set_mot_mode: stream %d slot %d has no PAD decoding (dabx_set_pad_mode)", stream, j); return DABX_E_ARG; }
  SubchDev sc;
  DABX_HIP(hipMemcpy(&sc, e->dev.subch + sj, sizeof(SubchDev), hipMemcpyDeviceToHost));
  auto &tab = e->mot;
  if (tab.host.empty()) {
    if (!cfg) return 0;
    tab.host.resize((size_t)e->dev.n_streams * e->dev.max_subch);
    tab.index.assign(tab.host.size(), -1);
  }
  if ((rc = tab.download(e->dev.max_subch))) return rc;
  tab.drop(sj);
  if (cfg) {
    decltype(e->mot)::Host h;
    h.on = true;
    h.st.s = stream; h.st.j = j; h.st.pad_index = e->pad.index[sj]; h.st.max_object_bytes = max_bytes;
    PadSlot ps;                                                        // the walk starts with the next PAD item emitted
    DABX_HIP(hipMemcpy(&ps, e->pad.dev.slots + e->pad.index[sj], sizeof(PadSlot), hipMemcpyDeviceToHost));
    h.st.items_seen = ps.out.count;
    h.st.h.transport_id = -1; h.st.h.num_segments = -1; h.st.h.max_seg = -1;      // mot_object.h:82-83
    const uint32_t ring = mot_byte_ring(max_bytes);                    // (mot_core.h has the derivations)
    if (!out_ring_create(&h.st.out, ring, MOT_REC_RING, 0, MOT_DL_REC_CAP, 2 * max_bytes, mot_extra_bytes(max_bytes))) {
      set_error("dabx_set_mot_mode: out of device memory");
      (void)tab.upload();
      return DABX_E_NOMEM;
    }
    h.st.arena = h.st.out.bytes + ring;
    h.st.name = h.st.arena + (((size_t)max_bytes + 7) & ~(size_t)7);
    h.st.table = reinterpret_cast<MotSeg *>(h.st.name + MOT_NAME_ROOM);
    tab.host[sj] = h;
    if (hipMemset(h.st.table, 0xFF, sizeof(MotSeg) * MOT_MAX_SEGMENTS) != hipSuccess) {       // every segment number absent (MOT_ABSENT)
      tab.drop(sj);
      (void)tab.upload();
      set_error("dabx_set_mot_mode: clearing the segment table failed");
      return DABX_E_HIP;
    }
  }
  if ((rc = tab.upload())) return rc;
  return relayout_open_delivery(e, sj, sc, e->pkt, e->pad, e->car, e->mpa, e->aac, e->dat);
}

int dabx_read_mot_objects(dabx_engine *e, int stream, int j, int n, dabx_mot_object *info, uint8_t *bytes, size_t max_bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || !info) { set_error("dabx_read_mot_objects: bad argument"); return DABX_E_ARG; }
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (e->car.on(sj)) return ring_read(e, e->car, sj, n, info, bytes, max_bytes);      // (a slot is a PAD slot or a packet slot, never both)
  return ring_read(e, e->mot, sj, n, info, bytes, max_bytes);
}

int dabx_get_mot_stats(dabx_engine *e, int stream, int j, dabx_mot_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_mot_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->mot.on(sj)) return sync_all(e);
  MotSlot st;
  long long lo = 0;
  if (int rc = ring_window(e, e->mot, sj, &st, &lo)) return rc;
  const MotCounters &c = st.c;
  auto i32 = [](long long v) { return (int32_t)std::min<long long>(v, INT32_MAX); };
  out->objects = st.out.count; out->object_bytes = st.out.n_bytes; out->objects_lost = e->mot.host[sj].lost;
  out->groups = c.groups; out->headers = c.headers; out->segments = c.segments;
  out->crc_bad = i32(c.crc_bad); out->type_other = i32(c.type_other); out->no_tid = i32(c.no_tid); out->grp_short = i32(c.grp_short);
  out->hdr_bad = i32(c.hdr_bad); out->seg_number_bad = i32(c.seg_number_bad); out->seg_duplicate = i32(c.seg_duplicate); out->resets = i32(c.resets);
  out->obj_overflow = i32(c.obj_overflow); out->pad_overrun = i32(c.pad_overrun); out->progress_events = i32(c.progress_events);
  out->progress_pct = st.h.progress_pct; out->transport_id = st.h.transport_id; out->segments_stored = st.h.n_stored; out->active = 1;
  return 0;
}

// ---- MOT objects of a packet-mode carousel (carousel_core.h, k_carousel) -----------------------------------------------------------------
int dabx_set_carousel_mode(dabx_engine *e, int stream, int j, const dabx_carousel_config *cfg)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch) { set_error("dabx_set_carousel_mode: bad argument"); return DABX_E_ARG; }
  if (cfg && cfg->size < sizeof(uint32_t)) { set_error("dabx_set_carousel_mode: bad configuration (size %u)", cfg->size); return DABX_E_ARG; }
  auto field = [&](size_t at, uint32_t v, uint32_t dflt) { return cfg && cfg->size >= at + sizeof(uint32_t) && v ? v : dflt; };
  const uint32_t max_bytes = field(4, cfg ? cfg->max_object_bytes : 0, MOT_OBJECT_BYTES_DEFAULT);
  const uint32_t max_objects = field(8, cfg ? cfg->max_dir_objects : 0, CAR_DIR_OBJECTS_DEFAULT);
  const uint32_t max_dir = field(12, cfg ? cfg->max_dir_bytes : 0, CAR_DIR_BYTES_DEFAULT);
  if (max_bytes < MOT_OBJECT_BYTES_MIN || max_bytes > MOT_OBJECT_BYTES_MAX || max_objects > CAR_DIR_OBJECTS_MAX || max_dir < CAR_DIR_BYTES_MIN || max_dir > CAR_DIR_BYTES_MAX) {
    set_error("dabx_set_carousel_mode: max_object_bytes %u is not within %u .. %u, max_dir_objects %u is above %u or max_dir_bytes %u is not within %u .. %u",
              max_bytes, MOT_OBJECT_BYTES_MIN, MOT_OBJECT_BYTES_MAX, max_objects, CAR_DIR_OBJECTS_MAX, max_dir, CAR_DIR_BYTES_MIN, CAR_DIR_BYTES_MAX);
    return DABX_E_ARG;
  }
  int rc;
  if ((rc = sync_all(e))) return rc;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (cfg && !e->pkt.on(sj)) { set_error("dabx_set_carousel_mode: stream %d slot %d is not in packet mode (dabx_set_packet_mode)", stream, j); return DABX_E_ARG; }
  SubchDev sc;
  DABX_HIP(hipMemcpy(&sc, e->dev.subch + sj, sizeof(SubchDev), hipMemcpyDeviceToHost));
  auto &tab = e->car;
  if (tab.host.empty()) {
    if (!cfg) return 0;
    tab.host.resize((size_t)e->dev.n_streams * e->dev.max_subch);
    tab.index.assign(tab.host.size(), -1);
  }
  if ((rc = tab.download(e->dev.max_subch))) return rc;
  tab.drop(sj);
  if (cfg) {
    decltype(e->car)::Host h;
    h.on = true;
    CarouselSlot &st = h.st;
    st.s = stream; st.j = j; st.pkt_index = e->pkt.index[sj];
    st.max_object_bytes = max_bytes; st.max_dir_objects = max_objects; st.max_dir_bytes = max_dir;
    PacketSlot ps;                                                     // the walk starts with the next data group completed
    DABX_HIP(hipMemcpy(&ps, e->pkt.dev.slots + e->pkt.index[sj], sizeof(PacketSlot), hipMemcpyDeviceToHost));
    st.groups_seen = ps.out.count;
    for (CarEntry &q : st.cache) q = CarEntry{-1, 0};                  // mot_handler.cpp:42-46
    const uint32_t ring = mot_byte_ring(max_bytes);                    // (mot_core.h has the derivations)
    const size_t extra = car_extra_bytes(max_bytes, max_objects, max_dir), n_obj = CAR_CACHE + max_objects;
    if (!out_ring_create(&st.out, ring, MOT_REC_RING, 0, MOT_DL_REC_CAP, 2 * max_bytes, extra)) {
      set_error("dabx_set_carousel_mode: out of device memory");
      (void)tab.upload();
      return DABX_E_NOMEM;
    }
    st.stores = st.out.bytes + ring;
    st.store_bytes = mot_extra_bytes(max_bytes);
    st.dir = st.stores + n_obj * st.store_bytes;
    st.marked = reinterpret_cast<uint32_t *>(st.dir + car_align8(max_dir));
    st.comp = st.marked + CAR_DIR_SEGMENTS / 32;
    st.obj = reinterpret_cast<MotState *>(reinterpret_cast<uint8_t *>(st.comp) + car_align8(4 * (size_t)max_objects));
    tab.host[sj] = h;
    MotState fresh{};
    fresh.transport_id = -1; fresh.num_segments = -1; fresh.max_seg = -1;          // mot_object.h:82-83
    const std::vector<MotState> objs(n_obj, fresh);
    // every segment number of every store absent (MOT_ABSENT); no directory, no mark, no component in use
    if (hipMemset(st.stores, 0xFF, n_obj * st.store_bytes) != hipSuccess ||
        hipMemset(st.dir, 0, (size_t)(reinterpret_cast<uint8_t *>(st.obj) - st.dir)) != hipSuccess ||
        hipMemcpy(st.obj, objs.data(), sizeof(MotState) * n_obj, hipMemcpyHostToDevice) != hipSuccess) {
      tab.drop(sj);
      (void)tab.upload();
      set_error("dabx_set_carousel_mode: clearing the object stores failed");
      return DABX_E_HIP;
    }
  }
  if ((rc = tab.upload())) return rc;
  return relayout_open_delivery(e, sj, sc, e->pkt, e->pad, e->mot, e->mpa, e->aac, e->dat);
}

int dabx_get_carousel_stats(dabx_engine *e, int stream, int j, dabx_carousel_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_carousel_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->car.on(sj)) return sync_all(e);
  CarouselSlot st;
  long long lo = 0;
  if (int rc = ring_window(e, e->car, sj, &st, &lo)) return rc;
  const MotCounters &c = st.c;
  const CarCounters &x = st.x;
  auto i32 = [](long long v) { return (int32_t)std::min<long long>(v, INT32_MAX); };
  out->objects = st.out.count; out->object_bytes = st.out.n_bytes; out->objects_lost = e->car.host[sj].lost;
  out->groups = i32(x.groups); out->headers = i32(c.headers); out->segments = i32(c.segments);
  out->crc_bad = i32(c.crc_bad); out->type_other = i32(c.type_other); out->no_tid = i32(c.no_tid); out->grp_short = i32(c.grp_short);
  out->hdr_bad = i32(c.hdr_bad); out->seg_number_bad = i32(c.seg_number_bad); out->seg_duplicate = i32(c.seg_duplicate); out->resets = i32(c.resets);
  out->obj_overflow = i32(c.obj_overflow); out->hdr_known = i32(x.hdr_known); out->hdr_not_first = i32(x.hdr_not_first); out->from_body = i32(x.from_body);
  out->evictions = i32(x.evictions); out->dirs_begun = i32(x.dirs_begun); out->dirs_repeated = i32(x.dirs_repeated); out->dirs_refused = i32(x.dirs_refused);
  out->dir_segments = i32(x.dir_segments); out->dir_objects = i32(x.dir_objects); out->dir_short = i32(x.dir_short); out->dir_seg_bad = i32(x.dir_seg_bad);
  out->dir_cut = i32(x.dir_cut); out->dg_overrun = i32(x.dg_overrun); out->active = 1;
  return 0;
}

// ---- the data handlers of a packet-mode slot (data_core.h, k_data_handler) ----------------------------------------------------------------
int dabx_set_data_mode(dabx_engine *e, int stream, int j, const dabx_data_config *cfg)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch) { set_error("dabx_set_data_mode: bad argument"); return DABX_E_ARG; }
  if (cfg && (cfg->size < 2 * sizeof(uint32_t) || cfg->handler < DABX_DATA_HANDLER_TDC || cfg->handler > DABX_DATA_HANDLER_JOURNALINE)) {
    set_error("dabx_set_data_mode: bad configuration (size %u, handler %d)", cfg->size, cfg->size >= 2 * sizeof(uint32_t) ? (int)cfg->handler : 0);
    return DABX_E_ARG;
  }
  if (cfg && cfg->size >= sizeof(dabx_data_config)) for (int r : cfg->reserved) if (r) { set_error("dabx_set_data_mode: a reserved word is not 0"); return DABX_E_ARG; }
  const int only_new = cfg && cfg->size >= 3 * sizeof(uint32_t) && cfg->only_new_revisions ? 1 : 0;
  int rc;
  if ((rc = sync_all(e))) return rc;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (cfg && !e->pkt.on(sj)) { set_error("dabx_set_data_mode: stream %d slot %d is not in packet mode (dabx_set_packet_mode)", stream, j); return DABX_E_ARG; }
  auto &tab = e->dat;
  if (tab.host.empty()) {
    if (!cfg) return 0;
    tab.host.resize((size_t)e->dev.n_streams * e->dev.max_subch);
    tab.index.assign(tab.host.size(), -1);
  }
  PacketSlot ps{};                                                     // the walk starts with the next data group completed (read before
  if (cfg) DABX_HIP(hipMemcpy(&ps, e->pkt.dev.slots + e->pkt.index[sj], sizeof(PacketSlot), hipMemcpyDeviceToHost));      // anything is dropped)
  if ((rc = tab.download(e->dev.max_subch))) return rc;
  tab.drop(sj);
  if (cfg) {
    decltype(e->dat)::Host h;
    h.on = true;
    DataSlot &st = h.st;
    st.s = stream; st.j = j; st.pkt_index = e->pkt.index[sj]; st.handler = cfg->handler; st.only_new = only_new;
    st.groups_seen = ps.out.count;
    // a handler's output is never longer than the groups it reads: the packet slot's byte ring, and in a chunk of the delivery the packet
    // slot's room; nothing is written beyond n_bytes before an item is complete
    const bool jl = cfg->handler == DABX_DATA_HANDLER_JOURNALINE;
    if (!out_ring_create(&st.out, ps.out.bytes_mask + 1, DATA_REC_RING, 0, DATA_REC_RING, ps.out.dl_bytes_cap, jl ? DATA_JL_TABLE : 0)) {
      set_error("dabx_set_data_mode: out of device memory");
      (void)tab.upload();
      return DABX_E_NOMEM;
    }
    tab.host[sj] = h;
    if (jl) {
      tab.host[sj].st.jl = st.out.bytes + (size_t)st.out.bytes_mask + 1;
      if (hipMemset(tab.host[sj].st.jl, DATA_JL_NONE, DATA_JL_TABLE) != hipSuccess) {      // no object id filed
        tab.drop(sj);
        (void)tab.upload();
        set_error("dabx_set_data_mode: clearing the Journaline table failed");
        return DABX_E_HIP;
      }
    }
  }
  if ((rc = tab.upload())) return rc;
  SubchDev sc;
  DABX_HIP(hipMemcpy(&sc, e->dev.subch + sj, sizeof(SubchDev), hipMemcpyDeviceToHost));
  return relayout_open_delivery(e, sj, sc, e->pkt, e->pad, e->mot, e->car, e->mpa, e->aac);
}

int dabx_read_data_items(dabx_engine *e, int stream, int j, int n, dabx_data_item *info, uint8_t *bytes, size_t max_bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || !info) { set_error("dabx_read_data_items: bad argument"); return DABX_E_ARG; }
  return ring_read(e, e->dat, (size_t)stream * e->dev.max_subch + j, n, info, bytes, max_bytes);
}

int dabx_get_data_stats(dabx_engine *e, int stream, int j, dabx_data_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) { set_error("dabx_get_data_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  out->launches = e->dat_ctl.launches;
  const size_t sj = (size_t)stream * e->dev.max_subch + j;
  if (!e->dat.on(sj)) return sync_all(e);
  DataSlot st;
  long long lo = 0;
  if (int rc = ring_window(e, e->dat, sj, &st, &lo)) return rc;
  out->groups = st.groups; out->items = st.out.count; out->bytes = st.out.n_bytes; out->lost = e->dat.host[sj].lost;
  memcpy(&out->dg_overrun, &st.c, sizeof(DataCounters));
  out->active = 1; out->handler = st.handler;
  return 0;
}

int dabx_data_handler_for(int dscty, int app_type) { return data_handler_for(dscty, app_type); }

// Measuring entry (tools/bench_data_handlers.py; not part of include/dabx.h), as dabx_internal_fig_timing: on = 1, every k_data_handler launch
// from now on lies between two events of its own; on = 0, the engine is drained, the launches' times go to ms[0 .. max), oldest first, and the
// events are freed.  Returns the number of launches that were timed.
int dabx_internal_data_timing(dabx_engine *e, int on, float *ms, int max)
{
  if (!e || (max > 0 && !ms) || max < 0) { set_error("dabx_internal_data_timing: bad argument"); return DABX_E_ARG; }
  if (int rc = sync_all(e)) return rc;
  DataStageCtl &T = e->dat_ctl;
  const int n = (int)(T.timed.size() / 2);
  for (int i = 0; i < n; i++) {
    float v = 0.f;
    if (i < max && hipEventElapsedTime(&v, T.timed[2 * (size_t)i], T.timed[2 * (size_t)i + 1]) == hipSuccess) ms[i] = v;
    (void)hipEventDestroy(T.timed[2 * (size_t)i]);
    (void)hipEventDestroy(T.timed[2 * (size_t)i + 1]);
  }
  T.timed.clear();
  T.timing = on != 0;
  return n;
}

}  // extern "C"
