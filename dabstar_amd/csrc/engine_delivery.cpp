// engine_delivery.cpp -- bulk delivery (include/dabx.h "Bulk delivery"): the slab layout, the copier thread and the dabx_delivery_* entries.
#include "engine.h"
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

// ---- bulk delivery (include/dabx.h "Bulk delivery", deliver.hip) -------------------------------------------------------
// the slab's records are ABI: hosts and the python binding (dabstar_amd/lib.py, CHUNK_*) parse them by these sizes
static_assert(sizeof(dabx_chunk_header) == 128 && sizeof(dabx_chunk_stream) == 72 && sizeof(dabx_chunk_frame) == 16 && sizeof(dabx_chunk_subch) == 144 && offsetof(dabx_chunk_header, off_mot) == 112 &&
              sizeof(dabx_superframe_info) == 32 && sizeof(dabx_chunk_eti) == 64 && offsetof(dabx_chunk_header, off_eti) == 120 &&
              sizeof(dabx_chunk_header_ext) == 64 && sizeof(dabx_chunk_tii) == 32 && sizeof(dabx_tii_event) == 32 && sizeof(dabx_tii_result) == 16 &&
              sizeof(dabx_chunk_mp2_audio) == 128 && offsetof(dabx_chunk_header_ext, off_mp2_audio) == 16 &&
              sizeof(dabx_chunk_aac) == 128 && offsetof(dabx_chunk_header_ext, off_aac) == 24 &&
              sizeof(dabx_chunk_header_ext2) == 64 && sizeof(dabx_chunk_data) == 128 && offsetof(dabx_chunk_data, groups) == 40,
              "include/dabx.h: chunk record layout");
static constexpr int DL_SF_CAP = (4 * DL_FRAMES + 4) / 5;          // super frames one chunk can complete (4 CIFs may be waiting from before)
#if DABX_MSC_BATCH == 7
static_assert(DL_FRAMES == DABX_CHUNK_FRAMES, "include/dabx.h: DABX_CHUNK_FRAMES is the library's MSC batch");
#endif
// the record sections (engine.h, Delivery::rec): a row of a section's table (pipeline.h: the four are one layout); the gather copies 16-byte words
static constexpr size_t rec_row_bytes = sizeof(dabx_chunk_scope);
static_assert(rec_row_bytes % 16 == 0 && DABX_TII_EVENT_SLOT_BYTES % 16 == 0 && SCOPE_SLOT_BYTES % 16 == 0 && CIR_SLOT_BYTES % 16 == 0 && SPEC_SLOT_BYTES % 16 == 0 &&
              FIG_SLOT_BYTES % 16 == 0 && sizeof(dabx_chunk_fig) == sizeof(dabx_chunk_scope) && offsetof(FigState, cnt) % 8 == 0,
              "a record section's slots are 16-aligned");

// What a record section gathers from (RecDeliverDev::ring, ::total, ::stride): all null / 0 while the engine has no such stage
struct RecSource { const uint8_t *ring; const long long *total; int32_t stride; };
static RecSource rec_source(const dabx_engine *e, int section)
{
  switch (section) {
  case REC_TII: if (e->tiis.exists()) return {e->tiis.dev.ring, &e->tiis.dev.cnt->events, (int32_t)(sizeof(TiiCounters) / sizeof(long long))}; break;
  case REC_SCOPE: if (e->scope.exists()) return {e->scope.dev.ring, &e->scope.dev.st->shows, (int32_t)(sizeof(ScopeState) / sizeof(long long))}; break;
  case REC_CIR: if (e->cir.exists()) return {e->cir.dev.ring, &e->cir.dev.st->shows, (int32_t)(sizeof(CirState) / sizeof(long long))}; break;
  case REC_SPECTRUM: if (e->spectrum.exists()) return {e->spectrum.dev.ring, &e->spectrum.dev.st->shows, (int32_t)(sizeof(SpecState) / sizeof(long long))}; break;
  case REC_FIG:
    if (e->fig.exists())
      return {reinterpret_cast<const uint8_t *>(e->fig.dev.ring), reinterpret_cast<const long long *>(&e->fig.dev.st->cnt.events), (int32_t)(sizeof(FigState) / sizeof(long long))};
    break;
  }
  return {nullptr, nullptr, 0};
}
// ... and whether stream s gets room in the section: it has the stage's mode on (a TII event is small: every stream has room)
static bool rec_stream_on(const dabx_engine *e, int section, size_t s)
{
  switch (section) {
  case REC_SCOPE: return e->scope.exists() && e->scope.cfg[s].enable;
  case REC_CIR: return e->cir.exists() && e->cir.cfg[s].enable;
  case REC_SPECTRUM: return e->spectrum.exists() && e->spectrum.cfg[s].enable;
  case REC_FIG: return e->fig.on_for((int)s);
  }
  return true;
}

// One section of the slab's head part for the slots of a job table: its table of S * M records at *off_table, then every slot's records and
// bytes, as much as one batch can emit (the caps of its ring).  Without such a slot, or unwanted: no section, the slots' offsets stay 0.
template <class Tab> static size_t layout_section(Tab &tab, bool want, size_t off, size_t table_bytes, uint64_t *off_table)
{
  bool any = false;
  for (auto &q : tab.host) { q.st.out.dl_rec_off = q.st.out.dl_bytes_off = 0; any = any || q.on; }
  if (!want || !any) return off;
  off = align_up(off, 16);
  if (!*off_table) { *off_table = off; off += table_bytes; }      // (the carousel slots share the MOT section's table)
  for (auto &q : tab.host) {
    if (!q.on) continue;
    auto &r = q.st.out;
    r.dl_rec_off = off; off += (size_t)r.dl_rec_cap * sizeof(*r.recs);
    r.dl_bytes_off = off; off = align_up(off + r.dl_bytes_cap, 16);
  }
  return off;
}
// ... and for dabx_delivery_open: the room that section needs for the slots there are now (one that is switched on later has to fit the
// slack); delivery starts with what they emit from now on
template <class Tab> static size_t section_capacity(Tab &tab, size_t table_bytes)
{
  size_t cap = tab.host.empty() ? 0 : table_bytes + 16;
  for (auto &q : tab.host)
    if (q.on) { q.st.out.dl_done = q.st.out.count; cap += (size_t)q.st.out.dl_rec_cap * sizeof(*q.st.out.recs) + q.st.out.dl_bytes_cap + 16; }
  return cap;
}

// Where every slot's bytes lie in a slab with the sub-channels configured now: table part (header, stream and slot records, FIBs,
// CRC flags, frame records), then the logical frames of all slots, then the super frames of all slots.  Uploaded to the device;
// called with the engine drained (dabx_delivery_open, dabx_set_subchannels*).
int dabx_engine::delivery_layout()
{
  Delivery &D = dl;
  const EngineDev &d = dev;
  const size_t S = (size_t)d.n_streams, M = (size_t)d.max_subch, F = DL_FRAMES;
  dabx_chunk_header h{};
  h.magic = DABX_CHUNK_MAGIC; h.abi = DABX_ABI_VERSION;
  h.n_streams = d.n_streams; h.max_subch = d.max_subch; h.max_frames = DL_FRAMES; h.what = D.what;
  size_t off = sizeof(dabx_chunk_header);
  dabx_chunk_header_ext x{};
  if (D.what & ~255) { x.magic = DABX_CHUNK_EXT_MAGIC; x.bytes = sizeof(x); off += sizeof(x); }     // a bit the header has no word for: its extension follows it
  dabx_chunk_header_ext2 x2{};
  if (D.data()) { x2.magic = DABX_CHUNK_EXT2_MAGIC; x2.bytes = sizeof(x2); off += sizeof(x2); }     // the first extension is full: a second one behind it, at byte 192
  h.off_stream = off; off = align_up(off + S * sizeof(dabx_chunk_stream), 16);
  h.off_subch = off; off = align_up(off + S * M * sizeof(dabx_chunk_subch), 16);
  const bool fib = (D.what & DABX_DELIVER_FIB) != 0;
  h.off_fib = off; if (fib) off = align_up(off + S * F * 384, 16);
  h.off_crc = off; if (fib) off = align_up(off + S * F * 12, 16);
  h.off_frame = off; if (fib) off = align_up(off + S * F * sizeof(dabx_chunk_frame), 16);
  std::vector<unsigned long long> lo(3 * S * M + 3, 0);
  // (super frames in front of the logical frames since round 6: the logical frames are the slab's TAIL, [off_msc, bytes), and travel first --
  //  behind the Viterbi decode, next to the DAB+ stage; the offsets in the records are what a host goes by)
  h.off_sf = off;
  if ((D.what & DABX_DELIVER_SF) && !d.fic_only)
    for (size_t sj = 0; sj < S * M; sj++) {
      const SubchDev &sc = subch_host[sj];
      if (!sc.active || !sc.dab_plus) continue;
      lo[3 * sj + 1] = off;
      off = align_up(off + (size_t)DL_SF_CAP * (size_t)((110 * (sc.kbps / 8) + 3) & ~3), 16);
      lo[3 * sj + 2] = off;
      off += (size_t)DL_SF_CAP * sizeof(dabx_superframe_info);
    }
  // the data-group section (dabx_chunk_dg) and behind it the PAD section (dabx_chunk_pad): only with such slots -- without one the slab is
  // what it has always been.  Callers hold fresh mirrors of the job tables (download with the engine drained); they go back to the device below
  off = layout_section(pkt, D.want_dg && !d.fic_only, off, S * M * sizeof(dabx_chunk_dg), &h.off_dg);
  if (h.off_dg) h.what |= DABX_DELIVER_DG;
  off = layout_section(pad, D.want_pad && !d.fic_only, off, S * M * sizeof(dabx_chunk_pad), &h.off_pad);
  if (h.off_pad) h.what |= DABX_DELIVER_PAD;
  off = layout_section(mot, D.want_mot && !d.fic_only, off, S * M * sizeof(dabx_chunk_mot), &h.off_mot);     // ... and behind that the MOT section (dabx_chunk_mot)
  off = layout_section(car, D.want_mot && !d.fic_only, off, S * M * sizeof(dabx_chunk_mot), &h.off_mot);     // ... with the rooms of the carousel slots
  if (h.off_mot) h.what |= DABX_DELIVER_MOT;
  if (D.eti()) { off = align_up(off, 16); h.off_eti = off; off += S * sizeof(dabx_chunk_eti); }     // the ETI section's table (its rows: the slab's end)
  // a record section: its table, then chunk_records slots for every stream that has room (all 16-aligned: the static_assert at rec_row_bytes)
  auto layout_records = [&](Delivery::RecSection &r) -> int {
    if (!(D.what & r.bit)) return 0;
    off = align_up(off, 16); x.*r.off_word = off; off += S * rec_row_bytes;
    std::vector<unsigned long long> so(S, 0);
    for (size_t s_ = 0; s_ < S; s_++)
      if (r.room[s_]) { so[s_] = off; off += (size_t)r.chunk_records * r.slot_bytes; }
    DABX_HIP(hipMemcpy(r.off, so.data(), sizeof(unsigned long long) * S, hipMemcpyHostToDevice));
    return 0;
  };
  if (int rc = layout_records(D.rec[REC_TII])) return rc;
  // the MP2 audio section (dabx_chunk_mp2_audio): with the bit and a slot that has the mode on
  off = layout_section(mpa, D.mp2_audio() && !d.fic_only, off, S * M * sizeof(dabx_chunk_mp2_audio), &x.off_mp2_audio);
  // ... and the AAC section (dabx_chunk_aac), in the same way
  off = layout_section(aac, D.aac() && !d.fic_only, off, S * M * sizeof(dabx_chunk_aac), &x.off_aac);
  // ... and the data section (dabx_chunk_data), announced by the second extension
  off = layout_section(dat, D.data() && !d.fic_only, off, S * M * sizeof(dabx_chunk_data), &x2.off_data);
  for (int i = REC_SCOPE; i < N_REC_SECTIONS; i++) if (int rc = layout_records(D.rec[i])) return rc;
  off = align_up(off, 256);
  h.off_msc = off;
  if ((D.what & (DABX_DELIVER_MSC | DABX_DELIVER_MSC_NOT_DABPLUS)) && !d.fic_only)
    for (size_t sj = 0; sj < S * M; sj++) {
      const SubchDev &sc = subch_host[sj];
      if (!sc.active || (!(D.what & DABX_DELIVER_MSC) && sc.dab_plus)) continue;
      lo[3 * sj] = off;
      off = align_up(off + (size_t)4 * F * 3 * sc.kbps, 16);
    }
  D.eti_rows_off = 0;
  if (D.eti()) { off = align_up(off, 256); D.eti_rows_off = off; off += S * 4 * F * DABX_ETI_FRAME_BYTES; }     // part of the tail: gathered with the logical frames
  h.bytes = off;
  if (off > D.capacity) {
    set_error("delivery: the configured sub-channels need %zu bytes per chunk, the slabs hold %zu (sub-channels of a stream that together "
              "exceed a CIF's capacity?)", off, D.capacity);
    return DABX_E_NOMEM;
  }
  D.hdr = h;
  D.ext = x;
  D.ext2 = x2;
  dat_ctl.off_data = x2.off_data;
  D.bytes = off;
  if (!pkt.host.empty()) if (int rc = pkt.upload()) return rc;
  if (!pad.host.empty()) if (int rc = pad.upload()) return rc;
  if (!mot.host.empty()) if (int rc = mot.upload()) return rc;
  if (!car.host.empty()) if (int rc = car.upload()) return rc;
  if (!mpa.host.empty()) if (int rc = mpa.upload()) return rc;
  if (!aac.host.empty()) if (int rc = aac.upload()) return rc;
  if (!dat.host.empty()) if (int rc = dat.upload()) return rc;
  if (S * M) {
    DABX_HIP(hipMemcpy(D.layout_off, lo.data(), sizeof(unsigned long long) * 3 * S * M, hipMemcpyHostToDevice));
    std::vector<int32_t> ids(subch_id_host.begin(), subch_id_host.begin() + S * M);
    DABX_HIP(hipMemcpy(D.subch_id, ids.data(), sizeof(int32_t) * S * M, hipMemcpyHostToDevice));
  }
  return 0;
}

// A chunk closes (dabx_process, before the MSC batch of its frames is launched): take a free host slab and the next device slab, and
// gather the front end's results of the chunk's frames on the front-end stream.
int dabx_engine::delivery_begin(DeliverDev *dv, int *slot, int *devslab)
{
  Delivery &D = dl;
  int h = -1;
  uint64_t seq;
  {
    std::unique_lock<std::mutex> lk(D.mu);
    if (!D.copier_error.empty()) { set_error("delivery: %s", D.copier_error.c_str()); return DABX_E_HIP; }
    for (size_t i = 0; i < D.slots.size() && h < 0; i++) if (D.slots[i].state == Delivery::FREE) h = (int)i;
    if (h < 0) { set_error("delivery: no free host slab (dabx_delivery_release)"); return DABX_E_STATE; }
    seq = D.next_seq++;
    const int k = (int)(seq % Delivery::NDEV);
    // the copy of chunk seq - NDEV has left the device slab (long ago, unless the link is the bottleneck: then the receiver waits here)
    // (bounded: a device slab that never comes back -- a copier that died -- must fail the call, not hang it)
    if (!D.cv.wait_for(lk, std::chrono::seconds(30), [&]() { return !D.dev_busy[k] || !D.copier_error.empty(); })) {
      D.next_seq--;
      set_error("delivery: device slab %d still busy after 30 s (chunk %llu)", k, (unsigned long long)seq);
      return DABX_E_STATE;
    }
    if (!D.copier_error.empty()) { D.next_seq--; set_error("delivery: %s", D.copier_error.c_str()); return DABX_E_HIP; }
    D.dev_busy[k] = true;
    D.slots[(size_t)h].state = Delivery::IN_FLIGHT;
    D.slots[(size_t)h].seq = seq;
    D.slots[(size_t)h].devslab = k;
    *devslab = k;
  }
  dv->slab = D.dev[*devslab]; dv->layout_off = D.layout_off; dv->subch_id = D.subch_id;
  dv->frames_done = D.frames_done; dv->cif_done = D.cif_done; dv->sf_done = D.sf_done;
  dv->hdr = D.hdr; dv->hdr.seq = seq;
  dv->off_mp2_audio = D.ext.off_mp2_audio;
  dv->off_aac = D.ext.off_aac;
  // two transfers when the slab has a tail of logical frames worth a transfer of its own (SDMA path)
  const size_t lf_from = (size_t)D.hdr.off_msc;
  const bool split = D.copy_engine == 0 && D.bytes > lf_from && D.bytes - lf_from >= ((size_t)1 << 20) && !dev.fic_only && dev.max_subch > 0 && dev.msc_out;
  dv->lf_done = split ? D.packed_lf[*devslab] : nullptr;
  {
    std::lock_guard<std::mutex> lk(D.mu);
    D.slots[(size_t)h].lf_from = split ? lf_from : 0;
  }
  *slot = h;
  int rc = launch_deliver_front(dev, *dv, stream);
  // the ETI stage's front half: the FIB ring is the front end's, which rewrites it while the chunk's MSC batch is decoded
  if (!rc && D.eti()) rc = launch_eti_front(dev, D.eti_dev(*devslab), stream, mk);
  if (!rc && D.ext.magic && !D.tii()) rc = launch_deliver_ext(D.ext, D.dev[*devslab], stream);
  if (!rc && D.ext2.magic) rc = launch_deliver_ext2(D.ext2, D.dev[*devslab], stream);      // (k_deliver_tii writes the header's extension otherwise)
  // the record sections: behind the stages' kernels of the chunk's last frame, which the front-end stream has run by now
  for (int i = 0; i < N_REC_SECTIONS && !rc; i++) {
    const Delivery::RecSection &r = D.rec[i];
    if (!(D.what & r.bit)) continue;
    const RecSource src = rec_source(this, i);
    rc = launch_deliver_records(i, dev.n_streams, RecDeliverDev{D.dev[*devslab], D.ext.*r.off_word, r.off, r.done, src.ring, src.total, src.stride, 0}, D.ext, stream);
  }
  if (rc) {                                                        // nothing was queued: give the slabs back
    std::lock_guard<std::mutex> lk(D.mu);
    D.dev_busy[*devslab] = false;
    D.slots[(size_t)h].state = Delivery::FREE;
    D.next_seq--;
    D.cv.notify_all();
  }
  return rc;
}

// A chunk that was begun cannot be finished (a launch of its MSC batch failed, or the event below): the host slab and the device slab go
// back, so that neither is lost and no later chunk waits for a copy nobody will make.  The chunk number is given back too (nothing was queued
// for the consumer); what the front gather already wrote into the device slab is overwritten by the next chunk that takes it.  The delivery
// is marked failed: every later call reports why.
void dabx_engine::delivery_abort(int slot, int devslab)
{
  Delivery &D = dl;
  std::lock_guard<std::mutex> lk(D.mu);
  D.slots[(size_t)slot].state = Delivery::FREE;
  D.dev_busy[devslab] = false;
  if (D.next_seq > 0) D.next_seq--;
  if (D.copier_error.empty()) D.copier_error = "a chunk was abandoned after a failed launch: " + std::string(dabx::last_error());
  D.cv.notify_all();
}

// ... and once its slot gather is queued behind the DAB+ stage on `tail`: the copier takes over.
int dabx_engine::delivery_finish(int slot, int devslab, hipStream_t tail)
{
  Delivery &D = dl;
  {
    const hipError_t he = hipEventRecord(D.packed[devslab], tail);
    if (he != hipSuccess) {
      set_error("HIP error %d (%s) at %s:%d", (int)he, hipGetErrorString(he), __FILE__, __LINE__);
      delivery_abort(slot, devslab);
      return DABX_E_HIP;
    }
  }
  std::lock_guard<std::mutex> lk(D.mu);
  D.slots[(size_t)slot].bytes = D.bytes;
  D.queue.push_back(slot);
  D.jobs.push_back(slot);
  D.cv.notify_all();
  return 0;
}

// The copier: one chunk at a time, in order -- wait for the gather kernels, ONE transfer of
// the slab, wait for it, hand the slab to the consumer.
static void delivery_copier(Delivery *Dp)
{
  Delivery &D = *Dp;
  (void)hipSetDevice(D.device);
  for (;;) {
    int h;
    {
      std::unique_lock<std::mutex> lk(D.mu);
      D.cv.wait(lk, [&]() { return D.quit || !D.jobs.empty(); });
      if (D.jobs.empty()) return;                // quit, nothing left to copy
      h = D.jobs.front();
    }
    Delivery::Slot &sl = D.slots[(size_t)h];
    std::string err;
    const auto t_a = std::chrono::steady_clock::now();
    // polled every 50 us, not hipEventSynchronize: see sdma_wait
    hipError_t he;
    // first the slab's tail -- the logical frames, gathered behind the Viterbi decode: on the link while the DAB+ stage and the second gather run
    size_t head_bytes = sl.bytes;
    bool lf_started = false;
    auto t_lf = t_a;
    if (sl.lf_from) {
      while ((he = hipEventQuery(D.packed_lf[sl.devslab])) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(50));
      if (he != hipSuccess) err = std::string("hipEventQuery: ") + hipGetErrorString(he);
      else if (sdma_copy(D.sdma, sl.host + sl.lf_from, D.dev[sl.devslab] + sl.lf_from, sl.bytes - sl.lf_from, true, sl.sig2)) err = dabx::last_error();
      else { lf_started = true; head_bytes = sl.lf_from; t_lf = std::chrono::steady_clock::now(); }
    }
    while ((he = hipEventQuery(D.packed[sl.devslab])) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(50));
    if (he != hipSuccess && err.empty()) err = std::string("hipEventQuery: ") + hipGetErrorString(he);
    const auto t_b = std::chrono::steady_clock::now();
    if (err.empty()) {
      if (D.copy_engine == 0) {
        if (sdma_copy(D.sdma, sl.host, D.dev[sl.devslab], head_bytes, true, sl.sig) || sdma_wait(sl.sig, head_bytes)) err = dabx::last_error();
        if (lf_started && sdma_wait(sl.sig2, 0) && err.empty()) err = dabx::last_error();
      } else {
        he = hipMemcpyAsync(sl.host, D.dev[sl.devslab], sl.bytes, hipMemcpyDeviceToHost, D.cs);
        if (he == hipSuccess) he = hipStreamSynchronize(D.cs);
        if (he != hipSuccess) err = std::string("hipMemcpyAsync: ") + hipGetErrorString(he);
      }
    }
    const auto t_c = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(D.mu);
    {
      // (two-part transfers: from the start of the first part to the end of the second, the wait for the second gather in between included --
      //  the link rate derived from it is a lower bound)
      const double cs_ = std::chrono::duration<double>(t_c - (lf_started ? t_lf : t_b)).count();
      D.gather_wait_s += std::chrono::duration<double>((lf_started ? t_lf : t_b) - t_a).count();
      D.copy_s += cs_; D.copy_s_max = std::max(D.copy_s_max, cs_);
      D.landed++; D.bytes_copied += sl.bytes;
    }
    D.jobs.pop_front();
    D.dev_busy[sl.devslab] = false;
    sl.state = Delivery::LANDED;                 // (after an error too: nobody may wait for ever; the error is reported by the next call)
    if (!err.empty() && D.copier_error.empty()) D.copier_error = err;
    D.cv.notify_all();
  }
}

namespace dabx {

// every chunk closed so far has landed in its host slab (dabx_synchronize and everything that drains the engine)
int delivery_drain(dabx_engine *e)
{
  Delivery &D = e->dl;
  if (!D.open) return 0;
  std::unique_lock<std::mutex> lk(D.mu);
  D.cv.wait(lk, [&]() { return D.jobs.empty(); });
  if (!D.copier_error.empty()) { set_error("delivery: %s", D.copier_error.c_str()); return DABX_E_HIP; }
  return 0;
}

void delivery_free(dabx_engine *e)
{
  Delivery &D = e->dl;
  if (D.copier.joinable()) {
    { std::lock_guard<std::mutex> lk(D.mu); D.quit = true; D.cv.notify_all(); }
    D.copier.join();
  }
  D.quit = false;
  if (D.cs) (void)hipStreamSynchronize(D.cs);
  for (auto &sl : D.slots) { if (sl.host) (void)hipHostFree(sl.host); sdma_signal_destroy(sl.sig); sdma_signal_destroy(sl.sig2); }
  D.slots.clear();
  D.queue.clear();
  D.jobs.clear();
  for (int k = 0; k < Delivery::NDEV; k++) {
    if (D.dev[k]) (void)hipFree(D.dev[k]);
    if (D.packed[k]) (void)hipEventDestroy(D.packed[k]);
    if (D.packed_lf[k]) (void)hipEventDestroy(D.packed_lf[k]);
    D.dev[k] = nullptr; D.packed[k] = nullptr; D.packed_lf[k] = nullptr; D.dev_busy[k] = false;
  }
  hip_free_all({D.layout_off, D.subch_id, D.frames_done, D.cif_done, D.sf_done, D.eti_front, D.eti_next, D.eti_stage[0], D.eti_stage[1], D.eti_stage[2]});
  for (Delivery::RecSection &r : D.rec) { hip_free_all({r.done, r.off}); r.done = nullptr; r.off = nullptr; r.room.clear(); }
  D.ext = dabx_chunk_header_ext{};
  D.ext2 = dabx_chunk_header_ext2{};
  e->dat_ctl.off_data = 0;
  D.layout_off = nullptr; D.subch_id = nullptr; D.frames_done = D.cif_done = D.sf_done = nullptr;
  D.eti_front = nullptr; D.eti_next = nullptr; D.eti_rows_off = 0;
  for (int k = 0; k < Delivery::NDEV; k++) D.eti_stage[k] = nullptr;
  if (D.cs) (void)hipStreamDestroy(D.cs);
  D.cs = nullptr;
  D.copier_error.clear();
  D.open = false; D.capacity = D.bytes = 0; D.next_seq = 0;
  D.landed = D.bytes_copied = 0; D.copy_s = D.copy_s_max = D.gather_wait_s = 0;
}

}  // namespace dabx

extern "C" {

int dabx_delivery_open(dabx_engine *e, const dabx_delivery_config *cfg)
{
  if (!e || (cfg && (cfg->host_slabs < 0 || cfg->host_slabs == 1 || cfg->host_slabs > 64 || (cfg->what & ~(1023 | DABX_DELIVER_AAC | DABX_DELIVER_SCOPE | DABX_DELIVER_CIR | DABX_DELIVER_SPECTRUM | DABX_DELIVER_FIG | DABX_DELIVER_DATA)) || cfg->copy_engine < 0 || cfg->copy_engine > 1))) {
    set_error("dabx_delivery_open: bad argument");
    return DABX_E_ARG;
  }
  // DABX_DELIVER_TII adds its section to a delivery of something else.  Alone it names nothing a chunk is made of: the mask 256 stays the
  // bad argument it was before the bit existed (a host that probes for bits it does not know sees no change)
  if (cfg && cfg->what == DABX_DELIVER_TII) {
    set_error("dabx_delivery_open: DABX_DELIVER_TII needs at least one other DABX_DELIVER_* bit beside it");
    return DABX_E_ARG;
  }
  // ... and so does DABX_DELIVER_MP2_AUDIO, alone or with DABX_DELIVER_TII: neither names anything a chunk is made of
  if (cfg && (cfg->what & DABX_DELIVER_MP2_AUDIO) && !(cfg->what & ~(DABX_DELIVER_MP2_AUDIO | DABX_DELIVER_TII))) {
    set_error("dabx_delivery_open: DABX_DELIVER_MP2_AUDIO needs at least one DABX_DELIVER_* bit below 256 beside it");
    return DABX_E_ARG;
  }
  // ... and DABX_DELIVER_AAC, alone or with only those two
  if (cfg && (cfg->what & DABX_DELIVER_AAC) && !(cfg->what & ~(DABX_DELIVER_AAC | DABX_DELIVER_MP2_AUDIO | DABX_DELIVER_TII))) {
    set_error("dabx_delivery_open: DABX_DELIVER_AAC needs at least one DABX_DELIVER_* bit below 256 beside it");
    return DABX_E_ARG;
  }
  // ... and DABX_DELIVER_SCOPE, alone or with only the other opt-in bits
  if (cfg && (cfg->what & DABX_DELIVER_SCOPE) &&
      !(cfg->what & ~(DABX_DELIVER_SCOPE | DABX_DELIVER_AAC | DABX_DELIVER_MP2_AUDIO | DABX_DELIVER_TII | DABX_DELIVER_ETI))) {
    set_error("dabx_delivery_open: DABX_DELIVER_SCOPE needs at least one DABX_DELIVER_* bit below 128 beside it");
    return DABX_E_ARG;
  }
  // ... and DABX_DELIVER_CIR, in the same way
  if (cfg && (cfg->what & DABX_DELIVER_CIR) &&
      !(cfg->what & ~(DABX_DELIVER_FIG | DABX_DELIVER_SPECTRUM | DABX_DELIVER_CIR | DABX_DELIVER_SCOPE | DABX_DELIVER_AAC | DABX_DELIVER_MP2_AUDIO | DABX_DELIVER_TII | DABX_DELIVER_ETI))) {
    set_error("dabx_delivery_open: DABX_DELIVER_CIR needs at least one DABX_DELIVER_* bit below 128 beside it");
    return DABX_E_ARG;
  }
  // ... and DABX_DELIVER_SPECTRUM, in the same way
  if (cfg && (cfg->what & DABX_DELIVER_SPECTRUM) &&
      !(cfg->what & ~(DABX_DELIVER_FIG | DABX_DELIVER_SPECTRUM | DABX_DELIVER_CIR | DABX_DELIVER_SCOPE | DABX_DELIVER_AAC | DABX_DELIVER_MP2_AUDIO | DABX_DELIVER_TII | DABX_DELIVER_ETI))) {
    set_error("dabx_delivery_open: DABX_DELIVER_SPECTRUM needs at least one DABX_DELIVER_* bit below 128 beside it");
    return DABX_E_ARG;
  }
  // ... and DABX_DELIVER_FIG, in the same way
  if (cfg && (cfg->what & DABX_DELIVER_FIG) &&
      !(cfg->what & ~(DABX_DELIVER_FIG | DABX_DELIVER_SPECTRUM | DABX_DELIVER_CIR | DABX_DELIVER_SCOPE | DABX_DELIVER_AAC | DABX_DELIVER_MP2_AUDIO | DABX_DELIVER_TII | DABX_DELIVER_ETI))) {
    set_error("dabx_delivery_open: DABX_DELIVER_FIG needs at least one DABX_DELIVER_* bit below 128 beside it");
    return DABX_E_ARG;
  }
  // ... and DABX_DELIVER_DATA, in the same way
  if (cfg && (cfg->what & DABX_DELIVER_DATA) &&
      !(cfg->what & ~(DABX_DELIVER_DATA | DABX_DELIVER_FIG | DABX_DELIVER_SPECTRUM | DABX_DELIVER_CIR | DABX_DELIVER_SCOPE | DABX_DELIVER_AAC | DABX_DELIVER_MP2_AUDIO |
                      DABX_DELIVER_TII | DABX_DELIVER_ETI))) {
    set_error("dabx_delivery_open: DABX_DELIVER_DATA needs at least one DABX_DELIVER_* bit below 128 beside it");
    return DABX_E_ARG;
  }
  if (e->dl.open) { set_error("dabx_delivery_open: already open"); return DABX_E_STATE; }
  int rc = sync_all(e);
  if (rc) return rc;
  Delivery &D = e->dl;
  const EngineDev &d = e->dev;
  D.want_dg = !cfg || !cfg->what || (cfg->what & DABX_DELIVER_DG);
  D.want_pad = !cfg || !cfg->what || (cfg->what & DABX_DELIVER_PAD);
  D.want_mot = !cfg || !cfg->what || (cfg->what & DABX_DELIVER_MOT);
  D.what = cfg && cfg->what ? (cfg->what & ~(DABX_DELIVER_DG | DABX_DELIVER_PAD | DABX_DELIVER_MOT)) : (DABX_DELIVER_FIB | DABX_DELIVER_MSC | DABX_DELIVER_SF);
  if ((D.what & DABX_DELIVER_FIB) && d.out_frames < DL_FRAMES) {
    set_error("dabx_delivery_open: the engine's FIB ring holds %d frames, a chunk up to %d: create it with dabx_config.out_frames >= %d "
              "(the FIBs of a chunk's first frames would have left the ring before they are gathered)", d.out_frames, DL_FRAMES, DL_FRAMES);
    return DABX_E_STATE;
  }
  if (D.eti() && (d.fic_only || d.out_frames < DL_FRAMES)) {       // the ETI stage reads the chunk's FIBs at chunk close, like the FIB gather
    if (d.fic_only) set_error("dabx_delivery_open: DABX_DELIVER_ETI on an engine that was created FIC-only");
    else set_error("dabx_delivery_open: DABX_DELIVER_ETI needs dabx_config.out_frames >= %d, the engine's FIB ring holds %d frames", DL_FRAMES, d.out_frames);
    return DABX_E_STATE;
  }
  D.copy_engine = cfg ? cfg->copy_engine : 0;
  D.device = e->device;
  if (D.copy_engine == 0 && (rc = sdma_open(e->device, &D.sdma))) return rc;
  const int n_slots = cfg && cfg->host_slabs ? cfg->host_slabs : 4;
  const size_t S = (size_t)d.n_streams, M = (size_t)d.max_subch, F = DL_FRAMES;
  // capacity: the tables + per stream what a full CIF can carry at the highest code rate of the standard (EEP 4-B, 4/5: 5530 B
  // of logical frames per CIF) for 4 F CIFs, and the same again for the super frames of up to DL_SF_CAP x 5 CIFs
  const size_t per_cif = 5632;
  size_t cap = sizeof(dabx_chunk_header) + S * sizeof(dabx_chunk_stream) + S * M * sizeof(dabx_chunk_subch) + S * F * (384 + 12 + sizeof(dabx_chunk_frame)) + 6 * 16 + 256;
  if (M && !d.fic_only) cap += S * ((size_t)4 * F * per_cif + (size_t)DL_SF_CAP * 5 * per_cif + 2 * 16 * M + M * DL_SF_CAP * sizeof(dabx_superframe_info));
  // ... and the data-group, the PAD and the MOT section
  if ((rc = e->pkt.download(d.max_subch)) || (rc = e->pad.download(d.max_subch)) || (rc = e->mot.download(d.max_subch)) ||
      (rc = e->car.download(d.max_subch)) || (rc = e->mpa.download(d.max_subch)) || (rc = e->aac.download(d.max_subch)) || (rc = e->dat.download(d.max_subch))) return rc;
  cap += section_capacity(e->pkt, S * M * sizeof(dabx_chunk_dg)) + section_capacity(e->pad, S * M * sizeof(dabx_chunk_pad)) +
         section_capacity(e->mot, S * M * sizeof(dabx_chunk_mot)) + section_capacity(e->car, S * M * sizeof(dabx_chunk_mot));
  if (D.eti()) cap += 16 + S * sizeof(dabx_chunk_eti) + 256 + S * 4 * F * DABX_ETI_FRAME_BYTES;      // ... and the ETI section: its table and 4 F rows per stream
  if (D.what & ~255) cap += sizeof(dabx_chunk_header_ext);          // ... and the header's extension, where delivery_layout puts one
  if (D.mp2_audio()) cap += section_capacity(e->mpa, S * M * sizeof(dabx_chunk_mp2_audio));   // ... and the MP2 audio section
  if (D.aac()) cap += section_capacity(e->aac, S * M * sizeof(dabx_chunk_aac));               // ... and the AAC section
  if (D.data()) cap += sizeof(dabx_chunk_header_ext2) + section_capacity(e->dat, S * M * sizeof(dabx_chunk_data));      // ... the second extension and the data section
  for (int i = 0; i < N_REC_SECTIONS; i++) {                        // ... and the record sections: a table and chunk_records slots per stream with room
    Delivery::RecSection &r = D.rec[i];
    const bool want = (D.what & r.bit) != 0;
    r.room.assign(want ? S : 0, 0);
    if (!want) continue;
    size_t n_room = 0;
    for (size_t s_ = 0; s_ < S; s_++) { r.room[s_] = (char)rec_stream_on(e, i, s_); n_room += r.room[s_] ? 1 : 0; }
    cap += 16 + S * rec_row_bytes + n_room * (size_t)r.chunk_records * r.slot_bytes;
  }
  D.capacity = align_up(cap, 4096);
#define H(x) do { hipError_t err__ = (x); if (err__ != hipSuccess) { set_error("HIP error %d (%s) at %s:%d", (int)err__, hipGetErrorString(err__), __FILE__, __LINE__); delivery_free(e); return DABX_E_HIP; } } while (0)
  if (D.copy_engine == 1) H(hipStreamCreateWithFlags(&D.cs, hipStreamNonBlocking));
  for (int k = 0; k < Delivery::NDEV; k++) {
    H(hipMalloc((void **)&D.dev[k], D.capacity));
    H(hipMemset(D.dev[k], 0, D.capacity));
    // system-scope release, explicitly: the SDMA engine (raw HSA, outside HIP's own fences) and the host read what the gather kernels wrote
    H(hipEventCreateWithFlags(&D.packed[k], hipEventDisableTiming | hipEventReleaseToSystem));
    H(hipEventCreateWithFlags(&D.packed_lf[k], hipEventDisableTiming | hipEventReleaseToSystem));
  }
  D.slots.resize((size_t)n_slots);
  for (auto &sl : D.slots) {
    H(hipHostMalloc((void **)&sl.host, D.capacity, hipHostMallocDefault));
    if (D.copy_engine == 0 && ((rc = sdma_signal_create(&sl.sig)) || (rc = sdma_signal_create(&sl.sig2)))) { delivery_free(e); return rc; }
  }
  H(hipMalloc((void **)&D.layout_off, sizeof(unsigned long long) * std::max<size_t>(3 * S * M, 3)));
  H(hipMalloc((void **)&D.subch_id, sizeof(int32_t) * std::max<size_t>(S * M, 1)));
  H(hipMalloc((void **)&D.frames_done, sizeof(long long) * S));
  H(hipMalloc((void **)&D.cif_done, sizeof(long long) * std::max<size_t>(S * M, 1)));
  H(hipMalloc((void **)&D.sf_done, sizeof(long long) * std::max<size_t>(S * M, 1)));
  // delivery starts with what is decoded from now on
  {
    std::vector<StreamCtl> ctl(S);
    H(hipMemcpy(ctl.data(), d.ctl, sizeof(StreamCtl) * S, hipMemcpyDeviceToHost));
    std::vector<long long> fr(S), cd(std::max<size_t>(S * M, 1), 0), sd(std::max<size_t>(S * M, 1), 0);
    for (size_t s_ = 0; s_ < S; s_++) fr[s_] = ctl[s_].frames;
    if (S * M) {
      H(hipMemcpy(e->subch_host.data(), d.subch, sizeof(SubchDev) * S * M, hipMemcpyDeviceToHost));
      for (size_t sj = 0; sj < S * M; sj++) { cd[sj] = e->subch_host[sj].cif_out; sd[sj] = e->subch_host[sj].sf_count; }
    }
    H(hipMemcpy(D.frames_done, fr.data(), sizeof(long long) * S, hipMemcpyHostToDevice));
    H(hipMemcpy(D.cif_done, cd.data(), sizeof(long long) * cd.size(), hipMemcpyHostToDevice));
    H(hipMemcpy(D.sf_done, sd.data(), sizeof(long long) * sd.size(), hipMemcpyHostToDevice));
    if (D.eti()) {
      // the ETI stage's cursor: the CIFs decoded from now on, the counter unknown until a delivered frame carries a FIG 0/0
      std::vector<EtiFront> ef(S);
      std::vector<long long> nc(S);
      for (size_t s_ = 0; s_ < S; s_++) { ef[s_] = EtiFront{ctl[s_].frames, -1, -1}; nc[s_] = ctl[s_].cif_no; }
      H(hipMalloc((void **)&D.eti_front, sizeof(EtiFront) * S));
      H(hipMalloc((void **)&D.eti_next, sizeof(long long) * S));
      H(hipMemcpy(D.eti_front, ef.data(), sizeof(EtiFront) * S, hipMemcpyHostToDevice));
      H(hipMemcpy(D.eti_next, nc.data(), sizeof(long long) * S, hipMemcpyHostToDevice));
      for (int k = 0; k < Delivery::NDEV; k++) {
        H(hipMalloc((void **)&D.eti_stage[k], sizeof(EtiStage) * S));
        H(hipMemset(D.eti_stage[k], 0, sizeof(EtiStage) * S));
      }
    }
    for (int i = 0; i < N_REC_SECTIONS; i++) {
      Delivery::RecSection &r = D.rec[i];
      if (!(D.what & r.bit)) continue;
      // the section's cursor: the records completed from now on (the counters lie src.stride long longs apart, from src.total on)
      const RecSource src = rec_source(e, i);
      std::vector<long long> cur(S, 0);
      if (src.total) {
        std::vector<long long> raw((S - 1) * (size_t)src.stride + 1);
        H(hipMemcpy(raw.data(), src.total, sizeof(long long) * raw.size(), hipMemcpyDeviceToHost));
        for (size_t s_ = 0; s_ < S; s_++) cur[s_] = raw[s_ * (size_t)src.stride];
      }
      H(hipMalloc((void **)&r.done, sizeof(long long) * S));
      H(hipMemcpy(r.done, cur.data(), sizeof(long long) * S, hipMemcpyHostToDevice));
      H(hipMalloc((void **)&r.off, sizeof(unsigned long long) * S));
    }
  }
#undef H
  if ((rc = e->delivery_layout())) { delivery_free(e); return rc; }
  // the engine the slabs will travel on must be one of the fast ones (sdma.h): checked with a 16-MiB transfer, replaced if it is not
  if (D.copy_engine == 0 && D.capacity >= ((size_t)16 << 20) && (rc = sdma_calibrate(D.sdma, D.slots[0].host, D.dev[0], true, D.slots[0].sig, &D.calib_gbps))) {
    delivery_free(e);
    return rc;
  }
  D.quit = false;
  D.copier = std::thread(delivery_copier, &D);
  D.open = true;
  return 0;
}

int dabx_delivery_close(dabx_engine *e)
{
  if (!e) return DABX_E_ARG;
  if (!e->dl.open) return 0;
  const int rc = sync_all(e);
  delivery_free(e);
  return rc;
}

long long dabx_delivery_slab_bytes(dabx_engine *e)
{
  if (!e) return DABX_E_ARG;
  if (!e->dl.open) { set_error("dabx_delivery_slab_bytes: no delivery open"); return DABX_E_STATE; }
  return (long long)e->dl.bytes;
}

// Consumer side (may run on a second thread): chunks in the order they were closed.
int dabx_delivery_next(dabx_engine *e, int wait, dabx_chunk *out)
{
  if (!e || !out) return DABX_E_ARG;
  Delivery &D = e->dl;
  if (!D.open) { set_error("dabx_delivery_next: no delivery open"); return DABX_E_STATE; }
  std::unique_lock<std::mutex> lk(D.mu);
  if (D.queue.empty()) return 0;
  Delivery::Slot &sl = D.slots[(size_t)D.queue.front()];      // only this thread pops: the front stays the front
  if (sl.state != Delivery::LANDED) {
    if (!wait) return 0;
    D.cv.wait(lk, [&]() { return sl.state == Delivery::LANDED; });
  }
  if (!D.copier_error.empty()) { set_error("delivery: %s", D.copier_error.c_str()); return DABX_E_HIP; }
  D.queue.pop_front();
  sl.state = Delivery::HELD;
  out->seq = sl.seq; out->data = sl.host; out->bytes = sl.bytes;
  return 1;
}

int dabx_delivery_release(dabx_engine *e, uint64_t seq)
{
  if (!e) return DABX_E_ARG;
  Delivery &D = e->dl;
  if (!D.open) { set_error("dabx_delivery_release: no delivery open"); return DABX_E_STATE; }
  std::lock_guard<std::mutex> lk(D.mu);
  for (auto &sl : D.slots)
    if (sl.state == Delivery::HELD && sl.seq == seq) { sl.state = Delivery::FREE; D.cv.notify_all(); return 0; }
  set_error("dabx_delivery_release: chunk %llu is not held", (unsigned long long)seq);
  return DABX_E_ARG;
}

int dabx_delivery_get_info(dabx_engine *e, dabx_delivery_info *out)
{
  if (!e || !out) return DABX_E_ARG;
  Delivery &D = e->dl;
  if (!D.open) { set_error("dabx_delivery_get_info: no delivery open"); return DABX_E_STATE; }
  std::lock_guard<std::mutex> lk(D.mu);
  memset(out, 0, sizeof(*out));
  out->chunks_closed = D.next_seq; out->chunks_landed = D.landed; out->bytes_copied = D.bytes_copied;
  out->copy_seconds = D.copy_s; out->copy_seconds_max = D.copy_s_max; out->gather_wait_seconds = D.gather_wait_s;
  out->copy_engine = D.copy_engine; out->sdma_engine_mask = D.copy_engine == 0 ? D.sdma.engine_to_host : 0;
  out->calibration_GBps = D.calib_gbps;
  return 0;
}

int dabx_delivery_wait_free(dabx_engine *e, int n, int timeout_ms)
{
  if (!e || n < 0) return DABX_E_ARG;
  Delivery &D = e->dl;
  if (!D.open) { set_error("dabx_delivery_wait_free: no delivery open"); return DABX_E_STATE; }
  if ((size_t)n > D.slots.size()) { set_error("dabx_delivery_wait_free: %d slabs asked for, the delivery has %zu", n, D.slots.size()); return DABX_E_ARG; }
  std::unique_lock<std::mutex> lk(D.mu);
  auto free_now = [&D]() { int k = 0; for (const auto &sl : D.slots) k += sl.state == Delivery::FREE; return k; };
  if (timeout_ms < 0) D.cv.wait(lk, [&]() { return free_now() >= n; });
  else D.cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), [&]() { return free_now() >= n; });
  return free_now();
}

}  // extern "C"
