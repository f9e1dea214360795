// engine.h -- internal: struct dabx_engine with its delivery, ingest and job-table parts, and what the engine*.cpp files share.
#pragma once
#include "pipeline.h"
#include "packet_core.h"
#include "pad_core.h"
#include "mot_core.h"
#include "carousel_core.h"
#include "data_core.h"
#include "mp2_core.h"
#include "aac_core.h"
#include "tii_core.h"
#include "scope_core.h"
#include "cir_core.h"
#include "spectrum_core.h"
#include "fig_core.h"
#include "rec_ring.h"
#include "sdma.h"
#include "iqfile.h"
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace dabx;                          // (a header of engine.cpp and the engine_*.cpp files only)

static constexpr int DL_FRAMES = MSC_BATCH_FRAMES;                 // a chunk = what one MSC batch decodes (the default slab of the bulk ingest too)

// Bulk delivery (include/dabx.h): host slabs (page-locked) the chunks land in, device slabs they are packed into, and the copier --
// a thread of the library that waits (polling every 50 us) for a chunk's gather kernels and then moves the slab with ONE SDMA
// transfer (sdma.h: the HIP runtime's own device-to-host copy is a shader copy that stalls the receiver's kernels while it runs).
struct Delivery {
  bool open = false;
  int what = 0;
  int copy_engine = 0;                           // dabx_delivery_config.copy_engine: 0 SDMA through the HSA runtime, 1 hipMemcpyAsync
  static constexpr int NDEV = 3;                 // device slabs: chunk n + 3 is packed into the slab of chunk n once its copy has left
  uint8_t *dev[NDEV] = {nullptr, nullptr, nullptr};
  hipEvent_t packed[NDEV] = {nullptr, nullptr, nullptr};    // the chunk's gather kernels have finished (system-scope release; the copier polls them)
  hipEvent_t packed_lf[NDEV] = {nullptr, nullptr, nullptr}; // ... its logical frames (the slab's tail, [off_msc, bytes)) are in the slab: that share of the
                                                            // transfer starts while the DAB+ stage still runs (round 6)
  bool dev_busy[NDEV] = {false, false, false};   // packed into or being copied from (guarded by mu)
  hipStream_t cs = nullptr;                      // copy_engine 1 only
  Sdma sdma;
  size_t capacity = 0, bytes = 0;                // bytes allocated per slab / bytes the current layout uses (= what is copied)
  enum { FREE = 0, IN_FLIGHT = 1, LANDED = 2, HELD = 3 };
  struct Slot { uint8_t *host = nullptr; uint64_t sig = 0, sig2 = 0; int state = FREE; uint64_t seq = 0; size_t bytes = 0, lf_from = 0; int devslab = 0; };
  std::vector<Slot> slots;
  std::deque<int> queue;                         // slots in flight or landed, oldest first (what dabx_delivery_next hands out)
  std::deque<int> jobs;                          // slots whose copy the copier still has to make
  std::mutex mu;                                 // everything above: the engine's thread, the copier and ONE consumer thread
  std::condition_variable cv;                    // any state change
  std::thread copier;
  bool quit = false;
  int device = 0;
  std::string copier_error;
  uint64_t next_seq = 0, landed = 0, bytes_copied = 0;
  double copy_s = 0, copy_s_max = 0, gather_wait_s = 0, calib_gbps = 0;
  unsigned long long *layout_off = nullptr;      // device tables (DeliverDev)
  int32_t *subch_id = nullptr;
  long long *frames_done = nullptr, *cif_done = nullptr, *sf_done = nullptr;
  dabx_chunk_header hdr{};
  bool want_pad = false;                         // DABX_DELIVER_PAD, or what == 0: a PAD section while there are PAD slots
  bool want_mot = false;                         // DABX_DELIVER_MOT, or what == 0: a MOT section while there are MOT or carousel slots
  bool want_dg = false;                          // DABX_DELIVER_DG, or what == 0: a data-group section while there are packet-mode slots
  // DABX_DELIVER_ETI (pipeline.h, EtiDev): the stage's cursor, one staging buffer per device slab, where the rows lie in a slab; all null / 0 without the bit
  EtiFront *eti_front = nullptr;
  long long *eti_next = nullptr;
  EtiStage *eti_stage[NDEV] = {nullptr, nullptr, nullptr};
  size_t eti_rows_off = 0;
  // The sections of fixed-size records (rec_ring.h; deliver.hip, k_deliver_tii and k_deliver_records), in the order they are gathered: a table of
  // one 32-byte row per stream at the extension's word, behind it chunk_records slots for every stream that has room.  done / off are null
  // and room is empty without the section's bit.
  struct RecSection {
    int bit;                                     // DABX_DELIVER_*
    int chunk_records, slot_bytes;               // the most a chunk delivers per stream
    uint64_t dabx_chunk_header_ext::*off_word;   // the word of the header's extension that announces the section
    long long *done = nullptr;                   // [S] device: records of the stream delivered or passed so far
    unsigned long long *off = nullptr;           // [S] device: where the stream's slots lie in a slab, 0 = it has no room
    std::vector<char> room;                      // [S] the stream had the mode on when the delivery was opened (TII: every stream)
  };
  RecSection rec[N_REC_SECTIONS] = {
    {DABX_DELIVER_TII, 4, DABX_TII_EVENT_SLOT_BYTES, &dabx_chunk_header_ext::off_tii},
    {DABX_DELIVER_SCOPE, DL_FRAMES, SCOPE_SLOT_BYTES, &dabx_chunk_header_ext::off_scope},
    {DABX_DELIVER_CIR, DABX_CIR_CHUNK_RECORDS, CIR_SLOT_BYTES, &dabx_chunk_header_ext::off_cir},
    {DABX_DELIVER_SPECTRUM, DABX_SPECTRUM_CHUNK_RECORDS, SPEC_SLOT_BYTES, &dabx_chunk_header_ext::off_spectrum},
    {DABX_DELIVER_FIG, DABX_FIG_CHUNK_RECORDS, FIG_SLOT_BYTES, &dabx_chunk_header_ext::off_fig}};
  dabx_chunk_header_ext ext{};                   // the header's extension as it goes into a slab; zeros without a bit >= 256
  bool tii() const { return (what & DABX_DELIVER_TII) != 0; }
  bool mp2_audio() const { return (what & DABX_DELIVER_MP2_AUDIO) != 0; }      // the MP2 audio section (deliver.hip, k_deliver_mp2_audio), while a slot has the mode on
  bool aac() const { return (what & DABX_DELIVER_AAC) != 0; }      // the AAC section (deliver.hip, k_deliver_aac), while a slot has the mode on
  bool eti() const { return (what & DABX_DELIVER_ETI) != 0; }
  bool data() const { return (what & DABX_DELIVER_DATA) != 0; }    // the data section (deliver.hip, k_deliver_data), while a slot has a handler on
  dabx_chunk_header_ext2 ext2{};                 // the second extension as it goes into a slab; zeros without DABX_DELIVER_DATA
  EtiDev eti_dev(int devslab) const
  {
    return EtiDev{eti_front, eti_next, eti_stage[devslab], dev[devslab], subch_id, hdr.off_eti, eti_rows_off, hdr.max_frames, 0};
  }
};

// Bulk ingest (include/dabx.h "Bulk ingest"): page-locked input slabs, their device twins, one SDMA transfer per slab.  Both forms are S
// jobs for iqfile.hip's table writer: dabx_ingest_open gives every stream the same decode and a dense slab, dabx_ingest_open_formats
// every stream its own container, rate, length and region.
struct Ingest {
  bool open = false;
  int copy_engine = 0, max_frames = 0;
  size_t capacity = 0;                           // bytes per slab
  struct Slab {
    uint8_t *host = nullptr, *dev = nullptr; uint64_t sig = 0; bool in_flight = false;
    size_t bytes = 0, pitch = 0;                 // what was submitted: bytes transferred, bytes from one stream's payload to the next
    std::vector<size_t> n_bytes;                 // [S] payload bytes per stream
    // the commit's table, [S] jobs and behind them [S] sample counts: page-locked staging / device.  One per slab: dabx_ingest_submit
    // drains the ingest stream, so by the slab's next commit the upload of this one has left the staging copy
    IqJob *jobs_host = nullptr, *jobs_dev = nullptr;      // (in Ingest::tables_host / tables_dev)
    hipEvent_t counts_read = nullptr;            // per-stream form: the commit kernel that reads the device table's counts has run (front-end stream)
  };
  std::vector<Slab> slabs;
  Sdma sdma;
  hipStream_t cs = nullptr;                      // copy_engine 1 only
  uint8_t *tables_host = nullptr, *tables_dev = nullptr;
  bool general = false;                          // dabx_ingest_open_formats
  size_t pitch = 0;                              // ... bytes per stream region of a slab
  std::vector<IqDecode> dec;                     // [S]
  std::vector<int> M, tab, carry_n;              // [S] input samples per ms (0 = 2.048 MS/s), table index, samples carried between slabs
  float2 *work = nullptr, *carry = nullptr;
  size_t work_pitch = 0, carry_pitch = 0;
  int16_t *tab_int = nullptr; float *tab_frac = nullptr;
};

// The job table of a stage that runs on some slots only (k_packet: PacketSlot / PacketDev, k_pad: PadSlot / PadDev, k_mot: MotSlot / MotDev, k_carousel: CarouselSlot / CarouselDev, k_data_handler: DataSlot / DataDev).  Nothing of it exists
// until the stage's dabx_set_*_mode first switches a slot on: host stays empty, dev.n stays 0 and no batch launches the kernel.
// host[sj].st mirrors the device's table entry of the slot; the device owns it between download and upload (both with the engine drained).
template <class Slot, class Dev> struct JobTable {
  struct Host { bool on = false; Slot st{}; long long seen = 0, lost = 0; };     // seen: items a read call has returned or passed, lost: those it found gone
  std::vector<Host> host;                      // [S][max_subch], or empty
  std::vector<int> index;                      // [S][max_subch] place in the table, -1 = not a slot of this stage
  Dev dev{};                                   // slots = the table on the device, n = its length
  int cap = 0;
  bool on(size_t sj) const { return !host.empty() && host[sj].on; }
  // the device's table back into the mirror
  int download(int max_subch)
  {
    if (dev.n <= 0) return 0;
    std::vector<Slot> tab((size_t)dev.n);
    DABX_HIP(hipMemcpy(tab.data(), dev.slots, sizeof(Slot) * tab.size(), hipMemcpyDeviceToHost));
    for (const Slot &q : tab) host[(size_t)q.s * max_subch + q.j].st = q;
    return 0;
  }
  // ... and the table rebuilt from the mirror: the stage's slots, in (stream, slot) order
  int upload()
  {
    std::vector<Slot> tab;
    std::fill(index.begin(), index.end(), -1);
    for (size_t sj = 0; sj < host.size(); sj++)
      if (host[sj].on) { index[sj] = (int)tab.size(); tab.push_back(host[sj].st); }
    if ((int)tab.size() > cap) {
      Slot *q = nullptr;
      const int n = std::max<int>(2 * cap, std::max<int>(16, (int)tab.size()));
      DABX_HIP(hipMalloc(&q, sizeof(Slot) * (size_t)n));
      if (dev.slots) (void)hipFree(dev.slots);
      dev.slots = q; cap = n;
    }
    if (!tab.empty()) DABX_HIP(hipMemcpy(dev.slots, tab.data(), sizeof(Slot) * tab.size(), hipMemcpyHostToDevice));
    dev.n = (int)tab.size();
    return 0;
  }
  void drop(size_t sj)                         // the slot leaves the stage: its rings are freed
  {
    if (sj >= host.size() || !host[sj].on) return;
    (void)hipFree(host[sj].st.out.bytes);
    (void)hipFree(host[sj].st.out.recs);
    host[sj] = Host{};
  }
  void destroy()
  {
    for (size_t sj = 0; sj < host.size(); sj++) drop(sj);
    if (dev.slots) (void)hipFree(dev.slots);
  }
};

// ---- what the stages with a record ring (rec_ring.h) share --------------------------------------------------------------------------------
inline void hip_free_all(std::initializer_list<void *> ptrs) { for (void *q : ptrs) if (q) (void)hipFree(q); }

// Every buffer of the table allocated and zeroed, or none of them: after a failure the pointers are null again, the error is set in the
// name of `who` and the return is DABX_E_NOMEM (out of memory) or DABX_E_HIP.
struct DevBuf { void **p; size_t bytes; };
inline int alloc_zeroed(const char *who, std::initializer_list<DevBuf> bufs)
{
  for (const DevBuf &b : bufs) *b.p = nullptr;
  for (const DevBuf &b : bufs) {
    hipError_t he = hipMalloc(b.p, b.bytes);
    if (he == hipSuccess) he = hipMemset(*b.p, 0, b.bytes);
    if (he == hipSuccess) continue;
    set_error("%s: HIP error %d (%s) allocating the stage", who, (int)he, hipGetErrorString(he));
    for (const DevBuf &q : bufs) { if (*q.p) (void)hipFree(*q.p); *q.p = nullptr; }
    return he == hipErrorOutOfMemory ? DABX_E_NOMEM : DABX_E_HIP;
  }
  return 0;
}

// One dabx_read_* call on a stream's ring: what the ring has overwritten since the last call is dropped and counted (*lost: this call's,
// *lost_total: the stage's running total, where it keeps one), then up to max_records records go through copy(n, slot), oldest first.
// total: the stream's record counter, just read from the device; seen: the records earlier calls have returned or passed.
template <int RING, int SLOT_BYTES, class CopySlot>
int rec_ring_read(const uint8_t *ring, int stream, long long total, long long &seen, long long *lost_total, int max_records, int32_t *lost, CopySlot copy)
{
  if (const long long gone = rec_window(total, seen, RING).gone) {
    if (lost) *lost = (int32_t)std::min<long long>(gone, INT32_MAX);
    if (lost_total) *lost_total += gone;
    seen += gone;
  }
  int n = 0;
  for (; n < max_records && seen < total; n++, seen++)
    if (int rc = copy(n, rec_slot<RING, SLOT_BYTES>(ring, stream, seen))) return rc;
  return n;
}

// The TII stage (include/dabx.h dabx_set_tii_mode, deliver.hip k_tii).  Nothing of it exists until the mode is first switched on: dev stays all
// null, n_on stays 0 and no step launches the kernel.
struct TiiStage {
  TiiDev dev{};
  uint8_t *tables = nullptr;                   // turn [768] + pattern [72]
  int n_on = 0;                                // streams with the mode on
  std::vector<TiiCfgDev> cfg;                  // [S] mirror of dev.cfg but for epoch_seen, which the device owns
  std::vector<long long> seen;                 // [S] events dabx_read_tii_events has returned or passed
  long long launches = 0;
  bool exists() const { return dev.pairs != nullptr; }
};

// What the scope, the CIR and the spectrum stage share: the streams with the mode on as a compacted list for the stage's kernels (one block
// each), a settings row per stream and the read-out's bookkeeping.  Nothing of a stage exists until its mode is first switched on: its dev
// stays all null, n_on stays 0 and no step launches a kernel of it.
template <class Cfg> struct ListedStage {
  int32_t *list = nullptr;                     // [S] device: the first n_on entries are the streams with the mode on
  Cfg *cfg_dev = nullptr;                      // [S] device
  int n_on = 0;
  std::vector<Cfg> cfg;                        // [S] mirror of cfg_dev
  std::vector<long long> seen, lost;           // [S] records the stage's dabx_read_* has returned or passed / found gone
  long long launches = 0;
  bool exists() const { return list != nullptr; }
  // the settings and the list rebuilt from them, to the device (with the engine drained); *dev_n: the length the stage's kernels go by
  int upload(int32_t *dev_n)
  {
    std::vector<int32_t> on;
    for (size_t s = 0; s < cfg.size(); s++) if (cfg[s].enable) on.push_back((int32_t)s);
    DABX_HIP(hipMemcpy(cfg_dev, cfg.data(), sizeof(Cfg) * cfg.size(), hipMemcpyHostToDevice));
    if (!on.empty()) DABX_HIP(hipMemcpy(list, on.data(), sizeof(int32_t) * on.size(), hipMemcpyHostToDevice));
    n_on = *dev_n = (int)on.size();
    return 0;
  }
  void start(size_t S) { cfg.assign(S, Cfg{}); seen.assign(S, 0); lost.assign(S, 0); }     // (a stage that was just created)
};

// The scope stage (include/dabx.h dabx_set_scope_mode, pipeline.hip k_scope)
struct ScopeStage : ListedStage<ScopeCfgDev> {
  ScopeDev dev{};
};

// The CIR / correlation plot stage (include/dabx.h dabx_set_cir_mode, pipeline.hip k_cir, k_cir_finish, k_cir_corr)
struct CirStage : ListedStage<CirCfgDev> {
  CirDev dev{};
  int n_corr = 0;                              // streams with the correlation plot on
  std::vector<CirState> walk;                  // [S] the host's own window / row bookkeeping (base, win, rows_done): the same function over the same
                                               //     wr as the device's, so that a step launches as many blocks per stream as rows are due
};

// The RF spectrum / waterfall stage (include/dabx.h dabx_set_spectrum_mode, pipeline.hip k_spectrum)
struct SpecStage : ListedStage<SpecCfgDev> {
  SpecDev dev{};
  float *window = nullptr;                     // [2048] device (SpecDev::window)
};

// The FIG stage (include/dabx.h dabx_set_fig_mode, deliver.hip k_fig).  Nothing of it exists until the mode is first switched on: dev stays all
// null, n_on stays 0 and no step launches the kernel.
struct FigStage {
  FigDev dev{};
  int n_on = 0;                                // streams with the mode on
  std::vector<int32_t> on;                     // [S] mirror of dev.on
  std::vector<int32_t> si_on;                  // [S] mirror of dev.si_on (empty until a stream first asks for the service information)
  int n_si = 0;                                // streams that follow it now: k_fig_si is launched while there is one, k_fig otherwise
  std::vector<long long> seen;                 // [S] events dabx_read_fig_events has returned or passed
  long long launches = 0;
  bool timing = false;                         // dabx_internal_fig_timing: every launch between two events of its own
  std::vector<hipEvent_t> timed;               // ... begin, end, begin, end, ...
  bool exists() const { return dev.st != nullptr; }
  bool on_for(int s) const { return exists() && on[(size_t)s] != 0; }
  bool si_for(int s) const { return on_for(s) && dev.si != nullptr && si_on[(size_t)s] != 0; }
};

struct dabx_engine : dabx::EngineHead {         // (iqfile.h: the ring format, where iqfile.cpp can read it)
  dabx_config cfg{};
  EngineDev dev{};
  hipStream_t stream = nullptr;                // == ss.a (front end)
  EngineStreams ss;
  BatchSnap *snap_buf[2] = {nullptr, nullptr};
  int device = 0;
  std::vector<unsigned long long> wr_host;     // host mirror of committed samples
  std::vector<SubchDev> subch_host;            // [S][max_subch]
  std::vector<int> subch_id_host;              // [S][max_subch] SubChId (host only: ETI STC field)
  struct EtiCursor { long long next_cif = -1; int hi = -1, lo = -1; long long fib_frames_seen = 0; };
  std::vector<EtiCursor> eti;                  // [S]
  std::vector<dabx_fibdec *> fibdec;           // [S] FIB decoders (current / next configuration), created on first dabx_follow_fic
  std::vector<long long> fib_frames_fed;       // [S] frames whose FIBs the decoder has seen
  bool fig_reference_quirks = false;           // dabx_set_fig_reference_quirks: the engine's own FIB decoders swap like the reference (flags 3 only)
  std::vector<dabx_tii *> tii;                 // [S] detectors, created on first dabx_read_tii
  std::vector<int> tii_epoch;                  // [S] reset epoch seen by the detector
  TiiStage tiis;                               // the detectors on the device
  ScopeStage scope;                            // the IQ scope and carrier plots on the device
  CirStage cir;                                // the channel impulse response and the correlation plot on the device
  SpecStage spectrum;                          // the RF spectrum and waterfall rows on the device
  FigStage fig;                                // the FIG walk on the device
  std::vector<void *> allocs;
  void *stage = nullptr;                       // host -> device staging of dabx_push_iq
  size_t stage_cap = 0;
  // dabx_push_iq_async: a small pool of device staging slots, each guarded by the event of its last conversion kernel, so
  // that consecutive pushes from pinned host memory queue back to back on the ingest stream (DMA at PCIe rate, no host wait)
  static constexpr int ASYNC_SLOTS = 8;
  void *aslot[ASYNC_SLOTS] = {nullptr};
  size_t aslot_cap[ASYNC_SLOTS] = {0};
  hipEvent_t aslot_done[ASYNC_SLOTS] = {nullptr};
  unsigned long long async_pushes = 0;
  hipStream_t ingest = nullptr;                // dabx_push_iq: copy + format conversion, concurrent with the receiver streams
  hipStream_t ingest2 = nullptr;               // dabx_push_iq_async alternates between the two: the DMA of push k + 1 runs under the conversion of push k
  hipEvent_t ingest_done = nullptr;
  std::vector<unsigned long long> rd_seen;     // [S] read index of every stream when last looked at (lower bound)
  std::vector<StreamCtl> ctl_peek;
  int max_kbps = 0;
  bool buffers_ready = false;
  Marker mk;
  double prof_ms[N_STEP_KERNELS] = {0};
  long long prof_n[N_STEP_KERNELS] = {0};
  int pending_frames = 0;                      // front-end steps whose CIFs still await the MSC decoder
  bool have_fast = false;
  MscFast fast{};

  std::vector<void *> fast_allocs;             // buffers of the current MSC classes (replaced on reconfiguration)
  bool classes_dirty = false;
  std::vector<char> announcing;                // per stream: the zero-copy producer uses dabx_announce_write
  unsigned long long *horizon_host = nullptr;  // hipHostMalloc'ed, EngineDev::wr_horizon: what pushes may have overwritten (written BEFORE a copy is issued)
  int32_t *locked_host = nullptr;              // hipHostMalloc'ed: number of streams in lock, kept by the device (EngineDev::locked_count)
  int32_t *seq_timeouts_host = nullptr;        // hipHostMalloc'ed: device-side waits that gave up (EngineDev::seq_timeouts)
  bool level_dirty = false;                    // exact_level_tracker: steps have been issued since k_level_exact last ran behind them
  Delivery dl;
  Ingest ing;
  JobTable<PacketSlot, PacketDev> pkt;         // packet-mode slots (include/dabx.h "Packet-mode data sub-channels", k_packet)
  JobTable<PadSlot, PadDev> pad;               // PAD slots (include/dabx.h "Programme-associated data", k_pad)
  JobTable<MotSlot, MotDev> mot;               // MOT slots (include/dabx.h "MOT objects of the X-PAD", k_mot): PAD slots all of them
  JobTable<CarouselSlot, CarouselDev> car;     // carousel slots (include/dabx.h "MOT objects of a packet-mode carousel", k_carousel): packet-mode slots all of them
  JobTable<Mp2AudioSlot, Mp2AudioDev> mpa;     // MP2 audio slots (include/dabx.h "MP2 audio", k_mp2_audio)
  long long mpa_launches = 0;                  // k_mp2_audio launches (dabx_mp2_audio_stats.launches)
  JobTable<AacStreamSlot, AacStreamDev> aac;   // AAC stream slots (include/dabx.h "AAC stream", k_aac_stream): DAB+ slots all of them
  long long aac_launches = 0;                  // k_aac_stream launches (dabx_aac_stream_stats.launches)
  JobTable<DataSlot, DataDev> dat;             // slots with a data handler (include/dabx.h "The data handlers of a packet-mode slot", k_data_handler): packet-mode slots all of them
  DataStageCtl dat_ctl;                        // k_data_handler launches (dabx_data_stats.launches) and their timing events
  int build_msc_classes();
  int delivery_layout();                       // offsets of every slot's bytes in a slab for the sub-channels configured now
  int delivery_begin(DeliverDev *dv, int *slot, int *devslab);     // a chunk closes: host + device slab, front gather on stream a
  int delivery_finish(int slot, int devslab, hipStream_t tail);    // ... its slot gather is queued on `tail`: the one copy
  void delivery_abort(int slot, int devslab);                      // ... or it cannot be: both slabs go back

  // stream s's ring: its first element, whatever the element is (EngineDev::ring_fmt)
  void *ring_of(int s) const { return static_cast<char *>(dev.iq) + (size_t)s * dev.ring_len * ring_bytes_per_sample(dev.ring_fmt); }
  template <class T> int alloc(T **p, size_t count, bool zero = true) { return alloc_bytes(p, count * sizeof(T), zero); }
  template <class T> int alloc_bytes(T **p, size_t n_bytes, bool zero = true)
  {
    void *q = nullptr;
    const size_t bytes = std::max<size_t>(n_bytes, 16);
    DABX_HIP(hipMalloc(&q, bytes));
    if (zero) DABX_HIP(hipMemsetAsync(q, 0, bytes, stream));
    allocs.push_back(q);
    *p = reinterpret_cast<T *>(q);
    return 0;
  }
};

// ---- helpers of more than one engine*.cpp file, each defined in the file that owns its subsystem -------------------------------------
namespace dabx {
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// engine.cpp
int need_device_e();
int use_device(const dabx_engine *e);
int sync_all(dabx_engine *e, bool chain_only = false);
int ring_takes(const dabx_engine *e, int fmt, const char *who);
void announce_write(dabx_engine *e, int stream, unsigned long long upto);
int commit_impl(dabx_engine *e, int stream, size_t n);
int push_room(dabx_engine *e, int stream, size_t n, const char *who);
// engine_delivery.cpp
int delivery_drain(dabx_engine *e);
void delivery_free(dabx_engine *e);
// engine_ingest.cpp
void ingest_free(dabx_engine *e);
// engine_tii.cpp
void tii_stage_free(dabx_engine *e);
// engine_fig.cpp
void fig_stage_free(dabx_engine *e);
int fig_step(dabx_engine *e);                     // k_fig behind a frame's FIC decoder, while a stream has the mode on
// engine_scope.cpp
void scope_stage_free(dabx_engine *e);
// engine_cir.cpp
void cir_stage_free(dabx_engine *e);
int cir_step_cap(dabx_engine *e, bool advance);   // the rows due per stream in the step about to be launched, at most; advance: the host's bookkeeping moves on
// engine_spectrum.cpp
void spectrum_stage_free(dabx_engine *e);
// engine_slots.cpp
void pad_count_sources(dabx_engine *e);
int mot_follow_pad(dabx_engine *e);
int carousel_follow_packet(dabx_engine *e);
int data_follow_packet(dabx_engine *e);

// How the dabx_read_* and dabx_get_*_stats entries of a ListedStage begin: the engine drained, the stream's state record read from the
// device.  0: *c holds it; 1: the stage does not exist (nothing to read: the entry returns 0); < 0: the error to return.
template <class Stage, class State> int stage_state(dabx_engine *e, const Stage &T, int stream, State *c)
{
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  if (!T.exists()) return 1;
  DABX_HIP(hipMemcpy(c, T.dev.st + stream, sizeof(*c), hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace dabx
