// engine.cpp -- host side of the stream-batched receiver and the engine-level C ABI (include/dabx.h): create, destroy, configure, push,
// process, read, statistics.  Its subsystems: engine_delivery.cpp (bulk delivery), engine_ingest.cpp (bulk ingest), engine_slots.cpp (packet-mode
// and PAD slots), engine_facade.cpp (dabx_fic_* / dabx_msc_* and the test entries); engine.h is what the five share.
#include "engine.h"
#include "viterbi_core.h"
#include "fig00.h"
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

// Groups the active (stream, slot) pairs by protection profile for the lane-per-trellis decoder (vit_t.hip): every
// class gets its depuncture map, pair list and transposed-symbol / decision scratch.  Up to MSC_MAX_CLASSES classes,
// largest first; classes too small to fill a few waves and anything beyond stay with the wave-per-trellis kernel.
int dabx_engine::build_msc_classes()
{
  const EngineDev &d = dev;
  have_fast = false;
  fast = MscFast{};
  for (void *q : fast_allocs) {
    (void)hipFree(q);
    allocs.erase(std::remove(allocs.begin(), allocs.end(), q), allocs.end());
  }
  fast_allocs.clear();
  for (auto &sc : subch_host) sc.fast_class = 0;
  if (d.max_subch <= 0) return 0;
  struct Key { int kbps, prot, shortf, cu; bool operator<(const Key &o) const { return std::tie(kbps, prot, shortf, cu) < std::tie(o.kbps, o.prot, o.shortf, o.cu); } };
  std::map<Key, std::vector<uint32_t>> groups;
  int active = 0;
  for (int s = 0; s < d.n_streams; s++)
    for (int j = 0; j < d.max_subch; j++) {
      const SubchDev &sc = subch_host[(size_t)s * d.max_subch + j];
      if (!sc.active) continue;
      active++;
      groups[Key{sc.kbps, sc.prot_level, sc.short_form, sc.cu_size}].push_back(((uint32_t)s << 8) | (uint32_t)j);
    }
  std::vector<std::pair<Key, std::vector<uint32_t>>> order(groups.begin(), groups.end());
  std::stable_sort(order.begin(), order.end(), [](const auto &a, const auto &b) {
    return (long long)a.second.size() * a.first.kbps > (long long)b.second.size() * b.first.kbps; });
  // 64 trellises per wave: measured break-even against the wave-per-trellis kernel at ~320 waves per batch (40-48 streams
  // of 18 sub-channels); a class with fewer than 4 decoder waves per full batch is not worth its own launch slice.
  // dabx_config.msc_fast_min_jobs / msc_class_min_jobs override both (include/dabx.h).
  const size_t min_jobs = cfg.msc_fast_min_jobs > 0 ? (size_t)cfg.msc_fast_min_jobs : (size_t)64 * 320;
  const size_t class_min_jobs = cfg.msc_class_min_jobs > 0 ? (size_t)cfg.msc_class_min_jobs : 256;
  const int max_cifs = 4 * MSC_BATCH_FRAMES;
  long long jobs_total = 0;
  std::vector<std::vector<uint32_t>> host_pairs;
  int rc;
  auto falloc = [&](auto **p, size_t count) {
    int r = alloc(p, count, false);
    if (!r) fast_allocs.push_back(*p);
    return r;
  };
  for (const auto &kv : order) {
    if (fast.n_cls >= MSC_MAX_CLASSES) break;
    const Key &k = kv.first;
    const std::vector<uint32_t> &pairs = kv.second;
    if (pairs.size() * (size_t)max_cifs < class_min_jobs) continue;
    std::vector<uint16_t> m;
    int n_in = 0;
    if ((rc = host_profile_map(k.kbps, k.prot, k.shortf, m, &n_in))) return rc;
    if (n_in % 64 != 0 || n_in != k.cu * 64) continue;
    for (auto &v : m) if (v == PUNCT) v = (uint16_t)n_in;
    MscClass c{};
    c.n_in = n_in; c.nbits = 24 * k.kbps; c.n_pairs = (int)pairs.size();
    uint16_t *map2 = nullptr;
    uint32_t *pr = nullptr;
    if ((rc = falloc(&map2, m.size()))) return rc;
    if ((rc = falloc(&pr, pairs.size()))) return rc;
    DABX_HIP(hipMemcpy(map2, m.data(), m.size() * 2, hipMemcpyHostToDevice));
    DABX_HIP(hipMemcpy(pr, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
    c.map2 = map2; c.pairs = pr;
    const size_t ngroups = (pairs.size() * (size_t)max_cifs + 63) / 64;
    if ((rc = falloc(&c.inT[0], ngroups * (size_t)(n_in / 4 + 1) * 64))) return rc;
    if ((rc = falloc(&c.inT[1], ngroups * (size_t)(n_in / 4 + 1) * 64))) return rc;
    if ((rc = falloc(&c.decT, ngroups * (size_t)(c.nbits + 6) * 64))) return rc;
    fast.cls[fast.n_cls++] = c;
    host_pairs.push_back(pairs);
    jobs_total += (long long)pairs.size() * max_cifs;
  }
  // launch order: longest trellises first, so that the short ones fill in behind them
  std::vector<int> idx(fast.n_cls);
  for (int i = 0; i < fast.n_cls; i++) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return fast.cls[a].nbits > fast.cls[b].nbits; });
  MscFast sorted = fast;
  for (int i = 0; i < fast.n_cls; i++) {
    sorted.cls[i] = fast.cls[idx[i]];
    for (uint32_t q : host_pairs[idx[i]]) subch_host[(size_t)(q >> 8) * d.max_subch + (q & 255u)].fast_class = i + 1;
  }
  fast = sorted;
  fast.min_jobs = (int)std::min<size_t>(min_jobs, 0x7fffffff);
  fast.slots_active = active;
  have_fast = fast.n_cls > 0 && (size_t)jobs_total >= min_jobs;   // every viterbi_tie_mode has its lane-per-trellis kernel (vit_t.hip)
  DABX_HIP(hipMemcpy(d.subch, subch_host.data(), sizeof(SubchDev) * subch_host.size(), hipMemcpyHostToDevice));
  return 0;
}

namespace dabx {

int need_device_e()
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device available (libdabx has no CPU fallback)"); return DABX_E_NODEVICE; }
  return 0;
}

// Engine calls may come from any host thread: bind the thread to the engine's device first (allocations, launches and
// copies below otherwise go to whatever device the calling thread happens to have current).
int use_device(const dabx_engine *e)
{
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur == e->device) return 0;
  DABX_HIP(hipSetDevice(e->device));
  return 0;
}

// chain_only: what dabx_process(sync != 0) waits for -- the frame chain, the MSC batches and the delivery of the frames it issued -- but not
// a search pass that runs next to them on stream q for streams out of lock (its results are picked up by the next step either way)
int sync_all(dabx_engine *e, bool chain_only)
{
  if (int rc = use_device(e)) return rc;
  DABX_HIP(hipStreamSynchronize(e->stream));
  if (e->ss.b) DABX_HIP(hipStreamSynchronize(e->ss.b));
  if (e->ss.d) DABX_HIP(hipStreamSynchronize(e->ss.d));
  if (e->seq_timeouts_host && __atomic_load_n(e->seq_timeouts_host, __ATOMIC_RELAXED) != 0) {
    set_error("%d device-side hand-overs of the few-stream schedule timed out (a kernel launch in front of them failed): the results since are undefined",
              (int)__atomic_load_n(e->seq_timeouts_host, __ATOMIC_RELAXED));
    return DABX_E_HIP;
  }
  if (int rc = delivery_drain(e)) return rc;                       // every chunk closed so far has landed
  if (chain_only && !e->dev.exact_level) return 0;
  if (e->ss.q) DABX_HIP(hipStreamSynchronize(e->ss.q));
  e->ss.acq_in_flight = false;
  // cfg.exact_level_tracker: the level tracker follows the frame chain on its own; behind the last frame it is run once more, so
  // that what the host reads next (dabx_get_stats, the ring's read cursor) includes every sample the receiver has read
  if (e->dev.exact_level && e->dev.level_pos && e->level_dirty) {
    if (int rc = launch_level_exact(e->dev, e->stream)) return rc;
    DABX_HIP(hipStreamSynchronize(e->stream));
    e->level_dirty = false;
  }
  return 0;
}

// a push / slab of fmt into this engine's ring?  (a native ring takes its own codes only: they are copied, never converted)
int ring_takes(const dabx_engine *e, int fmt, const char *who)
{
  if (e->dev.ring_fmt == RING_CF32 || fmt == e->dev.ring_fmt) return 0;
  static const char *const name[3] = {"cf32", "int16", "uint8"};
  set_error("%s: fmt %d (%s) into a DABX_RING_%s ring: a native ring takes its own codes only", who, fmt, name[fmt], e->dev.ring_fmt == RING_S16 ? "S16" : "U8");
  return DABX_E_ARG;
}

}  // namespace dabx

static int create_impl(const dabx_config *cfg, int ring_fmt, dabx_engine **out)
{
  if (!cfg || !out || cfg->n_streams <= 0 || cfg->ring_frames < 2 || cfg->max_subch < 0 || cfg->max_subch > MAX_SUBCH ||
      cfg->out_frames < 1 || cfg->soft_bit_type < 1 || cfg->soft_bit_type > 3 || cfg->dc_iq_correction < 0 || cfg->dc_iq_correction > 2 ||
      cfg->viterbi_tie_mode < 0 || cfg->viterbi_tie_mode > 2 || cfg->schedule < 0 || cfg->schedule > 1 ||
      cfg->msc_fast_min_jobs < 0 || cfg->msc_class_min_jobs < 0 || cfg->exact_level_tracker < 0 || cfg->exact_level_tracker > 2 ||
      cfg->acquire_mode < 0 || cfg->acquire_mode > 2) {
    set_error("dabx_create: bad configuration");
    return DABX_E_ARG;
  }
  int rc = need_device_e();
  if (rc) return rc;
  auto *e = new dabx_engine();
  e->cfg = *cfg;
  // from here on every failure goes through dabx_destroy (streams, events and buffers created so far are released)
#define H(x) do { hipError_t err__ = (x); if (err__ != hipSuccess) { set_error("HIP error %d (%s) at %s:%d", (int)err__, hipGetErrorString(err__), __FILE__, __LINE__); dabx_destroy(e); return DABX_E_HIP; } } while (0)
  H(hipGetDevice(&e->device));
  // front end (frame-to-frame feedback = critical path) above the batched MSC decode
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);       // lo = least urgent (numerically greatest)
  H(hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, prio_hi));
  e->ss.a = e->stream;
  if (cfg->schedule == 0) {
    // overlapped schedule (default): MSC batches on b, the MSC symbols' demapper on d (pipeline.hip, launch_front_step /
    // launch_msc_batch).  All streams live on this device: a device-scope release is all a dependency needs (the default
    // system-scope release writes the caches back for host visibility on every record)
    H(hipStreamCreateWithPriority(&e->ss.b, hipStreamNonBlocking, prio_lo));
    H(hipStreamCreateWithPriority(&e->ss.d, hipStreamNonBlocking, prio_hi));
    H(hipEventCreateWithFlags(&e->ss.prep_done, hipEventDisableTiming | hipEventReleaseToDevice));
    H(hipEventCreateWithFlags(&e->ss.msc_done, hipEventDisableTiming | hipEventReleaseToDevice));
    H(hipEventCreateWithFlags(&e->ss.fic_go, hipEventDisableTiming | hipEventReleaseToDevice));
    H(hipEventCreateWithFlags(&e->ss.prep_b_done, hipEventDisableTiming | hipEventReleaseToDevice));
    H(hipEventCreateWithFlags(&e->ss.demap_done, hipEventDisableTiming | hipEventReleaseToDevice));
    H(hipEventCreateWithFlags(&e->ss.sym_done, hipEventDisableTiming | hipEventReleaseToDevice));
    // few streams: the demapper of a frame on stream d in one launch, hand-overs by device-side sequence numbers (pipeline.h, fic_on_d /
    // EngineDev::flag_sync).  The threshold is k_symbols' own (FEW_STREAMS, sym_blocks_per_stream: below it a frame's symbols are spread over
    // more blocks because latency, not throughput, is what is left) -- and the bound under which every block of the kernels that wait for each
    // other is resident at once.
    e->ss.fic_on_d = cfg->n_streams < FEW_STREAMS;
    // the ingest stream BEFORE q: the runtime deals streams to its hardware queues in order of creation, and as the fifth stream the
    // ingest stream shared one (every synchronous push 20 us = 20 % dearer at 512 streams, tools/bench_ingest.py)
    H(hipStreamCreateWithFlags(&e->ingest, hipStreamNonBlocking));
    // streams out of lock are searched on q next to the steps of the others (dabx_process with sync == 0)
    // With the exact level tracker every stream has a block on q in every step (two lone waves for 1.6 ms): at the lowest queue
    // priority those blocks were dispatched only into the gaps the frame chain's kernels left (5 ms per step); at the chain's own
    // priority they are resident from the start of the step.
        H(hipStreamCreateWithPriority(&e->ss.q, hipStreamNonBlocking, cfg->exact_level_tracker == 1 ? prio_hi : prio_lo));
    H(hipEventCreateWithFlags(&e->ss.acq_done, hipEventDisableTiming | hipEventReleaseToDevice));
    H(hipEventCreateWithFlags(&e->ss.tail_done, hipEventDisableTiming | hipEventReleaseToDevice));
    H(hipEventCreateWithFlags(&e->ss.acq_a_done, hipEventDisableTiming | hipEventReleaseToDevice));
  }
  if (!e->ingest) H(hipStreamCreateWithFlags(&e->ingest, hipStreamNonBlocking));
  // (ingest2 is created by the first dabx_push_iq_async: every HIP stream that exists makes each synchronous push -- a pageable
  // hipMemcpyAsync, an event, a stream wait and a stream synchronisation -- about 20 us dearer, 20 % of a push at 512 streams)
  H(hipEventCreateWithFlags(&e->ingest_done, hipEventDisableTiming | hipEventReleaseToDevice));
  e->rd_seen.assign(cfg->n_streams, 0);
  const int S = cfg->n_streams;
  EngineDev &d = e->dev;
  d.n_streams = S; d.max_subch = cfg->max_subch; d.out_frames = cfg->out_frames;
  d.ring_len = cfg->ring_frames * TF;
  d.ring_fmt = e->ring_fmt = ring_fmt;
  d.threshold = cfg->sync_threshold; d.strongest = cfg->sync_strongest;
  d.fic_only = cfg->fic_only; d.capture_soft = cfg->capture_soft; d.tie_mode = cfg->viterbi_tie_mode;
  d.exact_level = cfg->exact_level_tracker == 1;
  d.anchor_level = cfg->exact_level_tracker == 0;
  const DevTables *t;
  if ((rc = get_tables(&t))) { dabx_destroy(e); return rc; }
#define A(x) if ((rc = (x))) { dabx_destroy(e); return rc; }
  A(e->alloc_bytes(&d.iq, (size_t)S * d.ring_len * ring_bytes_per_sample(ring_fmt), false));
  A(e->alloc(&d.wr, S));
  A(e->alloc(&d.ctl, S));
  A(e->alloc(&d.spectra, (size_t)2 * S * 75 * K, false));
  A(e->alloc(&d.fsnap, S));
  A(e->alloc(&d.sym_seq, S));
  A(e->alloc(&d.fic_seq, S));
  A(e->alloc(&d.demap_busy, S));
  A(e->alloc(&d.dciq_state, (size_t)S * 8));
  A(e->alloc(&d.dciq_done, S));
  if (d.exact_level) A(e->alloc(&d.level_pos, S));
  H(hipHostMalloc((void **)&e->locked_host, sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
  *e->locked_host = 0;
  H(hipHostMalloc((void **)&e->horizon_host, sizeof(unsigned long long) * S, hipHostMallocMapped | hipHostMallocCoherent));
  for (int s = 0; s < S; s++) e->horizon_host[s] = 0;
  e->announcing.assign(S, 0);
  H(hipHostGetDevicePointer((void **)&d.wr_horizon, e->horizon_host, 0));
  H(hipHostGetDevicePointer((void **)&d.locked_count, e->locked_host, 0));
  H(hipHostMalloc((void **)&e->seq_timeouts_host, sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
  *e->seq_timeouts_host = 0;
  H(hipHostGetDevicePointer((void **)&d.seq_timeouts, e->seq_timeouts_host, 0));
  {
    std::vector<float> st8((size_t)S * 8, 0.0f);                  // sample_reader.h:102-106: meanII = meanQQ = 1
    for (int s_ = 0; s_ < S; s_++) { st8[(size_t)s_ * 8 + 2] = 1.0f; st8[(size_t)s_ * 8 + 3] = 1.0f; }
    H(hipMemcpyAsync(d.dciq_state, st8.data(), sizeof(float) * st8.size(), hipMemcpyHostToDevice, e->stream));
    H(hipStreamSynchronize(e->stream));
  }
  A(e->alloc(&d.nco_tid, (size_t)S * 256));
  A(e->alloc(&d.nco_sym, (size_t)S * 76));
  A(e->alloc(&d.sym_off, (size_t)S * 76));
  A(e->alloc(&e->snap_buf[0], S));
  A(e->alloc(&e->snap_buf[1], S));
  d.snap = e->snap_buf[0];
  A(e->alloc(&d.tii_acc, (size_t)S * TU));
  A(e->alloc(&d.tii_cnt, (size_t)S * 2));
  e->tii.assign((size_t)S, nullptr);
  e->fibdec.assign((size_t)S, nullptr);
  e->fib_frames_fed.assign((size_t)S, 0);
  e->tii_epoch.assign((size_t)S, 0);
  A(e->alloc(&d.cp_part, (size_t)S * 75));
  A(e->alloc(&d.abs_part, (size_t)S * 76));
  A(e->alloc(&d.fic_sym, (size_t)S * 3 * K2));
  A(e->alloc(&d.tdi, (size_t)S * TDI_SLOTS * CIF_BITS));
  A(e->alloc(&d.subch, (size_t)S * std::max(1, d.max_subch)));
  A(e->alloc(&d.fib_out, (size_t)S * d.out_frames * 12 * 32));
  A(e->alloc(&d.fib_crc, (size_t)S * d.out_frames * 12));
  A(e->alloc(&d.frame_pos, (size_t)S * d.out_frames));
  A(e->alloc(&d.frame_start, (size_t)S * d.out_frames));
  if (d.capture_soft) A(e->alloc(&d.soft_cap, (size_t)S * 75 * K2));
  A(e->alloc(&d.sf_info, (size_t)S * std::max(1, d.max_subch) * SF_SLOTS));
  // demapper state (constructor defaults: ofdm_decoder.h:101-104)
  A(demap_alloc(d.demap, S));
  d.demap.soft_type = cfg->soft_bit_type;
  A(launch_demap_init(d.demap, e->stream));
  // per-stream scalars: SampleReader / DabProcessor defaults (sample_reader.h:95,101; dab_processor.h:129-138)
  std::vector<StreamCtl> ctl(S);
  for (auto &c : ctl) {
    memset(&c, 0, sizeof(c));
    c.state = ST_INIT; c.s_level = 0.1f; c.peak_level = -1.0e6f; c.sync_thr = cfg->sync_threshold;
    c.lvl_anchor_S = 0.1f;
  }
  H(hipMemcpyAsync(d.ctl, ctl.data(), sizeof(StreamCtl) * S, hipMemcpyHostToDevice, e->stream));
  H(hipStreamSynchronize(e->stream));
  e->wr_host.assign(S, 0);
  e->subch_host.assign((size_t)S * std::max(1, d.max_subch), SubchDev{});
  e->subch_id_host.assign((size_t)S * std::max(1, d.max_subch), -1);
  e->eti.assign((size_t)S, dabx_engine::EtiCursor{});
  // scratch sized for the FIC now; re-sized when sub-channels are configured
  d.vit_stride = (int)vit_scratch_words(FIC_OUT);
  A(e->alloc(&d.vit_scratch, (size_t)S * (4 + 4 * MSC_BATCH_FRAMES * d.max_subch) * d.vit_stride, false));
  d.msc_stride = 0; d.sf_stride = 0;
#undef A
#undef H
  *out = e;
  return 0;
}

extern "C" {

void dabx_default_config(dabx_config *c)
{
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->n_streams = 1; c->ring_frames = 4; c->max_subch = 18; c->out_frames = 4;
  c->sync_threshold = 3.0f;            // main/dabradio.cpp:92
  c->sync_strongest = 0;               // configuration.cpp:65
  c->soft_bit_type = 1;                // glob_enums.h:49-56 (SOFTDEC1)
}

int dabx_create(const dabx_config *cfg, dabx_engine **out) { return create_impl(cfg, RING_CF32, out); }
int dabx_create_ex(const dabx_config *cfg, const dabx_create_ext *ext, dabx_engine **out)
{
  if (!ext) return create_impl(cfg, RING_CF32, out);
  if (ext->size < offsetof(dabx_create_ext, reserved)) {
    set_error("dabx_create_ex: ext->size %u does not cover ring_format (sizeof(dabx_create_ext) is %zu)", ext->size, sizeof(dabx_create_ext));
    return DABX_E_ARG;
  }
  if (ext->ring_format < DABX_RING_CF32 || ext->ring_format > DABX_RING_U8) {
    set_error("dabx_create_ex: ring_format %d (DABX_RING_CF32 0, DABX_RING_S16 1, DABX_RING_U8 2)", ext->ring_format);
    return DABX_E_ARG;
  }
  if (ext->ring_format != DABX_RING_CF32 && cfg && cfg->dc_iq_correction) {
    set_error("dabx_create_ex: dc_iq_correction %d rewrites samples in place and its output is not a code: not with a DABX_RING_%s ring",
              cfg->dc_iq_correction, ext->ring_format == DABX_RING_S16 ? "S16" : "U8");
    return DABX_E_ARG;
  }
  // the native instantiations of the ring-reading kernels address an element by a 32-bit byte offset from its stream's ring (pipeline.hip, ring_elem)
  if (ext->ring_format != DABX_RING_CF32 && cfg && (unsigned long long)cfg->ring_frames * TF * ring_bytes_per_sample(ext->ring_format) >= (1ull << 32)) {
    set_error("dabx_create_ex: ring_frames %d: a stream's native ring stays below 4 GiB", cfg->ring_frames);
    return DABX_E_ARG;
  }
  return create_impl(cfg, ext->ring_format, out);
}
int dabx_get_ring_format(dabx_engine *e, int32_t *ring_format, int32_t *bytes_per_sample)
{
  if (!e) { set_error("dabx_get_ring_format: bad argument"); return DABX_E_ARG; }
  if (ring_format) *ring_format = e->dev.ring_fmt;
  if (bytes_per_sample) *bytes_per_sample = ring_bytes_per_sample(e->dev.ring_fmt);
  return 0;
}

void dabx_destroy(dabx_engine *e)
{
  if (!e) return;
  (void)use_device(e);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->ss.b) { (void)hipStreamSynchronize(e->ss.b); (void)hipStreamDestroy(e->ss.b); }
  if (e->ss.fic_go) (void)hipEventDestroy(e->ss.fic_go);
  if (e->ss.prep_b_done) (void)hipEventDestroy(e->ss.prep_b_done);
  if (e->ss.d) { (void)hipStreamSynchronize(e->ss.d); (void)hipStreamDestroy(e->ss.d); }
  if (e->ss.demap_done) (void)hipEventDestroy(e->ss.demap_done);
  if (e->ss.sym_done) (void)hipEventDestroy(e->ss.sym_done);
  if (e->ss.q) { (void)hipStreamSynchronize(e->ss.q); (void)hipStreamDestroy(e->ss.q); }
  if (e->ss.acq_done) (void)hipEventDestroy(e->ss.acq_done);
  if (e->ss.tail_done) (void)hipEventDestroy(e->ss.tail_done);
  if (e->ss.acq_a_done) (void)hipEventDestroy(e->ss.acq_a_done);
  if (e->ss.prep_done) (void)hipEventDestroy(e->ss.prep_done);
  if (e->ss.msc_done) (void)hipEventDestroy(e->ss.msc_done);
  delivery_free(e);
  ingest_free(e);
  for (dabx_tii *t : e->tii) dabx_tii_destroy(t);
  tii_stage_free(e);
  fig_stage_free(e);
  scope_stage_free(e);
  cir_stage_free(e);
  spectrum_stage_free(e);
  for (dabx_fibdec *f : e->fibdec) dabx_fibdec_destroy(f);
  if (e->ingest) { (void)hipStreamSynchronize(e->ingest); (void)hipStreamDestroy(e->ingest); }
  if (e->ingest2) { (void)hipStreamSynchronize(e->ingest2); (void)hipStreamDestroy(e->ingest2); }
  if (e->ingest_done) (void)hipEventDestroy(e->ingest_done);
  if (e->stage) (void)hipFree(e->stage);
  for (int i = 0; i < dabx_engine::ASYNC_SLOTS; i++) {
    if (e->aslot[i]) (void)hipFree(e->aslot[i]);
    if (e->aslot_done[i]) (void)hipEventDestroy(e->aslot_done[i]);
  }
  e->pkt.destroy();
  e->pad.destroy();
  e->mpa.destroy();
  e->aac.destroy();
  e->mot.destroy();
  e->car.destroy();
  e->dat.destroy();
  for (hipEvent_t ev : e->dat_ctl.timed) (void)hipEventDestroy(ev);
  for (void *p : e->allocs) (void)hipFree(p);
  if (e->locked_host) (void)hipHostFree(e->locked_host);
  if (e->seq_timeouts_host) (void)hipHostFree(e->seq_timeouts_host);
  if (e->horizon_host) (void)hipHostFree(e->horizon_host);
  for (auto &ev : e->mk.pool) (void)hipEventDestroy(ev);
  demap_free(e->dev.demap);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

static int set_subchannels_impl(dabx_engine *e, int stream, const dabx_subch_desc *desc, int n, long long at_cif /* < 0: the next CIF */)
{
  if (!e || n < 0 || n > e->dev.max_subch || (n > 0 && !desc) || stream >= e->dev.n_streams) {
    set_error("dabx_set_subchannels: bad argument");
    return DABX_E_ARG;
  }
  EngineDev &d = e->dev;
  int rc;
  if ((rc = sync_all(e))) return rc;
  // current CIF counters (Backend construction time, backend.cpp:38-70)
  std::vector<StreamCtl> ctl(d.n_streams);
  DABX_HIP(hipMemcpy(ctl.data(), d.ctl, sizeof(StreamCtl) * d.n_streams, hipMemcpyDeviceToHost));
  if (at_cif >= 0 && (stream < 0 || at_cif < ctl[stream].cif_no || at_cif > ctl[stream].cif_no + 3)) {
    set_error("dabx_set_subchannels_at: CIF %lld is not in the coming frame of stream %d (next CIF %lld)", at_cif, stream,
              stream < 0 ? -1ll : ctl[stream].cif_no);
    return DABX_E_ARG;
  }
  // refresh the host mirror: the device owns the dynamic fields (cif_out, super-frame state, counters)
  DABX_HIP(hipMemcpy(e->subch_host.data(), d.subch, sizeof(SubchDev) * e->subch_host.size(), hipMemcpyDeviceToHost));
  if ((rc = e->pkt.download(d.max_subch))) return rc;
  if ((rc = e->pad.download(d.max_subch))) return rc;
  if ((rc = e->mot.download(d.max_subch))) return rc;
  if ((rc = e->car.download(d.max_subch))) return rc;
  if ((rc = e->dat.download(d.max_subch))) return rc;
  if ((rc = e->mpa.download(d.max_subch))) return rc;
  if ((rc = e->aac.download(d.max_subch))) return rc;
  int max_kbps = e->max_kbps;
  std::vector<SubchDev> row(std::max(1, d.max_subch));
  for (int j = 0; j < n; j++) {
    const dabx_subch_desc &q = desc[j];
    SubchDev sc{};
    if (q.kbps == 0) { row[j] = sc; continue; }            // empty slot (keeps the indices of the others stable)
    const uint16_t *map = nullptr;
    int n_in = 0;
    if ((rc = get_profile_map(q.kbps, q.prot_level, q.short_form, &map, &n_in))) return rc;
    if (q.cu_size * 64 < n_in || q.cu_start < 0 || q.cu_start + q.cu_size > 864) {
      set_error("sub-channel %d: %d CU at %d do not hold %d coded bits", j, q.cu_size, q.cu_start, n_in);
      return DABX_E_PROFILE;
    }
    // the DAB+ stage (k_dabplus) holds a super frame of at most 384 kbit/s (RS interleaving depth kbps / 8 <= 48) in LDS;
    // ETSI TS 102 563 defines DAB+ sub-channels in multiples of 8 kbit/s only
    if (q.dab_plus && (q.kbps > 384 || q.kbps % 8 != 0)) {
      set_error("sub-channel %d: %d kbit/s is not a DAB+ rate (multiples of 8 up to 384); configure it with dab_plus = 0", j, q.kbps);
      return DABX_E_PROFILE;
    }
    sc.cu_start = q.cu_start; sc.cu_size = q.cu_size; sc.kbps = q.kbps; sc.prot_level = q.prot_level;
    sc.short_form = q.short_form; sc.dab_plus = q.dab_plus; sc.nbits = 24 * q.kbps; sc.active = 1; sc.map = map;
    row[j] = sc;
    max_kbps = std::max(max_kbps, q.kbps);
  }
  // When the largest bit rate grows the output rings get wider slots.  Running services are not disturbed
  // (MscHandler::set_channel only adds a Backend, msc_handler.cpp:95-131): the rings are re-strided with their contents,
  // every counter and ring index stays valid, the superseded buffers are freed.
  if (max_kbps > e->max_kbps) {
    // new buffers first; pointers, strides and max_kbps change only after all three exist and the contents are moved, so a
    // failed allocation leaves the engine exactly as it was
    const int new_msc = 3 * max_kbps, new_sf = ((110 * max_kbps / 8) + 15) & ~15;
    const int new_vit = (int)std::max(vit_scratch_words(FIC_OUT), vit_scratch_words(24 * max_kbps));
    const size_t msc_rows = (size_t)d.n_streams * d.max_subch * MSC_SLOTS, sf_rows = (size_t)d.n_streams * d.max_subch * SF_SLOTS;
    uint8_t *n_msc = nullptr, *n_sf = nullptr;
    uint32_t *n_scratch = nullptr;
    auto drop = [&](void *q) { if (q) { (void)hipFree(q); e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), q), e->allocs.end()); } };
    if ((rc = e->alloc(&n_msc, msc_rows * new_msc)) || (rc = e->alloc(&n_sf, sf_rows * new_sf)) ||
        (rc = e->alloc(&n_scratch, (size_t)d.n_streams * (4 + 4 * MSC_BATCH_FRAMES * d.max_subch) * new_vit, false))) {
      drop(n_msc); drop(n_sf); drop(n_scratch);
      return rc;
    }
    hipError_t herr = hipSuccess;
    if (d.msc_out && d.msc_stride > 0)
      herr = hipMemcpy2DAsync(n_msc, new_msc, d.msc_out, d.msc_stride, d.msc_stride, msc_rows, hipMemcpyDeviceToDevice, e->stream);
    if (herr == hipSuccess && d.sf_out && d.sf_stride > 0)
      herr = hipMemcpy2DAsync(n_sf, new_sf, d.sf_out, d.sf_stride, d.sf_stride, sf_rows, hipMemcpyDeviceToDevice, e->stream);
    if (herr == hipSuccess) herr = hipStreamSynchronize(e->stream);
    if (herr != hipSuccess) {
      drop(n_msc); drop(n_sf); drop(n_scratch);
      set_error("dabx_set_subchannels: HIP error %d (%s) while re-striding the output rings", (int)herr, hipGetErrorString(herr));
      return DABX_E_HIP;
    }
    drop(d.msc_out); drop(d.sf_out); drop(d.vit_scratch);
    d.msc_out = n_msc; d.sf_out = n_sf; d.vit_scratch = n_scratch;
    d.msc_stride = new_msc; d.sf_stride = new_sf; d.vit_stride = new_vit;
    e->max_kbps = max_kbps;
  }
  std::vector<size_t> restarted;
  for (int s = 0; s < d.n_streams; s++) {
    if (stream >= 0 && s != stream) continue;
    for (int j = 0; j < d.max_subch; j++) {
      SubchDev sc = j < n ? row[j] : SubchDev{};
      sc.start_cif = at_cif >= 0 ? at_cif : ctl[s].cif_no;
      // a slot whose description does not change keeps running (MscHandler::set_channel only adds a Backend,
      // msc_handler.cpp:95-131): its de-interleaver history, super-frame state and counters stay
      const SubchDev &old = e->subch_host[(size_t)s * d.max_subch + j];
      const bool same = old.active && sc.active && old.cu_start == sc.cu_start && old.cu_size == sc.cu_size &&
                        old.kbps == sc.kbps && old.prot_level == sc.prot_level && old.short_form == sc.short_form &&
                        old.dab_plus == sc.dab_plus && e->subch_id_host[(size_t)s * d.max_subch + j] == desc[j].subch_id;
      if (same) continue;
      // A sub-channel that only MOVES (same SubChId, size, bit rate, protection; other capacity units -- a multiplex reconfiguration):
      // the slot keeps running, its de-interleaver reads the CIFs before the change at the old address (what a Backend that is handed
      // its slice from another place does, msc_handler.cpp:161-166).  One move per 16 CIFs; anything faster restarts the slot.
      const bool moved = old.active && sc.active && old.cu_start != sc.cu_start && old.cu_size == sc.cu_size && old.kbps == sc.kbps &&
                         old.prot_level == sc.prot_level && old.short_form == sc.short_form && old.dab_plus == sc.dab_plus &&
                         e->subch_id_host[(size_t)s * d.max_subch + j] == desc[j].subch_id && sc.start_cif >= old.move_cif + 16;
      if (moved) {
        SubchDev keep = old;
        keep.prev_cu_start = old.cu_start; keep.cu_start = sc.cu_start; keep.move_cif = sc.start_cif;
        e->subch_host[(size_t)s * d.max_subch + j] = keep;
        continue;
      }
      e->subch_host[(size_t)s * d.max_subch + j] = sc;
      e->subch_id_host[(size_t)s * d.max_subch + j] = (j < n && sc.active) ? desc[j].subch_id : -1;
      e->eti[s] = dabx_engine::EtiCursor{};
      restarted.push_back((size_t)s * d.max_subch + j);
    }
  }
  DABX_HIP(hipMemcpy(d.subch, e->subch_host.data(), sizeof(SubchDev) * e->subch_host.size(), hipMemcpyHostToDevice));
  if (!e->pkt.host.empty()) {           // a new or changed slot loses its packet mode; one that keeps running (a move included) keeps it and its state
    for (size_t sj : restarted) e->pkt.drop(sj);
    if ((rc = e->pkt.upload())) return rc;
  }
  if (!e->car.host.empty()) {           // ... and the carousel decoding behind it
    for (size_t sj : restarted) e->car.drop(sj);
    if ((rc = carousel_follow_packet(e))) return rc;
  }
  if (!e->dat.host.empty()) {           // ... and the data handler behind it, in the same way
    for (size_t sj : restarted) e->dat.drop(sj);
    if ((rc = data_follow_packet(e))) return rc;
  }
  if (!e->pad.host.empty()) {           // ... and so does PAD decoding
    for (size_t sj : restarted) e->pad.drop(sj);
    if ((rc = e->pad.upload())) return rc;
    pad_count_sources(e);
  }
  if (!e->mot.host.empty()) {           // ... and the MOT decoding behind it
    for (size_t sj : restarted) e->mot.drop(sj);
    if ((rc = mot_follow_pad(e))) return rc;
  }
  if (!e->mpa.host.empty()) {           // ... and MP2 audio decoding, as PAD decoding
    for (size_t sj : restarted) e->mpa.drop(sj);
    if ((rc = e->mpa.upload())) return rc;
  }
  if (!e->aac.host.empty()) {           // ... and the LOAS framing, as PAD decoding
    for (size_t sj : restarted) e->aac.drop(sj);
    if ((rc = e->aac.upload())) return rc;
  }
  if (e->dl.open) {
    // slots that start anew count their frames from 0 again; the slab layout follows the new sub-channels (engine drained above)
    const long long zero = 0;
    for (size_t sj : restarted) {
      DABX_HIP(hipMemcpy(e->dl.cif_done + sj, &zero, sizeof(zero), hipMemcpyHostToDevice));
      DABX_HIP(hipMemcpy(e->dl.sf_done + sj, &zero, sizeof(zero), hipMemcpyHostToDevice));
      if (e->dl.eti()) {           // ... and the ETI stage forgets the stream's counter, as dabx_read_eti's cursor does above
        const int32_t unknown[2] = {-1, -1};
        DABX_HIP(hipMemcpy(&e->dl.eti_front[sj / (size_t)d.max_subch].hi, unknown, sizeof(unknown), hipMemcpyHostToDevice));
      }
    }
    if ((rc = e->delivery_layout())) {             // the new sub-channels do not fit the slabs: no gather may run with a stale layout
      const std::string why = dabx::last_error();
      delivery_free(e);
      set_error("%s -- the delivery has been closed", why.c_str());
      return rc;
    }
  }
  e->have_fast = false;
  e->classes_dirty = true;            // the decoder classes are rebuilt by the next dabx_process (one rebuild for a series of per-stream calls)
  return 0;
}

int dabx_set_subchannels(dabx_engine *e, int stream, const dabx_subch_desc *desc, int n) { return set_subchannels_impl(e, stream, desc, n, -1); }
int dabx_set_subchannels_at(dabx_engine *e, int stream, const dabx_subch_desc *desc, int n, int64_t at_cif)
{
  if (at_cif < 0 || stream < 0) { set_error("dabx_set_subchannels_at: bad argument"); return DABX_E_ARG; }
  return set_subchannels_impl(e, stream, desc, n, at_cif);
}

int dabx_iq_ring_dev(dabx_engine *e, int stream, void **ring, size_t *cap)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !ring) return DABX_E_ARG;
  *ring = e->ring_of(stream);
  if (cap) *cap = (size_t)e->dev.ring_len;
  return 0;
}

}  // extern "C"

namespace dabx {

// What a push may overwrite is announced BEFORE its copy is issued (EngineDev::wr_horizon, host memory the device reads): the level
// tracker's re-walk from its anchor (k_acquire) only trusts samples at or above horizon - ring_len, and looks again after the walk.
void announce_write(dabx_engine *e, int stream, unsigned long long upto)
{
  if (!e->horizon_host) return;
  for (int s = 0; s < e->dev.n_streams; s++)
    if ((stream < 0 || s == stream) && e->horizon_host[s] < upto) __atomic_store_n(&e->horizon_host[s], upto, __ATOMIC_RELEASE);
}

int commit_impl(dabx_engine *e, int stream, size_t n)
{
  if (!e || stream >= e->dev.n_streams) return DABX_E_ARG;
  if (int rc = use_device(e)) return rc;
  for (int s = 0; s < e->dev.n_streams; s++)
    if (stream < 0 || s == stream) e->wr_host[s] += n;
  if (int rc = launch_commit(e->dev, stream, n, e->stream)) return rc;
  // SampleReader's DC / IQ correction (off by default): the new samples are corrected in place before anything reads them
  if (e->cfg.dc_iq_correction) return launch_dciq(e->dev, e->cfg.dc_iq_correction, e->stream);
  return 0;
}

// never overwrite samples the receiver has not read yet.  rd only grows, so the value seen at the last look is a safe
// bound: the pipeline is drained (and rd read again) only when that bound says the ring is full
int push_room(dabx_engine *e, int stream, size_t n, const char *who)
{
  for (int attempt = 0; e->wr_host[stream] - e->rd_seen[stream] + n > (unsigned long long)e->dev.ring_len; attempt++) {
    if (attempt == 2) {
      set_error("%s: ring of stream %d has room for %llu samples, %zu offered (call dabx_process first)", who, stream,
                (unsigned long long)e->dev.ring_len - (e->wr_host[stream] - e->rd_seen[stream]), n);
      return DABX_E_STATE;
    }
    // first a look at the counters while the receiver keeps running (any value read is a valid lower bound), then,
    // if that is not enough, with the pipeline drained
    if (attempt == 1) { if (int rc0 = sync_all(e)) return rc0; }
    e->ctl_peek.resize(e->dev.n_streams);
    DABX_HIP(hipMemcpy(e->ctl_peek.data(), e->dev.ctl, sizeof(StreamCtl) * e->dev.n_streams, hipMemcpyDeviceToHost));
    if (e->dev.exact_level && e->dev.level_pos) {          // the exact level tracker still has to read what lies behind ITS cursor
      std::vector<unsigned long long> lp(e->dev.n_streams);
      DABX_HIP(hipMemcpy(lp.data(), e->dev.level_pos, sizeof(unsigned long long) * lp.size(), hipMemcpyDeviceToHost));
      for (int s = 0; s < e->dev.n_streams; s++) e->ctl_peek[s].rd = std::min(e->ctl_peek[s].rd, lp[s]);
    }
    for (int s = 0; s < e->dev.n_streams; s++) e->rd_seen[s] = std::max(e->rd_seen[s], e->ctl_peek[s].rd);
  }
  return 0;
}

}  // namespace dabx

extern "C" {

int dabx_commit_iq(dabx_engine *e, int stream, size_t n)
{
  if (!e || stream >= e->dev.n_streams) return DABX_E_ARG;
  // a zero-copy producer writes into the ring on its own: unless it has said how far (dabx_announce_write), nothing behind the read
  // cursor can be taken for intact from here on
  if (e->horizon_host)
    for (int s = 0; s < e->dev.n_streams; s++)
      if ((stream < 0 || s == stream) && !e->announcing[s]) __atomic_store_n(&e->horizon_host[s], ~0ull, __ATOMIC_RELEASE);
  return commit_impl(e, stream, n);
}
int dabx_announce_write(dabx_engine *e, int stream, size_t n)
{
  if (!e || stream >= e->dev.n_streams) { set_error("dabx_announce_write: bad argument"); return DABX_E_ARG; }
  if (!e->horizon_host) return 0;
  for (int s = 0; s < e->dev.n_streams; s++)
    if (stream < 0 || s == stream) {
      // from its first announcement on the producer is taken at its word: commits no longer mean "unknown writes" (a ring that is
      // filled once and only read again -- periodic test signals -- is announced once)
      const unsigned long long prev = e->announcing[s] ? e->horizon_host[s] : 0ull;
      e->announcing[s] = 1;
      __atomic_store_n(&e->horizon_host[s], std::max(prev, e->wr_host[s] + (unsigned long long)n), __ATOMIC_RELEASE);
    }
  return 0;
}
// iqfile.cpp: samples it converted into the ring itself, while nothing was running (dabx_internal_ring_info drains the engine)
int dabx_internal_commit(dabx_engine *e, int stream, size_t n)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams) return DABX_E_ARG;
  announce_write(e, stream, e->wr_host[stream] + n);
  return commit_impl(e, stream, n);
}

// Both pushes: copy + conversion on an ingest stream, next to whatever the receiver streams are computing: the samples land beyond the
// committed write index, which no queued kernel reads; only the commit is ordered into the front-end stream.
//   synchronous   the engine's one staging buffer (grown on demand), and the call waits: the caller's buffer is free again.
//   async         a small pool of device staging slots, each guarded by the event of its last conversion kernel, on two streams in turn
static int push_impl(dabx_engine *e, int stream, const void *iq, int fmt, size_t n, bool async, const char *who)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !iq || fmt < 0 || fmt > 2 || n > (size_t)e->dev.ring_len) {
    set_error("%s: bad argument", who);
    return DABX_E_ARG;
  }
  if (int rc = ring_takes(e, fmt, who)) return rc;
  if (n == 0) return 0;
  if (int rc = use_device(e)) return rc;
  if (int rc = push_room(e, stream, n, who)) return rc;
  IqJob j{};
  if (int rc = iq_push_decode(fmt, e->dev.ring_fmt, &j.dec)) return rc;
  const size_t bytes = n * (size_t)(2 * j.dec.bytes);
  void **buf = &e->stage; size_t *cap = &e->stage_cap; hipEvent_t *done = &e->ingest_done; hipStream_t st = e->ingest;
  if (async) {
    const int k = (int)(e->async_pushes++ % dabx_engine::ASYNC_SLOTS);
    buf = &e->aslot[k]; cap = &e->aslot_cap[k]; done = &e->aslot_done[k];
    if (!*done) DABX_HIP(hipEventCreateWithFlags(done, hipEventDisableTiming));
    else DABX_HIP(hipEventSynchronize(*done));                         // the slot's previous conversion has read it
    if (!e->ingest2) DABX_HIP(hipStreamCreateWithFlags(&e->ingest2, hipStreamNonBlocking));
    if (k & 1) st = e->ingest2;
  }
  if (bytes > *cap) {
    if (*buf) DABX_HIP(hipFree(*buf));
    *buf = nullptr; *cap = 0;
    DABX_HIP(hipMalloc(buf, bytes));
    *cap = bytes;
  }
  announce_write(e, stream, e->wr_host[stream] + n);
  DABX_HIP(hipMemcpyAsync(*buf, iq, bytes, hipMemcpyHostToDevice, st));
  IqIo io{};
  io.src = static_cast<const uint8_t *>(*buf); io.dst = e->ring_of(stream); io.dst_len = e->dev.ring_len;
  j.n = (unsigned)n; j.dst0 = e->wr_host[stream];
  if (int rc = launch_iq_job(io, j, st)) return rc;
  DABX_HIP(hipEventRecord(*done, st));
  DABX_HIP(hipStreamWaitEvent(e->stream, *done, 0));                   // the commit (and every frame after it) sees the samples
  const int rc = commit_impl(e, stream, n);
  if (!async) DABX_HIP(hipStreamSynchronize(st));                      // the caller's buffer and the staging buffer are free again
  return rc;
}
int dabx_push_iq(dabx_engine *e, int stream, const void *iq, int fmt, size_t n) { return push_impl(e, stream, iq, fmt, n, false, "dabx_push_iq"); }
// The same without waiting for the copy: for producers that keep their buffers alive and unchanged until dabx_push_wait --
// a file reader cycling through a few pinned buffers (hipHostMalloc / dabx_host_register).  From pinned memory the copies
// of consecutive calls run back to back as DMA at PCIe rate while the host already issues the next ones; from pageable
// memory the HIP runtime stages the copy itself and the call degrades gracefully to the synchronous behaviour.
int dabx_push_iq_async(dabx_engine *e, int stream, const void *iq, int fmt, size_t n) { return push_impl(e, stream, iq, fmt, n, true, "dabx_push_iq_async"); }

int dabx_push_wait(dabx_engine *e)
{
  if (!e) return DABX_E_ARG;
  if (int rc = use_device(e)) return rc;
  DABX_HIP(hipStreamSynchronize(e->ingest));
  if (e->ingest2) DABX_HIP(hipStreamSynchronize(e->ingest2));
  return 0;
}

// hipHostRegister / hipHostUnregister for a producer's own buffers (page-locks them so that pushes are true DMA)
int dabx_host_register(void *p, size_t bytes)
{
  if (!p || !bytes) return DABX_E_ARG;
  if (int rc = need_device_e()) return rc;
  DABX_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault));
  return 0;
}
int dabx_host_unregister(void *p)
{
  if (!p) return DABX_E_ARG;
  if (int rc = need_device_e()) return rc;
  DABX_HIP(hipHostUnregister(p));
  return 0;
}

int dabx_read_iq(dabx_engine *e, int stream, uint64_t first, size_t n, float *iq_out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !iq_out) return DABX_E_ARG;
  const unsigned long long wr = e->wr_host[stream];
  if (first + n > wr || wr - first > (unsigned long long)e->dev.ring_len) { set_error("dabx_read_iq: samples not in the ring"); return DABX_E_STATE; }
  if (int rc = sync_all(e)) return rc;
  // a native ring: its codes are copied, and become floats here by the very map the kernels apply (ring_fmt.h: exact on host and device)
  const size_t bps = (size_t)ring_bytes_per_sample(e->dev.ring_fmt);
  const char *ring = static_cast<const char *>(e->ring_of(stream));
  std::vector<char> codes(e->dev.ring_fmt == RING_CF32 ? 0 : n * bps);
  char *dst = e->dev.ring_fmt == RING_CF32 ? reinterpret_cast<char *>(iq_out) : codes.data();
  size_t done = 0;
  while (done < n) {
    const size_t o = (size_t)((first + done) % (unsigned long long)e->dev.ring_len);
    const size_t take = std::min(n - done, (size_t)e->dev.ring_len - o);
    DABX_HIP(hipMemcpy(dst + done * bps, ring + o * bps, take * bps, hipMemcpyDeviceToHost));
    done += take;
  }
  float2 *out2 = reinterpret_cast<float2 *>(iq_out);
  if (e->dev.ring_fmt == RING_S16) {
    const uint32_t *c = reinterpret_cast<const uint32_t *>(codes.data());
    for (size_t i = 0; i < n; i++) out2[i] = RingFmt<RING_S16>::cvt(c[i]);
  } else if (e->dev.ring_fmt == RING_U8) {
    const uint16_t *c = reinterpret_cast<const uint16_t *>(codes.data());
    for (size_t i = 0; i < n; i++) out2[i] = RingFmt<RING_U8>::cvt(c[i]);
  }
  return 0;
}

// internal hook of iqfile.cpp (not part of include/dabx.h)
int dabx_internal_ring_info(dabx_engine *e, int stream, float2 **ring, int *ring_len, unsigned long long *wr, unsigned long long *rd, hipStream_t *st)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams) { set_error("bad engine / stream"); return DABX_E_ARG; }
  if (int rc = sync_all(e)) return rc;
  StreamCtl c;
  DABX_HIP(hipMemcpy(&c, e->dev.ctl + stream, sizeof(StreamCtl), hipMemcpyDeviceToHost));
  *ring = static_cast<float2 *>(e->ring_of(stream)); *ring_len = e->dev.ring_len;   // (untyped in a native ring: EngineHead::ring_fmt, IqDecode::ring_fmt)
  *wr = e->wr_host[stream]; *rd = c.rd; *st = e->stream;
  return 0;
}

int dabx_process(dabx_engine *e, int max_frames, int sync)
{
  if (!e || max_frames < 0) return DABX_E_ARG;
  if (int rc = use_device(e)) return rc;
  // The front end (sync, FFT, demap, FIC) has frame-to-frame feedback and runs once per frame; the MSC decoder
  // has none, so its CIFs are decoded MSC_BATCH_FRAMES frames at a time (more trellises per launch) and always
  // before this call returns.
  if (e->classes_dirty) {
    if (int rc = e->build_msc_classes()) return rc;
    e->classes_dirty = false;
  }
  // Streams out of lock are searched next to the steps, on their own HIP stream (k_acquire on q): a step of the streams in lock never waits
  // for a stream in a drop-out -- with sync != 0 too: the call then waits for the frame chain it issued, not for the search pass beside it
  // (a pass costs ~2 ms, two steps of 512 streams).  cfg.acquire_mode 1 / 2 fixes either form.
  // (With cfg.dc_iq_correction the committed samples are corrected in place on the front-end stream before anything reads them:
  // a search running next to that stream could read them uncorrected, so it stays in step.)
  // And while fewer than half of the streams are in lock (start-up of a whole engine; the device keeps the count in host memory, read
  // here without a wait) the search runs in step: there is little to hold up, and streams that start together lock together instead of
  // falling behind their producers while nearly empty steps go by.  (A stream that joins late stays late: a step never advances a
  // stream by more than one frame.)
  if (e->dl.open && max_frames > 0) {
    // every chunk this call closes needs a free host slab; checked before anything is launched, so that a refused call changes nothing
    const int need = (e->pending_frames + max_frames + MSC_BATCH_FRAMES - 1) / MSC_BATCH_FRAMES;
    int free_slots = 0;
    {
      std::lock_guard<std::mutex> lk(e->dl.mu);
      for (const auto &sl : e->dl.slots) free_slots += sl.state == Delivery::FREE;
    }
    if (free_slots < need) {
      set_error("dabx_process: the call closes %d chunks, %d host slabs are free (dabx_delivery_next / dabx_delivery_release)", need, free_slots);
      return DABX_E_STATE;
    }
  }
  const bool some_locked = !e->locked_host || 2 * __atomic_load_n(e->locked_host, __ATOMIC_RELAXED) >= e->dev.n_streams;
  // (And while a stream has the correlation plot on -- dabx_set_cir_mode -- it stays in step as well: a search beside the step could hand a
  // stream to the frame head between k_cir_corr and the head, and the plot would miss a call that the head made.)
  // (... and while a stream has the spectrum on -- dabx_set_spectrum_mode: k_spectrum reads, behind the head, where the search has left the stream)
  const bool async_acquire = !e->cfg.dc_iq_correction && e->cir.n_corr == 0 && e->spectrum.n_on == 0 && (e->cfg.acquire_mode == 2 || (e->cfg.acquire_mode == 0 && some_locked));
  for (int i = 0; i < max_frames; i++) {
    // the 5th frame after a batch starts rewriting time-de-interleaver slots the previous batch's k_msc_prep (stream b) reads
    if (e->ss.prep_pending && e->pending_frames >= 4) {
      DABX_HIP(hipStreamWaitEvent(e->stream, e->ss.prep_b_done, 0));
      e->ss.prep_pending = false;
    }
    const bool all_locked = e->locked_host && __atomic_load_n(e->locked_host, __ATOMIC_RELAXED) == e->dev.n_streams;
    // (the scope stage's k_scope goes in front of the frame's first demapper launch, only while a stream has the mode on)
    // (the CIR stage's kernels go in front of the frame head, only while a stream has the mode on and a row is due or a plot is on)
    const int cir_cap = e->cir.n_on > 0 ? cir_step_cap(e, false) : 0;
    int rc = launch_front_step(e->dev, e->ss, e->mk, async_acquire, all_locked, e->scope.n_on > 0 ? &e->scope.dev : nullptr,
                               e->cir.n_on > 0 ? &e->cir.dev : nullptr, cir_cap, e->spectrum.n_on > 0 ? &e->spectrum.dev : nullptr);
    if (rc) return rc;
    if (cir_cap > 0) cir_step_cap(e, true);                // the step is launched: the host's count of rows done follows k_cir_finish's
    if (e->cir.n_on > 0 && (cir_cap > 0 || e->cir.n_corr > 0)) e->cir.launches++;
    if (e->scope.n_on > 0) e->scope.launches++;
    if (e->spectrum.n_on > 0) e->spectrum.launches++;
    // the TII detectors of the streams that have the mode on (deliver.hip): behind the frame tail, in front of the next frame's accumulation
    if (e->tiis.n_on > 0) {
      if ((rc = launch_tii(e->dev, e->tiis.dev, e->stream))) return rc;
      e->tiis.launches++;
    }
    // the FIG walk of the streams that have the mode on (deliver.hip): behind the frame's FIC decoder and its count, in front of the next frame's
    if ((rc = fig_step(e))) return rc;
    e->level_dirty = true;
    if (++e->pending_frames == MSC_BATCH_FRAMES || i == max_frames - 1) {
      DeliverDev dv{};
      int dl_slot = -1, dl_dev = -1;
      if (e->dl.open && (rc = e->delivery_begin(&dv, &dl_slot, &dl_dev))) return rc;
      e->dev.snap = e->snap_buf[e->ss.batch_parity];
      hipStream_t tail = e->stream;
      const bool with_eti = e->dl.open && e->dl.eti();
      const EtiDev eti = with_eti ? e->dl.eti_dev(dl_dev) : EtiDev{};
      rc = launch_msc_batch(e->dev, 4 * e->pending_frames, e->have_fast ? &e->fast : nullptr, e->ss, e->mk, e->dl.open ? &dv : nullptr, &tail,
                            e->pkt.dev.n > 0 ? &e->pkt.dev : nullptr, e->pad.dev.n > 0 ? &e->pad.dev : nullptr, e->mot.dev.n > 0 ? &e->mot.dev : nullptr,
                            e->car.dev.n > 0 ? &e->car.dev : nullptr, with_eti ? &eti : nullptr, e->mpa.dev.n > 0 ? &e->mpa.dev : nullptr, &e->mpa_launches,
                            e->aac.dev.n > 0 ? &e->aac.dev : nullptr, &e->aac_launches, e->dat.dev.n > 0 ? &e->dat.dev : nullptr, &e->dat_ctl);
      if (rc) {
        if (e->dl.open) e->delivery_abort(dl_slot, dl_dev);          // the slabs of the chunk that was begun: never left IN_FLIGHT without a copy job
        e->pending_frames = 0;
        return rc;
      }
      if (e->dl.open && (rc = e->delivery_finish(dl_slot, dl_dev, tail))) return rc;
      e->pending_frames = 0;
    }
  }
  if (sync && (max_frames = sync_all(e, async_acquire) ? -1 : max_frames) < 0) return DABX_E_HIP;
  return max_frames;
}

int dabx_synchronize(dabx_engine *e)
{
  if (!e) return DABX_E_ARG;
  return sync_all(e);
}
void *dabx_hip_stream(dabx_engine *e) { return e ? (void *)e->stream : nullptr; }

static int fetch_ctl(dabx_engine *e, int stream, StreamCtl *c)
{
  if (int rc = sync_all(e)) return rc;
  DABX_HIP(hipMemcpy(c, e->dev.ctl + stream, sizeof(StreamCtl), hipMemcpyDeviceToHost));
  return 0;
}

int dabx_read_fibs(dabx_engine *e, int stream, int n_frames, uint8_t *fibs, uint8_t *crc)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || n_frames <= 0 || n_frames > e->dev.out_frames || !fibs || !crc) return DABX_E_ARG;
  StreamCtl c;
  int rc = fetch_ctl(e, stream, &c);
  if (rc) return rc;
  const int have = (int)std::min<long long>(c.frames, n_frames);
  for (int i = 0; i < have; i++) {            // oldest first
    const long long fr = c.frames - have + i;
    const int slot = (int)(fr % e->dev.out_frames);
    DABX_HIP(hipMemcpy(fibs + (size_t)i * 384, e->dev.fib_out + ((size_t)stream * e->dev.out_frames + slot) * 384, 384, hipMemcpyDeviceToHost));
    DABX_HIP(hipMemcpy(crc + (size_t)i * 12, e->dev.fib_crc + ((size_t)stream * e->dev.out_frames + slot) * 12, 12, hipMemcpyDeviceToHost));
  }
  return have;
}

int dabx_read_frame_info(dabx_engine *e, int stream, int n_frames, int64_t *sym0_pos, int32_t *start_index)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || n_frames <= 0 || n_frames > e->dev.out_frames || (!sym0_pos && !start_index)) return DABX_E_ARG;
  if (!e->dev.frame_pos) { set_error("dabx_read_frame_info: engine keeps no frame records"); return DABX_E_STATE; }
  StreamCtl c;
  int rc = fetch_ctl(e, stream, &c);
  if (rc) return rc;
  const int have = (int)std::min<long long>(c.frames, n_frames);
  for (int i = 0; i < have; i++) {            // oldest first
    const long long fr = c.frames - have + i;
    const size_t slot = (size_t)stream * e->dev.out_frames + (size_t)(fr % e->dev.out_frames);
    if (sym0_pos) DABX_HIP(hipMemcpy(sym0_pos + i, e->dev.frame_pos + slot, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (start_index) DABX_HIP(hipMemcpy(start_index + i, e->dev.frame_start + slot, sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return have;
}

static int fetch_subch(dabx_engine *e, int stream, int j, SubchDev *sc)
{
  if (int rc = sync_all(e)) return rc;
  DABX_HIP(hipMemcpy(sc, e->dev.subch + (size_t)stream * e->dev.max_subch + j, sizeof(SubchDev), hipMemcpyDeviceToHost));
  return 0;
}

int dabx_read_msc(dabx_engine *e, int stream, int j, int n_cifs, uint8_t *bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n_cifs <= 0 || n_cifs > MSC_SLOTS || !bytes) return DABX_E_ARG;
  SubchDev sc;
  int rc = fetch_subch(e, stream, j, &sc);
  if (rc) return rc;
  if (!sc.active) return 0;
  const int have = (int)std::min<long long>(sc.cif_out, n_cifs), nb = 3 * sc.kbps;
  for (int i = 0; i < have; i++) {
    const long long q = sc.cif_out - have + i;
    DABX_HIP(hipMemcpy(bytes + (size_t)i * nb,
                       e->dev.msc_out + (((size_t)stream * e->dev.max_subch + j) * MSC_SLOTS + (size_t)(q % MSC_SLOTS)) * e->dev.msc_stride,
                       nb, hipMemcpyDeviceToHost));
  }
  return have;
}

int dabx_read_superframes(dabx_engine *e, int stream, int j, int n, uint8_t *bytes)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || n > SF_SLOTS || !bytes) return DABX_E_ARG;
  SubchDev sc;
  int rc = fetch_subch(e, stream, j, &sc);
  if (rc) return rc;
  if (!sc.active) return 0;
  const int have = (int)std::min<long long>(sc.sf_count, n), nb = 110 * sc.kbps / 8;
  for (int i = 0; i < have; i++) {
    const long long q = sc.sf_count - have + i;
    DABX_HIP(hipMemcpy(bytes + (size_t)i * nb,
                       e->dev.sf_out + (((size_t)stream * e->dev.max_subch + j) * SF_SLOTS + (size_t)(q % SF_SLOTS)) * e->dev.sf_stride,
                       nb, hipMemcpyDeviceToHost));
  }
  return have;
}

int dabx_read_superframe_info(dabx_engine *e, int stream, int j, int n, dabx_superframe_info *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || n <= 0 || n > SF_SLOTS || !out) return DABX_E_ARG;
  SubchDev sc;
  int rc = fetch_subch(e, stream, j, &sc);
  if (rc) return rc;
  if (!sc.active || !e->dev.sf_info) return 0;
  const int have = (int)std::min<long long>(sc.sf_count, n);
  std::vector<dabx_superframe_info> ring(SF_SLOTS);
  DABX_HIP(hipMemcpy(ring.data(), e->dev.sf_info + ((size_t)stream * e->dev.max_subch + j) * SF_SLOTS, sizeof(dabx_superframe_info) * SF_SLOTS,
                     hipMemcpyDeviceToHost));
  for (int i = 0; i < have; i++) out[i] = ring[(size_t)((sc.sf_count - have + i) % SF_SLOTS)];
  return have;
}

int dabx_read_eti(dabx_engine *e, int stream, int max_frames, uint8_t *out, int32_t *lost_cifs)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || max_frames < 0 || (!out && max_frames)) return DABX_E_ARG;
  if (lost_cifs) *lost_cifs = 0;
  if (e->dev.fic_only) { set_error("dabx_read_eti: engine was created FIC-only"); return DABX_E_STATE; }
  StreamCtl c;
  int rc = fetch_ctl(e, stream, &c);
  if (rc) return rc;
  const EngineDev &d = e->dev;
  std::vector<SubchDev> row(std::max(1, d.max_subch));
  DABX_HIP(hipMemcpy(row.data(), d.subch + (size_t)stream * d.max_subch, sizeof(SubchDev) * d.max_subch, hipMemcpyDeviceToHost));
  std::vector<int> act;
  for (int j = 0; j < d.max_subch; j++) if (row[j].active) act.push_back(j);
  // CIFs [lo_cif, hi_cif) are complete in both rings
  long long hi_cif = act.empty() ? c.cif_no : c.msc_done_cif, lo_cif = std::max(0ll, (c.frames - d.out_frames) * 4);
  for (int j : act) lo_cif = std::max(lo_cif, msc_first_cif(row[j].start_cif) + std::max(0ll, row[j].cif_out - MSC_SLOTS));   // the oldest logical frame still in the ring
  dabx_engine::EtiCursor &cur = e->eti[stream];
  if (cur.next_cif < 0) { cur.next_cif = lo_cif; cur.fib_frames_seen = lo_cif / 4; }
  if (cur.next_cif < lo_cif) {
    if (lost_cifs) *lost_cifs = (int32_t)(lo_cif - cur.next_cif);
    cur.next_cif = lo_cif;
  }
  cur.fib_frames_seen = std::max(cur.fib_frames_seen, std::max(0ll, c.frames - d.out_frames));
  int n = 0;
  std::vector<uint8_t> fibs(384), msc((size_t)act.size() * std::max(1, d.msc_stride));
  std::vector<dabx_subch_desc> desc(act.size());
  std::vector<const uint8_t *> ptr(act.size());
  for (size_t a = 0; a < act.size(); a++) {
    const SubchDev &sc = row[act[a]];
    desc[a] = dabx_subch_desc{e->subch_id_host[(size_t)stream * d.max_subch + act[a]], sc.cu_start, sc.cu_size, sc.kbps, sc.prot_level, sc.short_form, sc.dab_plus, 0};
    ptr[a] = msc.data() + a * (size_t)d.msc_stride;
  }
  long long fib_frame = -1;
  while (n < max_frames && cur.next_cif < hi_cif) {
    const long long r = cur.next_cif, F = r / 4;
    // FibDecoder state at symbol 4 of frame F: every FIB up to and including this frame's 12 has been parsed
    while (cur.fib_frames_seen <= F) {
      const long long G = cur.fib_frames_seen;
      std::vector<uint8_t> fb(384), fc(12);
      const size_t slot = (size_t)stream * d.out_frames + (size_t)(G % d.out_frames);
      DABX_HIP(hipMemcpy(fb.data(), d.fib_out + slot * 384, 384, hipMemcpyDeviceToHost));
      DABX_HIP(hipMemcpy(fc.data(), d.fib_crc + slot * 12, 12, hipMemcpyDeviceToHost));
      for (int i = 0; i < 12; i++) if (fc[i]) fib_fig00_counter(fb.data() + 32 * i, &cur.hi, &cur.lo);   // k_fic_frame's own walk: == dabx_stats.cif_count
      if (G == F) { fibs = fb; fib_frame = F; }
      cur.fib_frames_seen++;
    }
    if (fib_frame != F) {
      const size_t slot = (size_t)stream * d.out_frames + (size_t)(F % d.out_frames);
      DABX_HIP(hipMemcpy(fibs.data(), d.fib_out + slot * 384, 384, hipMemcpyDeviceToHost));
      fib_frame = F;
    }
    cur.next_cif++;
    if (cur.hi < 0 || cur.lo < 0) continue;              // eti_generator.cpp:156-160: no FIG 0/0 yet
    for (size_t a = 0; a < act.size(); a++) {
      const SubchDev &sc = row[act[a]];
      desc[a].cu_start = r < sc.move_cif ? sc.prev_cu_start : sc.cu_start;     // a sub-channel that moved: the address the FIC of CIF r gave it
      const long long lf = r - sc.start_cif - 16;
      DABX_HIP(hipMemcpy(msc.data() + a * (size_t)d.msc_stride,
                         d.msc_out + (((size_t)stream * d.max_subch + act[a]) * MSC_SLOTS + (size_t)(lf % MSC_SLOTS)) * d.msc_stride,
                         (size_t)3 * sc.kbps, hipMemcpyDeviceToHost));
    }
    rc = dabx_eti_frame(cur.hi, cur.lo, (int)(r & 3), desc.data(), (int)desc.size(), fibs.data() + 96 * (r & 3), ptr.data(), out + (size_t)n * 6144);
    if (rc < 0) return rc;
    n++;
  }
  return n;
}

int dabx_read_tii(dabx_engine *e, int stream, int min_frames, int threshold_db, int collisions, int collision_sub_id,
                  dabx_tii_result *out, int max_out, int32_t *frames_accumulated)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || (!out && max_out > 0) || max_out < 0) return DABX_E_ARG;
  if (!e->dev.tii_acc) { set_error("dabx_read_tii: engine has no TII accumulator"); return DABX_E_STATE; }
  if (e->tiis.exists() && e->tiis.cfg[(size_t)stream].enable) {
    set_error("dabx_read_tii: stream %d runs its detector on the device (dabx_set_tii_mode), which owns the sum: dabx_read_tii_events", stream);
    return DABX_E_STATE;
  }
  if (int rc = sync_all(e)) return rc;
  int32_t cnt[2];
  DABX_HIP(hipMemcpy(cnt, e->dev.tii_cnt + 2 * stream, sizeof(cnt), hipMemcpyDeviceToHost));
  if (frames_accumulated) *frames_accumulated = cnt[0];
  dabx_tii *&t = e->tii[(size_t)stream];
  if (!t) { if (int rc = dabx_tii_create(&t)) return rc; e->tii_epoch[(size_t)stream] = cnt[1]; }
  if (cnt[1] != e->tii_epoch[(size_t)stream]) { dabx_tii_reset(t); e->tii_epoch[(size_t)stream] = cnt[1]; }   // lock was lost meanwhile
  if (cnt[0] < std::max(1, min_frames)) return 0;
  std::vector<float> acc(2 * (size_t)TU);
  DABX_HIP(hipMemcpy(acc.data(), e->dev.tii_acc + (size_t)stream * TU, sizeof(float2) * TU, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemset(e->dev.tii_acc + (size_t)stream * TU, 0, sizeof(float2) * TU));
  DABX_HIP(hipMemset(e->dev.tii_cnt + 2 * stream, 0, sizeof(int32_t)));
  dabx_tii_set_collisions(t, collisions, collision_sub_id);
  dabx_tii_add(t, acc.data());
  return dabx_tii_process(t, threshold_db, out, max_out);
}

int dabx_read_soft(dabx_engine *e, int stream, int16_t *soft)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !soft) return DABX_E_ARG;
  if (!e->dev.soft_cap) { set_error("engine was created without capture_soft"); return DABX_E_STATE; }
  if (int rc = sync_all(e)) return rc;
  DABX_HIP(hipMemcpy(soft, e->dev.soft_cap + (size_t)stream * 75 * K2, sizeof(int16_t) * 75 * K2, hipMemcpyDeviceToHost));
  return 0;
}

int dabx_discover_subchannels(dabx_engine *e, int stream, dabx_subch_desc *out, int max_out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out || max_out <= 0) return DABX_E_ARG;
  const int nf = e->dev.out_frames;
  std::vector<uint8_t> fibs((size_t)nf * 384), crc((size_t)nf * 12);
  const int have = dabx_read_fibs(e, stream, nf, fibs.data(), crc.data());
  if (have < 0) return have;
  return dabx_parse_fibs(fibs.data(), crc.data(), have * 12, out, max_out, nullptr);
}

int dabx_set_fig_reference_quirks(dabx_engine *e, int on)
{
  if (!e) return DABX_E_ARG;
  e->fig_reference_quirks = on != 0;
  for (dabx_fibdec *fd : e->fibdec) if (fd) (void)dabx_fibdec_set_reference_quirks(fd, on);
  return 0;
}

int dabx_follow_fic(dabx_engine *e, int stream, dabx_reconf *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) return DABX_E_ARG;
  memset(out, 0, sizeof(*out));
  out->at_cif = out->last_change_cif = -1;
  if (e->fig.on_for(stream)) {
    set_error("dabx_follow_fic: stream %d follows the FIC on the device (dabx_set_fig_mode): dabx_fig_follow", stream);
    return DABX_E_STATE;
  }
  StreamCtl c;
  int rc = fetch_ctl(e, stream, &c);
  if (rc) return rc;
  dabx_fibdec *&fd = e->fibdec[(size_t)stream];
  if (!fd) {
    if ((rc = dabx_fibdec_create(&fd))) return rc;
    if (e->fig_reference_quirks) (void)dabx_fibdec_set_reference_quirks(fd, 1);
  }
  long long &fed = e->fib_frames_fed[(size_t)stream];
  const EngineDev &d = e->dev;
  if (c.frames - fed > d.out_frames) {                      // frames that have left the FIB ring: their FIGs are lost to the decoder
    out->frames_missed = (int32_t)std::min<long long>(c.frames - fed - d.out_frames, 0x7fffffff);
    fed = c.frames - d.out_frames;
  }
  // FIB k of frame f is FIB 12 f + k of the stream: the decoder counts the FIBs of missed frames as skipped
  dabx_fibdec_info inf;
  dabx_fibdec_get_info(fd, &inf);
  if (inf.fibs_processed < 12 * fed) dabx_internal_fibdec_skip(fd, 12 * fed - inf.fibs_processed);      // counted, not processed
  std::vector<uint8_t> fb(384), fc(12);
  for (; fed < c.frames; fed++) {
    const size_t slot = (size_t)stream * d.out_frames + (size_t)(fed % d.out_frames);
    DABX_HIP(hipMemcpy(fb.data(), d.fib_out + slot * 384, 384, hipMemcpyDeviceToHost));
    DABX_HIP(hipMemcpy(fc.data(), d.fib_crc + slot * 12, 12, hipMemcpyDeviceToHost));
    dabx_fibdec_process(fd, fb.data(), fc.data(), 12);
  }
  dabx_fibdec_get_info(fd, &inf);
  out->frames_fed = fed;
  out->n_changes = inf.n_changes;
  // FIB i of the stream belongs to frame i / 12 and, within its FIC, to the CIF (i % 12) / 3 (three FIBs per CIF in Mode I)
  auto cif_of_fib = [](long long i) { return 4 * (i / 12) + (i % 12) / 3; };
  if (inf.last_change_fib >= 0) out->last_change_cif = cif_of_fib(inf.last_change_fib);
  if (inf.change_flags != 0 && inf.fig00_fib >= 0) {
    out->pending = 1;
    // the announcing FIG 0/0 carried the counter of ITS CIF: the change applies (occurrence - lo) mod 250 CIFs later.  While the flags
    // are set the change has not happened yet: a distance of 0 is a full turn of the low counter (250 CIFs = the 6 s of lead)
    int ahead = ((inf.occurrence_change - inf.cif_count_lo) % 250 + 250) % 250;
    if (ahead == 0) ahead = 250;
    out->at_cif = cif_of_fib(inf.fig00_fib) + ahead;
  }
  return 0;
}

int dabx_next_subchannels(dabx_engine *e, int stream, dabx_subch_desc *out, int max_out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out || max_out <= 0) return DABX_E_ARG;
  dabx_fibdec *fd = e->fibdec[(size_t)stream];
  if (!fd) { set_error("dabx_next_subchannels: call dabx_follow_fic first"); return DABX_E_STATE; }
  return dabx_fibdec_subchannels(fd, 1, out, max_out);
}

int dabx_current_subchannels(dabx_engine *e, int stream, dabx_subch_desc *out, int max_out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out || max_out <= 0) return DABX_E_ARG;
  dabx_fibdec *fd = e->fibdec[(size_t)stream];
  if (!fd) { set_error("dabx_current_subchannels: call dabx_follow_fic first"); return DABX_E_STATE; }
  return dabx_fibdec_subchannels(fd, 0, out, max_out);
}

}  // extern "C"

#undef dabx_get_stats
static int get_stats_full(dabx_engine *e, int stream, dabx_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) return DABX_E_ARG;
  StreamCtl c;
  int rc = fetch_ctl(e, stream, &c);
  if (rc) return rc;
  memset(out, 0, sizeof(*out));
  out->level_margin_events = c.level_margin;
  out->level_rewalk_events = c.lvl_rewalks; out->level_unanchored_events = c.lvl_unanchored; out->level_healed_events = c.lvl_healed;
  out->frames = c.frames; out->samples_consumed = (int64_t)c.rd; out->state = c.state;
  out->fic_ratio_percent = c.fic_ratio * 10; out->freq_offs_bb_hz = c.f_bb; out->clock_err_hz = c.clock_err;
  out->snr_db_est = c.snr_db; out->mer_db_est = c.mer_db; out->last_start_index = c.start_index; out->cif_count = c.cif_count;
  out->fib_ok = c.fib_ok; out->fib_total = c.fib_total;
  out->signal_level = c.s_level; out->peak_level = c.peak_level;
  out->fic_ber_bits = c.fic_bits; out->fic_ber_errors = c.fic_errors;
  std::vector<SubchDev> sc(std::max(1, e->dev.max_subch));
  DABX_HIP(hipMemcpy(sc.data(), e->dev.subch + (size_t)stream * e->dev.max_subch, sizeof(SubchDev) * e->dev.max_subch, hipMemcpyDeviceToHost));
  for (int j = 0; j < e->dev.max_subch; j++) {
    out->sf_ok += sc[j].sf_ok; out->sf_fail += sc[j].sf_fail; out->rs_corrected += sc[j].rs_corr; out->rs_failed += sc[j].rs_fail;
    out->au_ok += sc[j].au_ok; out->au_bad += sc[j].au_bad; out->cifs_decoded += sc[j].cif_out;
  }
  return 0;
}

extern "C" {

// The entry point binaries built against ABI 3 call: writes exactly the ABI-3 record (up to and including peak_level), so a
// caller whose dabx_stats is the old, shorter one is not overrun.  Sources compiled against this header reach
// dabx_get_stats_sized through the macro of the same name and get everything their record has room for.
int dabx_get_stats(dabx_engine *e, int stream, dabx_stats *out)
{
  return dabx_get_stats_sized(e, stream, out, offsetof(dabx_stats, peak_level) + sizeof(float));
}
int dabx_get_stats_sized(dabx_engine *e, int stream, void *out, size_t size)
{
  if (!out || size < sizeof(int64_t)) return DABX_E_ARG;
  dabx_stats full;
  if (int rc = get_stats_full(e, stream, &full)) return rc;
  memcpy(out, &full, std::min(size, sizeof(full)));
  if (size > sizeof(full)) memset((char *)out + sizeof(full), 0, size - sizeof(full));
  return 0;
}

int dabx_get_subch_stats(dabx_engine *e, int stream, int j, dabx_subch_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || j < 0 || j >= e->dev.max_subch || !out) return DABX_E_ARG;
  SubchDev sc;
  int rc = fetch_subch(e, stream, j, &sc);
  if (rc) return rc;
  *out = dabx_subch_stats{sc.start_cif, sc.cif_out, sc.sf_count, sc.sf_ok, sc.sf_fail, sc.rs_corr, sc.rs_fail, sc.fc_corr, sc.au_ok,
                          sc.au_bad, sc.active, e->subch_id_host[(size_t)stream * e->dev.max_subch + j]};
  return 0;
}

int dabx_get_counters(dabx_engine *e, int64_t out[16])
{
  if (!e || !out) return DABX_E_ARG;
  if (int rc0 = sync_all(e)) return rc0;
  const int S = e->dev.n_streams;
  std::vector<StreamCtl> ctl(S);
  std::vector<SubchDev> sc((size_t)S * std::max(1, e->dev.max_subch));
  DABX_HIP(hipMemcpy(ctl.data(), e->dev.ctl, sizeof(StreamCtl) * S, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(sc.data(), e->dev.subch, sizeof(SubchDev) * sc.size(), hipMemcpyDeviceToHost));
  memset(out, 0, sizeof(int64_t) * 16);
  for (auto &c : ctl) {
    out[0] += c.frames; out[1] += (int64_t)c.rd; out[2] += c.fib_ok; out[3] += c.fib_total; out[4] += c.sync_lost;
    out[5] += (c.state == ST_EVAL_SYNC);
  }
  for (auto &q : sc) {
    out[6] += q.cif_out; out[7] += q.sf_ok; out[8] += q.sf_fail; out[9] += q.rs_corr; out[10] += q.rs_fail;
    out[11] += q.fc_corr; out[12] += q.au_ok; out[13] += q.au_bad;
    out[14] += (int64_t)q.cif_out * 3 * q.kbps;                 // MSC bytes out
  }
  return 0;
}

int dabx_set_lcd_statistics(dabx_engine *e, int on)
{
  if (!e) return DABX_E_ARG;
  if (int rc = sync_all(e)) return rc;          // no frame may see the switch between its two demapper launches
  e->dev.demap.track_mer = on != 0;
  return 0;
}

int dabx_set_profiling(dabx_engine *e, int on)
{
  if (!e) return DABX_E_ARG;
  if (int rc = sync_all(e)) return rc;
  e->mk.on = on != 0;
  e->mk.serial = on < 0;
  e->mk.only = on >= 2 ? on - 2 : -1;
  e->mk.used = 0;
  e->mk.recs.clear();
  for (int k = 0; k < N_STEP_KERNELS; k++) { e->prof_ms[k] = 0; e->prof_n[k] = 0; }
  return 0;
}

int dabx_get_profile(dabx_engine *e, double total_ms[DABX_MAX_KERNELS], int64_t launches[DABX_MAX_KERNELS],
                     const char *names[DABX_MAX_KERNELS])
{
  if (!e || !total_ms || !launches || !names) return DABX_E_ARG;
  if (int rc = sync_all(e)) return rc;
  for (const auto &r : e->mk.recs) {
    float ms = 0.f;
    DABX_HIP(hipEventElapsedTime(&ms, e->mk.pool[r.a], e->mk.pool[r.b]));
    e->prof_ms[r.k] += ms; e->prof_n[r.k]++;
  }
  e->mk.recs.clear();
  e->mk.used = 0;
  for (int k = 0; k < N_STEP_KERNELS; k++) { total_ms[k] = e->prof_ms[k]; launches[k] = e->prof_n[k]; names[k] = kStepKernelNames[k]; }
  return N_STEP_KERNELS;
}

}  // extern "C"
