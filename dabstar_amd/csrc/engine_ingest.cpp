// engine_ingest.cpp -- bulk ingest (include/dabx.h "Bulk ingest"): the input slabs, their transfers and the dabx_ingest_* entries.
#include "engine.h"
#include <algorithm>
#include <map>
#include <utility>
#include <vector>

namespace dabx {

void ingest_free(dabx_engine *e)
{
  Ingest &I = e->ing;
  for (auto &sl : I.slabs) {
    if (sl.in_flight && sl.bytes && I.copy_engine == 0) (void)sdma_wait(sl.sig, 0);
    if (sl.host) (void)hipHostFree(sl.host);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.counts_read) (void)hipEventDestroy(sl.counts_read);
    sdma_signal_destroy(sl.sig);
  }
  if (I.cs) { (void)hipStreamSynchronize(I.cs); (void)hipStreamDestroy(I.cs); }
  for (void *q : {(void *)I.tables_dev, (void *)I.work, (void *)I.carry, (void *)I.tab_int, (void *)I.tab_frac}) if (q) (void)hipFree(q);
  if (I.tables_host) (void)hipHostFree(I.tables_host);
  I = Ingest{};
}

}  // namespace dabx

static int ingest_open_impl(dabx_engine *e, const dabx_ingest_config *cfg, const dabx_iq_format *formats)
{
  if (!e || (cfg && (cfg->host_slabs < 0 || cfg->host_slabs > 64 || cfg->fmt < 0 || cfg->fmt > 2 || cfg->max_frames < 0 || cfg->copy_engine < 0 || cfg->copy_engine > 1))) {
    set_error("dabx_ingest_open: bad argument");
    return DABX_E_ARG;
  }
  if (e->ing.open) { set_error("dabx_ingest_open: already open"); return DABX_E_STATE; }
  if (!formats) { if (int rc = ring_takes(e, cfg ? cfg->fmt : 0, "dabx_ingest_open")) return rc; }
  if (int rc = use_device(e)) return rc;
  Ingest &I = e->ing;
  I.copy_engine = cfg ? cfg->copy_engine : 0;
  I.max_frames = cfg && cfg->max_frames ? cfg->max_frames : DL_FRAMES;
  if ((long long)I.max_frames * TF > e->dev.ring_len) { set_error("dabx_ingest_open: a slab of %d frames does not fit the ring (%d frames)", I.max_frames, e->dev.ring_len / TF); return DABX_E_ARG; }
  int rc;
  const int S_ = e->dev.n_streams;
  I.dec.assign((size_t)S_, IqDecode{}); I.M.assign((size_t)S_, 0); I.tab.assign((size_t)S_, 0); I.carry_n.assign((size_t)S_, 0);
  std::vector<int16_t> tabs_i; std::vector<float> tabs_f;
  int m_max = 0;
  if (formats) {
    // every stream's own recording: the region of a slab that holds max_frames frames' worth of ITS payload (+ one read block) sets the pitch
    I.general = true;
    std::map<std::pair<int, int>, int> tab_of;
    size_t need = 0;
    for (int s = 0; s < S_; s++) {
      if ((rc = iq_check_format(&formats[s], &I.dec[(size_t)s])) || (rc = iq_native_ring(&formats[s], &I.dec[(size_t)s], e->dev.ring_fmt))) { ingest_free(e); return rc; }
      const int rate = formats[s].sample_rate;
      if (rate != INPUT_RATE) {
        const auto key = std::make_pair((int)formats[s].family, rate);
        if (!tab_of.count(key)) {
          tab_of[key] = (int)tab_of.size();
          tabs_i.resize(tabs_i.size() + 2048); tabs_f.resize(tabs_f.size() + 2048);
          int m = 0;
          iq_resample_tables(formats[s].family, rate, &m, tabs_i.data() + tabs_i.size() - 2048, tabs_f.data() + tabs_f.size() - 2048);
        }
        I.tab[(size_t)s] = tab_of[key];
        I.M[(size_t)s] = rate / 1000;
        I.carry_n[(size_t)s] = formats[s].family == DABX_FAMILY_UFF ? 1 : 0;     // xml_reader.cpp:84-85,226: convBuffer[0] starts as a zero sample
        m_max = std::max(m_max, rate / 1000);
      }
      const size_t in_per_frame = (size_t)((long long)TF * (rate / 1000) / 2048) + (size_t)(rate / 1000);
      need = std::max(need, ((size_t)I.max_frames * in_per_frame + (size_t)(rate / 1000)) * 2 * (size_t)I.dec[(size_t)s].bytes);
    }
    I.pitch = align_up(need, 256);
    I.capacity = I.pitch * (size_t)S_;
  } else {
    // every stream the same push format: a slab is dense, [S][n] samples
    if ((rc = iq_push_decode(cfg ? cfg->fmt : 0, e->dev.ring_fmt, &I.dec[0]))) { ingest_free(e); return rc; }
    I.dec.assign((size_t)S_, I.dec[0]);
    I.capacity = (size_t)S_ * I.max_frames * TF * (size_t)(2 * I.dec[0].bytes);
  }
  if (I.copy_engine == 0 && (rc = sdma_open(e->device, &I.sdma))) { ingest_free(e); return rc; }      // (the per-stream tables above go with it)
#define H(x) do { hipError_t err__ = (x); if (err__ != hipSuccess) { set_error("HIP error %d (%s) at %s:%d", (int)err__, hipGetErrorString(err__), __FILE__, __LINE__); ingest_free(e); return DABX_E_HIP; } } while (0)
  if (I.copy_engine == 1) H(hipStreamCreateWithFlags(&I.cs, hipStreamNonBlocking));
  I.slabs.resize((size_t)(cfg && cfg->host_slabs ? cfg->host_slabs : 2));
  if (I.general) {
    if (m_max) {
      // [carry | decoded samples of one slab] per resampling stream, and the carry between slabs (<= M + 1 samples)
      size_t max_in = 0;
      for (int s = 0; s < S_; s++) if (I.M[(size_t)s]) max_in = std::max(max_in, I.pitch / (size_t)(2 * I.dec[(size_t)s].bytes));
      I.work_pitch = align_up(max_in + (size_t)m_max + 2, 64);
      I.carry_pitch = align_up((size_t)m_max + 2, 64);
      H(hipMalloc((void **)&I.work, sizeof(float2) * I.work_pitch * (size_t)S_));
      H(hipMalloc((void **)&I.carry, sizeof(float2) * I.carry_pitch * (size_t)S_));
      H(hipMemset(I.carry, 0, sizeof(float2) * I.carry_pitch * (size_t)S_));
      H(hipMalloc((void **)&I.tab_int, tabs_i.size() * sizeof(int16_t)));
      H(hipMalloc((void **)&I.tab_frac, tabs_f.size() * sizeof(float)));
      H(hipMemcpy(I.tab_int, tabs_i.data(), tabs_i.size() * sizeof(int16_t), hipMemcpyHostToDevice));
      H(hipMemcpy(I.tab_frac, tabs_f.data(), tabs_f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  for (auto &sl : I.slabs) {
    H(hipHostMalloc((void **)&sl.host, I.capacity, hipHostMallocDefault));
    H(hipMalloc((void **)&sl.dev, I.capacity));
    if (I.general) H(hipEventCreateWithFlags(&sl.counts_read, hipEventDisableTiming));
    if (I.copy_engine == 0 && (rc = sdma_signal_create(&sl.sig))) { ingest_free(e); return rc; }
  }
  // (the tables behind the slabs: the slabs' own allocations follow each other as they always have)
  const size_t table = (sizeof(IqJob) + sizeof(unsigned)) * (size_t)S_;
  H(hipHostMalloc((void **)&I.tables_host, table * I.slabs.size(), hipHostMallocDefault));
  H(hipMalloc((void **)&I.tables_dev, table * I.slabs.size()));
  for (size_t k = 0; k < I.slabs.size(); k++) {
    I.slabs[k].jobs_host = reinterpret_cast<IqJob *>(I.tables_host + k * table);
    I.slabs[k].jobs_dev = reinterpret_cast<IqJob *>(I.tables_dev + k * table);
  }
#undef H
  if (I.copy_engine == 0 && I.capacity >= ((size_t)16 << 20) && (rc = sdma_calibrate(I.sdma, I.slabs[0].host, I.slabs[0].dev, false, I.slabs[0].sig, nullptr))) {
    ingest_free(e);
    return rc;
  }
  I.open = true;
  return 0;
}

// slab k takes n_bytes[s] payload bytes per stream, `pitch` bytes apart: ONE transfer, up to the last byte any stream uses (the regions of
// streams that end early travel as they are)
static int ingest_submit(dabx_engine *e, int k, const std::vector<size_t> &n_bytes, size_t pitch, const char *who)
{
  Ingest &I = e->ing;
  if (int rc = use_device(e)) return rc;
  Ingest::Slab &sl = I.slabs[(size_t)k];
  if (sl.in_flight) { set_error("%s: slab %d has a transfer that was not committed", who, k); return DABX_E_STATE; }
  size_t last = 0;
  for (size_t s = 0; s < n_bytes.size(); s++) if (n_bytes[s]) last = s * pitch + n_bytes[s];
  // (the device twin is free: its converter ran on the ingest stream before the commit that cleared in_flight was queued, and a slab is
  //  only reused after its commit -- by then, with two slabs, a whole chunk later)
  DABX_HIP(hipStreamSynchronize(e->ingest));
  if (last) {
    if (I.copy_engine == 0) { if (int rc = sdma_copy(I.sdma, sl.dev, sl.host, last, false, sl.sig)) return rc; }
    else DABX_HIP(hipMemcpyAsync(sl.dev, sl.host, last, hipMemcpyHostToDevice, I.cs));
  }
  sl.n_bytes = n_bytes; sl.pitch = pitch; sl.bytes = last; sl.in_flight = true;
  return 0;
}

extern "C" {

int dabx_ingest_open(dabx_engine *e, const dabx_ingest_config *cfg) { return ingest_open_impl(e, cfg, nullptr); }
int dabx_ingest_open_formats(dabx_engine *e, const dabx_ingest_config *cfg, const dabx_iq_format *formats)
{
  if (!formats) { set_error("dabx_ingest_open_formats: bad argument"); return DABX_E_ARG; }
  return ingest_open_impl(e, cfg, formats);
}
long long dabx_ingest_pitch(dabx_engine *e)
{
  if (!e) return DABX_E_ARG;
  if (!e->ing.open) { set_error("dabx_ingest_pitch: no ingest open"); return DABX_E_STATE; }
  return (long long)(e->ing.general ? e->ing.pitch : e->ing.capacity / (size_t)e->dev.n_streams);
}

int dabx_ingest_close(dabx_engine *e)
{
  if (!e) return DABX_E_ARG;
  if (!e->ing.open) return 0;
  const int rc = sync_all(e);
  ingest_free(e);
  return rc;
}

int dabx_ingest_slab(dabx_engine *e, int k, void **host, size_t *capacity_bytes)
{
  if (!e || !host) return DABX_E_ARG;
  if (!e->ing.open || k < 0 || k >= (int)e->ing.slabs.size()) { set_error("dabx_ingest_slab: no such slab"); return DABX_E_STATE; }
  *host = e->ing.slabs[(size_t)k].host;
  if (capacity_bytes) *capacity_bytes = e->ing.capacity;
  return 0;
}

int dabx_ingest_submit(dabx_engine *e, int k, size_t n)
{
  if (!e) return DABX_E_ARG;
  Ingest &I = e->ing;
  if (!I.open || k < 0 || k >= (int)I.slabs.size()) { set_error("dabx_ingest_submit: no such slab"); return DABX_E_STATE; }
  if (I.general) { set_error("dabx_ingest_submit: this ingest was opened with per-stream formats (dabx_ingest_submit_bytes)"); return DABX_E_STATE; }
  if (n == 0 || n > (size_t)I.max_frames * TF) { set_error("dabx_ingest_submit: %zu samples per stream, the slabs hold %d frames", n, I.max_frames); return DABX_E_ARG; }
  const size_t bytes = n * (size_t)(2 * I.dec[0].bytes);
  return ingest_submit(e, k, std::vector<size_t>((size_t)e->dev.n_streams, bytes), bytes, "dabx_ingest_submit");
}

int dabx_ingest_submit_bytes(dabx_engine *e, int k, const size_t *n_bytes)
{
  if (!e || !n_bytes) return DABX_E_ARG;
  Ingest &I = e->ing;
  if (!I.open || !I.general || k < 0 || k >= (int)I.slabs.size()) { set_error("dabx_ingest_submit_bytes: no such slab of an ingest opened with dabx_ingest_open_formats"); return DABX_E_STATE; }
  for (int s = 0; s < e->dev.n_streams; s++) {
    const IqDecode &d = I.dec[(size_t)s];
    const size_t unit = (size_t)(2 * d.bytes) * (d.quirk_block ? (size_t)d.quirk_block : 1);
    if (n_bytes[s] > I.pitch || n_bytes[s] % unit) {
      set_error("dabx_ingest_submit_bytes: stream %d: %zu bytes -- at most %zu, whole samples%s only (a reader keeps the odd tail for its next slab)", s, n_bytes[s], I.pitch,
                d.quirk_block ? " and whole 1-ms read blocks" : "");
      return DABX_E_ARG;
    }
  }
  return ingest_submit(e, k, std::vector<size_t>(n_bytes, n_bytes + e->dev.n_streams), I.pitch, "dabx_ingest_submit_bytes");
}

// One job per stream -- its decode, its resampling state, its sample count -- and at most two launches for all streams together
int dabx_ingest_commit(dabx_engine *e, int k)
{
  if (!e) return DABX_E_ARG;
  Ingest &I = e->ing;
  if (!I.open || k < 0 || k >= (int)I.slabs.size()) { set_error("dabx_ingest_commit: no such slab"); return DABX_E_STATE; }
  if (int rc = use_device(e)) return rc;
  Ingest::Slab &sl = I.slabs[(size_t)k];
  if (!sl.in_flight) { set_error("dabx_ingest_commit: slab %d was not submitted", k); return DABX_E_STATE; }
  const int S = e->dev.n_streams;
  IqJob *jobs = sl.jobs_host;
  unsigned *counts = reinterpret_cast<unsigned *>(jobs + S);
  unsigned max_n = 0, max_out = 0;
  bool resamples = false;
  for (int s = 0; s < S; s++) {
    IqJob &j = jobs[s];
    j = IqJob{};
    j.dec = I.dec[(size_t)s];
    j.src_off = (unsigned long long)s * sl.pitch;
    j.n = (unsigned)(sl.n_bytes[(size_t)s] / (size_t)(2 * j.dec.bytes));
    j.M = (unsigned)I.M[(size_t)s]; j.tab = (unsigned)I.tab[(size_t)s]; j.carry_n = (unsigned)I.carry_n[(size_t)s];
    counts[s] = iq_plan(&j);
    max_n = std::max(max_n, j.n);
    if (j.M && j.n) { resamples = true; max_out = std::max(max_out, counts[s]); }
    if (int rc = push_room(e, s, counts[s], "dabx_ingest_commit")) return rc;   // (the transfer stays pending: process, then commit again)
  }
  if (sl.bytes) {
    if (I.copy_engine == 0) { if (int rc = sdma_wait(sl.sig, 0)) return rc; }
    else DABX_HIP(hipStreamSynchronize(I.cs));
  }
  for (int s = 0; s < S; s++) {
    jobs[s].dst0 = e->wr_host[s];                       // the host's own count of committed samples: no device-side index is read
    announce_write(e, s, e->wr_host[s] + counts[s]);
  }
  // The samples land beyond the committed indices, push_room has made the room: the writer waits for nothing on the front-end stream.
  // The device table does, in the per-stream form: k_commit_counts of this slab's PREVIOUS commit reads its counts on the front-end
  // stream, possibly still queued there behind steps.  counts_read was recorded right behind that kernel, and the upload below is
  // ordered behind counts_read in the ingest stream: the table is not rewritten before the kernel has run.  (The writer kernels read
  // the table on the ingest stream itself, in order.  The uniform form commits its count by value.)
  if (I.general) DABX_HIP(hipStreamWaitEvent(e->ingest, sl.counts_read, 0));
  DABX_HIP(hipMemcpyAsync(sl.jobs_dev, jobs, (sizeof(IqJob) + sizeof(unsigned)) * (size_t)S, hipMemcpyHostToDevice, e->ingest));
  IqIo io{};
  io.src = sl.dev; io.dst = e->dev.iq; io.dst_len = e->dev.ring_len; io.work = I.work; io.work_pitch = I.work_pitch;
  io.carry = I.carry; io.carry_pitch = I.carry_pitch; io.tab_int = I.tab_int; io.tab_frac = I.tab_frac;
  if (int rc = launch_iq_jobs(io, sl.jobs_dev, S, max_n, max_out, resamples, e->ingest)) return rc;
  DABX_HIP(hipEventRecord(e->ingest_done, e->ingest));
  DABX_HIP(hipStreamWaitEvent(e->stream, e->ingest_done, 0));
  for (int s = 0; s < S; s++) if (jobs[s].M) I.carry_n[(size_t)s] = (int)jobs[s].keep;
  sl.in_flight = false;
  if (!I.general) return commit_impl(e, -1, counts[0]);
  for (int s = 0; s < S; s++) e->wr_host[s] += counts[s];
  if (int rc = launch_commit_counts(e->dev.wr, reinterpret_cast<const unsigned *>(sl.jobs_dev + S), S, e->stream)) return rc;
  DABX_HIP(hipEventRecord(sl.counts_read, e->stream));
  if (e->cfg.dc_iq_correction) return launch_dciq(e->dev, e->cfg.dc_iq_correction, e->stream);
  return 0;
}

}  // extern "C"
