// engine_cir.cpp -- the channel impulse response and the correlation plot on the device (include/dabx.h dabx_set_cir_mode; cir_core.h,
// pipeline.hip k_cir / k_cir_finish / k_cir_corr): the stage's memory, its per-stream settings and compacted stream list, the host's copy of
// the window / row bookkeeping that sizes a step's launch, the record read-out, the counters and the host-callable entries.  The records of
// both kinds lie in one ring of CIR_RING fixed-size slots per stream, indexed by the stream's record count, read out as engine_scope.cpp
// reads the scope's.
#include "engine.h"
#include <cstring>

static_assert(sizeof(dabx_cir_config) == 32 && sizeof(dabx_cir_record) == 32 && sizeof(dabx_cir_stats) == 64 && sizeof(dabx_chunk_cir) == 32 &&
              sizeof(dabx_chunk_header_ext) == 64 && DABX_CIR_SLOT_BYTES == dabx::CIR_SLOT_BYTES && DABX_CIR_ROWS == dabx::CIR_ROWS &&
              DABX_CIR_WINDOW == dabx::CIR_WINDOW && DABX_CIR_PERIOD == dabx::CIR_PERIOD && DABX_CIR_CORR_LAGS == dabx::CIR_CORR_LAGS &&
              DABX_CIR_MAX_INDICES == dabx::CIR_MAX_INDICES && DABX_CIR_INDEX_ROOM == dabx::CIR_INDEX_ROOM && sizeof(dabx::CirState) == 64 &&
              DABX_CIR_CHUNK_RECORDS <= dabx::CIR_RING, "include/dabx.h: the CIR records");

namespace dabx {

void cir_stage_free(dabx_engine *e)
{
  CirStage &T = e->cir;
  for (void *q : {(void *)T.list, (void *)T.cfg_dev, (void *)T.dev.st, (void *)T.dev.acc, (void *)T.dev.mean, (void *)T.dev.ring}) if (q) (void)hipFree(q);
  T = CirStage{};
}

// the first enable: the stream list, a settings row, the bookkeeping, the row buffer, the running mean and a ring of CIR_RING record slots per stream
static int cir_stage_create(dabx_engine *e)
{
  CirStage &T = e->cir;
  const size_t S = (size_t)e->dev.n_streams;
  const struct { void **p; size_t n; } bufs[] = {{(void **)&T.list, sizeof(int32_t) * S}, {(void **)&T.cfg_dev, sizeof(CirCfgDev) * S},
                                                {(void **)&T.dev.st, sizeof(CirState) * S}, {(void **)&T.dev.acc, sizeof(float) * CIR_ROWS * S},
                                                {(void **)&T.dev.mean, sizeof(float) * TU * S}, {(void **)&T.dev.ring, (size_t)CIR_RING * CIR_SLOT_BYTES * S}};
  for (const auto &b : bufs) {
    hipError_t he = hipMalloc(b.p, b.n);
    if (he == hipSuccess) he = hipMemset(*b.p, 0, b.n);
    if (he != hipSuccess) {
      set_error("dabx_set_cir_mode: HIP error %d (%s) allocating the stage", (int)he, hipGetErrorString(he));
      cir_stage_free(e);
      return he == hipErrorOutOfMemory ? DABX_E_NOMEM : DABX_E_HIP;
    }
  }
  T.dev.list = T.list; T.dev.cfg = T.cfg_dev; T.dev.n = T.dev.n_corr = 0;
  T.cfg.assign(S, CirCfgDev{});
  T.walk.assign(S, CirState{});
  T.seen.assign(S, 0);
  T.lost.assign(S, 0);
  return 0;
}

// The rows due in the step about to be launched, the most any stream has (the launch's blocks per stream; 0: no launch): cir_rows_due over
// the host's count of committed samples, which is the device's at that point of the front-end stream (every commit is issued on it).
// advance = false: the count alone, in front of the launch; advance = true, behind a step that was launched: the host's bookkeeping moves on
// as k_cir_finish moves the device's (a step whose launch failed leaves both where they were).
int cir_step_cap(dabx_engine *e, bool advance)
{
  CirStage &T = e->cir;
  int cap = 0;
  for (int s = 0; s < e->dev.n_streams; s++) {
    if (!T.cfg[(size_t)s].enable || !T.cfg[(size_t)s].cir) continue;
    CirState &w = T.walk[(size_t)s];
    const int due = cir_rows_due(w.base, w.win, w.rows_done, e->wr_host[(size_t)s], CIR_ROWS);
    if (advance) cir_rows_advance(w.win, w.rows_done, due);
    cap = std::max(cap, due);
  }
  return cap;
}

}  // namespace dabx

extern "C" {

int dabx_set_cir_mode(dabx_engine *e, int stream, const dabx_cir_config *cfg)
{
  if (!e || stream < -1 || stream >= e->dev.n_streams) { set_error("dabx_set_cir_mode: bad argument"); return DABX_E_ARG; }
  const bool on = cfg && cfg->enable;
  if (on) {
    if ((cfg->cir & ~1) || (cfg->correlation & ~1) || !(cfg->cir | cfg->correlation)) { set_error("dabx_set_cir_mode: cir %d, correlation %d (0 / 1, one of them on)", cfg->cir, cfg->correlation); return DABX_E_ARG; }
    for (int r : cfg->reserved) if (r) { set_error("dabx_set_cir_mode: a reserved word is not 0"); return DABX_E_ARG; }
  }
  int rc;
  if ((rc = use_device(e))) return rc;
  if ((rc = sync_all(e))) return rc;
  CirStage &T = e->cir;
  if (!T.exists()) {
    if (!on) return 0;
    if ((rc = cir_stage_create(e))) return rc;
  }
  const size_t S = (size_t)e->dev.n_streams;
  std::vector<CirState> st(S);
  std::vector<StreamCtl> ctl(S);
  DABX_HIP(hipMemcpy(st.data(), T.dev.st, sizeof(CirState) * S, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(ctl.data(), e->dev.ctl, sizeof(StreamCtl) * S, hipMemcpyDeviceToHost));
  const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? e->dev.n_streams : stream + 1;
  for (int s = s0; s < s1; s++) {
    CirCfgDev &c = T.cfg[(size_t)s];
    const CirCfgDev was = c;
    c = on ? CirCfgDev{1, cfg->cir, cfg->correlation, 0} : CirCfgDev{};
    CirState &q = st[(size_t)s];
    if (c.cir && !was.cir) { q.base = ctl[(size_t)s].rd; q.win = 0; q.rows_done = 0; }     // a new window at the read position (the stated deviation)
    if (c.correlation && !was.correlation) {                                              // a fresh PhaseReference: mean 0, counter 0
      q.corr_counter = 0;
      DABX_HIP(hipMemset(T.dev.mean + (size_t)s * TU, 0, sizeof(float) * TU));
    }
  }
  std::vector<int32_t> list;
  int n_corr = 0;
  for (int s = 0; s < e->dev.n_streams; s++) if (T.cfg[(size_t)s].enable) { list.push_back(s); n_corr += T.cfg[(size_t)s].correlation; }
  DABX_HIP(hipMemcpy(T.dev.st, st.data(), sizeof(CirState) * S, hipMemcpyHostToDevice));
  DABX_HIP(hipMemcpy(T.cfg_dev, T.cfg.data(), sizeof(CirCfgDev) * S, hipMemcpyHostToDevice));
  if (!list.empty()) DABX_HIP(hipMemcpy(T.list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice));
  T.walk = st;                                            // the engine is drained: the device's bookkeeping is the host's
  T.n_on = T.dev.n = (int)list.size();
  T.n_corr = T.dev.n_corr = n_corr;
  return 0;
}

int dabx_read_cir(dabx_engine *e, int stream, int max_records, dabx_cir_record *recs, float *values, int16_t *indices, int32_t *lost)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || max_records < 0 || (max_records > 0 && !recs)) { set_error("dabx_read_cir: bad argument"); return DABX_E_ARG; }
  if (lost) *lost = 0;
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  CirStage &T = e->cir;
  if (!T.exists()) return 0;
  CirState c;
  DABX_HIP(hipMemcpy(&c, T.dev.st + stream, sizeof(c), hipMemcpyDeviceToHost));
  long long &seen = T.seen[(size_t)stream];
  if (c.shows - seen > CIR_RING) {
    const long long gone = c.shows - seen - CIR_RING;
    if (lost) *lost = (int32_t)std::min<long long>(gone, INT32_MAX);
    T.lost[(size_t)stream] += gone;
    seen = c.shows - CIR_RING;
  }
  int n = 0;
  while (n < max_records && seen < c.shows) {
    const uint8_t *slot = T.dev.ring + ((size_t)stream * CIR_RING + (size_t)(seen % CIR_RING)) * CIR_SLOT_BYTES;
    DABX_HIP(hipMemcpy(recs + n, slot, sizeof(dabx_cir_record), hipMemcpyDeviceToHost));
    if (values) DABX_HIP(hipMemcpy(values + (size_t)n * CIR_CORR_LAGS, slot + 32, sizeof(float) * CIR_CORR_LAGS, hipMemcpyDeviceToHost));
    if (indices) DABX_HIP(hipMemcpy(indices + (size_t)n * CIR_INDEX_ROOM, slot + 32 + CIR_CORR_LAGS * 4, sizeof(int16_t) * CIR_INDEX_ROOM, hipMemcpyDeviceToHost));
    n++; seen++;
  }
  return n;
}

int dabx_get_cir_stats(dabx_engine *e, int stream, dabx_cir_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) { set_error("dabx_get_cir_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  const CirStage &T = e->cir;
  if (!T.exists()) return 0;
  CirState c;
  DABX_HIP(hipMemcpy(&c, T.dev.st + stream, sizeof(c), hipMemcpyDeviceToHost));
  out->shows[0] = c.shows_kind[0]; out->shows[1] = c.shows_kind[1]; out->lost = T.lost[(size_t)stream];
  out->rows_untrusted = c.rows_untrusted; out->launches = T.launches;
  return 0;
}

int dabx_cir_rows_due(int64_t walk[3], uint64_t wr, int32_t cap, int64_t *first, int32_t *completed)
{
  if (!walk || walk[0] < 0 || walk[1] < 0 || walk[2] < 0 || walk[2] >= CIR_ROWS || cap < 0) { set_error("dabx_cir_rows_due: bad argument"); return DABX_E_ARG; }
  long long win = walk[1];
  int32_t rows_done = (int32_t)walk[2];
  const int n = cir_rows_due((unsigned long long)walk[0], win, rows_done, wr, cap);     // the functions k_cir and k_cir_finish run
  if (first) *first = (int64_t)cir_row_first((unsigned long long)walk[0], win, rows_done);
  const int done = cir_rows_advance(win, rows_done, n);
  if (completed) *completed = done;
  walk[1] = win; walk[2] = rows_done;
  return n;
}

int dabx_cir_row_trusted(uint64_t first, uint64_t rd, uint64_t horizon, uint64_t ring_len)
{
  return cir_row_trusted(first, rd, horizon, ring_len) ? 1 : 0;                          // the function k_cir runs
}

}  // extern "C"
