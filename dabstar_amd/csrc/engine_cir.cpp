// engine_cir.cpp -- the channel impulse response and the correlation plot on the device (include/dabx.h dabx_set_cir_mode; cir_core.h,
// pipeline.hip k_cir / k_cir_finish / k_cir_corr): the stage's memory, what a stream's settings may be and what a fresh enable resets, the
// host's copy of the window / row bookkeeping that sizes a step's launch, the parts of a record that dabx_read_cir copies, the counters and
// the host-callable entries.  The records of both kinds lie in one record ring (rec_ring.h) of CIR_RING slots per stream, indexed by the
// stream's record count.
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
  hip_free_all({T.list, T.cfg_dev, T.dev.st, T.dev.acc, T.dev.mean, T.dev.ring});
  T = CirStage{};
}

// the first enable: the stream list, a settings row, the bookkeeping, the row buffer, the running mean and a ring of CIR_RING record slots per stream
static int cir_stage_create(dabx_engine *e)
{
  CirStage &T = e->cir;
  const size_t S = (size_t)e->dev.n_streams;
  if (int rc = alloc_zeroed("dabx_set_cir_mode", {{(void **)&T.list, sizeof(int32_t) * S}, {(void **)&T.cfg_dev, sizeof(CirCfgDev) * S},
                                                  {(void **)&T.dev.st, sizeof(CirState) * S}, {(void **)&T.dev.acc, sizeof(float) * CIR_ROWS * S},
                                                  {(void **)&T.dev.mean, sizeof(float) * TU * S}, {(void **)&T.dev.ring, (size_t)CIR_RING * CIR_SLOT_BYTES * S}}))
    return rc;
  T.dev.list = T.list; T.dev.cfg = T.cfg_dev; T.dev.n = T.dev.n_corr = 0;
  T.start(S);
  T.walk.assign(S, CirState{});
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
  int n_corr = 0;
  for (const CirCfgDev &c : T.cfg) n_corr += c.enable ? c.correlation : 0;
  DABX_HIP(hipMemcpy(T.dev.st, st.data(), sizeof(CirState) * S, hipMemcpyHostToDevice));
  if ((rc = T.upload(&T.dev.n))) return rc;
  T.walk = st;                                            // the engine is drained: the device's bookkeeping is the host's
  T.n_corr = T.dev.n_corr = n_corr;
  return 0;
}

int dabx_read_cir(dabx_engine *e, int stream, int max_records, dabx_cir_record *recs, float *values, int16_t *indices, int32_t *lost)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || max_records < 0 || (max_records > 0 && !recs)) { set_error("dabx_read_cir: bad argument"); return DABX_E_ARG; }
  if (lost) *lost = 0;
  CirStage &T = e->cir;
  CirState c;
  if (int rc = stage_state(e, T, stream, &c)) return std::min(rc, 0);
  return rec_ring_read<CIR_RING, CIR_SLOT_BYTES>(T.dev.ring, stream, c.shows, T.seen[(size_t)stream], &T.lost[(size_t)stream], max_records, lost,
                                                  [&](int n, const uint8_t *slot) {
    DABX_HIP(hipMemcpy(recs + n, slot, sizeof(dabx_cir_record), hipMemcpyDeviceToHost));
    if (values) DABX_HIP(hipMemcpy(values + (size_t)n * CIR_CORR_LAGS, slot + 32, sizeof(float) * CIR_CORR_LAGS, hipMemcpyDeviceToHost));
    if (indices) DABX_HIP(hipMemcpy(indices + (size_t)n * CIR_INDEX_ROOM, slot + 32 + CIR_CORR_LAGS * 4, sizeof(int16_t) * CIR_INDEX_ROOM, hipMemcpyDeviceToHost));
    return 0;
  });
}

int dabx_get_cir_stats(dabx_engine *e, int stream, dabx_cir_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) { set_error("dabx_get_cir_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const CirStage &T = e->cir;
  CirState c;
  if (int rc = stage_state(e, T, stream, &c)) return std::min(rc, 0);
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
