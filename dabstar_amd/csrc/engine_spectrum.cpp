// engine_spectrum.cpp -- the RF spectrum and waterfall rows on the device (include/dabx.h dabx_set_spectrum_mode; spectrum_core.h, pipeline.hip
// k_spectrum): the stage's memory, its window table, what a stream's settings may be and what a fresh enable resets, the parts of a record
// that dabx_read_spectrum copies, the counters and the host-callable entries.  The records lie in a record ring (rec_ring.h) of SPEC_RING
// slots per stream, indexed by the stream's record count.
#include "engine.h"
#include <cstring>

static_assert(sizeof(dabx_spectrum_config) == 32 && sizeof(dabx_spectrum_record) == 32 && sizeof(dabx_spectrum_limits_rec) == 32 &&
              sizeof(dabx_spectrum_stats) == 64 && sizeof(dabx_chunk_spectrum) == 32 && sizeof(dabx_chunk_header_ext) == 64 &&
              DABX_SPECTRUM_SLOT_BYTES == dabx::SPEC_SLOT_BYTES && DABX_SPECTRUM_BINS == dabx::SPEC_DISPLAY && DABX_SPECTRUM_SIZE == dabx::SPEC_SIZE &&
              DABX_SPECTRUM_PERIOD == dabx::SPEC_PERIOD && DABX_SPECTRUM_RING == dabx::SPEC_RING && DABX_SPECTRUM_CHUNK_RECORDS <= dabx::SPEC_RING &&
              sizeof(dabx::SpecState) % 8 == 0, "include/dabx.h: the spectrum records");

namespace dabx {

void spectrum_stage_free(dabx_engine *e)
{
  SpecStage &T = e->spectrum;
  hip_free_all({T.list, T.cfg_dev, T.window, T.dev.st, T.dev.disp, T.dev.pend, T.dev.ring});
  T = SpecStage{};
}

// the first enable: the stream list, a settings row, the bookkeeping, the display buffer, the pending slot and a ring of SPEC_RING record slots per
// stream, and the flat-top window (8 KB)
static int spectrum_stage_create(dabx_engine *e)
{
  SpecStage &T = e->spectrum;
  const size_t S = (size_t)e->dev.n_streams;
  if (int rc = alloc_zeroed("dabx_set_spectrum_mode", {{(void **)&T.list, sizeof(int32_t) * S}, {(void **)&T.cfg_dev, sizeof(SpecCfgDev) * S},
                                                       {(void **)&T.window, sizeof(float) * SPEC_SIZE}, {(void **)&T.dev.st, sizeof(SpecState) * S},
                                                       {(void **)&T.dev.disp, sizeof(float) * SPEC_DISPLAY * S}, {(void **)&T.dev.pend, (size_t)SPEC_SLOT_BYTES * S},
                                                       {(void **)&T.dev.ring, (size_t)SPEC_RING * SPEC_SLOT_BYTES * S}}))
    return rc;
  std::vector<float> w(SPEC_SIZE);
  spectrum_make_window(w.data());
  const hipError_t he = hipMemcpy(T.window, w.data(), sizeof(float) * SPEC_SIZE, hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    set_error("dabx_set_spectrum_mode: HIP error %d (%s) allocating the stage", (int)he, hipGetErrorString(he));
    spectrum_stage_free(e);
    return he == hipErrorOutOfMemory ? DABX_E_NOMEM : DABX_E_HIP;
  }
  T.dev.list = T.list; T.dev.cfg = T.cfg_dev; T.dev.window = T.window; T.dev.n = 0;
  T.start(S);
  return 0;
}

}  // namespace dabx

extern "C" {

int dabx_set_spectrum_mode(dabx_engine *e, int stream, const dabx_spectrum_config *cfg)
{
  if (!e || stream < -1 || stream >= e->dev.n_streams) { set_error("dabx_set_spectrum_mode: bad argument"); return DABX_E_ARG; }
  const bool on = cfg && cfg->enable;
  if (on) {
    if (cfg->averaging < 0 || cfg->averaging > 2 || cfg->zoom_percent < 0 || cfg->zoom_percent > 100) {
      set_error("dabx_set_spectrum_mode: averaging %d (0..2), zoom_percent %d (0..100)", cfg->averaging, cfg->zoom_percent);
      return DABX_E_ARG;
    }
    for (int r : cfg->reserved) if (r) { set_error("dabx_set_spectrum_mode: a reserved word is not 0"); return DABX_E_ARG; }
  }
  int rc;
  if ((rc = use_device(e))) return rc;
  if ((rc = sync_all(e))) return rc;
  SpecStage &T = e->spectrum;
  if (!T.exists()) {
    if (!on) return 0;
    if ((rc = spectrum_stage_create(e))) return rc;
  }
  const size_t S = (size_t)e->dev.n_streams;
  std::vector<SpecState> st(S);
  std::vector<StreamCtl> ctl(S);
  DABX_HIP(hipMemcpy(st.data(), T.dev.st, sizeof(SpecState) * S, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(ctl.data(), e->dev.ctl, sizeof(StreamCtl) * S, hipMemcpyDeviceToHost));
  const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? e->dev.n_streams : stream + 1;
  for (int s = s0; s < s1; s++) {
    SpecCfgDev &c = T.cfg[(size_t)s];
    const SpecCfgDev was = c;
    c = on ? SpecCfgDev{1, cfg->averaging, cfg->zoom_percent, 0} : SpecCfgDev{};
    if (c.enable && !was.enable) {                          // a fresh capture at the read position (the stated deviation), a fresh SpectrumViewer
      SpecState &q = st[(size_t)s];
      const StreamCtl &k = ctl[(size_t)s];
      q.W = q.pos = k.rd; q.lost_seen = k.sync_lost; q.state_seen = k.state; q.computed = 0;
      q.lim = spectrum_limits_initial();
      DABX_HIP(hipMemset(T.dev.disp + (size_t)s * SPEC_DISPLAY, 0, sizeof(float) * SPEC_DISPLAY));
    }
  }
  DABX_HIP(hipMemcpy(T.dev.st, st.data(), sizeof(SpecState) * S, hipMemcpyHostToDevice));
  return T.upload(&T.dev.n);
}

int dabx_read_spectrum(dabx_engine *e, int stream, int max_records, dabx_spectrum_record *recs, dabx_spectrum_limits_rec *limits, float *db,
                       uint8_t *row, int32_t *lost)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || max_records < 0 || (max_records > 0 && !recs)) { set_error("dabx_read_spectrum: bad argument"); return DABX_E_ARG; }
  if (lost) *lost = 0;
  SpecStage &T = e->spectrum;
  SpecState c;
  if (int rc = stage_state(e, T, stream, &c)) return std::min(rc, 0);
  return rec_ring_read<SPEC_RING, SPEC_SLOT_BYTES>(T.dev.ring, stream, c.shows, T.seen[(size_t)stream], &T.lost[(size_t)stream], max_records, lost,
                                                    [&](int n, const uint8_t *slot) {
    DABX_HIP(hipMemcpy(recs + n, slot, sizeof(dabx_spectrum_record), hipMemcpyDeviceToHost));
    if (limits) DABX_HIP(hipMemcpy(limits + n, slot + 32, sizeof(dabx_spectrum_limits_rec), hipMemcpyDeviceToHost));
    if (db) DABX_HIP(hipMemcpy(db + (size_t)n * SPEC_DISPLAY, slot + 64, sizeof(float) * SPEC_DISPLAY, hipMemcpyDeviceToHost));
    if (row) DABX_HIP(hipMemcpy(row + (size_t)n * SPEC_DISPLAY, slot + 64 + SPEC_DISPLAY * 4, SPEC_DISPLAY, hipMemcpyDeviceToHost));
    return 0;
  });
}

int dabx_get_spectrum_stats(dabx_engine *e, int stream, dabx_spectrum_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) { set_error("dabx_get_spectrum_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const SpecStage &T = e->spectrum;
  SpecState c;
  if (int rc = stage_state(e, T, stream, &c)) return std::min(rc, 0);
  out->shows = c.shows; out->untrusted = c.untrusted; out->lost = T.lost[(size_t)stream]; out->launches = T.launches; out->inexact = c.inexact;
  return 0;
}

int dabx_spectrum_limits(const float ext[4], float limits[4], int averaging, int zoom_percent, float y[2])
{
  if (!ext || !limits || !y || averaging < 0 || averaging > 2 || zoom_percent < 0 || zoom_percent > 100) { set_error("dabx_spectrum_limits: bad argument"); return DABX_E_ARG; }
  SpecLimits l{limits[0], limits[1], limits[2], limits[3]};
  const int valid = spectrum_limits(ext, l, spectrum_alpha(averaging), zoom_percent, &y[0], &y[1]);     // the function k_spectrum runs
  limits[0] = l.glob_max; limits[1] = l.glob_min; limits[2] = l.loc_max; limits[3] = l.loc_min;
  return valid;
}

int dabx_spectrum_waterfall_row(const float *db, int n, const float y[2], uint8_t *row)
{
  if (!db || !row || !y || n < 0 || !(y[1] - y[0] > 0.0f)) { set_error("dabx_spectrum_waterfall_row: bad argument"); return DABX_E_ARG; }
  for (int i = 0; i < n; i++) row[i] = spectrum_pixel(db[i], y[0], y[1] - y[0]);                        // the function k_spectrum runs
  return 0;
}

int64_t dabx_spectrum_next_show(uint64_t W, int kind, uint64_t a, uint64_t b)
{
  if (kind != SPEC_SEARCHED && kind != SPEC_FRAME) { set_error("dabx_spectrum_next_show: bad argument"); return DABX_E_ARG; }
  const unsigned long long E = spectrum_next_show(W, kind, a, b);                                       // the function k_spectrum runs
  return E == SPEC_NONE ? -1 : (int64_t)E;
}

// One look of k_spectrum at a stream, on the host: walk = { W, pos, lost_seen, state_seen } in and out, as SpecState holds them; the rest is
// what the kernel reads out of the stream's control record behind the frame head.  As in the kernel, a show moves W on to E.
int64_t dabx_spectrum_look(int64_t walk[4], uint64_t rd, int state, int64_t sync_lost, int frame_ok, uint64_t sym0_pos, int32_t *inexact)
{
  if (!walk || state < 0 || state > 2 || walk[3] < 0 || walk[3] > 2) { set_error("dabx_spectrum_look: bad argument"); return DABX_E_ARG; }
  SpecState q{};
  q.W = (unsigned long long)walk[0]; q.pos = (unsigned long long)walk[1]; q.lost_seen = walk[2]; q.state_seen = (int32_t)walk[3];
  int inx = 0;
  const unsigned long long W = q.W;
  unsigned long long E = spectrum_look(q, rd, state, sync_lost, frame_ok ? 1 : 0, sym0_pos, &inx);      // the function k_spectrum runs
  if (q.W != W) E = SPEC_NONE;                              // (a stream that was put back shows nothing in this look)
  if (E != SPEC_NONE) q.W = E;
  walk[0] = (int64_t)q.W; walk[1] = (int64_t)q.pos; walk[2] = q.lost_seen; walk[3] = q.state_seen;
  if (inexact) *inexact = E != SPEC_NONE ? inx : 0;
  return E == SPEC_NONE ? -1 : (int64_t)E;
}

}  // extern "C"
