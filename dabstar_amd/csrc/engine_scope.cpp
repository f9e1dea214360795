// engine_scope.cpp -- the IQ scope and carrier plots on the device (include/dabx.h dabx_set_scope_mode; scope_core.h, pipeline.hip k_scope):
// the stage's memory, what a stream's settings may be, the parts of a record that dabx_read_scope copies and the counters.  The records lie in
// a record ring (rec_ring.h) of SCOPE_RING slots per stream that k_scope indexes by the stream's show count.
#include "engine.h"
#include <cstring>

static_assert(sizeof(dabx_chunk_scope) == 32 && sizeof(dabx_chunk_header_ext) == 64 && sizeof(dabx_scope_config) == 32 &&sizeof(dabx_scope_record) == 32 && sizeof(dabx_scope_stats) == 64 &&
              DABX_SCOPE_SLOT_BYTES == dabx::SCOPE_SLOT_BYTES && DABX_SCOPE_CARRIERS == dabx::K, "include/dabx.h: the scope records");

namespace dabx {

void scope_stage_free(dabx_engine *e)
{
  ScopeStage &T = e->scope;
  hip_free_all({T.list, T.cfg_dev, T.dev.st, T.dev.ring});
  T = ScopeStage{};
}

// the first enable: the stream list, a settings row, the counters and a ring of SCOPE_RING record slots per stream
static int scope_stage_create(dabx_engine *e)
{
  ScopeStage &T = e->scope;
  const size_t S = (size_t)e->dev.n_streams;
  if (int rc = alloc_zeroed("dabx_set_scope_mode", {{(void **)&T.list, sizeof(int32_t) * S}, {(void **)&T.cfg_dev, sizeof(ScopeCfgDev) * S},
                                                    {(void **)&T.dev.st, sizeof(ScopeState) * S}, {(void **)&T.dev.ring, (size_t)SCOPE_RING * SCOPE_SLOT_BYTES * S}}))
    return rc;
  // mNextShownOfdmSymbIdx = 1 (ofdm_decoder.h:88), both counters 0
  std::vector<ScopeState> st(S, ScopeState{0, 0, 1, 0, 0, 0});
  if (hipMemcpy(T.dev.st, st.data(), sizeof(ScopeState) * S, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("dabx_set_scope_mode: uploading the counters failed");
    scope_stage_free(e);
    return DABX_E_HIP;
  }
  T.dev.list = T.list; T.dev.cfg = T.cfg_dev; T.dev.n = 0;
  T.start(S);
  return 0;
}

}  // namespace dabx

extern "C" {

int dabx_set_scope_mode(dabx_engine *e, int stream, const dabx_scope_config *cfg)
{
  if (!e || stream < -1 || stream >= e->dev.n_streams) { set_error("dabx_set_scope_mode: bad argument"); return DABX_E_ARG; }
  const bool on = !cfg || cfg->enable;
  const int iq = cfg ? cfg->iq_type : 0, ct = cfg ? cfg->carrier_type : 0, sym = cfg ? cfg->symbol : 0;
  if (on) {
    if (iq < 0 || iq >= SCOPE_IQ_TYPES) { set_error("dabx_set_scope_mode: iq_type %d (0..2; the DC-offset plots 3, 4 are not built)", iq); return DABX_E_ARG; }
    if (!scope_carrier_type_built(ct)) { set_error("dabx_set_scope_mode: carrier_type %d (0..9, 13; the NULL_* level plots 10..12 are not built)", ct); return DABX_E_ARG; }
    if (sym < 0 || sym > 75) { set_error("dabx_set_scope_mode: symbol %d (0 = the reference's cadence, 1..75)", sym); return DABX_E_ARG; }
    if (!e->dev.spectra || !e->dev.demap.integ) { set_error("dabx_set_scope_mode: the engine has no demapper"); return DABX_E_STATE; }
    if (ct == SC_STD_DEV && !e->dev.demap.track_mer) { set_error("dabx_set_scope_mode: STD_DEV needs dabx_set_lcd_statistics(on)"); return DABX_E_STATE; }
  }
  int rc;
  if ((rc = use_device(e))) return rc;
  if ((rc = sync_all(e))) return rc;
  ScopeStage &T = e->scope;
  if (!T.exists()) {
    if (!on) return 0;
    if ((rc = scope_stage_create(e))) return rc;
  }
  const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? e->dev.n_streams : stream + 1;
  for (int s = s0; s < s1; s++) {
    ScopeCfgDev &c = T.cfg[(size_t)s];
    if (on) c = ScopeCfgDev{1, iq, ct, sym};          // (the two counters are the device's: an enabled stream keeps them)
    else c.enable = 0;
  }
  return T.upload(&T.dev.n);
}

int dabx_read_scope(dabx_engine *e, int stream, int max_records, dabx_scope_record *recs, float *iq, float *carr, int32_t *lost)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || max_records < 0 || (max_records > 0 && !recs)) { set_error("dabx_read_scope: bad argument"); return DABX_E_ARG; }
  if (lost) *lost = 0;
  ScopeStage &T = e->scope;
  ScopeState c;
  if (int rc = stage_state(e, T, stream, &c)) return std::min(rc, 0);
  return rec_ring_read<SCOPE_RING, SCOPE_SLOT_BYTES>(T.dev.ring, stream, c.shows, T.seen[(size_t)stream], &T.lost[(size_t)stream], max_records, lost,
                                                      [&](int n, const uint8_t *slot) {
    DABX_HIP(hipMemcpy(recs + n, slot, sizeof(dabx_scope_record), hipMemcpyDeviceToHost));
    if (iq) DABX_HIP(hipMemcpy(iq + (size_t)n * 2 * K, slot + 32, sizeof(float) * 2 * K, hipMemcpyDeviceToHost));
    if (carr) DABX_HIP(hipMemcpy(carr + (size_t)n * K, slot + 32 + K * 8, sizeof(float) * K, hipMemcpyDeviceToHost));
    return 0;
  });
}

int dabx_scope_cadence_frame(int32_t counters[3])
{
  if (!counters || counters[2] < 1 || counters[2] > 75) { set_error("dabx_scope_cadence_frame: bad argument"); return DABX_E_ARG; }
  ScopeState q{counters[0], counters[1], counters[2], 0, 0, 0};
  const int shown = scope_counters_frame(q);                // the function k_scope runs
  counters[0] = q.cnt_iq; counters[1] = q.cnt_stat; counters[2] = q.next_sym;
  return shown;
}

int dabx_get_scope_stats(dabx_engine *e, int stream, dabx_scope_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) { set_error("dabx_get_scope_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  const ScopeStage &T = e->scope;
  ScopeState c;
  if (int rc = stage_state(e, T, stream, &c)) return std::min(rc, 0);
  out->shows = c.shows; out->lost = T.lost[(size_t)stream]; out->launches = T.launches;
  return 0;
}

}  // extern "C"
