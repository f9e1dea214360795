// engine_tii.cpp -- the TII detectors on the device (include/dabx.h dabx_set_tii_mode; tii_core.h, deliver.hip k_tii): the stage's memory, its
// per-stream settings, the parts of an event that dabx_read_tii_events copies and the counters.  The events lie in a record ring (rec_ring.h)
// of TII_RING slots per stream, indexed by the stream's event count.
#include "engine.h"
#include <cstring>

namespace dabx {

void tii_stage_free(dabx_engine *e)
{
  TiiStage &T = e->tiis;
  hip_free_all({T.dev.pairs, T.dev.cfg, T.dev.ring, T.dev.cnt, T.tables});
  T = TiiStage{};
}

// the first enable: [S][768] pairs, a settings row, a ring of TII_RING event slots and the counters per stream, the detector's two tables
static int tii_stage_create(dabx_engine *e)
{
  TiiStage &T = e->tiis;
  const size_t S = (size_t)e->dev.n_streams;
  uint8_t tab[TII_PAIRS + 72];
  tii_tables_host(tab, tab + TII_PAIRS);
  if (int rc = alloc_zeroed("dabx_set_tii_mode", {{(void **)&T.dev.pairs, sizeof(float2) * TII_PAIRS * S}, {(void **)&T.dev.cfg, sizeof(TiiCfgDev) * S},
                                                  {(void **)&T.dev.ring, (size_t)TII_RING * TII_SLOT_BYTES * S}, {(void **)&T.dev.cnt, sizeof(TiiCounters) * S},
                                                  {(void **)&T.tables, sizeof(tab)}}))
    return rc;
  if (hipMemcpy(T.tables, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) { set_error("dabx_set_tii_mode: uploading the tables failed"); tii_stage_free(e); return DABX_E_HIP; }
  T.dev.turn = T.tables; T.dev.pattern = T.tables + TII_PAIRS;
  T.cfg.assign(S, TiiCfgDev{});
  T.seen.assign(S, 0);
  return 0;
}

}  // namespace dabx

extern "C" {

int dabx_set_tii_mode(dabx_engine *e, int stream, const dabx_tii_config *cfg)
{
  if (!e || stream < -1 || stream >= e->dev.n_streams) { set_error("dabx_set_tii_mode: bad argument"); return DABX_E_ARG; }
  const int min_frames = cfg && cfg->min_frames ? cfg->min_frames : 5, thr = cfg && cfg->threshold_db ? cfg->threshold_db : 8;
  const bool on = !cfg || cfg->enable;
  if (on && (min_frames < 1 || min_frames > 1 << 20 || thr < -100 || thr > 100)) {
    set_error("dabx_set_tii_mode: min_frames %d / threshold_db %d out of range", min_frames, thr);
    return DABX_E_ARG;
  }
  if (!e->dev.tii_acc) { set_error("dabx_set_tii_mode: engine has no TII accumulator"); return DABX_E_STATE; }
  int rc;
  if ((rc = sync_all(e))) return rc;
  TiiStage &T = e->tiis;
  if (!T.exists()) {
    if (!on) return 0;
    if ((rc = tii_stage_create(e))) return rc;
  }
  const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? e->dev.n_streams : stream + 1;
  for (int s = s0; s < s1; s++) {
    TiiCfgDev &c = T.cfg[(size_t)s];
    if (on) {
      if (!c.enable) {
        // the detector starts from TiiDetector's initial state, in the stream's current reset epoch; a sum the host path left behind is its first input
        int32_t cnt[2];
        DABX_HIP(hipMemcpy(cnt, e->dev.tii_cnt + 2 * s, sizeof(cnt), hipMemcpyDeviceToHost));
        DABX_HIP(hipMemset(T.dev.pairs + (size_t)s * TII_PAIRS, 0, sizeof(float2) * TII_PAIRS));
        c.epoch_seen = cnt[1];
      } else {
        DABX_HIP(hipMemcpy(&c.epoch_seen, &T.dev.cfg[s].epoch_seen, sizeof(int32_t), hipMemcpyDeviceToHost));    // the device's
      }
      c.enable = 1; c.min_frames = min_frames; c.threshold_db = thr; c.collisions = cfg && cfg->collisions ? 1 : 0;
      c.coll_sub_id = cfg ? cfg->collision_sub_id : 0; c.factor = tii_factor(thr); c.pad_ = 0;
    } else {
      c.enable = 0;
      // dabx_read_tii takes over: its host detector starts afresh too
      if (e->tii[(size_t)s]) { dabx_tii_destroy(e->tii[(size_t)s]); e->tii[(size_t)s] = nullptr; }
    }
    DABX_HIP(hipMemcpy(T.dev.cfg + s, &c, sizeof(c), hipMemcpyHostToDevice));
  }
  T.n_on = 0;
  for (const TiiCfgDev &c : T.cfg) T.n_on += c.enable;
  return 0;
}

int dabx_read_tii_events(dabx_engine *e, int stream, int max_events, dabx_tii_event *ev, dabx_tii_result *res, int32_t *lost)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || max_events < 0 || (max_events > 0 && !ev)) { set_error("dabx_read_tii_events: bad argument"); return DABX_E_ARG; }
  if (lost) *lost = 0;
  if (int rc = sync_all(e)) return rc;
  TiiStage &T = e->tiis;
  if (!T.exists()) return 0;
  TiiCounters c;
  DABX_HIP(hipMemcpy(&c, T.dev.cnt + stream, sizeof(c), hipMemcpyDeviceToHost));
  uint8_t slot[TII_SLOT_BYTES];
  return rec_ring_read<TII_RING, TII_SLOT_BYTES>(T.dev.ring, stream, c.events, T.seen[(size_t)stream], nullptr, max_events, lost,
                                                  [&](int n, const uint8_t *dev_slot) {
    DABX_HIP(hipMemcpy(slot, dev_slot, sizeof(slot), hipMemcpyDeviceToHost));
    memcpy(ev + n, slot, sizeof(dabx_tii_event));
    if (res) memcpy(res + (size_t)n * DABX_TII_MAX_RESULTS, slot + sizeof(dabx_tii_event), sizeof(dabx_tii_result) * DABX_TII_MAX_RESULTS);
    return 0;
  });
}

int dabx_get_tii_stats(dabx_engine *e, int stream, dabx_tii_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) { set_error("dabx_get_tii_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  if (int rc = sync_all(e)) return rc;
  const TiiStage &T = e->tiis;
  if (!T.exists()) return 0;
  TiiCounters c;
  DABX_HIP(hipMemcpy(&c, T.dev.cnt + stream, sizeof(c), hipMemcpyDeviceToHost));
  out->events = c.events; out->results = c.results; out->truncated = c.truncated; out->resets = c.resets; out->launches = T.launches;
  return 0;
}

}  // extern "C"
