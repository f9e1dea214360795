// engine_fig.cpp -- the FIC followed on the device (include/dabx.h dabx_set_fig_mode; fig_core.h, deliver.hip k_fig): the stage's memory, the
// per-stream switch, and the getters, each of which makes ONE device-to-host copy of the stream's decoder state (plus the label records or
// the event slots it returns) per call.  The events lie in a record ring (rec_ring.h) of FIG_RING slots per stream, indexed by the stream's
// event count.
#include "engine.h"
#include <cstring>

namespace dabx {

void fig_stage_free(dabx_engine *e)
{
  FigStage &T = e->fig;
  hip_free_all({T.dev.st, T.dev.labels, T.dev.ring, T.dev.on, T.dev.si, T.dev.si_on});
  for (hipEvent_t ev : T.timed) (void)hipEventDestroy(ev);
  T = FigStage{};
}

// the first enable: a decoder state, FIG_LAB_SLOTS label records, a ring of FIG_RING event slots and the switch per stream
static int fig_stage_create(dabx_engine *e)
{
  FigStage &T = e->fig;
  const size_t S = (size_t)e->dev.n_streams;
  if (int rc = alloc_zeroed("dabx_set_fig_mode", {{(void **)&T.dev.st, sizeof(FigState) * S}, {(void **)&T.dev.labels, sizeof(dabx_fig_label) * FIG_LAB_SLOTS * S},
                                                  {(void **)&T.dev.ring, sizeof(dabx_fig_event) * FIG_RING * S}, {(void **)&T.dev.on, sizeof(int32_t) * S}}))
    return rc;
  T.on.assign(S, 0);
  T.seen.assign(S, 0);
  return 0;
}

// the first service_info: a FigSiState and the switch per stream; k_fig_si takes k_fig's place from the next step on
static int fig_si_create(dabx_engine *e)
{
  FigStage &T = e->fig;
  const size_t S = (size_t)e->dev.n_streams;
  if (int rc = alloc_zeroed("dabx_set_fig_mode", {{(void **)&T.dev.si, sizeof(FigSiState) * S}, {(void **)&T.dev.si_on, sizeof(int32_t) * S}})) return rc;
  T.si_on.assign(S, 0);
  return 0;
}

int fig_step(dabx_engine *e)
{
  FigStage &T = e->fig;
  if (T.n_on <= 0) return 0;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (T.timing) {
    DABX_HIP(hipEventCreate(&t0));
    DABX_HIP(hipEventCreate(&t1));
    T.timed.push_back(t0); T.timed.push_back(t1);
    DABX_HIP(hipEventRecord(t0, e->stream));
  }
  FigDev dev = T.dev;
  if (T.n_si == 0) dev.si = nullptr;             // no stream follows the service information (any more): k_fig, which does not know of it
  if (int rc = launch_fig(e->dev, dev, e->stream)) return rc;
  if (T.timing) DABX_HIP(hipEventRecord(t1, e->stream));
  T.launches++;
  return 0;
}

static int fig_si_fetch(dabx_engine *e, int stream, const char *who, FigState *st, FigSiState *si);

// how every getter begins: the engine drained, the stream's decoder state on the host
static int fig_fetch(dabx_engine *e, int stream, const char *who, FigState *st)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams) { set_error("%s: bad argument", who); return DABX_E_ARG; }
  if (int rc = use_device(e)) return rc;
  if (!e->fig.on_for(stream)) { set_error("%s: stream %d does not follow the FIC on the device (dabx_set_fig_mode)", who, stream); return DABX_E_STATE; }
  if (int rc = sync_all(e)) return rc;
  DABX_HIP(hipMemcpy(st, e->fig.dev.st + stream, sizeof(FigState), hipMemcpyDeviceToHost));
  return 0;
}

// ... and how every SI getter begins: the stream's service information too (two copies: the two states lie apart)
static int fig_si_fetch(dabx_engine *e, int stream, const char *who, FigState *st, FigSiState *si)
{
  if (int rc = fig_fetch(e, stream, who, st)) return rc;
  if (!e->fig.si_for(stream)) { set_error("%s: stream %d does not follow the service information (dabx_fig_config.service_info)", who, stream); return DABX_E_STATE; }
  DABX_HIP(hipMemcpy(si, e->fig.dev.si + stream, sizeof(FigSiState), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace dabx

extern "C" {

int dabx_set_fig_mode(dabx_engine *e, int stream, const dabx_fig_config *cfg)
{
  if (!e || stream < -1 || stream >= e->dev.n_streams) { set_error("dabx_set_fig_mode: bad argument"); return DABX_E_ARG; }
  if (!e->dev.fib_out || !e->dev.fib_crc) { set_error("dabx_set_fig_mode: engine has no FIB ring"); return DABX_E_STATE; }
  const bool on = !cfg || cfg->enable, si = on && cfg && cfg->service_info;
  int rc;
  if ((rc = use_device(e))) return rc;
  if ((rc = sync_all(e))) return rc;
  FigStage &T = e->fig;
  if (!T.exists()) {
    if (!on) return 0;
    if ((rc = fig_stage_create(e))) return rc;
  }
  if (si && !T.dev.si && (rc = fig_si_create(e))) return rc;
  const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? e->dev.n_streams : stream + 1;
  FigState fresh;
  for (int s = s0; s < s1; s++) {
    if (T.dev.si) {
      // the service information goes with the decoder: a stream that switches it on (or starts afresh) begins with empty tables, one that is
      // enabled again with the switch as it was keeps them
      if (si && (!T.si_on[(size_t)s] || !T.on[(size_t)s])) DABX_HIP(hipMemset(T.dev.si + s, 0, sizeof(FigSiState)));
      T.si_on[(size_t)s] = si ? 1 : 0;
    }
    if (on) {
      // a fresh decoder; the kernel sets its FIB count to that of the first frame it walks, as dabx_follow_fic's decoder skips the frames before it.
      // An enabled stream that is enabled again keeps its database but takes the new swap rule.
      if (!T.on[(size_t)s]) {
        fig_state_init(fresh, cfg && cfg->reference_quirks ? 1 : 0, 0);
        DABX_HIP(hipMemcpy(T.dev.st + s, &fresh, sizeof(fresh), hipMemcpyHostToDevice));
        T.seen[(size_t)s] = 0;
        // dabx_follow_fic's decoder of the stream would be stale by the time the mode goes off again: it starts afresh then
        if (e->fibdec[(size_t)s]) { dabx_fibdec_destroy(e->fibdec[(size_t)s]); e->fibdec[(size_t)s] = nullptr; }
      } else {
        const int32_t strict = cfg && cfg->reference_quirks ? 1 : 0;
        DABX_HIP(hipMemcpy(&T.dev.st[s].strict, &strict, sizeof(strict), hipMemcpyHostToDevice));
      }
      T.on[(size_t)s] = 1;
    } else {
      T.on[(size_t)s] = 0;
    }
  }
  DABX_HIP(hipMemcpy(T.dev.on, T.on.data(), sizeof(int32_t) * T.on.size(), hipMemcpyHostToDevice));
  if (T.dev.si) DABX_HIP(hipMemcpy(T.dev.si_on, T.si_on.data(), sizeof(int32_t) * T.si_on.size(), hipMemcpyHostToDevice));
  T.n_on = 0;
  for (int32_t v : T.on) T.n_on += v;
  T.n_si = 0;
  for (int32_t v : T.si_on) T.n_si += v;
  return 0;
}

int dabx_fig_info(dabx_engine *e, int stream, dabx_fibdec_info *out)
{
  FigState st;
  if (!out) { set_error("dabx_fig_info: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_fetch(e, stream, "dabx_fig_info", &st)) return rc;
  fig_info(st, out);
  return 0;
}

int dabx_fig_subchannels(dabx_engine *e, int stream, int next, dabx_subch_desc *out, int max_out)
{
  FigState st;
  if ((!out && max_out > 0) || max_out < 0) { set_error("dabx_fig_subchannels: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_fetch(e, stream, "dabx_fig_subchannels", &st)) return rc;
  return fig_subchannels(st, next, out, max_out);
}

int dabx_fig_packet_components(dabx_engine *e, int stream, int next, dabx_packet_component *out, int max_out)
{
  FigState st;
  if ((!out && max_out > 0) || max_out < 0) { set_error("dabx_fig_packet_components: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_fetch(e, stream, "dabx_fig_packet_components", &st)) return rc;
  return fig_packet_components(st, next, out, max_out);
}

int dabx_fig_follow(dabx_engine *e, int stream, dabx_reconf *out)
{
  FigState st;
  if (!out) { set_error("dabx_fig_follow: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_fetch(e, stream, "dabx_fig_follow", &st)) return rc;
  fig_follow(st, out);
  // frames_fed as dabx_follow_fic reports it: the frames the stream has decoded (a decoder that has walked none yet counts none of its own)
  StreamCtl c;
  DABX_HIP(hipMemcpy(&c, e->dev.ctl + stream, sizeof(StreamCtl), hipMemcpyDeviceToHost));
  out->frames_fed = c.frames;
  return 0;
}

int dabx_fig_labels(dabx_engine *e, int stream, dabx_fig_label *out, int max_out)
{
  FigState st;
  if ((!out && max_out > 0) || max_out < 0) { set_error("dabx_fig_labels: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_fetch(e, stream, "dabx_fig_labels", &st)) return rc;
  const int n = st.n_labels < max_out ? st.n_labels : max_out;
  if (n > 0) DABX_HIP(hipMemcpy(out, e->fig.dev.labels + (size_t)stream * FIG_LAB_SLOTS, sizeof(dabx_fig_label) * (size_t)n, hipMemcpyDeviceToHost));
  return n;
}

int dabx_get_fig_stats(dabx_engine *e, int stream, dabx_fig_stats *out)
{
  if (!e || stream < 0 || stream >= e->dev.n_streams || !out) { set_error("dabx_get_fig_stats: bad argument"); return DABX_E_ARG; }
  memset(out, 0, sizeof(*out));
  if (!e->fig.on_for(stream)) { out->launches = e->fig.launches; return 0; }
  FigState st;
  if (int rc = fig_fetch(e, stream, "dabx_get_fig_stats", &st)) return rc;
  *out = st.cnt;
  out->launches = e->fig.launches;
  return 0;
}

// ---- the service information (include/dabx.h "Service information"): each getter one copy of the stream's two states ----
int dabx_fig_si_info(dabx_engine *e, int stream, dabx_fig_si_scalars *out)
{
  FigState st;
  FigSiState si;
  if (!out) { set_error("dabx_fig_si_info: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_si_fetch(e, stream, "dabx_fig_si_info", &st, &si)) return rc;
  fig_si_info(st, si, out);
  return 0;
}

#define DABX_FIG_SI_GETTER(name, type, call)                                                                                   \
  int name(dabx_engine *e, int stream, int next, type *out, int max_out)                                                       \
  {                                                                                                                            \
    FigState st;                                                                                                               \
    FigSiState si;                                                                                                             \
    if ((!out && max_out > 0) || max_out < 0) { set_error(#name ": bad argument"); return DABX_E_ARG; }                        \
    if (int rc = fig_si_fetch(e, stream, #name, &st, &si)) return rc;                                                          \
    return call;                                                                                                               \
  }
DABX_FIG_SI_GETTER(dabx_fig_user_apps, dabx_fig_user_apps_entry, fig_si_user_apps(st, si, next, out, max_out))
DABX_FIG_SI_GETTER(dabx_fig_global_defs, dabx_fig_global_def, fig_si_global_defs(st, si, next, out, max_out))
DABX_FIG_SI_GETTER(dabx_fig_fec_schemes, dabx_fig_fec_scheme, fig_si_fec(st, si, next, out, max_out))
DABX_FIG_SI_GETTER(dabx_fig_clusters, dabx_fig_cluster, fig_si_clusters(st, si, next, out, max_out))
#undef DABX_FIG_SI_GETTER

int dabx_fig_languages(dabx_engine *e, int stream, dabx_fig_language *out, int max_out)
{
  FigState st;
  FigSiState si;
  if ((!out && max_out > 0) || max_out < 0) { set_error("dabx_fig_languages: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_si_fetch(e, stream, "dabx_fig_languages", &st, &si)) return rc;
  return fig_si_languages(si, out, max_out);
}

int dabx_fig_programme_types(dabx_engine *e, int stream, dabx_fig_programme_type *out, int max_out)
{
  FigState st;
  FigSiState si;
  if ((!out && max_out > 0) || max_out < 0) { set_error("dabx_fig_programme_types: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_si_fetch(e, stream, "dabx_fig_programme_types", &st, &si)) return rc;
  return fig_si_ptys(si, out, max_out);
}

int dabx_get_fig_si_stats(dabx_engine *e, int stream, dabx_fig_si_stats *out)
{
  FigState st;
  FigSiState si;
  if (!out) { set_error("dabx_get_fig_si_stats: bad argument"); return DABX_E_ARG; }
  if (int rc = fig_si_fetch(e, stream, "dabx_get_fig_si_stats", &st, &si)) return rc;
  *out = si.cnt;
  return 0;
}

// One launch of k_fig_directory over the streams asked for, one copy of their records and one of their counts
int dabx_fig_directory(dabx_engine *e, int stream, int next, dabx_fig_service *out, int max_per_stream, int32_t *n_out)
{
  if (!e || stream < -1 || stream >= e->dev.n_streams || !n_out || max_per_stream < 0 || (max_per_stream > 0 && !out)) {
    set_error("dabx_fig_directory: bad argument");
    return DABX_E_ARG;
  }
  if (int rc = use_device(e)) return rc;
  FigStage &T = e->fig;
  if (stream >= 0 ? !T.si_for(stream) : T.n_si == 0) {
    set_error("dabx_fig_directory: %s not follow the service information (dabx_fig_config.service_info)", stream >= 0 ? "the stream does" : "the engine's streams do");
    return DABX_E_STATE;
  }
  if (int rc = sync_all(e)) return rc;
  const int first = stream < 0 ? 0 : stream, n = stream < 0 ? e->dev.n_streams : 1;
  const int max_per = max_per_stream < FIG_MAX_COMP ? max_per_stream : FIG_MAX_COMP;
  dabx_fig_service *drec = nullptr;
  int32_t *dn = nullptr;
  if (int rc = alloc_zeroed("dabx_fig_directory", {{(void **)&drec, sizeof(dabx_fig_service) * (size_t)n * (size_t)(max_per > 0 ? max_per : 1)}, {(void **)&dn, sizeof(int32_t) * (size_t)n}}))
    return rc;
  // (the zeroing ran on the null stream, which the engine's stream does not wait for: it has to be through before the kernel writes)
  if (hipError_t he0 = hipStreamSynchronize(nullptr); he0 != hipSuccess) {
    hip_free_all({drec, dn});
    set_error("dabx_fig_directory: HIP error %d (%s)", (int)he0, hipGetErrorString(he0));
    return DABX_E_HIP;
  }
  int rc = launch_fig_directory(T.dev.st, T.dev.si, T.dev.labels, T.dev.si_on, first, n, next ? 1 : 0, drec, max_per, max_per, dn, 1, e->stream);
  hipError_t he = rc ? hipSuccess : hipStreamSynchronize(e->stream);
  if (!rc && he == hipSuccess) he = hipMemcpy(n_out, dn, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost);
  if (!rc && he == hipSuccess && max_per > 0) {
    // the caller's rows are max_per_stream apart, the device's max_per: one copy when they agree (they do unless the caller asks for more than a table holds)
    if (max_per == max_per_stream) he = hipMemcpy(out, drec, sizeof(dabx_fig_service) * (size_t)n * (size_t)max_per, hipMemcpyDeviceToHost);
    else he = hipMemcpy2D(out, sizeof(dabx_fig_service) * (size_t)max_per_stream, drec, sizeof(dabx_fig_service) * (size_t)max_per,
                          sizeof(dabx_fig_service) * (size_t)max_per, (size_t)n, hipMemcpyDeviceToHost);
  }
  hip_free_all({drec, dn});
  if (!rc && he != hipSuccess) { set_error("dabx_fig_directory: HIP error %d (%s)", (int)he, hipGetErrorString(he)); return DABX_E_HIP; }
  return rc;
}

int dabx_read_fig_events(dabx_engine *e, int stream, int max_events, dabx_fig_event *ev, int32_t *lost)
{
  if (max_events < 0 || (max_events > 0 && !ev)) { set_error("dabx_read_fig_events: bad argument"); return DABX_E_ARG; }
  if (lost) *lost = 0;
  FigState st;
  if (int rc = fig_fetch(e, stream, "dabx_read_fig_events", &st)) return rc;
  FigStage &T = e->fig;
  return rec_ring_read<FIG_RING, FIG_SLOT_BYTES>(reinterpret_cast<const uint8_t *>(T.dev.ring), stream, st.cnt.events, T.seen[(size_t)stream], nullptr,
                                                 max_events, lost, [&](int n, const uint8_t *dev_slot) {
    DABX_HIP(hipMemcpy(ev + n, dev_slot, sizeof(dabx_fig_event), hipMemcpyDeviceToHost));
    return 0;
  });
}

// Measuring entry (tools/bench_fig.py; not part of include/dabx.h): on = 1, every k_fig launch from now on lies between two events of its own
// (a packet in front of and behind the kernel: the step is a little slower while this is on); on = 0, the engine is drained, the launches' times
// go to ms[0 .. max), oldest first, and the events are freed.  Returns the number of launches that were timed.
int dabx_internal_fig_timing(dabx_engine *e, int on, float *ms, int max)
{
  if (!e || (max > 0 && !ms) || max < 0) { set_error("dabx_internal_fig_timing: bad argument"); return DABX_E_ARG; }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  FigStage &T = e->fig;
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
