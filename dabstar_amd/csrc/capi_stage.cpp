// capi_stage.cpp -- stage-level C ABI (host-pointer entry points mirroring single reference functions).
#include <algorithm>
#include "dabx_internal.h"
#include "eti_core.h"
#include "tii_core.h"
#include "mp2_core.h"
#include "aac_core.h"
#include "spectrum_core.h"
#include "fig_core.h"
#include "data_core.h"
#include <cstring>
#include <vector>

namespace dabx { const char *last_error(); }
using namespace dabx;

namespace {
// RAII device buffer for the host-pointer convenience entry points
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t n) { DABX_HIP(hipMalloc(&p, n ? n : 1)); return 0; }
  int from_host(const void *h, size_t n) { int rc = alloc(n); if (rc) return rc; DABX_HIP(hipMemcpy(p, h, n, hipMemcpyHostToDevice)); return 0; }
  int to_host(void *h, size_t n) { DABX_HIP(hipMemcpy(h, p, n, hipMemcpyDeviceToHost)); return 0; }
  template <class T> T *as() { return reinterpret_cast<T *>(p); }
};
int need_device()
{
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) { set_error("no HIP device available (libdabx has no CPU fallback)"); return DABX_E_NODEVICE; }
  return 0;
}
}  // namespace

extern "C" {

const char *dabx_last_error(void) { return dabx::last_error(); }
int dabx_abi_version(void) { return DABX_ABI_VERSION; }
#ifndef DABX_HIPMODULE
// 0: the kernels are in this library's fat binary (default build); 1 in the hipModule form (csrc/hipmodule/hipmodule_rt.cpp)
int dabx_internal_hipmodule(void) { return 0; }
#endif
// Test entry of the MP2 audio stage (tests/test_mp2_audio_cases.py; not part of include/dabx.h): _mp2_decode_frame behind its counters on
// the HOST, through the kernel's own pieces lane after lane (mp2_core.h, mp2a_decode_host).  frame: MP2frame as the device keeps it,
// 6 kbps bytes; hist: [2][16][64] int32, the V rows of the 16 newest sub-blocks per channel, oldest first, in and out; pcm: [2304] int16.
// Returns the frame size, 0 where the decoder returns 0 (*status: 1 = :397-402, 2 = :412-421); *over: guard G1.  Needs no device.
int dabx_internal_mp2_decode_host(const uint8_t *frame, int kbps, int32_t *hist, int16_t *pcm, int32_t *status, int32_t *over)
{
  if (!frame || !hist || !pcm || !status || !over || kbps < 8 || kbps > MP2A_MAX_KBPS || kbps % 8 != 0) { set_error("dabx_internal_mp2_decode_host: bad argument"); return DABX_E_ARG; }
  int st = 0, ov = 0;
  const int size = mp2a_decode_host(frame, 6 * kbps, 48 * kbps, hist, pcm, &st, &ov);
  *status = st; *over = ov;
  return size;
}

// Test entry of the AAC stream stage (tests/test_aac_stream_cases.py; not part of include/dabx.h): the LOAS frame of ONE access unit on the
// HOST, through the kernel's own header and copy pieces lane after lane (aac_core.h, aac_frame_host).  au: the L <= 960 payload bytes;
// stream_parms as dabx_superframe_info holds them; out: room for DABX_AAC_MAX_FRAME_BYTES.  Returns the frame's size.  Needs no device.
int dabx_internal_aac_frame_host(const uint8_t *au, int L, int stream_parms, uint8_t *out)
{
  if ((!au && L > 0) || !out || L < 0 || L > AAC_MAX_AU_BYTES || stream_parms < 0 || stream_parms > 0x7F) { set_error("dabx_internal_aac_frame_host: bad argument"); return DABX_E_ARG; }
  return aac_frame_host(au, L, (unsigned)stream_parms, out);
}

int dabx_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
int dabx_set_device(int device)
{
  int rc = need_device();
  if (rc) return rc;
  DABX_HIP(hipSetDevice(device));
  return 0;
}

int dabx_viterbi(const int16_t *soft, int nbits, int batch, uint8_t *bits) { return dabx_viterbi_mode(soft, nbits, batch, 0, bits); }

int dabx_viterbi_mode(const int16_t *soft, int nbits, int batch, int tie_mode, uint8_t *bits)
{
  if (!soft || !bits || nbits <= 0 || batch <= 0 || tie_mode < 0 || tie_mode > 2) { set_error("dabx_viterbi: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf dsoft, dbits;
  const size_t nin = (size_t)batch * 4 * (nbits + 6);
  if ((rc = dsoft.from_host(soft, nin * 2))) return rc;
  if ((rc = dbits.alloc((size_t)batch * nbits))) return rc;
  if ((rc = launch_viterbi_i16(dsoft.as<int16_t>(), nbits, batch, dbits.as<uint8_t>(), 0, tie_mode))) return rc;
  return dbits.to_host(bits, (size_t)batch * nbits);
}

int dabx_profile_input_bits(int kbps, int prot_level, int short_form)
{
  std::vector<uint16_t> m;
  int n = 0;
  const int rc = host_profile_map(kbps, prot_level, short_form, m, &n);
  return rc ? rc : n;
}

// Host only: the depuncture index list itself (mother-code bit i <- transmitted bit map[i], 0xFFFF = punctured), the table
// the device kernels gather through; length 96*kbps + 24.  Returns the number of transmitted bits.
int dabx_profile_map(int kbps, int prot_level, int short_form, uint16_t *map, int max_entries)
{
  std::vector<uint16_t> m;
  int n = 0;
  const int rc = host_profile_map(kbps, prot_level, short_form, m, &n);
  if (rc) return rc;
  if (!map || max_entries < (int)m.size()) { set_error("dabx_profile_map: need room for %d entries", (int)m.size()); return DABX_E_ARG; }
  std::copy(m.begin(), m.end(), map);
  return n;
}

int dabx_deconvolve(const int16_t *in, int in_stride, int kbps, int prot_level, int short_form, int batch, uint8_t *bits)
{
  if (!in || !bits || batch <= 0) { set_error("dabx_deconvolve: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  const uint16_t *map = nullptr;
  int n_in = 0;
  if ((rc = get_profile_map(kbps, prot_level, short_form, &map, &n_in))) return rc;
  if (in_stride < n_in) { set_error("dabx_deconvolve: stride %d < %d input bits", in_stride, n_in); return DABX_E_ARG; }
  const int nbits = 24 * kbps;
  DevBuf din, dbits;
  if ((rc = din.from_host(in, (size_t)batch * in_stride * 2))) return rc;
  if ((rc = dbits.alloc((size_t)batch * nbits))) return rc;
  if ((rc = launch_deconvolve_i16(din.as<int16_t>(), in_stride, map, nbits, batch, dbits.as<uint8_t>(), 0))) return rc;
  return dbits.to_host(bits, (size_t)batch * nbits);
}

int dabx_rs_decode(const uint8_t *in, int batch, uint8_t *out, int16_t *ret)
{
  if (!in || !out || !ret || batch <= 0) { set_error("dabx_rs_decode: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf din, dout, dret;
  if ((rc = din.from_host(in, (size_t)batch * 120))) return rc;
  if ((rc = dout.alloc((size_t)batch * 110))) return rc;
  if ((rc = dret.alloc((size_t)batch * 2))) return rc;
  if ((rc = launch_rs_decode(din.as<uint8_t>(), batch, dout.as<uint8_t>(), dret.as<int16_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  if ((rc = dout.to_host(out, (size_t)batch * 110))) return rc;
  return dret.to_host(ret, (size_t)batch * 2);
}

static int firecode_common(uint8_t *x, int batch, uint8_t *ok, int correct)
{
  if (!x || !ok || batch <= 0) { set_error("dabx_firecode: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf dx, dok;
  if ((rc = dx.from_host(x, (size_t)batch * 12))) return rc;
  if ((rc = dok.alloc((size_t)batch))) return rc;
  if ((rc = launch_firecode(dx.as<uint8_t>(), batch, correct, dok.as<uint8_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  if (correct && (rc = dx.to_host(x, (size_t)batch * 12))) return rc;
  return dok.to_host(ok, (size_t)batch);
}
int dabx_firecode_check(const uint8_t *x, int batch, uint8_t *ok) { return firecode_common(const_cast<uint8_t *>(x), batch, ok, 0); }
int dabx_firecode_check_and_correct(uint8_t *x, int batch, uint8_t *ok) { return firecode_common(x, batch, ok, 1); }

int dabx_crc16_check(const uint8_t *msgs, int stride, int len, int batch, uint8_t *ok)
{
  if (!msgs || !ok || batch <= 0 || len < 0 || stride < len + 2) { set_error("dabx_crc16_check: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf dm, dok;
  if ((rc = dm.from_host(msgs, (size_t)batch * stride))) return rc;
  if ((rc = dok.alloc((size_t)batch))) return rc;
  if ((rc = launch_crc16_check(dm.as<uint8_t>(), stride, len, batch, dok.as<uint8_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return dok.to_host(ok, (size_t)batch);
}

// ETI(NI) frames on the device: eti_build_frame (eti_core.h), the body of the delivery's ETI stage, one wave per frame
int dabx_eti_frames_device(int n, const int32_t *cif_hi, const int32_t *cif_lo, const int32_t *minor, const dabx_subch_desc *sc, int n_subch,
                           const uint8_t *fic96, const uint8_t *msc, uint8_t *out, int32_t *used)
{
  if (n <= 0 || !cif_hi || !cif_lo || !minor || n_subch < 0 || n_subch > 64 || (n_subch && (!sc || !msc)) || !fic96 || !out || !used) {
    set_error("dabx_eti_frames_device: bad argument");
    return DABX_E_ARG;
  }
  for (int f = 0; f < n; f++)
    if (cif_hi[f] < 0 || cif_lo[f] < 0 || minor[f] < 0 || minor[f] > 3) { set_error("dabx_eti_frames_device: bad counter of frame %d", f); return DABX_E_ARG; }
  std::vector<uint32_t> stc((size_t)std::max(1, n_subch));
  std::vector<int32_t> ndw(stc.size()), off(stc.size());
  int sum_kbps = 0;
  for (int i = 0; i < n_subch; i++) {
    const dabx_subch_desc &q = sc[i];
    const bool lvl_ok = q.short_form ? (q.prot_level >= 1 && q.prot_level <= 5) : (q.prot_level >= 0 && q.prot_level <= 7);
    if (!lvl_ok || q.subch_id < 0 || q.subch_id > 63 || q.cu_start < 0 || q.cu_start > 863 || q.kbps <= 0 || q.kbps > 1023 || q.kbps % 8) {
      set_error("dabx_eti_frames_device: sub-channel %d is not a legal description (kbps a multiple of 8)", i);
      return DABX_E_ARG;
    }
    stc[(size_t)i] = eti_stc_word(q.subch_id, q.cu_start, q.kbps, q.prot_level, q.short_form);
    ndw[(size_t)i] = 3 * q.kbps / 4; off[(size_t)i] = 3 * sum_kbps / 4;
    sum_kbps += q.kbps;
  }
  if (eti_used_bytes(n_subch, sum_kbps) > DABX_ETI_FRAME_BYTES) {
    set_error("dabx_eti_frames_device: %d bytes of sub-channel data do not fit an ETI frame", 96 + 3 * sum_kbps);
    return DABX_E_ARG;
  }
  int rc = need_device();
  if (rc) return rc;
  const size_t N = (size_t)n, row = (size_t)3 * sum_kbps;
  DevBuf dhi, dlo, dmi, dstc, dndw, doff, dfic, dmsc, dout, dused;
  if ((rc = dhi.from_host(cif_hi, 4 * N)) || (rc = dlo.from_host(cif_lo, 4 * N)) || (rc = dmi.from_host(minor, 4 * N)) ||
      (rc = dstc.from_host(stc.data(), 4 * stc.size())) || (rc = dndw.from_host(ndw.data(), 4 * ndw.size())) ||
      (rc = doff.from_host(off.data(), 4 * off.size())) || (rc = dfic.from_host(fic96, 96 * N)) ||
      (rc = row ? dmsc.from_host(msc, row * N) : dmsc.alloc(4)) || (rc = dout.alloc((size_t)DABX_ETI_FRAME_BYTES * N)) || (rc = dused.alloc(4 * N))) return rc;
  if ((rc = launch_eti_frames(n, dhi.as<int32_t>(), dlo.as<int32_t>(), dmi.as<int32_t>(), n_subch, dstc.as<uint32_t>(), dndw.as<int32_t>(),
                              doff.as<int32_t>(), (int)(row / 4), dfic.as<uint32_t>(), dmsc.as<uint32_t>(), dout.as<uint32_t>(), dused.as<int32_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  if ((rc = dout.to_host(out, (size_t)DABX_ETI_FRAME_BYTES * N))) return rc;
  return dused.to_host(used, 4 * N);
}

// The TII detector on the device: tii_detect (tii_core.h), the body of the engine's k_tii, one block per detector
int dabx_tii_process_device(int n, const float *sums, float *pairs, const dabx_tii_config *cfg, dabx_tii_result *out, int32_t *n_results, int32_t *n_found)
{
  if (n <= 0 || !sums || !pairs || !cfg || !out || !n_results || !n_found) { set_error("dabx_tii_process_device: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  const size_t N = (size_t)n;
  std::vector<TiiCfgDev> c(N);
  for (size_t d = 0; d < N; d++) {
    const int thr = cfg[d].threshold_db ? cfg[d].threshold_db : 8;
    c[d] = TiiCfgDev{cfg[d].enable ? 1 : 0, 1, thr, cfg[d].collisions ? 1 : 0, cfg[d].collision_sub_id, 0, tii_factor(thr), 0};
  }
  uint8_t tab[TII_PAIRS + 72];
  tii_tables_host(tab, tab + TII_PAIRS);
  // (the outputs travel both ways: a detector with enable = 0 leaves its rows as the caller has them)
  DevBuf dsum, dpairs, dcfg, dtab, dout, dnr, dnf;
  if ((rc = dsum.from_host(sums, sizeof(float2) * TU * N)) || (rc = dpairs.from_host(pairs, sizeof(float2) * TII_PAIRS * N)) ||
      (rc = dcfg.from_host(c.data(), sizeof(TiiCfgDev) * N)) || (rc = dtab.from_host(tab, sizeof(tab))) ||
      (rc = dout.from_host(out, sizeof(dabx_tii_result) * DABX_TII_MAX_RESULTS * N)) || (rc = dnr.from_host(n_results, 4 * N)) ||
      (rc = dnf.from_host(n_found, 4 * N))) return rc;
  if ((rc = launch_tii_batch(n, dsum.as<float2>(), dpairs.as<float2>(), dcfg.as<TiiCfgDev>(), dtab.as<uint8_t>(), dtab.as<uint8_t>() + TII_PAIRS,
                             dout.as<dabx_tii_result>(), dnr.as<int32_t>(), dnf.as<int32_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  if ((rc = dpairs.to_host(pairs, sizeof(float2) * TII_PAIRS * N)) || (rc = dout.to_host(out, sizeof(dabx_tii_result) * DABX_TII_MAX_RESULTS * N)) ||
      (rc = dnr.to_host(n_results, 4 * N))) return rc;
  return dnf.to_host(n_found, 4 * N);
}

// The FIG walk on the device: fig_walk_fib (fig_core.h), the body of the engine's k_fig, one wave per decoder.  With `si` the decoders follow
// the service information too (fig_si_core.h, k_fig_si_batch) and k_fig_directory joins both configurations of each.
struct FigSiOuts {                               // one decoder's rows of dabx_fig_si_walk_device's SI outputs, every one optional
  dabx_fig_si_scalars *info; dabx_fig_si_stats *stats; dabx_fig_global_def *gd; dabx_fig_user_apps_entry *ua; dabx_fig_fec_scheme *fec; dabx_fig_cluster *cl;
  dabx_fig_language *lang; dabx_fig_programme_type *pty; int32_t *n_dir; dabx_fig_service *dir;
  FigSiOuts row(size_t d) const
  {
    return FigSiOuts{info ? info + d : nullptr, stats ? stats + d : nullptr, gd ? gd + 2 * SI_MAX_GD * d : nullptr, ua ? ua + 2 * SI_MAX_UA * d : nullptr,
                     fec ? fec + 2 * SI_MAX_FEC * d : nullptr, cl ? cl + 2 * SI_MAX_CL * d : nullptr, lang ? lang + SI_MAX_LANG * d : nullptr,
                     pty ? pty + SI_MAX_PTY * d : nullptr, n_dir ? n_dir + 2 * d : nullptr, dir ? dir + 2 * (size_t)FIG_MAX_COMP * d : nullptr};
  }
};
// the tables of one decoder (not its directory)
static void fig_si_present(const FigState &t, const FigSiState &s, const FigSiOuts &o)
{
  if (o.info) fig_si_info(t, s, o.info);
  if (o.stats) *o.stats = s.cnt;
  for (int k = 0; k < 2; k++) {
    if (o.gd) fig_si_global_defs(t, s, k, o.gd + (size_t)k * SI_MAX_GD, SI_MAX_GD);
    if (o.ua) fig_si_user_apps(t, s, k, o.ua + (size_t)k * SI_MAX_UA, SI_MAX_UA);
    if (o.fec) fig_si_fec(t, s, k, o.fec + (size_t)k * SI_MAX_FEC, SI_MAX_FEC);
    if (o.cl) fig_si_clusters(t, s, k, o.cl + (size_t)k * SI_MAX_CL, SI_MAX_CL);
  }
  if (o.lang) fig_si_languages(s, o.lang, SI_MAX_LANG);
  if (o.pty) fig_si_ptys(s, o.pty, SI_MAX_PTY);
}

static int fig_walk_device(const char *who, const uint8_t *fibs, const uint8_t *crc_ok, int n_decoders, int n_fibs, int reference_quirks, dabx_fibdec_info *info,
                           int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets, int32_t *n_labels, dabx_fig_label *labels,
                           dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events, const FigSiOuts *si)
{
  if (!fibs || !crc_ok || n_decoders <= 0 || n_decoders > 65535 || n_fibs <= 0 || n_fibs > 1 << 20) { set_error("%s: bad argument", who); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  const size_t N = (size_t)n_decoders;
  std::vector<FigDecoder> dec(N);
  for (FigDecoder &d : dec) { memset(&d, 0, sizeof(d)); fig_state_init(d.st, reference_quirks ? 1 : 0, 0); }
  std::vector<FigState> st(N);
  for (size_t d = 0; d < N; d++) st[d] = dec[d].st;
  DevBuf dfib, dcrc, dst, dlab, dring, dsi, ddir, dndir;
  if ((rc = dfib.from_host(fibs, N * n_fibs * 32)) || (rc = dcrc.from_host(crc_ok, N * n_fibs)) || (rc = dst.from_host(st.data(), sizeof(FigState) * N)) ||
      (rc = dlab.alloc(sizeof(dabx_fig_label) * FIG_LAB_SLOTS * N)) || (rc = dring.alloc(sizeof(dabx_fig_event) * FIG_RING * N))) return rc;
  DABX_HIP(hipMemset(dlab.p, 0, sizeof(dabx_fig_label) * FIG_LAB_SLOTS * N));
  DABX_HIP(hipMemset(dring.p, 0, sizeof(dabx_fig_event) * FIG_RING * N));
  if (si) {
    if ((rc = dsi.alloc(sizeof(FigSiState) * N)) || (rc = ddir.alloc(sizeof(dabx_fig_service) * 2 * FIG_MAX_COMP * N)) || (rc = dndir.alloc(sizeof(int32_t) * 2 * N))) return rc;
    DABX_HIP(hipMemset(dsi.p, 0, sizeof(FigSiState) * N));                  // fig_si_state_init
    DABX_HIP(hipMemset(ddir.p, 0, sizeof(dabx_fig_service) * 2 * FIG_MAX_COMP * N));
  }
  if ((rc = launch_fig_batch(dfib.as<uint8_t>(), dcrc.as<uint8_t>(), n_decoders, n_fibs, dst.as<FigState>(), si ? dsi.as<FigSiState>() : nullptr,
                             dlab.as<dabx_fig_label>(), dring.as<dabx_fig_event>(), 0))) return rc;
  for (int k = 0; si && k < 2; k++)
    if ((rc = launch_fig_directory(dst.as<FigState>(), dsi.as<FigSiState>(), dlab.as<dabx_fig_label>(), nullptr, 0, n_decoders, k,
                                   ddir.as<dabx_fig_service>() + (size_t)k * FIG_MAX_COMP, 2 * FIG_MAX_COMP, FIG_MAX_COMP, dndir.as<int32_t>() + k, 2, 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  if ((rc = dst.to_host(st.data(), sizeof(FigState) * N))) return rc;
  std::vector<FigSiState> sis(si ? N : 0);
  if (si) {
    if ((rc = dsi.to_host(sis.data(), sizeof(FigSiState) * N))) return rc;
    if (si->n_dir && (rc = dndir.to_host(si->n_dir, sizeof(int32_t) * 2 * N))) return rc;
    if (si->dir && (rc = ddir.to_host(si->dir, sizeof(dabx_fig_service) * 2 * FIG_MAX_COMP * N))) return rc;
  }
  for (size_t d = 0; d < N; d++) {
    dec[d].st = st[d];
    DABX_HIP(hipMemcpy(dec[d].labels, dlab.as<dabx_fig_label>() + d * FIG_LAB_SLOTS, sizeof(dec[d].labels), hipMemcpyDeviceToHost));
    DABX_HIP(hipMemcpy(dec[d].ring, dring.as<dabx_fig_event>() + d * FIG_RING, sizeof(dec[d].ring), hipMemcpyDeviceToHost));
    fig_present(dec[d], info ? info + d : nullptr, n_tab ? n_tab + 6 * d : nullptr, subch ? subch + 2 * FIG_MAX_SUB * d : nullptr,
                packets ? packets + 2 * FIG_MAX_PKT * d : nullptr, n_labels ? n_labels + d : nullptr, labels ? labels + FIG_LAB_SLOTS * d : nullptr,
                stats ? stats + d : nullptr, n_events ? n_events + d : nullptr, events ? events + FIG_RING * d : nullptr);
    if (si) fig_si_present(st[d], sis[d], si->row(d));
  }
  return 0;
}

int dabx_fig_walk_device(const uint8_t *fibs, const uint8_t *crc_ok, int n_decoders, int n_fibs, int reference_quirks, dabx_fibdec_info *info,
                         int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets, int32_t *n_labels, dabx_fig_label *labels,
                         dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events)
{
  return fig_walk_device("dabx_fig_walk_device", fibs, crc_ok, n_decoders, n_fibs, reference_quirks, info, n_tab, subch, packets, n_labels, labels, stats, n_events,
                         events, nullptr);
}

int dabx_fig_si_walk_device(const uint8_t *fibs, const uint8_t *crc_ok, int n_decoders, int n_fibs, int reference_quirks, dabx_fibdec_info *info,
                            int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets, int32_t *n_labels, dabx_fig_label *labels,
                            dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events, dabx_fig_si_scalars *si_info, dabx_fig_si_stats *si_stats,
                            dabx_fig_global_def *global_defs, dabx_fig_user_apps_entry *user_apps, dabx_fig_fec_scheme *fec, dabx_fig_cluster *clusters,
                            dabx_fig_language *languages, dabx_fig_programme_type *ptys, int32_t *n_dir, dabx_fig_service *dir)
{
  const FigSiOuts si{si_info, si_stats, global_defs, user_apps, fec, clusters, languages, ptys, n_dir, dir};
  return fig_walk_device("dabx_fig_si_walk_device", fibs, crc_ok, n_decoders, n_fibs, reference_quirks, info, n_tab, subch, packets, n_labels, labels, stats,
                         n_events, events, &si);
}

// Test entries of the FIG walk (tests/test_fig_cases.py; not part of include/dabx.h): the HOST build of fig_walk_fib on a decoder the caller
// keeps as bytes.  dabx_internal_fig_host_bytes: the size of one; _init: a fresh decoder; _walk: n_fibs FIBs of 32 bytes with their CRC
// verdicts; _read: the decoder presented as one row of dabx_fig_walk_device's outputs.  Needs no device.
int dabx_internal_fig_host_bytes(void) { return (int)sizeof(FigDecoder); }
int dabx_internal_fig_host_init(void *dec, int reference_quirks)
{
  if (!dec) return DABX_E_ARG;
  FigDecoder *d = static_cast<FigDecoder *>(dec);
  memset(d, 0, sizeof(*d));
  fig_state_init(d->st, reference_quirks ? 1 : 0, 0);
  return 0;
}
int dabx_internal_fig_host_walk(void *dec, const uint8_t *fibs, const uint8_t *crc_ok, int n_fibs)
{
  if (!dec || !fibs || !crc_ok || n_fibs < 0) return DABX_E_ARG;
  FigDecoder *d = static_cast<FigDecoder *>(dec);
  const FigOut o{d->labels, d->ring};
  for (int i = 0; i < n_fibs; i++) fig_walk_fib(d->st, fibs + (size_t)i * 32, crc_ok[i] != 0, o, 0);
  return 0;
}
int dabx_internal_fig_host_read(const void *dec, dabx_fibdec_info *info, int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets,
                                int32_t *n_labels, dabx_fig_label *labels, dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events)
{
  if (!dec) return DABX_E_ARG;
  fig_present(*static_cast<const FigDecoder *>(dec), info, n_tab, subch, packets, n_labels, labels, stats, n_events, events);
  return 0;
}

// ... and with the service information (tests/test_fig_si_cases.py): a FigSiHostDecoder is a FigDecoder with its FigSiState behind it; _read
// presents it as one row of dabx_fig_si_walk_device's outputs, the directory joined by the host build of fig_dir_record.
struct FigSiHostDecoder {
  FigDecoder dec;
  FigSiState si;
};
int dabx_internal_fig_si_host_bytes(void) { return (int)sizeof(FigSiHostDecoder); }
int dabx_internal_fig_si_host_init(void *dec, int reference_quirks)
{
  if (!dec) return DABX_E_ARG;
  FigSiHostDecoder *d = static_cast<FigSiHostDecoder *>(dec);
  memset(d, 0, sizeof(*d));
  fig_state_init(d->dec.st, reference_quirks ? 1 : 0, 0);
  fig_si_state_init(d->si);
  return 0;
}
int dabx_internal_fig_si_host_walk(void *dec, const uint8_t *fibs, const uint8_t *crc_ok, int n_fibs)
{
  if (!dec || !fibs || !crc_ok || n_fibs < 0) return DABX_E_ARG;
  FigSiHostDecoder *d = static_cast<FigSiHostDecoder *>(dec);
  const FigOut o{d->dec.labels, d->dec.ring, &d->si};
  for (int i = 0; i < n_fibs; i++) fig_walk_fib(d->dec.st, fibs + (size_t)i * 32, crc_ok[i] != 0, o, 0);
  return 0;
}
int dabx_internal_fig_si_host_read(const void *dec, dabx_fibdec_info *info, int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets,
                                   int32_t *n_labels, dabx_fig_label *labels, dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events,
                                   dabx_fig_si_scalars *si_info, dabx_fig_si_stats *si_stats, dabx_fig_global_def *global_defs, dabx_fig_user_apps_entry *user_apps,
                                   dabx_fig_fec_scheme *fec, dabx_fig_cluster *clusters, dabx_fig_language *languages, dabx_fig_programme_type *ptys,
                                   int32_t *n_dir, dabx_fig_service *dir)
{
  if (!dec) return DABX_E_ARG;
  const FigSiHostDecoder *d = static_cast<const FigSiHostDecoder *>(dec);
  fig_present(d->dec, info, n_tab, subch, packets, n_labels, labels, stats, n_events, events);
  fig_si_present(d->dec.st, d->si, FigSiOuts{si_info, si_stats, global_defs, user_apps, fec, clusters, languages, ptys, n_dir, dir});
  for (int k = 0; k < 2; k++) {
    const int n = d->dec.st.cfg[d->dec.st.cur ^ k].n_comp;
    if (n_dir) n_dir[k] = n;
    for (int i = 0; dir && i < n; i++) fig_dir_record(d->dec.st, d->si, d->dec.labels, k, i, dir + (size_t)k * FIG_MAX_COMP + i);
  }
  return 0;
}

// Test entries of the data handlers (tests/test_data_handler_cases.py, tests/test_gpu_data_handler_stage.py; not part of include/dabx.h): one
// slot's crafted data groups -- group i is bytes[groups[i].byte_pos .. + groups[i].length), with the verdicts and the last_frame of its
// record -- through the handler (data_core.h).  _host: the host build of data_group, needs no device.  _device: k_data_batch, the body of
// the engine's k_data_handler, one wave.  items [max_items], out_bytes [out_cap]: all items in emission order, byte_pos counted from
// out_bytes; more items or bytes than that room: DABX_E_ARG.  Returns the number of items; *stats as dabx_get_data_stats (launches 0).
static int data_walk_args(const char *who, int handler, int n_groups, const dabx_datagroup_info *groups, const uint8_t *bytes, size_t n_bytes, int max_items,
                          const dabx_data_item *items, const uint8_t *out_bytes, const dabx_data_stats *stats)
{
  bool ok = handler >= DABX_DATA_HANDLER_TDC && handler <= DABX_DATA_HANDLER_JOURNALINE && n_groups >= 0 && (groups || !n_groups) && (bytes || !n_bytes) && max_items > 0 &&
            max_items <= 1 << 20 && items && out_bytes && stats && n_bytes <= (size_t)1 << 30;
  for (int i = 0; ok && i < n_groups; i++)
    ok = groups[i].byte_pos >= 0 && (unsigned long long)groups[i].byte_pos + groups[i].length <= n_bytes && groups[i].length <= DABX_DG_MAX_BYTES;
  if (!ok) { set_error("%s: bad argument", who); return DABX_E_ARG; }
  return 0;
}
static size_t data_pow2(size_t v) { size_t p = 4; while (p < v) p <<= 1; return p; }

int dabx_internal_data_walk_host(int handler, int only_new_revisions, int n_groups, const dabx_datagroup_info *groups, const uint8_t *bytes, size_t n_bytes,
                                 int max_items, dabx_data_item *items, uint8_t *out_bytes, size_t out_cap, dabx_data_stats *stats)
{
  if (int rc = data_walk_args("dabx_internal_data_walk_host", handler, n_groups, groups, bytes, n_bytes, max_items, items, out_bytes, stats)) return rc;
  const size_t n_rec = data_pow2((size_t)max_items), n_out = data_pow2(out_cap);
  std::vector<dabx_data_item> recs(n_rec);
  std::vector<uint8_t> ring(n_out), jl(DATA_JL_TABLE, (uint8_t)DATA_JL_NONE);
  uint16_t crc[256], xpow[DATA_XPOW];
  data_host_tables(crc, xpow);
  DataWave w{};
  DataCounters cnt{};
  w.c = &cnt;
  w.recs = recs.data(); w.ring = ring.data(); w.rec_mask = n_rec - 1; w.bytes_mask = n_out - 1; w.jl = jl.data(); w.crc = crc; w.xpow = xpow;
  w.only_new = only_new_revisions ? 1 : 0;
  for (int i = 0; i < n_groups; i++)
    data_group(w, handler, bytes + groups[i].byte_pos, groups[i].length, groups[i].crc_flag != 0, groups[i].crc_ok != 0, groups[i].last_frame, (unsigned)i);
  data_present(w, handler, stats);
  if (w.n_recs > max_items || (unsigned long long)w.n_bytes > out_cap) { set_error("dabx_internal_data_walk_host: %lld items of %lld bytes do not fit the room", w.n_recs, w.n_bytes); return DABX_E_ARG; }
  memcpy(items, recs.data(), sizeof(dabx_data_item) * (size_t)w.n_recs);
  memcpy(out_bytes, ring.data(), (size_t)w.n_bytes);
  return (int)w.n_recs;
}

int dabx_internal_data_walk_device(int handler, int only_new_revisions, int n_groups, const dabx_datagroup_info *groups, const uint8_t *bytes, size_t n_bytes,
                                   int max_items, dabx_data_item *items, uint8_t *out_bytes, size_t out_cap, dabx_data_stats *stats)
{
  int rc = data_walk_args("dabx_internal_data_walk_device", handler, n_groups, groups, bytes, n_bytes, max_items, items, out_bytes, stats);
  if (rc) return rc;
  if (n_groups == 0) { set_error("dabx_internal_data_walk_device: no group"); return DABX_E_ARG; }      // (nothing to launch for)
  if ((rc = need_device())) return rc;
  const size_t n_rec = data_pow2((size_t)max_items), n_out = data_pow2(out_cap), n_in = data_pow2(n_bytes);
  const bool jl = handler == DABX_DATA_HANDLER_JOURNALINE;
  DevBuf dslot, dgrp, din, drec, dring;
  if ((rc = dslot.alloc(sizeof(DataBatchSlot))) || (rc = dgrp.from_host(groups, sizeof(dabx_datagroup_info) * (size_t)n_groups)) || (rc = din.alloc(n_in)) ||
      (rc = drec.alloc(sizeof(dabx_data_item) * n_rec)) || (rc = dring.alloc(n_out + (jl ? DATA_JL_TABLE : 0)))) return rc;
  DABX_HIP(hipMemset(din.p, 0, n_in));
  if (n_bytes) DABX_HIP(hipMemcpy(din.p, bytes, n_bytes, hipMemcpyHostToDevice));
  if (jl) DABX_HIP(hipMemset(dring.as<uint8_t>() + n_out, DATA_JL_NONE, DATA_JL_TABLE));
  DataBatchSlot b{};
  b.st.out.bytes = dring.as<uint8_t>(); b.st.out.recs = drec.as<dabx_data_item>(); b.st.out.bytes_mask = (uint32_t)(n_out - 1); b.st.out.rec_mask = (uint32_t)(n_rec - 1);
  b.st.handler = handler; b.st.only_new = only_new_revisions ? 1 : 0; b.st.jl = jl ? dring.as<uint8_t>() + n_out : nullptr;
  b.groups = dgrp.as<dabx_datagroup_info>(); b.n_groups = n_groups;
  DABX_HIP(hipMemcpy(dslot.p, &b, sizeof(b), hipMemcpyHostToDevice));
  if ((rc = launch_data_batch(dslot.as<DataBatchSlot>(), 1, din.as<uint8_t>(), (unsigned long long)n_in - 1, 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  if ((rc = dslot.to_host(&b, sizeof(b)))) return rc;
  memset(stats, 0, sizeof(*stats));
  stats->groups = b.st.groups; stats->items = b.st.out.count; stats->bytes = b.st.out.n_bytes;
  memcpy(&stats->dg_overrun, &b.st.c, sizeof(DataCounters));
  stats->active = 1; stats->handler = handler;
  if (b.st.out.count > max_items || (unsigned long long)b.st.out.n_bytes > out_cap) {
    set_error("dabx_internal_data_walk_device: %lld items of %lld bytes do not fit the room", b.st.out.count, b.st.out.n_bytes);
    return DABX_E_ARG;
  }
  if (b.st.out.count && (rc = drec.to_host(items, sizeof(dabx_data_item) * (size_t)b.st.out.count))) return rc;
  if (b.st.out.n_bytes && (rc = dring.to_host(out_bytes, (size_t)b.st.out.n_bytes))) return rc;
  return (int)b.st.out.count;
}

// cir_viewer.cpp:66-95 on crafted rows: the row function of k_cir (cir_core.h, cir_row_block), one block per row
int dabx_cir_rows_device(const float *iq, int n_rows, float *y)
{
  if (!iq || !y || n_rows <= 0 || n_rows > 65535) { set_error("dabx_cir_rows_device: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf din, dout;
  const size_t nb = sizeof(float2) * TU * (size_t)n_rows;
  if ((rc = din.alloc(nb)) || (rc = dout.alloc(sizeof(float) * (size_t)n_rows))) return rc;
  DABX_HIP(hipMemcpy(din.p, iq, nb, hipMemcpyHostToDevice));
  if ((rc = launch_cir_rows_test(din.as<float2>(), n_rows, dout.as<float>(), 0))) return rc;
  DABX_HIP(hipDeviceSynchronize());
  DABX_HIP(hipMemcpy(y, dout.p, sizeof(float) * (size_t)n_rows, hipMemcpyDeviceToHost));
  return 0;
}

// spectrum_viewer.cpp:169-218 on crafted windows: the row function of k_spectrum (spectrum_core.h, spectrum_row_block), one block walks the
// n windows through one display buffer
int dabx_spectrum_rows_device(const float *iq, int n, float *state, float *lin, float *db, float *ext)
{
  if (!iq || !state || !lin || !db || n <= 0 || n > 4096) { set_error("dabx_spectrum_rows_device: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf din, dst, dlin, ddb, dext, dwin;
  const size_t nb = sizeof(float2) * SPEC_SIZE * (size_t)n, no = sizeof(float) * SPEC_DISPLAY * (size_t)n, ns = sizeof(float) * (SPEC_DISPLAY + 4);
  if ((rc = din.alloc(nb)) || (rc = dst.alloc(ns)) || (rc = dlin.alloc(no)) || (rc = ddb.alloc(no)) || (rc = dext.alloc(sizeof(float) * 4 * (size_t)n)) ||
      (rc = dwin.alloc(sizeof(float) * SPEC_SIZE))) return rc;
  std::vector<float> w(SPEC_SIZE);
  spectrum_make_window(w.data());
  DABX_HIP(hipMemcpy(dwin.p, w.data(), sizeof(float) * SPEC_SIZE, hipMemcpyHostToDevice));
  DABX_HIP(hipMemcpy(din.p, iq, nb, hipMemcpyHostToDevice));
  DABX_HIP(hipMemcpy(dst.p, state, ns, hipMemcpyHostToDevice));
  if ((rc = launch_spectrum_rows_test(din.as<float2>(), n, dst.as<float>(), dlin.as<float>(), ddb.as<float>(), dext.as<float>(), dwin.as<float>(), 0))) return rc;
  DABX_HIP(hipDeviceSynchronize());
  DABX_HIP(hipMemcpy(state, dst.p, ns, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(lin, dlin.p, no, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(db, ddb.p, no, hipMemcpyDeviceToHost));
  if (ext) DABX_HIP(hipMemcpy(ext, dext.p, sizeof(float) * 4 * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

int dabx_fft2048(const dabx_cf32 *in, int batch, int inverse, dabx_cf32 *out)
{
  if (!in || !out || batch <= 0) { set_error("dabx_fft2048: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf din, dout;
  const size_t n = (size_t)batch * TU * sizeof(float2);
  if ((rc = din.from_host(in, n))) return rc;
  if ((rc = dout.alloc(n))) return rc;
  if ((rc = launch_fft2048(din.as<float2>(), batch, inverse, dout.as<float2>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return dout.to_host(out, n);
}

int dabx_prs_correlate(const dabx_cf32 *v, int batch, float threshold, int strongest, int32_t *start_index)
{
  if (!v || !start_index || batch <= 0) { set_error("dabx_prs_correlate: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf din, dout;
  if ((rc = din.from_host(v, (size_t)batch * TU * sizeof(float2)))) return rc;
  if ((rc = dout.alloc((size_t)batch * 4))) return rc;
  if ((rc = launch_prs_correlate(din.as<float2>(), batch, threshold, strongest, dout.as<int32_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return dout.to_host(start_index, (size_t)batch * 4);
}

int dabx_coarse_cfo(const dabx_cf32 *fft_sym0, int batch, int32_t *hz)
{
  if (!fft_sym0 || !hz || batch <= 0) { set_error("dabx_coarse_cfo: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  DevBuf din, dout;
  if ((rc = din.from_host(fft_sym0, (size_t)batch * TU * sizeof(float2)))) return rc;
  if ((rc = dout.alloc((size_t)batch * 4))) return rc;
  if ((rc = launch_coarse_cfo(din.as<float2>(), batch, dout.as<int32_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return dout.to_host(hz, (size_t)batch * 4);
}

struct dabx_demap { DemapDev d; };

int dabx_demap_create(int batch, dabx_demap **out)
{
  if (!out || batch <= 0) { set_error("dabx_demap_create: bad argument"); return DABX_E_ARG; }
  int rc = need_device();
  if (rc) return rc;
  auto *h = new dabx_demap();
  if ((rc = demap_alloc(h->d, batch))) { delete h; return rc; }
  if ((rc = launch_demap_init(h->d, 0))) { demap_free(h->d); delete h; return rc; }
  DABX_HIP(hipStreamSynchronize(0));
  *out = h;
  return 0;
}
void dabx_demap_destroy(dabx_demap *d) { if (d) { demap_free(d->d); delete d; } }
int dabx_demap_reset(dabx_demap *d)
{
  if (!d) return DABX_E_ARG;
  int rc = launch_demap_reset(d->d, 0);
  if (rc) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return 0;
}
int dabx_demap_set_soft_bit_gen_type(dabx_demap *d, int type)
{
  if (!d || type < 1 || type > 3) return DABX_E_ARG;
  d->d.soft_type = type;
  return 0;
}
static int demap_store(dabx_demap *d, const dabx_cf32 *fft, bool null_sym)
{
  if (!d || !fft) return DABX_E_ARG;
  DevBuf din;
  int rc = din.from_host(fft, (size_t)d->d.batch * TU * sizeof(float2));
  if (rc) return rc;
  rc = null_sym ? launch_demap_store_null(d->d, din.as<float2>(), 0) : launch_demap_store_ref(d->d, din.as<float2>(), 0);
  if (rc) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return 0;
}
int dabx_demap_store_reference_symbol_0(dabx_demap *d, const dabx_cf32 *fft) { return demap_store(d, fft, false); }
int dabx_demap_store_null_symbol_without_tii(dabx_demap *d, const dabx_cf32 *fft) { return demap_store(d, fft, true); }
int dabx_demap_get_snr_db(dabx_demap *d, float *snr_db)
{
  if (!d || !snr_db) return DABX_E_ARG;
  DevBuf dout;
  int rc;
  if ((rc = dout.alloc((size_t)d->d.batch * 4))) return rc;
  if ((rc = launch_demap_snr(d->d, dout.as<float>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return dout.to_host(snr_db, (size_t)d->d.batch * 4);
}
int dabx_demap_get_lcd_data(dabx_demap *d, float *snr_db, float *mer_db, float *mean_value)
{
  if (!d) return DABX_E_ARG;
  const int B = d->d.batch;
  DevBuf dout;
  int rc;
  if ((rc = dout.alloc((size_t)B * 12))) return rc;
  if ((rc = launch_demap_lcd(d->d, dout.as<float>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  std::vector<float> h((size_t)B * 3);
  if ((rc = dout.to_host(h.data(), (size_t)B * 12))) return rc;
  for (int s = 0; s < B; s++) {
    if (snr_db) snr_db[s] = h[3 * (size_t)s];
    if (mer_db) mer_db[s] = h[3 * (size_t)s + 1];
    if (mean_value) mean_value[s] = h[3 * (size_t)s + 2];
  }
  return 0;
}
int dabx_demap_decode_symbols(dabx_demap *d, const dabx_cf32 *fft, int n_sym, const float *clock_err, int16_t *soft)
{
  if (!d || !fft || !clock_err || !soft || n_sym <= 0) return DABX_E_ARG;
  const int B = d->d.batch;
  DevBuf din, dce, dsoft;
  int rc;
  if ((rc = din.from_host(fft, (size_t)B * n_sym * TU * sizeof(float2)))) return rc;
  if ((rc = dce.from_host(clock_err, (size_t)B * 4))) return rc;
  if ((rc = dsoft.alloc((size_t)B * n_sym * K2 * 2))) return rc;
  if ((rc = launch_demap_symbols(d->d, din.as<float2>(), n_sym, dce.as<float>(), dsoft.as<int16_t>(), 0))) return rc;
  DABX_HIP(hipStreamSynchronize(0));
  return dsoft.to_host(soft, (size_t)B * n_sym * K2 * 2);
}

}  // extern "C"
