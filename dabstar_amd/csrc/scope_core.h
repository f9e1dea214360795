// scope_core.h -- the demapper's IQ scope and carrier plots (include/dabx.h dabx_set_scope_mode; pipeline.hip k_scope): what OfdmDecoder hands
// its user on a shown symbol, mIqVector and mCarrVector (ofdm_decoder.cpp:258-291, 303-324), from the state the engine's demapper keeps.
// The stage's records, its two counters, and the evaluation of the shown symbol: demap_pair (ofdm_core.h) line for line, with raw, fftBin,
// phaseErr and the soft-bit weight kept.
#pragma once
#include "ofdm_core.h"

namespace dabx {

constexpr int SCOPE_RING = 8;                                        // records per stream
constexpr int SCOPE_SLOT_BYTES = 32 + K * 8 + K * 4;                 // dabx_scope_record, the IQ vector (cf32), the carrier vector (f32)
constexpr int SCOPE_IQ_TYPES = 3;                                    // EIqPlotType 0..2 (glob_enums.h); 3, 4 need the DC bin and mDcAdc
// ECarrierPlotType (glob_enums.h)
enum : int { SC_SB_WEIGHT = 0, SC_EVM_PER = 1, SC_EVM_DB = 2, SC_STD_DEV = 3, SC_PHASE_ERROR = 4, SC_PRS_PHASE = 5, SC_PRS_PHASE_UNWRAP = 6,
             SC_FOUR_QUAD_PHASE = 7, SC_REL_POWER = 8, SC_SNR = 9, SC_NULL_TII_LIN = 10, SC_NULL_TII_LOG = 11, SC_NULL_NO_TII = 12, SC_NULL_OVR_POW = 13 };
constexpr __host__ __device__ bool scope_carrier_type_built(int t) { return (t >= 0 && t <= 9) || t == 13; }

struct ScopeCfgDev { int32_t enable, iq_type, carrier_type, symbol; };   // symbol 0: the reference's cadence; 1..75: that symbol of every decoded frame
// mShowCntIqScope, mShowCntStatistics, mNextShownOfdmSymbIdx (ofdm_decoder.h:86-88) and the records written so far: the device owns them
struct ScopeState { int32_t cnt_iq, cnt_stat, next_sym, pad_; long long shows, pad2_; };
struct ScopeDev {
  const int32_t *list;            // [n] the streams with the mode on, ascending: one block each
  int32_t n, pad_;
  const ScopeCfgDev *cfg;         // [S]
  ScopeState *st;                 // [S]
  uint8_t *ring;                  // [S][SCOPE_RING][SCOPE_SLOT_BYTES]
};

// The two counters over the 75 decode_symbol calls of one decoded frame (ofdm_decoder.cpp:154-157, 323, 349-351).  Returns the symbol the
// reference shows in this frame (1..75), 0 = none.  A show clears mShowCntIqScope, so a frame never has two.
__host__ __device__ inline int scope_counters_frame(ScopeState &q)
{
  int shown = 0;
  for (int l = 1; l <= 75; l++) {
    ++q.cnt_iq; ++q.cnt_stat;
    const bool show_scope = q.cnt_iq > 76 && l == q.next_sym, show_stat = q.cnt_stat > 5 * 76 && l == q.next_sym;
    if (show_scope) { shown = l; q.cnt_iq = 0; }
    if (show_stat) {
      q.cnt_stat = 0;
      q.next_sym = (q.next_sym + 1) % 76;
      if (q.next_sym == 0) q.next_sym = 1;
    }
  }
  return shown;
}

#ifdef __HIPCC__
// What the plots need of two carriers of the shown symbol.  The carriers' state in c is advanced as demap_pair advances it.
struct ScopePairOut { v2f raw_re, raw_im, b_re, b_im, phase_err, r1_re, r1_im, power, mean_level, std_dev_sq; };

template <int SOFT_TYPE>
__device__ __forceinline__ void scope_pair(DemapPair &c, v2f x_re, v2f x_im, v2f rel_f, float clock_err, v2f std_dev_sq, bool track_mer, ScopePairOut &o)
{
  constexpr float ALPHA = 0.005f;
  const float F_PI = 3.14159265358979323846f;
  const float F_RAD_PER_DEG = 0.01745329251994329577f, F_SQRT1_2 = 0.70710678118654752440f;
  const v2f pr_re = c.prev_re, pr_im = c.prev_im;
  const v2f pr_sq = pr_re * pr_re + pr_im * pr_im;
  const v2f pr_inv = v2_rsq(pr_sq);
  const v2f pr_abs = pr_sq * pr_inv;
  o.raw_re = (x_re * pr_re + x_im * pr_im) * pr_inv;                // :188-189
  o.raw_im = (x_im * pr_re - x_re * pr_im) * pr_inv;
  o.phase_err = clock_err * (F_PI / 1024.0f / (float)(K / 2)) * rel_f + c.integ;   // :192
  const v2f xx = -o.phase_err, x2 = xx * xx;                        // cmplx_from_phase2, :70-88
  const v2f sine = xx * (x2 * -0.16034401953220367431640625f + 0.99903142452239990234375f);
  const v2f cosine = 0.9994032382965087890625f + x2 * (x2 * 3.679168224334716796875e-2f + -0.495580852031707763671875f);
  o.b_re = o.raw_re * cosine - o.raw_im * sine;
  o.b_im = o.raw_re * sine + o.raw_im * cosine;
  const v2f abs_re = v2_abs(o.b_re), abs_im = v2_abs(o.b_im);
  const v2f off = phase_offset_from_diagonal2(o.b_im, o.b_re, abs_im, abs_re);   // :197-201
  const v2f integ = c.integ + 0.2f * ALPHA * off;                   // :201-202
  const float lim = F_RAD_PER_DEG * 20.0f;
  c.integ = (v2f){__builtin_amdgcn_fmed3f(integ.x, -lim, lim), __builtin_amdgcn_fmed3f(integ.y, -lim, lim)};
  if (track_mer) std_dev_sq += ALPHA * (off * off - std_dev_sq);    // :205-208
  o.std_dev_sq = std_dev_sq;
  o.power = o.b_re * o.b_re + o.b_im * o.b_im;                      // :211-213
  c.mean_power += ALPHA * (o.power - c.mean_power);
  o.mean_level = v2_sqrt(c.mean_power);                             // :217-223
  const v2f at_axis = o.mean_level * F_SQRT1_2;
  const v2f rd = abs_re - at_axis, id = abs_im - at_axis;
  const v2f sigma_sq = rd * rd + id * id;
  c.mean_sigma_sq += ALPHA * (sigma_sq - c.mean_sigma_sq);
  v2f signal_power = c.mean_power - c.null_power;                   // :225-226
  signal_power = (signal_power <= 0.0f) ? (v2f)(0.1f) : signal_power;
  const v2f babs = v2_sqrt(o.power);
  const v2f nsr = c.null_power * v2_rcp(signal_power) + 0.7f;
  v2f w1;
  if (SOFT_TYPE == 3) w1 = pr_abs;                                  // :231-235
  else if (SOFT_TYPE == 2) w1 = pr_abs * v2_rcp(c.mean_sigma_sq * nsr);   // :236-242
  else w1 = v2_sqrt(babs * pr_abs) * o.mean_level * v2_rcp(nsr * (c.mean_sigma_sq * babs));   // :243-251
  o.r1_re = o.b_re * w1; o.r1_im = o.b_im * w1;
  c.prev_re = x_re; c.prev_im = x_im;                               // :354
}

__device__ __forceinline__ float scope_log10_times_10(float x) { return 10.0f * log10f(x); }
__device__ __forceinline__ float scope_deg(float rad) { return rad * 57.295779513082320877f; }   // conv_rad_to_deg, glob_defs.h:65-68

// Inclusive prefix sum over the block's threads in thread order (blockDim.x a multiple of 64, at most 16 waves).  lds: 16 floats, free to be
// used again behind the call.
__device__ __forceinline__ float block_scan_incl(float v, float *lds, int tid)
{
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  __syncthreads();
  if (lane == 63) lds[w] = v;
  __syncthreads();
  float base = 0.f;
  for (int i = 0; i < w; i++) base += lds[i];
  __syncthreads();
  return v + base;
}
// the block's total: the last thread's inclusive value, to every thread
__device__ __forceinline__ float block_last(float incl, float *lds, int tid)
{
  __syncthreads();
  if (tid == (int)blockDim.x - 1) lds[0] = incl;
  __syncthreads();
  const float t = lds[0];
  __syncthreads();
  return t;
}
#endif

}  // namespace dabx
