// tii_core.h -- the TII detector as device code: dabx_tii_process (tii.cpp; TiiDetector, base/ofdm/tii_detector.cpp:163-530) line for line, one
// 256-thread block per detector.  The body of k_tii (the engine's stage behind the frame tail) and of k_tii_batch (dabx_tii_process_device).
//
// What keeps it comparable with the host detector, which is pinned to the reference's object code (tests/test_tii.py):
//  * every float sum and product has tii.cpp's association and order (the build has -ffp-contract=off and no fast-math): the 4-term sums per
//    carrier column, the 8-term mean per sub-id, s_e / s_t and the pattern sums in group order are each ONE lane's serial sum; the only tree
//    is `top`, a maximum;
//  * |z| is (float)sqrt((double)x * x + (double)y * y) -- no overflow or flush where hypotf has none, within one rounding of libm's --, arg
//    is the device library's atan2f; nothing else can differ from the host, and 10^(dB / 10) comes from the host as a float (tii_factor).
// Results of equal strength (the ids of a collision list) keep the order in which the detector made them.
#pragma once
#include "dabx_internal.h"

namespace dabx {

constexpr int TII_PAIRS = K / 2;                 // 768 carrier pairs: 4 blocks x 8 groups x 24 sub-ids
constexpr int TII_NB = 4, TII_NG = 8, TII_GS = 24, TII_BS = TII_NG * TII_GS;
constexpr int TII_CAND = 128;                    // results one run can make: a main id per sub-id, "99" for 23 of them, <= 69 listed ids for one (118)
constexpr int TII_RING = 8;                      // event slots per stream
constexpr int TII_SLOT_BYTES = DABX_TII_EVENT_SLOT_BYTES;

// one detector's settings as the device reads them (the engine: a row per stream)
struct TiiCfgDev {
  int32_t enable, min_frames, threshold_db, collisions, coll_sub_id;
  int32_t epoch_seen;                            // the reset epoch (EngineDev::tii_cnt[2 s + 1]) the state in `pairs` belongs to
  float factor;                                  // tii_factor(threshold_db)
  int32_t pad_;
};
struct TiiCounters { long long events, results, truncated, resets; };
// The engine's stage (k_tii): nothing of it exists until dabx_set_tii_mode first switches a stream on.
struct TiiDev {
  float2 *pairs;                                 // [S][768] mDecodedBufferArr
  TiiCfgDev *cfg;                                // [S]
  uint8_t *ring;                                 // [S][TII_RING][TII_SLOT_BYTES]: event number n of a stream lies in slot n % TII_RING
  TiiCounters *cnt;                              // [S]
  const uint8_t *turn;                           // [768] phase turn per carrier pair, in quarter turns
  const uint8_t *pattern;                        // [70 (+ 2)] group pattern of each main id, MSB = group 0
};

// tii.cpp: the two tables as dabx_tii_create makes them, and powf(10, threshold_db / 10) as dabx_tii_process computes it
void tii_tables_host(uint8_t *turn /* 768 */, uint8_t *pattern /* 72 */);
float tii_factor(int threshold_db);
// deliver.hip
int launch_tii_batch(int n, float2 *sums, float2 *pairs, const TiiCfgDev *cfg, const uint8_t *turn, const uint8_t *pattern, dabx_tii_result *out,
                     int32_t *n_results, int32_t *n_found, hipStream_t st);
struct EngineDev;
int launch_tii(const EngineDev &e, const TiiDev &t, hipStream_t st);

#ifdef __HIPCC__
struct TiiLds {
  float2 work[TII_PAIRS];
  float2 etsi[TII_BS], turned[TII_BS];
  float etsi_abs[TII_BS], turned_abs[TII_BS];
  float avg[TII_GS];
  int n_cand[TII_GS];
  // `work` is dead once the 192 columns are collapsed: the maximum's tree and the result list lie in it
  __device__ float *red() { return reinterpret_cast<float *>(work); }                                   // [256]
  __device__ dabx_tii_result *cand() { return reinterpret_cast<dabx_tii_result *>(work + 128); }        // [TII_CAND]
};
static_assert(256 * sizeof(float) <= 128 * sizeof(float2) && 128 * sizeof(float2) + TII_CAND * sizeof(dabx_tii_result) <= TII_PAIRS * sizeof(float2),
              "tii_core.h: the scratch that lies in TiiLds::work");

__device__ __forceinline__ int tii_pair_bin(int i) { const int k = -K / 2 + 2 * i; return k < 0 ? k + TU : k + 1; }   // fft_shift_skip_dc
__device__ __forceinline__ float tii_abs(float2 a) { return (float)sqrt((double)a.x * (double)a.x + (double)a.y * (double)a.y); }
__device__ __forceinline__ float2 tii_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 tii_quarter_turn(float2 v, int q)      // tii_detector.cpp:282-297
{
  switch (q) {
  case 1: return make_float2(v.y, -v.x);
  case 2: return make_float2(-v.x, -v.y);
  case 3: return make_float2(-v.y, v.x);
  default: return v;
  }
}
__device__ __forceinline__ dabx_tii_result tii_result(int main_id, int sub, float strength, float2 sum, bool non_etsi)
{
  const float kDegPerRad = 180.0f / 3.14159265358979323846f;
  dabx_tii_result r;
  // (the record's two padding bytes are written too: a slab is compared byte by byte)
  *reinterpret_cast<uint32_t *>(&r) = (uint32_t)(main_id & 255) | (uint32_t)(sub & 255) << 8;
  r.strength = strength; r.phase_deg = atan2f(sum.y, sum.x) * kDegPerRad; r.non_etsi_phase = non_etsi ? 1 : 0;
  return r;
}

// One detector run by the whole block (256 threads; every thread must call it).  sum [2048]: read, then zeroed; pairs [768]: the IIR state,
// advanced; out [DABX_TII_MAX_RESULTS]: the strongest results, strongest first.  Returns the number found (every thread gets it); the number
// stored is min(found, DABX_TII_MAX_RESULTS).
__device__ __forceinline__ int tii_detect(float2 *sum, float2 *pairs, const TiiCfgDev &cfg, const uint8_t *turn, const uint8_t *pattern,
                                          dabx_tii_result *out, TiiLds &w, int tid)
{
  constexpr int NB = TII_NB, NG = TII_NG, GS = TII_GS, BS = TII_BS;
  for (int i = tid; i < TII_PAIRS; i += 256) {                  // :247-266
    const int b = tii_pair_bin(i);
    const float2 a = sum[b], c = sum[b + 1];
    const float2 prod = make_float2(a.x * c.x - a.y * (-c.y), a.x * (-c.y) + a.y * c.x);   // a * conj(c), tii.cpp's mul_conj
    float2 p = pairs[i];
    const float2 d = make_float2(prod.x - p.x, prod.y - p.y);
    p = tii_add(p, make_float2(d.x * 0.01f, d.y * 0.01f));
    pairs[i] = p;
    w.work[i] = p;
  }
  __syncthreads();
  for (int i = tid; i < TU; i += 256) sum[i] = make_float2(0.f, 0.f);   // (every read of the sum lies in front of the barrier)
  float col_max = 0.f;
  if (tid < BS) {
    const int i = tid;
    {                                                           // a carrier alone in its four blocks is no TII, :268-296
      float mx = 0, s = 0;
      int at = 0;
      for (int j = 0; j < NB; j++) {
        const float x = tii_abs(w.work[i + j * BS]);
        s += x;
        if (x > mx) { mx = x; at = j; }
      }
      const float mn = (s - mx) / (float)(NB - 1);
      if ((double)s < (double)mx * 1.5 && (double)mx > 0.0) {
        const float k = mn / mx;
        float2 &v = w.work[i + at * BS];
        v = make_float2(v.x * k, v.y * k);
      }
    }
    float2 e = make_float2(0.f, 0.f), t = make_float2(0.f, 0.f);          // :320-344
    for (int j = 0; j < NB; j++) {
      const float2 x = w.work[i + j * BS];
      e = tii_add(e, x);
      t = tii_add(t, tii_quarter_turn(x, turn[i + j * BS]));
    }
    w.etsi[i] = e; w.turned[i] = t;
    const float ea = tii_abs(e), ta = tii_abs(t);
    w.etsi_abs[i] = ea; w.turned_abs[i] = ta;
    col_max = fmaxf(ea, ta);
  }
  __syncthreads();                                              // (the columns are read: `work` becomes scratch)
  float *red = w.red();
  dabx_tii_result *cand = w.cand();
  red[tid] = col_max;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {                           // top: a maximum, the one reduction whose order does not matter
    if (tid < h) red[tid] = fmaxf(red[tid], red[tid + h]);
    __syncthreads();
  }
  const float top = red[0];
  if (tid < GS) {                                               // weakest sub-id, :513-530
    float avg = 0;
    for (int g = 0; g < NG; g++) avg += w.etsi_abs[tid + g * GS];
    avg /= (float)NG;
    w.avg[tid] = avg;
  }
  __syncthreads();
  // per sub-id, one lane each (:389-500); what the lane found stays in registers until every lane's place in the list is known
  int n_mine = 0, main_id = 0, count = 0, n_list = 0;
  bool non_etsi = false, list_ids = false;
  unsigned pat = 0;
  float2 s_main = make_float2(0.f, 0.f), rest = make_float2(0.f, 0.f);
  float strength_rest = 0.f;
  if (tid < GS) {
    const int sub = tid;
    float noise = 1e9f;
    for (int q = 0; q < GS; q++) if (w.avg[q] < noise) noise = w.avg[q];
    const float level = noise * cfg.factor;
    float2 s_e = make_float2(0.f, 0.f), s_t = make_float2(0.f, 0.f);
    int n_e = 0, n_t = 0;
    unsigned p_e = 0, p_t = 0;
    for (int g = 0; g < NG; g++) {                              // :389-441
      const int ix = sub + g * GS;
      if (w.etsi_abs[ix] > level) { n_e++; p_e |= 0x80u >> g; s_e = tii_add(s_e, w.etsi[ix]); }
      if (w.turned_abs[ix] > level) { n_t++; p_t |= 0x80u >> g; s_t = tii_add(s_t, w.turned[ix]); }
    }
    non_etsi = (n_e >= 4 || n_t >= 4) && tii_abs(s_t) > tii_abs(s_e);
    s_main = non_etsi ? s_t : s_e;
    count = non_etsi ? n_t : n_e;
    pat = non_etsi ? p_t : p_e;
    const float2 *tab = non_etsi ? w.turned : w.etsi;
    const float *tab_abs = non_etsi ? w.turned_abs : w.etsi_abs;
    if (count == 4) {                                           // :346-357
      main_id = -1;
      for (int m = 0; m < 70; m++) if (pattern[m] == pat) { main_id = m; break; }
    } else if (count > 4) {                                     // best four of the groups, :359-387: the first maximum wins
      float best = 0;
      main_id = -1;
      s_main = make_float2(0.f, 0.f);
      for (int m = 0; m < 70; m++) {
        float2 v = make_float2(0.f, 0.f);
        const unsigned pm = pattern[m];
        for (int g = 0; g < NG; g++) if (pm & (0x80u >> g)) v = tii_add(v, tab[sub + GS * g]);
        const float a = tii_abs(v);
        if (a > best) { best = a; s_main = v; main_id = m; }
      }
    }
    if (count >= 4) n_mine = 1;
    if (count > 4 && cfg.collisions && main_id >= 0) {          // :443-500 (main_id < 0: every candidate was NaN; the host indexes pattern[-1] there)
      const unsigned pm = pattern[main_id];
      for (int g = 0; g < NG; g++)
        if (!(pm & (0x80u >> g)) && tab_abs[sub + GS * g] > level) rest = tii_add(rest, tab[sub + GS * g]);
      strength_rest = tii_abs(rest) / top / (float)(count - 4);
      list_ids = sub == cfg.coll_sub_id;
      if (list_ids) {
        for (int m = 0; m < 70; m++) if (__popc(pattern[m] & pat) == 4 && m != main_id) n_list++;
      } else n_list = 1;
      n_mine += n_list;
    }
    w.n_cand[sub] = n_mine;
  }
  __syncthreads();
  int found = 0;
  for (int q = 0; q < GS; q++) found += w.n_cand[q];
  if (found > TII_CAND) found = TII_CAND;                       // (cannot happen: 24 + 23 + 69)
  if (tid < GS && n_mine) {
    int at = 0;
    for (int q = 0; q < tid; q++) at += w.n_cand[q];
    if (count >= 4 && at < TII_CAND) cand[at++] = tii_result(main_id, tid, tii_abs(s_main) / top / 4, s_main, non_etsi);
    if (n_list) {
      if (list_ids) {
        const dabx_tii_result r = tii_result(0, tid, strength_rest, rest, non_etsi);
        for (int m = 0; m < 70; m++)
          if (__popc(pattern[m] & pat) == 4 && m != main_id && at < TII_CAND) {
            cand[at] = r;
            *reinterpret_cast<uint8_t *>(&cand[at]) = (uint8_t)m;
            at++;
          }
      } else if (at < TII_CAND) cand[at] = tii_result(99, tid, strength_rest, rest, non_etsi);
    }
  }
  __syncthreads();
  // strongest first: a result's place is the number of results in front of it (equal strengths: the earlier one)
  if (tid < found) {
    const float mine = cand[tid].strength;
    const bool mine_nan = mine != mine;                         // (a NaN counts as weaker than every number: the places stay a permutation)
    int rank = 0;
    for (int q = 0; q < found; q++) {
      const float x = cand[q].strength;
      const bool x_nan = x != x;
      rank += (mine_nan ? (!x_nan || q < tid) : (!x_nan && (x > mine || (x == mine && q < tid)))) ? 1 : 0;
    }
    if (rank < DABX_TII_MAX_RESULTS) out[rank] = cand[tid];
  }
  __syncthreads();
  return found;
}
#endif

}  // namespace dabx
