// spectrum_core.h -- the RF spectrum and its waterfall row (include/dabx.h dabx_set_spectrum_mode; pipeline.hip k_spectrum;
// docs/history/spectrum.md): what SpectrumViewer::show_spectrum (base/spectrum_viewer/spectrum_viewer.cpp:141-234) and
// WaterfallScope::show_waterfall (waterfall_scope.cpp:52-79) make of the 2048 raw samples SampleReader captures at most every quarter second's
// worth of consumed samples (base/ofdm/sample_reader.cpp:198-205, :267-272, :285-296).  The stage's records, the evaluation of one window, the
// display limits and the capture schedule -- each ONE function that the kernels and the host entries both call.
#pragma once
#include "ofdm_core.h"
#include "pipeline.h"
#include "cir_core.h"
#include <math.h>

namespace dabx {

constexpr int SPEC_SIZE = TU;                                        // SP_SPECTRUMSIZE / SPEC_BUFF_SIZE: 2048 samples
constexpr int SPEC_DISPLAY = 512;                                    // SP_DISPLAYSIZE
constexpr int SPEC_OVR = SPEC_SIZE / SPEC_DISPLAY;                   // SP_SPEC_OVR_SMP_FAC: 4 bins per display bin
constexpr long long SPEC_PERIOD = INPUT_RATE / 4;                    // sample_reader.cpp:287: sampleCount > INPUT_RATE / 4 (strictly)
constexpr int SPEC_LOC_BEGIN = 64, SPEC_LOC_END = 447;               // signalBeginIdx, signalEndIdx (spectrum_viewer.cpp:201-202), both inclusive
constexpr int SPEC_RING = 8;                                         // records per stream
constexpr int SPEC_SLOT_BYTES = 32 + 32 + SPEC_DISPLAY * 4 + SPEC_DISPLAY;   // dabx_spectrum_record, dabx_spectrum_limits_rec, db [512] f32, row [512] u8
constexpr unsigned long long SPEC_NONE = ~0ull;                      // spectrum_next_show: "not in here"
static_assert(SPEC_OVR == 4 && SPEC_PERIOD == 512000 && SPEC_SLOT_BYTES % 16 == 0 && SPEC_SLOT_BYTES == 2624, "spectrum_core.h");
static_assert(SPEC_LOC_BEGIN == (int)(SPEC_DISPLAY * (1.0 - (1536000.0 / INPUT_RATE)) / 2.0) && SPEC_LOC_END == SPEC_DISPLAY - SPEC_LOC_BEGIN - 1, "spectrum_core.h");

// mSpecViewLimits (dab_constants.h:96-102) in the order of its members: Glob {Max, Min}, Loc {Max, Min}
struct SpecLimits { float glob_max, glob_min, loc_max, loc_min; };
__host__ __device__ inline SpecLimits spectrum_limits_initial() { return SpecLimits{-30.0f, -90.0f, -31.0f, -50.0f}; }
// mAvrAlpha of SpectrumViewer::slot_handle_avr_rate (spectrum_viewer.cpp:397-403): 0 slow, 1 medium, 2 fast
__host__ __device__ inline float spectrum_alpha(int averaging) { return averaging == 0 ? 0.01f : (averaging == 1 ? 0.10f : 1.00f); }

struct SpecCfgDev { int32_t enable, averaging, zoom_percent, pad_; };
// where the stream's capture stands: the device owns it (the host writes it only with the engine drained)
struct SpecState {
  unsigned long long W;           // first sample of the window being captured, or captured and waiting for its show
  unsigned long long pos;         // the schedule has been evaluated up to this sample
  long long lost_seen;            // StreamCtl::sync_lost at the last look
  long long shows;                // records completed
  long long untrusted;            // ... of them given up for the trust rule
  long long inexact;              // ... of them shown in a searched range that held a failed correlation (see spectrum_look)
  int32_t state_seen;             // StreamCtl::state at the last look (ST_EVAL_SYNC also where that look saw a frame begin)
  int32_t computed;               // 0: the window is not evaluated yet, 1: it is, `pend` holds it, 2: it was given up for the trust rule
  SpecLimits lim;                 // mSpecViewLimits
};
struct SpecDev {
  const int32_t *list;            // [n] the streams with the mode on, ascending
  int32_t n, pad_;
  const SpecCfgDev *cfg;          // [S]
  SpecState *st;                  // [S]
  float *disp;                    // [S][512] mDisplayBuffer
  uint8_t *pend;                  // [S][SPEC_SLOT_BYTES] the evaluated window that waits for its show
  uint8_t *ring;                  // [S][SPEC_RING][SPEC_SLOT_BYTES]
  const float *window;            // [2048] mWindowVec, made by the host (spectrum_make_window)
};

// create_flattop_window (glob_defs.h:252-266) exactly: the five-term cosine sum over i / 2047 in double, cast to float
inline void spectrum_make_window(float *w)
{
  const double a[5] = {0.21557895, -0.41663158, 0.277263158, -0.083578947, 0.006947368};
  for (int i = 0; i < SPEC_SIZE; i++) {
    double x = 0.0;
    for (int j = 0; j < 5; ++j) x += a[j] * cos(j * i * 2.0 * M_PI / (SPEC_SIZE - 1));
    w[i] = (float)x;
  }
}

// ---- the capture schedule --------------------------------------------------------------------------------------------------------
// sample_reader.cpp:285-296 in positions: W = the first sample of the window (the read position at which specBuffIdx and sampleCount were
// last put to 0).  A get_samples call that ends at sample position E (one past its last sample) shows the window if it was made with
// iShowSpec == true and E - W > 512 000; the buffer is full then anyway.  Calls made with true: every single-sample call of the
// null-symbol search (sample_reader.cpp:96-99) -- a searched range [a, b) has the call ends a + 1 .. b --, and the reads of symbols 1..75
// of a frame (dab_processor.cpp:321) -- the ends sym0_end + 2552 j, j = 1..75.  Returns the smallest such E of the range or frame, or
// SPEC_NONE.  The next window starts at E.
constexpr int SPEC_SEARCHED = 0, SPEC_FRAME = 1;
__host__ __device__ inline unsigned long long spectrum_next_show(unsigned long long W, int kind, unsigned long long a, unsigned long long b)
{
  const unsigned long long target = W + (unsigned long long)SPEC_PERIOD + 1;     // the smallest E with E - W > 512 000
  if (kind == SPEC_SEARCHED) {
    if (b <= a) return SPEC_NONE;
    const unsigned long long E = a + 1 > target ? a + 1 : target;
    return E <= b ? E : SPEC_NONE;
  }
  // a = sym0_end: one past the last sample of symbol 0
  unsigned long long j = 1;
  if (target > a + (unsigned long long)TS) j = (target - a + (unsigned long long)TS - 1) / (unsigned long long)TS;
  return j <= 75 ? a + j * (unsigned long long)TS : SPEC_NONE;
}

// One look at a stream, directly behind the frame head of a front-end step, at what the existing kernels leave: the read position, the
// state, the count of failed correlations, and whether this step's head has begun a frame (frame_ok, sym0_pos).  Since the last look
// (q.pos, q.state_seen) the stream has, in this order: if it was out of lock, been searched by k_acquire from q.pos to rd (the 20 T_u reads
// that seed the level of a fresh stream, dab_processor.cpp:139-142, do not show, but they are the stream's first 40 960 samples and no show
// position lies below 512 001: they need no case); if it was in lock, had its T_u block correlated by the
// head, which either failed (the block is read without a show, sync_lost counts it) or began a frame at sym0_pos (symbol 0 does not show,
// symbols 1..75 do, the null symbol does not).  A frame is evaluated as a whole when it begins: its window, if it has one, starts at a
// symbol end the receiver has not read yet.  Returns E or SPEC_NONE; *inexact = 1 if E lies in a searched range in which a correlation of
// the search failed: k_acquire leaves the position of a failed candidate's T_u block nowhere, so if sample W + 512 000 lies inside one the
// reference shows at the end of the block + 1 and this look up to 2048 samples earlier (counted: SpecState::inexact).
__host__ __device__ inline unsigned long long spectrum_look(SpecState &q, unsigned long long rd, int st, long long lost, int frame_ok,
                                                            unsigned long long sym0_pos, int *inexact)
{
  unsigned long long E = SPEC_NONE, cursor = q.pos;
  *inexact = 0;
  if (rd < cursor && !frame_ok) {                          // the stream was put back (a reset): the capture starts again at its read position
    q.W = rd; q.computed = 0; cursor = rd;
  } else if (q.state_seen == ST_EVAL_SYNC) {
    if (!frame_ok && lost > q.lost_seen) cursor += (unsigned long long)TU;       // dab_processor.cpp:392, :396-400
  } else {
    if (rd > cursor) {
      E = spectrum_next_show(q.W, SPEC_SEARCHED, cursor, rd);
      if (E != SPEC_NONE && lost > q.lost_seen) *inexact = 1;
    }
  }
  const unsigned long long sym0_end = sym0_pos + (unsigned long long)TU;
  if (E == SPEC_NONE && frame_ok) E = spectrum_next_show(q.W, SPEC_FRAME, sym0_end, 0);
  q.pos = frame_ok ? sym0_end + 75ull * (unsigned long long)TS + (unsigned long long)TN : rd;
  q.state_seen = frame_ok ? (int32_t)ST_EVAL_SYNC : st;
  q.lost_seen = lost;
  return E;
}

// ---- the display limits -------------------------------------------------------------------------------------------------------------
// _calc_spectrum_display_limits (spectrum_viewer.cpp:112-139), on one Max / Min pair
__host__ __device__ inline bool spectrum_calc_limits(float &mx, float &mn)
{
  const float cMinShownLevel = -99.0f, cMinLevelRange = 20.0f;
  bool changed = false;
  if (mn < cMinShownLevel) { changed = true; mn = cMinShownLevel; }              // :119-123
  if (mx - mn < cMinLevelRange) {                                                 // :126-137
    changed = true;
    const float mean = (mx + mn) / 2;
    mn = mean - cMinLevelRange / 2;
    mx = mean + cMinLevelRange / 2;
    if (mn < cMinShownLevel) { mx += cMinShownLevel - mn; mn = cMinShownLevel; }
  }
  return changed;
}
// spectrum_viewer.cpp:220-230 and waterfall_scope.cpp:57-60: the four extrema of a show {glob max, glob min, loc max, loc min} go through
// mean_filter (glob_defs.h:217-220) with mAvrAlpha into the four limits, Glob is put right and Loc only if Glob changed; yMin / yMax of
// the waterfall for zoom s = zoom_percent / 100.  Returns 1 if the waterfall has a row (yRange > 0).
__host__ __device__ inline int spectrum_limits(const float ext[4], SpecLimits &l, float alpha, int zoom_percent, float *y_min, float *y_max)
{
  l.glob_max += alpha * (ext[0] - l.glob_max);
  l.glob_min += alpha * (ext[1] - l.glob_min);
  l.loc_min += alpha * (ext[3] - l.loc_min);
  l.loc_max += alpha * (ext[2] - l.loc_max);
  if (spectrum_calc_limits(l.glob_max, l.glob_min)) spectrum_calc_limits(l.loc_max, l.loc_min);
  const float s = (float)zoom_percent / 100.0f;                                   // slot_scaling_changed, waterfall_scope.cpp:83
  const float yMax = (l.glob_max + 5.0f) * (1.0f - s) + l.loc_max * s;
  const float yMin = l.glob_min * (1.0f - s) + l.loc_min * s;
  *y_min = yMin; *y_max = yMax;
  return yMax - yMin <= 0.0f ? 0 : 1;                                             // (a NaN range is "a row": the reference goes on as well)
}
// waterfall_scope.cpp:73-74: the colour index of one bin.  std::clamp leaves a NaN a NaN and the reference's cast of it is undefined: 0 here.
__host__ __device__ inline uint8_t spectrum_pixel(float disp, float y_min, float y_range)
{
  float t = (disp - y_min) / y_range;
  if (t < 0.0f) t = 0.0f; else if (1.0f < t) t = 1.0f;
  return t == t ? (uint8_t)(int)(t * 255.0f) : (uint8_t)0;
}

#ifdef __HIPCC__
// One window: v = its 2048 samples in the strided register layout of fft_core.h.  spectrum_viewer.cpp:169-218: the flat-top window, the
// forward transform, per display bin the mean of |X| over its four bins in j order -- the upper half of the transform first (:187-193: display
// bin i < 256 from bins 1024 + 4 i + j), then the lower (:179-185: 256 + i from 4 i + j) --, val = 20 log10f(y / 512 + 1e-6f), the IIR
// disp += 0.2f (val - disp) and the four extrema with strict comparisons from -1000 / +1000.  The thread handles display bins tid and
// tid + 256: lin[h] is mYValVec, disp[h] the bin's mDisplayBuffer in and out; ext [4] = {glob max, glob min, loc max, loc min}, the same in
// every thread.  Deviation: |X| is sqrtf(re^2 + im^2) as k_cir computes it, not std::abs (hypotf): it differs only where the squares leave
// the float range.  A NaN sample is kept as the reference keeps it: every bin's disp becomes NaN and stays NaN, and a NaN wins no
// comparison, so the extrema stay at -1000 / +1000.  lds: FFT_LDS_FLOAT2 float2, 16-byte aligned; red: >= 16 floats.
__device__ __forceinline__ void spectrum_row_block(float2 v[8], const float *window, const DevTables &t, float2 *lds, float *red, int tid,
                                                   float lin[2], float disp[2], float ext[4])
{
#pragma unroll
  for (int u = 0; u < 8; u++) { const float w = window[tid + 256 * u]; v[u].x *= w; v[u].y *= w; }      // :169-172
  fft2048<false>(v, lds, t.twiddle, tid);                                                                // :174 (its last barrier frees lds)
  float *mag = reinterpret_cast<float *>(lds);
#pragma unroll
  for (int u = 0; u < 8; u++) mag[tid + 256 * u] = sqrtf(v[u].x * v[u].x + v[u].y * v[u].y);
  __syncthreads();
  float m[4] = {-1000.0f, 1000.0f, -1000.0f, 1000.0f};                                                   // :196-199
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int d = tid + 256 * h;
    const float4 b = *reinterpret_cast<const float4 *>(&mag[h == 0 ? SPEC_SIZE / 2 + SPEC_OVR * tid : SPEC_OVR * tid]);
    float f = 0.0f;
    f += b.x; f += b.y; f += b.z; f += b.w;                                                              // :179-183
    lin[h] = f / (float)SPEC_OVR;
    const float val = 20.0f * log10f(lin[h] / (float)SPEC_DISPLAY + 1.0e-6f);                            // :207
    disp[h] += 0.2f * (val - disp[h]);                                                                   // :209, averageCount = 5
    if (disp[h] > m[0]) m[0] = disp[h];                                                                  // :211-217
    if (disp[h] < m[1]) m[1] = disp[h];
    if (d >= SPEC_LOC_BEGIN && d <= SPEC_LOC_END) {
      if (disp[h] > m[2]) m[2] = disp[h];
      if (disp[h] < m[3]) m[3] = disp[h];
    }
  }
  // (no m is a NaN: the strict comparisons are order-independent, so the tree gives what the loop over i gives)
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const bool is_max = (k & 1) == 0;
    m[k] = __builtin_bit_cast(float, wave_butterfly_u32(__builtin_bit_cast(unsigned, m[k]), [is_max](unsigned x, unsigned y) {
      const float a = __builtin_bit_cast(float, x), b = __builtin_bit_cast(float, y);
      return __builtin_bit_cast(unsigned, is_max ? (b > a ? b : a) : (b < a ? b : a)); }));
  }
  __syncthreads();                                                                                       // (every thread has read mag)
  if ((tid & 63) == 0) for (int k = 0; k < 4; k++) red[4 * (tid >> 6) + k] = m[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float r = red[k];
    for (int q = 1; q < 4; q++) { const float b = red[4 * q + k]; if ((k & 1) == 0 ? b > r : b < r) r = b; }
    ext[k] = r;
  }
  __syncthreads();                                                                                       // (red may be written again)
}
#endif

}  // namespace dabx
