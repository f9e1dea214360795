// cir_core.h -- the channel impulse response plot (include/dabx.h dabx_set_cir_mode; pipeline.hip k_cir; docs/history/cir.md): what
// CirViewer::show_cir (base/spectrum_viewer/cir_viewer.cpp:54-107) draws from the 97 x 2048 raw samples SampleReader captures every six
// frames' worth of consumed samples (sample_reader.cpp:179-196, :250-265; CIR_BUFF_SIZE).  The stage's records, its window / row
// bookkeeping, the trust rule and the evaluation of one row -- each ONE function that the kernels and the host entries both call.
#pragma once
#include "ofdm_core.h"

namespace dabx {

constexpr int CIR_ROW_STEP = 512;                                    // cir_viewer.cpp:68: row j starts at cirbuffer[j * 512]
constexpr int CIR_WINDOW = 97 * TU;                                  // CIR_SPECTRUMSIZE / CIR_BUFF_SIZE: 198 656 samples
constexpr int CIR_ROWS = (CIR_WINDOW - TU) / CIR_ROW_STEP + 1;       // sPlotLength (:56): 385
constexpr long long CIR_PERIOD = 6LL * TF;                           // a window every six frames' worth of samples: 1 179 648
constexpr int CIR_CORR_LAGS = TU;                                    // the correlation plot's |corr| (kind 1)
// The index list of the correlation plot: the walk of phasereference.cpp:143-169 visits i = T_g - 250 .. T_g + 499, 750 positions, and an
// accepted peak skips gap = 10 positions on top of the loop's own step, 11 in all: accepted peaks lie at least 11 apart, the first at the
// earliest on position 0 of the 750, so there are at most ceil(750 / 11) = 69 of them.
constexpr int CIR_MAX_INDICES = (750 + 10) / 11;
constexpr int CIR_INDEX_ROOM = (CIR_MAX_INDICES + 7) / 8 * 8;        // int16 slots, padded so that a slot is a whole number of 16-byte words
constexpr int CIR_ROWS_PER_BLOCK = 4;                                // rows a block of k_cir walks: one look at the write horizon (host memory) in front of them, one behind
constexpr int CIR_RING = 4;                                          // records per stream
constexpr int CIR_SLOT_BYTES = 32 + CIR_CORR_LAGS * 4 + CIR_INDEX_ROOM * 2;   // dabx_cir_record, the values (f32), the indices (int16)
constexpr float CIR_SCALE = 26000.0f;                                // :84 / :93
static_assert(CIR_ROWS == 385 && CIR_MAX_INDICES == 69 && CIR_SLOT_BYTES % 16 == 0 && CIR_PERIOD == 1179648 && CIR_WINDOW == 198656, "cir_core.h");

struct CirCfgDev { int32_t enable, cir, correlation, pad_; };
// where the stream's CIR stands, and the records written so far: the device owns it (the host writes it only with the engine drained)
struct CirState {
  unsigned long long base;        // the stream's read position when the CIR was switched on: window n begins at base + n * CIR_PERIOD
  long long win;                  // the window being computed
  int32_t rows_done;              // rows 0 .. rows_done - 1 of it lie in acc
  int32_t corr_counter;           // mDisplayCounter (phasereference.h) of the correlation plot
  long long shows;                // records completed
  long long shows_kind[2];        // ... per kind
  long long rows_untrusted;       // rows given up for the trust rule, all windows
  long long pad2_;
};
struct CirDev {
  const int32_t *list;            // [n] the streams with the mode on, ascending
  int32_t n, n_corr;              // ... and how many of them have the correlation plot on
  const CirCfgDev *cfg;           // [S]
  CirState *st;                   // [S]
  float *acc;                     // [S][CIR_ROWS] the rows of the window being computed
  float *mean;                    // [S][2048] mMeanCorrPeakValues of the correlation plot
  uint8_t *ring;                  // [S][CIR_RING][CIR_SLOT_BYTES]
};

// The window / row bookkeeping.  Rows rows_done .. rows_done + n - 1 of window `win` are due: not done yet, and all 2048 samples of each
// committed (wr = one past the last committed sample).  Never more than `cap` (the rows the launch has blocks for, per stream), never beyond the window:
// the next window's rows are the next step's.
__host__ __device__ inline int cir_rows_due(unsigned long long base, long long win, int rows_done, unsigned long long wr, int cap)
{
  const unsigned long long w0 = base + (unsigned long long)win * (unsigned long long)CIR_PERIOD;
  if (wr < w0 + (unsigned long long)TU) return 0;
  unsigned long long avail = (wr - w0 - (unsigned long long)TU) / (unsigned long long)CIR_ROW_STEP + 1;
  if (avail > (unsigned long long)CIR_ROWS) avail = CIR_ROWS;
  int n = (int)avail - rows_done;
  if (n > cap) n = cap;
  return n < 0 ? 0 : n;
}
__host__ __device__ inline unsigned long long cir_row_first(unsigned long long base, long long win, int row)
{
  return base + (unsigned long long)win * (unsigned long long)CIR_PERIOD + (unsigned long long)row * (unsigned long long)CIR_ROW_STEP;
}
// n rows further; 1 = row 384 is among them: the record is complete and the next window begins
__host__ __device__ inline int cir_rows_advance(long long &win, int32_t &rows_done, int n)
{
  rows_done += n;
  if (rows_done < CIR_ROWS) return 0;
  rows_done = 0; win++;
  return 1;
}

// The trust rule.  A row whose first sample is `first` may be read -- no push the ABI has accepted can be writing any of its ring slots --
// if the receiver has not read it yet (push_room never lets a push reach an unread sample), or if nothing issued so far reaches round the
// ring to it (EngineDev::wr_horizon: one past the highest sample a push has been issued for, ~0 after a zero-copy commit).  The row's later
// samples lie further from both bounds.  k_cir looks before and after its loads, as the level re-walk of k_acquire does.
__host__ __device__ inline bool cir_row_trusted(unsigned long long first, unsigned long long rd, unsigned long long horizon, unsigned long long ring_len)
{
  return first >= rd || (first <= ~0ull - ring_len && first + ring_len >= horizon);   // (first >= horizon - ring_len, without the wrap)
}

#ifdef __HIPCC__
// One row: v = its 2048 samples in the strided register layout of fft_core.h.  cir_viewer.cpp:69-93, scalar build: forward transform,
// product with conj(mRefTable) in registers, unnormalised backward transform, the largest re^2 + im^2 with max starting at 0 and a strict
// `>` -- a NaN never wins a comparison, so a row with a NaN anywhere gives 0; a square that overflows gives inf -- and sqrt(max) / 26000.
__device__ __forceinline__ float cir_row_block(float2 v[8], const DevTables &t, float2 *lds, float *red, int tid)
{
  fft2048<false>(v, lds, t.twiddle, tid);
#pragma unroll
  for (int u = 0; u < 8; u++) v[u] = cmul_conj(v[u], t.prs_ref[tid + 256 * u]);   // :74-77
  fft2048<true>(v, lds, t.twiddle, tid);
  float mx = 0.f;
#pragma unroll
  for (int u = 0; u < 8; u++) {                                                  // :86-92
    const float x = v[u].x * v[u].x + v[u].y * v[u].y;
    if (x > mx) mx = x;
  }
  // mx is no NaN and not negative: the order of such floats is the order of their bits
  const unsigned w = wave_butterfly_u32(__builtin_bit_cast(unsigned, mx), [](unsigned x, unsigned y) { return x > y ? x : y; });
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = __builtin_bit_cast(float, w);
  __syncthreads();
  float r = red[0];
  for (int q = 1; q < 4; q++) if (red[q] > r) r = red[q];
  return sqrtf(r) / CIR_SCALE;                                                    // :93
}
#endif

}  // namespace dabx
