// eti_core.h -- ETI(NI) frame assembly on the device: one wave builds one 6144-byte frame, byte for byte dabx_eti_frame's (eti.cpp;
// base/eti_handler/eti_generator.cpp:169-199 and :207-308).  Used by k_eti_rows (deliver.hip: the ETI stage of the bulk delivery) and by
// k_eti_frames (dabx_eti_frames_device, the stage-level entry) -- one body for both.
//
// A frame is dwords throughout: SYNC | FC | STC x NST | MNSC + header CRC | FIC (24 dwords) | the sub-channels' 3 * kbps bytes (kbps is a
// multiple of 8) | EOF CRC + RFU | TIST | 0x55555555 up to dword 1536.  Every payload dword is loaded once, stored once, and folded into
// the EOF CRC on its way.
//
// The two CRCs (CCITT, P = x^16 + x^12 + x^5 + 1, initial value 0xFFFF, complemented) are computed in parallel; CRC-16 is linear over GF(2):
//   * crc0(M) = M(x) * x^16 mod P is the CRC register after message M with a ZERO initial value.  A dword B (first byte = highest
//     coefficients) followed by t more bytes contributes crc0(B) * x^(8t) mod P, and the register is the XOR of all contributions.
//   * The initial value I is I * x^(8 len) mod P on top of that (the same as XORing I into the message's first two bytes).
//   * The MST -- FIC and sub-channels as ONE sequence of T dwords -- is walked by the wave in rounds of 64 dwords ALIGNED TO ITS END (the
//     first round is the partial one), lane l taking dword l of the round: the stores are one contiguous run per round, the loads are
//     contiguous within a sub-channel.  Per lane the rounds are a Horner scheme, a = a * x^2048 + crc0(B) (one reduction mod P per dword,
//     crc0_horner), and the lane's share of the register is a * x^(32 (63 - l)) -- a factor that depends on the lane alone.  The wave XORs
//     the shares.  A lane finds the sub-channel of its dword by moving a cursor along the sub-channels' end offsets (LDS): its position
//     grows by 64 dwords per round.  Four rounds' loads are issued before the first of their stores.
//   * The header CRC: lane i holds STC word i; its share is crc0(STC_i) * x^(32 (n - 1 - i)).
// Products are 16-bit carry-less multiplies mod P (gf16_mul); the powers x^(32 k), k <= 1536, are a table computed at compile time.
// The arithmetic is __host__ __device__ so that a host program can check it.
#pragma once
#include <stdint.h>

namespace dabx {

// r mod P for r below 2^31: four folds of the high half, x^16 = x^12 + x^5 + 1
__host__ __device__ constexpr uint32_t gf16_reduce(uint32_t r)
{
  for (int i = 0; i < 4; i++) { const uint32_t h = r >> 16; r = (r & 0xFFFFu) ^ h ^ (h << 5) ^ (h << 12); }
  return r;
}
// a * b over GF(2), not reduced (below 2^31 for a, b below 2^16); with a constant b the sum has one term per set bit
__host__ __device__ constexpr uint32_t gf16_clmul(uint32_t a, uint32_t b)
{
  uint32_t r = 0;
  for (int i = 0; i < 16; i++) r ^= (0u - ((b >> i) & 1u)) & (a << i);
  return r;
}
__host__ __device__ constexpr uint32_t gf16_mul(uint32_t a, uint32_t b) { return gf16_reduce(gf16_clmul(a, b)); }
struct Gf16Pow32 {                                           // x^(32 k) mod P, k = 0 .. 1536 (a frame has 1536 dwords)
  uint16_t v[1537];
  constexpr Gf16Pow32() : v{}
  {
    uint32_t q = 1;
    for (int k = 0; k <= 1536; k++) { v[k] = (uint16_t)q; q = gf16_mul(q, gf16_mul(0x1021u, 0x1021u)); }
  }
};
constexpr uint32_t GF16_X16 = 0x1021u;                       // x^16 mod P
constexpr uint32_t GF16_X32 = gf16_mul(GF16_X16, GF16_X16);
constexpr uint32_t GF16_X48 = gf16_mul(GF16_X32, GF16_X16);
constexpr uint32_t gf16_x2048()
{
  uint32_t q = 2;                                            // x, squared 11 times
  for (int j = 0; j < 11; j++) q = gf16_mul(q, q);
  return q;
}
constexpr uint32_t GF16_X2048 = gf16_x2048();
// crc0 of the four bytes of B (B = the dword in message order: first byte in bits 31..24)
__host__ __device__ constexpr uint32_t crc0_dword(uint32_t B) { return gf16_reduce(gf16_clmul(B >> 16, GF16_X32) ^ gf16_clmul(B & 0xFFFFu, GF16_X16)); }
// a * x^2048 + crc0(B): one step of a lane's Horner scheme, one reduction
__host__ __device__ constexpr uint32_t crc0_horner(uint32_t a, uint32_t B)
{
  return gf16_reduce(gf16_clmul(a, GF16_X2048) ^ gf16_clmul(B >> 16, GF16_X32) ^ gf16_clmul(B & 0xFFFFu, GF16_X16));
}

// The STC word of a sub-channel in message order (SCID | SAD | TPL | STL, eti_generator.cpp:271-294); sad = the start address
__host__ __device__ inline uint32_t eti_stc_word(int subch_id, int sad, int kbps, int prot_level, int short_form)
{
  const uint32_t tpl = short_form ? (0x10u | (uint32_t)(prot_level - 1)) : (0x20u | (uint32_t)prot_level);
  const uint32_t stl = (uint32_t)kbps * 3u / 8u;
  return ((uint32_t)subch_id << 26) | (((uint32_t)sad & 0x3FFu) << 16) | (tpl << 10) | (stl & 0x3FFu);
}
// bytes of a frame with n_subch sub-channels of sum_kbps kbit/s in all, before the padding (dabx_eti_frame's return value); a frame
// beyond DABX_ETI_FRAME_BYTES is refused
__host__ __device__ constexpr int eti_used_bytes(int n_subch, int sum_kbps) { return 4 + 4 + 4 * n_subch + 4 + 96 + 3 * sum_kbps + 8; }

struct EtiSlot {                  // one sub-channel of the frame, in LDS: entry i = the i-th sub-channel in STC order
  const uint32_t *src;            // its 3 * kbps logical-frame bytes (dword aligned)
  uint32_t stc;                   // eti_stc_word
  int32_t ndw;                    // 3 * kbps / 4 from the caller; eti_build_frame turns it into the sub-channel's END in the MST, in dwords
};

#ifdef __HIPCC__
}  // namespace dabx
#include "wave_ops.h"
namespace dabx {
static __constant__ Gf16Pow32 ETI_POW32 = Gf16Pow32();

// A lane's place in the MST: the sub-channel its current dword lies in (c = -1: the FIC) and that sub-channel's dword range
struct EtiCursor { int c, start, end; };
__device__ __forceinline__ const uint32_t *eti_locate(EtiCursor &q, int p, const EtiSlot *slots, const uint32_t *fic)
{
  while (p >= q.end) { q.c++; q.start = q.end; q.end = slots[q.c].ndw; }
  return (q.c < 0 ? fic : slots[q.c].src) + (p - q.start);
}

// The whole wave: frame with counter (cif_hi, cif_lo) + minor, n_subch sub-channels slots[0 .. n_subch) (LDS, written by the caller, who
// has synchronised; ndw is rewritten here), the CIF's three FIBs fic (24 dwords) into out (1536 dwords).  The caller has checked that the
// frame fits.  Returns the bytes used.
__device__ __forceinline__ int eti_build_frame(int cif_hi, int cif_lo, int minor, int n_subch, EtiSlot *slots, const uint32_t *fic,
                                               uint32_t *__restrict__ out, int lane)
{
  cif_lo += minor;                                         // eti.cpp:43-45, eti_generator.cpp:212-220
  if (cif_lo >= 250) { cif_lo %= 250; cif_hi++; }
  if (cif_hi >= 20) cif_hi = 20;
  const bool mine = lane < n_subch;
  const uint32_t stc = mine ? slots[lane].stc : 0u;
  int end = mine ? slots[lane].ndw : 0;                    // inclusive scan over the lanes: the sub-channel's end in the MST
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(end, d); if (lane >= d) end += o; }
  end += 24;
  __syncthreads();                                         // (every lane has read its ndw)
  if (mine) slots[lane].ndw = end;
  const int mst_dw = __shfl(end, 63);
  __syncthreads();
  const int fl = mst_dw + n_subch + 1;                     // words: STC + EOH + FIC + sub-channel data
  const int fp = (cif_hi * 250 + cif_lo) % 8;
  const uint32_t fc = ((uint32_t)cif_lo << 24) | ((0x80u | (uint32_t)n_subch) << 16) | ((uint32_t)((fp << 5) | (1 << 3) | ((fl >> 8) & 7)) << 8) | (uint32_t)(fl & 0xFF);
  // header CRC over FC | STC x n | 0xFFFF: 4 n + 6 bytes
  uint32_t h = mine ? gf16_mul(crc0_dword(stc), ETI_POW32.v[n_subch - 1 - lane]) : 0u;
  const uint32_t pn = ETI_POW32.v[n_subch];
  h = wave_xor(h) ^ gf16_mul(crc0_dword(fc), pn);
  h = gf16_mul(h ^ 0xFFFFu, GF16_X16);                     // the two MNSC bytes appended
  const uint32_t hcrc = ~(h ^ gf16_mul(0xFFFFu, gf16_mul(pn, GF16_X48))) & 0xFFFFu;
  if (lane == 0) {
    out[0] = (cif_lo & 1) ? 0x49C5F8FFu : 0xB63A07FFu;     // ERR = 0xFF | FSYNC, alternating
    out[1] = __builtin_bswap32(fc);
    out[2 + n_subch] = 0x0000FFFFu | ((hcrc >> 8) << 16) | ((hcrc & 0xFFu) << 24);
  }
  if (mine) out[2 + lane] = __builtin_bswap32(stc);
  // MST: FIC, then the sub-channels in order, as one run of mst_dw dwords
  uint32_t *__restrict__ mst = out + 3 + n_subch;
  const int rounds = (mst_dw + 63) >> 6, pad = (rounds << 6) - mst_dw;
  EtiCursor q{-1, 0, 24};
  uint32_t a = 0;
  for (int g = 0; g < rounds; g += 4) {
    uint32_t v[4];
    int p[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      p[u] = ((g + u) << 6) - pad + lane;
      v[u] = 0;
      if (g + u < rounds && p[u] >= 0) v[u] = *eti_locate(q, p[u], slots, fic);
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (g + u < rounds) {
        a = crc0_horner(a, __builtin_bswap32(v[u]));
        if (p[u] >= 0) mst[p[u]] = v[u];
      }
  }
  const uint32_t z = wave_xor(gf16_mul(a, ETI_POW32.v[63 - lane]));
  const uint32_t crc = ~(z ^ gf16_mul(0xFFFFu, ETI_POW32.v[mst_dw])) & 0xFFFFu;
  const int tail = 3 + n_subch + mst_dw;                   // EOF: CRC + RFU, then the unused TIST, then padding
  for (int w = tail + lane; w < 1536; w += 64)
    out[w] = w == tail ? (0xFFFF0000u | (crc >> 8) | ((crc & 0xFFu) << 8)) : (w == tail + 1 ? 0xFFFFFFFFu : 0x55555555u);
  return 4 * (tail + 2);
}
#endif

}  // namespace dabx
