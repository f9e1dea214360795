// aac_core.h -- the LOAS/LATM stream of a DAB+ slot: the per-slot state, the argument of k_aac_stream (msc_stages.hip) and the frame's pieces.
// Mp4Processor::_build_aac_stream over BitWriter (base/backend/audio/mp4processor.cpp:395-445, bit_writer.cpp:29-59) without a serial bit
// writer: everything in front of PayloadLengthInfo is 69 bits (no SBR) or 78 bits (SBR) of which only three 4-bit fields and the 13-bit
// audioMuxLengthBytes vary, so the header is one of two constant templates with those or-ed in (aac_header); what follows -- L / 255 bytes
// 0xFF, one byte L % 255, the L payload bytes -- is a run of whole bytes that lies 5 or 6 bits off the byte grid, so output byte i behind
// the header is ((b[i - 1] << 8 | b[i]) >> s) & 0xFF, b[-1] being the header's last partial byte and b[n] = 0 (aac_frame_byte).
// include/dabx.h "AAC stream" states the semantics.  The functions marked AAC_HD are the kernel's and, lane after lane,
// dabx_internal_aac_frame_host's (capi_stage.cpp): tests/test_aac_stream_cases.py holds them against the model without a device.
#pragma once
#include "pipeline.h"
#include "out_ring.h"

namespace dabx {

#define AAC_HD __host__ __device__ __forceinline__

constexpr int AAC_MAX_AU_BYTES = 960;                     // cAacCoreFrameBytes (:313)
constexpr int AAC_MAX_FRAME_BYTES = DABX_AAC_MAX_FRAME_BYTES;
static_assert(AAC_MAX_FRAME_BYTES == 11 + AAC_MAX_AU_BYTES / 255 + AAC_MAX_AU_BYTES, "include/dabx.h: DABX_AAC_MAX_FRAME_BYTES");
// The rings hold two batches of super frames whose AU tables are in order: a batch completes at most 6 super frames of at most 6 access
// units -> 72 -> 128 records; such a super frame's access units partition its 110 R bytes, an access unit takes L + 2 of them (its CRC)
// and gives 10 | 11 + L / 255 + L, at most 12 more, so a super frame emits at most 110 R + 72 bytes and a batch 6 times that.  A frame is
// written at n_bytes before n_bytes moves on: asm_room one frame.
constexpr uint32_t AAC_REC_RING = 128;
constexpr uint32_t AAC_DL_REC_CAP = 36;
AAC_HD uint32_t aac_batch_bytes(int kbps) { return 6u * (110u * (uint32_t)(kbps / 8) + 72u); }

// One slot with the mode on.  The job table of k_aac_stream is an array of these in HBM.
struct AacStreamSlot {
  OutRing<dabx_aac_frame> out;
  int32_t s, j;                       // stream, slot
  long long sf_seen;                  // super frames of the slot (SubchDev::sf_count) walked so far
  long long superframes, records, frames, frame_bytes, lost_len, lost_crc;      // dabx_aac_stream_stats
};
// k_aac_stream's argument, by value: the job table and what the kernel reads of the engine (launch_aac_stream_stage fills those in)
struct AacStreamDev {
  AacStreamSlot *slots;
  int32_t n;                          // slots = blocks of one wave
  int32_t max_subch, sf_stride, pad_;
  const SubchDev *subch;
  const uint8_t *sf_out;
  const dabx_superframe_info *sf_info;
};

// ---- the frame's pieces -----------------------------------------------------------------------------------------------------------------------
// size of the LOAS frame of an access unit of L bytes (:399-441: 69 / 78 bits, L / 255 + 1 length bytes, L bytes, rounded up)
AAC_HD int aac_frame_size(int sbr, int L) { return (sbr ? 11 : 10) + L / 255 + L; }

// Everything in front of PayloadLengthInfo: hi = its first 64 bits, tail = the 5 (no SBR) / 14 (SBR) bits behind them, right-aligned.
//   bits  0 .. 10  0x2B7 (:399)        11 .. 23  audioMuxLengthBytes = size - 3 (:400, bit_writer.cpp:54-59)
//        24 .. 39  0, 0, 1, 000000, 0000, 000 (:403-410) = 0x2000
//   no SBR (:423-426): 40 .. 44 AAC LC 00010, 45 .. 48 CoreSrIndex, 49 .. 52 CoreChConfig, 53 .. 55 100
//   SBR (:414-419):    40 .. 44 SBR 00101, 45 .. 48 CoreSrIndex, 49 .. 52 CoreChConfig, 53 .. 56 ExtensionSrIndex, 57 .. 61 00010, 62 .. 64 100
//   then (:429-432) 000, 0xFF, 0, 0
struct AacHeader { unsigned long long hi; unsigned tail; };
AAC_HD AacHeader aac_header(unsigned stream_parms, int size)
{
  const unsigned dac = (stream_parms >> 6) & 1u, sbr = (stream_parms >> 5) & 1u, chm = (stream_parms >> 4) & 1u;      // :259-261
  const unsigned long long sr = dac ? (sbr ? 6u : 3u) : (sbr ? 8u : 5u);       // :266 CoreSrIndex
  const unsigned long long ch = chm ? 2u : 1u;                                 // :267 CoreChConfig
  const unsigned long long ext = dac ? 3u : 5u;                                // :269 ExtensionSrIndex
  const unsigned long long front = (0x2B7ull << 53) | ((unsigned long long)((size - 3) & 0x1FFF) << 40) | (0x2000ull << 24);
  AacHeader h;
  if (sbr) { h.hi = front | (5ull << 19) | (sr << 15) | (ch << 11) | (ext << 7) | (2ull << 2) | 2ull; h.tail = 0x3FCu; }     // 0 000 11111111 00
  else     { h.hi = front | (2ull << 19) | (sr << 15) | (ch << 11) | (4ull << 8) | 0x1Full;           h.tail = 0x1Cu; }      // 111 00
  return h;
}

// byte j of what follows the header: PayloadLengthInfo (:435-439), the payload (:441); j = -1: the header's last partial byte, j past the
// end: the zero bits that fill the last byte
AAC_HD unsigned aac_body_byte(const AacHeader &h, int L, const uint8_t *au, int j)
{
  const int k = L / 255;
  if (j < 0) return h.tail;
  if (j < k) return 0xFFu;
  if (j == k) return (unsigned)(L - 255 * k);
  return j <= k + L ? (unsigned)au[j - k - 1] : 0u;
}

// byte i of the LOAS frame, 0 <= i < aac_frame_size(sbr, L)
AAC_HD unsigned aac_frame_byte(const AacHeader &h, int sbr, int L, const uint8_t *au, int i)
{
  if (i < 8) return (unsigned)(h.hi >> (56 - 8 * i)) & 0xFFu;
  if (sbr && i == 8) return (h.tail >> 6) & 0xFFu;
  const int j = i - (sbr ? 9 : 8), s = sbr ? 6 : 5;
  return (((aac_body_byte(h, L, au, j - 1) << 8) | aac_body_byte(h, L, au, j)) >> s) & 0xFFu;
}

// What k_aac_stream's lane a knows of access unit a of a super frame (:320-333 on k_dabplus's verdicts)
struct AacAu { int L, flags, length; };
AAC_HD AacAu aac_au(const dabx_superframe_info &inf, int a)
{
  AacAu u;
  u.L = (int)inf.au_start[a + 1] - (int)inf.au_start[a] - 2;                   // :322
  u.flags = ((inf.au_len_bad >> a) & 1) ? DABX_AAC_LOST_LEN : ((inf.au_crc_ok >> a) & 1) ? 0 : DABX_AAC_LOST_CRC;      // :325, :333, :377
  u.length = u.flags ? 0 : aac_frame_size((inf.stream_parms >> 5) & 1, u.L);
  return u;
}

// dabx_internal_aac_frame_host: the frame of one access unit, byte after byte as the kernel's lanes produce them
inline int aac_frame_host(const uint8_t *au, int L, unsigned stream_parms, uint8_t *out)
{
  const int sbr = (stream_parms >> 5) & 1, size = aac_frame_size(sbr, L);
  const AacHeader h = aac_header(stream_parms, size);
  for (int i = 0; i < size; i++) out[i] = (uint8_t)aac_frame_byte(h, sbr, L, au, i);
  return size;
}

}  // namespace dabx
