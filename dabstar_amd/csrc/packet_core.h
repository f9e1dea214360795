// packet_core.h -- packet-mode data sub-channels: the per-slot state, the argument of k_packet (msc_stages.hip) and its device helpers.
// DataProcessor (base/backend/data/data_processor.cpp:106-254): packet walk, address filter, continuity index, packet CRC and the
// assembly of the MSC data groups.  include/dabx.h "Packet-mode data sub-channels" states the semantics and the two guards.
#pragma once
#include "pipeline.h"
#include "out_ring.h"
#ifdef __HIPCC__
#include "fec_core.h"
#endif

namespace dabx {

// One packet-mode slot: DataProcessor's members (data_processor.h: mPacketAddress, mExpectedIndex, mPacketState, mSeriesVec), the slot's
// output rings (out_ring.h: one record per completed group) and its counters.  The job table of k_packet is an array of these, packet-mode
// slots only, in HBM; the kernel's own arrays, none of them part of EngineDev / SubchDev.
//
// The series under assembly is kept IN the byte ring, at the place the completed group will have: bytes [out.n_bytes, out.n_bytes + fill) of
// the slot's data-group byte sequence.  Completing the group moves n_bytes on, abandoning the series leaves it: no second buffer, no copy.
// The ring's asm_room is DABX_DG_MAX_BYTES, the bound of a series.
struct PacketSlot {
  OutRing<dabx_datagroup_info> out;
  int32_t s, j;                   // stream, slot
  int32_t address;                // mPacketAddress
  int32_t expected;               // mExpectedIndex
  int32_t state;                  // mPacketState: 0 waiting for a start, 1 within a series
  int32_t fill;                   // bytes of the series so far (mSeriesVec.size() / 8)
  int32_t first_byte;             // byte 0 of the series, -1 while it is empty (the data-group CRC flag is its bit 6)
  uint32_t run_crc;               // CCITT register (start value 0xFFFF) over the series so far
  long long first_frame;          // logical frame of the packet that started the series
  long long frames, packets, addr_match, continuity_err, crc_bad, len_bad, walk_short, dg_crc_bad, dg_overflow;      // (dg_count, dg_bytes: out.count, out.n_bytes)
};

// k_packet's argument, by value: the job table and what the kernel reads of the engine (the MSC batch's snapshot, the slots' descriptions
// and the ring of logical frames; launch_packet_stage fills those in).
struct PacketDev {
  PacketSlot *slots;
  int32_t n;                      // packet-mode slots = blocks of one wave
  int32_t max_subch, msc_stride;
  const SubchDev *subch;
  const BatchSnap *snap;
  const uint8_t *msc_out;
  const uint16_t *crc_ccitt, *crc_xpow;
};

constexpr int PKT_MAX_KBPS = 384;                      // 1152-byte logical frames: 48 granules of 24 bytes, one lane each
constexpr int PKT_GRANULE = 24;
constexpr unsigned PKT_CRC_RESIDUE = 0x1D0Fu;          // the CCITT register (start 0xFFFF) after a message followed by its complemented CRC

#ifdef __HIPCC__
// Stages logical frame f of a slot in LDS for its wave (k_packet, k_pad_mp2): `ring` = the slot's MSC_SLOTS frames in msc_out, nbytes = 3 kbps
// <= 3 * PKT_MAX_KBPS, a multiple of 4.  The barrier in front says the previous frame (and whatever else the wave put into LDS) is done with,
// the one behind that the frame is there.
__device__ __forceinline__ void slot_stage_frame(uint8_t *frm, const uint8_t *ring, int msc_stride, long long f, int nbytes, int lane)
{
  __syncthreads();
  const uint32_t *src = reinterpret_cast<const uint32_t *>(ring + (size_t)(f % MSC_SLOTS) * msc_stride);
  for (int i = lane; i < nbytes / 4; i += 64) reinterpret_cast<uint32_t *>(frm)[i] = src[i];
  __syncthreads();
}

// the packets of one logical frame (data_processor.cpp:123-150) from the length codes of its granules: bit g of the result = a packet starts
// at granule g.  b0 / b1 = the two bits of every granule's first byte's length code as lane masks; wave-uniform, scalar work.  *walk_short:
// the walk ended at a packet that needs more bytes than remain (:129-133).
__device__ __forceinline__ unsigned long long pkt_walk(unsigned long long b0, unsigned long long b1, int n_gran, bool *walk_short)
{
  unsigned long long starts = 0;
  int pos = 0;
  *walk_short = false;
  while (pos < n_gran) {
    const int len = 1 + (int)((b0 >> pos) & 1ull) + 2 * (int)((b1 >> pos) & 1ull);      // (bits 0..1 + 1) granules
    if (pos + len > n_gran) { *walk_short = true; break; }
    starts |= 1ull << pos;
    pos += len;
  }
  return starts;
}

// The CCITT register from start value 0 over granule g: all granules of the frame in parallel, 24 look-ups each.  A packet's register is
// then folded from those of its granules (c = c * x^(8 * 24) + part), not walked byte by byte by one lane.
__device__ __forceinline__ unsigned pkt_granule_crc(const uint8_t *frm, int g, const uint16_t *s_crc)
{
  const uint8_t *p = frm + g * PKT_GRANULE;
  unsigned c = 0;
#pragma unroll
  for (int i = 0; i < PKT_GRANULE; i++) c = (s_crc[(p[i] ^ (c >> 8)) & 0xFF] ^ (c << 8)) & 0xFFFFu;
  return c;
}

// What the state machine needs of one packet, packed: bit 0 address matches, 1 packet CRC holds, 2 the payload lies inside the logical
// frame, 3-4 continuity index, 5-6 first/last, 7-13 useful length, 16-31 the CCITT register over the payload from start value 0.
// s_part: pkt_granule_crc of every granule of the frame; s_xpow[m] = x^(8 m) mod P, m <= 127.
__device__ __forceinline__ unsigned pkt_describe(const uint8_t *frm, int g0, int frame_bytes, int address, const uint16_t *s_crc,
                                                 const uint16_t *s_part, const uint16_t *s_xpow)
{
  const int start = g0 * PKT_GRANULE;
  const uint8_t *p = frm + start;
  const int n_g = (p[0] >> 6) + 1;                                                         // :158 packet length in granules
  const unsigned ci = (p[0] >> 4) & 3u, fl = (p[0] >> 2) & 3u;                             // :159-160
  const int addr = ((p[0] & 3) << 8) | p[1], ulen = p[2] & 0x7F;                           // :161-163
  if (addr != address) return 0u;                                                          // :165
  const unsigned x24 = s_xpow[PKT_GRANULE];
  // check_CRC_bits (crc.cpp:98-132): register all ones, the last 16 bits inverted, remainder zero -- the same as: the register, started
  // at 0xFFFF and run over the WHOLE packet, its complemented CRC included, ends at the residue
  unsigned crc = 0xFFFFu;
  for (int k = 0; k < n_g; k++) crc = crc_mulmod(crc, x24) ^ s_part[g0 + k];
  const bool ok = crc == PKT_CRC_RESIDUE;
  const bool inside = start + 3 + ulen <= frame_bytes;
  unsigned part = 0;
  if (ok && inside) {
    // register over the payload [3, 3 + ulen) from 0 = (register over [0, 3 + ulen)) + (register over the 3 header bytes) * x^(8 ulen):
    // whole granules folded, fewer than 24 bytes walked
    const int end = 3 + ulen, full = end / PKT_GRANULE, rem = end - full * PKT_GRANULE;
    unsigned pre = 0, hdr = 0;
    for (int k = 0; k < full; k++) pre = crc_mulmod(pre, x24) ^ s_part[g0 + k];
    const uint8_t *q = p + full * PKT_GRANULE;
    for (int i = 0; i < rem; i++) pre = (s_crc[(q[i] ^ (pre >> 8)) & 0xFF] ^ (pre << 8)) & 0xFFFFu;
#pragma unroll
    for (int i = 0; i < 3; i++) hdr = (s_crc[(p[i] ^ (hdr >> 8)) & 0xFF] ^ (hdr << 8)) & 0xFFFFu;
    part = pre ^ crc_mulmod(hdr, s_xpow[ulen]);
  }
  return 1u | (ok ? 2u : 0u) | (inside ? 4u : 0u) | (ci << 3) | (fl << 5) | ((unsigned)ulen << 7) | (part << 16);
}
#endif

}  // namespace dabx
