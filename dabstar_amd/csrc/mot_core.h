// mot_core.h -- MOT objects of the X-PAD: the per-slot state, the argument of k_mot (msc_stages.hip) and its device helpers.  The tail of
// PadHandler::_build_MSC_segment (base/backend/data/pad_handler.cpp:553-622: the MSC data group header) and the handler's one MotObject
// (base/backend/data/mot/mot_object.cpp:71-323, constructed at pad_handler.cpp:54 as a PAD element that is no directory element):
// set_header, add_body_segment, _check_if_complete, _handle_complete, reset.  k_mot walks the DABX_PAD_DATAGROUP items k_pad / k_pad_mp2
// have put into the slot's PAD rings (pad_core.h) -- it reads what they emit and changes nothing of theirs -- and every
// `emit signal_new_mot_object` becomes one dabx_mot_object record plus its bytes in the slot's own output rings (out_ring.h).
// include/dabx.h "MOT objects of the X-PAD" states the semantics, the quirks that are kept and the three guards M1..M3.
#pragma once
#include "pipeline.h"
#include "out_ring.h"
#include "pad_core.h"

namespace dabx {

constexpr int MOT_MAX_SEGMENTS = 8192;                 // add_body_segment refuses numbers from here on (mot_object.cpp:119)
constexpr uint32_t MOT_ABSENT = 0xFFFFFFFFu;           // MotSeg::len of a segment number that is not in the map
constexpr uint32_t MOT_NAME_ROOM = 8192;               // a name lies inside a header segment, and segmentSize has 13 bits: < 8192 bytes
constexpr uint32_t MOT_OBJECT_BYTES_DEFAULT = 65536, MOT_OBJECT_BYTES_MIN = 256, MOT_OBJECT_BYTES_MAX = 4u << 20;   // dabx_mot_config.max_object_bytes
// Ring sizes.  An object is written whole at its emit, inside one launch, so the rings' asm_room is 0.  Bytes: the largest item is
// max_object_bytes of body (guard M3) and fewer than MOT_NAME_ROOM bytes of name; the byte ring holds at least two of them (a power of
// two).  Records: one group emits at most one object and a batch brings at most 144 groups (pad_core.h), so 256 records hold everything of
// a batch until the next one; which of them still have their BYTES is out_ring_intact's to say -- repeated headers of a complete object
// re-emit it (mot_object.cpp:111-114), and a reader or a chunk that finds an object gone counts it in objects_lost.
constexpr uint32_t MOT_REC_RING = 256;
static_assert(144 <= MOT_REC_RING, "mot_core.h: the records of one batch");
constexpr uint32_t mot_byte_ring(uint32_t max_object_bytes)
{
  uint32_t p = 1;
  while (p < 2 * (max_object_bytes + MOT_NAME_ROOM)) p <<= 1;
  return p;
}
static_assert(mot_byte_ring(MOT_OBJECT_BYTES_MAX) == (16u << 20) && mot_byte_ring(MOT_OBJECT_BYTES_MIN) == 32768, "mot_core.h: byte ring sizes");
// Per chunk of the bulk delivery: 16 records, 2 * max_object_bytes bytes (include/dabx.h, dabx_chunk_mot)
constexpr uint32_t MOT_DL_REC_CAP = 16;

// MotObject's members (mot_object.h:78-86).  mMotMap is MotSlot::table + arena, mName is MotSlot::name with its length here;
// mStartSegment and mProgressMax are written and never read.
struct MotState {
  int32_t transport_id;           // mTransportId, -1 at the start
  int32_t num_segments;           // mNumOfSegments, -1: not known
  int32_t sum;                    // mSumSegmentSize = bytes of the arena in use
  int32_t n_stored;               // mMotMap.size()
  int32_t max_seg;                // the highest segment number in the map, -1: none (reset clears the table up to it)
  int32_t hdr_init;               // mHeaderCore.initialized
  int32_t body_size, header_size, content_type, content_subtype;      // mHeaderCore
  int32_t name_len;               // mName.size() in bytes; 0: the host forms "trid_<transport_id>" (mot_object.cpp:293-297)
  int32_t emits;                  // signal_new_mot_object since the last reset()
  int32_t progress_pct;           // the last signal_pad_mot_progress (:168)
  int32_t reserved;
};
struct MotCounters {              // dabx_mot_stats; one per decision of include/dabx.h "MOT objects of the X-PAD"
  long long groups, headers, segments, object_bytes;
  long long crc_bad, type_other, no_tid, grp_short, hdr_bad, seg_number_bad, seg_duplicate, resets, obj_overflow, pad_overrun, progress_events;
};
struct MotSeg { uint32_t off, len; };                  // a stored body segment: arena[off .. off + len); len == MOT_ABSENT: not in the map

// One MOT-enabled PAD slot.  The job table of k_mot is an array of these in HBM.  arena, name and table lie behind the byte ring in the
// ring's allocation (out.bytes), so the slot's memory is freed with its rings.
struct MotSlot {
  OutRing<dabx_mot_object> out;
  int32_t s, j;                   // stream, slot
  int32_t pad_index;              // the slot's place in the PAD job table (PadDev::slots); follows every upload of that table
  uint32_t max_object_bytes;      // guard M3
  long long items_seen;           // PAD items (PadSlot::out.count) walked so far
  MotState h;
  MotCounters c;
  uint8_t *arena;                 // [max_object_bytes] the stored segments' bytes in the order they arrived
  uint8_t *name;                  // [MOT_NAME_ROOM]
  MotSeg *table;                  // [MOT_MAX_SEGMENTS] direct-indexed by segment number
};
// the bytes behind the byte ring: arena, name, table (8-byte aligned: the ring and MOT_NAME_ROOM are powers of two >= 8)
constexpr size_t mot_extra_bytes(uint32_t max_object_bytes) { return (((size_t)max_object_bytes + 7) & ~(size_t)7) + MOT_NAME_ROOM + sizeof(MotSeg) * MOT_MAX_SEGMENTS; }

// k_mot's argument, by value: the job table and the PAD job table of the launch in front (launch_mot_stage fills that in)
struct MotDev {
  MotSlot *slots;
  int32_t n;                      // MOT slots = blocks of one wave
  int32_t max_subch;
  const PadSlot *pad_slots;
  int32_t n_pad, reserved;
};

#ifdef __HIPCC__
// What one wave carries through the groups of a launch.  Everything here is wave-uniform: header bytes come out of the PAD ring (or, for a
// MOT header segment, out of LDS) through pad_u, so the state machine is scalar; the lanes differ only inside the copies, the ballots over
// the table and the gather of an emit.
struct MotWave {
  MotState h;
  MotCounters c;
  const uint8_t *pad_ring;        // the PAD slot's byte ring
  unsigned long long pad_mask;
  uint8_t *arena, *name, *ring;
  MotSeg *table;
  dabx_mot_object *recs;
  unsigned long long bytes_mask, rec_mask;
  long long n_recs, n_bytes;
  uint32_t max_object_bytes;
  long long frame;                // of the PAD item being walked
  int au, lane;
  uint8_t *hdr;                   // LDS: the header segment being walked, MOT_NAME_ROOM bytes
};

// byte k of the group at byte_pos of the PAD ring, wave-uniform
__device__ __forceinline__ unsigned mot_g(const MotWave &w, long long pos, int k)
{
  return pad_u(w.pad_ring[(size_t)((unsigned long long)(pos + k) & w.pad_mask)]);
}

// reset() (mot_object.cpp:313-323); the table is cleared up to the highest number seen
__device__ __forceinline__ void mot_reset(MotWave &w)
{
  for (int i = w.lane; i <= w.h.max_seg; i += 64) w.table[i].len = MOT_ABSENT;
  w.h.num_segments = -1; w.h.sum = 0; w.h.n_stored = 0; w.h.max_seg = -1;
  w.h.hdr_init = 0; w.h.body_size = 0; w.h.header_size = 0; w.h.content_type = 0; w.h.content_subtype = 0;
  w.h.name_len = 0; w.h.emits = 0;
  w.c.resets++;
  __syncthreads();
}

// _check_if_complete (:240-278): ballots over the table, 64 entries per pass
__device__ __forceinline__ bool mot_complete(const MotWave &w)
{
  if (!w.h.hdr_init) return false;                               // :242
  if (w.h.num_segments < 0) return false;                        // :248
  if ((int)(int16_t)w.h.n_stored < w.h.num_segments) return false;      // :254
  for (int base = 0; base < w.h.num_segments; base += 64) {      // :262-269
    const int i = base + w.lane;
    const bool missing = i < w.h.num_segments && w.table[i].len == MOT_ABSENT;
    if (__ballot(missing)) return false;
  }
  return true;
}

// _handle_complete (:281-301): ALL stored segments in key order -- those numbered at or above mNumOfSegments too -- straight into the byte
// ring, then the name; lane 0 writes the record.  Per pass of 64 table entries the lanes' lengths are prefix-summed and the wave copies one
// present segment after the other to its place.
__device__ __forceinline__ void mot_emit(MotWave &w)
{
  long long at = w.n_bytes;
  for (int base = 0; base <= w.h.max_seg; base += 64) {
    const int i = base + w.lane;
    MotSeg q{0u, MOT_ABSENT};
    if (i <= w.h.max_seg) q = w.table[i];
    const bool present = q.len != MOT_ABSENT;
    unsigned incl = present ? q.len : 0u;                        // inclusive prefix sum of the lengths over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)incl, d);
      if (w.lane >= d) incl += up;
    }
    const unsigned excl = incl - (present ? q.len : 0u);
    for (unsigned long long m = __ballot(present); m; m &= m - 1) {
      const int l = __ffsll((long long)m) - 1;
      const unsigned off = pad_u((unsigned)__shfl((int)q.off, l)), len = pad_u((unsigned)__shfl((int)q.len, l)), to = pad_u((unsigned)__shfl((int)excl, l));
      for (unsigned k = w.lane; k < len; k += 64) w.ring[(size_t)((unsigned long long)(at + to + k) & w.bytes_mask)] = w.arena[off + k];
    }
    at += pad_u((unsigned)__shfl((int)incl, 63));
  }
  const int body_len = (int)(at - w.n_bytes);                    // == mSumSegmentSize
  for (int k = w.lane; k < w.h.name_len; k += 64) w.ring[(size_t)((unsigned long long)(at + k) & w.bytes_mask)] = w.name[k];
  const unsigned content = (((unsigned)w.h.content_type << 8) & 0x3F00u) | ((unsigned)w.h.content_subtype & 0xFFu);      // get_content_type, mot_object.h:71-75
  const unsigned repeat = w.h.emits < 255 ? (unsigned)w.h.emits : 255u;
  if (w.lane == 0) {                     // the 32 bytes of a dabx_mot_object as four little-endian words (no record on the stack)
    unsigned long long *o = reinterpret_cast<unsigned long long *>(w.recs + (size_t)((unsigned long long)w.n_recs & w.rec_mask));
    o[0] = (unsigned long long)w.n_bytes; o[1] = (unsigned long long)w.frame;
    o[2] = (unsigned long long)(unsigned)body_len | ((unsigned long long)(unsigned)w.h.body_size << 32);
    o[3] = (unsigned long long)((unsigned)w.h.transport_id & 0xFFFFu) | ((unsigned long long)content << 16) |
           ((unsigned long long)((unsigned)w.h.name_len & 0xFFFFu) << 32) | ((unsigned long long)(w.au & 0xFF) << 48) | ((unsigned long long)repeat << 56);
  }
  w.n_recs++; w.n_bytes = at + w.h.name_len;
  w.c.object_bytes += body_len + w.h.name_len;
  if (w.h.emits < 0x7FFFFFFF) w.h.emits++;
}

// set_header (:71-115) on the segsize >= 7 bytes at `seg` of the group (guard M2 in front, by the caller)
__device__ __forceinline__ void mot_set_header(MotWave &w, long long pos, int seg, int segsize, int tid)
{
  if (w.h.transport_id != tid) mot_reset(w);                     // :75-79
  w.h.transport_id = tid;                                        // :81
  __syncthreads();                                               // the previous header's bytes are done with
  for (int k = w.lane; k < segsize; k += 64) w.hdr[k] = w.pad_ring[(size_t)((unsigned long long)(pos + seg + k) & w.pad_mask)];
  __syncthreads();
  const uint8_t *s = w.hdr;
  const unsigned s3 = pad_u(s[3]), s5 = pad_u(s[5]);
  w.h.body_size = (int)((pad_u(s[0]) << 20) | (pad_u(s[1]) << 12) | (pad_u(s[2]) << 4) | (s3 >> 4));      // :84 b55..b28
  w.h.header_size = (int)(((s3 & 0x0Fu) << 9) | (pad_u(s[4]) << 1) | (s5 >> 7));                           // :85 b27..b15
  w.h.content_type = (int)((s5 >> 1) & 0x3Fu);                   // :86 b14..b9
  w.h.content_subtype = (int)(((s5 & 1u) << 8) | pad_u(s[6]));   // :87 b8..b0
  w.h.hdr_init = 1;                                              // :95
  w.c.headers++;
  int p = 7;                                                     // :99
  while (p < w.h.header_size) {                                  // :101 _process_header_extension (:210-238)
    if (p >= segsize) { w.c.hdr_bad++; break; }                  // M2: the parameter byte
    const unsigned b = pad_u(s[p]);
    const unsigned pli = b >> 6, id = b & 0x3Fu;
    if (pli == 0) { p += 1; continue; }                          // :219
    if (pli == 1) { p += 2; continue; }                          // :220
    if (pli == 2) { p += 5; continue; }                          // :221
    if (p + 1 >= segsize) { w.c.hdr_bad++; break; }              // M2: the length byte
    const unsigned b1 = pad_u(s[p + 1]);
    int length, q;
    if (b1 & 0x80u) {                                            // :223-227
      if (p + 2 >= segsize) { w.c.hdr_bad++; break; }            // M2: the second length byte
      length = (int)(((b1 & 0x7Fu) << 8) | pad_u(s[p + 2]));
      q = p + 3;
    } else {                                                     // :228-232
      length = (int)(b1 & 0x7Fu);
      q = p + 2;
    }
    // _process_parameter_id (:177-208)
    if (id == 0x0C) {                                            // :181-189 ContentName: bytes [q + 1, q + length)
      if (length >= 2 && q + length > segsize) { w.c.hdr_bad++; break; }      // M2: a name byte
      const int n = length >= 1 ? length - 1 : 0;
      __syncthreads();
      for (int k = w.lane; k < n; k += 64) w.name[k] = s[q + 1 + k];
      w.h.name_len = n;
      p = q + length;
    } else if ((id >= 0x02 && id <= 0x08) || id == 0x0A || id == 0x0B || id == 0x0F) {
      p = q;                                                     // :191-201 the pointer is NOT moved past the value: its bytes are walked as parameters
    } else {
      p = q + length;                                            // :203-206
    }
  }
  __syncthreads();                                               // the name's bytes are in memory
  if (mot_complete(w)) mot_emit(w);                              // :111-114
}

// add_body_segment (:117-175) on the segsize bytes at `seg` of the group.  PAD_ELEMENT: mIsPadElement (:160); false for the objects of a
// packet-mode carousel (carousel_core.h), which signal no progress
template <bool PAD_ELEMENT = true>
__device__ __forceinline__ void mot_add_body(MotWave &w, long long pos, int seg, int number, int segsize, bool last, int tid)
{
  if (number < 0 || number >= MOT_MAX_SEGMENTS) { w.c.seg_number_bad++; return; }      // :119-123
  if (w.h.transport_id != tid) { mot_reset(w); w.h.transport_id = tid; }                // :125-130
  if (pad_u(w.table[number].len) != MOT_ABSENT) { w.c.seg_duplicate++; return; }        // :139-143
  if ((long long)w.h.sum + segsize > (long long)w.max_object_bytes) {                   // M3: the object is reset, the transport id stays
    mot_reset(w);
    w.c.obj_overflow++;
    return;
  }
  for (int k = w.lane; k < segsize; k += 64) w.arena[w.h.sum + k] = w.pad_ring[(size_t)((unsigned long long)(pos + seg + k) & w.pad_mask)];      // :135-136
  if (w.lane == 0) w.table[number] = MotSeg{(uint32_t)w.h.sum, (uint32_t)segsize};
  w.h.sum += segsize;                                            // :137
  w.h.n_stored++;
  if (number > w.h.max_seg) w.h.max_seg = number;
  w.c.segments++;
  if (last) w.h.num_segments = number + 1;                       // :145-148
  if (PAD_ELEMENT && w.h.body_size > 0 && w.h.content_type == 2) { // :160 a PAD element, base type image ((contentType << 8 & 0x3f00) >> 8 == MOTBaseTypeImage)
    int pct = (int)(100ll * w.h.sum / w.h.body_size);            // :162 (the reference's i32 product cannot overflow below 21 MiB; M3 bounds the sum at 4 MiB)
    if (pct > 100) pct = 100;                                    // :163-167
    w.h.progress_pct = pct;                                      // :168
    w.c.progress_events++;
  }
  __syncthreads();                                               // the segment and its table entry are in memory
  if (mot_complete(w)) mot_emit(w);                              // :171-174
}

// The tail of _build_MSC_segment (pad_handler.cpp:539-622) on one DABX_PAD_DATAGROUP item: `length` bytes at `pos` of the PAD ring with
// the verdicts k_pad recorded.  Guard M1: a read at or beyond `length` ends the group, state unchanged.
__device__ __forceinline__ void mot_group(MotWave &w, long long pos, int length, bool crc_flag, bool crc_ok)
{
  w.c.groups++;
  if (crc_flag && !crc_ok) { w.c.crc_bad++; return; }            // :539-545
  const unsigned b0 = mot_g(w, pos, 0);                          // (an item has at least 2 bytes, :530)
  const int type = (int)(b0 & 0x0Fu);                            // :524, :554 DataGroupType
  if (type != 3 && type != 4) { w.c.type_other++; return; }      // :556-560
  int index = (b0 & 0x80u) ? 4 : 2;                              // :564 ExtensionFlag
  int number = -1;                                               // :553
  bool last = false;
  if (b0 & 0x20u) {                                              // :567 SegmentFlag
    if (index + 2 > length) { w.c.grp_short++; return; }         // M1
    const unsigned a = mot_g(w, pos, index);
    last = (a & 0x80u) != 0;                                     // :569
    number = (int)(((a & 0x7Fu) << 8) | mot_g(w, pos, index + 1));      // :570 (an i16: 0 .. 32767)
    index += 2;
  }
  int tid = 0;
  bool tid_flag = false;
  if (b0 & 0x10u) {                                              // :579 UserAccessFlag
    if (index + 1 > length) { w.c.grp_short++; return; }         // M1
    const unsigned a = mot_g(w, pos, index);
    tid_flag = (a & 0x10u) != 0;                                 // :583
    if (tid_flag) {
      if (index + 3 > length) { w.c.grp_short++; return; }       // M1 (the id is read whatever lengthIndicator says, :587)
      tid = (int)((mot_g(w, pos, index + 1) << 8) | mot_g(w, pos, index + 2));
    }
    index += 1 + (int)(a & 0x0Fu);                               // :589
  }
  if (!tid_flag) { w.c.no_tid++; return; }                       // :593-597
  if (index + 2 > length) { w.c.grp_short++; return; }           // M1: the segmentation header
  const int segsize = (int)(((mot_g(w, pos, index) & 0x1Fu) << 8) | mot_g(w, pos, index + 1));      // :605
  if (index + 2 + segsize > length) { w.c.grp_short++; return; } // M1: the segment
  if (type == 3) {                                               // :611-613
    if (segsize < 7) { w.c.hdr_bad++; return; }                  // M2: no header core
    mot_set_header(w, pos, index + 2, segsize, tid);
  } else {                                                       // :615-617
    mot_add_body(w, pos, index + 2, number, segsize, last, tid);
  }
}
#endif

}  // namespace dabx
