// pad_core.h -- programme-associated data of DAB+ access units and of DAB (MP2) audio frames: the per-slot state, the argument of k_pad and
// k_pad_mp2 (msc_stages.hip) and their device helpers.  mp4processor.cpp:345-353 (the data stream element of an access unit) and PadHandler (base/backend/data/pad_handler.cpp:67-547):
// F-PAD dispatch, short and variable X-PAD, the dynamic label, the data-group length indicator and the assembly of the X-PAD MSC data
// groups, up to the two hand-over points (the label's bytes in front of the charset conversion, the data group in front of the MOT
// parser).  include/dabx.h "Programme-associated data" states the semantics and the four guards G1..G4.  For a DAB (MP2) slot the front of
// the walk is Mp2Processor's (base/backend/audio/mp2processor.cpp:250-285, :611-747): MP2 frame sync over the logical frames' bits and the
// PAD at the end of the logical frame in which an MP2 frame completes; Mp2State and the mp2_* helpers below.
#pragma once
#include "pipeline.h"
#include "out_ring.h"
#ifdef __HIPCC__
#include "fec_core.h"
#include "wave_ops.h"
#endif

namespace dabx {

// PadHandler's members (pad_handler.h:68-86).  mDynamicLabelTextUnConverted and mShortPadData are PadSlot::dl_text / short_data with their
// sizes here; mMscDataGroupBuffer is `fill` bytes of the slot's byte ring (below); mDataBuffer is a view of the staged X-PAD.
struct PadState {
  int32_t charset;                // mCharSet (EbuLatin = 0)
  int32_t last_app_type;          // mLastAppType
  int32_t msc_group_element;      // mMscGroupElement
  int32_t xpad_length;            // mXPadLength, -1 at the start
  int32_t still_to_go;            // mStillToGo
  int32_t short_n;                // mShortPadData.size() <= 16
  int32_t last_segment, first_segment;   // mLastSegment, mFirstSegment
  int32_t segment_number;         // mSegmentNumber (written at :140, read nowhere)
  int32_t dg_length;              // mDataGroupLength
  int32_t fill;                   // mMscDataGroupBuffer.size()
  int32_t segment_no;             // mSegmentNo, -1 at the start
  int32_t remain;                 // mRemainDataLength
  int32_t is_last_segment;        // mIsLastSegment
  int32_t more_xpad;              // mMoreXPad
  int32_t dl_len;                 // mDynamicLabelTextUnConverted.size() <= DABX_DL_MAX_BYTES (G4)
};
struct PadCounters {              // dabx_pad_stats
  long long superframes, aus, pad_aus, fpad_other, xpad_short, xpad_variable, xpad_other, pad_bad, li_bad, labels, label_bytes, dl_overflow,
            groups, group_bytes, dg_crc_bad, dg_small;
};

// The largest span of the byte ring the device may write beyond n_bytes before it moves n_bytes on (the ring's asm_room): the group under assembly -- fewer
// than mDataGroupLength <= 16 383 bytes before an append, at most 196 more after it (a no-CI continuation is mXPadLength bytes long, :224)
// -- moved up once by a label of at most DABX_DL_MAX_BYTES that is emitted while the group is open.  16 382 + 196 + 256 < 16 896.
constexpr int PAD_ASM_ROOM = 16896;
// Ring sizes (powers of two): what TWO full batches can emit plus PAD_ASM_ROOM.  A batch completes at most 6 super frames (28 new logical
// frames + 4 waiting, SF_SLOTS) of at most 6 access units; one X-PAD has at most 4 sub-fields (four contents indicators, :254-262) and a
// sub-field emits at most one item (one signal_show_label or one _build_MSC_segment call): 6 * 6 * 4 = 144 items per batch, 288 -> 512.
// Bytes: a label item is at most DABX_DL_MAX_BYTES; the data-group items of a batch are together at most the bytes that were under
// assembly (< PAD_ASM_ROOM) plus <= 48 per sub-field (< a label's 256): 2 * 144 * 256 + PAD_ASM_ROOM + PAD_ASM_ROOM = 107 520 -> 131 072.
// An MP2 source slot (k_pad_mp2) stays inside the same bound: a batch walks at most 28 logical frames, a logical frame completes at most one
// MP2 frame (mp2processor.cpp:691: lf is at least the logical frame's bits) and so hands on at most one X-PAD of at most 4 sub-fields:
// 28 * 4 = 112 <= 144 items, and the bytes follow as above.
constexpr uint32_t PAD_ITEM_RING = 512;
constexpr uint32_t PAD_BYTE_RING = 131072;
static_assert(4 * MSC_BATCH_FRAMES * 4 <= 144, "pad_core.h: the items of an MP2 source slot per batch");
static_assert(2 * 144 <= PAD_ITEM_RING && 2 * 144 * DABX_DL_MAX_BYTES + 2 * PAD_ASM_ROOM <= PAD_BYTE_RING, "pad_core.h: ring sizes");
// Per chunk of the bulk delivery (one batch): 144 items, 144 * 256 + PAD_ASM_ROOM bytes.
constexpr uint32_t PAD_DL_ITEM_CAP = 144;
constexpr uint32_t PAD_DL_BYTES_CAP = 144 * DABX_DL_MAX_BYTES + PAD_ASM_ROOM;

// Mp2Processor's sync members (mp2processor.h:85-90, mp2processor.cpp:236-240) and what dabx_mp2_sync_stats counts.  Of MP2frame only the
// 24 header bits are ever read for our purpose (_get_mp2_sample_rate, :271-285): the first 12 are the sync word's ones, the other 12 are
// collected in `header` while the state is GetSampleRate (a header may straddle a logical-frame boundary).
enum { MP2_SEARCHING = 0, MP2_GET_RATE = 1, MP2_GET_DATA = 2 };          // ESyncState, dabx_mp2_sync_stats.state
struct Mp2State {
  int32_t state;                  // MP2SyncState
  int32_t header_count;           // MP2headerCount: the run of ones in front of the next bit (< 12)
  int32_t bit_count;              // MP2bitCount
  int32_t sample_rate;            // sampleRate: 48 000 at the start, sticky (:250-264)
  int32_t header;                 // bits 12 .. MP2bitCount - 1 of MP2frame while state == MP2_GET_RATE
  int32_t last_sync_bit;          // bit index in its logical frame of the 12th one of the last sync word, -1: none yet
  long long syncs, frames, hdr_refused, rate_unsupported;
};

// One PAD-enabled slot.  The job table of k_pad and k_pad_mp2 is an array of these, PAD slots only, in HBM; none of it is part of EngineDev /
// SubchDev.  Labels and groups share the slot's output rings (out_ring.h) in emission order.  The group under assembly is kept IN the byte
// ring where the completed group will be: bytes [out.n_bytes, out.n_bytes + fill) (as packet_core.h keeps its series).  A label emitted
// while a group is open moves those bytes up by the label's length first.  The ring's asm_room is PAD_ASM_ROOM.
struct PadSlot {
  OutRing<dabx_pad_item> out;
  int32_t s, j;                   // stream, slot
  long long sf_seen;              // super frames of the slot (SubchDev::sf_count) walked so far
  PadState h;
  uint8_t short_data[16];         // mShortPadData: one byte from :151 and at most mStillToGo <= 15 more
  uint8_t dl_text[DABX_DL_MAX_BYTES];
  PadCounters c;
  // behind everything k_pad reads: the slot's source (DABX_PAD_SOURCE_*) and the front of k_pad_mp2's walk
  int32_t source, reserved;
  Mp2State m;
};

// k_pad's and k_pad_mp2's argument, by value: the job table and what the kernel reads of the engine (launch_pad_stage fills those in).
struct PadDev {
  PadSlot *slots;
  int32_t n;                      // PAD slots = blocks of one wave
  int32_t max_subch, sf_stride;
  const SubchDev *subch;
  const uint8_t *sf_out;
  const dabx_superframe_info *sf_info;
  const uint16_t *crc_ccitt, *crc_xpow;
  // k_pad_mp2: slots with source MP2 among the n (the kernel is launched only when there is one), and the logical frames of the batch
  int32_t n_mp2, msc_stride;
  const BatchSnap *snap;
  const uint8_t *msc_out;
};

#ifdef __HIPCC__
// What one wave carries through the access units of a launch.  Everything here is wave-uniform: header bytes come out of LDS through
// pad_u, so the state machine is scalar work and its branches are scalar branches; the lanes differ only inside the copies and the CRC.
struct PadWave {
  PadState h;
  PadCounters c;
  uint8_t *ring;
  dabx_pad_item *items;
  unsigned long long bytes_mask, item_mask;
  long long n_items, n_bytes;
  long long frame;                // dabx_superframe_info.first_frame of the super frame being walked
  int au, lane;
  uint8_t *text, *shortd;         // LDS: dl_text, short_data
  const uint16_t *s_crc, *s_xpow; // LDS: CCITT table, x^(8 m) mod P for m < 1024
};

// The wave's LDS, declared __shared__ by the kernel: the PAD bytes being walked and the slot's tables for the launch.
struct PadLds {
  __attribute__((aligned(16))) uint16_t xpow[1024];              // x^(8 m) mod P
  uint16_t crc[256];                                             // CCITT table
  uint8_t rb[256];                                               // the PAD reversed: rb[0] = L0, rb[1] = L1, rb[2 + k] = the X-PAD from its end (pad_process)
  uint8_t text[DABX_DL_MAX_BYTES], shortd[16];                   // PadSlot::dl_text, short_data
};
// Opens the slot for the launch: tables and the slot's label text and short X-PAD bytes into LDS (the caller's next barrier publishes them),
// PadHandler's state and the output rings' cursors into registers.  pad_wave_close puts back what the launch changed; whatever else a
// kernel keeps per slot (k_pad: sf_seen, k_pad_mp2: m) is its own to store.
__device__ __forceinline__ void pad_wave_open(PadWave &w, const PadSlot &ps, const PadDev &pd, PadLds &lds, int lane)
{
  static_assert(DABX_DL_MAX_BYTES == 256, "pad_core.h: the label text is loaded beside the 256-entry CCITT table");
  for (int i = lane; i < 256; i += 64) { lds.crc[i] = pd.crc_ccitt[i]; lds.text[i] = ps.dl_text[i]; }
  for (int i = lane; i < 128; i += 64) reinterpret_cast<uint4 *>(lds.xpow)[i] = reinterpret_cast<const uint4 *>(pd.crc_xpow)[i];
  if (lane < 16) lds.shortd[lane] = ps.short_data[lane];
  w.h = ps.h; w.c = ps.c;
  w.ring = ps.out.bytes; w.items = ps.out.recs; w.bytes_mask = ps.out.bytes_mask; w.item_mask = ps.out.rec_mask;
  w.n_items = ps.out.count; w.n_bytes = ps.out.n_bytes;
  w.lane = lane; w.au = 0; w.text = lds.text; w.shortd = lds.shortd; w.s_crc = lds.crc; w.s_xpow = lds.xpow;
}
__device__ __forceinline__ void pad_wave_close(const PadWave &w, PadSlot &ps, const PadLds &lds, int lane)
{
  __syncthreads();
  for (int i = lane; i < DABX_DL_MAX_BYTES; i += 64) ps.dl_text[i] = lds.text[i];
  if (lane < 16) ps.short_data[lane] = lds.shortd[lane];
  if (lane == 0) { ps.h = w.h; ps.c = w.c; ps.out.count = w.n_items; ps.out.n_bytes = w.n_bytes; }
}

__device__ __forceinline__ unsigned pad_u(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned pad_crc_step(unsigned c, unsigned b, const uint16_t *s_crc) { return (s_crc[(b ^ (c >> 8)) & 0xFF] ^ (c << 8)) & 0xFFFFu; }

// ContInd::get_length (:44, :48): 4, 6, 8, 12, 16, 24, 32, 48 by the top three bits
__device__ __forceinline__ int pad_ci_length(unsigned ci) { return (int)((0x302018100C080604ull >> (8 * (ci >> 5))) & 0xFFull); }

// x^(8 m) mod P for m < 16 384 from the table of the first 1024: x^(8 m) = x^(8 (m & 1023)) * (x^(8 * 1024))^(m >> 10)
__device__ __forceinline__ unsigned pad_xpow(const uint16_t *s_xpow, int m)
{
  unsigned r = s_xpow[m & 1023], b = crc_mulmod(s_xpow[1023], s_xpow[1]);
  for (int hi = m >> 10; hi; hi >>= 1) {
    if (hi & 1) r = crc_mulmod(r, b);
    b = crc_mulmod(b, b);
  }
  return r;
}

// check_crc_bytes(iData, size - 2) (crc.cpp:89-96) over the `size` >= 2 bytes at n_bytes of the byte ring.  Not one lane walking up to
// 16 KB: every lane runs the register from 0 over its own slice, the slice registers are moved to the end of the message with x^(8 n) and
// folded (the register is linear in the message); the 0xFFFF start value is one more term.  All lanes active.
__device__ __forceinline__ bool pad_ring_check_crc(const PadWave &w, int size)
{
  const int m = size - 2;
  const int per = (m + 63) >> 6, from = min(m, w.lane * per), to = min(m, from + per);
  unsigned c = 0;
  for (int i = from; i < to; i++) c = pad_crc_step(c, w.ring[(size_t)((unsigned long long)(w.n_bytes + i) & w.bytes_mask)], w.s_crc);
  unsigned acc = from < to ? crc_mulmod(c, pad_xpow(w.s_xpow, m - to)) : 0u;
  if (w.lane == 0) acc ^= crc_mulmod(0xFFFFu, pad_xpow(w.s_xpow, m));
  acc = wave_xor(acc);
  const unsigned want = ((unsigned)w.ring[(size_t)((unsigned long long)(w.n_bytes + m) & w.bytes_mask)] << 8) |
                        w.ring[(size_t)((unsigned long long)(w.n_bytes + m + 1) & w.bytes_mask)];
  return pad_u((~acc) & 0xFFFFu) == pad_u(want);
}

__device__ __forceinline__ void pad_put_item(PadWave &w, int length, int kind, int charset, int crc_flag, int crc_ok)
{
  if (w.lane == 0) {                     // the 32 bytes of a dabx_pad_item as four little-endian words (no record on the stack)
    unsigned long long *o = reinterpret_cast<unsigned long long *>(w.items + (size_t)((unsigned long long)w.n_items & w.item_mask));
    o[0] = (unsigned long long)w.n_bytes; o[1] = (unsigned long long)w.frame;
    o[2] = (unsigned long long)(length & 0xFFFF) | ((unsigned long long)(kind & 0xFF) << 16) | ((unsigned long long)(w.au & 0xFF) << 24) |
           ((unsigned long long)(charset & 0xFF) << 32) | ((unsigned long long)(crc_flag & 1) << 40) | ((unsigned long long)(crc_ok & 1) << 48);
    o[3] = 0;
  }
  w.n_items++; w.n_bytes += length;
}

// mDynamicLabelTextUnConverted.append (:163, :183, :407, :446) with guard G4: an append that would pass DABX_DL_MAX_BYTES is dropped whole
__device__ __forceinline__ void pad_text_append(PadWave &w, const uint8_t *src, int n)
{
  if (w.h.dl_len + n > DABX_DL_MAX_BYTES) { w.c.dl_overflow++; return; }
  for (int i = w.lane; i < n; i += 64) w.text[w.h.dl_len + i] = src[i];
  w.h.dl_len += n;
  __syncthreads();
}

// emit signal_show_label (:144, :193, :416, :452): the text as it stands, and mCharSet.  A group under assembly moves up by the label's
// length, chunk by chunk from the top, every chunk read before it is written.
__device__ __forceinline__ void pad_emit_label(PadWave &w)
{
  const int len = w.h.dl_len;
  if (len > 0 && w.h.fill > 0) {
    for (int top = w.h.fill; top > 0; top -= 64) {
      const int i = top - 64 + w.lane;
      uint8_t v = 0;
      if (i >= 0) v = w.ring[(size_t)((unsigned long long)(w.n_bytes + i) & w.bytes_mask)];
      __syncthreads();
      if (i >= 0) w.ring[(size_t)((unsigned long long)(w.n_bytes + i + len) & w.bytes_mask)] = v;
      __syncthreads();
    }
  }
  for (int i = w.lane; i < len; i += 64) w.ring[(size_t)((unsigned long long)(w.n_bytes + i) & w.bytes_mask)] = w.text[i];
  pad_put_item(w, len, DABX_PAD_LABEL, w.h.charset, 0, 0);
  w.c.labels++; w.c.label_bytes += len;
}

// _build_MSC_segment (:522-547) on the n bytes at n_bytes of the ring, up to the hand-over: the MOT parsing from :553 on is the host's
__device__ __forceinline__ void pad_build_msc(PadWave &w, int n)
{
  const int size = min(n, w.h.dg_length);                        // :528
  if (size < 2) { w.c.dg_small++; return; }                      // :530-534
  __syncthreads();                                               // the sub-field's bytes are in the ring
  const int flag = (int)(pad_u(w.ring[(size_t)((unsigned long long)w.n_bytes & w.bytes_mask)]) >> 6) & 1;      // :539 CrcFlag
  const bool ok = pad_ring_check_crc(w, size);                   // :541
  pad_put_item(w, size, DABX_PAD_DATAGROUP, 0, flag, ok ? 1 : 0);
  w.c.groups++; w.c.group_bytes += size; w.c.dg_crc_bad += (flag && !ok) ? 1 : 0;
}

__device__ __forceinline__ void pad_ring_store(PadWave &w, int at, const uint8_t *data, int n)
{
  for (int i = w.lane; i < n; i += 64) w.ring[(size_t)((unsigned long long)(w.n_bytes + at + i) & w.bytes_mask)] = data[i];
}

// _new_MSC_element (:460-487)
__device__ __forceinline__ void pad_new_msc(PadWave &w, const uint8_t *data, int n)
{
  w.h.fill = 0;                                                  // :473
  pad_ring_store(w, 0, data, n);
  if (n >= w.h.dg_length) {                                      // :475 single item
    pad_build_msc(w, n);
    w.h.msc_group_element = 0;
    return;
  }
  w.h.msc_group_element = 1;                                     // :484-485
  w.h.fill = n;
}

// _add_MSC_element (:490-519)
__device__ __forceinline__ void pad_add_msc(PadWave &w, const uint8_t *data, int n)
{
  if (w.h.fill == 0) return;                                     // :494 no type 12 in front
  pad_ring_store(w, w.h.fill, data, n);                          // :507
  w.h.fill += n;
  if (w.h.fill >= w.h.dg_length) {                               // :512
    pad_build_msc(w, w.h.fill);
    w.h.fill = 0;
  }
}

// _dynamic_label (:335-455); data: n >= 4 bytes in LDS
__device__ __forceinline__ void pad_dynamic_label(PadWave &w, const uint8_t *data, int n, int type)
{
  if (type == 2) {                                               // :339 start of segment
    const unsigned prefix = pad_u(((unsigned)data[0] << 8) | data[1]);
    const int field_1 = (prefix >> 8) & 15, cflag = (prefix >> 12) & 1, first = (prefix >> 14) & 1, last = (prefix >> 13) & 1;
    if (first) {                                                 // :350-356
      w.h.segment_no = 1;
      w.h.charset = (prefix >> 4) & 15;
      w.h.dl_len = 0;
    } else {
      const int test = (int)((prefix >> 4) & 7) + 1;             // :359
      if (test != w.h.segment_no + 1) { w.h.segment_no = -1; return; }     // :361-366
      w.h.segment_no = test;
    }
    if (cflag) {                                                 // :371 command
      if (field_1 == 1) { w.h.dl_len = 0; w.h.segment_no = -1; } // :375-381 clear the display
      return;
    }
    const int total = field_1 + 1;                               // :394
    int len;
    if (n - 2 < total) { len = n - 2; w.h.more_xpad = 1; }       // :396-400
    else { len = total; w.h.more_xpad = 0; }                     // :401-405
    pad_text_append(w, data + 2, len);                           // :407
    if (last) {                                                  // :411
      if (!w.h.more_xpad) { pad_emit_label(w); w.h.segment_no = -1; }      // :413-419
      else w.h.is_last_segment = 1;                              // :422
    } else w.h.is_last_segment = 0;                              // :427
    w.h.remain = total - len;                                    // :430
  } else if (type == 3 && w.h.more_xpad) {                       // :433
    int len;
    if (w.h.remain > n) { len = n; w.h.remain -= n; }            // :435-439
    else { len = w.h.remain; w.h.more_xpad = 0; }                // :440-444
    pad_text_append(w, data, len);                               // :446
    if (!w.h.more_xpad && w.h.is_last_segment) pad_emit_label(w);          // :449-453
  }
}

// _handle_short_PAD (:111-200); xp[k] = iBuffer[iLast - k], iLast >= 3 (G2, checked by the caller)
__device__ __forceinline__ void pad_short(PadWave &w, const uint8_t *xp, bool ci_flag)
{
  if (ci_flag) {                                                 // :115
    const unsigned x0 = pad_u(xp[0]), x1 = pad_u(xp[1]), x2 = pad_u(xp[2]);
    w.h.first_segment = (x1 & 0x40) ? 1 : 0;                     // :120-122
    w.h.last_segment = (x1 & 0x20) ? 1 : 0;
    w.h.charset = x2 & 0x0F;
    if (w.h.first_segment) w.h.dl_len = 0;                       // :124-128
    switch (x0 & 0x1F) {
    case 2:                                                      // :137 start of fragment
      if (w.h.first_segment && !w.h.last_segment) {
        w.h.segment_number = x2 >> 4;                            // :140
        if (w.h.dl_len > 0) pad_emit_label(w);                   // :141-145
        w.h.dl_len = 0;                                          // :146
      }
      w.h.still_to_go = x1 & 0x0F;                               // :149
      if (w.lane == 0) w.shortd[0] = xp[3];                      // :150-151
      w.h.short_n = 1;
      __syncthreads();
      break;
    case 3:                                                      // :154 continuation of fragment
      for (int i = 0; i < 3 && w.h.still_to_go > 0; i++) {       // :155-159
        w.h.still_to_go--;
        if (w.lane == 0 && w.h.short_n < 16) w.shortd[w.h.short_n] = xp[1 + i];
        w.h.short_n++;
      }
      __syncthreads();
      if (w.h.still_to_go <= 0 && w.h.short_n > 1) {             // :161-166
        pad_text_append(w, w.shortd, w.h.short_n);
        w.h.short_n = 0;
      }
      break;
    default: break;                                              // :132-135
    }
  } else {                                                       // :170 the X-PAD field is all data
    for (int i = 0; i < 4 && w.h.still_to_go > 0; i++) {         // :173-177
      if (w.lane == 0 && w.h.short_n < 16) w.shortd[w.h.short_n] = xp[i];
      w.h.short_n++;
      w.h.still_to_go--;
    }
    __syncthreads();
    if (w.h.still_to_go <= 0 && w.h.short_n > 0) {               // :180
      pad_text_append(w, w.shortd, w.h.short_n);                 // :183
      w.h.short_n = 0;
      if (!w.h.first_segment && w.h.last_segment) {              // :188
        if (w.h.dl_len > 0) pad_emit_label(w);                   // :190-194
        w.h.dl_len = 0;                                          // :195
      }
    }
  }
}

// _handle_variable_PAD (:208-330); xp[k] = iBuffer[iLast - k] for k = 0 .. last (last = -1: no X-PAD byte)
__device__ __forceinline__ void pad_variable(PadWave &w, const uint8_t *xp, int last, bool ci_flag)
{
  if (!ci_flag) {                                                // :215
    const int n = w.h.xpad_length;
    if (n > 0) {                                                 // :217
      if (last < n - 1) return;                                  // :219-222
      switch (w.h.last_app_type) {                               // :230
      case 2: case 3: pad_dynamic_label(w, xp, n, 3); break;     // :232-235
      case 12: case 13: if (w.h.msc_group_element) pad_add_msc(w, xp, n); break;   // :237-241
      default: break;
      }
    }
    return;                                                      // :245
  }
  // :251-262 the contents indicators; G3: a list that would be read below index 0 is skipped before any state is touched
  int num_ci = 0, at = 0;                                        // at = iLast - base
  unsigned ci = 0;                                               // CI_table, a byte each
  do {
    if (at > last) { w.c.pad_bad++; return; }
    const unsigned v = pad_u(xp[at++]);                          // :256
    ci |= v << (8 * num_ci);
    if ((v & 0x1F) == 0) break;                                  // :259
    num_ci++;
  } while (num_ci < 4);
  int total = 0;
  for (int i = 0; i < num_ci; i++) total += pad_ci_length((ci >> (8 * i)) & 0xFFu);
  w.h.xpad_length = total + (num_ci == 4 ? 4 : num_ci + 1);      // :268-273: the CI bytes and the end marker count too
  for (int k = 0; k < num_ci; k++) {                             // :277
    const int type = (int)((ci >> (8 * k)) & 0x1Fu), n = pad_ci_length((ci >> (8 * k)) & 0xFFu);
    if (at + n - 1 > last) { w.c.pad_bad++; return; }            // G3: the sub-field would reach below index 0 (:284-287)
    const uint8_t *data = xp + at;
    switch (type) {                                              // :289
    case 1: {                                                    // :291-300 data-group length indicator
      bool ok = n == 4;
      if (ok) {
        const unsigned d0 = pad_u(data[0]), d1 = pad_u(data[1]), d2 = pad_u(data[2]), d3 = pad_u(data[3]);
        const unsigned c = pad_crc_step(pad_crc_step(0xFFFFu, d0, w.s_crc), d1, w.s_crc);
        ok = pad_u((~c) & 0xFFFFu) == ((d2 << 8) | d3);          // check_crc_bytes(data, 2)
        if (ok) w.h.dg_length = (int)(((d0 & 0x3F) << 8) | d1);  // :294
      }
      if (!ok) w.c.li_bad++;
      break;
    }
    case 2: case 3: pad_dynamic_label(w, data, n, type); break;  // :302-306
    case 12: pad_new_msc(w, data, n); break;                     // :308-311
    case 13: pad_add_msc(w, data, n); break;                     // :313-316
    default: return;                                             // :318
    }
    w.h.last_app_type = type;                                    // :321
    at += n;                                                     // :322 (base < -1, :324, cannot happen behind G3)
  }
}

// process_PAD (:67-97) behind mp4processor.cpp:347-352; rb[k] = buffer[count - 1 - k]: rb[0] = L0, rb[1] = L1, rb + 2 = the X-PAD
// reversed, iLast = count - 3.  count >= 2 (G1, checked by the caller).
__device__ __forceinline__ void pad_process(PadWave &w, const uint8_t *rb, int count)
{
  const unsigned l0 = pad_u(rb[0]), l1 = pad_u(rb[1]);
  const int last = count - 3;
  if (((l1 >> 6) & 3) != 0) { w.c.fpad_other++; return; }        // :69-75 F-PAD type
  const bool ci_flag = (l0 & 2) != 0;                            // :78
  switch ((l1 >> 4) & 3) {                                       // :77, :81
  case 1:                                                        // :87-90
    w.c.xpad_short++;
    if (last < 3) { w.c.pad_bad++; return; }                     // G2
    pad_short(w, rb + 2, ci_flag);
    break;
  case 2:                                                        // :92-95
    w.c.xpad_variable++;
    pad_variable(w, rb + 2, last, ci_flag);
    break;
  default: w.c.xpad_other++; break;                              // :83-85
  }
}
// ---- the front of k_pad_mp2's walk: Mp2Processor::add_to_frame (mp2processor.cpp:678-747) without a bit-serial loop ----------------------
// The logical frame is staged in LDS as bytes; bit i of the frame (iBits[i]) is bit 7 - (i & 7) of byte i >> 3, so a 32-bit word read
// big-endian holds bits 32 w .. 32 w + 31 from its top bit down.
__device__ __forceinline__ unsigned mp2_word_be(const uint8_t *frm, int w) { return __builtin_bswap32(reinterpret_cast<const uint32_t *>(frm)[w]); }

// :715-733 for the bits [pos, nbits) at once: the first bit index at which MP2headerCount reaches 12, given the `run` ones counted in front
// of pos (run < 12); -1: none, and *run_out = the count behind the last bit.  Lane l of pass k tests word pos / 32 + 64 k + l together with
// the word in front of it (a run of 12 may end in the first bits of a word); bits in front of pos are replaced by `run` ones behind a zero.
// The first hit of a pass comes from a ballot, so a sync word within 2048 bits of pos -- bit 0 in steady state -- costs one pass.
__device__ __forceinline__ int mp2_find_sync(const uint8_t *frm, int nbits, int pos, int run, int lane, int *run_out)
{
  const int n_words = nbits >> 5;                                // 24 kbps bits: a multiple of 32 for every multiple of 8 kbit/s
  for (int w0 = pos >> 5; w0 < n_words; w0 += 64) {
    const int w = w0 + lane;
    unsigned long long v = 0;
    if (w < n_words) v = ((unsigned long long)(w > 0 ? mp2_word_be(frm, w - 1) : 0u) << 32) | mp2_word_be(frm, w);
    const int first = 32 * (w - 1);                              // the frame's bit index of v's top bit
    if (first < pos) {                                           // the top pos - first bits of v (1 .. 63, w >= pos / 32) lie in front of pos
      const int cut = pos - first;
      v = (v & (~0ull >> cut)) | (((1ull << run) - 1ull) << (64 - cut));     // (ones beyond the top bit fall away)
    }
    unsigned long long m = v & (v >> 1);                         // bit q: v[q .. q + 1] are ones
    m &= m >> 2;                                                 // ... v[q .. q + 3]
    const unsigned long long m8 = m & (m >> 4);                  // ... v[q .. q + 7]
    const unsigned hit = (unsigned)(m8 & (m >> 8));              // ... v[q .. q + 11], for the bits of word w: a run of 12 ends there
    const unsigned long long who = __ballot(hit != 0u);
    if (who) {
      const int l = __ffsll((long long)who) - 1;
      const unsigned h = pad_u(__shfl(hit, l));
      return 32 * (w0 + l) + __clz(h);
    }
  }
  // no sync word: the run of ones at the end of the frame (at most 11, or the search would have ended), counted from pos on
  int r = 0;
  for (int i = nbits - 1; i >= pos && r < 12; i--) {             // wave-uniform, at most 12 steps
    if (!((pad_u(frm[i >> 3]) >> (7 - (i & 7))) & 1u)) { *run_out = r; return -1; }
    r++;
  }
  *run_out = r + run;                                            // every bit from pos on is a one (fewer than 12 - run of them)
  return -1;
}

// the n <= 12 bits from bit `pos` on, first bit on top (:737)
__device__ __forceinline__ unsigned mp2_bits(const uint8_t *frm, int nbytes, int pos, int n)
{
  const int b = pos >> 3;
  const unsigned v = (pad_u(frm[b]) << 16) | (b + 1 < nbytes ? pad_u(frm[b + 1]) << 8 : 0u) | (b + 2 < nbytes ? pad_u(frm[b + 2]) : 0u);
  return (v >> (24 - (pos & 7) - n)) & ((1u << n) - 1u);
}

// :740: _set_sample_rate(_get_mp2_sample_rate(MP2frame)) on MP2frame[0 .. 2] = 0xFF, 0xF0 | header >> 8, header & 0xFF
__device__ __forceinline__ void mp2_header(Mp2State &m)
{
  const int b1 = 0xF0 | (m.header >> 8), b2 = m.header & 0xFF;
  const bool refused = (b1 & 0xF6) != 0xF4 || (b2 - 0x10) >= 0xE0;         // :277-282 (in int: only bit-rate index 15 is "invalid", index 0 passes)
  const int at = (((b1 & 0x08) >> 1) ^ 4) + ((b2 >> 2) & 3);     // :283-284 sample_rates = 44100, 48000, 32000, 0, 22050, 24000, 16000, 0
  const int rate = refused ? 0 : at == 1 ? 48000 : at == 5 ? 24000 : 1;    // (1: any of the rates _set_sample_rate refuses, :257-261, 0 included)
  m.hdr_refused += refused ? 1 : 0;                              // (sums, not branches: the counters stay in registers)
  m.rate_unsupported += rate == 1 ? 1 : 0;                       // a refused header's 0 ends at :257-261 too: sampleRate stays
  if (rate == 48000 || rate == 24000) m.sample_rate = rate;      // :252-263
}
#endif

}  // namespace dabx
