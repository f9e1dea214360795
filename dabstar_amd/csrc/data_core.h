// data_core.h -- the data handlers of a packet-mode slot for the device (msc_stages.hip: k_data_handler behind k_packet, k_data_batch for
// dabx_internal_data_walk_device) and for the host (dabx_internal_data_walk_host, tests/cxx/data_core_check.cpp): what DataProcessor hands a
// completed MSC data group to beside MotHandler (base/backend/data/data_processor.cpp:53-101) --
//   tdc_dataHandler::add_MSC_data_group          base/backend/data/tdc_datahandler.cpp:52-193, cited as tdc:
//   IpDataHandler::add_MSC_data_group            base/backend/data/ip_datahandler.cpp:44-148, cited as ip:
//   JournalineDataHandler::add_MSC_data_group    base/backend/data/journaline/dabdgdec_impl.c:130-296 (dg:), journaline_datahandler.cpp:38-132
//                                                (jl:) and the head of NMLFactory::CreateNML, NML.cpp:363-385 (nml:)
// -- down to the bytes a TPEG decoder, a UDP socket or an NML parser is fed.  include/dabx.h "The data handlers of a packet-mode slot" states
// the semantics, the quirks that are kept and the guards T1..T3, I1, J1.  The handlers exist once: the code below.
//
// On the device one wave takes one group, which its kernel has staged in LDS: `g` points at the group's N bytes and nothing is read outside
// them.  Header fields are the same in all 64 lanes and come out of data_u (a readfirstlane), so every lane takes every branch together.
// The wave is used for what is parallel: the sync search tests 64 positions per pass and a ballot decides (data_find_sync), a CRC is 64
// slices whose registers are moved to the end of the message with crc_mulmod and folded (data_crc), the IP header checksum is a half-word
// per lane and a sum over the wave, and a payload is copied by the whole wave to its place in the slot's byte ring (data_emit).  For the
// host the same functions are loops (DATA_LANES = 1, lane 0).
//
// Plain C++ but for those few functions: a host compiler takes the part in front of the slot structures without HIP.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/dabx.h"

#if defined(__HIPCC__)
#define DATA_HD __host__ __device__ __forceinline__
#else
#define DATA_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#include "fec_core.h"
#include "wave_ops.h"
#include "pad_core.h"
#define DATA_LANES 64
#else
#define DATA_LANES 1
#endif

namespace dabx {

constexpr int DATA_REC_RING = 256;                     // items of a slot's record ring (and the most a chunk delivers)
constexpr int DATA_JL_TABLE = 65536;                   // Journaline: object id -> revision index last filed
constexpr int DATA_JL_NONE = 0xFF;                     // ... or this: never filed
constexpr int DATA_NML_MAX = 4096;                     // RawNewsObject_t::nml (guard J1)
constexpr int DATA_XPOW = 1024;                        // entries of the table of x^(8 m) mod P (DevTables::crc_xpow)

// One counter per decision and per guard of include/dabx.h, in the order of dabx_data_stats (its fields 4 .. 28)
struct DataCounters {
  long long dg_overrun;
  long long walk_end, tdc_cut, tdc_len_bad, tdc_hdr_crc_bad, tdc_crc0_bad, tdc_crc0_short, tdc_type_other;
  long long ip_dg_crc_bad, ip_len_bad, ip_not_v4, ip_checksum_bad, ip_proto_other, ip_short;
  long long jl_hdr_short, jl_segmented, jl_empty, jl_len_bad, jl_crc_bad, jl_no_crc, jl_type_other, nml_too_long, nml_short, nml_type_bad, nml_repeat;
};
static_assert(sizeof(DataCounters) == 25 * 8 && sizeof(dabx_data_item) == 32 && sizeof(dabx_data_stats) == 256, "record sizes of include/dabx.h");

// What a handler works with: where items go (rings of powers of two, item i at i & rec_mask, its bytes from byte_pos & bytes_mask on), the
// Journaline table, the CRC tables and the counters.  The same in every lane.
struct DataWave {
  dabx_data_item *recs;
  uint8_t *ring;
  unsigned long long rec_mask, bytes_mask;
  long long n_recs, n_bytes;      // items and bytes emitted so far
  long long groups;               // groups taken so far
  uint8_t *jl;                    // [DATA_JL_TABLE], Journaline only
  const uint16_t *crc, *xpow;     // [256] CCITT table, [DATA_XPOW] x^(8 m) mod P
  int only_new, lane;
  DataCounters *c;                // the wave's: in LDS for the launch (lane 0 counts), the slot's copy is written at the end
};

// ---- the few functions that differ between the wave and the host ---------------------------------------------------------------------------
DATA_HD int data_u(int v)                       // a value every lane holds: into a scalar
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}
DATA_HD void data_count(DataWave &w, long long DataCounters::*which)      // one decision: lane 0 keeps the counters
{
  if (w.lane == 0) (w.c->*which)++;
}
DATA_HD unsigned data_fold_xor(unsigned v)      // over the lanes
{
#if defined(__HIP_DEVICE_COMPILE__)
  return wave_xor(v);
#else
  return v;
#endif
}
DATA_HD unsigned data_fold_sum(unsigned v)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned)wave_sum_int((int)v);
#else
  return v;
#endif
}
DATA_HD unsigned data_mulmod(unsigned a, unsigned b)      // a(x) b(x) mod x^16 + x^12 + x^5 + 1
{
#if defined(__HIP_DEVICE_COMPILE__)
  return crc_mulmod(a, b);
#else
  unsigned r = 0;
  for (int i = 15; i >= 0; i--) {
    r <<= 1;
    if (r & 0x10000u) r ^= 0x11021u;
    if ((a >> i) & 1u) r ^= b;
  }
  return r;
#endif
}
// the first p >= o with p + 2 < N and bytes p, p + 1 = FF 0F (tdc:62-72), -1: none.  64 positions per pass, a ballot decides.
DATA_HD int data_find_sync(const uint8_t *g, int o, int N, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
  for (int base = o; base + 2 < N; base += 64) {
    const int p = base + lane;
    const unsigned long long m = __ballot(p + 2 < N && g[p] == 0xFF && g[p + 1] == 0x0F);
    if (m) return base + __ffsll((long long)m) - 1;
  }
  return -1;
#else
  (void)lane;
  for (int p = o; p + 2 < N; p++) if (g[p] == 0xFF && g[p + 1] == 0x0F) return p;
  return -1;
#endif
}

// ---- pieces ------------------------------------------------------------------------------------------------------------------------------------
// the two CRC tables as tables.cpp builds them for the device (host only)
inline void data_host_tables(uint16_t *crc, uint16_t *xpow)
{
  for (int i = 0; i < 256; i++) {
    unsigned c = (unsigned)i << 8;
    for (int k = 0; k < 8; k++) c = (c & 0x8000u) ? ((c << 1) ^ 0x1021u) & 0xFFFFu : (c << 1) & 0xFFFFu;
    crc[i] = (uint16_t)c;
  }
  uint16_t st = 1;
  for (int m = 0; m < DATA_XPOW; m++) { xpow[m] = st; st = (uint16_t)(crc[st >> 8] ^ (uint16_t)(st << 8)); }
}

// x^(8 m) mod P for any m >= 0: the table below DATA_XPOW, beyond it a few squarings of x^(8 * 1024) (the wave: pad_core.h's pad_xpow)
DATA_HD unsigned data_xpow(const DataWave &w, int m)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return pad_xpow(w.xpow, m);
#else
  unsigned r = w.xpow[m & (DATA_XPOW - 1)];
  unsigned sq = data_mulmod(w.xpow[DATA_XPOW - 1], w.xpow[1]);
  for (int k = m / DATA_XPOW; k; k >>= 1) {
    if (k & 1) r = data_mulmod(r, sq);
    sq = data_mulmod(sq, sq);
  }
  return r;
#endif
}

// calc_crc (crc.cpp:75-86) over the n bytes at(0) .. at(n - 1): CCITT, start 0xFFFF, complemented.  Every lane runs the table recursion over
// its own slice from register 0; the slices' registers and the start value are moved to the end of the message (a multiplication by
// x^(8 bytes behind)) and folded.
template <class At> DATA_HD unsigned data_crc(const DataWave &w, int n, At at)
{
  const int per = (n + DATA_LANES - 1) / DATA_LANES, from = w.lane * per, to = from + per < n ? from + per : n;
  unsigned c = 0;
  for (int i = from; i < to; i++) c = (w.crc[(at(i) ^ (c >> 8)) & 0xFF] ^ (c << 8)) & 0xFFFFu;
  unsigned acc = from < to ? data_mulmod(c, data_xpow(w, n - to)) : 0u;
  if (w.lane == 0) acc ^= data_mulmod(0xFFFFu, data_xpow(w, n));
  return (unsigned)data_u((int)((~data_fold_xor(acc)) & 0xFFFFu));
}

// One item: len bytes of the group from g[from] on into the byte ring, copied by the whole wave, and its record (the 32 bytes of a
// dabx_data_item as four little-endian words, from lane 0)
DATA_HD void data_emit(DataWave &w, const uint8_t *g, int from, int len, int kind, int flags, unsigned a, unsigned b, long long frame, unsigned group)
{
  for (int i = w.lane; i < len; i += DATA_LANES) w.ring[(size_t)((unsigned long long)(w.n_bytes + i) & w.bytes_mask)] = g[from + i];
  if (w.lane == 0) {
    unsigned long long *o = reinterpret_cast<unsigned long long *>(w.recs + (size_t)((unsigned long long)w.n_recs & w.rec_mask));
    o[0] = (unsigned long long)w.n_bytes; o[1] = (unsigned long long)frame;
    o[2] = (unsigned long long)(len & 0xFFFF) | ((unsigned long long)(kind & 0xFF) << 16) | ((unsigned long long)(flags & 0xFF) << 24) |
           ((unsigned long long)(a & 0xFFFFu) << 32) | ((unsigned long long)(b & 0xFFFFu) << 48);
    o[3] = (unsigned long long)group;
  }
  w.n_recs++; w.n_bytes += len;
}

// ---- TDC (TPEG), tdc:52-193 ------------------------------------------------------------------------------------------------------------------
// The whole group is searched, header and CRC included; the group's own CRC verdict is not looked at.
DATA_HD void data_tdc(DataWave &w, const uint8_t *g, int N, long long frame, unsigned group)
{
  int o = 0;
  while (o < N) {                                                // tdc:60
    o = data_find_sync(g, o, N, w.lane);                         // tdc:62-72
    if (o < 0) { data_count(w, &DataCounters::walk_end); return; }                       // tdc:73-76 (a sync word in the last two bytes is never found)
    if (o + 7 > N) { data_count(w, &DataCounters::tdc_cut); return; }                    // guard T1: length, CRC and type lie beyond the group
    const unsigned b2 = (unsigned)data_u(g[o + 2]), b3 = (unsigned)data_u(g[o + 3]);
    const int length = (int)(int16_t)(uint16_t)(b2 << 8 | b3);   // tdc:80, an i16
    if (length < 0 || length >= N - o) { data_count(w, &DataCounters::tdc_len_bad); return; }       // tdc:85-88
    if (o + 7 + length > N) { data_count(w, &DataCounters::tdc_cut); return; }           // guard T2: the check vector and the copy would pass the group's end
    const int s = length < 11 ? length : 11;                     // tdc:102
    // tdc:91-113 the vector: sync word and length, the frame type, s bytes of the frame; compared with bytes 4 and 5
    const uint8_t *h = g + o;
    const unsigned hdr = data_crc(w, 5 + s, [&](int i) { return (unsigned)h[i < 4 ? i : i + 2]; });
    if (hdr != (((unsigned)data_u(h[4]) << 8) | (unsigned)data_u(h[5]))) { data_count(w, &DataCounters::tdc_hdr_crc_bad); return; }
    const int type = data_u(h[6]);                               // tdc:84
    const uint8_t *f = h + 7;
    if (type == 0) {                                             // tdc:130-151
      int flags = 0;
      if (length < 2) data_count(w, &DataCounters::tdc_crc0_short);                      // guard T3: check_crc_bytes(buffer, length - 2) reads in front of the buffer
      else if (data_crc(w, length - 2, [&](int i) { return (unsigned)f[i]; }) == (((unsigned)data_u(f[length - 2]) << 8) | (unsigned)data_u(f[length - 1])))
        flags = DABX_DATA_CRC_OK;                                // tdc:140
      else data_count(w, &DataCounters::tdc_crc0_bad);                                   // tdc:142: reported, the frame goes out all the same
      data_emit(w, g, o + 7, length, DABX_DATA_TDC_0, flags, (unsigned)o, 0, frame, group);      // tdc:148-149
    } else if (type == 1) {                                      // tdc:153-193 (the component walk of :171-190 changes nothing: not performed)
      data_emit(w, g, o + 7, length, DABX_DATA_TDC_1, 0, (unsigned)o, 0, frame, group);          // tdc:170, :191
    } else { data_count(w, &DataCounters::tdc_type_other); return; }                     // tdc:123-126
    o += 7 + length;                                             // tdc:150, :192
  }
}

// ---- IP, ip:44-148 -----------------------------------------------------------------------------------------------------------------------------
DATA_HD void data_ip(DataWave &w, const uint8_t *g, int N, bool crc_flag, bool crc_ok, long long frame, unsigned group)
{
  if (crc_flag && !crc_ok) { data_count(w, &DataCounters::ip_dg_crc_bad); return; }      // ip:59 (the verdict of the record: the CRC is not run again)
  if (N < 1) { data_count(w, &DataCounters::ip_short); return; }                         // guard I1: the flags
  const unsigned b0 = (unsigned)data_u(g[0]);
  int next = 2;                                                  // ip:51
  if (b0 & 0x80) next += 2;                                      // ip:64-67 extension
  if (b0 & 0x20) next += 2;                                      // ip:69-74 segment (its fields are not used)
  if (b0 & 0x10) {                                               // ip:78-88 user access (the transport id is not used)
    if (next >= N) { data_count(w, &DataCounters::ip_short); return; }                   // guard I1
    next += 1 + (data_u(g[next]) & 0x0F);
  }
  if (next + 4 > N) { data_count(w, &DataCounters::ip_short); return; }                  // guard I1: the length word
  const int ip_len = data_u(g[next + 2]) << 8 | data_u(g[next + 3]);        // ip:94
  if (!(ip_len < N)) { data_count(w, &DataCounters::ip_len_bad); return; }               // ip:95
  if (ip_len < 10 || next + ip_len > N) { data_count(w, &DataCounters::ip_short); return; }         // guard I1: ipVector[0], data[9]; the copy of ip:99-102
  const uint8_t *v = g + next;
  if ((data_u(v[0]) >> 4) != 4) { data_count(w, &DataCounters::ip_not_v4); return; }     // ip:103
  const int h = data_u(v[0]) & 0x0F;                             // ip:114
  if (4 * h > ip_len) { data_count(w, &DataCounters::ip_short); return; }                // guard I1: the header's half-words
  unsigned sum = 0;                                              // ip:121-124: 2 h <= 30 half-words, one per lane
  for (int i = w.lane; i < 2 * h; i += DATA_LANES) sum += (unsigned)v[2 * i] << 8 | v[2 * i + 1];
  sum = (unsigned)data_u((int)data_fold_sum(sum));
  sum = (sum >> 16) + (sum & 0xFFFFu);                           // ip:125 folded once
  if ((~sum & 0xFFFFu) != 0) { data_count(w, &DataCounters::ip_checksum_bad); return; }  // ip:126-129
  if (data_u(v[9]) != 17) { data_count(w, &DataCounters::ip_proto_other); return; }      // ip:131-137
  const int len = ip_len - 4 * h - 8;                            // ip:134, :146
  if (len < 0) { data_count(w, &DataCounters::ip_short); return; }                       // guard I1
  const uint8_t *u = v + 4 * h;
  data_emit(w, g, next + 4 * h + 8, len, DABX_DATA_UDP, 0, (unsigned)(data_u(u[0]) << 8 | data_u(u[1])), (unsigned)(data_u(u[2]) << 8 | data_u(u[3])), frame, group);
}

// ---- Journaline, dg:130-296, jl:38-132, nml:363-385 --------------------------------------------------------------------------------------------
DATA_HD void data_journaline(DataWave &w, const uint8_t *g, int N, bool crc_ok, long long frame, unsigned group)
{
  if (N < 2) { data_count(w, &DataCounters::jl_hdr_short); return; }                     // dg:251-258 (code 2)
  const unsigned b0 = (unsigned)data_u(g[0]);
  const int ext = (b0 >> 7) & 1;
  if (ext && N < 4) { data_count(w, &DataCounters::jl_hdr_short); return; }              // dg:271-280 (code 2)
  if (b0 & 0x20) { data_count(w, &DataCounters::jl_segmented); return; }                 // dg:170-177 (code 3)
  const int hl = 2 + 2 * ext;                                    // dg:179
  int len = N - hl;                                              // dg:181
  if (len == 0) { data_count(w, &DataCounters::jl_empty); return; }                      // dg:183-190 (code 4)
  if (b0 & 0x40) {                                               // dg:192
    if (len < 2) { data_count(w, &DataCounters::jl_len_bad); return; }                   // dg:194-201 (code 5)
    len -= 2;                                                    // dg:202
    if (!crc_ok) { data_count(w, &DataCounters::jl_crc_bad); return; }                   // dg:209-216 (code 6): the verdict of the record
  } else { data_count(w, &DataCounters::jl_no_crc); return; }                            // dg:218-225 (code 7)
  if (b0 & 0x0F) { data_count(w, &DataCounters::jl_type_other); return; }                // dg:227-235
  // (the user-access flag is ignored: its field stays in the object, dg:238)
  if (len > DATA_NML_MAX) { data_count(w, &DataCounters::nml_too_long); return; }        // guard J1: jl:48 copies into nml[4096]
  if (len < 4) { data_count(w, &DataCounters::nml_short); return; }                      // nml:363-368
  const uint8_t *nml = g + hl;
  const unsigned id = (unsigned)data_u(nml[0]) << 8 | (unsigned)data_u(nml[1]), b2 = (unsigned)data_u(nml[2]);      // nml:371
  if ((b2 >> 5) == 0 || (b2 >> 5) > 4) { data_count(w, &DataCounters::nml_type_bad); return; }      // nml:374-379, jl:105-106
  int old = 0;                                                   // jl:113-125; one lane reads and files: its own store is what it loads next
  if (w.lane == 0) { old = w.jl[id]; w.jl[id] = (uint8_t)(b2 & 7); }
  old = data_u(old);
  const bool fresh = old == DATA_JL_NONE || old != (int)(b2 & 7);
  if (!fresh && w.only_new) { data_count(w, &DataCounters::nml_repeat); return; }
  data_emit(w, g, hl, len, DABX_DATA_NML, fresh ? DABX_DATA_NEW_REVISION : 0, id, b2 | ((unsigned)data_u(g[1]) << 8), frame, group);
}

// one completed MSC data group (DataProcessor's mpDataHandler->add_MSC_data_group, data_processor.cpp:208, :236) to the slot's handler
DATA_HD void data_group(DataWave &w, int handler, const uint8_t *g, int N, bool crc_flag, bool crc_ok, long long frame, unsigned group)
{
  w.groups++;
  if (handler == DABX_DATA_HANDLER_TDC) data_tdc(w, g, N, frame, group);
  else if (handler == DABX_DATA_HANDLER_IP) data_ip(w, g, N, crc_flag, crc_ok, frame, group);
  else if (handler == DABX_DATA_HANDLER_JOURNALINE) data_journaline(w, g, N, crc_ok, frame, group);
}

// dabx_data_handler_for: the switch of data_processor.cpp:53-101
inline int data_handler_for(int dscty, int app_type)
{
  switch (dscty) {
  case 5: return app_type == 0x44a ? DABX_DATA_HANDLER_JOURNALINE : app_type == 4 ? DABX_DATA_HANDLER_TDC : 0;      // :55-80 (1500 and the rest: an empty handler)
  case 44: return DABX_DATA_HANDLER_JOURNALINE;                  // :82-85
  case 59: return DABX_DATA_HANDLER_IP;                          // :87-90
  case 60: return DABX_DATA_HANDLER_MOT;                         // :92-95
  default: return 0;                                             // :97-100
  }
}

// the counters as dabx_data_stats presents them
inline void data_present(const DataWave &w, int handler, dabx_data_stats *out)
{
  memset(out, 0, sizeof(*out));
  out->groups = w.groups; out->items = w.n_recs; out->bytes = w.n_bytes;
  memcpy(&out->dg_overrun, w.c, sizeof(DataCounters));
  out->active = 1; out->handler = handler;
}

}  // namespace dabx

#ifdef __HIPCC__
#include "packet_core.h"

namespace dabx {

// One packet-mode slot with a data handler on.  The job table of k_data_handler is an array of these in HBM.  The Journaline table lies
// behind the byte ring in the ring's allocation (out.bytes), so the slot's memory is freed with its rings.
struct DataSlot {
  OutRing<dabx_data_item> out;
  int32_t s, j;                   // stream, slot
  int32_t pkt_index;              // the slot's place in the packet job table (PacketDev::slots); follows every upload of that table
  int32_t handler, only_new, reserved;
  long long groups_seen;          // data groups (PacketSlot::out.count) walked so far
  long long groups;               // ... and handed to the handler
  DataCounters c;
  uint8_t *jl;                    // [DATA_JL_TABLE] behind the byte ring; Journaline only, else null
};

// k_data_handler's argument, by value: the job table and the packet job table of the launch in front (launch_data_stage fills that in)
struct DataDev {
  DataSlot *slots;
  int32_t n;                      // slots with a handler = blocks of one wave
  int32_t max_subch;
  const PacketSlot *pkt_slots;
  int32_t n_pkt, reserved;
  const uint16_t *crc_ccitt, *crc_xpow;
};

// k_data_batch's argument (dabx_internal_data_walk_device): one wave per crafted slot, its groups' records in `groups`, their bytes in a
// ring of bytes_mask + 1 bytes that all slots share
struct DataBatchSlot {
  DataSlot st;
  const dabx_datagroup_info *groups;
  int32_t n_groups, reserved;
};
// msc_stages.hip
int launch_data_batch(DataBatchSlot *slots, int n_slots, const uint8_t *bytes, unsigned long long bytes_mask, hipStream_t st);

}  // namespace dabx
#endif
