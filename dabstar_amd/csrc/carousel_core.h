// carousel_core.h -- MOT objects of a packet-mode carousel: the per-slot state, the argument of k_carousel (msc_stages.hip) and its device
// helpers.  MotHandler::add_MSC_data_group with its 15-entry cache (base/backend/data/mot/mot_handler.cpp:69-259, cited as mh:) and
// MotDirectory (base/backend/data/mot/mot_dir.cpp:28-156, cited as md:) around the MotObject restatement of mot_core.h, which is used as it
// is: an object of the carousel is an arena, a name room and a segment table of its own (a "store"), MotWave is pointed at the store the
// group belongs to, and the byte source is the packet slot's data-group byte ring -- or, for a directory element's header, the directory
// buffer.  k_carousel walks the dabx_datagroup_info records k_packet has completed (packet_core.h) -- it reads what k_packet emits and changes
// nothing of it -- and every `emit signal_new_mot_object` becomes one dabx_mot_object record plus its bytes in the slot's own output rings.
// include/dabx.h "MOT objects of a packet-mode carousel" states the semantics, the quirks that are kept and the guards C1..C3, D1..D4.
#pragma once
#include "mot_core.h"
#include "packet_core.h"

namespace dabx {

constexpr int CAR_CACHE = 15;                          // mMotTable (mot_handler.h:60)
constexpr int CAR_DIR_SEGMENTS = 512;                  // marked[512] (mot_dir.h:56)
constexpr int CAR_DIR_CORE = 13;                       // what segment 0 must hold: the fields of mh:188-189 and the bytes 11, 12 md:127 reads
constexpr uint32_t CAR_DIR_OBJECTS_DEFAULT = 49, CAR_DIR_OBJECTS_MAX = 1009;                             // dabx_carousel_config.max_dir_objects
constexpr uint32_t CAR_DIR_BYTES_DEFAULT = 65536, CAR_DIR_BYTES_MIN = 256, CAR_DIR_BYTES_MAX = 1u << 20; // ... and max_dir_bytes
constexpr uint32_t CAR_COMP_USED = 0x10000u;           // a component in use: CAR_COMP_USED | transportId; 0: not in use (md:49)

struct CarEntry { int32_t order, tid; };               // SMotTable (mot_handler.h:50-55): orderNumber -1 = free; motSlide is store number `index`
// MotHandler's and MotDirectory's own members (mot_handler.h:57-60, mot_dir.h:52-66)
struct CarState {
  int32_t order_next;             // mOrderNumber
  int32_t dir_on;                 // mpDirectory != nullptr
  int32_t dir_tid, dir_size, dir_objects, dir_seg_size, dir_num_segments;      // transportId, dirSize (the i32 of the constructor), numObjects, dir_segmentSize, num_dirSegments
  int32_t reserved;
};
struct CarCounters {              // dabx_carousel_stats beyond MotCounters; one per decision of include/dabx.h
  long long groups, hdr_known, hdr_not_first, from_body, evictions, dirs_begun, dirs_repeated, dirs_refused, dir_segments, dir_objects;
  long long dir_short, dir_seg_bad, dir_cut, dg_overrun;
};

// One carousel-enabled packet-mode slot.  The job table of k_carousel is an array of these in HBM.  Everything from `stores` on lies behind
// the byte ring in the ring's allocation (out.bytes), so the slot's memory is freed with its rings.
struct CarouselSlot {
  OutRing<dabx_mot_object> out;
  int32_t s, j;                   // stream, slot
  int32_t pkt_index;              // the slot's place in the packet job table (PacketDev::slots); follows every upload of that table
  uint32_t max_object_bytes;      // guard C3
  uint32_t max_dir_objects, max_dir_bytes;      // guard D2
  long long groups_seen;          // data groups (PacketSlot::out.count) walked so far
  CarState d;
  CarEntry cache[16];             // [CAR_CACHE] (+ one unused)
  MotCounters c;
  CarCounters x;
  uint8_t *stores;                // [CAR_CACHE + max_dir_objects] of store_bytes each: arena, name, table (mot_extra_bytes); the cache's first
  unsigned long long store_bytes;
  MotState *obj;                  // [CAR_CACHE + max_dir_objects] the MotObject members of every store
  uint8_t *dir;                   // [max_dir_bytes, rounded up to 8] dir_segments
  uint32_t *marked;               // [CAR_DIR_SEGMENTS / 32] marked, one bit each
  uint32_t *comp;                 // [max_dir_objects] motComponents
};
constexpr size_t car_align8(size_t v) { return (v + 7) & ~(size_t)7; }
// the bytes behind the byte ring, in this order: stores, dir, marked, comp, obj
constexpr size_t car_extra_bytes(uint32_t max_object_bytes, uint32_t max_dir_objects, uint32_t max_dir_bytes)
{
  return (size_t)(CAR_CACHE + max_dir_objects) * (mot_extra_bytes(max_object_bytes) + sizeof(MotState)) + car_align8(max_dir_bytes) + CAR_DIR_SEGMENTS / 8 +
         car_align8(4 * (size_t)max_dir_objects);
}
static_assert(sizeof(MotState) % 8 == 0 && mot_extra_bytes(MOT_OBJECT_BYTES_MIN) % 8 == 0, "carousel_core.h: the parts are 8-byte aligned");

// k_carousel's argument, by value: the job table and the packet job table of the launch in front (launch_carousel_stage fills that in)
struct CarouselDev {
  CarouselSlot *slots;
  int32_t n;                      // carousel slots = blocks of one wave
  int32_t max_subch;
  const PacketSlot *pkt_slots;
  int32_t n_pkt, reserved;
};

#ifdef __HIPCC__
// What one wave carries through the groups of a launch beside the MotWave of mot_core.h.  Wave-uniform like that: the lanes differ inside the
// look-ups, the copies and the ballots only.
struct CarWave {
  MotWave w;                      // w.h: the members of the store that is open; w.c: the slot's MotCounters
  CarState d;
  CarCounters x;
  CarouselSlot *cs;
  const uint8_t *pkt_ring;        // the packet slot's byte ring
  unsigned long long pkt_mask;
  int open;                       // the store w points at
};

// a store's MotObject is taken up / put back.  The barrier: what lane 0 stored is in memory before any lane loads it again.
__device__ __forceinline__ void car_open(CarWave &cw, int idx)
{
  MotWave &w = cw.w;
  uint8_t *st = cw.cs->stores + (size_t)idx * cw.cs->store_bytes;
  w.arena = st;
  w.name = st + car_align8(w.max_object_bytes);
  w.table = reinterpret_cast<MotSeg *>(w.name + MOT_NAME_ROOM);
  w.h = cw.cs->obj[idx];
  w.au = idx >= CAR_CACHE ? 1 : 0;                               // dabx_mot_object flags, bit 0: mIsDirElement (md:141)
  cw.open = idx;
}
__device__ __forceinline__ void car_close(CarWave &cw)
{
  if (cw.w.lane == 0) cw.cs->obj[cw.open] = cw.w.h;
  __syncthreads();
}

// MotHandler::getHandle (mh:211-227): the cache first -- 15 entries, one compare and a ballot --, then MotDirectory::getHandle (md:68-76) in
// passes of 64 components.  The store's number, -1: no handle.
__device__ __forceinline__ int car_get_handle(const CarWave &cw, int tid)
{
  const int lane = cw.w.lane;
  CarEntry q{-1, 0};
  if (lane < CAR_CACHE) q = cw.cs->cache[lane];
  const unsigned long long hit = __ballot(q.order >= 0 && q.tid == tid);      // mh:216
  if (hit) return __ffsll((long long)hit) - 1;
  if (!cw.d.dir_on) return -1;                                   // mh:222
  const unsigned want = CAR_COMP_USED | (unsigned)tid;
  for (int base = 0; base < cw.d.dir_objects; base += 64) {      // md:70-73
    const int i = base + lane;
    const unsigned long long m = __ballot(i < cw.d.dir_objects && cw.cs->comp[i] == want);
    if (m) return CAR_CACHE + base + __ffsll((long long)m) - 1;
  }
  return -1;
}

// MotHandler::setHandle (mh:229-259): the first free entry, else the one with the lowest order number is evicted.  The object that was there
// is gone: its store keeps its bytes until the constructor's set_header resets it (transport id -1 differs from every id, mo:75-79).
__device__ __forceinline__ int car_set_handle(CarWave &cw, int tid)
{
  const int lane = cw.w.lane;
  CarEntry q{0, 0};
  if (lane < CAR_CACHE) q = cw.cs->cache[lane];
  const unsigned long long free_m = __ballot(lane < CAR_CACHE && q.order == -1);      // mh:231-240
  int index;
  if (free_m) {
    index = __ffsll((long long)free_m) - 1;
  } else {                                                       // mh:243-253
    int oldest = cw.d.order_next;
    index = 0;
    for (int i = 0; i < CAR_CACHE; i++) {
      const int o = (int)pad_u((unsigned)__shfl(q.order, i));
      if (o < oldest) { oldest = o; index = i; }
    }
    cw.x.evictions++;                                            // mh:255
  }
  __syncthreads();
  if (lane == 0) cw.cs->cache[index] = CarEntry{cw.d.order_next, tid};       // mh:235-237, :256-258
  cw.d.order_next++;
  __syncthreads();
  return index;
}

// `new MotObject(..., transportId, segment, segmentSize, lastFlag)` (mot_object.cpp:45-57) in store idx: a fresh object's mTransportId is -1,
// so set_header resets first
__device__ __forceinline__ void car_new_object(CarWave &cw, int idx, long long pos, int seg, int segsize, int tid)
{
  car_open(cw, idx);
  cw.w.h.transport_id = -1;
  mot_set_header(cw.w, pos, seg, segsize, tid);
}

// byte k of the directory buffer, wave-uniform
__device__ __forceinline__ unsigned car_d(const CarWave &cw, int k) { return pad_u(cw.cs->dir[k]); }

// analyse_theDirectory (md:124-152).  Guard D4: a read at or beyond dirSize ends the walk.
__device__ __forceinline__ void car_analyse(CarWave &cw)
{
  const int lane = cw.w.lane, size = cw.d.dir_size;
  __syncthreads();                                               // the directory's bytes are in memory
  if (CAR_DIR_CORE > size) { cw.x.dir_cut++; return; }           // D4: the extension length (md:127)
  int base = 11;                                                 // md:125
  base += 2 + (int)((car_d(cw, base) << 8) | car_d(cw, base + 1));             // md:127-130
  for (int i = 0; i < cw.d.dir_objects; i++) {                   // md:132
    if (base + 2 > size) { cw.x.dir_cut++; break; }              // D4: the entry's id
    const int tid = (int)((car_d(cw, base) << 8) | car_d(cw, base + 1));      // md:133
    if (tid == 0) break;                                         // md:135
    if (base + 2 + 7 > size) { cw.x.dir_cut++; break; }          // D4: the entry's header core
    int c = -1;                                                  // setHandle (md:78-88): the first component that is not in use
    for (int b = 0; b < cw.d.dir_objects && c < 0; b += 64) {
      const int k = b + lane;
      const unsigned long long m = __ballot(k < cw.d.dir_objects && cw.cs->comp[k] == 0u);
      if (m) c = b + __ffsll((long long)m) - 1;
    }
    int header_size;
    if (c < 0) {
      // all components are in use: the reference builds the object, takes its headerSize and drops it (md:140-150, :81-87 finds no place).
      // Nothing of it can be seen, so only the headerSize is read (mo:85)
      header_size = (int)(((car_d(cw, base + 5) & 0x0Fu) << 9) | (car_d(cw, base + 6) << 1) | (car_d(cw, base + 7) >> 7));
    } else {
      // md:140-146: a directory element, set_header on the entry's bytes; C2: the extension walk ends at the directory's end, and at
      // MOT_NAME_ROOM bytes (headerSize has 13 bits)
      const int room = min(size - (base + 2), (int)MOT_NAME_ROOM);
      cw.w.pad_ring = cw.cs->dir; cw.w.pad_mask = ~0ull;
      car_new_object(cw, CAR_CACHE + c, 0, base + 2, room, tid);
      cw.w.pad_ring = cw.pkt_ring; cw.w.pad_mask = cw.pkt_mask;
      header_size = cw.w.h.header_size;                          // get_header_size (mo:303-311)
      car_close(cw);
      if (lane == 0) cw.cs->comp[c] = CAR_COMP_USED | (unsigned)tid;         // md:83-85
      __syncthreads();
      cw.x.dir_objects++;
    }
    base += 2 + header_size;                                     // md:149
  }
}

// `new MotDirectory` (mh:186-194, md:28-57) from segment 0: segsize >= CAR_DIR_CORE bytes at `seg` of the group (guards D1, D2 in front)
__device__ __forceinline__ void car_new_directory(CarWave &cw, long long pos, int seg, int segsize, int tid, int dir_size, int objects)
{
  const int lane = cw.w.lane;
  CarouselSlot *cs = cw.cs;
  cw.d.dir_on = 1; cw.d.dir_tid = tid; cw.d.dir_size = dir_size; cw.d.dir_objects = objects; cw.d.dir_seg_size = segsize;      // md:40-43
  cw.d.dir_num_segments = -1;                                    // md:39
  if (lane < CAR_DIR_SEGMENTS / 32) cs->marked[lane] = lane == 0 ? 1u : 0u;  // md:37-38, :53
  for (int i = lane; i < objects; i += 64) cs->comp[i] = 0u;     // md:47-51
  unsigned long long *z = reinterpret_cast<unsigned long long *>(cs->dir);
  for (int i = lane; i < (dir_size + 7) / 8; i += 64) z[i] = 0ull;           // md:46 resize: zeroes
  __syncthreads();
  const int n = min(segsize, dir_size);                          // md:52; D3: the copy is clipped to dirSize
  for (int k = lane; k < n; k += 64) cs->dir[k] = cw.pkt_ring[(size_t)((unsigned long long)(pos + seg + k) & cw.pkt_mask)];
  cw.x.dirs_begun++; cw.x.dir_segments++;
  if (segsize >= dir_size) car_analyse(cw);                      // md:54-55
}

// MotDirectory::directorySegment (md:92-119); the caller has checked the transport id (mh:198, md:100)
__device__ __forceinline__ void car_dir_segment(CarWave &cw, long long pos, int seg, int number, int segsize, bool last)
{
  const int lane = cw.w.lane;
  CarouselSlot *cs = cw.cs;
  if (number >= CAR_DIR_SEGMENTS) { cw.x.dir_seg_bad++; return; }            // D3: marked[512]
  if ((pad_u(cs->marked[number >> 5]) >> (number & 31)) & 1u) return;          // md:102-103
  const long long at = (long long)number * cw.d.dir_seg_size;   // md:107
  if (at + segsize > (long long)cw.d.dir_size) { cw.x.dir_seg_bad++; return; } // D3: the copy would pass dirSize
  if (last) cw.d.dir_num_segments = number + 1;                  // md:104-105
  __syncthreads();
  if (lane == 0) cs->marked[number >> 5] |= 1u << (number & 31); // md:106
  for (int k = lane; k < segsize; k += 64) cs->dir[at + k] = cw.pkt_ring[(size_t)((unsigned long long)(pos + seg + k) & cw.pkt_mask)];   // md:108
  cw.x.dir_segments++;
  __syncthreads();
  if (cw.d.dir_num_segments != -1) {                             // md:112-118: all 512 marks at once
    unsigned word = 0xFFFFFFFFu;
    if (lane < CAR_DIR_SEGMENTS / 32) {
      const int below = cw.d.dir_num_segments - 32 * lane;       // marks of this word that count
      const unsigned need = below >= 32 ? 0xFFFFFFFFu : below <= 0 ? 0u : (1u << below) - 1u;
      word = cs->marked[lane] | ~need;
    }
    if (__ballot(word != 0xFFFFFFFFu)) return;                   // md:114-115
    car_analyse(cw);                                             // md:117
  }
}

// byte k of the group at byte position pos of the packet slot's byte ring, wave-uniform
__device__ __forceinline__ unsigned car_g(const CarWave &cw, long long pos, int k)
{
  return pad_u(cw.pkt_ring[(size_t)((unsigned long long)(pos + k) & cw.pkt_mask)]);
}

// MotHandler::add_MSC_data_group (mh:69-209) on one dabx_datagroup_info: `length` bytes at `pos` with the verdicts k_packet recorded
__device__ __forceinline__ void car_group(CarWave &cw, long long pos, int length, bool crc_flag, bool crc_ok)
{
  MotWave &w = cw.w;
  cw.x.groups++;
  if (length <= 0) { w.c.grp_short++; return; }                  // mh:86-89 (counted with C1: both leave the state as it is)
  if (crc_flag && !crc_ok) { w.c.crc_bad++; return; }            // mh:91-94
  const unsigned b0 = car_g(cw, pos, 0);
  const int type = (int)(b0 & 0x0Fu);                            // mh:76
  int next = (b0 & 0x80u) ? 4 : 2;                               // mh:78, :96-99 (bytes)
  int number = 0;                                                // mh:80
  bool last = false;
  if (b0 & 0x20u) {                                              // mh:101-106
    if (next + 2 > length) { w.c.grp_short++; return; }          // C1
    const unsigned a = car_g(cw, pos, next);
    last = (a & 0x80u) != 0;
    number = (int)(((a & 0x7Fu) << 8) | car_g(cw, pos, next + 1));
    next += 2;
  }
  int tid = 0;
  bool tid_flag = false;
  if (b0 & 0x10u) {                                              // mh:108-118
    if (next + 1 > length) { w.c.grp_short++; return; }          // C1
    const unsigned a = car_g(cw, pos, next);
    tid_flag = (a & 0x10u) != 0;                                 // mh:110
    next += 1;                                                   // mh:112
    if (tid_flag) {
      if (next + 2 > length) { w.c.grp_short++; return; }        // C1 (the id is read whatever lengthInd says, mh:115)
      tid = (int)((car_g(cw, pos, next) << 8) | car_g(cw, pos, next + 1));
    }
    next += (int)(a & 0x0Fu);                                    // mh:117
  }
  const int payload = length - next - (crc_flag ? 2 : 0);        // mh:120
  if (!tid_flag) { w.c.no_tid++; return; }                       // mh:122-125
  if (payload < 2) { w.c.grp_short++; return; }                  // C1: motVector[0], [1] (mh:139)
  const int segsize = (int)(((car_g(cw, pos, next) & 0x1Fu) << 8) | car_g(cw, pos, next + 1));       // mh:139
  if (2 + segsize > payload) { w.c.grp_short++; return; }        // C1: the segment
  const int seg = next + 2;
  if (type == 3) {                                               // mh:142-154
    if (number != 0) { cw.x.hdr_not_first++; return; }           // mh:143
    if (car_get_handle(cw, tid) >= 0) { cw.x.hdr_known++; return; }          // mh:145-149
    if (segsize < 7) { w.c.hdr_bad++; return; }                  // C2: no header core, no handle
    const int idx = car_set_handle(cw, tid);                     // mh:152 (behind the constructor there; nothing in between looks at the cache)
    car_new_object(cw, idx, pos, seg, segsize, tid);             // mh:150-151
    car_close(cw);
  } else if (type == 4) {                                        // mh:156-170
    int idx = car_get_handle(cw, tid);                           // mh:158
    if (idx < 0) {                                               // mh:159-164: the object is made with set_header run over the BODY segment
      if (segsize < 7) { w.c.hdr_bad++; return; }                // C2
      idx = car_set_handle(cw, tid);
      car_new_object(cw, idx, pos, seg, segsize, tid);
      cw.x.from_body++;
    } else {
      car_open(cw, idx);
    }
    mot_add_body<false>(w, pos, seg, number, segsize, last, tid);               // mh:167
    car_close(cw);
  } else if (type == 6) {                                        // mh:172-204
    if (number == 0) {
      if (cw.d.dir_on && cw.d.dir_tid == tid) { cw.x.dirs_repeated++; return; }          // mh:175-181
      if (segsize < CAR_DIR_CORE) { cw.x.dir_short++; return; }  // D1
      cw.d.dir_on = 0;                                           // mh:183-184
      const int dir_size = (int)(((car_g(cw, pos, seg) & 0x3Fu) << 24) | (car_g(cw, pos, seg + 1) << 16) | (car_g(cw, pos, seg + 2) << 8) | car_g(cw, pos, seg + 3));   // mh:188
      const int objects = (int)((car_g(cw, pos, seg + 4) << 8) | car_g(cw, pos, seg + 5));           // mh:189
      if ((unsigned)dir_size > cw.cs->max_dir_bytes || (unsigned)objects > cw.cs->max_dir_objects) { cw.x.dirs_refused++; return; }      // D2
      car_new_directory(cw, pos, seg, segsize, tid, dir_size, objects);      // mh:194
    } else {
      if (!cw.d.dir_on || cw.d.dir_tid != tid) return;           // mh:198-201
      car_dir_segment(cw, pos, seg, number, segsize, last);      // mh:202
    }
  } else {
    w.c.type_other++;                                            // mh:206-207
  }
}
#endif

}  // namespace dabx
