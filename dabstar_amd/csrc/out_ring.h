// out_ring.h -- the output rings of a slot whose stage emits items of any length (packet_core.h: MSC data groups; pad_core.h: dynamic labels
// and X-PAD data groups): a ring of 32-byte records and a ring of bytes, both in emission order -- item i has its record at i & rec_mask and
// its bytes from byte_pos & bytes_mask on.  The item under assembly lives IN the byte ring, where the completed item will be: bytes
// [n_bytes, n_bytes + fill), so the device may have written up to asm_room bytes beyond n_bytes, and whatever that range covers in the
// ring is gone.  A reader -- dabx_read_datagroups / dabx_read_pad_items (engine_slots.cpp) and the slab gather (deliver.hip) -- therefore trusts
// item i only while its record is still in the record ring (out_ring_oldest) and its bytes are (out_ring_intact).  This is the only place
// that states the rule.
#pragma once
#include <cstddef>
#include "pipeline.h"

namespace dabx {

template <class Rec> struct OutRing {
  static_assert(sizeof(Rec) == 32 && offsetof(Rec, byte_pos) == 0 && sizeof(Rec::byte_pos) == 8, "out_ring.h: what the records share");
  uint8_t *bytes;                 // [bytes_mask + 1]
  Rec *recs;                      // [rec_mask + 1]
  uint32_t bytes_mask, rec_mask;  // ring sizes - 1 (powers of two)
  uint32_t asm_room;              // the largest span beyond n_bytes the stage writes before it moves n_bytes on (set at creation)
  // bulk delivery (deliver.hip, out_ring_gather): the slot's room in a slab (offsets 0 = the slab has no section for it) ...
  uint32_t dl_rec_cap, dl_bytes_cap;
  unsigned long long dl_rec_off, dl_bytes_off;
  long long dl_done;              // ... and the items delivered so far
  long long count, n_bytes;       // items and bytes emitted so far
};

// the oldest item whose record the record ring still holds
template <class Rec> __host__ __device__ inline long long out_ring_oldest(const OutRing<Rec> &r)
{
  const long long n = (long long)r.rec_mask + 1;
  return r.count > n ? r.count - n : 0;
}
// ... and whether the bytes of the item at byte_pos are all still there
template <class Rec> __host__ __device__ inline bool out_ring_intact(const OutRing<Rec> &r, long long byte_pos)
{
  return r.n_bytes + r.asm_room - byte_pos <= (long long)r.bytes_mask + 1;
}

#ifdef __HIPCC__
// One wave moves the items emitted since the previous chunk into the slot's room in the slab -- as many of the newest as are still intact and
// fit that room -- records with byte_pos counted from the slot's bytes in the slab.  The caller writes its table record and sets dl_done.
struct OutGather { long long first, n_bytes, done; int n; };
template <class Rec> __device__ __forceinline__ OutGather out_ring_gather(const OutRing<Rec> &r, uint8_t *slab, int lane)
{
  const long long count = r.count, n_all = r.n_bytes;
  const unsigned long long rec_mask = r.rec_mask, bytes_mask = r.bytes_mask;
  const Rec *recs = r.recs;
  const uint8_t *ring = r.bytes;
  OutGather g;
  g.done = r.dl_done;
  g.first = g.done;
  if (count - g.first > (long long)r.dl_rec_cap) g.first = count - r.dl_rec_cap;
  if (g.first < out_ring_oldest(r)) g.first = out_ring_oldest(r);
  while (g.first < count) {
    const long long pos = recs[(size_t)((unsigned long long)g.first & rec_mask)].byte_pos;
    if (out_ring_intact(r, pos) && n_all - pos <= (long long)r.dl_bytes_cap) break;
    g.first++;
  }
  g.n = (int)(count - g.first);
  const long long base = g.n ? recs[(size_t)((unsigned long long)g.first & rec_mask)].byte_pos : n_all;
  g.n_bytes = n_all - base;
  Rec *ro = reinterpret_cast<Rec *>(slab + r.dl_rec_off);
  for (int i = lane; i < g.n; i += 64) {
    Rec q = recs[(size_t)((unsigned long long)(g.first + i) & rec_mask)];
    q.byte_pos -= base;
    ro[i] = q;
  }
  uint8_t *bo = slab + r.dl_bytes_off;
  for (long long k = lane; k < g.n_bytes; k += 64) bo[k] = ring[(size_t)((unsigned long long)(base + k) & bytes_mask)];
  return g;
}
#endif

}  // namespace dabx
