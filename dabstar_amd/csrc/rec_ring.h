// rec_ring.h -- the record rings of the per-stream stages that write records of one size (tii_core.h: TII events; scope_core.h: scope records;
// cir_core.h: CIR and correlation records; spectrum_core.h: spectrum records): RING slots of SLOT_BYTES per stream, record number k of
// stream s in slot k % RING, one writer per stream that counts the records it has written.  (out_ring.h serves the items of any length that the
// slot stages behind the MSC batch emit.)  A reader -- the dabx_read_* entries (engine.h, rec_ring_read) and the slab gather (deliver.hip,
// deliver_records) -- keeps the number of records it has passed and takes the newest that the ring, or its own room, still holds.  This is
// the only place that states the rule.  Plain C++: a host compiler takes it without HIP (tests/cxx/rec_ring_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define REC_HD __host__ __device__
#else
#define REC_HD
#endif

namespace dabx {

// Of the records passed .. total - 1 a reader with room for cap takes the newest n, first .. total - 1; the gone before them are lost to it.
// A reader ahead of the counter (passed > total) takes none.
struct RecWindow { long long first; int n; long long gone; };
REC_HD inline RecWindow rec_window(long long total, long long passed, int cap)
{
  const long long have = total - passed;
  const int n = have < 0 ? 0 : (int)(have < cap ? have : cap);
  return RecWindow{total - n, n, have > n ? have - n : 0};
}

// the slot of stream s's record number k
template <int RING, int SLOT_BYTES> REC_HD inline const uint8_t *rec_slot(const uint8_t *ring, int s, long long k)
{
  return ring + ((size_t)s * RING + (size_t)(k % RING)) * SLOT_BYTES;
}

}  // namespace dabx
