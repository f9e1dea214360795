// rec_ring_check.cpp -- dabstar_amd/csrc/rec_ring.h under a plain host compiler, without HIP: the window function against a brute-force model
// (the record numbers passed .. total - 1 listed, the newest cap of them kept) for every total in 0..40, every passed in 0..total and a few
// beyond it, and every cap the library uses; the two invariants the delivery tests rely on; the slot address inside a real ring, so that
// the sanitized build of this program (tests/cxx/Makefile, target recring) faults on an address outside it.
#include "dabx.h"
#include "rec_ring.h"
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void check_window(long long total, long long passed, int cap)
{
  std::vector<long long> kept;
  long long listed = 0;
  for (long long k = passed; k < total; k++, listed++) {
    kept.push_back(k);
    if ((int)kept.size() > cap) kept.erase(kept.begin());
  }
  const dabx::RecWindow w = dabx::rec_window(total, passed, cap);
  CHECK(w.n == (int)kept.size() && w.gone == listed - (long long)kept.size() && w.first == (kept.empty() ? total : kept.front()),
        "total %lld passed %lld cap %d: first %lld n %d gone %lld", total, passed, cap, w.first, w.n, w.gone);
  CHECK(w.first + w.n == total, "total %lld passed %lld cap %d: first %lld + n %d", total, passed, cap, w.first, w.n);
  if (passed > total) return;
  // the reader's next look, after which it has passed `total`: no record between the two windows but the gone ones
  for (long long next = total; next <= 40; next++) {
    const dabx::RecWindow v = dabx::rec_window(next, total, cap);
    CHECK(v.first == w.first + w.n + v.gone, "total %lld then %lld, cap %d: first %lld, was %lld + %d, gone %lld", total, next, cap, v.first, w.first, w.n, v.gone);
  }
}

template <int RING, int SLOT_BYTES> static void check_slots()
{
  constexpr int S = 3;
  std::vector<uint8_t> ring((size_t)S * RING * SLOT_BYTES);
  for (size_t i = 0; i < ring.size(); i++) ring[i] = (uint8_t)(i / SLOT_BYTES);         // every byte: its slot's number in the ring
  for (int s = 0; s < S; s++)
    for (long long k = 0; k <= 40; k++) {
      const uint8_t *p = dabx::rec_slot<RING, SLOT_BYTES>(ring.data(), s, k);
      const int want = s * RING + (int)(k % RING);
      CHECK(p - ring.data() == (std::ptrdiff_t)want * SLOT_BYTES && p[0] == (uint8_t)want && p[SLOT_BYTES - 1] == (uint8_t)want,
            "ring %d slot bytes %d stream %d record %lld: offset %td", RING, SLOT_BYTES, s, k, p - ring.data());
    }
}

int main()
{
  const int caps[] = {4, 8, DABX_SPECTRUM_RING, 8,                                      // the rings: CIR, scope, spectrum, TII
                      DABX_CHUNK_FRAMES, DABX_CIR_CHUNK_RECORDS, DABX_SPECTRUM_CHUNK_RECORDS, 4};     // a chunk's share: scope, CIR, spectrum, TII
  long long cases = 0;
  for (int cap : caps)
    for (long long total = 0; total <= 40; total++)
      for (long long passed = 0; passed <= total + 3; passed++, cases++) check_window(total, passed, cap);
  check_slots<8, DABX_TII_EVENT_SLOT_BYTES>();
  check_slots<8, DABX_SCOPE_SLOT_BYTES>();
  check_slots<4, DABX_CIR_SLOT_BYTES>();
  check_slots<DABX_SPECTRUM_RING, DABX_SPECTRUM_SLOT_BYTES>();
  if (failures) { std::printf("rec_ring_check: %d failures\n", failures); return 1; }
  std::printf("rec_ring_check ok: %lld windows\n", cases);
  return 0;
}
