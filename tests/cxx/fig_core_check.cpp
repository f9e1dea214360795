// fig_core_check.cpp -- dabstar_amd/csrc/fig_core.h under a plain host compiler, without HIP: the host build of the device's FIG walk over
// random bytes, thinned random bytes (short FIGs, type 0 / 1 and the known extensions frequent) and truncated FIGs -- every FIG type 0 and 1
// with every known extension, at every position of the FIB, with every length the header can claim -- under both swap rules.  Every FIB
// is handed over in a heap block of exactly its 30 data bytes, so that AddressSanitizer sees a read past the data field (the walk never
// needs the CRC bytes), and after every FIB the decoder's invariants are checked: table sizes within their caps, keys unique, sub-channels
// inside 864 CU and disjoint, counters consistent.  tests/test_fig_cases.py builds and runs it plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "fig_core.h"

using namespace dabx;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) std::printf("line %d: %s fails (FIB %lld)\n", __LINE__, #c, fib_no); } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 24);
}

static long long fib_no = 0;

static void invariants(const FigDecoder &d)
{
  const FigState &t = d.st;
  CHECK(t.cur == 0 || t.cur == 1);
  for (int k = 0; k < 2; k++) {
    const FigCfg &c = t.cfg[k];
    CHECK(c.n_sub >= 0 && c.n_sub <= FIG_MAX_SUB && c.n_comp >= 0 && c.n_comp <= FIG_MAX_COMP && c.n_pkt >= 0 && c.n_pkt <= FIG_MAX_PKT);
    for (int i = 0; i < c.n_sub; i++) {
      const int s = (int)(c.sub_span[i] & 0xFFFF), z = (int)(c.sub_span[i] >> 16);
      CHECK(c.sub_id[i] < 64 && s + z <= 864);
      for (int j = 0; j < i; j++) {
        const int s2 = (int)(c.sub_span[j] & 0xFFFF), z2 = (int)(c.sub_span[j] >> 16);
        CHECK(c.sub_id[j] != c.sub_id[i]);
        CHECK(!(s < s2 + z2 && s2 < s + z));
      }
    }
    for (int i = 0; i < c.n_comp; i++)
      for (int j = 0; j < i; j++) CHECK(!(c.comp_sid[i] == c.comp_sid[j] && (c.comp_info[i] & 15) == (c.comp_info[j] & 15)));
    for (int i = 0; i < c.n_pkt; i++)
      for (int j = 0; j < i; j++) CHECK(c.pkt_scid[i] != c.pkt_scid[j]);
  }
  CHECK(t.n_labels >= 0 && t.n_labels <= 1 + 3 * FIG_MAX_LAB && t.n_labels == t.n_kind[0] + t.n_kind[1] + t.n_kind[2] + t.n_kind[3]);
  CHECK(t.n_kind[0] <= 1 && t.n_kind[1] <= FIG_MAX_LAB && t.n_kind[2] <= FIG_MAX_LAB && t.n_kind[3] <= FIG_MAX_LAB);
  for (int i = 0; i < t.n_labels; i++) {
    const dabx_fig_label &r = d.labels[i];
    CHECK(r.charset == 0 || r.charset == 6 || r.charset == 15);
    CHECK(r.kind == (t.lab_sel[i] & 15));
    for (int j = 0; j < i; j++) CHECK(!(t.lab_id[i] == t.lab_id[j] && t.lab_sel[i] == t.lab_sel[j]));
  }
  CHECK(t.fibs == t.cnt.fibs_good + t.cnt.fibs_bad);
  CHECK(t.n_restarts == t.cnt.restarts && t.n_changes == t.cnt.swaps);
  CHECK(t.cnt.events >= t.cnt.restarts + t.cnt.swaps + t.cnt.announces + t.cnt.label_new);
  CHECK((t.cif_count == -1) == (t.fig00_fib == -1));
  if (t.cnt.events > 0) {
    const dabx_fig_event &e = d.ring[(t.cnt.events - 1) % FIG_RING];
    CHECK(e.kind >= DABX_FIG_ANNOUNCE && e.kind <= DABX_FIG_LABEL && e.fib >= 0 && e.fib <= t.fibs && e.frame == e.fib / 12);
  }
}

// one FIB through both decoders, out of a heap block of its 30 data bytes
static void feed(FigDecoder *dec, const uint8_t *data30, bool crc_ok)
{
  std::unique_ptr<uint8_t[]> block(new uint8_t[30]);
  memcpy(block.get(), data30, 30);
  for (int q = 0; q < 2; q++) {
    const FigOut o{dec[q].labels, dec[q].ring};
    fig_walk_fib(dec[q].st, block.get(), crc_ok, o, 0);
    invariants(dec[q]);
  }
  fib_no++;
}

int main()
{
  std::vector<FigDecoder> dec(2);
  for (int q = 0; q < 2; q++) { memset(&dec[q], 0, sizeof(FigDecoder)); fig_state_init(dec[q].st, q, 0); }
  uint8_t fib[30];
  // random bytes
  for (int n = 0; n < 20000; n++) {
    for (int i = 0; i < 30; i++) fib[i] = (uint8_t)rnd();
    feed(dec.data(), fib, rnd() % 16 != 0);
  }
  // thinned: a random mask per byte
  static const uint8_t masks[8] = {0xFF, 0x1F, 0x3F, 0x07, 0x03, 0x25, 0x01, 0x00};
  for (int n = 0; n < 40000; n++) {
    for (int i = 0; i < 30; i++) fib[i] = (uint8_t)rnd() & masks[rnd() % 8];
    feed(dec.data(), fib, true);
  }
  // truncated FIGs: type 0 with extensions 0..3 (both C/N, both P/D) and type 1 with every extension and charset of interest, the header at
  // every byte, every length it can claim; in front of it FIGs to step over, behind it random bytes or end markers
  for (int type = 0; type < 2; type++)
    for (int ext = 0; ext < 8; ext++)
      for (int p = 0; p < 30; p++)
        for (int len = 0; len < 32; len++)
          for (int variant = 0; variant < 4; variant++) {
            for (int i = 0; i < 30; i++) fib[i] = variant & 1 ? 0xFF : (uint8_t)rnd();
            int at = 0;
            while (at < p) { const int take = p - at < 8 ? p - at : 8; fib[at] = (uint8_t)(0x40 | (take - 1)); at += take; }    // type-2 FIGs up to p
            fib[p] = (uint8_t)(type << 5 | len);
            if (p + 1 < 30) {
              if (type == 0) fib[p + 1] = (uint8_t)((variant & 2 ? 0x80 : 0) | (rnd() & 0x20) | (ext & 3));
              else fib[p + 1] = (uint8_t)((variant & 2 ? 0x60 : (rnd() % 3 == 0 ? 0xF0 : 0x00)) | ext);
            }
            feed(dec.data(), fib, true);
          }
  // the caps: distinct keys until every table is full, and past that
  for (int n = 0; n < 400; n++) {
    memset(fib, 0xFF, 30);
    fib[0] = 0x06; fib[1] = 0x02; fib[2] = (uint8_t)(0x40 | (n >> 8)); fib[3] = (uint8_t)n; fib[4] = 0x01; fib[5] = 0xC0 | (uint8_t)(n >> 6); fib[6] = (uint8_t)(n << 2);
    fib[7] = 0x06; fib[8] = 0x03; fib[9] = (uint8_t)(n >> 4); fib[10] = (uint8_t)(n << 4); fib[11] = 60; fib[12] = (uint8_t)((n & 63) << 2); fib[13] = (uint8_t)n;
    feed(dec.data(), fib, true);
    memset(fib, 0xFF, 30);
    const int ext = n % 3 == 0 ? 1 : n % 3 == 1 ? 4 : 5, ident = ext == 1 ? 2 : ext == 4 ? 3 : 4;
    fib[0] = (uint8_t)(0x20 | (1 + ident + 18)); fib[1] = (uint8_t)ext;
    fib[2] = 0; fib[3] = (uint8_t)(n >> 8); fib[4] = (uint8_t)n; fib[5] = (uint8_t)(n >> 3);
    for (int i = 0; i < 18; i++) fib[2 + ident + i] = (uint8_t)('A' + i);
    feed(dec.data(), fib, true);
  }
  for (int q = 0; q < 2; q++) {
    const dabx_fig_stats &c = dec[q].st.cnt;
    std::printf("swap rule %d: %lld FIBs, %lld FIGs, %lld restarts, %lld swaps, %lld labels filed, guards %lld / %lld / %lld, %lld label fields cut, %lld events\n", q,
                (long long)dec[q].st.fibs, (long long)c.figs, (long long)c.restarts, (long long)c.swaps, (long long)c.label_new, (long long)c.over_components,
                (long long)c.over_packets, (long long)c.over_labels, (long long)c.label_short, (long long)c.events);
    if (!(c.restarts > 0 && c.swaps > 0 && c.label_new > 0 && c.label_short > 0 && c.fig_overrun > 0 && c.over_components > 0 && c.over_packets > 0 &&
          c.over_labels > 0)) { std::printf("an input class reached nothing\n"); failures++; }
  }
  if (failures) { std::printf("fig_core_check: %d failures\n", failures); return 1; }
  std::printf("fig_core_check ok: %lld FIBs\n", fib_no);
  return 0;
}
