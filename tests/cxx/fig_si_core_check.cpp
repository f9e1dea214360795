// fig_si_core_check.cpp -- dabstar_amd/csrc/fig_si_core.h (through fig_core.h) under a plain host compiler, without HIP: the host build of the
// device's FIG walk with the service information followed, and of the service directory's join, over random bytes, thinned random bytes and
// truncated FIGs -- FIG 0 with every extension the SI walk knows (and the MCI ones, so that there are components to join), both C/N, both
// P/D, the header at every byte of the FIB, every length it can claim -- under both swap rules.  Every FIB is handed over in a heap block of
// exactly its 30 data bytes, so that AddressSanitizer sees a read past the data field, and after every FIB the invariants are checked: table
// sizes within their caps, keys unique where the walk files a key once, cluster bookkeeping consistent, counters consistent; every so often
// both directories are joined.  tests/test_fig_si_cases.py builds and runs it plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "fig_core.h"

using namespace dabx;

static int failures = 0;
static long long fib_no = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) std::printf("line %d: %s fails (FIB %lld)\n", __LINE__, #c, fib_no); } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 24);
}

struct Decoder {
  FigDecoder dec;
  FigSiState si;
};

static void invariants(const Decoder &d)
{
  const FigState &t = d.dec.st;
  const FigSiState &s = d.si;
  CHECK(s.n_lang >= 0 && s.n_lang <= SI_MAX_LANG && s.n_pty >= 0 && s.n_pty <= SI_MAX_PTY && (s.has9 == 0 || s.has9 == 1));
  CHECK(s.lto_minutes >= -31 * 30 && s.lto_minutes <= 31 * 30 && s.hour < 32 && s.minute < 64 && s.second >= -1 && s.second < 64 && s.mjd < (1 << 17));
  for (int i = 0; i < s.n_pty; i++)
    for (int j = 0; j < i; j++) CHECK((s.pty[i] & 0xFFFF) != (s.pty[j] & 0xFFFF));
  for (int k = 0; k < 2; k++) {
    const FigSiCfg &c = s.cfg[k];
    CHECK(c.n_gd >= 0 && c.n_gd <= SI_MAX_GD && c.n_ua >= 0 && c.n_ua <= SI_MAX_UA && c.n_fec >= 0 && c.n_fec <= SI_MAX_FEC);
    CHECK(c.n_cl >= 0 && c.n_cl <= SI_MAX_CL && c.n_cm >= 0 && c.n_cm <= SI_MAX_CM && (c.gained & ~255) == 0);
    for (int i = 0; i < c.n_gd; i++)
      for (int j = 0; j < i; j++) CHECK(!(c.gd_sid[i] == c.gd_sid[j] && (c.gd_info[i] & 15) == (c.gd_info[j] & 15)));
    for (int i = 0; i < c.n_fec; i++)
      for (int j = 0; j < i; j++) CHECK((c.fec[i] & 63) != (c.fec[j] & 63));
    for (int i = 0; i < c.n_ua; i++) {
      const int n = (int)(c.ua_info[i] >> 8 & 15), bits = (int)(c.ua_info[i] >> 16);
      CHECK(n <= 6 && bits % 8 == 0 && bits >= 24 && bits <= 29 * 8);
      for (int a = n; a < 6; a++) CHECK(c.ua_app[i * SI_UA_WORDS + 2 * a] == 0 && c.ua_app[i * SI_UA_WORDS + 2 * a + 1] == 0);
    }
    int members = 0;
    for (int i = 0; i < c.n_cl; i++) {
      int m = 0;
      for (int j = 0; j < c.n_cm; j++) m += (int)(c.cm[j] >> 16) == i;
      CHECK(m == (int)c.cl_n[i] && c.cl_id[i] < 256 && c.cl_flags[i] < 65536);
      for (int j = 0; j < i; j++) CHECK(c.cl_id[i] != c.cl_id[j]);
      members += m;
    }
    CHECK(members == c.n_cm);
    for (int i = 0; i < c.n_cm; i++)
      for (int j = 0; j < i; j++) CHECK(c.cm[i] != c.cm[j]);
  }
  const dabx_fig_si_stats &n = s.cnt;
  CHECK(n.si_figs <= t.cnt.fig0_other_ext);
  CHECK(n.asw_start <= n.asw_count && n.cluster_new <= n.cluster_sid_new + n.over_cluster_sids + n.asw_unknown);
  if (t.cnt.events > 0) {
    const dabx_fig_event &e = d.dec.ring[(t.cnt.events - 1) % FIG_RING];
    CHECK(e.kind >= DABX_FIG_ANNOUNCE && e.kind <= DABX_FIG_ANNOUNCE_STOP && e.fib >= 0 && e.fib <= t.fibs && e.frame == e.fib / 12);
  }
}

// both directories of a decoder, each record into a heap block of its own
static void directories(const Decoder &d)
{
  const FigState &t = d.dec.st;
  for (int k = 0; k < 2; k++) {
    const int n = t.cfg[t.cur ^ k].n_comp;
    for (int i = 0; i < n; i++) {
      std::unique_ptr<dabx_fig_service> r(new dabx_fig_service);
      fig_dir_record(t, d.si, d.dec.labels, k, i, r.get());
      CHECK(r->n_apps <= 6 && r->tmid >= 0 && r->tmid <= 3 && r->comp_idx >= 0 && r->comp_idx < 16 && (r->joined & ~255u) == 0);
      CHECK((r->label.kind == 0xFF) == !(r->joined & DABX_FIG_JOIN_LABEL));
      CHECK(!r->reference_defined || (r->joined & DABX_FIG_JOIN_SUBCH));
    }
  }
}

// one FIB through both decoders, out of a heap block of its 30 data bytes
static void feed(Decoder *dec, const uint8_t *data30, bool crc_ok)
{
  std::unique_ptr<uint8_t[]> block(new uint8_t[30]);
  memcpy(block.get(), data30, 30);
  for (int q = 0; q < 2; q++) {
    const FigOut o{dec[q].dec.labels, dec[q].dec.ring, &dec[q].si};
    fig_walk_fib(dec[q].dec.st, block.get(), crc_ok, o, 0);
    invariants(dec[q]);
    if (fib_no % 64 == 0) directories(dec[q]);
  }
  fib_no++;
}

int main()
{
  static const int exts[16] = {0, 1, 2, 3, 5, 7, 8, 9, 10, 13, 14, 17, 18, 19, 6, 21};
  std::vector<Decoder> dec(2);
  for (int q = 0; q < 2; q++) { memset(&dec[q], 0, sizeof(Decoder)); fig_state_init(dec[q].dec.st, q, 0); fig_si_state_init(dec[q].si); }
  uint8_t fib[30];
  // random bytes, the first FIG a FIG 0 of an extension the walks know in every second FIB
  for (int n = 0; n < 30000; n++) {
    for (int i = 0; i < 30; i++) fib[i] = (uint8_t)rnd();
    if (n & 1) { fib[0] &= 0x1F; fib[1] = (uint8_t)((fib[1] & 0xE0) | exts[rnd() % 16]); }
    feed(dec.data(), fib, rnd() % 16 != 0);
  }
  // thinned: a random mask per byte (few keys, so that entries are known, clusters count up and stop, swaps happen)
  static const uint8_t masks[8] = {0xFF, 0x1F, 0x3F, 0x07, 0x03, 0x25, 0x01, 0x00};
  for (int n = 0; n < 60000; n++) {
    for (int i = 0; i < 30; i++) fib[i] = (uint8_t)rnd() & masks[rnd() % 8];
    if (n % 3) { fib[0] &= 0x1F; fib[1] = (uint8_t)((fib[1] & 0xA0) | exts[rnd() % 16]); }
    feed(dec.data(), fib, true);
  }
  // truncated FIGs: FIG 0 with every extension above, the header at every byte, every length it can claim; in front of it FIGs to step
  // over, behind it random bytes or end markers
  for (int x = 0; x < 16; x++)
    for (int p = 0; p < 30; p++)
      for (int len = 0; len < 32; len++)
        for (int variant = 0; variant < 8; variant++) {
          for (int i = 0; i < 30; i++) fib[i] = variant & 1 ? 0xFF : (uint8_t)rnd();
          int at = 0;
          while (at < p) { const int take = p - at < 8 ? p - at : 8; fib[at] = (uint8_t)(0x40 | (take - 1)); at += take; }    // type-2 FIGs up to p
          fib[p] = (uint8_t)len;
          if (p + 1 < 30) fib[p + 1] = (uint8_t)((variant & 2 ? 0x80 : 0) | (variant & 4 ? 0x20 : 0) | exts[x]);
          feed(dec.data(), fib, true);
        }
  // the caps: distinct keys until every SI table is full, and past that
  for (int n = 0; n < 600; n++) {
    memset(fib, 0xFF, 30);
    fib[0] = 0x05; fib[1] = 0x08; fib[2] = (uint8_t)(0x40 | (n >> 8)); fib[3] = (uint8_t)n; fib[4] = (uint8_t)(n & 15); fib[5] = (uint8_t)(n & 63);        // 0/8
    fib[6] = 0x06; fib[7] = 0x0D; fib[8] = (uint8_t)(0x40 | (n >> 8)); fib[9] = (uint8_t)n; fib[10] = (uint8_t)((n & 15) << 4 | 1); fib[11] = 0x00; fib[12] = 0x40;     // 0/13
    fib[13] = 0x04; fib[14] = 0x05; fib[15] = (uint8_t)(0x81 + (n >> 8)); fib[16] = (uint8_t)n; fib[17] = 9;                                              // 0/5, SCId >= 256
    fib[18] = 0x05; fib[19] = 0x11; fib[20] = (uint8_t)(n >> 8); fib[21] = (uint8_t)n; fib[22] = 0; fib[23] = 3;                                          // 0/17
    fib[24] = 0x05; fib[25] = 0x12; fib[26] = (uint8_t)(n >> 8); fib[27] = (uint8_t)n; fib[28] = 0; fib[29] = 1;                                          // 0/18 cut (outside)
    feed(dec.data(), fib, true);
    memset(fib, 0xFF, 30);
    fib[0] = 0x09; fib[1] = 0x12; fib[2] = (uint8_t)(n >> 8); fib[3] = (uint8_t)n; fib[4] = 0; fib[5] = 1; fib[6] = 3; fib[7] = (uint8_t)(1 + n % 70);
    fib[8] = (uint8_t)(1 + (n + 1) % 70); fib[9] = (uint8_t)(1 + (n + 2) % 70);                                                                           // 0/18, 3 clusters
    fib[10] = 0x05; fib[11] = 0x13; fib[12] = (uint8_t)(1 + n % 70); fib[13] = 0; fib[14] = (uint8_t)((n / 70) % 7 == 6 ? 2 : 1); fib[15] = 7;                        // 0/19
    feed(dec.data(), fib, true);
  }
  for (int q = 0; q < 2; q++) {
    const dabx_fig_si_stats &c = dec[q].si.cnt;
    std::printf("swap rule %d: %lld FIBs, %lld SI FIGs, %lld outside, guards %lld / %lld / %lld / %lld / %lld, %lld starts, %lld stops, %lld fallbacks, %lld clamped\n", q,
                (long long)dec[q].dec.st.fibs, (long long)c.si_figs, (long long)c.outside, (long long)c.over_global_defs, (long long)c.over_user_apps,
                (long long)c.over_languages, (long long)c.over_ptys, (long long)c.over_cluster_sids, (long long)c.asw_start, (long long)c.asw_stop,
                (long long)c.cluster_fallback, (long long)c.user_apps_clamped);
    if (!(c.outside > 0 && c.over_global_defs > 0 && c.over_user_apps > 0 && c.over_languages > 0 && c.over_ptys > 0 && c.over_cluster_sids > 0 && c.asw_start > 0 &&
          c.asw_stop > 0 && c.cluster_fallback > 0 && c.user_apps_clamped > 0 && c.time_set > 0 && c.lto_new > 0 && dec[q].dec.st.cnt.swaps > 0 &&
          dec[q].dec.st.cnt.restarts > 0)) { std::printf("an input class reached nothing\n"); failures++; }
  }
  if (failures) { std::printf("fig_si_core_check: %d failures\n", failures); return 1; }
  std::printf("fig_si_core_check ok: %lld FIBs\n", fib_no);
  return 0;
}
