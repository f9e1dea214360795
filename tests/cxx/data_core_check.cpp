// data_core_check.cpp -- dabstar_amd/csrc/data_core.h under a plain host compiler, without HIP: the host build of the device's data handlers
// (TDC, IP, Journaline) over the crafted groups of tests/data_handler_cases.py -- handed over in files, one per handler: u32 handler, u32
// only_new_revisions, u32 count, then per group u32 length, u8 crc_flag, u8 crc_ok and the bytes -- and over random groups behind plausible
// heads.  Every group is handed over in a heap block of exactly its length, so that AddressSanitizer sees a read outside the group, and
// after every group the invariants are checked: what a group emitted is no longer than the group, every item's record is whole, exactly
// one decision counter moved for a group that emitted nothing (TDC: at most one).  For every file it prints the counters, which the test
// compares with the model's.  tests/test_data_handler_cases.py builds and runs it plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "data_core.h"

using namespace dabx;

static int failures = 0;
static long long group_no = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) std::printf("line %d: %s fails (group %lld)\n", __LINE__, #c, group_no); } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 24);
}

static uint16_t crc_tab[256], xpow_tab[DATA_XPOW];

static unsigned crc16(const uint8_t *p, int n)        // bit by bit: calc_crc (crc.cpp:75-86)
{
  unsigned c = 0xFFFF;
  for (int i = 0; i < n; i++) {
    c ^= (unsigned)p[i] << 8;
    for (int k = 0; k < 8; k++) c = (c & 0x8000u) ? ((c << 1) ^ 0x1021u) & 0xFFFFu : (c << 1) & 0xFFFFu;
  }
  return ~c & 0xFFFFu;
}

struct Slot {
  static constexpr size_t N_REC = 1 << 12, N_BYTES = 1 << 16;
  std::vector<dabx_data_item> recs = std::vector<dabx_data_item>(N_REC);
  std::vector<uint8_t> ring = std::vector<uint8_t>(N_BYTES), jl = std::vector<uint8_t>(DATA_JL_TABLE, (uint8_t)DATA_JL_NONE);
  DataWave w{};
  DataCounters cnt{};
  int handler;
  Slot(int h, int only_new) : handler(h)
  {
    w.recs = recs.data(); w.ring = ring.data(); w.rec_mask = N_REC - 1; w.bytes_mask = N_BYTES - 1; w.jl = jl.data();
    w.crc = crc_tab; w.xpow = xpow_tab; w.only_new = only_new; w.c = &cnt;
  }
  static long long decisions(const DataCounters &c)
  {
    const long long *p = &c.dg_overrun;
    long long s = 0;
    for (size_t i = 0; i < sizeof(DataCounters) / 8; i++) s += p[i];
    return s - c.tdc_crc0_bad - c.tdc_crc0_short;      // (these two go with an item)
  }
  void feed(const uint8_t *g, int n, bool flag, bool ok)
  {
    std::unique_ptr<uint8_t[]> block(new uint8_t[n]);
    if (n) memcpy(block.get(), g, (size_t)n);
    const long long recs0 = w.n_recs, bytes0 = w.n_bytes, dec0 = decisions(cnt);
    data_group(w, handler, block.get(), n, flag, ok, group_no / 3, (unsigned)group_no);
    const long long emitted = w.n_recs - recs0, moved = decisions(cnt) - dec0;
    CHECK(w.n_bytes - bytes0 <= n && emitted >= 0 && moved >= 0 && moved <= 1);
    if (handler != DABX_DATA_HANDLER_TDC) CHECK(emitted + moved == 1);
    else CHECK(7 * emitted <= n && (moved == 1 || n == 0 || emitted > 0));
    long long at = bytes0;
    for (long long i = recs0; i < w.n_recs; i++) {
      const dabx_data_item &r = recs[(size_t)i & (N_REC - 1)];
      CHECK(r.byte_pos == at && r.group == (unsigned)group_no && r.reserved == 0 && r.kind >= DABX_DATA_TDC_0 && r.kind <= DABX_DATA_NML);
      CHECK((handler == DABX_DATA_HANDLER_TDC) == (r.kind <= DABX_DATA_TDC_1) && (handler == DABX_DATA_HANDLER_IP) == (r.kind == DABX_DATA_UDP));
      if (r.kind == DABX_DATA_TDC_0 && r.length >= 2 && r.length <= 4096) {      // the folded CRC against the bit-serial one
        uint8_t tmp[4096];
        for (int k = 0; k < r.length; k++) tmp[k] = ring[(size_t)(at + k) & (N_BYTES - 1)];
        CHECK(((r.flags & DABX_DATA_CRC_OK) != 0) == (crc16(tmp, r.length - 2) == (unsigned)(tmp[r.length - 2] << 8 | tmp[r.length - 1])));
      }
      at += r.length;
    }
    CHECK(at == w.n_bytes);
    group_no++;
  }
  void report(const char *what) const
  {
    dabx_data_stats st;
    data_present(w, handler, &st);
    std::printf("%s handler %d:", what, handler);
    const int64_t *p = &st.groups;
    for (int i = 0; i < 29; i++) std::printf(" %lld", (long long)p[i]);
    std::printf("\n");
  }
};

static bool run_file(const char *path)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); return false; }
  uint32_t head[3];
  if (std::fread(head, 4, 3, f) != 3 || head[0] < 1 || head[0] > 3) { std::fclose(f); return false; }
  Slot s((int)head[0], (int)head[1]);
  std::vector<uint8_t> buf;
  for (uint32_t i = 0; i < head[2]; i++) {
    uint32_t len;
    uint8_t v[2];
    if (std::fread(&len, 4, 1, f) != 1 || std::fread(v, 1, 2, f) != 2 || len > 65535) { std::fclose(f); return false; }
    buf.resize(len);
    if (len && std::fread(buf.data(), 1, len, f) != len) { std::fclose(f); return false; }
    s.feed(buf.data(), (int)len, v[0] != 0, v[1] != 0);
  }
  std::fclose(f);
  s.report("file");
  return true;
}

int main(int argc, char **argv)
{
  data_host_tables(crc_tab, xpow_tab);
  for (int i = 1; i < argc; i++)
    if (!run_file(argv[i])) { std::printf("data_core_check: bad input file %s\n", argv[i]); return 2; }
  // random groups: plain random bytes, and random bytes behind a head that lets the handler get somewhere
  for (int h = DABX_DATA_HANDLER_TDC; h <= DABX_DATA_HANDLER_JOURNALINE; h++) {
    Slot s(h, (int)(rnd() & 1));
    uint8_t g[600];
    for (int n = 0; n < 60000; n++) {
      const int len = (int)(rnd() % (n % 50 == 0 ? 600 : 80));
      for (int i = 0; i < len; i++) g[i] = (uint8_t)rnd();
      const int variant = n & 3;
      if (h == DABX_DATA_HANDLER_TDC && variant && len > 7) {
        const int at = (int)(rnd() % (unsigned)(len - 6));
        g[at] = 0xFF; g[at + 1] = 0x0F; g[at + 2] = (uint8_t)(variant == 3 ? rnd() : 0); g[at + 3] = (uint8_t)(rnd() % (unsigned)(len + 4));
        g[at + 6] = (uint8_t)(rnd() % 3);
        const int length = (int)(int16_t)(uint16_t)(g[at + 2] << 8 | g[at + 3]);
        if (variant == 1 && length >= 0 && at + 7 + length <= len) {      // a good header CRC
          uint8_t v[16];
          const int sz = length < 11 ? length : 11;
          memcpy(v, g + at, 4); v[4] = g[at + 6]; memcpy(v + 5, g + at + 7, (size_t)sz);
          const unsigned c = crc16(v, 5 + sz);
          g[at + 4] = (uint8_t)(c >> 8); g[at + 5] = (uint8_t)c;
        }
      }
      if (h == DABX_DATA_HANDLER_IP && variant && len > 4) {
        g[0] &= variant == 1 ? 0x9F : 0xFF;
        const int next = 2 + ((g[0] & 0x80) ? 2 : 0) + ((g[0] & 0x20) ? 2 : 0) + ((g[0] & 0x10) && 2 < len ? 1 + (g[len > 6 ? 6 : 2] & 15) : 0);
        if (next + 12 < len) {
          g[next] = (uint8_t)(0x40 | (rnd() % 7)); g[next + 2] = 0; g[next + 3] = (uint8_t)(rnd() % (unsigned)(len + 2)); g[next + 9] = (uint8_t)(rnd() % 4 ? 17 : 6);
          const int hw = 2 * (g[next] & 15);
          if (variant == 1 && hw >= 6 && next + 2 * hw <= len) {      // a good header checksum
            g[next + 10] = g[next + 11] = 0;
            unsigned sum = 0;
            for (int i = 0; i < hw; i++) sum += (unsigned)(g[next + 2 * i] << 8 | g[next + 2 * i + 1]);
            while (sum > 0xFFFF) sum = (sum >> 16) + (sum & 0xFFFF);
            g[next + 10] = (uint8_t)(~sum >> 8); g[next + 11] = (uint8_t)~sum;
          }
        }
      }
      if (h == DABX_DATA_HANDLER_JOURNALINE && variant && len > 0) g[0] = (uint8_t)((g[0] & (variant == 1 ? 0x90 : 0xB7)) | 0x40);
      s.feed(g, len, len > 0 && (g[0] & 0x40), (rnd() & 7) != 0);
    }
    s.report("random");
    const DataCounters &c = s.cnt;
    const bool reached = h == DABX_DATA_HANDLER_TDC ? s.w.n_recs > 0 && c.walk_end > 0 && c.tdc_cut > 0 && c.tdc_len_bad > 0 && c.tdc_hdr_crc_bad > 0 && c.tdc_type_other > 0 && c.tdc_crc0_short > 0
                       : h == DABX_DATA_HANDLER_IP ? s.w.n_recs > 0 && c.ip_dg_crc_bad > 0 && c.ip_len_bad > 0 && c.ip_not_v4 > 0 && c.ip_checksum_bad > 0 && c.ip_proto_other > 0 && c.ip_short > 0
                                                   : s.w.n_recs > 0 && c.jl_hdr_short > 0 && c.jl_segmented > 0 && c.jl_crc_bad > 0 && c.jl_type_other > 0 && c.nml_short > 0 && c.nml_type_bad > 0;
    if (!reached) { std::printf("an input class reached nothing (handler %d)\n", h); failures++; }
  }
  if (failures) { std::printf("data_core_check: %d failures\n", failures); return 1; }
  std::printf("data_core_check ok: %lld groups\n", group_no);
  return 0;
}
