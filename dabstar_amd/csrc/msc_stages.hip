// msc_stages.hip -- the slot stages behind the MSC decoder of a batch: one wave per (stream, sub-channel) slot walks what the decoder -- or
// the stage in front -- has just produced for the slot.  launch_msc_batch (pipeline.hip) runs them on the batch's stream in this order:
//
//   k_packet       packet-mode data sub-channels: packet walk, packet CRCs, assembly of the MSC data groups (data_processor.cpp:106-254)
//   k_dabplus      super-frame sync, RS(120,110), fire code, AU CRCs (mp4processor.cpp:96-333); moves the slots' frame counters on
//   k_pad          PAD of the DAB+ access units: dynamic labels and X-PAD MSC data groups (mp4processor.cpp:345-353, pad_handler.cpp:67-547)
//   k_pad_mp2      PAD of DAB (MP2) audio frames: MP2 frame sync over the logical frames and the same PadHandler (mp2processor.cpp:611-747)
//   k_mp2_audio    MP2 audio of DAB audio slots: frame assembly and the MP2 decoder, 1152 stereo samples per MP2 frame (mp2processor.cpp:292-609, :678-763)
//   k_aac_stream   LOAS/LATM frames of the DAB+ access units that passed their CRC, one record per access unit (mp4processor.cpp:320-391, :395-445)
//   k_mot          MOT objects out of the X-PAD data groups the two PAD kernels have just emitted (pad_handler.cpp:553-622, mot_object.cpp:71-323)
//   k_carousel     MOT objects out of the MSC data groups k_packet has just completed: MotHandler and MotDirectory (mot_handler.cpp:69-259,
//                  mot_dir.cpp:28-156); launched right behind k_packet
//   k_data_handler TDC frames, UDP payloads and NML objects out of the MSC data groups k_packet has just completed: tdc_dataHandler, IpDataHandler
//                  and JournalineDataHandler (data_core.h); launched behind k_packet too, beside k_carousel
//
// Which logical frames of a slot are new in a batch is msc_new_frames (pipeline.h), for every stage and for the delivery (deliver.hip).
#include "pipeline.h"
#include "packet_core.h"
#include "pad_core.h"
#include "mot_core.h"
#include "carousel_core.h"
#include "data_core.h"
#include "mp2_core.h"
#include "aac_core.h"
#include "fec_core.h"
#include "wave_ops.h"

namespace dabx {

// ------------------------------------------------------------------------------------------------- DAB+
// One wave per (stream, sub-channel); walks the logical frames produced in this batch step.
// The 5-frame window is staged in LDS once per super frame.  RS code word j is the byte sequence
// window[j + k R], k < 120 (mp4processor.cpp:193-201) and its corrected data bytes go back to the same
// positions of mOutVec (:225-228), so the super frame is simply window[0 .. 110 R) corrected in place.
// Syndromes of all R code words x 10 roots are evaluated lane-parallel (Horner over LDS); the full
// Berlekamp-Massey / Chien / Forney decoder runs only for code words whose syndromes are not all zero.
__global__ __launch_bounds__(64, 4) void k_dabplus(EngineDev e, DevTables t)   // <= 128 VGPRs: four waves per SIMD (it took 129)
{
  const int job = blockIdx.x, lane = threadIdx.x;
  const int s = job / e.max_subch, j = job % e.max_subch;
  SubchDev &sc = e.subch[(size_t)s * e.max_subch + j];
  if (!sc.active) return;
  const BatchSnap bs = e.snap[s];
  const long long n_new = msc_new_frames(bs.msc_done, bs.cif_no, sc.start_cif).n;   // logical frames the decoder just produced for this sub-channel
  if (n_new == 0) return;
  const int R = sc.kbps / 8, nbytes = 3 * sc.kbps;         // nbytes = 24 R
  const uint8_t *ring = e.msc_out + ((size_t)s * e.max_subch + j) * MSC_SLOTS * e.msc_stride;
  long long cif_out = sc.cif_out;
  int blocks_in_buf = sc.blocks_in_buf, sf_sync = sc.sf_sync;
  long long sf_count = sc.sf_count, sf_ok = 0, sf_fail = 0, rs_corr = 0, rs_fail = 0, fc_corr = 0, au_ok = 0, au_bad = 0;
  __shared__ __attribute__((aligned(16))) uint8_t win[120 * 48 + 16];   // 5 logical frames (<= 384 kbit/s)
  __shared__ uint8_t gexp[512], glog[256];
  __shared__ uint16_t s_crc[256], s_fc[256];                // CCITT and fire-code CRC tables (serial look-up chains: keep them in LDS)
  __shared__ __attribute__((aligned(16))) uint16_t s_xpow[1024];   // x^(8 m) mod P, m <= 960: two look-ups per access unit sat behind an L2 round trip each
  __shared__ unsigned syn_or[48];                           // != 0: some syndrome of the code word is non-zero
  __shared__ __attribute__((aligned(4))) unsigned syn_w[48][3];   // the code word's ten syndromes (bytes 0..9 of the three words): the full decoder starts from them
  __shared__ uint8_t s_lam[48][12], s_deg[48], s_root[48][RS_NR];  // per dirty code word: locator (index form) + degree -> roots found by the wave-wide Chien search
  __shared__ int s_rootn[48];
  __shared__ uint8_t hdr0[12];
  __shared__ int s_flag;
  __shared__ int s_au[8];
  if (sc.dab_plus) {
    for (int i = lane; i < 512; i += 64) gexp[i] = t.gf_exp[i];
    for (int i = lane; i < 256; i += 64) { glog[i] = t.gf_log[i]; s_crc[i] = t.crc_ccitt[i]; s_fc[i] = t.fc_crctab[i]; }
    for (int i = lane; i < 128; i += 64) reinterpret_cast<uint4 *>(s_xpow)[i] = reinterpret_cast<const uint4 *>(t.crc_xpow)[i];
  }
  unsigned syn_ex[2][3];                      // (r (119 - k)) mod 255 for r = 0..9 as bytes, k = lane + 64 h: the syndrome sums' exponents
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int m = 119 - (lane + 64 * h);
    int ex = 0;
    syn_ex[h][0] = syn_ex[h][1] = syn_ex[h][2] = 0;
#pragma unroll
    for (int r = 0; r < 10; r++) {
      syn_ex[h][r >> 2] |= (unsigned)ex << (8 * (r & 3));
      ex += m;
      if (ex >= 255) ex -= 255;
    }
  }
  __syncthreads();
  for (long long n = 0; n < n_new; n++) {
    const long long newest = cif_out;        // index of the logical frame just added
    cif_out++;
    if (!sc.dab_plus) continue;
    blocks_in_buf++;                         // mp4processor.cpp:113
    if (blocks_in_buf < 5) continue;
    const long long oldest = newest - 4;
    if (sf_sync == 0) {                      // :132-142: fire code over the first 11 bytes of the oldest frame
      const uint8_t *f0 = ring + (size_t)(oldest % MSC_SLOTS) * e.msc_stride;
      const bool ok = firecode_syndrome([&](int i) { return f0[i]; }, s_fc) == 0;
      if (ok) sf_sync = 4; else { blocks_in_buf = 4; continue; }
    }
    blocks_in_buf = 0;                       // :147
    // ---- stage the window (coalesced 4-byte loads) and the GF tables
    __syncthreads();
    {                                         // the five frames' loads of a chunk in flight together (they were five memory latencies in a row)
      const uint32_t *src[5];
#pragma unroll
      for (int f = 0; f < 5; f++) src[f] = reinterpret_cast<const uint32_t *>(ring + (size_t)((oldest + f) % MSC_SLOTS) * e.msc_stride);
      for (int i = lane; i < nbytes / 4; i += 64) {
        uint32_t w[5];
#pragma unroll
        for (int f = 0; f < 5; f++) w[f] = src[f][i];
#pragma unroll
        for (int f = 0; f < 5; f++) reinterpret_cast<uint32_t *>(win + f * nbytes)[i] = w[f];
      }
    }
    if (lane < 12) hdr0[lane] = 0;
    __syncthreads();
    if (lane < 11) hdr0[lane] = win[lane];
    // ---- syndromes S_r(j) = XOR_k c_k alpha^(r (119 - k)), r < 10: the Horner recursion of reed_solomon.cpp:254-290 written
    //      as a sum, lanes over the byte index k (no 120-step dependent look-up chain); only "all ten are zero" is needed
    //      here, the full decoder below recomputes them for the code words that are not clean
    // one code word's partial sums of this lane: ten 8-bit sums packed into three words
    auto syn_partial = [&](int j, unsigned &a0, unsigned &a1, unsigned &a2) {
      a0 = a1 = a2 = 0;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int k = lane + 64 * h;
        const int b = k < 120 ? win[j + k * R] : 0;
        if (b) {
          const int lg = glog[b];
#pragma unroll
          for (int r = 0; r < 10; r++) {                      // exponents r (119 - k) mod 255: per-lane constants (syn_ex), no running sum on the look-up chain
            const unsigned v = gexp[lg + (int)((syn_ex[h][r >> 2] >> (8 * (r & 3))) & 0xFFu)];
            if (r < 4) a0 ^= v << (8 * r); else if (r < 8) a1 ^= v << (8 * (r - 4)); else a2 ^= v << (8 * (r - 8));
          }
        }
      }
    };
    int cw = 0;
    for (; cw + 1 < R; cw += 2) {                               // two code words at a time: their look-up and reduction chains interleave
      unsigned a0, a1, a2, b0, b1, b2;
      syn_partial(cw, a0, a1, a2);
      syn_partial(cw + 1, b0, b1, b2);
      a0 = wave_xor(a0); b0 = wave_xor(b0); a1 = wave_xor(a1); b1 = wave_xor(b1); a2 = wave_xor(a2); b2 = wave_xor(b2);
      if (lane == 0) {
        syn_or[cw] = a0 | a1 | a2; syn_or[cw + 1] = b0 | b1 | b2;
        syn_w[cw][0] = a0; syn_w[cw][1] = a1; syn_w[cw][2] = a2; syn_w[cw + 1][0] = b0; syn_w[cw + 1][1] = b1; syn_w[cw + 1][2] = b2;
      }
    }
    if (cw < R) {
      unsigned a0, a1, a2;
      syn_partial(cw, a0, a1, a2);
      a0 = wave_xor(a0); a1 = wave_xor(a1); a2 = wave_xor(a2);
      if (lane == 0) { syn_or[cw] = a0 | a1 | a2; syn_w[cw][0] = a0; syn_w[cw][1] = a1; syn_w[cw][2] = a2; }
    }
    __syncthreads();
    // ---- full decoder only where needed.  Berlekamp-Massey and Forney: one lane per dirty code word, from the syndromes summed above (byte r of
    //      syn_w[code word]: no second, 1200-step pass over the 120 bytes on one lane).  The Chien search over all 255 positions, the longest part
    //      (255 x deg dependent table look-ups per lane), is made by the WHOLE wave for one dirty code word after the other: 4 positions per lane, the
    //      roots collected in the order the serial loop finds them (ballot + prefix count).  At 5 dB, where most super frames have dirty code words,
    //      the kernel went 0.178 -> 0.117 (syndromes) -> see docs/history/r06.md ms per step; at 8 dB and above nothing of this runs.
    int my_ret = 0;
    const bool dirty = lane < R && syn_or[lane];
    const Gf gf{gexp, glog};
    uint8_t lam[RS_NR + 1];
    int deg_lambda = 0;
    if (__builtin_amdgcn_ballot_w64(dirty)) {                  // wave-uniform: clean super frames skip all of it
      if (dirty) {
        rs_berlekamp_massey(reinterpret_cast<const uint8_t *>(syn_w[lane]), gf, lam, deg_lambda);
#pragma unroll
        for (int i = 0; i <= RS_NR; i++) s_lam[lane][i] = lam[i];
        s_deg[lane] = (uint8_t)deg_lambda;
      }
      __syncthreads();
      unsigned long long dm = __builtin_amdgcn_ballot_w64(dirty);
      while (dm) {
        const int c = __builtin_ctzll(dm);
        dm &= dm - 1;
        const int dg = s_deg[c];
        int count = 0;
#pragma unroll
        for (int pass = 0; pass < 4; pass++) {
          const int i = 64 * pass + lane + 1;
          const bool root = i <= RS_NN && rs_chien_at(s_lam[c], dg, gexp, i) == 0;
          const unsigned long long b = __builtin_amdgcn_ballot_w64(root);
          const int idx = count + __builtin_popcountll(b & ((1ull << lane) - 1ull));
          if (root && idx < RS_NR) s_root[c][idx] = (uint8_t)i;
          count += __builtin_popcountll(b);
        }
        if (lane == 0) s_rootn[c] = count;
      }
      __syncthreads();
      if (dirty)
        my_ret = s_rootn[lane] != deg_lambda ? -1
                                             : rs_forney(CwStrided{win + lane, R}, gf, reinterpret_cast<const uint8_t *>(syn_w[lane]), lam, deg_lambda, s_root[lane], s_rootn[lane]);
    }
    int corr = my_ret > 0 ? my_ret : 0, fail = my_ret < 0 ? 1 : 0;
    corr = wave_sum_int(corr); fail = wave_sum_int(fail);
    rs_corr += corr; rs_fail += fail;
    __syncthreads();
    if (lane == 0) {
      uint8_t hdr[12];
      for (int i = 0; i < 12; i++) hdr[i] = win[i];
      const bool ok = firecode_check_and_correct(hdr, s_fc, t.fc_syndrome);   // :230-240
      int flag = ok ? 1 : 0;
      if (ok) {
        bool changed = false;
        for (int i = 0; i < 11; i++) changed = changed || (hdr[i] != hdr0[i]);
        if (changed) flag |= 2;
        for (int i = 0; i < 12; i++) win[i] = hdr[i];
        // AU table, mp4processor.cpp:256-306
        const int dac = (hdr[2] >> 6) & 1, sbr = (hdr[2] >> 5) & 1, end = 110 * R;
        int n_au;
        switch (2 * dac + sbr) {
        case 0: n_au = 4; s_au[0] = 8; s_au[1] = hdr[3] * 16 + (hdr[4] >> 4); s_au[2] = (hdr[4] & 0xf) * 256 + hdr[5];
                s_au[3] = hdr[6] * 16 + (hdr[7] >> 4); s_au[4] = end; break;
        case 1: n_au = 2; s_au[0] = 5; s_au[1] = hdr[3] * 16 + (hdr[4] >> 4); s_au[2] = end; break;
        case 2: n_au = 6; s_au[0] = 11; s_au[1] = hdr[3] * 16 + (hdr[4] >> 4); s_au[2] = (hdr[4] & 0xf) * 256 + hdr[5];
                s_au[3] = hdr[6] * 16 + (hdr[7] >> 4); s_au[4] = (hdr[7] & 0xf) * 256 + hdr[8];
                s_au[5] = hdr[9] * 16 + (hdr[10] >> 4); s_au[6] = end; break;
        default: n_au = 3; s_au[0] = 6; s_au[1] = hdr[3] * 16 + (hdr[4] >> 4); s_au[2] = (hdr[4] & 0xf) * 256 + hdr[5];
                s_au[3] = end; break;
        }
        s_au[7] = n_au;
      }
      s_flag = flag;
    }
    __syncthreads();
    const int flag = s_flag;
    if (flag & 1) {                          // :149-158
      if (flag & 2) fc_corr++;
      sf_sync = 4; sf_ok++;
      const int n_au = s_au[7];
      // :318-333 AU CRCs.  The CRC register is linear in the message: every lane runs the table recursion over its own
      // slice from state 0, the slice results are moved to the end of the AU by multiplying with x^(8 n) mod P
      // (crc_xpow, in LDS) and XOR-ed together; the 0xFFFF start value rides on the first two bytes -- calc_crc (crc.cpp:75-86)
      // without a several-hundred-step look-up chain on one lane.
      int good = 0, bad = 0;
      unsigned crc_mask = 0, len_mask = 0;     // per access unit: passed its CRC / failed the length check (dabx_superframe_info)
      for (int a = 0; a < n_au; a++) {
        const int st = s_au[a], len = s_au[a + 1] - st - 2;
        if (len > 960 || len < 0 || st + len + 2 > 110 * R) { bad++; len_mask |= 1u << a; continue; }
        const int per = (len + 63) >> 6, from = lane * per, to = min(len, from + per);
        const unsigned xp_slice = s_xpow[from < to ? len - to : 0];
        // The 0xFFFF start value of a 16-bit CRC is the same as complementing the first two message bytes and starting from 0
        // (the register only ever shifts the start value through those two steps): the lanes that own bytes 0 and 1 do that, and
        // the second crc_mulmod that lane 0 ran for the start value's contribution -- with the other 63 lanes waiting -- is gone.
        const unsigned first2 = len >= 2 ? 0xFFu : 0u;
        unsigned crc = 0;
        for (int i = from; i < to; i++) crc = (s_crc[(win[st + i] ^ (i < 2 ? first2 : 0u) ^ (crc >> 8)) & 0xFF] ^ (crc << 8)) & 0xFFFFu;
        unsigned acc = from < to ? crc_mulmod(crc, xp_slice) : 0u;
        if (len < 2 && lane == 0) acc ^= crc_mulmod(0xFFFFu, s_xpow[len]);      // a message shorter than the register: the start value's contribution as it was
        acc = wave_xor(acc);
        const unsigned want = ((unsigned)win[st + len] << 8) | win[st + len + 1];
        if (((~acc) & 0xFFFFu) == want) { good++; crc_mask |= 1u << a; } else bad++;
      }
      au_ok += good; au_bad += bad;
      if (lane == 0 && e.sf_info) {            // what _process_super_frame knows when it hands the access units on (mp4processor.cpp:256-333)
        dabx_superframe_info r;
        r.num_aus = (uint8_t)n_au; r.au_crc_ok = (uint8_t)crc_mask; r.au_len_bad = (uint8_t)len_mask; r.stream_parms = (uint8_t)(win[2] & 0x7F);
#pragma unroll
        for (int a = 0; a < 7; a++) r.au_start[a] = a <= n_au ? (uint16_t)s_au[a] : (uint16_t)0;
        r.rs_corrected = (uint16_t)corr; r.rs_failed = (uint8_t)fail; r.fc_corrected = (flag & 2) ? 1 : 0; r.reserved = 0;
        r.first_frame = oldest;
        e.sf_info[((size_t)s * e.max_subch + j) * SF_SLOTS + (size_t)(sf_count % SF_SLOTS)] = r;
      }
      uint8_t *sfo = e.sf_out + (((size_t)s * e.max_subch + j) * SF_SLOTS + (size_t)(sf_count % SF_SLOTS)) * e.sf_stride;
      for (int i = lane; i < (110 * R + 3) / 4; i += 64)
        reinterpret_cast<uint32_t *>(sfo)[i] = reinterpret_cast<const uint32_t *>(win)[i];
      sf_count++;
    } else {                                 // :159-169
      sf_sync--;
      if (sf_sync == 0) { blocks_in_buf = 4; sf_fail++; }
    }
  }
  if (lane == 0) {
    sc.cif_out = cif_out; sc.blocks_in_buf = blocks_in_buf; sc.sf_sync = sf_sync; sc.sf_count = sf_count;
    sc.sf_ok += sf_ok; sc.sf_fail += sf_fail; sc.rs_corr += rs_corr; sc.rs_fail += rs_fail;
    sc.fc_corr += fc_corr; sc.au_ok += au_ok; sc.au_bad += au_bad;
  }
}

// ------------------------------------------------------------------------------------------ packet mode
// One wave per packet-mode slot (PacketDev::slots: those slots only); walks the logical frames the decoder produced in this batch step
// (msc_new_frames, pipeline.h), in order, numbered from the slot's cif_out (it runs in front of k_dabplus, which moves cif_out on).  Per frame: the frame is
// staged in LDS; lane g reads the length code of granule g and the packet boundaries follow from two ballots (pkt_walk: scalar), and runs the
// CCITT register over its granule; the lanes at packet starts fold the packet CRC from their granules' registers and, for packets that pass
// it, the register over the payload from 0 (pkt_describe: all packets of the frame in parallel, tables in LDS); the state machine (data_processor.cpp:165-253) then runs wave-uniform over header fields only --
// the data-group CRC register is carried from packet to packet with one multiplication by x^(8 n) -- and every accepted payload is copied
// by the whole wave to its place in the slot's byte ring.  include/dabx.h states the semantics and the two guards.
__global__ __launch_bounds__(64) void k_packet(PacketDev pk)
{
  const int lane = threadIdx.x;
  PacketSlot &ps = pk.slots[blockIdx.x];
  const SubchDev &sc = pk.subch[(size_t)ps.s * pk.max_subch + ps.j];
  if (!sc.active) return;
  const BatchSnap bs = pk.snap[ps.s];
  const long long n_new = msc_new_frames(bs.msc_done, bs.cif_no, sc.start_cif).n;   // logical frames the decoder just produced for this sub-channel
  if (n_new == 0) return;
  const int nbytes = 3 * sc.kbps, n_gran = sc.kbps / 8;       // <= 1152 bytes, <= 48 granules (dabx_set_packet_mode)
  const uint8_t *ring = pk.msc_out + ((size_t)ps.s * pk.max_subch + ps.j) * MSC_SLOTS * pk.msc_stride;
  __shared__ __attribute__((aligned(16))) uint8_t frm[3 * PKT_MAX_KBPS];
  __shared__ uint16_t s_crc[256], s_xpow[128];               // CCITT table; x^(8 m) mod P for m = useful length <= 127
  __shared__ unsigned s_info[64];
  __shared__ uint16_t s_part[64];                             // the CCITT register from 0 over every granule of the frame
  for (int i = lane; i < 256; i += 64) s_crc[i] = pk.crc_ccitt[i];
  for (int i = lane; i < 128; i += 64) s_xpow[i] = pk.crc_xpow[i];
  const int address = ps.address;
  uint8_t *const dg_ring = ps.out.bytes;                         // (locals: the stores below must not make the loop reload them from the table)
  dabx_datagroup_info *const dg_recs = ps.out.recs;
  const unsigned long long bytes_mask = ps.out.bytes_mask, rec_mask = ps.out.rec_mask;
  int expected = ps.expected, state = ps.state, fill = ps.fill, first_byte = ps.first_byte;
  unsigned run_crc = ps.run_crc;
  long long first_frame = ps.first_frame, dg_count = ps.out.count, dg_bytes = ps.out.n_bytes;
  long long packets = 0, addr_match = 0, continuity_err = 0, crc_bad = 0, len_bad = 0, walk_short = 0, dg_crc_bad = 0, dg_overflow = 0;
  const long long frame0 = sc.cif_out;
  for (long long n = 0; n < n_new; n++) {
    const long long frame = frame0 + n;      // index of the logical frame in the slot's sequence
    slot_stage_frame(frm, ring, pk.msc_stride, frame, nbytes, lane);
    const unsigned code = lane < n_gran ? (unsigned)(frm[lane * PKT_GRANULE] >> 6) : 0u;
    s_part[lane] = lane < n_gran ? (uint16_t)pkt_granule_crc(frm, lane, s_crc) : (uint16_t)0;
    bool short_walk;
    const unsigned long long starts = pkt_walk(__ballot(code & 1u), __ballot(code & 2u), n_gran, &short_walk);
    __syncthreads();
    s_info[lane] = ((starts >> lane) & 1ull) ? pkt_describe(frm, lane, nbytes, address, s_crc, s_part, s_xpow) : 0u;
    __syncthreads();
    packets += __popcll(starts);
    walk_short += short_walk ? 1 : 0;
    for (unsigned long long m = starts; m; m &= m - 1) {
      const int g = __ffsll((long long)m) - 1;
      const unsigned inf = s_info[g];
      if (!(inf & 1u)) continue;                                                            // :165 another address
      addr_match++;
      if ((int)((inf >> 3) & 3u) != expected) { continuity_err++; expected = 0; continue; }   // :170-178
      expected = (expected + 1) & 3;                                                        // :181, before the CRC
      if (!(inf & 2u)) { crc_bad++; continue; }                                             // :184-187
      if (!(inf & 4u)) { len_bad++; continue; }                                             // guard: the payload would pass the end of the logical frame
      const int fl = (int)((inf >> 5) & 3u), ulen = (int)((inf >> 7) & 0x7Fu);
      bool start = false, append = false, emit = false;
      if (state == 0) {                                                                     // :191-215 waiting for a start
        if (fl == 2) { start = true; state = 1; }
        else if (fl == 3) { start = true; emit = true; }
        else fill = 0;
      } else {                                                                              // :216-253 within a series
        if (fl == 0) append = true;
        else if (fl == 1) { append = true; emit = true; }
        else if (fl == 2) start = true;
        else { state = 0; fill = 0; }
      }
      if (append && fill + ulen > DABX_DG_MAX_BYTES) { dg_overflow++; state = 0; fill = 0; continue; }   // guard: bounded assembly
      if (start) { fill = 0; run_crc = 0xFFFFu; first_frame = frame; first_byte = -1; }
      if (start || append) {
        const int from = g * PKT_GRANULE + 3;
        for (int i = lane; i < ulen; i += 64) dg_ring[(size_t)((unsigned long long)(dg_bytes + fill + i) & bytes_mask)] = frm[from + i];
        if (fill == 0 && ulen > 0) first_byte = frm[from];
        run_crc = crc_mulmod(run_crc, s_xpow[ulen]) ^ (inf >> 16);
        fill += ulen;
      }
      if (emit) {
        const bool flag = first_byte >= 0 && (first_byte & 0x40);
        const bool good = flag && fill >= 2 && run_crc == PKT_CRC_RESIDUE;
        if (lane == 0) {
          dabx_datagroup_info r;
          r.byte_pos = dg_bytes; r.first_frame = first_frame; r.last_frame = frame; r.length = (uint16_t)fill;
          r.crc_flag = flag ? 1 : 0; r.crc_ok = good ? 1 : 0; r.reserved = 0;
          dg_recs[(size_t)((unsigned long long)dg_count & rec_mask)] = r;
        }
        dg_crc_bad += (flag && !good) ? 1 : 0;
        dg_count++; dg_bytes += fill;
        fill = 0; state = 0;
      }
    }
  }
  if (lane == 0) {
    ps.expected = expected; ps.state = state; ps.fill = fill; ps.first_byte = first_byte; ps.run_crc = run_crc;
    ps.first_frame = first_frame; ps.out.count = dg_count; ps.out.n_bytes = dg_bytes;
    ps.frames += n_new; ps.packets += packets; ps.addr_match += addr_match; ps.continuity_err += continuity_err; ps.crc_bad += crc_bad;
    ps.len_bad += len_bad; ps.walk_short += walk_short; ps.dg_crc_bad += dg_crc_bad; ps.dg_overflow += dg_overflow;
  }
}

// --------------------------------------------------------------------------------------------------- PAD
// One wave per PAD-enabled DAB+ slot (PadDev::slots: those slots only), behind k_dabplus: walks the super frames k_dabplus has completed
// since the slot's last visit (SubchDev::sf_count against PadSlot::sf_seen: a batch adds at most 6, the rings hold SF_SLOTS) out of the
// super-frame ring and their dabx_superframe_info records, and of every access unit that passed its CRC the data stream element
// (mp4processor.cpp:345-353).  The PAD bytes (<= 255) are staged REVERSED in LDS, so that PadHandler's iBuffer[iLast - k] is xp[k] and a
// sub-field is a forward run of bytes; the state machine (pad_core.h: pad_handler.cpp:67-519 line by line) runs wave-uniform on header
// bytes, the whole wave copies sub-fields straight to their place in the slot's byte ring -- the group under assembly lives where the
// completed group will be -- and the data-group CRC at completion is folded from per-lane slices.  The dynamic label's text and the
// short X-PAD's bytes are in LDS for the launch.  include/dabx.h states the semantics and the guards G1..G4.
__global__ __launch_bounds__(64) void k_pad(PadDev pd)
{
  const int lane = threadIdx.x;
  PadSlot &ps = pd.slots[blockIdx.x];
  const size_t sj = (size_t)ps.s * pd.max_subch + ps.j;
  const SubchDev &sc = pd.subch[sj];
  if (!sc.active || !sc.dab_plus) return;
  const long long have = sc.sf_count;
  long long seen = ps.sf_seen;
  if (have <= seen) return;
  if (have - seen > SF_SLOTS) seen = have - SF_SLOTS;         // (cannot happen: the stage runs behind every batch)
  const int end = 110 * (sc.kbps / 8);
  __shared__ PadLds lds;                                       // lds.rb: the AU's PAD reversed, rb[k] = buffer[count - 1 - k]
  PadWave w;
  pad_wave_open(w, ps, pd, lds, lane);
  __syncthreads();
  for (long long sf = seen; sf < have; sf++) {
    const size_t slot = sj * SF_SLOTS + (size_t)(sf % SF_SLOTS);
    const dabx_superframe_info *inf = pd.sf_info + slot;
    const uint8_t *sfb = pd.sf_out + slot * pd.sf_stride;
    const int n_au = min((int)inf->num_aus, 6);
    const unsigned take = (unsigned)inf->au_crc_ok & ~(unsigned)inf->au_len_bad;
    w.frame = inf->first_frame;
    w.c.superframes++;
    for (int a = 0; a < n_au; a++) {                           // mp4processor.cpp:320
      if (!((take >> a) & 1u)) continue;                       // :325, :333
      w.c.aus++;
      const int st = inf->au_start[a];
      if (st >= end || ((sfb[st] >> 5) & 7) != 4) continue;    // :345
      w.c.pad_aus++;
      if (st + 2 > end) { w.c.pad_bad++; continue; }           // G1
      const int count = sfb[st + 1];                           // :347
      if (count < 2 || st + 2 + count > end) { w.c.pad_bad++; continue; }      // G1
      __syncthreads();                                         // the previous AU's bytes are done with
      for (int k = lane; k < count; k += 64) lds.rb[k] = sfb[st + 2 + count - 1 - k];      // :349-351
      __syncthreads();
      w.au = a;
      pad_process(w, lds.rb, count);                           // :352
    }
  }
  pad_wave_close(w, ps, lds, lane);
  if (lane == 0) ps.sf_seen = have;
}

// One wave per PAD slot whose source is the MP2 frames of a DAB audio sub-channel (PadSlot::source; the blocks of the other slots of the
// table return at once, as k_pad's do for these), behind k_dabplus, which has moved the slots' frame counters on: walks the logical frames
// the decoder produced in this batch step, the frames k_packet walks (msc_new_frames, pipeline.h) in its numbering.  Per frame: the frame
// is staged in LDS and Mp2Processor::add_to_frame (mp2processor.cpp:678-747) runs over its 24 kbps bits as a handful of wave-uniform phase
// changes -- at most one completed MP2 frame (:691: lf is at least a logical frame's bits) and two searches -- the search for the 12 ones
// being one wave-wide pass (mp2_find_sync).  When an MP2 frame completes, _process_pad_data (:611-674) takes the PAD from the end of the
// CURRENT logical frame (:695): F-PAD in the last two bytes, the X-PAD in front of the ScF-CRC, staged reversed as k_pad stages it and
// handed to the same pad_process.  Only the newest 254 X-PAD bytes are staged: PadHandler reads at most 196 below iLast.
__global__ __launch_bounds__(64) void k_pad_mp2(PadDev pd)
{
  const int lane = threadIdx.x;
  PadSlot &ps = pd.slots[blockIdx.x];
  if (ps.source != DABX_PAD_SOURCE_MP2) return;
  const size_t sj = (size_t)ps.s * pd.max_subch + ps.j;
  const SubchDev &sc = pd.subch[sj];
  if (!sc.active || sc.dab_plus) return;
  const BatchSnap bs = pd.snap[ps.s];
  const long long n_new = msc_new_frames(bs.msc_done, bs.cif_no, sc.start_cif).n;   // logical frames the decoder just produced for this sub-channel
  if (n_new == 0) return;
  const int nbytes = 3 * sc.kbps, nbits = 8 * nbytes;          // <= 1152 bytes (dabx_set_pad_mode); MP2framesize = 24 * bitRate (:236)
  const int v_len = nbytes - (sc.kbps >= 56 ? 4 : 2) - 2;       // :613-621
  const int n_stage = min(v_len, 254);
  const uint8_t *ring = pd.msc_out + sj * MSC_SLOTS * pd.msc_stride;
  __shared__ __attribute__((aligned(16))) uint8_t frm[3 * PKT_MAX_KBPS];
  __shared__ PadLds lds;                                       // lds.rb: rb[0] = L0, rb[1] = L1, rb[2 + k] = frame[vLen - 1 - k]
  PadWave w;
  pad_wave_open(w, ps, pd, lds, lane);
  Mp2State m = ps.m;
  const long long frame0 = sc.cif_out - n_new;
  for (long long n = 0; n < n_new; n++) {
    w.frame = frame0 + n;                     // index of the logical frame in the slot's sequence
    slot_stage_frame(frm, ring, pd.msc_stride, w.frame, nbytes, lane);
    w.c.superframes++;                        // (dabx_pad_stats of an MP2 source slot: logical frames walked)
    int pos = 0;                              // :685 i
    while (pos < nbits) {
      if (m.state == MP2_GET_DATA) {                             // :687-714
        const int lf = m.sample_rate == 48000 ? nbits : 2 * nbits;      // :680, :741
        const int need = lf - m.bit_count;                       // (>= 1: a frame that completes leaves the state)
        if (need > nbits - pos) { m.bit_count += nbits - pos; break; }
        pos += need;                                             // :691 the MP2 frame is complete with bit pos - 1
        m.frames++;
        w.c.aus++; w.c.pad_aus++;                                // :695 _process_pad_data(iBits): the PAD at the end of THIS logical frame
        const unsigned l1 = pad_u(frm[nbytes - 2]);              // :624
        const int count = (((l1 >> 4) & 3) == 1 ? 4 : n_stage) + 2;     // :649-657; F-PAD type and the indicators 0 and 3: pad_process (:629-645)
        __syncthreads();                                         // the previous PAD's bytes are done with
        if (lane < 2) lds.rb[lane] = frm[nbytes - 1 - lane];     // :623-624 L0, L1
        for (int k = lane; k < n_stage; k += 64) lds.rb[2 + k] = frm[v_len - 1 - k]; // :660-673 pPadData[vLengthBytes - 1 - k]
        __syncthreads();
        pad_process(w, lds.rb, count);                           // :673 process_PAD(pPadData, vLengthBytes - 1, L1, L0)
        m.state = MP2_SEARCHING; m.header_count = 0; m.bit_count = 0;   // :710-712
      } else if (m.state == MP2_SEARCHING) {                     // :715-734
        int run;
        const int p = mp2_find_sync(frm, nbits, pos, m.header_count, lane, &run);
        if (p < 0) { m.header_count = run; break; }              // :720, :732 to the end of the frame
        m.syncs++; m.last_sync_bit = p;
        m.header_count = 12; m.bit_count = 12; m.header = 0;     // :720-726
        m.state = MP2_GET_RATE;                                  // :727
        pos = p + 1;
      } else {                                                   // :735-744
        const int k = min(24 - m.bit_count, nbits - pos);
        m.header = (m.header << k) | (int)mp2_bits(frm, nbytes, pos, k);       // :737
        m.bit_count += k; pos += k;
        if (m.bit_count == 24) {                                 // :738
          mp2_header(m);                                         // :740
          m.state = MP2_GET_DATA;                                // :742
        }
      }
    }
  }
  pad_wave_close(w, ps, lds, lane);
  if (lane == 0) ps.m = m;
}

// --------------------------------------------------------------------------------------------- MP2 audio
// One block of 256 threads per slot whose MP2 audio is decoded (Mp2AudioDev::slots: those slots only), behind k_dabplus, beside the PAD
// stage: walks the logical frames the decoder produced in this batch step as k_pad_mp2 does -- the same sync walk (pad_core.h) on state of
// its own, every wave running its wave-uniform steps in step with the others -- but keeps every bit of GetSampleRate and GetData in MP2frame
// (mp2processor.cpp:689, :725, :737; in LDS for the launch, 6 kbps bytes in HBM between launches, never cleared): a run of bits goes from
// the staged logical frame to its bit offset in MP2frame as one funnel shift per destination byte (mp2a_copy_bits).  When an MP2 frame
// completes, _mp2_decode_frame (:377-609, mp2_core.h) runs on it:
//   parse     every wave the same: lane 2 sb + ch reads its allocation, scfsi and scale factors at positions that are wave prefix sums
//             (mp2a_scan), then wave w reads and requantises the sample triples of granules w, w + 4, w + 8 into smp[ch][sub-block][sb];
//   matrix    all 2 x 36 x 64 values of V at once: wave w takes (sub-block, channel) pairs w, w + 4, ..., lane i holds row i of N in
//             registers and reads the 32 samples as broadcasts; the rows go behind the channel's 16 history rows in LDS;
//   window    lane (ch << 5 | j) holds its 16 taps of D in registers and reads 16 values of V per output sample, straight into the
//             slot's byte ring; then the newest 16 rows become the history.
// LDS: frm 1152 + mp2f 2320 + smp 2 x (36 x 32 + 16) x 4 + v 2 x 52 x 64 x 4 = 39 440 bytes; tests/test_mp2_audio_lds.py states the bank
// behaviour of every access.  include/dabx.h "MP2 audio" states the semantics and guard G1.
struct Mp2AudioLds {
  __attribute__((aligned(16))) uint8_t frm[3 * MP2A_MAX_KBPS];            // the logical frame being walked
  __attribute__((aligned(16))) uint8_t mp2f[MP2A_FRAME_ROOM + 16];        // MP2frame
  __attribute__((aligned(16))) int smp[2][MP2A_SUBBLOCKS * 32 + 16];      // sample[ch][sub-block][sb]; + 16: the channels' lanes of a store on different banks
  __attribute__((aligned(16))) int v[2][(MP2A_HIST_ROWS + MP2A_SUBBLOCKS) * 64];      // V rows of a channel, oldest first: 16 of history, then the frame's 36
};

// exclusive prefix sum over the wave's 64 lanes; *total: the sum
__device__ __forceinline__ int mp2a_scan(int v, int lane, int *total)
{
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  *total = __shfl(incl, 63);
  return incl - v;
}

// bits [sbit, sbit + k) of src (n_src bytes) to bits [dbit, dbit + k) of dst, bit i of an array being bit 7 - (i & 7) of byte i >> 3
// (_add_bit_to_mp2, :749-763, k times): one thread per destination byte takes the 16 source bits its byte lies in and merges the part of
// the byte the run covers.  The barrier in front says that whatever wrote dst before is done (the first and last byte are shared with the
// neighbouring runs); callers put one behind before dst is read.
__device__ __forceinline__ void mp2a_copy_bits(uint8_t *dst, int dbit, const uint8_t *src, int n_src, int sbit, int k, int tid)
{
  __syncthreads();
  const int first = dbit >> 3, last = (dbit + k - 1) >> 3;
  for (int b = first + tid; b <= last; b += 256) {
    const int lo = max(dbit, 8 * b) - 8 * b, hi = min(dbit + k, 8 * b + 8) - 8 * b;      // the byte's bits [lo, hi), from the top
    const int s0 = sbit + 8 * b - dbit;                              // the source bit of the byte's top bit (>= -7)
    const int sb = s0 >> 3, sh = s0 & 7;
    const unsigned w = ((sb >= 0 && sb < n_src ? (unsigned)src[sb] : 0u) << 8) | (sb + 1 >= 0 && sb + 1 < n_src ? (unsigned)src[sb + 1] : 0u);
    const unsigned val = (w >> (8 - sh)) & 0xFFu, mask = (0xFFu >> lo) & (0xFF00u >> hi) & 0xFFu;
    dst[b] = (uint8_t)((dst[b] & ~mask) | (val & mask));
  }
}

__global__ __launch_bounds__(256) void k_mp2_audio(Mp2AudioDev ad)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Mp2AudioSlot &as = ad.slots[blockIdx.x];
  const size_t sj = (size_t)as.s * ad.max_subch + as.j;
  const SubchDev &sc = ad.subch[sj];
  if (!sc.active || sc.dab_plus || sc.kbps > MP2A_MAX_KBPS) return;
  const BatchSnap bs = ad.snap[as.s];
  const long long n_new = msc_new_frames(bs.msc_done, bs.cif_no, sc.start_cif).n;   // logical frames the decoder just produced for this sub-channel
  if (n_new == 0) return;
  const int nbytes = 3 * sc.kbps, nbits = 8 * nbytes;          // <= 1152 bytes (dabx_set_mp2_audio_mode); MP2framesize = 24 * bitRate (:236)
  const int cap = 6 * sc.kbps, limit = 48 * sc.kbps;            // MP2frame as kept / as the reference sizes it (:237)
  const uint8_t *ring = ad.msc_out + sj * MSC_SLOTS * ad.msc_stride;
  __shared__ Mp2AudioLds lds;
  uint8_t *const pcm_ring = as.out.bytes;
  dabx_mp2_audio_frame *const recs = as.out.recs;
  const unsigned long long bytes_mask = as.out.bytes_mask, rec_mask = as.out.rec_mask;
  long long n_recs = as.out.count, n_bytes = as.out.n_bytes;
  int32_t *const hist = as.hist;
  uint8_t *const mp2frame = as.mp2frame;
  for (int i = tid; i < (MP2A_FRAME_ROOM + 16) / 4; i += 256) reinterpret_cast<uint32_t *>(lds.mp2f)[i] = 4 * i < cap ? reinterpret_cast<const uint32_t *>(mp2frame)[i] : 0u;
  for (int i = tid; i < 2 * MP2A_HIST_ROWS * 64; i += 256) lds.v[i >> 10][i & 1023] = hist[i];
  int n_row[32], d_tap[16];                   // row `lane` of N; the window taps of output sample lane & 31
#pragma unroll
  for (int j = 0; j < 32; j++) n_row[j] = MP2_N[lane][j];
#pragma unroll
  for (int i = 0; i < 8; i++) { d_tap[2 * i] = MP2_D[64 * i + (lane & 31)]; d_tap[2 * i + 1] = MP2_D[64 * i + 32 + (lane & 31)]; }
  Mp2State m = as.m;
  Mp2AudioState a = as.a;
  const long long frame0 = sc.cif_out - n_new;
  for (long long n = 0; n < n_new; n++) {
    const long long frame = frame0 + n;       // index of the logical frame in the slot's sequence
    __syncthreads();
    {
      const uint32_t *src = reinterpret_cast<const uint32_t *>(ring + (size_t)(frame % MSC_SLOTS) * ad.msc_stride);
      for (int i = tid; i < nbytes / 4; i += 256) reinterpret_cast<uint32_t *>(lds.frm)[i] = src[i];
    }
    __syncthreads();
    int pos = 0;                              // :685 i
    while (pos < nbits) {
      if (m.state == MP2_GET_DATA) {                             // :687-714
        const int lf = m.sample_rate == 48000 ? nbits : 2 * nbits;      // :680, :741
        const int k = min(lf - m.bit_count, nbits - pos);
        mp2a_copy_bits(lds.mp2f, m.bit_count, lds.frm, nbytes, pos, k, tid);      // :689
        m.bit_count += k; pos += k;
        if (m.bit_count < lf) break;                             // (the logical frame is used up)
        m.frames++;                                              // :691 the MP2 frame is complete
        __syncthreads();
        // ---- _mp2_decode_frame (:377-609)
        a.decode_calls++;
        a.number_of_frames++;                                    // :388-394
        if (a.number_of_frames >= 25) { a.number_of_frames = 0; a.error_frames = 0; }
        const Mp2Header h = mp2a_header(pad_u(lds.mp2f[0]), pad_u(lds.mp2f[1]), pad_u(lds.mp2f[2]), pad_u(lds.mp2f[3]));
        if (h.status == 1) { a.error_frames++; a.bad_header++; }           // :397-403
        else if (h.status == 2) a.refused++;                     // :412-421
        else {
          const int sb = lane >> 1, ch = lane & 1;
          int at = h.pos, total;
          // allocation (:482-487): a lane from `bound` on whose channel is 1 has its neighbour's
          const int w_alloc = mp2a_alloc_bits(h, lane);
          unsigned av = mp2a_bits(lds.mp2f, cap, at + mp2a_scan(w_alloc, lane, &total), w_alloc);
          at += total;
          const unsigned av0 = (unsigned)__shfl((int)av, lane & ~1);
          const int q = mp2a_quantiser(h, sb, w_alloc || !ch ? av : av0);
          // scfsi (:491-499) and scale factors (:502-535).  Channel 1 of a mono frame reads none: its samples are channel 0's (below)
          const bool has_scf = q != 0 && ch < h.nch;
          const int w_sel = has_scf ? 2 : 0;
          const unsigned sel = mp2a_bits(lds.mp2f, cap, at + mp2a_scan(w_sel, lane, &total), w_sel);
          at += total;
          const int n_scf = has_scf ? mp2a_scf_count(sel) : 0;
          const int p_scf = at + mp2a_scan(6 * n_scf, lane, &total);
          at += total;
          const int v0 = (int)mp2a_bits(lds.mp2f, cap, p_scf, n_scf > 0 ? 6 : 0), v1 = (int)mp2a_bits(lds.mp2f, cap, p_scf + 6, n_scf > 1 ? 6 : 0),
                    v2 = (int)mp2a_bits(lds.mp2f, cap, p_scf + 12, n_scf > 2 ? 6 : 0);
          // samples (:538-556): every granule has the same size, so granule g of this lane starts at at + g * gran + off
          const bool reads = w_alloc != 0 && q != 0;
          int gran;
          const int off = mp2a_scan(reads ? mp2a_sample_bits(q) : 0, lane, &gran);
          for (int g = wave; g < 12; g += 4) {
            int s[3] = {0, 0, 0};
            if (reads) mp2a_read_samples(lds.mp2f, cap, at + g * gran + off, q, mp2a_scf_of(sel, g >> 2, v0, v1, v2), s);
#pragma unroll
            for (int idx = 0; idx < 3; idx++) {
              const int s0 = __shfl(s[idx], lane & ~1);          // :548-550: channel 0's sample, already scaled with channel 0's factor
              lds.smp[ch][(3 * g + idx) * 32 + sb] = w_alloc || !ch ? s[idx] : s0;
            }
          }
          const bool over = mp2a_refill_pos(at + 12 * gran) > limit;       // guard G1
          __syncthreads();
          // matrixing (:567-575)
          for (int p = wave; p < 2 * MP2A_SUBBLOCKS; p += 4) {
            const int k2 = p >> 1, c = p & 1;
            lds.v[c][(MP2A_HIST_ROWS + k2) * 64 + lane] = mp2a_matrix(n_row, &lds.smp[c][k2 * 32]);
          }
          __syncthreads();
          // window and output (:578-601): opPcm[(sub-block << 6) | (j << 1) | ch]
          for (int k2 = wave; k2 < MP2A_SUBBLOCKS; k2 += 4) {
            const int c = lane >> 5, j = lane & 31;
            const int sum = mp2a_window(lds.v[c], MP2A_HIST_ROWS + k2, j, d_tap);
            *reinterpret_cast<int16_t *>(pcm_ring + (size_t)((unsigned long long)(n_bytes + 2 * ((k2 << 6) | (j << 1) | c)) & bytes_mask)) = (int16_t)sum;
          }
          __syncthreads();
          int keep[8];                                           // the newest 16 rows of both channels become the history
#pragma unroll
          for (int i = 0; i < 8; i++) { const int e = tid + 256 * i; keep[i] = lds.v[e >> 10][MP2A_SUBBLOCKS * 64 + (e & 1023)]; }
#pragma unroll
          for (int i = 0; i < 8; i++) { const int e = tid + 256 * i; lds.v[e >> 10][e & 1023] = keep[i]; }
          a.voffs = (a.voffs - MP2A_SUBBLOCKS * 64) & 1023;      // :562, 36 times
          if (tid == 0) {                     // the 32 bytes of a dabx_mp2_audio_frame as four little-endian words
            unsigned long long *o = reinterpret_cast<unsigned long long *>(recs + (size_t)((unsigned long long)n_recs & rec_mask));
            o[0] = (unsigned long long)n_bytes; o[1] = (unsigned long long)frame;
            o[2] = (unsigned long long)(unsigned)m.sample_rate | ((unsigned long long)(unsigned)h.frame_size << 32);
            o[3] = (unsigned long long)lds.mp2f[1] | ((unsigned long long)lds.mp2f[2] << 8) | ((unsigned long long)lds.mp2f[3] << 16) |
                   ((unsigned long long)(h.stereo ? 1 : 0) << 24) | ((unsigned long long)(over ? 1 : 0) << 32);
          }
          a.frames_out++; a.overread += over ? 1 : 0;
          n_recs++; n_bytes += MP2A_PCM_BYTES;
        }
        m.state = MP2_SEARCHING; m.header_count = 0; m.bit_count = 0;   // :710-712
      } else if (m.state == MP2_SEARCHING) {                     // :715-734
        int run;
        const int p = mp2_find_sync(lds.frm, nbits, pos, m.header_count, lane, &run);
        if (p < 0) { m.header_count = run; break; }              // :720, :732 to the end of the frame
        m.syncs++; m.last_sync_bit = p;
        __syncthreads();
        if (tid == 0) { lds.mp2f[0] = 0xFF; lds.mp2f[1] |= 0xF0; }      // :722-726 twelve ones
        m.header_count = 12; m.bit_count = 12; m.header = 0;
        m.state = MP2_GET_RATE;                                  // :727
        pos = p + 1;
      } else {                                                   // :735-744
        const int k = min(24 - m.bit_count, nbits - pos);
        mp2a_copy_bits(lds.mp2f, m.bit_count, lds.frm, nbytes, pos, k, tid);      // :737
        m.header = (m.header << k) | (int)mp2_bits(lds.frm, nbytes, pos, k);
        m.bit_count += k; pos += k;
        if (m.bit_count == 24) {                                 // :738
          mp2_header(m);                                         // :740
          m.state = MP2_GET_DATA;                                // :742
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < cap / 4; i += 256) reinterpret_cast<uint32_t *>(mp2frame)[i] = reinterpret_cast<const uint32_t *>(lds.mp2f)[i];
  for (int i = tid; i < 2 * MP2A_HIST_ROWS * 64; i += 256) hist[i] = lds.v[i >> 10][i & 1023];
  if (tid == 0) { as.m = m; as.a = a; as.out.count = n_recs; as.out.n_bytes = n_bytes; }
}

// ------------------------------------------------------------------------------------------- AAC stream
// One wave per DAB+ slot whose access units are framed (AacStreamDev::slots: those slots only), behind k_dabplus, beside the PAD stage:
// walks the super frames k_dabplus has completed since the slot's last visit as k_pad does (SubchDev::sf_count against
// AacStreamSlot::sf_seen) and their dabx_superframe_info records -- no CRC runs here.  Per super frame, staged in LDS with dword loads:
// lane a < num_aus computes L, the verdict and the LOAS frame's length of access unit a (aac_core.h, aac_au: mp4processor.cpp:320-333,
// :377), a prefix sum over the lanes gives every access unit its byte_pos, lanes 0 .. num_aus - 1 store the records, and the frames are
// written straight to their place in the slot's byte ring, a byte per lane: the header from one of two templates (aac_header), everything
// behind it a copy shifted by 5 or 6 bits (aac_frame_byte).  A length-good access unit lies inside the super frame (k_dabplus's length
// check), so every LDS read does.  LDS: 5280 bytes.  include/dabx.h "AAC stream" states the semantics; there is no guard on the output's
// size.
__global__ __launch_bounds__(64) void k_aac_stream(AacStreamDev ad)
{
  const int lane = threadIdx.x;
  AacStreamSlot &as = ad.slots[blockIdx.x];
  const size_t sj = (size_t)as.s * ad.max_subch + as.j;
  const SubchDev &sc = ad.subch[sj];
  if (!sc.active || !sc.dab_plus || sc.kbps > 384) return;
  const long long have = sc.sf_count;
  long long seen = as.sf_seen;
  if (have <= seen) return;
  if (have - seen > SF_SLOTS) seen = have - SF_SLOTS;         // (cannot happen: the stage runs behind every batch)
  const int end = 110 * (sc.kbps / 8);
  __shared__ __attribute__((aligned(16))) uint8_t sfb[110 * 48];
  uint8_t *const ring = as.out.bytes;                            // (locals: the stores below must not make the loop reload them from the table)
  dabx_aac_frame *const recs = as.out.recs;
  const unsigned long long bytes_mask = as.out.bytes_mask, rec_mask = as.out.rec_mask;
  long long n_recs = as.out.count, n_bytes = as.out.n_bytes;
  long long frames = 0, lost_len = 0, lost_crc = 0;
  const long long recs0 = n_recs, bytes0 = n_bytes;
  for (long long sf = seen; sf < have; sf++) {
    const size_t slot = sj * SF_SLOTS + (size_t)(sf % SF_SLOTS);
    const dabx_superframe_info *inf = ad.sf_info + slot;
    __syncthreads();                                             // the previous super frame's bytes are done with
    {
      const uint32_t *src = reinterpret_cast<const uint32_t *>(ad.sf_out + slot * ad.sf_stride);
      for (int i = lane; i < (end + 3) / 4; i += 64) reinterpret_cast<uint32_t *>(sfb)[i] = src[i];
    }
    __syncthreads();
    const int n_au = min((int)inf->num_aus, 6);
    const unsigned parms = inf->stream_parms;
    const int sbr = (parms >> 5) & 1;
    AacAu u{0, 0, 0};
    if (lane < n_au) u = aac_au(*inf, lane);                     // mp4processor.cpp:320-333
    const int incl = row_prefix_sum_int(u.length);               // (lanes 0 .. 5: one row of 16)
    const int off = incl - u.length, total = __shfl(incl, 15);
    if (lane < n_au) {                           // the 32 bytes of a dabx_aac_frame as four little-endian words
      unsigned long long *o = reinterpret_cast<unsigned long long *>(recs + (size_t)((unsigned long long)(n_recs + lane) & rec_mask));
      o[0] = (unsigned long long)(n_bytes + off); o[1] = (unsigned long long)inf->first_frame;
      o[2] = (unsigned long long)(u.length & 0xFFFF) | ((unsigned long long)(u.L & 0xFFFF) << 16) | ((unsigned long long)lane << 32) |
             ((unsigned long long)n_au << 40) | ((unsigned long long)parms << 48) | ((unsigned long long)u.flags << 56);
      o[3] = 0;
    }
    frames += __popcll(__ballot(lane < n_au && u.flags == 0));
    lost_len += __popcll(__ballot(lane < n_au && u.flags == DABX_AAC_LOST_LEN));
    lost_crc += __popcll(__ballot(lane < n_au && u.flags == DABX_AAC_LOST_CRC));
    for (int a = 0; a < n_au; a++) {
      const int len = __shfl(u.length, a);
      if (len == 0) continue;                                    // :325-331, :377-382: the reference conceals
      const int L = __shfl(u.L, a);
      const long long at = n_bytes + __shfl(off, a);
      const uint8_t *au = sfb + inf->au_start[a];
      const AacHeader h = aac_header(parms, len);                // :399-432
      for (int i = lane; i < len; i += 64) ring[(size_t)((unsigned long long)(at + i) & bytes_mask)] = (uint8_t)aac_frame_byte(h, sbr, L, au, i);
    }
    n_recs += n_au; n_bytes += total;
  }
  if (lane == 0) {
    as.sf_seen = have; as.out.count = n_recs; as.out.n_bytes = n_bytes;
    as.superframes += have - seen; as.records += n_recs - recs0; as.frames += frames; as.frame_bytes += n_bytes - bytes0;
    as.lost_len += lost_len; as.lost_crc += lost_crc;
  }
}

// --------------------------------------------------------------------------------------------------- MOT
// One wave per MOT-enabled PAD slot (MotDev::slots: those slots only), behind k_pad and k_pad_mp2: walks the items the slot's PAD kernel has
// emitted since this slot's last visit (PadSlot::out.count against MotSlot::items_seen) out of the PAD rings and takes the
// DABX_PAD_DATAGROUP items through the tail of _build_MSC_segment and the handler's MotObject (mot_core.h: pad_handler.cpp:539-622 and
// mot_object.cpp:71-323 line by line).  The PAD rings hold what two batches emit, so every item of this batch is intact; the rule is
// checked all the same (out_ring_oldest, out_ring_intact) and a violation is counted in pad_overrun instead of read.  Header fields are
// wave-uniform and the state machine is scalar; the whole wave copies a body segment into the slot's arena and a header segment into LDS,
// completeness is a ballot over the segment table, and an emit gathers the stored segments in key order straight into the byte ring.
// include/dabx.h "MOT objects of the X-PAD" states the semantics and the guards M1..M3.
__global__ __launch_bounds__(64) void k_mot(MotDev md)
{
  const int lane = threadIdx.x;
  MotSlot &ms = md.slots[blockIdx.x];
  if (ms.pad_index < 0 || ms.pad_index >= md.n_pad) return;
  const PadSlot &ps = md.pad_slots[ms.pad_index];
  const long long count = ps.out.count;
  long long seen = ms.items_seen;
  if (count <= seen) return;
  __shared__ __attribute__((aligned(16))) uint8_t s_hdr[MOT_NAME_ROOM];
  MotWave w;
  w.h = ms.h; w.c = ms.c;
  w.pad_ring = ps.out.bytes; w.pad_mask = ps.out.bytes_mask;
  w.arena = ms.arena; w.name = ms.name; w.table = ms.table;
  w.ring = ms.out.bytes; w.recs = ms.out.recs; w.bytes_mask = ms.out.bytes_mask; w.rec_mask = ms.out.rec_mask;
  w.n_recs = ms.out.count; w.n_bytes = ms.out.n_bytes;
  w.max_object_bytes = ms.max_object_bytes;
  w.lane = lane; w.hdr = s_hdr; w.frame = 0; w.au = 0;
  const dabx_pad_item *items = ps.out.recs;
  const unsigned long long item_mask = ps.out.rec_mask;
  const long long oldest = out_ring_oldest(ps.out);
  if (seen < oldest) { w.c.pad_overrun += oldest - seen; seen = oldest; }      // (cannot happen: the stage runs behind every batch)
  for (long long i = seen; i < count; i++) {
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(items + (size_t)((unsigned long long)i & item_mask));
    const unsigned long long r2 = r[2];                          // length, kind, au, charset, crc_flag, crc_ok (pad_put_item)
    const unsigned lo = pad_u((unsigned)r2), hi = pad_u((unsigned)(r2 >> 32));
    if (((lo >> 16) & 0xFFu) != DABX_PAD_DATAGROUP) continue;
    const long long pos = (long long)(((unsigned long long)pad_u((unsigned)(r[0] >> 32)) << 32) | pad_u((unsigned)r[0]));
    if (!out_ring_intact(ps.out, pos)) { w.c.pad_overrun++; continue; }
    w.frame = (long long)(((unsigned long long)pad_u((unsigned)(r[1] >> 32)) << 32) | pad_u((unsigned)r[1]));
    w.au = (int)((lo >> 24) & 0xFFu);
    mot_group(w, pos, (int)(lo & 0xFFFFu), ((hi >> 8) & 1u) != 0, ((hi >> 16) & 1u) != 0);
  }
  __syncthreads();
  if (lane == 0) { ms.h = w.h; ms.c = w.c; ms.out.count = w.n_recs; ms.out.n_bytes = w.n_bytes; ms.items_seen = count; }
}

// ---------------------------------------------------------------------------------------------- carousel
// One wave per carousel-enabled packet-mode slot (CarouselDev::slots: those slots only), behind k_packet: walks the data groups k_packet has
// completed since this slot's last visit (PacketSlot::out.count against CarouselSlot::groups_seen) out of the packet slot's rings and takes
// them through MotHandler::add_MSC_data_group, its cache, MotDirectory and the MotObject of the store each group belongs to
// (carousel_core.h: mot_handler.cpp:69-259 and mot_dir.cpp:28-156 line by line; mot_core.h for the object).  The packet rings hold what two
// batches emit, so every group of this batch is intact; the rule is checked all the same (out_ring_oldest, out_ring_intact) and a violation
// is counted in dg_overrun instead of read.  Header fields are wave-uniform and the state machine is scalar; the wave as a whole looks an
// id up in the cache (one compare and a ballot) and in the directory (64 components per pass), copies segments and directory segments,
// checks the 512 marks and the segment table with ballots and gathers an emit into the byte ring.
// include/dabx.h "MOT objects of a packet-mode carousel" states the semantics and the guards C1..C3, D1..D4.
__global__ __launch_bounds__(64) void k_carousel(CarouselDev cd)
{
  const int lane = threadIdx.x;
  CarouselSlot &cs = cd.slots[blockIdx.x];
  if (cs.pkt_index < 0 || cs.pkt_index >= cd.n_pkt) return;
  const PacketSlot &ps = cd.pkt_slots[cs.pkt_index];
  const long long count = ps.out.count;
  long long seen = cs.groups_seen;
  if (count <= seen) return;
  __shared__ __attribute__((aligned(16))) uint8_t s_hdr[MOT_NAME_ROOM];
  CarWave cw;
  MotWave &w = cw.w;
  cw.cs = &cs; cw.d = cs.d; cw.x = cs.x; cw.open = 0;
  cw.pkt_ring = ps.out.bytes; cw.pkt_mask = ps.out.bytes_mask;
  w.h = MotState{}; w.c = cs.c;
  w.pad_ring = cw.pkt_ring; w.pad_mask = cw.pkt_mask;
  w.arena = cs.stores; w.name = cs.stores; w.table = nullptr;    // (car_open sets them)
  w.ring = cs.out.bytes; w.recs = cs.out.recs; w.bytes_mask = cs.out.bytes_mask; w.rec_mask = cs.out.rec_mask;
  w.n_recs = cs.out.count; w.n_bytes = cs.out.n_bytes;
  w.max_object_bytes = cs.max_object_bytes;
  w.lane = lane; w.hdr = s_hdr; w.frame = 0; w.au = 0;
  const dabx_datagroup_info *recs = ps.out.recs;
  const unsigned long long rec_mask = ps.out.rec_mask;
  const long long oldest = out_ring_oldest(ps.out);
  if (seen < oldest) { cw.x.dg_overrun += oldest - seen; seen = oldest; }      // (cannot happen: the stage runs behind every batch)
  for (long long i = seen; i < count; i++) {
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(recs + (size_t)((unsigned long long)i & rec_mask));
    const long long pos = (long long)(((unsigned long long)pad_u((unsigned)(r[0] >> 32)) << 32) | pad_u((unsigned)r[0]));
    if (!out_ring_intact(ps.out, pos)) { cw.x.dg_overrun++; continue; }
    w.frame = (long long)(((unsigned long long)pad_u((unsigned)(r[2] >> 32)) << 32) | pad_u((unsigned)r[2]));      // last_frame
    const unsigned lo = pad_u((unsigned)r[3]);                   // length, crc_flag, crc_ok
    car_group(cw, pos, (int)(lo & 0xFFFFu), ((lo >> 16) & 0xFFu) != 0, ((lo >> 24) & 0xFFu) != 0);
  }
  __syncthreads();
  if (lane == 0) { cs.d = cw.d; cs.c = w.c; cs.x = cw.x; cs.out.count = w.n_recs; cs.out.n_bytes = w.n_bytes; cs.groups_seen = count; }
}

// ----------------------------------------------------------------------------------------- data handlers
// One wave per packet-mode slot with a data handler on (DataDev::slots: those slots only), behind k_packet: walks the data groups k_packet
// has completed since this slot's last visit as k_carousel does (PacketSlot::out.count against DataSlot::groups_seen; out_ring_oldest and
// out_ring_intact are checked and a violation is counted in dg_overrun instead of read) and hands each to the slot's handler
// (data_core.h: tdc_datahandler.cpp:52-193, ip_datahandler.cpp:44-148, dabdgdec_impl.c:130-296 with journaline_datahandler.cpp:38-132,
// line by line).  The group is staged in LDS with dword loads -- at the byte offset it has in its first ring word, so ring words and LDS
// words line up; a ring of a power of two never splits a word at its end -- and a handler reads nothing but those N bytes.
// LDS: the group (DABX_DG_MAX_BYTES + 8), the two CRC tables (2 560) and the counters (200).  include/dabx.h "The data handlers of a packet-mode slot" states the semantics and the guards T1..T3, I1, J1.
struct DataLds {
  __attribute__((aligned(16))) uint8_t g[DABX_DG_MAX_BYTES + 8];
  uint16_t crc[256], xpow[DATA_XPOW];        // the CCITT table and x^(8 m) mod P (serial look-up chains: in LDS, as k_packet keeps them)
  DataCounters c;                              // the slot's counters for the launch: lane 0 counts
};

// the group at ring bytes [pos, pos + N), N <= DABX_DG_MAX_BYTES, into lds.g; returns where its byte 0 lies.  The barrier in front says the
// previous group is done with, the one behind that this one is there.
__device__ __forceinline__ const uint8_t *data_stage(DataLds &lds, const uint8_t *ring, unsigned long long mask, long long pos, int N, int lane)
{
  const int skew = (int)(pos & 3);
  __syncthreads();
  for (int k = lane; 4 * k < skew + N; k += 64)
    reinterpret_cast<uint32_t *>(lds.g)[k] = *reinterpret_cast<const uint32_t *>(ring + (size_t)((unsigned long long)(pos - skew + 4 * k) & mask));
  __syncthreads();
  return lds.g + skew;
}

__device__ __forceinline__ void data_wave_open(DataWave &w, DataLds &lds, const DataSlot &ds, const uint16_t *crc, const uint16_t *xpow, int lane)
{
  for (int i = lane; i < 256; i += 64) lds.crc[i] = crc[i];
  for (int i = lane; i < DATA_XPOW; i += 64) lds.xpow[i] = xpow[i];
  if (lane == 0) lds.c = ds.c;               // (data_stage's barrier in front of the first group says all of it is there)
  w.recs = ds.out.recs; w.ring = ds.out.bytes; w.rec_mask = ds.out.rec_mask; w.bytes_mask = ds.out.bytes_mask;
  w.n_recs = ds.out.count; w.n_bytes = ds.out.n_bytes; w.groups = ds.groups;
  w.jl = ds.jl; w.crc = lds.crc; w.xpow = lds.xpow; w.only_new = ds.only_new; w.lane = lane; w.c = &lds.c;
}

// the records [seen, count) of a ring of data groups (recs, rec_mask; their bytes in ring, mask) through the slot's handler
__device__ __forceinline__ void data_walk(DataWave &w, DataLds &lds, int handler, const dabx_datagroup_info *recs, unsigned long long rec_mask, const uint8_t *ring,
                                          unsigned long long mask, const OutRing<dabx_datagroup_info> *intact, long long seen, long long count, int lane)
{
  for (long long i = seen; i < count; i++) {
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(recs + (size_t)((unsigned long long)i & rec_mask));
    const long long pos = (long long)(((unsigned long long)pad_u((unsigned)(r[0] >> 32)) << 32) | pad_u((unsigned)r[0]));
    if (intact && !out_ring_intact(*intact, pos)) { data_count(w, &DataCounters::dg_overrun); continue; }
    const long long frame = (long long)(((unsigned long long)pad_u((unsigned)(r[2] >> 32)) << 32) | pad_u((unsigned)r[2]));      // last_frame
    const unsigned lo = pad_u((unsigned)r[3]);                   // length, crc_flag, crc_ok
    const int N = (int)(lo & 0xFFFFu);
    if (N > DABX_DG_MAX_BYTES) { data_count(w, &DataCounters::dg_overrun); continue; }   // (cannot happen: k_packet bounds a series there)
    const uint8_t *g = data_stage(lds, ring, mask, pos, N, lane);
    data_group(w, handler, g, N, ((lo >> 16) & 0xFFu) != 0, ((lo >> 24) & 0xFFu) != 0, frame, (unsigned)i);
  }
}

__global__ __launch_bounds__(64) void k_data_handler(DataDev dd)
{
  const int lane = threadIdx.x;
  DataSlot &ds = dd.slots[blockIdx.x];
  if (ds.pkt_index < 0 || ds.pkt_index >= dd.n_pkt) return;
  const PacketSlot &ps = dd.pkt_slots[ds.pkt_index];
  const long long count = ps.out.count;
  long long seen = ds.groups_seen;
  if (count <= seen) return;
  __shared__ DataLds lds;
  DataWave w;
  data_wave_open(w, lds, ds, dd.crc_ccitt, dd.crc_xpow, lane);
  const long long oldest = out_ring_oldest(ps.out);
  if (seen < oldest) { if (lane == 0) lds.c.dg_overrun += oldest - seen; seen = oldest; }      // (cannot happen: the stage runs behind every batch)
  data_walk(w, lds, ds.handler, ps.out.recs, ps.out.rec_mask, ps.out.bytes, ps.out.bytes_mask, &ps.out, seen, count, lane);
  if (lane == 0) { ds.c = lds.c; ds.groups = w.groups; ds.out.count = w.n_recs; ds.out.n_bytes = w.n_bytes; ds.groups_seen = count; }
}

// ... and the same walk over crafted groups without an engine (dabx_internal_data_walk_device): slot b's n_groups records, byte_pos counted
// in a ring of bytes_mask + 1 bytes that all slots share
__global__ __launch_bounds__(64) void k_data_batch(DataBatchSlot *slots, const uint8_t *bytes, unsigned long long bytes_mask, const uint16_t *crc, const uint16_t *xpow)
{
  const int lane = threadIdx.x;
  DataBatchSlot &bs = slots[blockIdx.x];
  DataSlot &ds = bs.st;
  __shared__ DataLds lds;
  DataWave w;
  data_wave_open(w, lds, ds, crc, xpow, lane);
  data_walk(w, lds, ds.handler, bs.groups, ~0ull, bytes, bytes_mask, nullptr, 0, bs.n_groups, lane);
  if (lane == 0) { ds.c = lds.c; ds.groups = w.groups; ds.out.count = w.n_recs; ds.out.n_bytes = w.n_bytes; ds.groups_seen = bs.n_groups; }
}

int launch_data_batch(DataBatchSlot *slots, int n_slots, const uint8_t *bytes, unsigned long long bytes_mask, hipStream_t st)
{
  const DevTables *t;
  int rc = get_tables(&t);
  if (rc) return rc;
  hipLaunchKernelGGL(k_data_batch, dim3(n_slots), dim3(64), 0, st, slots, bytes, bytes_mask, t->crc_ccitt, t->crc_xpow);
  DABX_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------- launchers
// One per stage, on the stream launch_msc_batch gives them.  The packet and PAD launchers take the engine's job table (null or n = 0: the
// engine has no such slot, no launch), fill in what the kernel reads of the engine and leave the argument they launched with in *used for
// the delivery's gather of the same slots (deliver.hip); used->n = 0 says that nothing ran.
__global__ void k_msc_done(EngineDev e)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < e.n_streams) e.ctl[s].msc_done_cif = e.snap[s].cif_no;
}

// every slot of the engine; closes the batch: msc_done_cif moves up to the snapshot's cif_no
int launch_dabplus_stage(const EngineDev &e, hipStream_t st, Marker &mk)
{
  const DevTables *t;
  int rc = get_tables(&t);
  if (rc) return rc;
  mk.begin(9, st);
  hipLaunchKernelGGL(k_dabplus, dim3(e.n_streams * e.max_subch), dim3(64), 0, st, e, *t);
  hipLaunchKernelGGL(k_msc_done, dim3((e.n_streams + 255) / 256), dim3(256), 0, st, e);
  mk.end(9, st);
  DABX_HIP(hipGetLastError());
  return 0;
}

// in front of k_dabplus, which moves the slots' frame counters on
int launch_packet_stage(const EngineDev &e, const PacketDev *pk, hipStream_t st, Marker &mk, PacketDev *used)
{
  *used = PacketDev{};
  if (!pk || pk->n <= 0) return 0;
  const DevTables *t;
  int rc = get_tables(&t);
  if (rc) return rc;
  PacketDev p = *pk;
  p.max_subch = e.max_subch; p.msc_stride = e.msc_stride; p.subch = e.subch; p.snap = e.snap; p.msc_out = e.msc_out;
  p.crc_ccitt = t->crc_ccitt; p.crc_xpow = t->crc_xpow;
  mk.begin(11, st);
  hipLaunchKernelGGL(k_packet, dim3(p.n), dim3(64), 0, st, p);
  mk.end(11, st);
  DABX_HIP(hipGetLastError());
  *used = p;
  return 0;
}

// behind k_packet: k_carousel reads the packet rings as that launch left them (`pk`: the argument launch_packet_stage launched with)
int launch_carousel_stage(const EngineDev &e, const CarouselDev *car, const PacketDev &pk, hipStream_t st, Marker &mk, CarouselDev *used)
{
  *used = CarouselDev{};
  if (!car || car->n <= 0 || pk.n <= 0) return 0;
  CarouselDev q = *car;
  q.max_subch = e.max_subch; q.pkt_slots = pk.slots; q.n_pkt = pk.n;
  mk.begin(14, st);
  hipLaunchKernelGGL(k_carousel, dim3(q.n), dim3(64), 0, st, q);
  mk.end(14, st);
  DABX_HIP(hipGetLastError());
  *used = q;
  return 0;
}

// behind k_packet, as k_carousel: k_data_handler reads the packet rings as that launch left them.  No marker: the profile table has no row
// for it (ctl->launches counts for dabx_data_stats; tools/bench_data_handlers.py times it through dabx_internal_data_timing)
int launch_data_stage(const EngineDev &e, const DataDev *data, const PacketDev &pk, hipStream_t st, DataStageCtl *ctl, DataDev *used)
{
  *used = DataDev{};
  if (!data || data->n <= 0 || pk.n <= 0) return 0;
  DataDev q = *data;
  q.max_subch = e.max_subch; q.pkt_slots = pk.slots; q.n_pkt = pk.n; q.crc_ccitt = pk.crc_ccitt; q.crc_xpow = pk.crc_xpow;
  hipEvent_t ev[2] = {nullptr, nullptr};     // dabx_internal_data_timing: the launch between two events of its own
  if (ctl && ctl->timing && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess || hipEventRecord(ev[0], st) != hipSuccess)) {
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
    set_error("launch_data_stage: no event pair for the launch");
    return DABX_E_HIP;
  }
  hipLaunchKernelGGL(k_data_handler, dim3(q.n), dim3(64), 0, st, q);
  if (ev[1]) {                               // the pair is kept only once both events are recorded
    if (hipEventRecord(ev[1], st) != hipSuccess) {
      for (hipEvent_t v : ev) (void)hipEventDestroy(v);
      set_error("launch_data_stage: the event behind the launch was not recorded");
      return DABX_E_HIP;
    }
    ctl->timed.push_back(ev[0]); ctl->timed.push_back(ev[1]);
  }
  if (ctl) ctl->launches++;
  DABX_HIP(hipGetLastError());
  *used = q;
  return 0;
}

// behind k_dabplus: k_pad walks the super frames it has just completed for the DAB+ slots, k_pad_mp2 the batch's logical frames of the slots
// whose source is MP2 (pad->n_mp2 of the pad->n), each launched only when it has a slot, both inside marker 12
int launch_pad_stage(const EngineDev &e, const PadDev *pad, hipStream_t st, Marker &mk, PadDev *used)
{
  *used = PadDev{};
  if (!pad || pad->n <= 0) return 0;
  const DevTables *t;
  int rc = get_tables(&t);
  if (rc) return rc;
  PadDev q = *pad;
  q.max_subch = e.max_subch; q.sf_stride = e.sf_stride; q.subch = e.subch; q.sf_out = e.sf_out; q.sf_info = e.sf_info;
  q.crc_ccitt = t->crc_ccitt; q.crc_xpow = t->crc_xpow;
  q.msc_stride = e.msc_stride; q.snap = e.snap; q.msc_out = e.msc_out;
  mk.begin(12, st);
  if (q.n > q.n_mp2) hipLaunchKernelGGL(k_pad, dim3(q.n), dim3(64), 0, st, q);
  if (q.n_mp2 > 0) hipLaunchKernelGGL(k_pad_mp2, dim3(q.n), dim3(64), 0, st, q);
  mk.end(12, st);
  DABX_HIP(hipGetLastError());
  *used = q;
  return 0;
}

// behind k_dabplus, beside the PAD stage: k_mp2_audio walks the batch's logical frames of the slots whose MP2 audio is decoded.  No marker:
// the profile table has no row for it (dabx_mp2_audio_stats.launches counts; tools/bench_mp2_audio.py times it)
int launch_mp2_audio_stage(const EngineDev &e, const Mp2AudioDev *ma, hipStream_t st, Mp2AudioDev *used)
{
  *used = Mp2AudioDev{};
  if (!ma || ma->n <= 0) return 0;
  Mp2AudioDev q = *ma;
  q.max_subch = e.max_subch; q.msc_stride = e.msc_stride; q.subch = e.subch; q.snap = e.snap; q.msc_out = e.msc_out;
  hipLaunchKernelGGL(k_mp2_audio, dim3(q.n), dim3(256), 0, st, q);
  DABX_HIP(hipGetLastError());
  *used = q;
  return 0;
}

// behind k_dabplus, beside the PAD stage: k_aac_stream walks the super frames just completed of the slots whose access units are framed.
// No marker: the profile table has no row for it (dabx_aac_stream_stats.launches counts; tools/bench_aac_stream.py times it)
int launch_aac_stream_stage(const EngineDev &e, const AacStreamDev *aa, hipStream_t st, AacStreamDev *used)
{
  *used = AacStreamDev{};
  if (!aa || aa->n <= 0 || !e.sf_info) return 0;
  AacStreamDev q = *aa;
  q.max_subch = e.max_subch; q.sf_stride = e.sf_stride; q.subch = e.subch; q.sf_out = e.sf_out; q.sf_info = e.sf_info;
  hipLaunchKernelGGL(k_aac_stream, dim3(q.n), dim3(64), 0, st, q);
  DABX_HIP(hipGetLastError());
  *used = q;
  return 0;
}

// behind the PAD stage: k_mot reads the PAD rings as that launch left them (`pad`: the argument launch_pad_stage launched with)
int launch_mot_stage(const EngineDev &e, const MotDev *mot, const PadDev &pad, hipStream_t st, Marker &mk, MotDev *used)
{
  *used = MotDev{};
  if (!mot || mot->n <= 0 || pad.n <= 0) return 0;
  MotDev q = *mot;
  q.max_subch = e.max_subch; q.pad_slots = pad.slots; q.n_pad = pad.n;
  mk.begin(13, st);
  hipLaunchKernelGGL(k_mot, dim3(q.n), dim3(64), 0, st, q);
  mk.end(13, st);
  DABX_HIP(hipGetLastError());
  *used = q;
  return 0;
}

}  // namespace dabx
