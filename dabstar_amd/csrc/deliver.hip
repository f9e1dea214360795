// deliver.hip -- bulk delivery of a chunk's results (include/dabx.h, "Bulk delivery"): two gather kernels pack everything the
// frames of one MSC batch produced -- FIBs + CRC flags + frame records (front-end stream), logical frames + super frames + the
// slots' counters (behind the DAB+ stage, on the stream that ran it) -- into ONE device slab; engine_delivery.cpp then moves the slab to a
// page-locked host slab with ONE transfer on an SDMA engine (sdma.h; the copier thread).  The host side of what the reference does per item:
// IFibDecoder::process_FIB from fic_decoder.cpp:234-261, FrameProcessor::add_to_frame from backend.cpp:160, the super frame of
// mp4processor.cpp:149-158.  Pure HBM copies: 14 208 B of results per frame + 13 % (super frames are the logical
// frames' bytes again, RS-corrected) -- 0.7 % of the chain's algorithmic bytes.
#include "pipeline.h"
#include "packet_core.h"
#include "pad_core.h"
#include "mot_core.h"
#include "carousel_core.h"
#include "mp2_core.h"
#include "aac_core.h"
#include "data_core.h"
#include "eti_core.h"
#include "tii_core.h"
#include "scope_core.h"
#include "cir_core.h"
#include "spectrum_core.h"
#include "fig_core.h"
#include "rec_ring.h"
#include "fig00.h"

namespace dabx {

// grid = n_streams, 128 threads, front-end stream, behind the chunk's last frame tail
__global__ __launch_bounds__(128) void k_deliver_front(EngineDev e, DeliverDev dv)
{
  const int s = blockIdx.x, tid = threadIdx.x;
  const StreamCtl &c = e.ctl[s];
  uint8_t *slab = dv.slab;
  if (s == 0 && tid == 0) *reinterpret_cast<dabx_chunk_header *>(slab) = dv.hdr;
  const int F = dv.hdr.max_frames;
  const long long done = dv.frames_done[s], have = c.frames - done;
  int n = (int)(have < F ? have : F);
  if (n > e.out_frames) n = e.out_frames;
  if (!(dv.hdr.what & DABX_DELIVER_FIB)) n = (int)(have < F ? have : F);     // no FIB bytes wanted: the count alone
  const long long first = c.frames - n;
  if (tid == 0) {
    dabx_chunk_stream r;
    r.first_frame = first; r.n_frames = n; r.frames_lost = (int)(have - n);
    r.state = c.state == ST_EVAL_SYNC ? 2 : (c.state == ST_WAIT_SYNC ? 1 : 0);
    r.fic_ratio_percent = c.fic_ratio * 10; r.cif_count = c.cif_count;
    r.snr_db_est = c.snr_db; r.freq_offs_bb_hz = c.f_bb; r.clock_err_hz = c.clock_err; r.signal_level = c.s_level;
    r.fic_ber_bits = c.fic_bits; r.fic_ber_errors = c.fic_errors; r.mer_db_est = c.mer_db;
    r.fib_ok = c.fib_ok; r.fib_total = c.fib_total;
    reinterpret_cast<dabx_chunk_stream *>(slab + dv.hdr.off_stream)[s] = r;
  }
  if (dv.hdr.what & DABX_DELIVER_FIB) {
    uint32_t *fo = reinterpret_cast<uint32_t *>(slab + dv.hdr.off_fib) + (size_t)s * F * 96;
    uint32_t *co = reinterpret_cast<uint32_t *>(slab + dv.hdr.off_crc) + (size_t)s * F * 3;
    dabx_chunk_frame *ro = reinterpret_cast<dabx_chunk_frame *>(slab + dv.hdr.off_frame) + (size_t)s * F;
    for (int i = tid; i < n * 96; i += 128) {
      const int f = i / 96, w = i - 96 * f;
      const size_t slot = (size_t)s * e.out_frames + (size_t)((first + f) % e.out_frames);
      fo[i] = reinterpret_cast<const uint32_t *>(e.fib_out + slot * 384)[w];
    }
    for (int i = tid; i < n * 3; i += 128) {
      const int f = i / 3, w = i - 3 * f;
      const size_t slot = (size_t)s * e.out_frames + (size_t)((first + f) % e.out_frames);
      co[i] = reinterpret_cast<const uint32_t *>(e.fib_crc + slot * 12)[w];
    }
    if (tid < n) {
      const size_t slot = (size_t)s * e.out_frames + (size_t)((first + tid) % e.out_frames);
      dabx_chunk_frame q;
      q.sym0_pos = e.frame_pos ? e.frame_pos[slot] : -1; q.start_index = e.frame_start ? e.frame_start[slot] : -1; q.reserved = 0;
      ro[tid] = q;
    }
  }
  if (tid == 0) dv.frames_done[s] = c.frames;
}

// Which logical frames of slot sj the chunk carries.  Called BEFORE the DAB+ stage (k_deliver_lf: cif_out has not been moved on yet, the
// batch's new frames are counted from its snapshot, msc_new_frames as in k_dabplus) and after it (k_deliver_msc: pre = false).
struct LfRange { long long first; int n, lost; };
__device__ __forceinline__ LfRange deliver_lf_range(const EngineDev &e, const DeliverDev &dv, int sj, const SubchDev &sc, bool pre)
{
  long long cif_out = sc.cif_out;
  if (pre) {
    const BatchSnap bs = e.snap[sj / e.max_subch];
    cif_out += msc_new_frames(bs.msc_done, bs.cif_no, sc.start_cif).n;
  }
  const int cap_cifs = 4 * dv.hdr.max_frames;
  const long long have = cif_out - dv.cif_done[sj];
  LfRange q;
  q.n = (int)(have < cap_cifs ? have : cap_cifs);
  if (q.n > MSC_SLOTS) q.n = MSC_SLOTS;
  if (q.n < 0) q.n = 0;
  q.lost = (int)(have > q.n ? have - q.n : 0);
  q.first = cif_out - q.n;
  const bool want_lf = (dv.hdr.what & DABX_DELIVER_MSC) || ((dv.hdr.what & DABX_DELIVER_MSC_NOT_DABPLUS) && !sc.dab_plus);
  if (!want_lf) { q.lost = 0; q.first = cif_out; q.n = 0; }      // not wanted: nothing is "lost"
  return q;
}

// grid = n_streams * max_subch, 64 threads, behind the chunk's Viterbi decode and IN FRONT of the DAB+ stage (same stream): the logical frames --
// half of an "everything" slab -- are gathered as soon as they exist, and their share of the slab goes onto the link while k_dabplus still runs
__global__ __launch_bounds__(64) void k_deliver_lf(EngineDev e, DeliverDev dv)
{
  const int sj = blockIdx.x, lane = threadIdx.x;
  const SubchDev &sc = e.subch[sj];
  if (!(sc.active && e.msc_out && !e.fic_only)) return;
  const LfRange q = deliver_lf_range(e, dv, sj, sc, true);
  if (q.n == 0) return;
  const uint8_t *ring = e.msc_out + (size_t)sj * MSC_SLOTS * e.msc_stride;
  uint32_t *o = reinterpret_cast<uint32_t *>(dv.slab + dv.layout_off[3 * (size_t)sj]);
  const int wpf = 3 * sc.kbps / 4;
  for (int f = 0; f < q.n; f++) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(ring + (size_t)((q.first + f) % MSC_SLOTS) * e.msc_stride);
    for (int w = lane; w < wpf; w += 64) o[(size_t)f * wpf + w] = src[w];
  }
}

// grid = n_streams * max_subch, 64 threads, behind k_dabplus of the chunk's MSC batch (same stream)
__global__ __launch_bounds__(64) void k_deliver_msc(EngineDev e, DeliverDev dv, int with_lf)
{
  const int sj = blockIdx.x, lane = threadIdx.x;
  const SubchDev &sc = e.subch[sj];
  uint8_t *slab = dv.slab;
  const unsigned long long msc_off = dv.layout_off[3 * (size_t)sj], sf_off = dv.layout_off[3 * (size_t)sj + 1], sfi_off = dv.layout_off[3 * (size_t)sj + 2];
  const int R = sc.kbps / 8, nb = 3 * sc.kbps, sfb = 110 * R, pitch = (sfb + 3) & ~3;
  const int cap_sf = (4 * dv.hdr.max_frames + 4) / 5;
  long long c_done = dv.cif_done[sj], s_done = dv.sf_done[sj];
  int n_c = 0, n_s = 0, lost_c = 0, lost_s = 0;
  long long first_c = c_done, first_s = s_done;
  const bool live = sc.active && e.msc_out && !e.fic_only;
  if (live) {
    const long long have_s = sc.sf_count - s_done;
    const LfRange q = deliver_lf_range(e, dv, sj, sc, false);          // the very range k_deliver_lf copied (it counted this batch's frames ahead)
    n_c = q.n; lost_c = q.lost; first_c = q.first;
    n_s = (int)(have_s < cap_sf ? have_s : cap_sf);
    if (n_s > SF_SLOTS) n_s = SF_SLOTS;
    if (n_s < 0) n_s = 0;
    lost_s = (int)(have_s > n_s ? have_s - n_s : 0);
    first_s = sc.sf_count - n_s;
    if (with_lf && n_c) {                                              // (no k_deliver_lf ran in front: the logical frames here as well)
      const uint8_t *ring = e.msc_out + (size_t)sj * MSC_SLOTS * e.msc_stride;
      uint32_t *o = reinterpret_cast<uint32_t *>(slab + msc_off);
      const int wpf = nb / 4;
      for (int f = 0; f < n_c; f++) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(ring + (size_t)((first_c + f) % MSC_SLOTS) * e.msc_stride);
        for (int w = lane; w < wpf; w += 64) o[(size_t)f * wpf + w] = src[w];
      }
    }
    if ((dv.hdr.what & DABX_DELIVER_SF) && sc.dab_plus) {
      const uint8_t *ring = e.sf_out + (size_t)sj * SF_SLOTS * e.sf_stride;
      uint32_t *o = reinterpret_cast<uint32_t *>(slab + sf_off);
      const int wpf = pitch / 4;
      for (int f = 0; f < n_s; f++) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(ring + (size_t)((first_s + f) % SF_SLOTS) * e.sf_stride);
        for (int w = lane; w < wpf; w += 64) o[(size_t)f * wpf + w] = src[w];
      }
      // ... and their records (32 bytes = 8 words each)
      if (e.sf_info && lane < 8 * n_s) {
        const uint32_t *inf = reinterpret_cast<const uint32_t *>(e.sf_info + (size_t)sj * SF_SLOTS);
        uint32_t *oi = reinterpret_cast<uint32_t *>(slab + sfi_off);
        for (int w = lane; w < 8 * n_s; w += 64) oi[w] = inf[(size_t)((first_s + (w >> 3)) % SF_SLOTS) * 8 + (w & 7)];
      }
    }
  }
  if (lane == 0) {
    dabx_chunk_subch r;
    r.active = live ? 1 : 0; r.subch_id = dv.subch_id[sj]; r.kbps = sc.kbps; r.dab_plus = sc.dab_plus;
    r.start_cif = sc.start_cif; r.first_cif = first_c; r.n_cifs = n_c; r.cifs_lost = lost_c;
    r.first_sf = first_s; r.n_sf = n_s; r.sf_lost = lost_s; r.msc_off = msc_off; r.sf_off = sf_off; r.sf_pitch = pitch; r.reserved = 0;
    r.sf_ok = sc.sf_ok; r.sf_fail = sc.sf_fail; r.rs_corrected = sc.rs_corr; r.rs_failed = sc.rs_fail; r.fc_corrected = sc.fc_corr;
    r.au_ok = sc.au_ok; r.au_bad = sc.au_bad; r.sfi_off = sfi_off;
    reinterpret_cast<dabx_chunk_subch *>(slab + dv.hdr.off_subch)[sj] = r;
    if (live) { dv.cif_done[sj] = sc.cif_out; dv.sf_done[sj] = sc.sf_count; }
  }
}

// The data-group section (include/dabx.h, dabx_chunk_dg): one wave per packet-mode slot, behind k_deliver_msc of the chunk (same stream; the
// table has been zeroed in front).  The groups completed since the previous chunk go out of the slot's rings (out_ring.h, out_ring_gather).
__global__ __launch_bounds__(64) void k_deliver_dg(PacketDev pk, uint8_t *slab, unsigned long long off_dg)
{
  PacketSlot &ps = pk.slots[blockIdx.x];
  if (!ps.out.dl_rec_off) return;
  const OutGather g = out_ring_gather(ps.out, slab, threadIdx.x);
  if (threadIdx.x == 0) {
    dabx_chunk_dg t;
    t.first_dg = g.first; t.n_dg = g.n; t.dg_lost = (int)(g.first - g.done); t.rec_off = ps.out.dl_rec_off; t.bytes_off = ps.out.dl_bytes_off; t.n_bytes = g.n_bytes;
    t.frames = ps.frames; t.packets = ps.packets; t.addr_match = ps.addr_match; t.continuity_err = ps.continuity_err; t.crc_bad = ps.crc_bad;
    t.len_bad = ps.len_bad; t.walk_short = ps.walk_short; t.dg_count = ps.out.count; t.dg_bytes = ps.out.n_bytes; t.dg_crc_bad = ps.dg_crc_bad;
    t.dg_overflow = ps.dg_overflow;
    reinterpret_cast<dabx_chunk_dg *>(slab + off_dg)[(size_t)ps.s * pk.max_subch + ps.j] = t;
    ps.out.dl_done = ps.out.count;
  }
}
int launch_deliver_dg(const EngineDev &e, const DeliverDev &dv, const PacketDev &pk, hipStream_t st)
{
  if (!dv.hdr.off_dg || pk.n <= 0) return 0;
  DABX_HIP(hipMemsetAsync(dv.slab + dv.hdr.off_dg, 0, sizeof(dabx_chunk_dg) * (size_t)e.n_streams * e.max_subch, st));
  hipLaunchKernelGGL(k_deliver_dg, dim3(pk.n), dim3(64), 0, st, pk, dv.slab, (unsigned long long)dv.hdr.off_dg);
  DABX_HIP(hipGetLastError());
  return 0;
}

// The PAD section (include/dabx.h, dabx_chunk_pad): one wave per PAD slot, behind k_deliver_dg of the chunk, in the same way.
__global__ __launch_bounds__(64) void k_deliver_pad(PadDev pd, uint8_t *slab, unsigned long long off_pad)
{
  PadSlot &ps = pd.slots[blockIdx.x];
  if (!ps.out.dl_rec_off) return;
  const OutGather g = out_ring_gather(ps.out, slab, threadIdx.x);
  if (threadIdx.x == 0) {
    dabx_chunk_pad t;
    t.first_item = g.first; t.n_items = g.n; t.items_lost = (int)(g.first - g.done); t.item_off = ps.out.dl_rec_off; t.bytes_off = ps.out.dl_bytes_off; t.n_bytes = g.n_bytes;
    t.superframes = ps.c.superframes; t.aus = ps.c.aus; t.pad_aus = ps.c.pad_aus; t.pad_bad = ps.c.pad_bad; t.labels = ps.c.labels;
    t.label_bytes = ps.c.label_bytes; t.groups = ps.c.groups; t.group_bytes = ps.c.group_bytes; t.dg_crc_bad = ps.c.dg_crc_bad;
    t.dl_overflow = ps.c.dl_overflow; t.li_bad = ps.c.li_bad;
    reinterpret_cast<dabx_chunk_pad *>(slab + off_pad)[(size_t)ps.s * pd.max_subch + ps.j] = t;
    ps.out.dl_done = ps.out.count;
  }
}
int launch_deliver_pad(const EngineDev &e, const DeliverDev &dv, const PadDev &pd, hipStream_t st)
{
  if (!dv.hdr.off_pad || pd.n <= 0) return 0;
  DABX_HIP(hipMemsetAsync(dv.slab + dv.hdr.off_pad, 0, sizeof(dabx_chunk_pad) * (size_t)e.n_streams * e.max_subch, st));
  hipLaunchKernelGGL(k_deliver_pad, dim3(pd.n), dim3(64), 0, st, pd, dv.slab, (unsigned long long)dv.hdr.off_pad);
  DABX_HIP(hipGetLastError());
  return 0;
}

// The MOT section (include/dabx.h, dabx_chunk_mot): one wave per MOT slot, behind k_deliver_pad of the chunk, in the same way.
__global__ __launch_bounds__(64) void k_deliver_mot(MotDev md, uint8_t *slab, unsigned long long off_mot)
{
  MotSlot &ms = md.slots[blockIdx.x];
  if (!ms.out.dl_rec_off) return;
  const OutGather g = out_ring_gather(ms.out, slab, threadIdx.x);
  if (threadIdx.x == 0) {
    dabx_chunk_mot t;
    t.first_object = g.first; t.n_objects = g.n; t.objects_lost = (int)(g.first - g.done); t.rec_off = ms.out.dl_rec_off; t.bytes_off = ms.out.dl_bytes_off; t.n_bytes = g.n_bytes;
    t.objects = ms.out.count; t.object_bytes = ms.out.n_bytes; t.groups = ms.c.groups; t.headers = ms.c.headers; t.segments = ms.c.segments;
    t.crc_bad = ms.c.crc_bad; t.grp_short = ms.c.grp_short; t.hdr_bad = ms.c.hdr_bad; t.obj_overflow = ms.c.obj_overflow; t.resets = ms.c.resets;
    t.progress_events = ms.c.progress_events;
    reinterpret_cast<dabx_chunk_mot *>(slab + off_mot)[(size_t)ms.s * md.max_subch + ms.j] = t;
    ms.out.dl_done = ms.out.count;
  }
}
int launch_deliver_mot(const EngineDev &e, const DeliverDev &dv, const MotDev &md, hipStream_t st)
{
  if (!dv.hdr.off_mot || md.n <= 0) return 0;
  DABX_HIP(hipMemsetAsync(dv.slab + dv.hdr.off_mot, 0, sizeof(dabx_chunk_mot) * (size_t)e.n_streams * e.max_subch, st));
  hipLaunchKernelGGL(k_deliver_mot, dim3(md.n), dim3(64), 0, st, md, dv.slab, (unsigned long long)dv.hdr.off_mot);
  DABX_HIP(hipGetLastError());
  return 0;
}

// ... and the rows of the carousel slots (a slot is a PAD slot or a packet slot, never both), by a second launch over their job table.
// clear_table: no k_deliver_mot ran for this chunk, the table is zeroed here.
__global__ __launch_bounds__(64) void k_deliver_carousel(CarouselDev cd, uint8_t *slab, unsigned long long off_mot)
{
  CarouselSlot &cs = cd.slots[blockIdx.x];
  if (!cs.out.dl_rec_off) return;
  const OutGather g = out_ring_gather(cs.out, slab, threadIdx.x);
  if (threadIdx.x == 0) {
    dabx_chunk_mot t;
    t.first_object = g.first; t.n_objects = g.n; t.objects_lost = (int)(g.first - g.done); t.rec_off = cs.out.dl_rec_off; t.bytes_off = cs.out.dl_bytes_off; t.n_bytes = g.n_bytes;
    t.objects = cs.out.count; t.object_bytes = cs.out.n_bytes; t.groups = cs.x.groups; t.headers = cs.c.headers; t.segments = cs.c.segments;
    t.crc_bad = cs.c.crc_bad; t.grp_short = cs.c.grp_short; t.hdr_bad = cs.c.hdr_bad; t.obj_overflow = cs.c.obj_overflow; t.resets = cs.c.resets;
    t.progress_events = 0;
    reinterpret_cast<dabx_chunk_mot *>(slab + off_mot)[(size_t)cs.s * cd.max_subch + cs.j] = t;
    cs.out.dl_done = cs.out.count;
  }
}
int launch_deliver_carousel(const EngineDev &e, const DeliverDev &dv, const CarouselDev &cd, hipStream_t st, bool clear_table)
{
  if (!dv.hdr.off_mot || cd.n <= 0) return 0;
  if (clear_table) DABX_HIP(hipMemsetAsync(dv.slab + dv.hdr.off_mot, 0, sizeof(dabx_chunk_mot) * (size_t)e.n_streams * e.max_subch, st));
  hipLaunchKernelGGL(k_deliver_carousel, dim3(cd.n), dim3(64), 0, st, cd, dv.slab, (unsigned long long)dv.hdr.off_mot);
  DABX_HIP(hipGetLastError());
  return 0;
}

// The MP2 audio section (include/dabx.h, dabx_chunk_mp2_audio): one wave per slot with the mode on, behind the other sections' gathers of the
// chunk, in the same way.
__global__ __launch_bounds__(64) void k_deliver_mp2_audio(Mp2AudioDev ad, uint8_t *slab, unsigned long long off_mp2_audio)
{
  Mp2AudioSlot &as = ad.slots[blockIdx.x];
  if (!as.out.dl_rec_off) return;
  const OutGather g = out_ring_gather(as.out, slab, threadIdx.x);
  if (threadIdx.x == 0) {
    dabx_chunk_mp2_audio t;
    t.first_frame = g.first; t.n_frames = g.n; t.frames_lost = (int)(g.first - g.done); t.rec_off = as.out.dl_rec_off; t.bytes_off = as.out.dl_bytes_off; t.n_bytes = g.n_bytes;
    t.decode_calls = as.a.decode_calls; t.frames_out = as.a.frames_out; t.bad_header = as.a.bad_header; t.refused = as.a.refused; t.overread = as.a.overread;
    t.sample_rate = as.m.sample_rate; t.voffs = as.a.voffs; t.number_of_frames = as.a.number_of_frames; t.error_frames = as.a.error_frames;
    t.reserved[0] = t.reserved[1] = 0;
    reinterpret_cast<dabx_chunk_mp2_audio *>(slab + off_mp2_audio)[(size_t)as.s * ad.max_subch + as.j] = t;
    as.out.dl_done = as.out.count;
  }
}
int launch_deliver_mp2_audio(const EngineDev &e, const DeliverDev &dv, const Mp2AudioDev &ad, unsigned long long off_mp2_audio, hipStream_t st)
{
  if (!off_mp2_audio || ad.n <= 0) return 0;
  DABX_HIP(hipMemsetAsync(dv.slab + off_mp2_audio, 0, sizeof(dabx_chunk_mp2_audio) * (size_t)e.n_streams * e.max_subch, st));
  hipLaunchKernelGGL(k_deliver_mp2_audio, dim3(ad.n), dim3(64), 0, st, ad, dv.slab, off_mp2_audio);
  DABX_HIP(hipGetLastError());
  return 0;
}

// The AAC section (include/dabx.h, dabx_chunk_aac): one wave per slot with the mode on, behind the other sections' gathers of the chunk, in
// the same way.
__global__ __launch_bounds__(64) void k_deliver_aac(AacStreamDev ad, uint8_t *slab, unsigned long long off_aac)
{
  AacStreamSlot &as = ad.slots[blockIdx.x];
  if (!as.out.dl_rec_off) return;
  const OutGather g = out_ring_gather(as.out, slab, threadIdx.x);
  if (threadIdx.x == 0) {
    dabx_chunk_aac t;
    t.first_frame = g.first; t.n_frames = g.n; t.frames_lost = (int)(g.first - g.done); t.rec_off = as.out.dl_rec_off; t.bytes_off = as.out.dl_bytes_off; t.n_bytes = g.n_bytes;
    t.superframes = as.superframes; t.records = as.records; t.frames = as.frames; t.frame_bytes = as.frame_bytes; t.lost_len = as.lost_len; t.lost_crc = as.lost_crc;
    for (int i = 0; i < 5; i++) t.reserved[i] = 0;
    reinterpret_cast<dabx_chunk_aac *>(slab + off_aac)[(size_t)as.s * ad.max_subch + as.j] = t;
    as.out.dl_done = as.out.count;
  }
}
int launch_deliver_aac(const EngineDev &e, const DeliverDev &dv, const AacStreamDev &ad, unsigned long long off_aac, hipStream_t st)
{
  if (!off_aac || ad.n <= 0) return 0;
  DABX_HIP(hipMemsetAsync(dv.slab + off_aac, 0, sizeof(dabx_chunk_aac) * (size_t)e.n_streams * e.max_subch, st));
  hipLaunchKernelGGL(k_deliver_aac, dim3(ad.n), dim3(64), 0, st, ad, dv.slab, off_aac);
  DABX_HIP(hipGetLastError());
  return 0;
}

// The data section (dabx_chunk_data): one wave per slot with a data handler on, behind k_data_handler -- out_ring_gather of what the slot
// emitted since the previous chunk into its room, and its row of the table (zeroed in front: rows of slots without a handler stay zero)
__global__ __launch_bounds__(64) void k_deliver_data(DataDev dd, uint8_t *slab, unsigned long long off_data)
{
  DataSlot &ds = dd.slots[blockIdx.x];
  if (!ds.out.dl_rec_off) return;
  const OutGather g = out_ring_gather(ds.out, slab, threadIdx.x);
  if (threadIdx.x == 0) {
    dabx_chunk_data t;
    t.first_item = g.first; t.n_items = g.n; t.items_lost = (int)(g.first - g.done); t.rec_off = ds.out.dl_rec_off; t.bytes_off = ds.out.dl_bytes_off; t.n_bytes = g.n_bytes;
    t.groups = ds.groups; t.items = ds.out.count; t.bytes = ds.out.n_bytes;
    for (int i = 0; i < 8; i++) t.reserved[i] = 0;
    reinterpret_cast<dabx_chunk_data *>(slab + off_data)[(size_t)ds.s * dd.max_subch + ds.j] = t;
    ds.out.dl_done = ds.out.count;
  }
}
int launch_deliver_data(const EngineDev &e, const DeliverDev &dv, const DataDev &dd, unsigned long long off_data, hipStream_t st)
{
  if (!off_data || dd.n <= 0) return 0;
  DABX_HIP(hipMemsetAsync(dv.slab + off_data, 0, sizeof(dabx_chunk_data) * (size_t)e.n_streams * e.max_subch, st));
  hipLaunchKernelGGL(k_deliver_data, dim3(dd.n), dim3(64), 0, st, dd, dv.slab, off_data);
  DABX_HIP(hipGetLastError());
  return 0;
}

// The second extension of a slab that carries DABX_DELIVER_DATA, at byte 192
__global__ void k_deliver_ext2(dabx_chunk_header_ext2 ext2, uint8_t *slab)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<dabx_chunk_header_ext2 *>(slab + sizeof(dabx_chunk_header) + sizeof(dabx_chunk_header_ext)) = ext2;
}
int launch_deliver_ext2(const dabx_chunk_header_ext2 &ext2, uint8_t *slab, hipStream_t st)
{
  hipLaunchKernelGGL(k_deliver_ext2, dim3(1), dim3(64), 0, st, ext2, slab);
  DABX_HIP(hipGetLastError());
  return 0;
}

// The header's extension of a slab that has one but no TII section (k_deliver_tii writes it otherwise)
__global__ void k_deliver_ext(dabx_chunk_header_ext ext, uint8_t *slab)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<dabx_chunk_header_ext *>(slab + sizeof(dabx_chunk_header)) = ext;
}
int launch_deliver_ext(const dabx_chunk_header_ext &ext, uint8_t *slab, hipStream_t st)
{
  hipLaunchKernelGGL(k_deliver_ext, dim3(1), dim3(64), 0, st, ext, slab);
  DABX_HIP(hipGetLastError());
  return 0;
}

int launch_deliver_front(const EngineDev &e, const DeliverDev &dv, hipStream_t st)
{
  hipLaunchKernelGGL(k_deliver_front, dim3(e.n_streams), dim3(128), 0, st, e, dv);
  DABX_HIP(hipGetLastError());
  return 0;
}

// ---- the record sections (include/dabx.h, dabx_chunk_tii / _scope / _cir / _spectrum; pipeline.h, RecDeliverDev) ----------------------------------
// One block gathers stream s = blockIdx.x's share of a section, with NT threads: the records the stream has written since the previous chunk,
// the newest CAP of them (what a chunk's frames can complete, and no more than the ring holds), out of the stage's record ring (rec_ring.h)
// into the stream's slots in the slab, and the stream's row of the section's table.  A stream without room in the slab (rec_off 0) delivers none.
template <int RING, int SLOT_BYTES, int CAP, int NT> __device__ __forceinline__ void deliver_records(const RecDeliverDev &rd)
{
  static_assert(SLOT_BYTES % 16 == 0 && sizeof(dabx_chunk_scope) % 16 == 0, "a record slot is copied in 16-byte words, out of and into 16-aligned slots");
  constexpr int SLOT_Q = SLOT_BYTES / 16;
  const int s = blockIdx.x, tid = threadIdx.x;
  const unsigned long long rec_off = rd.rec_off[s];
  const long long total = rd.ring ? rd.total[(size_t)s * rd.stride] : 0;
  const RecWindow w = rec_window(total, rec_off ? rd.done[s] : total, CAP);
  if (tid == 0) {
    dabx_chunk_scope r;
    r.first_record = w.first; r.n_records = w.n; r.records_lost = (int)w.gone; r.rec_off = rec_off; r.records_total = total;
    reinterpret_cast<dabx_chunk_scope *>(rd.slab + rd.off_table)[s] = r;
  }
  uint4 *o = reinterpret_cast<uint4 *>(rd.slab + rec_off);
  for (int i = tid; i < w.n * SLOT_Q; i += NT) {
    const int k = i / SLOT_Q, wd = i - k * SLOT_Q;
    o[i] = reinterpret_cast<const uint4 *>(rec_slot<RING, SLOT_BYTES>(rd.ring, s, w.first + k))[wd];
  }
  __syncthreads();
  if (tid == 0) rd.done[s] = total;
}

// grid = n_streams, 256 threads, front-end stream, behind k_deliver_front and the header's extension -- so behind the chunk's last k_scope
// (whichever HIP stream ran it: the frame's FIC decoder waits for the demapper launch behind k_scope), k_cir_finish and k_cir_corr, and
// k_spectrum, which run on that stream
template <int RING, int SLOT_BYTES, int CHUNK_RECORDS> __global__ __launch_bounds__(256) void k_deliver_records(RecDeliverDev rd)
{
  deliver_records<RING, SLOT_BYTES, (CHUNK_RECORDS < RING ? CHUNK_RECORDS : RING), 256>(rd);
}

// The TII section: grid = n_streams, 128 threads, front-end stream, behind k_deliver_front -- so behind the k_tii of the chunk's last frame;
// 4 events at the most (a chunk's frames cannot complete more), and every stream has room.  Block 0 writes the header's extension.
__global__ __launch_bounds__(128) void k_deliver_tii(RecDeliverDev rd, dabx_chunk_header_ext ext)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<dabx_chunk_header_ext *>(rd.slab + sizeof(dabx_chunk_header)) = ext;
  deliver_records<TII_RING, TII_SLOT_BYTES, 4, 128>(rd);
}

int launch_deliver_records(int section, int n_streams, const RecDeliverDev &rd, const dabx_chunk_header_ext &ext, hipStream_t st)
{
  const dim3 grid(n_streams), nt(256);
  switch (section) {
  case REC_TII: hipLaunchKernelGGL(k_deliver_tii, grid, dim3(128), 0, st, rd, ext); break;
  case REC_SCOPE: hipLaunchKernelGGL((k_deliver_records<SCOPE_RING, SCOPE_SLOT_BYTES, DABX_CHUNK_FRAMES>), grid, nt, 0, st, rd); break;
  case REC_CIR: hipLaunchKernelGGL((k_deliver_records<CIR_RING, CIR_SLOT_BYTES, DABX_CIR_CHUNK_RECORDS>), grid, nt, 0, st, rd); break;
  case REC_SPECTRUM: hipLaunchKernelGGL((k_deliver_records<SPEC_RING, SPEC_SLOT_BYTES, DABX_SPECTRUM_CHUNK_RECORDS>), grid, nt, 0, st, rd); break;
  case REC_FIG: hipLaunchKernelGGL((k_deliver_records<FIG_RING, FIG_SLOT_BYTES, DABX_FIG_CHUNK_RECORDS>), grid, nt, 0, st, rd); break;
  default: set_error("launch_deliver_records: section %d", section); return DABX_E_ARG;
  }
  DABX_HIP(hipGetLastError());
  return 0;
}

// with_lf: no launch_deliver_lf went in front (the logical frames are gathered here too)
int launch_deliver_msc(const EngineDev &e, const DeliverDev &dv, hipStream_t st, bool with_lf)
{
  if (e.max_subch <= 0) return 0;
  hipLaunchKernelGGL(k_deliver_msc, dim3(e.n_streams * e.max_subch), dim3(64), 0, st, e, dv, with_lf ? 1 : 0);
  DABX_HIP(hipGetLastError());
  return 0;
}
// behind the batch's Viterbi decode, in front of its DAB+ stage; records dv.lf_done behind the gather
int launch_deliver_lf(const EngineDev &e, const DeliverDev &dv, hipStream_t st)
{
  if (e.max_subch <= 0 || !dv.lf_done) return 0;
  hipLaunchKernelGGL(k_deliver_lf, dim3(e.n_streams * e.max_subch), dim3(64), 0, st, e, dv);
  DABX_HIP(hipEventRecord(dv.lf_done, st));
  DABX_HIP(hipGetLastError());
  return 0;
}

// ---- the ETI stage (include/dabx.h, dabx_chunk_eti; pipeline.h, EtiDev): the stream of frames dabx_read_eti defines, built on the device ----
// Front half, grid = n_streams, 128 threads, front-end stream, beside k_deliver_front: the FIBs of the chunk's frames into the chunk's
// staging, and the FIG 0/0 counter walked over those whose CRC is good (fib_fig00_counter, one FIB per thread; thread 0 strings them together).
__global__ __launch_bounds__(128) void k_eti_front(EngineDev e, EtiDev t)
{
  constexpr int F = MSC_BATCH_FRAMES;
  __shared__ int32_t found[12 * F], fhi[12 * F], flo[12 * F];
  const int s = blockIdx.x, tid = threadIdx.x;
  const StreamCtl &c = e.ctl[s];
  const EtiFront cur = t.front[s];
  EtiStage &st = t.stage[s];
  const long long frames = c.frames, have = frames - cur.fib_frames;
  const int n = have < 0 ? 0 : (int)(have < F ? have : F);           // (older frames have left the chunk: their FIBs are not walked, as in dabx_read_eti)
  const long long first = frames - n;
  for (int i = tid; i < n * 96; i += 128) {
    const int f = i / 96, w = i - 96 * f;
    const size_t slot = (size_t)s * e.out_frames + (size_t)((first + f) % e.out_frames);
    st.fib[f][w] = reinterpret_cast<const uint32_t *>(e.fib_out + slot * 384)[w];
  }
  for (int q = tid; q < 12 * n; q += 128) {
    const int f = q / 12, i = q - 12 * f;
    const size_t slot = (size_t)s * e.out_frames + (size_t)((first + f) % e.out_frames);
    int hi = -1, lo = -1;
    found[q] = e.fib_crc[slot * 12 + i] && fib_fig00_counter(e.fib_out + slot * 384 + 32 * i, &hi, &lo);
    fhi[q] = hi; flo[q] = lo;
  }
  __syncthreads();
  if (tid == 0) {
    int hi = cur.hi, lo = cur.lo;
    for (int f = 0; f < n; f++) {
      for (int i = 0; i < 12; i++) if (found[12 * f + i]) { hi = fhi[12 * f + i]; lo = flo[12 * f + i]; }
      st.hi[f] = hi; st.lo[f] = lo;
    }
    st.first_frame = first; st.n_frames = n; st.hi_cif = c.cif_no; st.end_hi = hi; st.end_lo = lo; st.pad_ = 0; st.fib_frames = frames;
    t.front[s] = EtiFront{frames, hi, lo};
  }
}

// Which CIFs of stream s the chunk turns into rows: [first_cif, first_cif + n_eti), and why the others of [next_cif, hi_cif) are not.
// In CIF order: lost (gone from a ring, or more than the rows' room), waiting (a de-interleaver not filled, no FIG 0/0 yet), then the rows
// -- or none of them, refused, when the layout does not fit a frame.  Computed by every wave that needs it, all lanes.
struct EtiPlan { long long first_cif, hi_cif; int n_eti, lost, waiting, refused, n_subch; };
__device__ __forceinline__ long long wave_max_ll(long long v)
{
  for (int d = 32; d > 0; d >>= 1) { const long long o = __shfl_xor(v, d); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ EtiPlan eti_plan(const EngineDev &e, const EtiDev &t, int s, int lane, bool pre)
{
  const EtiStage &st = t.stage[s];
  const long long next = t.next_cif[s], hi_cif = st.hi_cif > next ? st.hi_cif : next;
  long long wait_lo = 0, over_lo = 0;
  int n_act = 0, sum_kbps = 0;
  for (int j0 = 0; j0 < e.max_subch; j0 += 64) {
    const int j = j0 + lane;
    long long w = 0, o = 0;
    int a = 0, k = 0;
    if (j < e.max_subch && e.msc_out) {
      const SubchDev &sc = e.subch[(size_t)s * e.max_subch + j];
      if (sc.active) {
        a = 1; k = sc.kbps; w = msc_first_cif(sc.start_cif);
        long long cif_out = sc.cif_out;
        if (pre) { const BatchSnap bs = e.snap[s]; cif_out += msc_new_frames(bs.msc_done, bs.cif_no, sc.start_cif).n; }
        if (cif_out > MSC_SLOTS) o = w + cif_out - MSC_SLOTS;          // the oldest logical frame still in the slot's ring
      }
    }
    n_act += wave_sum_int(a); sum_kbps += wave_sum_int(k);
    w = wave_max_ll(w); o = wave_max_ll(o);
    wait_lo = w > wait_lo ? w : wait_lo; over_lo = o > over_lo ? o : over_lo;
  }
  const int cap = 4 * t.max_frames;
  long long lost_lo = next;
  if (over_lo > lost_lo) lost_lo = over_lo;
  if (4 * st.first_frame > lost_lo) lost_lo = 4 * st.first_frame;                  // the FIBs of older frames were not staged
  if (hi_cif - cap > lost_lo) lost_lo = hi_cif - cap;
  if (hi_cif > 4 * (st.first_frame + st.n_frames) || lost_lo > hi_cif) lost_lo = hi_cif;
  long long ctr_lo = hi_cif;                                                       // eti_generator.cpp:156-160: no frame before the first FIG 0/0
  for (int i = st.n_frames - 1; i >= 0; i--) if (st.hi[i] >= 0 && st.lo[i] >= 0) ctr_lo = 4 * (st.first_frame + i);
  long long emit_lo = lost_lo;
  if (wait_lo > emit_lo) emit_lo = wait_lo;
  if (ctr_lo > emit_lo) emit_lo = ctr_lo;
  if (emit_lo > hi_cif) emit_lo = hi_cif;
  const bool refused = n_act > 64 || eti_used_bytes(n_act, sum_kbps) > DABX_ETI_FRAME_BYTES;
  EtiPlan p;
  p.hi_cif = hi_cif; p.lost = (int)(lost_lo - next); p.waiting = (int)(emit_lo - lost_lo);
  p.refused = refused ? (int)(hi_cif - emit_lo) : 0;
  p.n_eti = refused ? 0 : (int)(hi_cif - emit_lo);
  p.first_cif = hi_cif - p.n_eti; p.n_subch = n_act;
  return p;
}

// grid = (4 * max_frames, n_streams), one wave each: row k of stream s, behind the batch's Viterbi decode (pre != 0: in front of its DAB+ stage,
// SubchDev::cif_out not moved on yet).  The FIC of CIF r with the logical frame r - start_cif - 16 of every active slot, in slot order.
__global__ __launch_bounds__(64) void k_eti_rows(EngineDev e, EtiDev t, int pre)
{
  __shared__ EtiSlot slots[64];
  const int k = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const EtiPlan p = eti_plan(e, t, s, lane, pre != 0);
  if (k >= p.n_eti) return;
  const long long r = p.first_cif + k;
  int base = 0;
  for (int j0 = 0; j0 < e.max_subch; j0 += 64) {
    const int j = j0 + lane;
    const size_t sj = (size_t)s * e.max_subch + (j < e.max_subch ? j : 0);
    const bool a = j < e.max_subch && e.msc_out && e.subch[sj].active;
    const unsigned long long m = __ballot(a);
    if (a) {
      const SubchDev &sc = e.subch[sj];
      const long long lf = r - sc.start_cif - 16;
      EtiSlot q;
      q.src = reinterpret_cast<const uint32_t *>(e.msc_out + (sj * MSC_SLOTS + (size_t)(lf % MSC_SLOTS)) * e.msc_stride);
      q.stc = eti_stc_word(t.subch_id[sj], r < sc.move_cif ? sc.prev_cu_start : sc.cu_start, sc.kbps, sc.prot_level, sc.short_form);
      q.ndw = 3 * sc.kbps / 4;
      slots[base + __popcll(m & ((1ull << lane) - 1ull))] = q;
    }
    base += __popcll(m);
  }
  __syncthreads();
  const EtiStage &st = t.stage[s];
  const int fi = (int)(r / 4 - st.first_frame);
  uint32_t *row = reinterpret_cast<uint32_t *>(t.slab + t.rows_off + ((size_t)s * 4 * t.max_frames + k) * DABX_ETI_FRAME_BYTES);
  eti_build_frame(st.hi[fi], st.lo[fi], (int)(r & 3), p.n_subch, slots, st.fib[fi] + 24 * (int)(r & 3), row, lane);
}

// grid = n_streams, one wave each, behind k_eti_rows: the stream's record, and the cursor moves on
__global__ __launch_bounds__(64) void k_eti_close(EngineDev e, EtiDev t, int pre)
{
  const int s = blockIdx.x, lane = threadIdx.x;
  const EtiPlan p = eti_plan(e, t, s, lane, pre != 0);
  if (lane != 0) return;
  const EtiStage &st = t.stage[s];
  dabx_chunk_eti r{};
  r.first_cif = p.first_cif; r.n_eti = p.n_eti; r.cifs_lost = p.lost; r.cifs_waiting = p.waiting; r.cifs_refused = p.refused;
  r.cif_hi = st.end_hi; r.cif_lo = st.end_lo; r.fib_frames = st.fib_frames;
  r.rows_off = t.rows_off + (size_t)s * 4 * t.max_frames * DABX_ETI_FRAME_BYTES;
  reinterpret_cast<dabx_chunk_eti *>(t.slab + t.off_eti)[s] = r;
  t.next_cif[s] = p.hi_cif;
}

int launch_eti_front(const EngineDev &e, const EtiDev &t, hipStream_t st, Marker &mk)
{
  mk.begin(15, st);
  hipLaunchKernelGGL(k_eti_front, dim3(e.n_streams), dim3(128), 0, st, e, t);
  mk.end(15, st);
  DABX_HIP(hipGetLastError());
  return 0;
}
int launch_eti_back(const EngineDev &e, const EtiDev &t, hipStream_t st, Marker &mk, bool pre)
{
  mk.begin(15, st);
  hipLaunchKernelGGL(k_eti_rows, dim3(4 * t.max_frames, e.n_streams), dim3(64), 0, st, e, t, pre ? 1 : 0);
  hipLaunchKernelGGL(k_eti_close, dim3(e.n_streams), dim3(64), 0, st, e, t, pre ? 1 : 0);
  mk.end(15, st);
  DABX_HIP(hipGetLastError());
  return 0;
}

// dabx_eti_frames_device (capi_stage.cpp): n frames of one layout through the same body, a wave each
__global__ __launch_bounds__(64) void k_eti_frames(const int32_t *cif_hi, const int32_t *cif_lo, const int32_t *minor, int n_subch, const uint32_t *stc,
                                                   const int32_t *ndw, const int32_t *off, int sum_dw, const uint32_t *fic, const uint32_t *msc,
                                                   uint32_t *out, int32_t *used)
{
  __shared__ EtiSlot slots[64];
  const int f = blockIdx.x, lane = threadIdx.x;
  if (lane < n_subch) slots[lane] = EtiSlot{msc + (size_t)f * sum_dw + off[lane], stc[lane], ndw[lane]};
  __syncthreads();
  const int u = eti_build_frame(cif_hi[f], cif_lo[f], minor[f], n_subch, slots, fic + (size_t)f * 24, out + (size_t)f * 1536, lane);
  if (lane == 0) used[f] = u;
}
int launch_eti_frames(int n, const int32_t *cif_hi, const int32_t *cif_lo, const int32_t *minor, int n_subch, const uint32_t *stc, const int32_t *ndw,
                      const int32_t *off, int sum_dw, const uint32_t *fic, const uint32_t *msc, uint32_t *out, int32_t *used, hipStream_t st)
{
  hipLaunchKernelGGL(k_eti_frames, dim3(n), dim3(64), 0, st, cif_hi, cif_lo, minor, n_subch, stc, ndw, off, sum_dw, fic, msc, out, used);
  DABX_HIP(hipGetLastError());
  return 0;
}

// ---- the TII detector on the device (tii_core.h): k_tii, the engine's stage behind the frame tail (include/dabx.h, dabx_set_tii_mode), and
// k_tii_batch, the same device function on crafted sums (dabx_tii_process_device) ----
// grid = n_streams, 256 threads, front-end stream, behind k_frame_tail of the same step: the next frame's accumulation cannot start before
// this kernel has finished.  A block has work only in the step whose TII null symbol brought its stream's sum to min_frames -- when
// DabProcessor runs process_tii_data (dab_processor.cpp:287-300).  A stream that is out of lock has no frame in the step (frame_ok = 0); its
// sum and count belong to the search (k_acquire), which may be running on its own HIP stream, and are not looked at.
__global__ __launch_bounds__(256) void k_tii(EngineDev e, TiiDev t)
{
  __shared__ TiiLds w;
  const int s = blockIdx.x, tid = threadIdx.x;
  const TiiCfgDev cfg = t.cfg[s];
  if (!cfg.enable) return;
  const StreamCtl &c = e.ctl[s];
  if (!c.frame_ok || (c.cif_count & 7) < 4) return;          // no frame in this step, or its null symbol was not a TII one (:274)
  const int in_sum = e.tii_cnt[2 * s], epoch = e.tii_cnt[2 * s + 1];
  if (in_sum < cfg.min_frames) return;
  float2 *pairs = t.pairs + (size_t)s * TII_PAIRS;
  const bool reset = epoch != cfg.epoch_seen;                 // the lock was lost since the detector last ran: TiiDetector::reset clears both buffers (:149-153)
  if (reset) for (int i = tid; i < TII_PAIRS; i += 256) pairs[i] = make_float2(0.f, 0.f);   // (each thread clears the pairs it advances below)
  const TiiCounters n = t.cnt[s];
  uint8_t *slot = t.ring + ((size_t)s * TII_RING + (size_t)(n.events % TII_RING)) * TII_SLOT_BYTES;
  dabx_tii_result *res = reinterpret_cast<dabx_tii_result *>(slot + sizeof(dabx_tii_event));
  const int found = tii_detect(e.tii_acc + (size_t)s * TU, pairs, cfg, t.turn, t.pattern, res, w, tid);
  const int stored = found < DABX_TII_MAX_RESULTS ? found : DABX_TII_MAX_RESULTS;
  if (tid >= stored && tid < DABX_TII_MAX_RESULTS) {          // the rest of the slot: zeros, whatever an older event left there
    uint32_t *z = reinterpret_cast<uint32_t *>(res + tid);
    z[0] = z[1] = z[2] = z[3] = 0;
  }
  if (tid == 0) {
    dabx_tii_event ev;
    ev.frame = c.frames - 1;                                  // (the tail has counted the frame)
    ev.n_results = stored; ev.n_found = found; ev.frames_in_sum = in_sum; ev.epoch = epoch; ev.threshold_db = cfg.threshold_db; ev.reserved = 0;
    *reinterpret_cast<dabx_tii_event *>(slot) = ev;
    e.tii_cnt[2 * s] = 0;                                     // mTiiCounter = 0
    if (reset) t.cfg[s].epoch_seen = epoch;
    t.cnt[s] = TiiCounters{n.events + 1, n.results + stored, n.truncated + (found > stored ? 1 : 0), n.resets + (reset ? 1 : 0)};
  }
}

int launch_tii(const EngineDev &e, const TiiDev &t, hipStream_t st)
{
  hipLaunchKernelGGL(k_tii, dim3(e.n_streams), dim3(256), 0, st, e, t);
  DABX_HIP(hipGetLastError());
  return 0;
}

// grid = n detectors, 256 threads
__global__ __launch_bounds__(256) void k_tii_batch(float2 *sums, float2 *pairs, const TiiCfgDev *cfg, const uint8_t *turn, const uint8_t *pattern,
                                                   dabx_tii_result *out, int32_t *n_results, int32_t *n_found)
{
  __shared__ TiiLds w;
  const int d = blockIdx.x, tid = threadIdx.x;
  const TiiCfgDev c = cfg[d];
  if (!c.enable) return;
  const int found = tii_detect(sums + (size_t)d * TU, pairs + (size_t)d * TII_PAIRS, c, turn, pattern, out + (size_t)d * DABX_TII_MAX_RESULTS, w, tid);
  if (tid == 0) { n_found[d] = found; n_results[d] = found < DABX_TII_MAX_RESULTS ? found : DABX_TII_MAX_RESULTS; }
}

int launch_tii_batch(int n, float2 *sums, float2 *pairs, const TiiCfgDev *cfg, const uint8_t *turn, const uint8_t *pattern, dabx_tii_result *out,
                     int32_t *n_results, int32_t *n_found, hipStream_t st)
{
  hipLaunchKernelGGL(k_tii_batch, dim3(n), dim3(256), 0, st, sums, pairs, cfg, turn, pattern, out, n_results, n_found);
  DABX_HIP(hipGetLastError());
  return 0;
}

// ---- the FIG walk on the device (fig_core.h): k_fig, the engine's stage behind the FIC decoder of the same frame (include/dabx.h,
// dabx_set_fig_mode), and k_fig_batch, the same device function on crafted FIBs (dabx_fig_walk_device).  One wave per decoder: the decoder's
// state comes into LDS with coalesced loads, the frame's 12 FIBs and CRC verdicts with one load per lane, the FIBs are walked in
// transmission order, and the state goes back. ----
struct FigLds {
  FigState st;
  uint32_t fib[96];                              // 12 FIBs of 32 bytes
  uint32_t crc[3];                               // their 12 verdicts
};
struct FigSiLds {                                // ... with the service information of the decoder beside it (fig_si_core.h)
  FigLds w;
  FigSiState si;
};
static_assert(sizeof(FigSiLds) < 64 * 1024, "FigState, FigSiState and the frame share the 64 KB of static LDS a workgroup can have");

__device__ inline void fig_words_move(uint32_t *dst, const uint32_t *src, int n_words, int lane)
{
  for (int i = lane; i < n_words; i += 64) dst[i] = src[i];
  fig_sync();
}
__device__ inline void fig_state_move(uint32_t *dst, const uint32_t *src, int lane) { fig_words_move(dst, src, (int)(sizeof(FigState) / 4), lane); }
__device__ inline void fig_si_move(FigSiState *dst, const FigSiState *src, int lane)
{
  fig_words_move(reinterpret_cast<uint32_t *>(dst), reinterpret_cast<const uint32_t *>(src), (int)(sizeof(FigSiState) / 4), lane);
}

// One stream's frame: the state into LDS, the 12 FIBs walked, the state back.  si: the stream's service information in LDS, loaded and
// stored by the caller; nullptr: not followed (k_fig passes the constant, and nothing of fig_si_core.h remains in it).
__device__ __forceinline__ void fig_frame(FigLds &w, FigSiState *si, const StreamCtl *ctl, const uint8_t *fib_out, const uint8_t *fib_crc, int out_frames, const FigDev &f,
                                 int s, int lane)
{
  const StreamCtl &c = ctl[s];
  const long long frame = c.frames - 1;                      // (the frame has been counted)
  const size_t slot = (size_t)s * out_frames + (size_t)(frame % out_frames);
  w.fib[lane] = reinterpret_cast<const uint32_t *>(fib_out + slot * 384)[lane];
  if (lane < 32) w.fib[64 + lane] = reinterpret_cast<const uint32_t *>(fib_out + slot * 384)[64 + lane];
  if (lane < 3) w.crc[lane] = reinterpret_cast<const uint32_t *>(fib_crc + slot * 12)[lane];
  fig_state_move(reinterpret_cast<uint32_t *>(&w.st), reinterpret_cast<const uint32_t *>(f.st + s), lane);
  if (w.st.fibs < 12 * frame) w.st.fibs = 12 * frame;        // FIB k of frame n is FIB 12 n + k of the stream, as dabx_follow_fic counts
  fig_sync();
  const FigOut o{f.labels + (size_t)s * FIG_LAB_SLOTS, f.ring + (size_t)s * FIG_RING, si};
  const uint8_t *fb = reinterpret_cast<const uint8_t *>(w.fib), *ok = reinterpret_cast<const uint8_t *>(w.crc);
  for (int i = 0; i < 12; i++) fig_walk_fib(w.st, fb + 32 * i, fig_u(ok[i]) != 0, o, lane);
  fig_sync();
  fig_state_move(reinterpret_cast<uint32_t *>(f.st + s), reinterpret_cast<const uint32_t *>(&w.st), lane);
}

// grid = n_streams, 64 threads, front-end stream, behind k_fic_frame and the frame's count (k_frame_tail, k_fic_advance) and in front of the
// next frame's k_fic_frame: the frame's slot of fib_out is read before anything can rewrite it, and no frame is skipped.  A stream with the
// mode off, or without a frame in this step, returns at once.  k_fig: an engine none of whose streams follows the service information;
// k_fig_si: one that has such streams -- a stream with that switch on brings its FigSiState into LDS beside FigState and writes it back.
__global__ __launch_bounds__(64) void k_fig(const StreamCtl *ctl, const uint8_t *fib_out, const uint8_t *fib_crc, int out_frames, FigDev f)
{
  __shared__ FigLds w;
  const int s = blockIdx.x, lane = threadIdx.x;
  if (!f.on[s]) return;
  if (!ctl[s].frame_ok || ctl[s].frames <= 0) return;
  fig_frame(w, nullptr, ctl, fib_out, fib_crc, out_frames, f, s, lane);
}

__global__ __launch_bounds__(64) void k_fig_si(const StreamCtl *ctl, const uint8_t *fib_out, const uint8_t *fib_crc, int out_frames, FigDev f)
{
  __shared__ FigSiLds w;
  const int s = blockIdx.x, lane = threadIdx.x;
  if (!f.on[s]) return;
  if (!ctl[s].frame_ok || ctl[s].frames <= 0) return;
  const bool si = fig_u(f.si_on[s]) != 0;
  if (si) fig_si_move(&w.si, f.si + s, lane);
  fig_frame(w.w, si ? &w.si : nullptr, ctl, fib_out, fib_crc, out_frames, f, s, lane);
  if (si) fig_si_move(f.si + s, &w.si, lane);
}

int launch_fig(const EngineDev &e, const FigDev &f, hipStream_t st)
{
  if (f.si) hipLaunchKernelGGL(k_fig_si, dim3(e.n_streams), dim3(64), 0, st, e.ctl, e.fib_out, e.fib_crc, e.out_frames, f);
  else hipLaunchKernelGGL(k_fig, dim3(e.n_streams), dim3(64), 0, st, e.ctl, e.fib_out, e.fib_crc, e.out_frames, f);
  DABX_HIP(hipGetLastError());
  return 0;
}

// grid = n decoders, 64 threads: decoder d walks fibs[d][n_fibs][32] with crc_ok[d][n_fibs] from the state st[d]
__device__ __forceinline__ void fig_batch(FigLds &w, FigSiState *si, const uint8_t *fibs, const uint8_t *crc_ok, int n_fibs, FigState *st, dabx_fig_label *labels,
                                 dabx_fig_event *ring, int d, int lane)
{
  fig_state_move(reinterpret_cast<uint32_t *>(&w.st), reinterpret_cast<const uint32_t *>(st + d), lane);
  const FigOut o{labels + (size_t)d * FIG_LAB_SLOTS, ring + (size_t)d * FIG_RING, si};
  const uint8_t *fb = reinterpret_cast<const uint8_t *>(w.fib);
  for (int i = 0; i < n_fibs; i++) {
    const size_t k = (size_t)d * n_fibs + i;
    if (lane < 8) w.fib[lane] = reinterpret_cast<const uint32_t *>(fibs + k * 32)[lane];
    fig_sync();
    fig_walk_fib(w.st, fb, fig_u(crc_ok[k]) != 0, o, lane);
    fig_sync();
  }
  fig_state_move(reinterpret_cast<uint32_t *>(st + d), reinterpret_cast<const uint32_t *>(&w.st), lane);
}

__global__ __launch_bounds__(64) void k_fig_batch(const uint8_t *fibs, const uint8_t *crc_ok, int n_fibs, FigState *st, dabx_fig_label *labels, dabx_fig_event *ring)
{
  __shared__ FigLds w;
  fig_batch(w, nullptr, fibs, crc_ok, n_fibs, st, labels, ring, blockIdx.x, threadIdx.x);
}

__global__ __launch_bounds__(64) void k_fig_si_batch(const uint8_t *fibs, const uint8_t *crc_ok, int n_fibs, FigState *st, FigSiState *si, dabx_fig_label *labels,
                                                     dabx_fig_event *ring)
{
  __shared__ FigSiLds w;
  const int d = blockIdx.x, lane = threadIdx.x;
  fig_si_move(&w.si, si + d, lane);
  fig_batch(w.w, &w.si, fibs, crc_ok, n_fibs, st, labels, ring, d, lane);
  fig_si_move(si + d, &w.si, lane);
}

int launch_fig_batch(const uint8_t *fibs, const uint8_t *crc_ok, int n_decoders, int n_fibs, FigState *st, FigSiState *si, dabx_fig_label *labels,
                     dabx_fig_event *ring, hipStream_t stream)
{
  if (si) hipLaunchKernelGGL(k_fig_si_batch, dim3(n_decoders), dim3(64), 0, stream, fibs, crc_ok, n_fibs, st, si, labels, ring);
  else hipLaunchKernelGGL(k_fig_batch, dim3(n_decoders), dim3(64), 0, stream, fibs, crc_ok, n_fibs, st, labels, ring);
  DABX_HIP(hipGetLastError());
  return 0;
}

// ---- the service directory (include/dabx.h, dabx_fig_directory): grid = decoders, one wave each, one lane per service component of the chosen
// configuration, 64 at a step.  Block b joins decoder first + b (fig_dir_record) into out[b * out_stride ...], at most max_per records, and
// leaves the number of components in n_out[b * n_stride].  on (optional): a decoder without service information has none. ----
__global__ __launch_bounds__(64) void k_fig_directory(const FigState *st, const FigSiState *si, const dabx_fig_label *labels, const int32_t *on, int first, int next,
                                                      dabx_fig_service *out, long long out_stride, int max_per, int32_t *n_out, int n_stride)
{
  const int b = blockIdx.x, s = first + b, lane = threadIdx.x;
  int n = 0;
  if (!on || on[s]) {
    const FigState &t = st[s];
    n = t.cfg[next ? t.cur ^ 1 : t.cur].n_comp;
    if (n > FIG_MAX_COMP) n = FIG_MAX_COMP;                  // (a state the walk wrote never has more)
    const int m = n < max_per ? n : max_per;
    for (int i = lane; i < m; i += 64) fig_dir_record(t, si[s], labels + (size_t)s * FIG_LAB_SLOTS, next, i, out + (size_t)b * out_stride + i);
  }
  if (lane == 0) n_out[(size_t)b * n_stride] = n;
}

int launch_fig_directory(const FigState *st, const FigSiState *si, const dabx_fig_label *labels, const int32_t *on, int first, int n, int next,
                         dabx_fig_service *out, long long out_stride, int max_per, int32_t *n_out, int n_stride, hipStream_t stream)
{
  hipLaunchKernelGGL(k_fig_directory, dim3(n), dim3(64), 0, stream, st, si, labels, on, first, next, out, out_stride, max_per, n_out, n_stride);
  DABX_HIP(hipGetLastError());
  return 0;
}

}  // namespace dabx
