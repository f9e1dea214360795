// iqfile.hip -- IQ payload bytes -> a stream's ring (or a linear cf32 buffer) on the GPU: HBM-bound byte work, one sample at a time per thread.
// Every entry point that stores samples comes through here (pushes, bulk ingest, file feed, dabx_convert_iq_bytes):
//   put_sample    container bytes -> cf32, or the codes as they are into a native ring (raw_reader.cpp:66-70,155-158; libsndfile
//                 sf_readf_float rules for wav_reader.cpp:164; xml_reader.cpp:254-398)
//   write_job     n samples of one payload into a ring / a work row / a linear buffer   (k_iq_write, k_iq_write_tab)
//   resample_job  linear interpolation of 1-ms blocks to 2048 samples (wav_reader.cpp:190-206, xml_reader.cpp:237-244)
//                                                                                        (k_iq_resample, k_iq_resample_tab)
#include "dabx_internal.h"
#include "iqfile.h"
#include "ring_fmt.h"
#include <algorithm>

namespace dabx {

__device__ __forceinline__ uint32_t ld_be(const uint8_t *p, int n)
{
  uint32_t v = 0;
  for (int i = 0; i < n; i++) v = (v << 8) | p[i];
  return v;
}
__device__ __forceinline__ uint32_t ld_le(const uint8_t *p, int n)
{
  uint32_t v = 0;
  for (int i = n - 1; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}
// The two channels' codes of the sample at p, first channel in a.  A payload starts on a sample boundary of an allocation (IqJob::src_off),
// so a sample of 2, 4 or 8 bytes is aligned to its size: the little-endian ones are ONE load
__device__ __forceinline__ void ld_codes(const uint8_t *p, const IqDecode &d, uint32_t &a, uint32_t &b)
{
  if (d.bytes == 1) { const uint32_t v = *reinterpret_cast<const uint16_t *>(p); a = v & 0xFFu; b = v >> 8; }
  else if (d.bytes == 2 && !d.big_endian) { const uint32_t v = *reinterpret_cast<const uint32_t *>(p); a = v & 0xFFFFu; b = v >> 16; }
  else if (d.bytes == 4 && !d.big_endian) { const uint2 v = *reinterpret_cast<const uint2 *>(p); a = v.x; b = v.y; }
  else if (d.big_endian) { a = ld_be(p, d.bytes); b = ld_be(p + d.bytes, d.bytes); }
  else { a = ld_le(p, d.bytes); b = ld_le(p + d.bytes, d.bytes); }
}

__device__ __forceinline__ float decode_one(uint32_t c, const IqDecode &d)
{
  switch (d.container) {
  case DABX_C_U8:
    return d.family == DABX_FAMILY_WAV ? __fmul_rn((float)((int)c - 128), 1.0f / 128.0f)             // pcm.c uc2f: (x - 128) / 0x80
                                       : __fdiv_rn(__fsub_rn((float)c, 127.38f), 128.0f);            // raw_reader.cpp:69, xml_reader.cpp:85
  case DABX_C_S8:
    return d.family == DABX_FAMILY_UFF ? __fdiv_rn((float)(int8_t)c, 127.0f)                         // xml_reader.cpp:266
                                       : __fmul_rn((float)(int8_t)c, 1.0f / 128.0f);
  case DABX_C_I16:
    return __fmul_rn((float)(int16_t)c, d.int_scale);                                                // x / 2^15 or x / 2^(Bits-1): exact
  case DABX_C_I24: {
    int32_t v = (int32_t)c;
    if (v & 0x800000) v |= (int32_t)0xFF000000;
    return __fmul_rn((float)v, d.int_scale);
  }
  case DABX_C_I32:
    return __fmul_rn((float)(int32_t)c, d.int_scale);
  default:
    return __uint_as_float(c);
  }
}

// THE place where sample i of a payload (that starts at src -- on a read block, for the quirk mode) becomes element o of a destination:
// a float2, the decoded value, where d.ring_fmt is RING_CF32; in a native ring (admitted by iq_native_ring: uint8 pairs of the 127.38 map,
// or 16-bit int16 pairs) the codes as the ring keeps them -- I in the low half, Q in the high half, int16 in machine byte order
__device__ __forceinline__ void put_sample(const uint8_t *src, const IqDecode &d, size_t i, void *dst, size_t o)
{
  uint32_t ca, cb;
  float a, b;
  if (d.quirk_i24) {
    // the reference's int24 / MSB loops, literally (xml_reader.cpp:312-325 IQ, :458-472 QI): `src` starts on a read block
    const size_t c = i / (size_t)d.quirk_block, ii = i - c * (size_t)d.quirk_block;
    const uint8_t *lbuf = src + c * (size_t)d.quirk_block * 6;
    int32_t t1 = (int32_t)((lbuf[6 * ii] << 16) | (lbuf[6 * ii + 1] << 8) | lbuf[6 * ii + 2]);
    int32_t t2 = (int32_t)((lbuf[6 * ii + 3] << 16) | (lbuf[4 * ii + 4] << 8) | lbuf[6 * ii + 5]);
    const int32_t ext = d.quirk_sign7f ? (int32_t)0x7F000000 : (int32_t)0xFF000000;
    if (t1 & 0x800000) t1 |= ext;
    if (t2 & 0x800000) t2 |= ext;
    a = __fmul_rn((float)t1, d.int_scale); b = __fmul_rn((float)t2, d.int_scale);
  } else {
    ld_codes(src + i * (size_t)(2 * d.bytes), d, ca, cb);
    if (d.ring_fmt != RING_CF32) {
      if (d.swap_iq) { const uint32_t t = ca; ca = cb; cb = t; }
      if (d.ring_fmt == RING_U8) reinterpret_cast<uint16_t *>(dst)[o] = (uint16_t)(ca | (cb << 8));
      else reinterpret_cast<uint32_t *>(dst)[o] = ca | (cb << 16);
      return;
    }
    a = decode_one(ca, d); b = decode_one(cb, d);
  }
  if (d.swap_iq) { const float t = a; a = b; b = t; }
  reinterpret_cast<float2 *>(dst)[o] = make_float2(a, b);
}

// n samples from src through put_sample to dst[(dst0 + i) % dst_len] (dst_len 0: dst[dst0 + i]), this thread's share
__device__ __forceinline__ void write_run(const uint8_t *src, const IqDecode &d, size_t n, void *dst, unsigned long long dst0, int dst_len)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t0; i < n; i += stride)
    put_sample(src, d, i, dst, dst_len ? (size_t)((dst0 + i) % (unsigned long long)dst_len) : (size_t)(dst0 + i));
}
// ... with what put_sample tests per sample known before the loop: the plain little-endian layouts, the three push formats among them
// (measured on 1-GB uint8 slabs: 2.6 ms per slab with the tests inside the loop, docs/history/iq_write_path.md)
template <int CONTAINER, int BYTES, int RING>
__device__ __forceinline__ void write_run_as(const uint8_t *src, IqDecode d, size_t n, void *dst, unsigned long long dst0, int dst_len)
{
  d.family = CONTAINER == DABX_C_U8 ? DABX_FAMILY_RAW : d.family;      // (uint8: chosen for the 127.38 map only; the others do not look at it)
  d.container = CONTAINER; d.bytes = BYTES; d.ring_fmt = RING; d.big_endian = d.swap_iq = d.quirk_i24 = 0;
  write_run(src, d, n, dst, dst0, dst_len);
}
__device__ __forceinline__ void write_dispatch(const uint8_t *src, const IqDecode &d, size_t n, void *dst, unsigned long long dst0, int dst_len)
{
  const bool cf32 = d.ring_fmt == RING_CF32;
  if (d.big_endian || d.swap_iq || d.quirk_i24) write_run(src, d, n, dst, dst0, dst_len);
  else if (d.container == DABX_C_U8 && d.family != DABX_FAMILY_WAV && cf32) write_run_as<DABX_C_U8, 1, RING_CF32>(src, d, n, dst, dst0, dst_len);
  else if (d.container == DABX_C_U8 && d.ring_fmt == RING_U8) write_run_as<DABX_C_U8, 1, RING_U8>(src, d, n, dst, dst0, dst_len);
  else if (d.container == DABX_C_I16 && cf32) write_run_as<DABX_C_I16, 2, RING_CF32>(src, d, n, dst, dst0, dst_len);
  else if (d.container == DABX_C_I16 && d.ring_fmt == RING_S16) write_run_as<DABX_C_I16, 2, RING_S16>(src, d, n, dst, dst0, dst_len);
  else if (d.container == DABX_C_F32 && cf32) write_run_as<DABX_C_F32, 4, RING_CF32>(src, d, n, dst, dst0, dst_len);
  else write_run(src, d, n, dst, dst0, dst_len);
}

// n samples of job j, stream s: straight into the destination (2.048 MS/s), or -- cf32, linear -- behind the carried samples in the work row
__device__ __forceinline__ void write_job(const IqIo &io, const IqJob &j, int s)
{
  if (j.n == 0) return;
  const uint8_t *src = io.src + j.src_off;
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j.M) {                                                 // (never into a native ring: refused where the feed / the ingest was opened)
    float2 *work = io.work + (size_t)s * io.work_pitch;
    for (size_t i = t0; i < j.carry_n; i += stride) work[i] = io.carry[(size_t)s * io.carry_pitch + i];
    write_dispatch(src, j.dec, j.n, work, j.carry_n, 0);
    return;
  }
  write_dispatch(src, j.dec, j.n, static_cast<char *>(io.dst) + (size_t)s * io.dst_len * ring_bytes_per_sample(j.dec.ring_fmt), j.dst0, io.dst_len);
}
// A resampling job: the 1-ms blocks of V = [carry | decoded] -> 2048 samples each, and what is left over -> the carry row for the next job.
// Block c, output q: conv = V + c M ; out = conv[base_q + 1] * frac_q + conv[base_q] * (1 - frac_q)
__device__ __forceinline__ void resample_job(const IqIo &io, const IqJob &j, int s)
{
  if (j.n == 0 || j.M == 0) return;
  const float2 *V = io.work + (size_t)s * io.work_pitch;
  float2 *dst = static_cast<float2 *>(io.dst) + (size_t)s * io.dst_len;
  const int16_t *ti = io.tab_int + (size_t)j.tab * 2048;
  const float *tf = io.tab_frac + (size_t)j.tab * 2048;
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n_out = (size_t)j.blocks * 2048;
  for (size_t n = t0; n < n_out; n += stride) {
    const size_t c = n >> 11;
    const int q = (int)(n & 2047), base = ti[q];
    const float r = tf[q], w = __fsub_rn(1.0f, r);
    const float2 lo = V[c * (size_t)j.M + base], hi = V[c * (size_t)j.M + base + 1];
    dst[io.dst_len ? (size_t)((j.dst0 + n) % (unsigned long long)io.dst_len) : (size_t)(j.dst0 + n)] =
        make_float2(__fadd_rn(__fmul_rn(hi.x, r), __fmul_rn(lo.x, w)), __fadd_rn(__fmul_rn(hi.y, r), __fmul_rn(lo.y, w)));
  }
  for (size_t i = t0; i < j.keep; i += stride) io.carry[(size_t)s * io.carry_pitch + i] = V[(size_t)j.blocks * j.M + i];
}

// The job arrives by value (one stream), or from a table with blockIdx.y = stream (a slab)
__global__ __launch_bounds__(256) void k_iq_write(IqIo io, IqJob j) { write_job(io, j, 0); }
__global__ __launch_bounds__(256) void k_iq_resample(IqIo io, IqJob j) { resample_job(io, j, 0); }
__global__ __launch_bounds__(256) void k_iq_write_tab(IqIo io, const IqJob *jobs) { const IqJob j = jobs[blockIdx.y]; write_job(io, j, blockIdx.y); }
__global__ __launch_bounds__(256) void k_iq_resample_tab(IqIo io, const IqJob *jobs) { const IqJob j = jobs[blockIdx.y]; resample_job(io, j, blockIdx.y); }

__global__ void k_commit_counts(unsigned long long *wr, const unsigned *counts, int n_streams)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n_streams) wr[s] += counts[s];
}

// Blocks per stream: about 16 K in all (64 per CU), so that a wave's start and the job's decode are spread over many samples of a big slab
// (uint8, 512 streams x 5 frames: 2.2 ms with 2048 blocks per stream); the bodies stride over what a grid does not cover
static unsigned grid_x(unsigned n, int n_streams) { return std::min<unsigned>((std::max(n, 1u) + 255) / 256, std::max(16384u / (unsigned)n_streams, 16u)); }

int launch_iq_job(const IqIo &io, const IqJob &j, hipStream_t st)
{
  if (j.n == 0) return 0;
  hipLaunchKernelGGL(k_iq_write, dim3(grid_x(j.n, 1)), dim3(256), 0, st, io, j);
  if (j.M) hipLaunchKernelGGL(k_iq_resample, dim3(grid_x(j.blocks * 2048, 1)), dim3(256), 0, st, io, j);
  DABX_HIP(hipGetLastError());
  return 0;
}
int launch_iq_jobs(const IqIo &io, const IqJob *jobs_dev, int n_streams, unsigned max_n, unsigned max_out, bool resamples, hipStream_t st)
{
  if (max_n == 0) return 0;
  hipLaunchKernelGGL(k_iq_write_tab, dim3(grid_x(max_n, n_streams), n_streams), dim3(256), 0, st, io, jobs_dev);
  // (also where no stream completes a block: the leftover samples are saved whenever there are any)
  if (resamples) hipLaunchKernelGGL(k_iq_resample_tab, dim3(grid_x(max_out, n_streams), n_streams), dim3(256), 0, st, io, jobs_dev);
  DABX_HIP(hipGetLastError());
  return 0;
}
int launch_commit_counts(unsigned long long *wr, const unsigned *counts_dev, int n_streams, hipStream_t st)
{
  hipLaunchKernelGGL(k_commit_counts, dim3((n_streams + 255) / 256), dim3(256), 0, st, wr, counts_dev, n_streams);
  DABX_HIP(hipGetLastError());
  return 0;
}

}  // namespace dabx
