// ring_fmt.h -- the element of the IQ ring, and the ONE place where it becomes a float2 (include/dabx.h, DABX_RING_*).
//
// A cf32 ring holds what the reference's file devices hand to SampleReader: floats.  A native ring holds what they READ -- the
// recording's own codes -- and the device's map to float is applied where a kernel consumes a sample instead of where the ingest
// stores it:
//   S16  interleaved I, Q int16, machine byte order      value = (float)c / 32768               (wav_reader.cpp:164)
//   U8   interleaved I, Q uint8                          value = ((float)c - 127.38f) / 128     (raw_reader.cpp:66-70)
// Both maps are the expressions the writer's decode_one (iqfile.hip) uses, one convert, (one subtract) and one division by a power of two per
// component: every code has exactly one float, on the device and on the host alike (-fno-fast-math -ffp-contract=off), so a native
// ring changes no bit downstream.  An element is ONE integer register -- I in the low half, Q in the high half -- loaded with its
// own alignment (4 / 2 bytes) and nothing wider: frames start on any sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dabx {

constexpr int RING_CF32 = 0, RING_S16 = 1, RING_U8 = 2;   // = DABX_RING_*, = dabx_push_iq's fmt
__host__ __device__ constexpr int ring_bytes_per_sample(int ring_fmt) { return ring_fmt == RING_S16 ? 4 : (ring_fmt == RING_U8 ? 2 : 8); }

template <int RF> struct RingFmt;
template <> struct RingFmt<RING_CF32> {
  typedef float2 Elem;
  static __host__ __device__ __forceinline__ float2 cvt(Elem c) { return c; }
  static __host__ __device__ __forceinline__ Elem filler() { return make_float2(0.f, 0.f); }
};
template <> struct RingFmt<RING_S16> {
  typedef uint32_t Elem;
  static __host__ __device__ __forceinline__ float2 cvt(Elem c)
  {
    return make_float2((float)(int16_t)(c & 0xFFFFu) / 32768.0f, (float)(int16_t)(c >> 16) / 32768.0f);
  }
  static __host__ __device__ __forceinline__ Elem filler() { return 0u; }
};
template <> struct RingFmt<RING_U8> {
  typedef uint16_t Elem;
  static __host__ __device__ __forceinline__ float2 cvt(Elem c)
  {
    return make_float2(((float)(uint8_t)(c & 0xFFu) - 127.38f) / 128.0f, ((float)(uint8_t)(c >> 8) - 127.38f) / 128.0f);
  }
  static __host__ __device__ __forceinline__ Elem filler() { return 0u; }
};
// (filler: what a prefetch register holds for a sample that is not there.  Only the cf32 filler IS the value zero; a kernel that
//  needs a zero sample in a native ring keeps a validity bit next to the code -- pipeline.hip, ring_value.)

}  // namespace dabx
