// wave.hpp -- what the batched steps of frame_codec_core.hpp ask of a "wave policy" Wv, as host and device code:
// the serial policy (a phase is a loop over the 64 lanes) and the 64-bit lane-mask helpers.  The device's own
// policy, a lane per hardware lane with a wave barrier between the phases, is wave_dev.hpp (.hip files only).
//   Wv::lanes(f)       f(lane) for the 64 lanes; what the lanes wrote before is visible to all after
//   Wv::one(f)         f() once
//   Wv::ballot(f)      the 64-bit mask of the lanes for which f(lane) is true, the same in every lane
//   Wv::sum(f)         the sum of f(lane) over the 64 lanes, the same in every lane
//   Wv::sync()         what Wv::one wrote is visible to every lane after it
//   Wv::or64 / add64   atomic on the device (vector atomics on LDS), plain here
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ufc_codec {

// The lanes 0..63 one after the other: the host entries (frame_codec.cpp), the host checks under tests/c, and on
// the device the lane-per-connection form of the resend kernels (resend.hip), where a phase is a loop in the lane.
struct SerialWave {
  template <class F>
  __host__ __device__ __forceinline__ void lanes(const F& f) const {
    for (uint32_t l = 0; l < 64; l++) f(l);
  }
  template <class F>
  __host__ __device__ __forceinline__ void one(const F& f) const {
    f();
  }
  template <class F>
  __host__ __device__ __forceinline__ unsigned long long ballot(const F& f) const {
    unsigned long long m = 0;
    for (uint32_t l = 0; l < 64; l++)
      if (f(l)) m |= 1ull << l;
    return m;
  }
  template <class F>
  __host__ __device__ __forceinline__ uint64_t sum(const F& f) const {
    uint64_t v = 0;
    for (uint32_t l = 0; l < 64; l++) v += f(l);
    return v;
  }
  __host__ __device__ __forceinline__ void sync() const {}
  static __host__ __device__ __forceinline__ void or64(unsigned long long* p, unsigned long long v) { *p |= v; }
  static __host__ __device__ __forceinline__ void add64(unsigned long long* p, unsigned long long v) { *p += v; }
};

// Bit positions in a lane mask.  high_bit and low_bit want m != 0 (the count of leading or trailing zeros of 0 is
// undefined): every caller tests its mask first.
__host__ __device__ __forceinline__ uint32_t high_bit(unsigned long long m) { return 63u - (uint32_t)__builtin_clzll(m); }
__host__ __device__ __forceinline__ uint32_t low_bit(unsigned long long m) { return (uint32_t)__builtin_ctzll(m); }
__host__ __device__ __forceinline__ uint32_t popc(unsigned long long m) { return (uint32_t)__builtin_popcountll(m); }

}  // namespace ufc_codec
