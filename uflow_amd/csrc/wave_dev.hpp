// wave_dev.hpp -- the device side of wave.hpp, for .hip files only: the wave barrier, the wave policy that gives
// every hardware lane one lane of a phase, and the kernel-argument segment read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ufc_dev {

// The lanes of one wave meet: what each wrote (to LDS or to memory) before is what the others read after.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave policy of the core's steps on the device, one wave per connection: every lane runs each phase, a wave
// barrier in between.  (A member a step does not use is never instantiated.)
struct DevWave {
  static __device__ __forceinline__ void sync() { wave_sync(); }
  template <class F>
  __device__ __forceinline__ void lanes(const F& f) const {
    f(threadIdx.x & 63u);
    wave_sync();
  }
  template <class F>
  __device__ __forceinline__ void one(const F& f) const {
    if ((threadIdx.x & 63u) == 0) f();
  }
  template <class F>
  __device__ __forceinline__ unsigned long long ballot(const F& f) const {
    const unsigned long long m = __ballot(f(threadIdx.x & 63u) ? 1 : 0);
    wave_sync();
    return m;
  }
  template <class F>
  __device__ __forceinline__ uint64_t sum(const F& f) const {
    unsigned long long v = f(threadIdx.x & 63u);
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    wave_sync();
    return v;
  }
  static __device__ __forceinline__ void or64(unsigned long long* p, unsigned long long v) { atomicOr(p, v); }
  static __device__ __forceinline__ void add64(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
};

// A kernel's one by-value argument, read where it is needed from the kernel-argument segment (it lies at the
// segment's start) instead of being held in scalar registers for the whole step: with the frame queue's 17
// arguments held in 34 of them the compiler spilled 21 scalar registers.  The kernel declares the parameter
// unnamed and takes `const Args& a = kernargs<Args>();`.
template <class Args>
__device__ __forceinline__ const Args& kernargs() {
  typedef const Args __attribute__((address_space(4))) * KernArgs;
  return *(const Args*)(KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
}

}  // namespace ufc_dev
