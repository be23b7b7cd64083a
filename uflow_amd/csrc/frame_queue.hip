// frame_queue.hip -- batched FrameQueue step on device-resident records: many connections' parsed ack frames
// turned into acked-fragment marks, the transfer window and the rate control's feedback in one call
// (ufc_frame_queue_varlen, include/uflow_frame_codec.h), the sender's step behind frame_parse.hip.
//
// The step's code is frame_codec_core.hpp's fq_step, shared with the host (where a phase is a loop over the
// lanes).  One wave runs a connection: the running state (ids, reorder buffer, pending ack data) is the same in
// every lane, the loss intervals sit in LDS and are touched by lane 0 alone, and everything that reads or writes a
// run of log entries takes a lane per entry: the <= 32 entries of a group, the nack runs and the expiry cutoff in
// tiles of 64 with wave ballots, the pushes as a copy of 64 records per phase.  No lane ever walks log entries
// alone.  No output needs a scan, so one launch does the call and no scratch is used; past the launch grid the
// waves stride over the connections.  The file is compiled without fast-math, and the core keeps the loss rate's
// sums unfused (fp contract off), so every float equals the host's in every bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "frame_queue.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::FqArgs;

constexpr uint32_t kFqBlocksMax = 1u << 16;  // the waves stride over the connections beyond
static_assert(sizeof(ufc_sent_frame) == 24 && sizeof(ufc_frame_queue) == 192 && sizeof(ufc_frame_queue_step) == 40 &&
                  sizeof(ufc_frame_queue_result) == 80,
              "record layouts");

// The wave policy of fq_step on the device: every lane runs each phase, a wave barrier in between.
struct FqDevWave {
  static __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  template <class F>
  __device__ __forceinline__ void lanes(const F& f) const {
    f(threadIdx.x & 63u);
    sync();
  }
  template <class F>
  __device__ __forceinline__ void one(const F& f) const {
    if ((threadIdx.x & 63u) == 0) f();
  }
  template <class F>
  __device__ __forceinline__ unsigned long long ballot(const F& f) const {
    const unsigned long long m = __ballot(f(threadIdx.x & 63u) ? 1 : 0);
    sync();
    return m;
  }
};

// One wave per connection.  The 17 arguments are read where they are needed, from the kernel-argument segment (the
// one by-value argument lies at its start), not held in 34 scalar registers for the whole step: with them held the
// compiler spilled 21 scalar registers.
__global__ __launch_bounds__(64) void fq_step_kernel(FqArgs) {
  __shared__ ufc_codec::FqWaveShared sh;
  typedef const FqArgs __attribute__((address_space(4))) * KernArgs;
  const FqArgs& a = *(const FqArgs*)(KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  for (uint64_t c = blockIdx.x; c < a.n_queues; c += gridDim.x) ufc_codec::fq_step(FqDevWave{}, sh, a, c);
}

}  // namespace

hipError_t queue_batch(const FqArgs& a, hipStream_t stream) {
  const unsigned blocks = (unsigned)std::min<uint64_t>(a.n_queues, kFqBlocksMax);
  fq_step_kernel<<<blocks, 64, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace ufc_dev
