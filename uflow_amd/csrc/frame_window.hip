// frame_window.hip -- batched FrameAckQueue step on device-resident records: many connections' parsed frames
// judged against their frame windows and marked into ack groups in one call (ufc_frame_window_varlen,
// include/uflow_frame_codec.h), the step between frame_parse.hip and packet_receive.hip, and the source of the
// ack flushes frame_pack.hip cuts into frames.
//
// The step's code is frame_codec_core.hpp's fw_walk_tiles, shared with the host (where a phase is a loop over the
// lanes).  One wave walks a connection in tiles of 64 consecutive frames, a coalesced 32-byte record per lane;
// the lanes meet in 64-bit lane masks in LDS.  The order dependence of the window (a frame's verdict hangs on the
// base the frames before it left) is resolved by rounds: all lanes test against the lane before them, the first
// failing lane is final and drops out, the rest test again; ordinary traffic takes one round per tile.  The
// groups take a round per group the tile touches.  No lane ever walks a connection's frames alone.  Launches:
//   1. count: one wave per connection -> its group count (nothing else is written);
//   2. an exclusive sum over the n_windows + 1 counts -> group_first;
//   3. write: the same walk again, with the connection's first group index -> frame_accept, the groups, the
//      results, the state; *groups_used.
// Only step 3 writes what the caller sees, so windows_out may be windows itself.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "frame_window.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::FwArgs;

// One-wave workgroups: four waves per workgroup measured the same (0.292 against 0.302 ms on the small grouping).
constexpr uint32_t kFwBlocksMax = 1u << 16;  // the walks stride over the connections beyond
static_assert(sizeof(ufc_frame_window) == 24 && sizeof(ufc_frame_window_result) == 40, "record layouts");

// The wave policy of fw_walk_tiles on the device: every lane runs each phase, a wave barrier in between.
struct FwDevWave {
  template <class F>
  __device__ __forceinline__ void lanes(const F& f) const {
    f(threadIdx.x & 63u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  template <class F>
  __device__ __forceinline__ void one(const F& f) const {
    if ((threadIdx.x & 63u) == 0) f();
  }
  static __device__ __forceinline__ void or64(unsigned long long* p, unsigned long long v) { atomicOr(p, v); }
};

// One wave per connection.  kWrite = false: the group counts (and the zero behind the last); true: the outputs.
template <bool kWrite>
__global__ __launch_bounds__(64) void fw_walk_kernel(FwArgs a, uint64_t* counts) {
  __shared__ ufc_codec::FwWaveShared sh;
  for (uint64_t r = blockIdx.x; r < a.n_windows; r += gridDim.x) {
    const uint64_t gfirst = kWrite ? a.group_first[r] : 0;
    const uint64_t count = ufc_codec::fw_walk_tiles(FwDevWave{}, sh, a, r, kWrite, gfirst);
    if (!kWrite && threadIdx.x == 0) counts[r] = count;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (kWrite) *a.groups_used = a.group_first[a.n_windows];
    else counts[a.n_windows] = 0;
  }
}

struct FwLayout {  // scratch of a frame window call (256-byte aligned parts)
  uint64_t counts, temp, end;
  FwLayout(uint64_t n_windows, size_t temp_bytes) {
    auto up = [](uint64_t b) { return (b + 255) / 256 * 256; };
    counts = 0;
    temp = counts + up((n_windows + 1) * 8);
    end = temp + up(temp_bytes);
  }
};
size_t fw_temp_bytes(uint64_t n_windows) {
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n_windows + 1));
  return t;
}

}  // namespace

size_t window_scratch_bytes(uint64_t n_windows) { return FwLayout(n_windows, fw_temp_bytes(n_windows)).end; }

hipError_t window_batch(const FwArgs& a, void* scratch, size_t scratch_bytes, hipStream_t stream) {
  const FwLayout lay(a.n_windows, fw_temp_bytes(a.n_windows));
  if (lay.end > scratch_bytes) return hipErrorInvalidValue;
  char* sc = (char*)scratch;
  uint64_t* counts = (uint64_t*)(sc + lay.counts);
  const unsigned blocks = (unsigned)std::min<uint64_t>(a.n_windows, kFwBlocksMax);
  hipError_t e;
  fw_walk_kernel<false><<<blocks, 64, 0, stream>>>(a, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t temp_bytes = lay.end - lay.temp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(sc + lay.temp, temp_bytes, counts, a.group_first, (int)(a.n_windows + 1), stream)) !=
      hipSuccess)
    return e;
  fw_walk_kernel<true><<<blocks, 64, 0, stream>>>(a, counts);
  return hipGetLastError();
}

}  // namespace ufc_dev
