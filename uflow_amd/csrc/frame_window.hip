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

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "frame_window.hpp"
#include "scan.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::FwArgs;

// One-wave workgroups: four waves per workgroup measured the same (0.292 against 0.302 ms on the small grouping).
constexpr uint32_t kFwBlocksMax = 1u << 16;  // the walks stride over the connections beyond
static_assert(sizeof(ufc_frame_window) == 24 && sizeof(ufc_frame_window_result) == 40, "record layouts");

// One wave per connection.  kWrite = false: the group counts (and the zero behind the last); true: the outputs.
template <bool kWrite>
__global__ __launch_bounds__(64) void fw_walk_kernel(FwArgs a, uint64_t* counts) {
  __shared__ ufc_codec::FwWaveShared sh;
  for (uint64_t r = blockIdx.x; r < a.n_windows; r += gridDim.x) {
    const uint64_t gfirst = kWrite ? a.group_first[r] : 0;
    const uint64_t count = ufc_codec::fw_walk_tiles(DevWave{}, sh, a, r, kWrite, gfirst);
    if (!kWrite && threadIdx.x == 0) counts[r] = count;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (kWrite) *a.groups_used = a.group_first[a.n_windows];
    else counts[a.n_windows] = 0;
  }
}

}  // namespace

hipError_t window_batch(const FwArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  ScratchPlan plan;  // a group count per connection (+ 1 entry), the scan's temporaries
  const uint64_t at_counts = plan.take((a.n_windows + 1) * 8);
  const size_t temp_bytes = scan_temp_bytes<uint64_t>(a.n_windows + 1);
  const uint64_t at_temp = plan.take(temp_bytes);
  char* sc;
  hipError_t e;
  if ((e = scratch.get(plan.end, &sc)) != hipSuccess) return e;
  uint64_t* counts = (uint64_t*)(sc + at_counts);
  const unsigned blocks = (unsigned)std::min<uint64_t>(a.n_windows, kFwBlocksMax);
  fw_walk_kernel<false><<<blocks, 64, 0, stream>>>(a, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(sc + at_temp, temp_bytes, counts, a.group_first, a.n_windows + 1, stream)) != hipSuccess) return e;
  fw_walk_kernel<true><<<blocks, 64, 0, stream>>>(a, counts);
  return hipGetLastError();
}

}  // namespace ufc_dev
