// flush_ctl.hip -- batched flush control on device-resident records: the ack flush with its dud frame and its
// carry, and the sync frame's decision, for many connections in one call each (ufc_flush_acks_varlen,
// ufc_flush_sync_varlen, include/uflow_flush_ctl.h): the glue of HalfConnection::flush between the frame window
// and the resend calls, and behind the data flush.
//
// The steps are frame_codec_core.hpp's fa_plan / fa_write and fs_decide_tile / fs_write_tile, shared with the host
// (where a phase is a loop over the lanes).  Launches of the ack flush:
//   1. count: a lane per connection -> its merged group count and its frame count (a loop over frames: every group
//      is 9 bytes, a full frame 161 of them); nothing the caller sees is written but merged_first;
//   2. two exclusive sums over the n + 1 counts -> merged_first, and the frames' firsts in scratch;
//   3. write: a wave per connection, a lane per group (the shape of rs_place_kernel, for its reason: with a group
//      or two a connection, a lane per group over the whole batch would search the CSR for its connection) -> the
//      merged groups through LDS, the new carry, the frame records, the results and the states.
// Only launch 3 writes what launch 1 reads, so windows_out and ctl_out may be the inputs and the carry rooms are
// updated in place.  Launches of the sync decision:
//   1. decide: a lane per connection in tiles of 64 -> results, ctl_out, alloc_adjust; the tile's ballot count;
//   2. an exclusive sum over the tiles' counts;
//   3. write: the same tiles -> sync_index and the frames' records, compacted in connection order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "flush_ctl.hpp"
#include "frame_codec_core.hpp"
#include "scan.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::FaArgs;
using ufc_codec::FsArgs;

constexpr uint32_t kFcBlocksMax = 1u << 16;   // wave per connection: the waves stride over the connections beyond
constexpr uint32_t kFcLaneBlocksMax = 4096;   // lane per connection: 262,144 lanes, striding beyond (as send_rate.hip)
static_assert(sizeof(ufc_flush_ctl) == 40 && sizeof(ufc_flush_acks_result) == 24 && sizeof(ufc_flush_sync_result) == 24,
              "record layouts");

// The arguments are read from the kernel-argument segment (wave_dev.hpp), as the resend kernels read theirs.
__global__ __launch_bounds__(64) void fa_count_kernel(FaArgs, uint64_t* frame_counts) {
  const FaArgs& a = kernargs<FaArgs>();
  for (uint64_t c = (uint64_t)blockIdx.x * 64 + threadIdx.x; c < a.n; c += (uint64_t)gridDim.x * 64) {
    const ufc_codec::FaPlan p = ufc_codec::fa_plan(a, c);
    a.merged_first[c] = p.merged;
    frame_counts[c] = p.frames;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.merged_first[a.n] = 0;
    frame_counts[a.n] = 0;
  }
}

__global__ __launch_bounds__(64) void fa_write_kernel(FaArgs, const uint64_t* frame_first) {
  __shared__ ufc_codec::FaWaveShared sh;
  const FaArgs& a = kernargs<FaArgs>();
  for (uint64_t c = blockIdx.x; c < a.n; c += gridDim.x) ufc_codec::fa_write(DevWave{}, sh, a, c, frame_first[c]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *a.merged_used = a.merged_first[a.n];
    *a.frames_used = frame_first[a.n];
  }
}

__global__ __launch_bounds__(64) void fs_decide_kernel(FsArgs, uint64_t* tile_counts, uint64_t n_tiles) {
  const FsArgs& a = kernargs<FsArgs>();
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t count = ufc_codec::fs_decide_tile(DevWave{}, a, t);
    if (threadIdx.x == 0) tile_counts[t] = count;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_counts[n_tiles] = 0;
}

__global__ __launch_bounds__(64) void fs_write_kernel(FsArgs, const uint64_t* tile_first, uint64_t n_tiles) {
  const FsArgs& a = kernargs<FsArgs>();
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) ufc_codec::fs_write_tile(DevWave{}, a, t, tile_first[t]);
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.syncs_used = tile_first[n_tiles];
}

}  // namespace

hipError_t flush_acks_batch(const FaArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  ScratchPlan plan;  // a frame count per connection (+ 1 entry), the scan's temporaries
  const uint64_t at_counts = plan.take((a.n + 1) * 8);
  const size_t temp_bytes = scan_temp_bytes<uint64_t>(a.n + 1);
  const uint64_t at_temp = plan.take(temp_bytes);
  char* sc;
  hipError_t e;
  if ((e = scratch.get(plan.end, &sc)) != hipSuccess) return e;
  uint64_t* counts = (uint64_t*)(sc + at_counts);
  fa_count_kernel<<<(unsigned)std::min<uint64_t>((a.n + 63) / 64, kFcLaneBlocksMax), 64, 0, stream>>>(a, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(sc + at_temp, temp_bytes, a.merged_first, a.merged_first, a.n + 1, stream)) != hipSuccess ||
      (e = exclusive_sum(sc + at_temp, temp_bytes, counts, counts, a.n + 1, stream)) != hipSuccess)
    return e;
  fa_write_kernel<<<(unsigned)std::min<uint64_t>(a.n, kFcBlocksMax), 64, 0, stream>>>(a, counts);
  return hipGetLastError();
}

hipError_t flush_sync_batch(const FsArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  const uint64_t n_tiles = (a.n + 63) / 64;
  ScratchPlan plan;  // a count per tile (+ 1 entry), the scan's temporaries
  const uint64_t at_counts = plan.take((n_tiles + 1) * 8);
  const size_t temp_bytes = scan_temp_bytes<uint64_t>(n_tiles + 1);
  const uint64_t at_temp = plan.take(temp_bytes);
  char* sc;
  hipError_t e;
  if ((e = scratch.get(plan.end, &sc)) != hipSuccess) return e;
  uint64_t* counts = (uint64_t*)(sc + at_counts);
  const unsigned blocks = (unsigned)std::min<uint64_t>(n_tiles, kFcLaneBlocksMax);
  fs_decide_kernel<<<blocks, 64, 0, stream>>>(a, counts, n_tiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(sc + at_temp, temp_bytes, counts, counts, n_tiles + 1, stream)) != hipSuccess) return e;
  fs_write_kernel<<<blocks, 64, 0, stream>>>(a, counts, n_tiles);
  return hipGetLastError();
}

}  // namespace ufc_dev
