// route.hip -- batched frame routing on device-resident records: every frame's source address to its connection,
// and the batch grouped by connection in arrival order (ufc_route_frames_varlen, include/uflow_route.h): the address
// lookup and dispatch of Server::handle_frames in front of the frame window.
//
// What a lane does for a frame is frame_codec_core.hpp's rt_lookup / rt_classify / rt_bucket, shared with the host.
// Launches:
//   1. init: a lane per connection -> results (no frames, no first control), the bucket counts zero;
//   2. lookup: a lane per frame -> route[i], the frame's kind class parked in cls[i]; a control frame takes
//      the minimum of its index into its connection's first_control, or into first_unknown_control (a minimum is
//      the same in whatever order it is taken);
//   3. classify: a lane per frame -> cls[i], the frame's bucket number as its sort key, its connection's count of
//      deferred frames (a count has no order either);
//   4. P passes of a stable least-significant-digit radix placement over 8-bit digits of the keys, P = the bytes
//      the largest key n_conns + 1 needs.  A pass is: hist (a workgroup per tile of 1024 frames counts its digits in
//      LDS and writes its column of the digit-major matrix hist[digit][tile]); an exclusive sum over the matrix, which
//      is where every (digit, tile) run starts; scatter (the same tile: 256 cursors in LDS start at the tile's
//      column; in 4 rounds of 256 frames a wave finds, by 8 ballots, the lanes that share its lane's digit, and the
//      4 waves one after the other, a barrier in between, read their digits' cursors and advance them by the digits'
//      lane counts: rank = cursor + the lanes of the same digit below).  Rounds, waves and lanes go in index order,
//      so equal keys keep their order and the placement is a function of the keys alone.  The first pass takes the
//      frame index as the payload, the last writes `order`;
//   5. count: a lane per grouped position over the placed keys -> every bucket's length from the two ends of its run
//      (counting the buckets with an atomic per frame took 1.4 ms at 2,048 connections: profiles/EXPERIMENTS.md);
//      an exclusive sum over the n_conns + 3 counts -> bucket_first;
//   6. gather: a lane per grouped position -> infos_out (two 16-byte loads and stores where both arrays are 16-byte
//      aligned, as device allocations are), src_base_out;
//   7. finish: a lane per connection -> results[c].frames, timeout_out.
// No kernel waits for another workgroup; every launch reads what earlier launches wrote.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "route.hpp"
#include "scan.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::RtArgs;

constexpr uint32_t kRtBlock = 256;
constexpr uint32_t kRtLaneBlocksMax = 1024;  // lane per frame / connection: 262,144 lanes, striding beyond
constexpr uint32_t kRtRounds = 4;
constexpr uint32_t kRtTile = kRtBlock * kRtRounds;  // frames per workgroup of a pass; a workgroup per tile (< 2^21)
static_assert(sizeof(ufc_addr) == 32 && sizeof(ufc_route_slot) == 48 && sizeof(ufc_route_result) == 16 &&
                  sizeof(ufc_frame_info) == 32,
              "record layouts");

__device__ __forceinline__ uint64_t lane_index() { return (uint64_t)blockIdx.x * kRtBlock + threadIdx.x; }
__device__ __forceinline__ uint64_t lane_stride() { return (uint64_t)gridDim.x * kRtBlock; }

__global__ __launch_bounds__(kRtBlock) void rt_init_kernel(RtArgs) {
  const RtArgs& a = kernargs<RtArgs>();
  for (uint64_t c = lane_index(); c < a.n_conns + 3; c += lane_stride()) {
    a.bucket_first[c] = 0;
    if (c < a.n_conns) a.results[c] = ufc_route_result{0, UFC_NO_PARENT, 0, 0};
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.first_unknown_control = UFC_NO_PARENT;
}

// (cls[i] holds the frame's kind class until the classify kernel, which then need not read the info again.)
__global__ __launch_bounds__(kRtBlock) void rt_lookup_kernel(RtArgs) {
  const RtArgs& a = kernargs<RtArgs>();
  for (uint64_t i = lane_index(); i < a.n; i += lane_stride()) {
    const uint32_t c = ufc_codec::rt_lookup(a.slots, a.n_slots, a.seed, a.max_probe, a.n_conns, a.addrs[i]);
    const uint32_t k = ufc_codec::rt_kind_class(a.infos[i]);
    a.route[i] = c;
    a.cls[i] = (uint8_t)k;
    if (k == 1)
      atomicMin(c == UFC_NO_PARENT ? a.first_unknown_control : &a.results[c].first_control, (uint32_t)i);
  }
}

__global__ __launch_bounds__(kRtBlock) void rt_classify_kernel(RtArgs, uint32_t* keys) {
  const RtArgs& a = kernargs<RtArgs>();
  for (uint64_t i = lane_index(); i < a.n; i += lane_stride()) {
    const uint32_t cls = ufc_codec::rt_classify(a, i, a.cls[i]);
    const uint32_t b = ufc_codec::rt_bucket(a, i, cls);
    a.cls[i] = (uint8_t)cls;
    keys[i] = b;
    if (cls == UFC_ROUTE_DEFERRED && a.route[i] != UFC_NO_PARENT) atomicAdd(&a.results[a.route[i]].deferred, 1u);
  }
}

// hist[digit * n_tiles + tile] = the tile's frames whose key has that digit at `shift`.
__global__ __launch_bounds__(kRtBlock) void rt_hist_kernel(const uint32_t* keys, uint64_t n, uint32_t shift,
                                                           uint32_t* hist, uint32_t n_tiles) {
  __shared__ uint32_t h[256];
  const uint32_t tile = blockIdx.x;
  h[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t r = 0; r < kRtRounds; r++) {
    const uint64_t i = (uint64_t)tile * kRtTile + r * kRtBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * n_tiles + tile] = h[threadIdx.x];
}

// The tile's frames to their places: `first` is the scanned matrix.  vals_in == nullptr: the payload is the frame
// index (the first pass).
__global__ __launch_bounds__(kRtBlock) void rt_scatter_kernel(const uint32_t* keys_in, const uint32_t* vals_in,
                                                              uint64_t n, uint32_t shift, const uint32_t* first,
                                                              uint32_t n_tiles, uint32_t* keys_out,
                                                              uint32_t* vals_out) {
  __shared__ uint32_t cursor[256];
  const uint32_t tile = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  cursor[threadIdx.x] = first[(uint64_t)threadIdx.x * n_tiles + tile];
  __syncthreads();
  for (uint32_t r = 0; r < kRtRounds; r++) {
    const uint64_t i = (uint64_t)tile * kRtTile + r * kRtBlock + threadIdx.x;
    const bool valid = i < n;
    const uint32_t key = valid ? keys_in[i] : 0;
    const uint32_t d = (key >> shift) & 255u;
    unsigned long long same = __ballot(valid);  // the wave's lanes that hold a frame with this lane's digit
    for (uint32_t bit = 0; bit < 8; bit++) {
      const bool set = (d >> bit) & 1u;
      const unsigned long long with = __ballot(valid && set);
      same &= set ? with : ~with;
    }
    const uint32_t below = ufc_codec::popc(same & ((1ull << lane) - 1));
    uint32_t base = 0;
    for (uint32_t w = 0; w < kRtBlock / 64; w++) {  // the waves in index order; every lane meets every barrier
      if (wave == w && valid) {
        base = cursor[d];
        wave_sync();  // the digit's lanes have all read the cursor before its first lane moves it
        if (below == 0) cursor[d] = base + ufc_codec::popc(same);
      }
      __syncthreads();
    }
    const uint64_t at = (uint64_t)base + below;
    if (valid && at < n) {  // (at < n holds when `first` is the scan of this pass's histogram)
      vals_out[at] = vals_in ? vals_in[i] : (uint32_t)i;
      keys_out[at] = key;
    }
  }
}

// The buckets' lengths from the placed keys: a bucket is a run of equal keys, its length the position behind the
// run's last frame minus the position of its first.  The two lanes that hold a run's ends add those two numbers into
// the bucket's zeroed count (wrapping 64-bit sums: the order does not matter, and an address is met twice at most).
__global__ __launch_bounds__(kRtBlock) void rt_count_kernel(const uint32_t* sorted_keys, uint64_t n,
                                                            uint64_t* counts) {
  for (uint64_t k = lane_index(); k < n; k += lane_stride()) {
    const uint32_t key = sorted_keys[k];
    const bool first = k == 0 || sorted_keys[k - 1] != key, last = k + 1 == n || sorted_keys[k + 1] != key;
    if (first && last)
      counts[key] = 1;
    else if (first)
      atomicAdd((unsigned long long*)&counts[key], 0ull - k);
    else if (last)
      atomicAdd((unsigned long long*)&counts[key], k + 1);
  }
}

template <bool Vec>
__global__ __launch_bounds__(kRtBlock) void rt_gather_kernel(RtArgs) {
  const RtArgs& a = kernargs<RtArgs>();
  for (uint64_t k = lane_index(); k < a.n; k += lane_stride()) {
    const uint32_t i = a.order[k];
    if (Vec) {
      const uint4* src = (const uint4*)&a.infos[i];
      const uint4 lo = src[0], hi = src[1];
      uint4* dst = (uint4*)&a.infos_out[k];
      dst[0] = lo;
      dst[1] = hi;
    } else {
      const uint32_t* src = (const uint32_t*)&a.infos[i];
      uint32_t* dst = (uint32_t*)&a.infos_out[k];
      for (int j = 0; j < 8; j++) dst[j] = src[j];
    }
    a.src_base_out[k] = ufc_codec::rt_src_base(a, i);
  }
}

__global__ __launch_bounds__(kRtBlock) void rt_finish_kernel(RtArgs) {
  const RtArgs& a = kernargs<RtArgs>();
  for (uint64_t c = lane_index(); c < a.n_conns; c += lane_stride()) ufc_codec::rt_finish_conn(a, c);
}

unsigned lane_blocks(uint64_t lanes) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((lanes + kRtBlock - 1) / kRtBlock, kRtLaneBlocksMax));
}

}  // namespace

uint32_t route_passes(uint64_t n_conns) {  // the bytes of the largest key, n_conns + 1
  uint32_t passes = 1;
  for (uint64_t top = (n_conns + 1) >> 8; top; top >>= 8) passes++;
  return passes;
}

hipError_t route_frames_batch(const RtArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  const uint32_t passes = route_passes(a.n_conns);
  const uint64_t n_tiles = (a.n + kRtTile - 1) / kRtTile;
  ScratchPlan plan;  // the keys; the keys and indices in flight between passes; the histograms; the scans' temporaries
  const uint64_t at_keys0 = plan.take(a.n * 4);
  const uint64_t at_keys1 = plan.take(a.n * 4);
  const uint64_t at_vals0 = plan.take(passes > 1 ? a.n * 4 : 0);
  const uint64_t at_vals1 = plan.take(passes > 1 ? a.n * 4 : 0);
  const uint64_t at_hist = plan.take(n_tiles * 256 * 4);
  const size_t hist_temp_bytes = a.n ? scan_temp_bytes<uint32_t>(n_tiles * 256) : 0;
  const uint64_t at_hist_temp = plan.take(hist_temp_bytes);
  const size_t bucket_temp_bytes = scan_temp_bytes<uint64_t>(a.n_conns + 3);
  const uint64_t at_bucket_temp = plan.take(bucket_temp_bytes);
  char* sc;
  hipError_t e;
  if ((e = scratch.get(plan.end, &sc)) != hipSuccess) return e;
  rt_init_kernel<<<lane_blocks(a.n_conns + 3), kRtBlock, 0, stream>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.n) {
    uint32_t* keys[2] = {(uint32_t*)(sc + at_keys0), (uint32_t*)(sc + at_keys1)};
    uint32_t* vals[2] = {(uint32_t*)(sc + at_vals0), (uint32_t*)(sc + at_vals1)};
    uint32_t* hist = (uint32_t*)(sc + at_hist);
    rt_lookup_kernel<<<lane_blocks(a.n), kRtBlock, 0, stream>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    rt_classify_kernel<<<lane_blocks(a.n), kRtBlock, 0, stream>>>(a, keys[0]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (uint32_t p = 0; p < passes; p++) {
      const bool last = p + 1 == passes;
      const uint32_t* keys_in = keys[p & 1];
      rt_hist_kernel<<<(unsigned)n_tiles, kRtBlock, 0, stream>>>(keys_in, a.n, 8 * p, hist, (uint32_t)n_tiles);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = exclusive_sum(sc + at_hist_temp, hist_temp_bytes, hist, hist, n_tiles * 256, stream)) != hipSuccess)
        return e;
      rt_scatter_kernel<<<(unsigned)n_tiles, kRtBlock, 0, stream>>>(
          keys_in, p ? vals[(p - 1) & 1] : nullptr, a.n, 8 * p, hist, (uint32_t)n_tiles,
          keys[(p + 1) & 1], last ? a.order : vals[p & 1]);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    rt_count_kernel<<<lane_blocks(a.n), kRtBlock, 0, stream>>>(keys[passes & 1], a.n, a.bucket_first);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = exclusive_sum(sc + at_bucket_temp, bucket_temp_bytes, a.bucket_first, a.bucket_first, a.n_conns + 3,
                           stream)) != hipSuccess)
      return e;
    const bool vec = (((uintptr_t)a.infos | (uintptr_t)a.infos_out) & 15) == 0;
    if (vec)
      rt_gather_kernel<true><<<lane_blocks(a.n), kRtBlock, 0, stream>>>(a);
    else
      rt_gather_kernel<false><<<lane_blocks(a.n), kRtBlock, 0, stream>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.n_conns) {
    rt_finish_kernel<<<lane_blocks(a.n_conns), kRtBlock, 0, stream>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ufc_dev
