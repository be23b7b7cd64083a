// packet_receive.hip -- batched PacketReceiver step on device-resident records: many receivers' parsed
// datagrams reassembled and delivered in one call (ufc_receive_packets_varlen, include/uflow_frame_codec.h),
// the step behind frame_parse.hip on the receive side.
//
// Plan first, then move bytes.  The step's code is frame_codec_core.hpp's, shared with the host call.  What the
// order of arrival does not touch runs in parallel: the verdicts on validity, the payload range, the window and
// the channel (base_id and the channel bases do not move while datagrams are handled) per item, and receive()
// per receiver on a wave, in tiles of 64 ids: delivery as per-channel prefixes over 64-bit lane masks in LDS, the
// window advance as the ENTRY slots' prefix, advance_window's clears lane by lane (rx_receive_tiles).  What the
// order does touch (the opener of a slot, the allocation test that skips and continues, the first arrival of a
// fragment) is walked by one lane per receiver over the datagrams the verdicts let through; the duplicate rule is
// a keyed table sized from n_items that the lanes fill with atomicCAS.  The bytes move in parallel from copy
// segments the plan leaves behind.  Launches:
//   1. (memsets: the duplicate table, the segments, the chunk counts)
//   2. begin: one lane per receiver -> the state check, a plan record per slot, resynchronize;
//   3. verdicts: a workgroup per receiver, a lane per frame of its range -> a verdict byte per item;
//   4. items: one lane per receiver -> try_add for the items that go on, slots, item status, the result's counts;
//   5. receive: one wave per receiver -> delivery and the window advance in tiles, the carry size, three counts;
//   6. three exclusive sums over the n_receivers + 1 counts -> packet_first, the out offsets, carry_first;
//   7. finish: one lane per receiver -> records, the slots' carry offsets, the received-bits words, one copy
//      segment per stored datagram and two per slot, the chunk count of every slot segment; the used totals;
//   8. an exclusive sum over the 2 n_slots + 1 chunk counts;
//   9. slot copy: one wave per chunk of kRxChunk bytes; the wave finds its segment by binary search in the
//      chunk prefix (a held packet or a fragment buffer may be tens of megabytes);
//  10. item copy: 16 lanes per datagram (at most 1448 bytes), after 9 because a new fragment overwrites the
//      unspecified bytes a carried buffer has in its place.
// Either side of a copy has any byte alignment: the destination is written in aligned 8-byte words between a
// head and a tail of single bytes, the source read with unaligned 8-byte loads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "packet_receive.hpp"
#include "scan.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::RxArgs;
using ufc_codec::RxDupSet;
using ufc_codec::RxPlan;
using ufc_codec::RxSegment;

constexpr uint32_t kRxThreads = 64;       // walk and finish: one lane per receiver, at most a wave per workgroup ...
constexpr uint32_t kRxThreadsFew = 8;     // ... and 8 lanes where the receivers are few: more waves, on more CUs, each
                                          // of whose memory instructions then touches 8 lines, not 64
constexpr uint64_t kRxFew = 32768;
constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyBlocksMax = 16384;  // the copy kernels stride over what lies beyond
constexpr uint32_t kItemLanes = 16;       // lanes per datagram in the item copy
static_assert(sizeof(ufc_receiver) == 560 && sizeof(ufc_rx_slot) == 32 && sizeof(ufc_rx_packet) == 24 &&
                  sizeof(ufc_receiver_result) == 80, "record layouts");

// begin: one lane per receiver (the state check, the plan records, resynchronize).
__global__ __launch_bounds__(kRxThreads) void rx_begin_kernel(RxArgs a, RxPlan* plans) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_receivers) return;
  if (a.receivers_out != a.receivers) {
    const uint64_t* src = (const uint64_t*)(a.receivers + r);
    uint64_t* dst = (uint64_t*)(a.receivers_out + r);
    for (uint32_t k = 0; k < sizeof(ufc_receiver) / 8; k++) dst[k] = src[k];
  }
  ufc_codec::rx_walk_begin(a, r, plans);
}

// verdicts: one workgroup per receiver, a lane per frame of its range; validity, the payload range, the window
// and the channel test of every item (base_id and the channel bases do not move while datagrams are handled).
__global__ __launch_bounds__(kRxThreads) void rx_verdict_kernel(RxArgs a, uint8_t* verdicts) {
  for (uint64_t r = blockIdx.x; r < a.n_receivers; r += gridDim.x) {
    if (a.results[r].stop != UFC_RX_DONE) continue;
    const uint64_t ff0 = a.frame_first[r], ff1 = a.frame_first[r + 1];  // (checked by begin)
    for (uint64_t i = ff0 + threadIdx.x; i < ff1; i += blockDim.x) ufc_codec::rx_frame_verdicts(a, r, i, verdicts);
  }
}

// items: one lane per receiver walks the datagrams the verdict pass let through, in arrival order.
__global__ __launch_bounds__(kRxThreads) void rx_items_kernel(RxArgs a, RxPlan* plans, uint8_t* status, RxDupSet dups,
                                                              const uint8_t* verdicts) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_receivers) return;
  ufc_codec::rx_walk_items(a, r, plans, status, dups, verdicts);
}

// receive and end: one wave per receiver; delivery and the window advance in tiles of 64 ids (rx_receive_tiles),
// then the carry size summed over the lanes.
__global__ __launch_bounds__(64) void rx_receive_kernel(RxArgs a, RxPlan* plans, uint64_t* c_packets, uint64_t* c_out,
                                                       uint64_t* c_carry) {
  __shared__ ufc_codec::RxWaveShared sh;
  const uint64_t r = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (r == a.n_receivers) {
    if (lane == 0) c_packets[r] = c_out[r] = c_carry[r] = 0;
    return;
  }
  uint32_t delivered;
  uint64_t out_bytes;
  ufc_codec::rx_receive_tiles(DevWave{}, sh, a, r, plans, delivered, out_bytes);
  uint64_t carry = 0;
  const bool done = a.results[r].stop == UFC_RX_DONE;
  if (done) {
    const ufc_rx_slot* slots = a.slots + a.slot_first[r];
    const uint32_t W = a.receivers_out[r].window_size;
    for (uint32_t j = lane; j < W; j += 64) carry += ufc_codec::rx_slot_region(slots[j]);
  }
#pragma unroll
  for (uint32_t d = 32; d > 0; d >>= 1) carry += __shfl_down(carry, d);
  if (lane == 0) {
    if (done) {
      a.results[r].packet_count = delivered;
      a.results[r].bytes_delivered = out_bytes;
    }
    c_packets[r] = done ? delivered : 0;
    c_out[r] = done ? out_bytes : 0;
    c_carry[r] = carry;
  }
}

__global__ __launch_bounds__(kRxThreads) void rx_finish_kernel(RxArgs a, RxPlan* plans, const uint8_t* status,
                                                               const uint64_t* out_first, RxSegment* segs,
                                                               uint32_t* chunks) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > a.n_receivers) return;
  if (r == a.n_receivers) {
    *a.packets_used = a.packet_first[r];
    *a.out_used = out_first[r];
    *a.carry_used = a.carry_first[r];
    return;
  }
  ufc_codec::rx_finish(a, r, plans, status, out_first[r], segs, nullptr);
  if (a.results[r].stop != UFC_RX_DONE) return;
  const uint64_t s0 = a.slot_first[r];
  const uint32_t W = a.receivers_out[r].window_size;
  for (uint64_t k = 2 * s0; k < 2 * (s0 + W); k++) chunks[k] = (segs[k].len + kRxChunk - 1) / kRxChunk;
}

// len bytes from src to dst by the `lanes` lanes of a group, this one `lane`; any alignment on both sides.
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane, uint32_t lanes) {
  typedef const __attribute__((address_space(1), aligned(1))) uint64_t g_u64_a1;
  const uint32_t head = min(len, (uint32_t)((8 - ((uintptr_t)dst & 7)) & 7));
  const uint32_t words = (len - head) / 8, tail = head + 8 * words;
  if (lane < head) dst[lane] = src[lane];
  for (uint32_t w = lane; w < words; w += lanes)
    *(uint64_t*)(dst + head + 8 * w) = *(g_u64_a1*)(src + head + 8 * w);
  if (lane < len - tail) dst[tail + lane] = src[tail + lane];
}

// The part of a segment inside its destination's cap.
__device__ __forceinline__ bool segment_ends(const RxArgs& a, const RxSegment& sg, uint8_t*& dst, const uint8_t*& src,
                                             uint64_t& len) {
  const bool to_carry = (sg.kinds & ufc_codec::kRxDstCarry) != 0;
  const uint64_t cap = to_carry ? a.carry_cap : a.out_cap;
  if (sg.len == 0 || sg.dst >= cap) return false;
  len = min((uint64_t)sg.len, cap - sg.dst);
  dst = (to_carry ? a.carry_out : a.out_bytes) + sg.dst;
  src = ((sg.kinds & ufc_codec::kRxSrcCarry) ? a.carry_in : a.payload) + sg.src;
  return true;
}

// One wave per chunk of the segments [0, n_segs); first[k] = chunks before segment k, first[n_segs] = all.
__global__ __launch_bounds__(kCopyThreads) void rx_copy_slots_kernel(RxArgs a, const RxSegment* segs, const uint32_t* first,
                                                                     uint64_t n_segs) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = ((uint64_t)blockIdx.x * kCopyThreads + threadIdx.x) >> 6;
  const uint64_t waves = (uint64_t)gridDim.x * (kCopyThreads / 64);
  const uint64_t total = first[n_segs];
  for (uint64_t c = wave; c < total; c += waves) {
    uint64_t lo = 0, hi = n_segs - 1;  // the last segment whose first chunk is at or before c (it has chunks)
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const RxSegment sg = segs[lo];
    uint8_t* dst;
    const uint8_t* src;
    uint64_t len;
    if (!segment_ends(a, sg, dst, src, len)) continue;
    const uint64_t at = (c - first[lo]) * kRxChunk;
    if (at >= len) continue;
    copy_bytes(dst + at, src + at, (uint32_t)min((uint64_t)kRxChunk, len - at), lane, 64);
  }
}

// kItemLanes lanes per datagram segment.
__global__ __launch_bounds__(kCopyThreads) void rx_copy_items_kernel(RxArgs a, const RxSegment* segs) {
  const uint32_t lane = threadIdx.x % kItemLanes;
  const uint64_t group = ((uint64_t)blockIdx.x * kCopyThreads + threadIdx.x) / kItemLanes;
  const uint64_t groups = (uint64_t)gridDim.x * (kCopyThreads / kItemLanes);
  for (uint64_t g = group; g < a.n_items; g += groups) {
    const RxSegment sg = segs[g];
    uint8_t* dst;
    const uint8_t* src;
    uint64_t len;
    if (!segment_ends(a, sg, dst, src, len)) continue;
    copy_bytes(dst, src, (uint32_t)len, lane, kItemLanes);
  }
}

}  // namespace

hipError_t receive_batch(const RxArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  const uint64_t n1 = a.n_receivers + 1, n_segs = 2 * a.n_slots, dup_entries = ufc_codec::rx_dup_entries(a.n_items);
  const size_t temp_bytes = std::max(scan_temp_bytes<uint64_t>(n1), scan_temp_bytes<uint32_t>(n_segs + 1));
  ScratchPlan plan;  // (the segments and the chunk counts are zeroed as one range, the table as another)
  const uint64_t at_plans = plan.take(a.n_slots * sizeof(RxPlan));
  const uint64_t at_segs = plan.take((n_segs + a.n_items) * sizeof(RxSegment));
  const uint64_t at_chunks = plan.take((n_segs + 1) * 4);
  const uint64_t at_chunk_first = plan.take((n_segs + 1) * 4);
  const uint64_t at_status = plan.take(a.n_items);
  const uint64_t at_verdicts = plan.take(a.n_items);
  const uint64_t at_dups = plan.take(dup_entries * 8);
  const uint64_t at_counts = plan.take(6 * n1 * 8);
  const uint64_t at_temp = plan.take(temp_bytes);
  char* sc;
  hipError_t e;
  if ((e = scratch.get(plan.end, &sc)) != hipSuccess) return e;
  RxPlan* plans = (RxPlan*)(sc + at_plans);
  RxSegment* segs = (RxSegment*)(sc + at_segs);
  uint32_t* chunks = (uint32_t*)(sc + at_chunks);
  uint32_t* chunk_first = (uint32_t*)(sc + at_chunk_first);
  uint8_t* status = a.item_status ? a.item_status : (uint8_t*)(sc + at_status);
  uint8_t* verdicts = (uint8_t*)(sc + at_verdicts);
  const RxDupSet dups{(unsigned long long*)(sc + at_dups), dup_entries - 1};
  uint64_t* counts = (uint64_t*)(sc + at_counts);
  uint64_t *c_packets = counts, *c_out = counts + n1, *c_carry = counts + 2 * n1, *out_first = counts + 3 * n1;
  if ((e = hipMemsetAsync(sc + at_segs, 0, at_chunk_first - at_segs, stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(sc + at_dups, 0, dup_entries * 8, stream)) != hipSuccess) return e;
  const unsigned rthreads = n1 < kRxFew ? kRxThreadsFew : kRxThreads;
  const unsigned rblocks = (unsigned)((n1 + rthreads - 1) / rthreads);
  rx_begin_kernel<<<rblocks, rthreads, 0, stream>>>(a, plans);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.n_frames) {
    // a lane per frame: a wave's worth of lanes where the receivers are few and their ranges long
    const unsigned vthreads = a.n_frames >= 16 * a.n_receivers ? 64 : 8;
    rx_verdict_kernel<<<(unsigned)std::min<uint64_t>(a.n_receivers, 1u << 20), vthreads, 0, stream>>>(a, verdicts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  rx_items_kernel<<<rblocks, rthreads, 0, stream>>>(a, plans, status, dups, verdicts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  rx_receive_kernel<<<(unsigned)n1, 64, 0, stream>>>(a, plans, c_packets, c_out, c_carry);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(sc + at_temp, temp_bytes, c_packets, a.packet_first, n1, stream)) != hipSuccess ||
      (e = exclusive_sum(sc + at_temp, temp_bytes, c_out, out_first, n1, stream)) != hipSuccess ||
      (e = exclusive_sum(sc + at_temp, temp_bytes, c_carry, a.carry_first, n1, stream)) != hipSuccess)
    return e;
  rx_finish_kernel<<<rblocks, rthreads, 0, stream>>>(a, plans, status, out_first, segs, chunks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.n_slots) {
    if ((e = exclusive_sum(sc + at_temp, temp_bytes, chunks, chunk_first, n_segs + 1, stream)) != hipSuccess) return e;
    const uint64_t blocks = (n_segs + 3) / 4;  // a wave per segment where every segment is one chunk
    rx_copy_slots_kernel<<<(unsigned)std::min<uint64_t>(blocks, kCopyBlocksMax), kCopyThreads, 0, stream>>>(
        a, segs, chunk_first, n_segs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.n_items) {
    const uint64_t per_block = kCopyThreads / kItemLanes;
    const uint64_t blocks = (a.n_items + per_block - 1) / per_block;
    rx_copy_items_kernel<<<(unsigned)std::min<uint64_t>(blocks, kCopyBlocksMax), kCopyThreads, 0, stream>>>(
        a, segs + 2 * a.n_slots);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ufc_dev
