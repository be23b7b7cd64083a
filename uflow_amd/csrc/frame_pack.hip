// frame_pack.hip -- batched DataFrameEmitter / AckFrameEmitter push and finalize on device-resident records:
// many flushes cut into frames in one call (ufc_pack_varlen, include/uflow_frame_codec.h), the step before
// frame_build.hip on the send side.
//
// The per-flush arithmetic (frame overheads, limits, the stop predicate, the hop) is frame_codec_core.hpp,
// shared with the host pack (frame_codec.cpp).  A flush's frame starts are a greedy chain over the prefix
// sums of its items' encoded sizes, s_0 = first, s_{k+1} = min(s_k + hop(s_k), end); flush_alloc and the
// frame window only cut that chain at one item, the stop.  Four launches and two scans:
//   1. item sizes: one thread per item -> its encoded size as a datagram;
//   2. scan:  exclusive sum over the n_items + 1 sizes -> P (ack flushes do not use it: their sizes are 9 i);
//   3. hops:  one thread per item -> the items a data frame starting there takes when the flush does not end
//      first (1..127, one byte; a binary search over the workgroup's slice of P, staged in LDS);
//   4. chain, count: one wave per flush, kPackWaves flushes per workgroup.  The wave stages kPackTile hops in
//      LDS, marks the chain's starts inside the tile by pointer doubling (every marked item marks the item
//      2^r hops on; ceil(log2(tile)) rounds, all lanes together), carries the chain's exit into the next tile
//      -- one dependent step per tile, not per frame -- and ranks the starts with ballots.  With the rank,
//      each lane tests the stop predicate of its items (F(i) = H starts + bytes never decreases, so the first
//      item that fails is the stop) and the walk ends there.  -> the flush's result record and frame count;
//   5. scan:  exclusive sum over the n_flushes + 1 frame counts -> frame_first, frames_used;
//   6. chain, emit: the same walk up to the stop that launch 4 found; every start writes its record at
//      frame_first + rank.
// Walking the chain twice keeps the scratch at 9 bytes per item and needs no per-item flags or ranks in
// global memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "frame_pack.hpp"
#include "scan.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

constexpr uint32_t kPackThreads = 256;
constexpr uint32_t kPackWaves = kPackThreads / 64;  // flushes per workgroup of the chain kernel
constexpr uint32_t kSlots = kPackTile / 64;         // items of a tile per lane
constexpr uint32_t kHopWindow = 128;                // prefix sums a hop may look past its own item
// A chain that leaves a tile lands inside the next one.
static_assert(ufc_codec::kAckFrameMaxGroups < kPackTile && UFC_DATA_FRAME_MAX_DATAGRAM_COUNT < kPackTile, "tile");
static_assert(UFC_DATA_FRAME_MAX_DATAGRAM_COUNT < kHopWindow, "hop window");

__global__ __launch_bounds__(kPackThreads) void pack_item_sizes_kernel(const ufc_item* items, uint64_t n_items,
                                                                        uint64_t* P) {
  const uint64_t g = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
  if (g < n_items)
    P[g] = ufc_codec::datagram_encoded_size(items[g]);
  else if (g == n_items)
    P[g] = 0;
}

__global__ __launch_bounds__(kPackThreads) void pack_hops_kernel(const uint64_t* P, uint64_t n_items, uint8_t* hops) {
  __shared__ uint64_t sP[kPackThreads + kHopWindow];
  const uint64_t base = (uint64_t)blockIdx.x * kPackThreads;
  for (uint32_t t = threadIdx.x; t < kPackThreads + kHopWindow; t += kPackThreads) sP[t] = P[min(base + t, n_items)];
  __syncthreads();
  const uint64_t i = base + threadIdx.x;
  if (i >= n_items) return;
  // (the hop reads P(i .. i + 127), capped at n_items: indices below kPackThreads + kHopWindow)
  hops[i] = (uint8_t)ufc_codec::pack_data_hop([&](uint64_t k) -> uint64_t { return sP[k - base]; }, i, n_items);
}

// kEmit false: results (frame_first left 0) and counts[j] = frame_count, counts[n_flushes] = 0.
// kEmit true: frame_first (the scanned counts) into the results, frames_used, and the frames' records.
template <bool kEmit>
__global__ __launch_bounds__(kPackThreads) void pack_chain_kernel(PackArgs a, const uint64_t* P, const uint8_t* hops,
                                                                  uint32_t* counts, const uint32_t* frame_first) {
  __shared__ uint16_t s_next[kPackWaves][kPackTile];
  __shared__ uint8_t s_mark[kPackWaves][kPackTile];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t j = (uint64_t)blockIdx.x * kPackWaves + w;  // (uniform in the wave; no workgroup barrier below)
  if (j > a.n_flushes) return;
  if (j == a.n_flushes) {
    if (lane == 0) {
      if (kEmit)
        *a.frames_used = frame_first[j];
      else
        counts[j] = 0;
    }
    return;
  }
  const ufc_flush fl = a.flushes[j];
  const uint64_t first = a.flush_first[j];
  uint64_t end = a.flush_first[j + 1];
  const bool ack = ufc_codec::pack_is_ack(fl);
  const uint32_t H = ufc_codec::pack_overhead(ack);
  uint64_t ff = 0;
  if (kEmit) {
    const uint32_t frame_count = a.results[j].frame_count, items_packed = a.results[j].items_packed;
    ff = frame_first[j];
    if (lane == 0) a.results[j].frame_first = (uint32_t)ff;
    if (frame_count == 0) return;  // (a bad range among them)
    end = first + items_packed;    // the stop: within the flush's range, which the count launch checked
  } else if (first > end || end > a.n_items) {
    if (lane == 0) {
      a.results[j] = ufc_flush_result{0, 0, 0, UFC_PACK_BAD_RANGE, fl.flush_alloc};
      counts[j] = 0;
    }
    return;
  }
  uint16_t* nx = s_next[w];
  uint8_t* mk = s_mark[w];
  const uint64_t P0 = ack ? 0 : P[first];  // (first <= n_items; P holds n_items + 1 sums)
  const uint64_t lanes_below = (1ull << lane) - 1;
  uint64_t cur = first;  // the chain's next start
  uint32_t k = 0;        // starts before the tile (after the loop: before the stop)
  uint64_t stop = end;
  uint32_t why = UFC_PACK_DONE;
  bool stopped = false;
  for (uint64_t t0 = first; t0 < end && !stopped; t0 += kPackTile) {
    const uint32_t nv = (uint32_t)min((uint64_t)kPackTile, end - t0);  // items of this tile
    const uint32_t cur_rel = (uint32_t)(cur - t0);  // < kPackTile; == nv when the last frame covers the tile
    uint32_t hop[kSlots];
#pragma unroll
    for (uint32_t r = 0; r < kSlots; r++) {
      const uint32_t jj = r * 64 + lane;
      hop[r] = 0;
      if (jj < nv) {
        hop[r] = ack ? ufc_codec::kAckFrameMaxGroups : (uint32_t)hops[t0 + jj];
        nx[jj] = (uint16_t)(jj + hop[r]);  // tile-relative; >= nv: outside the tile, and stays
        mk[jj] = jj == cur_rel ? 1 : 0;
      }
    }
    wave_sync();
    // Pointer doubling: after round r, nx = the item 2^(r + 1) hops on and the chain's first 2^(r + 1) starts
    // in the tile are marked (a mark set earlier in the same round only marks a further start early).
    for (uint32_t span = 1; span < nv; span <<= 1) {
      uint32_t nj[kSlots];
#pragma unroll
      for (uint32_t r = 0; r < kSlots; r++) {
        const uint32_t jj = r * 64 + lane;
        nj[r] = 0;
        if (jj < nv) {
          const uint32_t J = nx[jj];
          nj[r] = J;
          if (J < nv) {
            if (mk[jj]) mk[J] = 1;
            nj[r] = nx[J];
          }
        }
      }
      wave_sync();  // every lane has read the round's nx
#pragma unroll
      for (uint32_t r = 0; r < kSlots; r++) {
        const uint32_t jj = r * 64 + lane;
        if (jj < nv) nx[jj] = (uint16_t)nj[r];
      }
      wave_sync();
    }
    const uint32_t exit_rel = cur_rel < nv ? nx[cur_rel] : cur_rel;  // where the chain leaves the tile
#pragma unroll
    for (uint32_t r = 0; r < kSlots; r++) {
      const uint32_t jj = r * 64 + lane;
      const uint64_t i = t0 + jj;
      const bool valid = jj < nv;
      const bool m = valid && mk[jj] != 0;
      const uint64_t mask = __ballot(m);
      const uint32_t kk = k + (uint32_t)__popcll(mask & lanes_below);  // starts before item i
      if (!kEmit) {
        uint32_t y = UFC_PACK_DONE;
        if (valid && !stopped) {
          const uint64_t bytes = ack ? (uint64_t)UFC_ACK_GROUP_SIZE * (i - first) : P[i] - P0;
          y = ufc_codec::pack_stop(fl, ack, (uint64_t)H * kk + bytes, m, kk);
        }
        const uint64_t smask = __ballot(y != UFC_PACK_DONE);
        if (smask != 0 && !stopped) {  // (uniform)
          const int l = __ffsll((long long)smask) - 1;
          stop = t0 + r * 64 + (uint32_t)l;
          why = (uint32_t)__shfl((int)y, l);
          k = (uint32_t)__shfl((int)kk, l);
          stopped = true;
        }
      } else if (m) {
        const uint64_t g = ff + kk;
        if (g < a.frames_cap)
          a.infos[g] = ufc_codec::pack_frame_info(fl, ack, kk, g, a.nonce_bits, i, (uint32_t)(min(i + hop[r], end) - i));
      }
      if (!stopped) k += (uint32_t)__popcll(mask);
    }
    cur = min(t0 + exit_rel, end);
  }
  if (!kEmit && lane == 0) {
    const uint64_t bytes = ack ? (uint64_t)UFC_ACK_GROUP_SIZE * (stop - first) : P[stop] - P0;
    a.results[j] = ufc_flush_result{0, k, (uint32_t)(stop - first), why, fl.flush_alloc - (int64_t)((uint64_t)H * k + bytes)};
    counts[j] = k;
  }
}

}  // namespace

hipError_t pack_batch(const PackArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  // the larger of the two scans' temporaries
  const size_t temp_bytes = std::max(scan_temp_bytes<uint64_t>(a.n_items + 1), scan_temp_bytes<uint32_t>(a.n_flushes + 1));
  ScratchPlan plan;
  const uint64_t at_psum = plan.take((a.n_items + 1) * 8);
  const uint64_t at_hops = plan.take(a.n_items);
  const uint64_t at_counts = plan.take((a.n_flushes + 1) * 4);
  const uint64_t at_firsts = plan.take((a.n_flushes + 1) * 4);
  const uint64_t at_temp = plan.take(temp_bytes);
  char* s;
  hipError_t e;
  if ((e = scratch.get(plan.end, &s)) != hipSuccess) return e;
  uint64_t* P = (uint64_t*)(s + at_psum);
  uint8_t* hops = (uint8_t*)(s + at_hops);
  uint32_t* counts = (uint32_t*)(s + at_counts);
  uint32_t* firsts = (uint32_t*)(s + at_firsts);
  const unsigned iblocks = (unsigned)((a.n_items + 1 + kPackThreads - 1) / kPackThreads);
  pack_item_sizes_kernel<<<iblocks, kPackThreads, 0, stream>>>(a.items, a.n_items, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(s + at_temp, temp_bytes, P, P, a.n_items + 1, stream)) != hipSuccess) return e;
  if (a.n_items) {
    pack_hops_kernel<<<(unsigned)((a.n_items + kPackThreads - 1) / kPackThreads), kPackThreads, 0, stream>>>(P, a.n_items,
                                                                                                           hops);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const unsigned cblocks = (unsigned)((a.n_flushes + 1 + kPackWaves - 1) / kPackWaves);
  pack_chain_kernel<false><<<cblocks, kPackThreads, 0, stream>>>(a, P, hops, counts, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(s + at_temp, temp_bytes, counts, firsts, a.n_flushes + 1, stream)) != hipSuccess) return e;
  pack_chain_kernel<true><<<cblocks, kPackThreads, 0, stream>>>(a, P, hops, nullptr, firsts);
  return hipGetLastError();
}

}  // namespace ufc_dev
