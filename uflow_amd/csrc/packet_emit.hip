// packet_emit.hip -- batched PacketSender::emit_packet and fragmentation on device-resident records: many
// senders' queued packets turned into datagram items in one call (ufc_emit_packets_varlen,
// include/uflow_frame_codec.h), the step before frame_pack.hip on the send side.
//
// The per-packet arithmetic (class, alloc size, fragment count, leads, the item) is frame_codec_core.hpp,
// shared with the host emit (frame_codec.cpp).  The reference walks a queue packet by packet; along the live
// packets (neither bad nor stale) of one queue
//   sequence id   = next_id + rank, rank = the live packets before it (a count),
//   allocation    = alloc + A, A = their alloc sizes summed (a prefix sum),
//   the stop      = the first packet that is bad, or live with rank >= room or A + a > max_alloc - alloc (both
//                   stay true from there on),
//   window parent = the last live reliable packet before it (below the stop), else the sender's,
//   channel parent= the last such packet on its channel, else the sender's for that channel,
// so a tile of 64 packets resolves with ballots and two wave scans.  Three launches and one scan:
//   1. senders: one wave per sender, kEmitWaves senders per workgroup, one lane per packet of a tile.  Classify,
//      ballot the live lanes, rank by the lanes below, scan the alloc sizes, find the stop by ballot and
//      find-first, scan the fragment counts.  Window parent: the highest reliable lane below, or the carry.
//      Channel parent: reliable lanes OR their bit into the wave's 64 per-channel lane masks in LDS, every lane
//      reads its channel's mask below itself; lane c then moves channel c's last reliable id into the wave's
//      64-entry parent table, the carry to the next tile.  -> per packet: its first item relative to the
//      sender's range, sequence id and leads (scratch), the packet's result; per sender: the result, the state
//      after the consumed prefix and the item count, reserved slots included;
//   2. scan: exclusive sum over the n_senders + 1 item counts -> flush_first;
//   3. finish: item_first of the sender results and packet results made absolute, items_used (64 lanes per
//      sender, 8 where the queues are short);
//   4. items: one lane per item slot (a packet may have 65 536 fragments).  The lane finds its sender in
//      flush_first (a search narrowed to the senders of the workgroup's 256 slots), then its packet among the
//      sender's consumed packets by their first items, skips slots that belong to no packet (reserved ones) and
//      writes one 24-byte record; consecutive lanes write consecutive records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "packet_emit.hpp"
#include "scan.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

constexpr uint32_t kEmitThreads = 256;
constexpr uint32_t kEmitWaves = kEmitThreads / 64;  // senders per workgroup of the sender kernel
constexpr uint32_t kItemBlocksMax = 16384;          // the item kernel strides over the slots beyond
static_assert(kEmitTile == 64 && UFC_MAX_CHANNELS == 64, "one lane per packet of a tile and per channel");
static_assert(sizeof(ufc_packet) == 16 && sizeof(ufc_sender) == 304 && sizeof(ufc_packet_result) == 16 &&
                  sizeof(ufc_sender_result) == 32, "record layouts");

// Inclusive sum over the wave's lanes.
template <class T>
__device__ __forceinline__ T wave_inclusive_sum(T v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(v, d);
    if (lane >= d) v += up;
  }
  return v;
}

__global__ __launch_bounds__(kEmitThreads) void emit_senders_kernel(EmitArgs a, uint32_t* rel_first, uint2* meta,
                                                                    uint64_t* counts) {
  __shared__ unsigned long long s_mask[kEmitWaves][64];  // per channel: the tile's reliable lanes
  __shared__ uint32_t s_parent[kEmitWaves][64];          // per channel: the parent id carried across tiles
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint64_t s = (uint64_t)blockIdx.x * kEmitWaves + w;  // (uniform in the wave; no workgroup barrier below)
  if (s > a.n_senders) return;
  if (s == a.n_senders) {
    if (lane == 0) counts[s] = 0;
    return;
  }
  // The sender's record, whole, before anything is written: senders_out may be the same array.
  const ufc_sender* in = a.senders + s;
  const uint32_t base_id = in->base_id, next_id = in->next_id, window_size = in->window_size, flush_id = in->flush_id;
  const uint64_t alloc = in->alloc, max_alloc_in = in->max_alloc;
  const uint32_t take = in->take, reserve_items = in->reserve_items, reserved = in->reserved;
  uint32_t wparent = in->window_parent_id;
  const uint32_t cparent_in = in->channel_parent_id[lane];
  const uint64_t first = a.packet_first[s], end = a.packet_first[s + 1];
  ufc_sender* out = a.senders_out ? a.senders_out + s : nullptr;
  const bool bad_range = first > end || end > a.n_packets;

  unsigned long long* mask = s_mask[w];
  uint32_t* parent = s_parent[w];
  mask[lane] = 0;
  parent[lane] = cparent_in;
  wave_sync();

  const uint64_t n = bad_range ? 0 : min(end - first, (uint64_t)take);
  const uint32_t room = ufc_codec::emit_window_room(base_id, next_id, window_size);
  const uint64_t max_alloc = ufc_codec::emit_max_alloc(max_alloc_in);
  const uint64_t lanes_below = (1ull << lane) - 1;
  uint32_t rank_base = 0;            // live packets before the tile (after the loop: emitted)
  uint64_t A_base = 0;               // their alloc sizes
  uint64_t made = reserve_items;     // the sender's items before the tile, reserved slots included
  uint32_t dropped = 0;
  uint64_t dropped_bytes = 0;
  uint64_t stop = n, done = 0;       // the stopping packet; packets whose records are written
  uint32_t why = UFC_EMIT_DONE;
  bool stopped = false;
  for (uint64_t t0 = 0; t0 < n && !stopped; t0 += kEmitTile) {
    const uint32_t nv = (uint32_t)min((uint64_t)kEmitTile, n - t0);  // packets of this tile
    const uint64_t idx = first + t0 + lane;                          // < end <= n_packets for lane < nv
    ufc_packet pk{};
    uint32_t cls = ufc_codec::kEmitStale;  // (lanes past the tile: neither live nor bad, and never `in`)
    if (lane < nv) {
      pk = a.packets[idx];
      cls = ufc_codec::emit_packet_class(pk, flush_id);
    }
    const bool live = cls == ufc_codec::kEmitLive;
    const uint64_t live_mask = __ballot(live);
    const uint32_t rank = rank_base + (uint32_t)__popcll(live_mask & lanes_below);
    const uint64_t a_sz = live ? ufc_codec::emit_alloc_size(pk.data_len) : 0;
    const uint64_t A_incl = wave_inclusive_sum(a_sz, lane);
    const uint64_t A_ex = A_base + A_incl - a_sz;  // alloc sizes of the live packets before this one
    uint32_t y = UFC_EMIT_DONE;
    if (lane < nv) {
      if (cls == ufc_codec::kEmitBad)
        y = UFC_EMIT_BAD_PACKET;
      else if (live && rank >= room)
        y = UFC_EMIT_WINDOW_LIMITED;
      else if (live && ufc_codec::emit_alloc_fails(alloc, A_ex, a_sz, max_alloc))
        y = UFC_EMIT_ALLOC_LIMITED;
    }
    const uint64_t fail_mask = __ballot(y != UFC_EMIT_DONE);
    uint32_t limit = nv;  // lanes below it are consumed
    if (fail_mask != 0) {  // (uniform)
      const int l = __ffsll((long long)fail_mask) - 1;
      limit = (uint32_t)l;
      stop = t0 + limit;
      why = (uint32_t)__shfl((int)y, l);
      A_base = __shfl(A_ex, l);
      stopped = true;
    } else {
      A_base += __shfl(A_incl, 63);
    }
    const bool in_prefix = lane < limit;
    const bool emitted = live && in_prefix, drop = cls == ufc_codec::kEmitStale && in_prefix;
    const uint64_t emit_mask = __ballot(emitted), drop_mask = __ballot(drop);
    const uint32_t fc = emitted ? ufc_codec::emit_fragment_count(pk.data_len) : 0;
    const uint32_t f_incl = wave_inclusive_sum(fc, lane);
    const uint64_t item_rel = made + (f_incl - fc);  // the packet's first item, relative to the sender's range
    // The sequence id of the tile's live packet in lane h (below the stop).
    auto seq_of = [&](uint32_t h) -> uint32_t {
      return (next_id + rank_base + (uint32_t)__popcll(live_mask & ((1ull << h) - 1))) & ufc_codec::kPacketIdMask;
    };
    const uint32_t seq = (next_id + rank) & ufc_codec::kPacketIdMask;
    const bool reliable = emitted && pk.mode == UFC_SEND_RELIABLE;
    const uint64_t rel_mask = __ballot(reliable);
    const uint64_t rel_below = rel_mask & lanes_below;
    const uint32_t wp = rel_below ? seq_of(ufc_codec::high_bit(rel_below)) : wparent;
    // (an emitted packet's channel_id is below 64: its class is not bad)
    if (reliable) atomicOr(&mask[pk.channel_id], 1ull << lane);
    wave_sync();
    uint32_t cp = UFC_NO_PARENT;
    if (emitted) {
      const uint64_t m = mask[pk.channel_id] & lanes_below;
      cp = m ? seq_of(ufc_codec::high_bit(m)) : parent[pk.channel_id];
    }
    wave_sync();  // every lane has read its channel's mask and carried parent
    {
      const uint64_t m = mask[lane];  // lane c: channel c
      if (m) {
        parent[lane] = seq_of(ufc_codec::high_bit(m));
        mask[lane] = 0;
      }
    }
    wave_sync();
    if (rel_mask) wparent = seq_of(ufc_codec::high_bit(rel_mask));  // (uniform)
    if (lane < nv) {
      if (in_prefix) rel_first[idx] = (uint32_t)item_rel;
      if (emitted)
        meta[idx] = make_uint2(seq, (uint32_t)ufc_codec::emit_lead(seq, wp) |
                                        ((uint32_t)ufc_codec::emit_lead(seq, cp) << 16));
      if (a.packet_results) {
        ufc_packet_result pr{};
        if (emitted) {
          pr.sequence_id = seq;
          pr.item_first = (uint32_t)item_rel;  // (made absolute by the finish kernel)
          pr.item_count = fc;
          pr.status = UFC_PACKET_EMITTED;
          pr.resend = pk.mode >= UFC_SEND_PERSISTENT ? 1 : 0;
        } else if (drop) {
          pr.status = UFC_PACKET_DROPPED;
        }
        a.packet_results[idx] = pr;
      }
    }
    rank_base += (uint32_t)__popcll(emit_mask);
    made += __shfl(f_incl, 63);
    if (drop_mask != 0) {  // (uniform)
      dropped += (uint32_t)__popcll(drop_mask);
      dropped_bytes += __shfl(wave_inclusive_sum(drop ? (uint64_t)pk.data_len : 0ull, lane), 63);
    }
    done = t0 + nv;
  }
  // The packets of the range that were not reached (past the stop's tile, or past `take`).
  if (a.packet_results && !bad_range)
    for (uint64_t k = first + done + lane; k < end; k += 64) a.packet_results[k] = ufc_packet_result{};
  if (lane == 0) {
    ufc_sender_result r{};
    r.item_count = bad_range ? 0u : (uint32_t)made;
    r.packets_consumed = (uint32_t)stop;
    r.packets_emitted = rank_base;
    r.packets_dropped = dropped;
    r.stop = bad_range ? (uint32_t)UFC_EMIT_BAD_RANGE : why;
    r.bytes_dropped = dropped_bytes;
    a.sender_results[s] = r;
    counts[s] = bad_range ? 0 : made;
    if (out) {
      out->base_id = base_id;
      out->next_id = (next_id + rank_base) & ufc_codec::kPacketIdMask;
      out->window_size = window_size;
      out->flush_id = flush_id;
      out->alloc = alloc + A_base;
      out->max_alloc = max_alloc_in;
      out->window_parent_id = wparent;
      out->take = take;
      out->reserve_items = reserve_items;
      out->reserved = reserved;
    }
  }
  if (out) out->channel_parent_id[lane] = parent[lane];
}

// After the scan: item_first of the results made absolute, items_used.  kLanes lanes per sender (short queues
// take 8, so that a wave serves 8 senders; nothing here is wave-wide).
template <uint32_t kLanes>
__global__ __launch_bounds__(kEmitThreads) void emit_finish_kernel(EmitArgs a) {
  const uint32_t lane = threadIdx.x % kLanes;
  const uint64_t s = (uint64_t)blockIdx.x * (kEmitThreads / kLanes) + threadIdx.x / kLanes;
  if (s > a.n_senders) return;
  const uint64_t ff = a.flush_first[s];
  if (s == a.n_senders) {
    if (lane == 0) *a.items_used = ff;
    return;
  }
  if (lane == 0) a.sender_results[s].item_first = (uint32_t)ff;
  if (!a.packet_results || a.sender_results[s].stop == UFC_EMIT_BAD_RANGE) return;
  const uint64_t first = a.packet_first[s];
  const uint32_t consumed = a.sender_results[s].packets_consumed;  // (within the range, which launch 1 checked)
  for (uint32_t p = lane; p < consumed; p += kLanes) {
    ufc_packet_result* pr = a.packet_results + first + p;
    if (pr->status == UFC_PACKET_EMITTED) pr->item_first += (uint32_t)ff;
  }
}

__global__ __launch_bounds__(kEmitThreads) void emit_items_kernel(EmitArgs a, const uint32_t* rel_first,
                                                                  const uint2* meta) {
  const uint64_t total = min(a.flush_first[a.n_senders], a.items_cap);
  // The last sender in [lo, hi] whose range starts at or before slot g (flush_first[lo] <= g).
  auto sender_of = [&](uint64_t g, uint64_t lo, uint64_t hi) -> uint64_t {
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (a.flush_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  for (uint64_t g0 = (uint64_t)blockIdx.x * kEmitThreads; g0 < total; g0 += (uint64_t)gridDim.x * kEmitThreads) {
    // The senders of this workgroup's slots (uniform), then each lane's among them.
    const uint64_t s_lo = sender_of(g0, 0, a.n_senders - 1);
    const uint64_t s_hi = sender_of(min(g0 + kEmitThreads, total) - 1, s_lo, a.n_senders - 1);
    const uint64_t g = g0 + threadIdx.x;
    if (g >= total) continue;
    const uint64_t s = sender_of(g, s_lo, s_hi);
    const uint32_t consumed = a.sender_results[s].packets_consumed;
    if (consumed == 0 || a.sender_results[s].stop == UFC_EMIT_BAD_RANGE) continue;
    const uint64_t first = a.packet_first[s];  // [first, first + consumed) lies inside [0, n_packets)
    const uint32_t r = (uint32_t)(g - a.flush_first[s]);
    if (rel_first[first] > r) continue;  // a reserved slot
    uint32_t lo = 0, hi = consumed - 1;  // the last consumed packet whose first item is at or before r
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (rel_first[first + mid] <= r) lo = mid; else hi = mid - 1;
    }
    const ufc_packet pk = a.packets[first + lo];
    const uint32_t f = r - rel_first[first + lo], last = ufc_codec::emit_fragment_count(pk.data_len) - 1;
    if (f > last || last > 0xFFFFu) continue;  // (only where senders' ranges overlap: unspecified, but in bounds)
    const uint2 m = meta[first + lo];
    a.items[g] = ufc_codec::emit_item(pk, m.x, (uint16_t)(m.y & 0xFFFFu), (uint16_t)(m.y >> 16), f, last);
  }
}

}  // namespace

hipError_t emit_batch(const EmitArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  const size_t temp_bytes = scan_temp_bytes<uint64_t>(a.n_senders + 1);
  ScratchPlan plan;
  const uint64_t at_rel_first = plan.take(a.n_packets * 4);
  const uint64_t at_meta = plan.take(a.n_packets * 8);
  const uint64_t at_counts = plan.take((a.n_senders + 1) * 8);
  const uint64_t at_temp = plan.take(temp_bytes);
  char* sc;
  hipError_t e;
  if ((e = scratch.get(plan.end, &sc)) != hipSuccess) return e;
  uint32_t* rel_first = (uint32_t*)(sc + at_rel_first);
  uint2* meta = (uint2*)(sc + at_meta);
  uint64_t* counts = (uint64_t*)(sc + at_counts);
  const unsigned sblocks = (unsigned)((a.n_senders + 1 + kEmitWaves - 1) / kEmitWaves);
  emit_senders_kernel<<<sblocks, kEmitThreads, 0, stream>>>(a, rel_first, meta, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(sc + at_temp, temp_bytes, counts, a.flush_first, a.n_senders + 1, stream)) != hipSuccess) return e;
  if (a.n_packets <= 16 * a.n_senders)
    emit_finish_kernel<8><<<(unsigned)((a.n_senders + 1 + 31) / 32), kEmitThreads, 0, stream>>>(a);
  else
    emit_finish_kernel<64><<<sblocks, kEmitThreads, 0, stream>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.items_cap == 0 || a.n_packets == 0) return hipSuccess;
  const uint64_t iblocks = (a.items_cap + kEmitThreads - 1) / kEmitThreads;
  emit_items_kernel<<<(unsigned)std::min<uint64_t>(iblocks, kItemBlocksMax), kEmitThreads, 0, stream>>>(a, rel_first,
                                                                                                      meta);
  return hipGetLastError();
}

}  // namespace ufc_dev
