// packet_emit.hpp -- interface between the C-ABI layer and the GPU batch packet emit (packet_emit.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/uflow_frame_codec.h"
#include "scratch.hpp"

namespace ufc_dev {

// Packets of a sender that one wave resolves at a time (packet_emit.hip): one lane each.
constexpr uint32_t kEmitTile = 64;

struct EmitArgs {
  const ufc_packet* packets;        // null when n_packets == 0
  uint64_t n_packets;               // < 2^31 - 1
  const uint64_t* packet_first;     // n_senders + 1
  const ufc_sender* senders;
  uint64_t n_senders;               // < 2^31 - 1 (one scan over n_senders + 1 counts)
  ufc_item* items;                  // null when items_cap == 0
  uint64_t items_cap;
  uint64_t* flush_first;            // n_senders + 1
  ufc_packet_result* packet_results;  // nullable
  ufc_sender_result* sender_results;
  ufc_sender* senders_out;          // nullable; may be `senders`
  uint64_t* items_used;
};

// The scratch of an emit: per packet its first item relative to the sender's range (4 bytes) and its
// sequence id and leads (8 bytes), one 8-byte item count per sender (+ 1) and the scan's temporaries.
hipError_t emit_batch(const EmitArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
