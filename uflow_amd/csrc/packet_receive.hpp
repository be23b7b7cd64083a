// packet_receive.hpp -- interface between the C-ABI layer and the GPU batch packet receive (packet_receive.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"
#include "scratch.hpp"

namespace ufc_dev {

// Bytes of a slot's copy segment that one wave moves (packet_receive.hip): larger segments are split.
constexpr uint32_t kRxChunk = 2048;

// The scratch of a receive: a plan record per slot (48 bytes); a copy segment per datagram and two per slot
// (24 bytes each); a chunk count and its prefix per slot segment (4 + 4 bytes, + 1 entry); a status and a verdict byte per
// datagram; the duplicate table (8 bytes per entry, the power of two at or above 2 n_items, at least 64); six
// 8-byte counts per receiver (+ 1); the scans' temporaries.
hipError_t receive_batch(const ufc_codec::RxArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
