// frame_pack.hpp -- interface between the C-ABI layer and the GPU batch pack (frame_pack.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/uflow_frame_codec.h"
#include "scratch.hpp"

namespace ufc_dev {

// Items of a flush whose chain one wave resolves in LDS at a time (frame_pack.hip).
constexpr uint32_t kPackTile = 256;

struct PackArgs {
  const ufc_item* items;        // null when n_items == 0
  uint64_t n_items;             // < 2^31 - 1 (one scan over n_items + 1 sizes)
  const uint64_t* flush_first;  // n_flushes + 1
  const ufc_flush* flushes;
  uint64_t n_flushes;           // < 2^31 - 1
  const uint32_t* nonce_bits;   // nullable
  ufc_frame_info* infos;        // null when frames_cap == 0
  uint64_t frames_cap;
  ufc_flush_result* results;
  uint64_t* frames_used;
};

// The scratch of a pack: the items' size prefix sums (8 (n_items + 1) bytes), one hop byte per item, two
// words per flush (frame counts and their exclusive sum) and the scan temporaries.
hipError_t pack_batch(const PackArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
