// frame_parse.hpp -- interface between the C-ABI layer and the GPU batch parse (frame_parse.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/uflow_frame_codec.h"
#include "scratch.hpp"

namespace ufc_dev {

// Byte i (0..15) of a frame's first 16 bytes held as two little-endian words (the parse walk's head,
// frame_parse.hip DevBytesHead): shift amounts always in range (host and device; tests/c/ubsan_helpers.hip).
__host__ __device__ __forceinline__ uint32_t head_byte(uint64_t w0, uint64_t w1, uint32_t i) {
  return (uint32_t)(((i & 15u) < 8 ? w0 : w1) >> (8 * (i & 7u))) & 0xFFu;
}

struct ParseArgs {
  const uint8_t* bytes;
  const uint64_t* offsets;
  uint64_t n;              // frames (< 2^31: one scan)
  const uint8_t* valid;    // the CRC gate's flags
  ufc_frame_info* infos;
  ufc_item* items;         // nullable
  uint64_t items_cap;
  uint64_t* items_used;    // device word, nullable
};

hipError_t parse_batch(const ParseArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
