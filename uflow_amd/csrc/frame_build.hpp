// frame_build.hpp -- interface between the C-ABI layer and the GPU batch build (frame_build.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/uflow_frame_codec.h"
#include "scratch.hpp"

namespace ufc_dev {

struct BuildArgs {
  const ufc_frame_info* infos;
  const ufc_item* items;     // null when n_items == 0
  uint64_t n_items;          // < 2^31 - 1 (one scan over n_items + 1 sizes)
  const uint64_t* src_base;  // nullable: all zero
  const uint8_t* payload;    // write only; null when payload_len == 0
  uint64_t payload_len;
  uint64_t n;                // frames (< 2^31: one scan)
  uint64_t* out_offsets;     // n + 1; written by build_sizes, read by build_write
  uint8_t* status;           // build_sizes only, nullable
  uint8_t* out_bytes;        // build_write only
  uint64_t out_len;
};

// out_offsets (exclusive sum of the frames' encoded sizes, 0 for frames not UFC_BUILD_OK) and status.
hipError_t build_sizes(const BuildArgs& a, const ScratchSource& scratch, hipStream_t stream);
// Every frame whose span matches its size, trailer bytes zero.
hipError_t build_write(const BuildArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
