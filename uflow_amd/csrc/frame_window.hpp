// frame_window.hpp -- interface between the C-ABI layer and the GPU batch frame window (frame_window.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"

namespace ufc_dev {

// Device scratch of a frame window call: a group count per connection (8 bytes, + 1 entry) and the scan's
// temporaries, each part rounded up to 256.
size_t window_scratch_bytes(uint64_t n_windows);
hipError_t window_batch(const ufc_codec::FwArgs& a, void* scratch, size_t scratch_bytes, hipStream_t stream);

}  // namespace ufc_dev
