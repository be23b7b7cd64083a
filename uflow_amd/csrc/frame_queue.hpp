// frame_queue.hpp -- interface between the C-ABI layer and the GPU batch frame queue (frame_queue.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"

namespace ufc_dev {

// One launch, no device scratch: no output of the frame queue needs a scan.
hipError_t queue_batch(const ufc_codec::FqArgs& a, hipStream_t stream);

}  // namespace ufc_dev
