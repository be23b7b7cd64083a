// send_rate.hpp -- interface between the C-ABI layer and the GPU batch send rate control (send_rate.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"

namespace ufc_dev {

// One launch each, no device scratch.
hipError_t rate_begin_batch(const ufc_codec::RateBeginArgs& a, hipStream_t stream);
hipError_t rate_step_batch(const ufc_codec::RateArgs& a, hipStream_t stream);

}  // namespace ufc_dev
