// frame_window.hpp -- interface between the C-ABI layer and the GPU batch frame window (frame_window.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"
#include "scratch.hpp"

namespace ufc_dev {

hipError_t window_batch(const ufc_codec::FwArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
