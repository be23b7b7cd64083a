// route.hpp -- interface between the C-ABI layer and the GPU batch frame routing (route.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"
#include "scratch.hpp"

namespace ufc_dev {

// The radix passes a routing call makes over its keys: the bytes of the largest bucket number, n_conns + 1.
uint32_t route_passes(uint64_t n_conns);
hipError_t route_frames_batch(const ufc_codec::RtArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
