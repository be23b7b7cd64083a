// flush_ctl.hpp -- interface between the C-ABI layer and the GPU batch flush control (flush_ctl.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"
#include "scratch.hpp"

namespace ufc_dev {

hipError_t flush_acks_batch(const ufc_codec::FaArgs& a, const ScratchSource& scratch, hipStream_t stream);
hipError_t flush_sync_batch(const ufc_codec::FsArgs& a, const ScratchSource& scratch, hipStream_t stream);

}  // namespace ufc_dev
