// resend.hpp -- interface between the C-ABI layer and the GPU batch resend calls (resend.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_codec_core.hpp"

namespace ufc_dev {

// One launch each, no device scratch: no output needs a scan (sent_first is the pack's frame_first).
hipError_t resend_begin_batch(const ufc_codec::RsBeginArgs& a, hipStream_t stream);
hipError_t resend_place_batch(const ufc_codec::RsPlaceArgs& a, hipStream_t stream);
hipError_t resend_commit_batch(const ufc_codec::RsCommitArgs& a, hipStream_t stream);

}  // namespace ufc_dev
