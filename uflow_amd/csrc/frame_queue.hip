// frame_queue.hip -- batched FrameQueue step on device-resident records: many connections' parsed ack frames
// turned into acked-fragment marks, the transfer window and the rate control's feedback in one call
// (ufc_frame_queue_varlen, include/uflow_frame_codec.h), the sender's step behind frame_parse.hip.
//
// The step's code is frame_codec_core.hpp's fq_step, shared with the host (where a phase is a loop over the
// lanes).  One wave runs a connection: the running state (ids, reorder buffer, pending ack data) is the same in
// every lane, the loss intervals sit in LDS and are touched by lane 0 alone, and everything that reads or writes a
// run of log entries takes a lane per entry: the <= 32 entries of a group, the nack runs and the expiry cutoff in
// tiles of 64 with wave ballots, the pushes as a copy of 64 records per phase.  No lane ever walks log entries
// alone.  No output needs a scan, so one launch does the call and no scratch is used; past the launch grid the
// waves stride over the connections.  The file is compiled without fast-math, and the core keeps the loss rate's
// sums unfused (fp contract off), so every float equals the host's in every bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "frame_queue.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::FqArgs;

constexpr uint32_t kFqBlocksMax = 1u << 16;  // the waves stride over the connections beyond
static_assert(sizeof(ufc_sent_frame) == 24 && sizeof(ufc_frame_queue) == 192 && sizeof(ufc_frame_queue_step) == 40 &&
                  sizeof(ufc_frame_queue_result) == 80,
              "record layouts");

// One wave per connection.  The 17 arguments are read from the kernel-argument segment (wave_dev.hpp).
__global__ __launch_bounds__(64) void fq_step_kernel(FqArgs) {
  __shared__ ufc_codec::FqWaveShared sh;
  const FqArgs& a = kernargs<FqArgs>();
  for (uint64_t c = blockIdx.x; c < a.n_queues; c += gridDim.x) ufc_codec::fq_step(DevWave{}, sh, a, c);
}

}  // namespace

hipError_t queue_batch(const FqArgs& a, hipStream_t stream) {
  const unsigned blocks = (unsigned)std::min<uint64_t>(a.n_queues, kFqBlocksMax);
  fq_step_kernel<<<blocks, 64, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace ufc_dev
