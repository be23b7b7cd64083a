// resend.hip -- batched resend on device-resident records: packet acks, the resend heap and the pending queue of
// many connections around the emit and the pack (ufc_resend_begin_varlen, ufc_resend_place_varlen,
// ufc_resend_commit_varlen, include/uflow_frame_codec.h).
//
// The steps are frame_codec_core.hpp's rs_begin, rs_place and rs_commit, shared with the host (where a phase is a loop
// over the lanes).  One wave runs a connection, as in frame_queue.hip: the running state is the same in every lane;
// the live refs, the slots acknowledge frees (wave sums and a ballot), the pending fragments' items, and commit's
// table entries, ack bytes and refs take a lane per record; the heap operations and the pack rule are a dependent
// chain of loads and run in lane 0, the other lanes waiting at the wave barrier behind it.  No output needs a scan,
// so each call is one launch and uses no scratch; past the launch grid the waves stride over the connections.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "resend.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::RsBeginArgs;
using ufc_codec::RsCommitArgs;
using ufc_codec::RsPlaceArgs;

constexpr uint32_t kRsBlocksMax = 1u << 16;  // the waves stride over the connections beyond
static_assert(sizeof(ufc_resend_entry) == 16 && sizeof(ufc_sent_packet) == 24 && sizeof(ufc_tx_ref) == 8 &&
                  sizeof(ufc_resend) == 104 && sizeof(ufc_resend_result) == 48 && sizeof(ufc_resend_commit_result) == 40,
              "record layouts");

// The arguments are read from the kernel-argument segment (wave_dev.hpp), as fq_step_kernel reads its own.
__global__ __launch_bounds__(64) void rs_begin_kernel(RsBeginArgs) {
  __shared__ ufc_codec::RsWaveShared sh;
  const RsBeginArgs& a = kernargs<RsBeginArgs>();
  for (uint64_t c = blockIdx.x; c < a.n; c += gridDim.x) ufc_codec::rs_begin(DevWave{}, sh, a, c);
}

__global__ __launch_bounds__(64) void rs_place_kernel(RsPlaceArgs a) {
  for (uint64_t c = blockIdx.x; c < a.n; c += gridDim.x) ufc_codec::rs_place(DevWave{}, a, c);
}

__global__ __launch_bounds__(64) void rs_commit_kernel(RsCommitArgs) {
  __shared__ ufc_codec::RsWaveShared sh;
  const RsCommitArgs& a = kernargs<RsCommitArgs>();
  for (uint64_t c = blockIdx.x; c < a.n; c += gridDim.x) ufc_codec::rs_commit(DevWave{}, sh, a, c);
}

// The other grouping of the same steps: a lane per connection.  A phase is a loop in the lane, as on the host, so a
// wave has 64 heap walks in flight in place of one, and pays for it with uncoalesced records, 64 shared blocks (18 KiB
// of LDS) and lanes that diverge.  Measured (profiles/EXPERIMENTS.md): 3.7 times faster at 250,000 connections, where
// the wave form leaves 63 lanes of every wave waiting on one chain; twice slower at 2,048, which are 32 waves on 256
// CUs.  So the launch takes this form from kRsLaneFrom connections on; -DUFC_RS_FORM=1 / =2 builds a library with
// the wave / the lane form alone (tools/build_variant.py, for the A/B).  The policy is the serial one (wave.hpp).
__global__ __launch_bounds__(64) void rs_begin_lane_kernel(RsBeginArgs) {
  __shared__ ufc_codec::RsWaveShared sh[64];
  const RsBeginArgs& a = kernargs<RsBeginArgs>();
  for (uint64_t c = (uint64_t)blockIdx.x * 64 + threadIdx.x; c < a.n; c += (uint64_t)gridDim.x * 64)
    ufc_codec::rs_begin(ufc_codec::SerialWave{}, sh[threadIdx.x], a, c);
}

__global__ __launch_bounds__(64) void rs_commit_lane_kernel(RsCommitArgs) {
  __shared__ ufc_codec::RsWaveShared sh[64];
  const RsCommitArgs& a = kernargs<RsCommitArgs>();
  for (uint64_t c = (uint64_t)blockIdx.x * 64 + threadIdx.x; c < a.n; c += (uint64_t)gridDim.x * 64)
    ufc_codec::rs_commit(ufc_codec::SerialWave{}, sh[threadIdx.x], a, c);
}

#if !defined(UFC_RS_FORM)
#define UFC_RS_FORM 0
#endif
constexpr uint64_t kRsLaneFrom = 16384;  // between the two measured groupings: see profiles/EXPERIMENTS.md
inline bool rs_lane_form(uint64_t n) { return UFC_RS_FORM == 2 || (UFC_RS_FORM == 0 && n >= kRsLaneFrom); }

}  // namespace

hipError_t resend_begin_batch(const RsBeginArgs& a, hipStream_t stream) {
  if (rs_lane_form(a.n))
    rs_begin_lane_kernel<<<(unsigned)std::min<uint64_t>((a.n + 63) / 64, kRsBlocksMax), 64, 0, stream>>>(a);
  else
    rs_begin_kernel<<<(unsigned)std::min<uint64_t>(a.n, kRsBlocksMax), 64, 0, stream>>>(a);
  return hipGetLastError();
}

hipError_t resend_place_batch(const RsPlaceArgs& a, hipStream_t stream) {
  rs_place_kernel<<<(unsigned)std::min<uint64_t>(a.n, kRsBlocksMax), 64, 0, stream>>>(a);
  return hipGetLastError();
}

hipError_t resend_commit_batch(const RsCommitArgs& a, hipStream_t stream) {
  if (rs_lane_form(a.n))
    rs_commit_lane_kernel<<<(unsigned)std::min<uint64_t>((a.n + 63) / 64, kRsBlocksMax), 64, 0, stream>>>(a);
  else
    rs_commit_kernel<<<(unsigned)std::min<uint64_t>(a.n, kRsBlocksMax), 64, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace ufc_dev
