// send_rate.hip -- batched TFRC send rate step and flush allocation on device-resident records
// (ufc_rate_begin_varlen, ufc_rate_step_varlen, include/uflow_frame_codec.h): the two calls around
// frame_queue.hip's that close a sender's tick without the host.
//
// The step's code is frame_codec_core.hpp's rate_step, shared with the host.  One lane runs a connection: the work
// is a few dozen double operations and a handful of set entries, so a wave per connection would idle 63 lanes.
// The cost is memory.  A lane that read its own 112-byte state would turn every load into a gather with a stride
// of 112 bytes, so a wave (one block) moves a tile of 64 states, ticks and frame queue results through LDS: the
// global side is read and written as consecutive 8-byte words, lane after lane, and each lane then takes its own
// record from an LDS row.  A row is padded to an odd number of dwords, so the 64 lanes that read the same field
// hit 64 different banks.  The entries of the receive-rate set and the two flush gathers are touched per lane.
// The bisection of the first loss diverges (5 or 6 rounds as a rule, about 1,100 at the very worst) and stays in
// line.  Past the launch grid the blocks stride over the tiles.  The file is compiled without fast-math and the
// core keeps every float operation unfused, so every double equals the host's in every bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_codec_core.hpp"
#include "send_rate.hpp"
#include "wave_dev.hpp"

namespace ufc_dev {

namespace {

using ufc_codec::RateArgs;
using ufc_codec::RateBeginArgs;

constexpr uint32_t kRateTile = 64;             // connections per wave
constexpr uint32_t kRateBlocksMax = 1u << 12;  // 262,144 lanes; the blocks stride over the tiles beyond
static_assert(sizeof(ufc_recv_rate_entry) == 16 && sizeof(ufc_rate_state) == 112 && sizeof(ufc_rate_tick) == 32 &&
                  sizeof(ufc_rate_result) == 56 && sizeof(ufc_frame_queue_result) == 80 &&
                  sizeof(ufc_frame_queue_step) == 40,
              "record layouts");

// A tile of `cnt` records of type T between global memory and LDS rows of kRow dwords.
template <class T>
struct Staged {
  static constexpr uint32_t kWords = sizeof(T) / 8, kDwords = sizeof(T) / 4;
  static constexpr uint32_t kRow = kDwords | 1u;  // odd: lane l's field k lies in bank (l * kRow + k) % 64
  static_assert(sizeof(T) % 8 == 0 && alignof(T) <= 8, "records are moved as 8-byte words");
  uint32_t rows[kRateTile * kRow];

  // Word w of the tile (consecutive in global memory) belongs to record w / kWords.
  __device__ __forceinline__ void load(const T* g, uint32_t cnt, uint32_t lane) {
    const uint2* src = reinterpret_cast<const uint2*>(g);
    const uint32_t total = cnt * kWords;
#pragma unroll
    for (uint32_t k = 0; k < kWords; k++) {
      const uint32_t w = k * kRateTile + lane;
      if (w < total) {
        const uint2 v = src[w];
        const uint32_t r = w / kWords, col = w % kWords;
        rows[r * kRow + 2 * col] = v.x;
        rows[r * kRow + 2 * col + 1] = v.y;
      }
    }
  }
  __device__ __forceinline__ void store(T* g, uint32_t cnt, uint32_t lane) const {
    uint2* dst = reinterpret_cast<uint2*>(g);
    const uint32_t total = cnt * kWords;
#pragma unroll
    for (uint32_t k = 0; k < kWords; k++) {
      const uint32_t w = k * kRateTile + lane;
      if (w < total) {
        const uint32_t r = w / kWords, col = w % kWords;
        dst[w] = make_uint2(rows[r * kRow + 2 * col], rows[r * kRow + 2 * col + 1]);
      }
    }
  }
  __device__ __forceinline__ T get(uint32_t lane) const {
    uint32_t w[kDwords];
#pragma unroll
    for (uint32_t k = 0; k < kDwords; k++) w[k] = rows[lane * kRow + k];
    T t;
    __builtin_memcpy(&t, w, sizeof(T));
    return t;
  }
  __device__ __forceinline__ void put(uint32_t lane, const T& t) {
    uint32_t w[kDwords];
    __builtin_memcpy(w, &t, sizeof(T));
#pragma unroll
    for (uint32_t k = 0; k < kDwords; k++) rows[lane * kRow + k] = w[k];
  }
};

// One wave per block and a tile of 64 connections per round.  The state rows serve states_out and the frame
// queue result rows the results on the way back; a tile is read completely before any of it is written, and the
// tiles are disjoint, so states_out may be `states`.
// The 14 arguments are read from the kernel-argument segment (wave_dev.hpp): held in scalar registers through the
// step they spilled.
__global__ __launch_bounds__(64) void rate_step_kernel(RateArgs) {
  const RateArgs& a = kernargs<RateArgs>();
  __shared__ Staged<ufc_rate_state> st;
  __shared__ Staged<ufc_rate_tick> tk;
  __shared__ union {
    Staged<ufc_frame_queue_result> fq;
    Staged<ufc_rate_result> res;
  } io;
  const uint32_t lane = threadIdx.x;
  const uint64_t tiles = (a.n + kRateTile - 1) / kRateTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t c0 = t * kRateTile;
    const uint32_t cnt = a.n - c0 < kRateTile ? (uint32_t)(a.n - c0) : kRateTile;
    st.load(a.states + c0, cnt, lane);
    tk.load(a.ticks + c0, cnt, lane);
    io.fq.load(a.fq + c0, cnt, lane);
    __syncthreads();
    ufc_rate_state S;
    ufc_rate_result R;
    if (lane < cnt) {
      S = st.get(lane);
      const ufc_rate_tick T = tk.get(lane);
      const ufc_frame_queue_result F = io.fq.get(lane);
      ufc_codec::rate_step(a, c0 + lane, S, T, F, R);
    }
    __syncthreads();  // (every lane has taken its frame queue result: the rows now hold the results)
    if (lane < cnt) {
      st.put(lane, S);
      io.res.put(lane, R);
    }
    __syncthreads();
    st.store(a.states_out + c0, cnt, lane);
    io.res.store(a.results + c0, cnt, lane);
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void rate_begin_kernel(const RateBeginArgs a) {
  __shared__ Staged<ufc_rate_state> st;
  __shared__ Staged<ufc_frame_queue_step> sp;
  const uint32_t lane = threadIdx.x;
  const uint64_t tiles = (a.n + kRateTile - 1) / kRateTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t c0 = t * kRateTile;
    const uint32_t cnt = a.n - c0 < kRateTile ? (uint32_t)(a.n - c0) : kRateTile;
    st.load(a.states + c0, cnt, lane);
    __syncthreads();
    if (lane < cnt) {
      ufc_rate_state S = st.get(lane);
      ufc_frame_queue_step Q;
      ufc_codec::rate_begin(S, a.now_ms[c0 + lane], a.extra_flags ? a.extra_flags[c0 + lane] : 0, Q);
      st.put(lane, S);
      sp.put(lane, Q);
    }
    __syncthreads();
    st.store(a.states_out + c0, cnt, lane);
    sp.store(a.steps + c0, cnt, lane);
    __syncthreads();
  }
}

unsigned rate_blocks(size_t n) {
  return (unsigned)std::min<uint64_t>((n + kRateTile - 1) / kRateTile, kRateBlocksMax);
}

}  // namespace

hipError_t rate_begin_batch(const RateBeginArgs& a, hipStream_t stream) {
  rate_begin_kernel<<<rate_blocks(a.n), kRateTile, 0, stream>>>(a);
  return hipGetLastError();
}

hipError_t rate_step_batch(const RateArgs& a, hipStream_t stream) {
  rate_step_kernel<<<rate_blocks(a.n), kRateTile, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace ufc_dev
