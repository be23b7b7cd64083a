// scratch.hpp -- the device scratch of a batched call: where a *_batch function (the .hip files) gets it, and how it
// lays its parts out.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct ufc_ctx;

namespace ufc_dev {

// "Give me N bytes": the context's grow-only scratch buffer of one (kind, stream), handed to a *_batch function by
// its C-ABI wrapper (ufc_api.cpp, which defines get).  A call asks once, for the end of its plan.
struct ScratchSource {
  ufc_ctx* ctx;
  int kind;
  hipStream_t stream;
  hipError_t get(size_t bytes, char** out) const;
};

// The parts of a call's scratch, one after the other in the order taken, each at a 256-byte aligned offset.
struct ScratchPlan {
  uint64_t end = 0;  // the bytes planned so far
  uint64_t take(uint64_t bytes) {
    const uint64_t at = end;
    end += (bytes + 255) / 256 * 256;
    return at;
  }
};

}  // namespace ufc_dev
