// scan.hpp -- the exclusive sum the batched calls put between their launches (hipcub's DeviceScan), for the host
// side of the .hip files.  The counts are 32-bit: every caller's n is below 2^31 (the C-ABI wrappers check).
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstddef>
#include <cstdint>

namespace ufc_dev {

template <class T>
size_t scan_temp_bytes(uint64_t n) {  // the temporaries of an exclusive sum over n values of type T
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (T*)nullptr, (T*)nullptr, (int)n);
  return bytes;
}

// out[i] = in[0] + ... + in[i - 1] for i < n; `out` may be `in`.
template <class T>
hipError_t exclusive_sum(void* temp, size_t temp_bytes, T* in, T* out, uint64_t n, hipStream_t stream) {
  return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)n, stream);
}

}  // namespace ufc_dev
