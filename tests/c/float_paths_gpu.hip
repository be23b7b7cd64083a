// The float helpers of the send rate control and of the frame queue's feedback (frame_codec_core.hpp), each run on
// its own, on the host or on the device, and every result written out as 64 bits: the square root and the division
// as the core's statements compile them (under the same pragma, with the flags of send_rate.hip), rate_round,
// rate_max, the three casts, rate_s_to_ms, rate_initial_send_rate, rate_update_rto, the throughput equation's value
// before its cast, its inverse (the midpoint as bits, the iterations, the stall), fq_loss_rate, fq_reset_length and
// fq_receive_rate.  The core's own text runs; nothing of it is restated here.  tests/test_float_paths.py writes the
// input file, builds this program, runs it and compares both modes with a Python reference, bit for bit.
//
//   float_paths_gpu host|device <input> <output>
//
// Input: a header {magic, count} and `count` records {op, n, a, b, len[8]}; output: `count` records {r0, r1}.  The
// device mode gives a record to a thread, the grid striding over the records; a thread touches in[i] and out[i] for
// i < count only.  Exit 0 and "ok: <count>"; a bad file or argument exits 1, a HIP error exits 2.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "frame_codec_core.hpp"

namespace {

constexpr uint64_t kMagic = 0x3153485441504C46ull;  // "FLPATHS1"

enum Op : uint32_t {
  kSqrt, kDiv, kRound, kMax, kToU32, kToU64, kToI64, kSToMs, kInitialRate, kUpdateRto, kThroughput, kThroughputInv,
  kLossRate, kResetLength, kReceiveRate, kOps
};

struct In {
  uint32_t op, n;
  uint64_t a, b;  // a double's bits or an integer, as the operation takes it
  uint32_t len[8];
};
struct Out {
  uint64_t r0, r1;
};
static_assert(sizeof(In) == 56 && sizeof(Out) == 16, "record layouts");

__host__ __device__ inline double f64(uint64_t bits) {
  double v;
  __builtin_memcpy(&v, &bits, 8);
  return v;
}
__host__ __device__ inline uint64_t bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  return b;
}
// The two primitives as a statement of the core has them.
__host__ __device__ inline double root(double x) {
#pragma clang fp contract(off)
  const double r = __builtin_sqrt(x);
  return r;
}
__host__ __device__ inline double quotient(double x, double y) {
#pragma clang fp contract(off)
  const double q = x / y;
  return q;
}

__host__ __device__ inline Out eval(const In& r) {
  using namespace ufc_codec;
  Out o{0, 0};
  const double a = f64(r.a), b = f64(r.b);
  switch (r.op) {
    case kSqrt: o.r0 = bits(root(a)); break;
    case kDiv: o.r0 = bits(quotient(a, b)); break;
    case kRound: o.r0 = bits(rate_round(a)); break;
    case kMax: o.r0 = bits(rate_max(a, b)); break;
    case kToU32: o.r0 = rate_f64_u32(a); break;
    case kToU64: o.r0 = rate_f64_u64(a); break;
    case kToI64: o.r0 = (uint64_t)rate_f64_i64(a); break;
    case kSToMs: o.r0 = rate_s_to_ms(a); break;
    case kInitialRate: o.r0 = rate_initial_send_rate(a); break;
    case kUpdateRto: {
      ufc_rate_state S{};
      o.r0 = bits(rate_update_rto(S, a, (uint32_t)r.b));
      o.r1 = S.rto_ms;
      break;
    }
    case kThroughput:
      o.r0 = bits(rate_tcp_throughput_f64(a, b));
      o.r1 = rate_tcp_throughput(a, b);
      break;
    case kThroughputInv: {
      uint32_t iterations;
      bool stalled;
      o.r0 = bits(rate_tcp_throughput_inv(a, (uint32_t)r.b, iterations, stalled));
      o.r1 = iterations | (stalled ? 1ull << 32 : 0);
      break;
    }
    case kLossRate: o.r0 = bits(fq_loss_rate(r.len, r.n <= 8 ? r.n : 8)); break;
    case kResetLength: o.r0 = fq_reset_length(a); break;
    case kReceiveRate: o.r0 = fq_receive_rate(r.a, r.b); break;
    default: o.r0 = o.r1 = ~0ull; break;
  }
  return o;
}

__global__ __launch_bounds__(256) void eval_kernel(const In* in, Out* out, uint64_t count) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = eval(in[i]);
}

#define HIP_OK(call)                                                                   \
  do {                                                                                 \
    const hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                            \
      std::printf("%s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);       \
      return 2;                                                                        \
    }                                                                                  \
  } while (0)

int run_device(const std::vector<In>& in, std::vector<Out>& out) {
  const uint64_t count = in.size();
  if (count == 0) return 0;
  In* d_in = nullptr;
  Out* d_out = nullptr;
  HIP_OK(hipMalloc(&d_in, count * sizeof(In)));
  HIP_OK(hipMalloc(&d_out, count * sizeof(Out)));
  HIP_OK(hipMemcpy(d_in, in.data(), count * sizeof(In), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_out, 0xEE, count * sizeof(Out)));
  const uint64_t blocks = (count + 255) / 256;
  eval_kernel<<<(unsigned)(blocks < 1024 ? blocks : 1024), 256>>>(d_in, d_out, count);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out.data(), d_out, count * sizeof(Out), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_out));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 || (std::strcmp(argv[1], "host") && std::strcmp(argv[1], "device"))) {
    std::printf("usage: float_paths_gpu host|device <input> <output>\n");
    return 1;
  }
  std::FILE* f = std::fopen(argv[2], "rb");
  uint64_t head[2] = {0, 0};
  if (!f || std::fread(head, 8, 2, f) != 2 || head[0] != kMagic || head[1] > (1u << 24)) {
    std::printf("bad input file\n");
    return 1;
  }
  std::vector<In> in(head[1]);
  const bool whole = std::fread(in.data(), sizeof(In), in.size(), f) == in.size() && std::fgetc(f) == EOF;
  std::fclose(f);
  if (!whole) {
    std::printf("bad input file: %llu records announced\n", (unsigned long long)head[1]);
    return 1;
  }
  std::vector<Out> out(in.size());
  if (!std::strcmp(argv[1], "host")) {
    for (size_t i = 0; i < in.size(); i++) out[i] = eval(in[i]);
  } else if (const int rc = run_device(in, out)) {
    return rc;
  }
  f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(Out), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::printf("cannot write the output file\n");
    return 1;
  }
  std::printf("ok: %zu\n", out.size());
  return 0;
}
