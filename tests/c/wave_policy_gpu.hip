// The wave policies of uflow_amd/csrc/wave.hpp and wave_dev.hpp, checked directly: one templated exerciser runs under
//   - DevWave in one-wave blocks, 7 blocks striding over 100 work items with one LDS block each, as the kernels do;
//   - SerialWave inside a lane (the resend's lane form), a work item per lane, two blocks;
//   - SerialWave on the host, one shared block carried from item to item;
// and the three outputs must be equal byte for byte, and equal to values that plain loops in this file write down
// (`expected`, which uses no policy).  What the exerciser asks of a policy is what the batched steps of
// frame_codec_core.hpp ask: ballots true on lane 0 only, on lane 63 only, on lanes 31 and 32, on all lanes, on none
// and on an item's own pattern; sums of per-lane values above 2^32, one carried by lane 63 alone, one that wraps;
// or64 from all 64 lanes onto one word; add64 with carries across bit 32; a phase that writes sh[lane] and a phase
// that reads sh[63 - lane] and sh[(lane + 1) & 63]; one + sync in a loop of 100 changing values, each read by every
// lane; phases inside a loop whose trip count is read back from the shared block; high_bit, low_bit and popc on
// bits 0, 32 and 63.  Then kernargs<Args>() for a struct of FqArgs' size and for one of the largest argument
// struct's size, every field echoed.  Every index is in range by construction: lanes are 0..63, the shared words
// are 64, an item's output is kOut words of a buffer of kItems * kOut.
// Prints "ok: <words compared>" and exits 0; a difference prints its place and exits 1, a HIP error exits 2.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../uflow_amd/csrc/frame_codec_core.hpp"
#include "../../uflow_amd/csrc/wave.hpp"
#include "../../uflow_amd/csrc/wave_dev.hpp"

namespace {

using ufc_codec::high_bit;
using ufc_codec::low_bit;
using ufc_codec::popc;

constexpr uint32_t kItems = 100, kOut = 24, kWaveBlocks = 7, kLaneBlocks = 2;

struct Shared {
  unsigned long long word[64];
  uint32_t back[64];
  unsigned long long acc, total;
  uint32_t trips, value;
};

// An item's own numbers (plain arithmetic, shared by the exerciser and the plain loops).
__host__ __device__ inline uint64_t pattern(uint64_t item) {  // splitmix64 of the item: a 64-bit lane pattern
  uint64_t z = (item + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint32_t value_of(uint64_t item, uint32_t turn) { return (uint32_t)(pattern(item + 1000 * turn) >> 7); }
__host__ __device__ inline uint64_t word_of(uint64_t item, uint32_t lane) { return pattern(item) ^ ((uint64_t)lane * 0x100000001B3ull); }
__host__ __device__ inline uint32_t trips_of(uint64_t item) { return 3 + (uint32_t)(item % 5); }

// Every lane of the policy runs this; what goes to `out` is written by Wv::one.
template <class Wv>
__host__ __device__ void exercise(const Wv& wv, Shared& sh, uint64_t* out, uint64_t item) {
  const uint64_t x = pattern(item);
  const auto put = [&](uint32_t k, uint64_t v) { wv.one([&]() { out[k] = v; }); };
  // ballots
  const unsigned long long m0 = wv.ballot([&](uint32_t lane) { return lane == 0; });
  const unsigned long long m63 = wv.ballot([&](uint32_t lane) { return lane == 63; });
  const unsigned long long mid = wv.ballot([&](uint32_t lane) { return lane == 31 || lane == 32; });
  const unsigned long long all = wv.ballot([&](uint32_t) { return true; });
  const unsigned long long none = wv.ballot([&](uint32_t) { return false; });
  const unsigned long long own = wv.ballot([&](uint32_t lane) { return ((x >> lane) & 1u) != 0; });
  const unsigned long long m32 = wv.ballot([&](uint32_t lane) { return lane == 32; });
  put(0, m0), put(1, m63), put(2, mid), put(3, all), put(4, none), put(5, own);
  // sums
  put(6, wv.sum([&](uint32_t lane) -> uint64_t { return (1ull << 33) + (uint64_t)lane * (uint32_t)x; }));
  put(7, wv.sum([&](uint32_t lane) -> uint64_t { return lane == 63 ? 0xFFFFFFFF00000001ull + item : 0; }));
  put(8, wv.sum([&](uint32_t lane) -> uint64_t { return ((uint64_t)lane << 58) + (x >> lane); }));
  // or64 from all 64 lanes onto one word, then from the item's own lanes, rotated
  wv.one([&]() { sh.acc = 0; });
  wv.sync();
  wv.lanes([&](uint32_t lane) { Wv::or64(&sh.acc, 1ull << lane); });
  put(9, sh.acc);
  wv.lanes([&](uint32_t lane) {
    if (lane == 0) sh.acc = 0;
  });
  wv.lanes([&](uint32_t lane) {
    if ((x >> lane) & 1u) Wv::or64(&sh.acc, 1ull << ((lane + item) & 63u));
  });
  put(10, sh.acc);
  // add64 with carries across bit 32
  wv.one([&]() { sh.total = 0xFFFFFFF0ull + item; });
  wv.sync();
  wv.lanes([&](uint32_t lane) { Wv::add64(&sh.total, 0xFFFFFFFFull + lane); });
  put(11, sh.total);
  // a phase that writes sh[lane], a phase that reads sh[63 - lane] and sh[(lane + 1) & 63]
  wv.lanes([&](uint32_t lane) { sh.word[lane] = word_of(item, lane); });
  wv.lanes([&](uint32_t lane) { sh.back[lane] = (uint32_t)(sh.word[63 - lane] * 3 + (sh.word[(lane + 1) & 63] >> 5)); });
  put(12, wv.sum([&](uint32_t lane) -> uint64_t { return (uint64_t)sh.back[lane] * (lane + 1); }));
  put(13, wv.ballot([&](uint32_t lane) { return (sh.back[lane] & 1u) != 0; }));
  // one + sync in a loop of 100 changing values, each read by every lane
  uint64_t seen = 0;
  unsigned long long right = ~0ull;
  for (uint32_t turn = 0; turn < 100; turn++) {
    wv.one([&]() { sh.value = value_of(item, turn); });
    wv.sync();
    right &= wv.ballot([&](uint32_t) { return sh.value == value_of(item, turn); });
    seen += wv.sum([&](uint32_t lane) -> uint64_t { return (uint64_t)sh.value + lane * turn; });
  }
  put(14, right), put(15, seen);
  // phases inside a loop whose trip count is read back from the shared block
  wv.one([&]() { sh.trips = trips_of(item); });
  wv.sync();
  const uint32_t trips = sh.trips;
  for (uint32_t turn = 0; turn < trips; turn++)
    wv.lanes([&](uint32_t lane) { sh.word[lane] += (uint64_t)turn * sh.back[(lane + turn) & 63]; });
  put(16, trips);
  put(17, wv.sum([&](uint32_t lane) -> uint64_t { return sh.word[lane]; }));
  // high_bit, low_bit and popc on bits 0, 32 and 63 (masks from ballots, so that nothing folds)
  const unsigned long long three = m0 | m32 | m63;
  put(18, (uint64_t)high_bit(m0) | (uint64_t)low_bit(m0) << 8 | (uint64_t)high_bit(m32) << 16 | (uint64_t)low_bit(m32) << 24 |
              (uint64_t)high_bit(m63) << 32 | (uint64_t)low_bit(m63) << 40 | (uint64_t)popc(three) << 48 | (uint64_t)popc(all) << 56);
  put(19, (uint64_t)high_bit(three) | (uint64_t)low_bit(three) << 8 | (uint64_t)high_bit(m32 | m0) << 16 |
              (uint64_t)low_bit(m32 | m63) << 24 | (uint64_t)popc(own) << 32 | (uint64_t)high_bit(own | 1u) << 40 |
              (uint64_t)low_bit(own | 1ull << 63) << 48);
  put(20, popc(m0) + popc(m32) * 10 + popc(m63) * 100 + popc(mid) * 1000 + popc(none) * 10000);
  put(21, item);
  put(22, x);
  put(23, 0x600DF00Dull);
}

// The same values from plain loops over the lanes: no policy, no shared block.
void expected(uint64_t item, uint64_t* out) {
  const uint64_t x = pattern(item);
  out[0] = 1, out[1] = 1ull << 63, out[2] = 3ull << 31, out[3] = ~0ull, out[4] = 0, out[5] = x;
  uint64_t s6 = 0, s8 = 0;
  for (uint32_t lane = 0; lane < 64; lane++) {
    s6 += (1ull << 33) + (uint64_t)lane * (uint32_t)x;
    s8 += ((uint64_t)lane << 58) + (x >> lane);
  }
  out[6] = s6, out[7] = 0xFFFFFFFF00000001ull + item, out[8] = s8;
  out[9] = ~0ull;
  uint64_t rot = 0;
  for (uint32_t lane = 0; lane < 64; lane++)
    if ((x >> lane) & 1u) rot |= 1ull << ((lane + item) & 63u);
  out[10] = rot;
  uint64_t total = 0xFFFFFFF0ull + item;
  for (uint32_t lane = 0; lane < 64; lane++) total += 0xFFFFFFFFull + lane;
  out[11] = total;
  uint64_t word[64];
  uint32_t back[64];
  for (uint32_t lane = 0; lane < 64; lane++) word[lane] = word_of(item, lane);
  for (uint32_t lane = 0; lane < 64; lane++) back[lane] = (uint32_t)(word[63 - lane] * 3 + (word[(lane + 1) & 63] >> 5));
  uint64_t s12 = 0, b13 = 0;
  for (uint32_t lane = 0; lane < 64; lane++) {
    s12 += (uint64_t)back[lane] * (lane + 1);
    if (back[lane] & 1u) b13 |= 1ull << lane;
  }
  out[12] = s12, out[13] = b13;
  uint64_t seen = 0;
  for (uint32_t turn = 0; turn < 100; turn++)
    for (uint32_t lane = 0; lane < 64; lane++) seen += (uint64_t)value_of(item, turn) + lane * turn;
  out[14] = ~0ull, out[15] = seen;
  const uint32_t trips = trips_of(item);
  for (uint32_t turn = 0; turn < trips; turn++)
    for (uint32_t lane = 0; lane < 64; lane++) word[lane] += (uint64_t)turn * back[(lane + turn) & 63];
  uint64_t s17 = 0;
  for (uint32_t lane = 0; lane < 64; lane++) s17 += word[lane];
  out[16] = trips, out[17] = s17;
  // (positions spelled out: bit 0, bit 32, bit 63)
  out[18] = 0ull | 0ull << 8 | 32ull << 16 | 32ull << 24 | 63ull << 32 | 63ull << 40 | 3ull << 48 | 64ull << 56;
  uint32_t ones = 0, top = 0, low = 63;
  for (uint32_t lane = 0; lane < 64; lane++)
    if ((x >> lane) & 1u) ones++, top = lane;
  for (uint32_t lane = 64; lane-- > 0;)
    if ((x >> lane) & 1u) low = lane;
  out[19] = 63ull | 0ull << 8 | 32ull << 16 | 32ull << 24 | (uint64_t)ones << 32 | (uint64_t)top << 40 | (uint64_t)low << 48;
  out[20] = 1 + 10 + 100 + 2000 + 0;
  out[21] = item, out[22] = x, out[23] = 0x600DF00Dull;
}

// ---- the three forms ----
__global__ __launch_bounds__(64) void wave_form(uint64_t* out, uint32_t n_items) {
  __shared__ Shared sh;
  for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x)
    exercise(ufc_dev::DevWave{}, sh, out + (uint64_t)item * kOut, item);
}

__global__ __launch_bounds__(64) void lane_form(uint64_t* out, uint32_t n_items) {
  __shared__ Shared sh[64];
  for (uint32_t item = blockIdx.x * 64 + threadIdx.x; item < n_items; item += gridDim.x * 64)
    exercise(ufc_codec::SerialWave{}, sh[threadIdx.x], out + (uint64_t)item * kOut, item);
}

// ---- kernargs<Args>(): a struct of N 8-byte fields, the first the output, every other one echoed ----
template <uint32_t N>
struct EchoArgs {
  uint64_t* out;
  uint64_t field[N - 1];
};
template <uint32_t N>
__global__ __launch_bounds__(64) void echo(EchoArgs<N>) {
  const EchoArgs<N>& a = ufc_dev::kernargs<EchoArgs<N>>();
  for (uint32_t k = threadIdx.x; k < N - 1; k += 64) a.out[k] = a.field[k];
}

constexpr uint32_t kSmall = sizeof(ufc_codec::FqArgs) / 8, kLarge = sizeof(ufc_codec::RsCommitArgs) / 8;
static_assert(sizeof(EchoArgs<kSmall>) == sizeof(ufc_codec::FqArgs), "a struct of FqArgs' size");
static_assert(sizeof(EchoArgs<kLarge>) == sizeof(ufc_codec::RsCommitArgs), "a struct of RsCommitArgs' size");
static_assert(sizeof(ufc_codec::RsCommitArgs) >= sizeof(ufc_codec::RsBeginArgs) && sizeof(ufc_codec::RsCommitArgs) >= sizeof(ufc_codec::RxArgs) &&
                  sizeof(ufc_codec::RsCommitArgs) >= sizeof(ufc_codec::FwArgs) && sizeof(ufc_codec::RsCommitArgs) >= sizeof(ufc_codec::RateArgs),
              "RsCommitArgs is the largest argument struct");

void hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return;
  std::printf("HIP error at %s: %s\n", what, hipGetErrorString(e));
  std::exit(2);
}

template <uint32_t N>
long check_echo(uint64_t* d_out) {
  EchoArgs<N> a;
  a.out = d_out;
  for (uint32_t k = 0; k < N - 1; k++) a.field[k] = pattern(N * 1000 + k);
  hip_ok(hipMemset(d_out, 0xA5, (N - 1) * sizeof(uint64_t)), "memset");
  echo<N><<<1, 64>>>(a);
  hip_ok(hipGetLastError(), "echo launch");
  hip_ok(hipDeviceSynchronize(), "echo");
  std::vector<uint64_t> got(N - 1);
  hip_ok(hipMemcpy(got.data(), d_out, got.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "copy back");
  for (uint32_t k = 0; k < N - 1; k++)
    if (got[k] != a.field[k]) {
      std::printf("FAIL kernargs of %u fields: field %u is %016llx, not %016llx\n", N, k + 1, (unsigned long long)got[k],
                  (unsigned long long)a.field[k]);
      std::exit(1);
    }
  return N - 1;
}

}  // namespace

int main() {
  const size_t words = (size_t)kItems * kOut;
  std::vector<uint64_t> want(words), host(words, 0xA5A5A5A5A5A5A5A5ull), wave(words), lane(words);
  for (uint32_t item = 0; item < kItems; item++) expected(item, want.data() + (size_t)item * kOut);
  Shared sh;
  std::memset((void*)&sh, 0xCD, sizeof sh);
  for (uint32_t item = 0; item < kItems; item++) exercise(ufc_codec::SerialWave{}, sh, host.data() + (size_t)item * kOut, item);
  uint64_t* d_out = nullptr;
  hip_ok(hipMalloc(&d_out, words * sizeof(uint64_t)), "malloc");
  hip_ok(hipMemset(d_out, 0xA5, words * sizeof(uint64_t)), "memset");
  wave_form<<<kWaveBlocks, 64>>>(d_out, kItems);
  hip_ok(hipGetLastError(), "wave_form launch");
  hip_ok(hipDeviceSynchronize(), "wave_form");
  hip_ok(hipMemcpy(wave.data(), d_out, words * sizeof(uint64_t), hipMemcpyDeviceToHost), "copy back");
  hip_ok(hipMemset(d_out, 0xA5, words * sizeof(uint64_t)), "memset");
  lane_form<<<kLaneBlocks, 64>>>(d_out, kItems);
  hip_ok(hipGetLastError(), "lane_form launch");
  hip_ok(hipDeviceSynchronize(), "lane_form");
  hip_ok(hipMemcpy(lane.data(), d_out, words * sizeof(uint64_t), hipMemcpyDeviceToHost), "copy back");
  long compared = 0;
  const struct {
    const char* name;
    const std::vector<uint64_t>* got;
  } forms[3] = {{"SerialWave on the host", &host}, {"DevWave", &wave}, {"SerialWave inside a lane", &lane}};
  for (const auto& f : forms)
    for (size_t k = 0; k < words; k++, compared++)
      if ((*f.got)[k] != want[k]) {
        std::printf("FAIL %s: item %zu word %zu is %016llx, not %016llx\n", f.name, k / kOut, k % kOut, (unsigned long long)(*f.got)[k],
                    (unsigned long long)want[k]);
        return 1;
      }
  if (std::memcmp(host.data(), wave.data(), words * 8) || std::memcmp(host.data(), lane.data(), words * 8)) {
    std::printf("FAIL the three outputs differ\n");
    return 1;
  }
  compared += check_echo<kSmall>(d_out);
  compared += check_echo<kLarge>(d_out);
  hip_ok(hipFree(d_out), "free");
  std::printf("ok: %ld\n", compared);
  return 0;
}
