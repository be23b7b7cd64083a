// The pack core (uflow_amd/csrc/frame_codec_core.hpp: pack_overhead, pack_max_count, pack_frame_takes,
// pack_stop, pack_data_hop, pack_frame_info) as host code under AddressSanitizer and UBSan.  Seeded flushes
// are packed twice: by the emitters' loop of src/half_connection/emit.rs:47-125, 170-211, restated here item
// by item with plain comparisons (none of the core's predicates), and by the parallel form the GPU pack
// takes (frame_pack.hip): prefix sums of exactly n_items + 1 words, one hop per item, the chain of starts,
// their ranks, the stop predicate evaluated at every item of the flush, the records from hop and stop.  Both
// must agree in every frame and every result field, and F(i) must never decrease along a flush.
// Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../uflow_amd/csrc/frame_codec_core.hpp"

namespace {

long checks = 0;

void fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  std::exit(1);
}

uint64_t rng_state = 0x5EED0F1Au;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Frame {
  uint64_t first;
  uint32_t count;
};
struct Packed {
  std::vector<Frame> frames;
  uint32_t stop;
  uint64_t pushed;
  int64_t alloc;
};

// emit.rs, item by item.  sizes: the flush's encoded sizes.
Packed reference_pack(const uint64_t* sizes, uint64_t n, bool ack, int64_t flush_alloc, uint32_t window_room) {
  const int64_t overhead = ack ? 15 : 10;
  Packed r{{}, UFC_PACK_DONE, n, flush_alloc};
  bool open = false;
  uint64_t start = 0;
  int64_t size = 0;
  uint32_t count = 0;
  auto finalize = [&] {
    if (!open) return;
    r.frames.push_back({start, count});
    r.alloc -= size;
    open = false;
  };
  for (uint64_t i = 0; i < n; i++) {
    const int64_t e = (int64_t)sizes[i];
    if (open) {
      if (r.alloc - size < 0) {
        finalize();
        r.stop = UFC_PACK_SIZE_LIMITED;
        r.pushed = i;
        return r;
      }
      if (size + e > 1472 || (!ack && count >= 127)) {
        finalize();
      } else {
        size += e;
        count++;
        continue;
      }
    }
    if (r.alloc < 0) {
      r.stop = UFC_PACK_SIZE_LIMITED;
      r.pushed = i;
      return r;
    }
    if (!ack && r.frames.size() >= window_room) {
      r.stop = UFC_PACK_WINDOW_LIMITED;
      r.pushed = i;
      return r;
    }
    open = true;
    start = i;
    size = overhead + e;
    count = 1;
  }
  finalize();
  return r;
}

ufc_item random_item() {
  ufc_item d{};
  const uint32_t t = rnd() % 8;
  d.data_len = t == 0 ? 0 : t == 1 ? rnd() % 64 : t == 2 ? 63 + rnd() % 3 : t == 3 ? 254 + rnd() % 3
               : t == 4 ? 1400 + rnd() % 100 : t == 5 ? 3000 + rnd() % 60000 : rnd() % 400;
  d.window_parent_lead = (uint16_t)(rnd() % 3 == 0 ? 126 + rnd() % 4 : rnd() % 128);
  d.channel_parent_lead = (uint16_t)(rnd() % 3 == 0 ? 254 + rnd() % 4 : rnd() % 256);
  d.fragment_id_last = (uint16_t)(rnd() % 4 == 0 ? 1 + rnd() % 3 : 0);
  return d;
}

void check_batch(uint64_t n_items, uint32_t n_flushes) {
  // exactly-sized arrays: a read past P[n_items] or items[n_items - 1] is a sanitizer report
  ufc_item* items = new ufc_item[n_items ? n_items : 1];
  uint64_t* P = new uint64_t[n_items + 1];
  uint8_t* hops = new uint8_t[n_items ? n_items : 1];
  uint64_t* sizes = new uint64_t[n_items ? n_items : 1];
  const bool tiny = rnd() % 4 == 0;  // a batch of micro datagrams: hops up to the count limit
  P[0] = 0;
  for (uint64_t i = 0; i < n_items; i++) {
    items[i] = random_item();
    if (tiny) items[i].data_len = rnd() % 4, items[i].fragment_id_last = 0;
    sizes[i] = ufc_codec::datagram_encoded_size(items[i]);
    P[i + 1] = P[i] + sizes[i];
  }
  for (uint64_t i = 0; i < n_items; i++) {
    hops[i] = (uint8_t)ufc_codec::pack_data_hop([&](uint64_t k) -> uint64_t { return P[k]; }, i, n_items);
    if (hops[i] < 1 || hops[i] > 127 || i + hops[i] > n_items) fail("hop range", (long)i, hops[i], (long)n_items);
  }
  std::vector<uint64_t> first(n_flushes + 1, 0);
  for (uint32_t j = 1; j <= n_flushes; j++) first[j] = rnd() % (n_items + 1);
  first[n_flushes] = n_items;
  for (uint32_t j = 1; j < n_flushes; j++)  // nondecreasing
    if (first[j] < first[j - 1]) first[j] = first[j - 1];
  uint64_t g = 0;
  for (uint32_t j = 0; j < n_flushes; j++) {
    const uint64_t a = first[j], b = first[j + 1] < a ? a : first[j + 1], n = b - a;
    ufc_flush fl{};
    const bool ack = rnd() % 4 == 0;
    fl.kind = ack ? UFC_FRAME_ACK : UFC_FRAME_DATA;
    const uint64_t total = (ack ? 9 * n : P[b] - P[a]) + 15 * (n + 1);
    fl.flush_alloc = rnd() % 3 == 0 ? (int64_t)1 << 50 : (int64_t)(rnd() % (total + 3)) - 2;
    fl.window_room = rnd() % 2 ? 0xFFFFFFFFu : rnd() % (uint32_t)(n / 2 + 2);
    fl.id0 = rnd() | (rnd() << 16);
    fl.id1 = rnd();
    std::vector<uint64_t> fs(n);
    for (uint64_t i = 0; i < n; i++) fs[i] = ack ? 9 : sizes[a + i];
    const Packed ref = reference_pack(fs.data(), n, ack, fl.flush_alloc, fl.window_room);
    // the parallel form
    const uint32_t H = ufc_codec::pack_overhead(ack);
    std::vector<uint8_t> is_start(n + 1, 0);
    for (uint64_t s = a; s < b; s += ack ? ufc_codec::kAckFrameMaxGroups : hops[s]) is_start[s - a] = 1;
    uint64_t stop = b, prevF = 0;
    uint32_t why = UFC_PACK_DONE, starts = 0, frame_count = 0;
    std::vector<uint32_t> rank(n + 1, 0);
    for (uint64_t i = a; i < b; i++) {
      rank[i - a] = starts;
      const uint64_t F = (uint64_t)H * starts + (ack ? 9 * (i - a) : P[i] - P[a]);
      if (F < prevF) fail("F decreases", (long)j, (long)i, (long)F);
      prevF = F;
      const uint32_t y = ufc_codec::pack_stop(fl, ack, F, is_start[i - a] != 0, starts);
      if (y != UFC_PACK_DONE && stop == b && why == UFC_PACK_DONE) stop = i, why = y, frame_count = starts;
      starts += is_start[i - a];
    }
    if (why == UFC_PACK_DONE) frame_count = starts;
    const int64_t alloc_left = fl.flush_alloc - (int64_t)((uint64_t)H * frame_count + (ack ? 9 * (stop - a) : P[stop] - P[a]));
    if (why != ref.stop || stop - a != ref.pushed || frame_count != ref.frames.size() || alloc_left != ref.alloc)
      fail("result", (long)j, (long)why, (long)(stop - a));
    uint32_t k = 0;
    for (uint64_t i = a; i < stop; i++) {
      if (!is_start[i - a]) continue;
      uint64_t next = i + (ack ? ufc_codec::kAckFrameMaxGroups : hops[i]);
      if (next > stop) next = stop;
      const ufc_frame_info info = ufc_codec::pack_frame_info(fl, ack, rank[i - a], g + k, nullptr, i, (uint32_t)(next - i));
      if (rank[i - a] != k || info.item_first != a + ref.frames[k].first || info.item_count != ref.frames[k].count ||
          info.ok != 1 || info.kind != fl.kind || info.f[0] != (ack ? fl.id0 : fl.id0 + k))
        fail("frame", (long)j, (long)k, (long)i);
      k++;
      checks++;
    }
    if (k != frame_count) fail("frame count", (long)j, (long)k, (long)frame_count);
    g += frame_count;
    checks++;
  }
  delete[] items;
  delete[] P;
  delete[] hops;
  delete[] sizes;
}

}  // namespace

int main() {
  check_batch(0, 3);
  check_batch(1, 1);
  for (int r = 0; r < 60; r++) check_batch(1 + rnd() % 3000, 1 + rnd() % 40);
  std::printf("ok: %ld\n", checks);
  return 0;
}
