// The pack core (uflow_amd/csrc/frame_codec_core.hpp: pack_overhead, pack_max_count, pack_frame_takes,
// pack_stop, pack_data_hop, pack_frame_info) as host code under AddressSanitizer and UBSan.  Seeded flushes
// are packed twice: by the emitters' loop of src/half_connection/emit.rs:47-125, 170-211, restated here item
// by item with plain comparisons (none of the core's predicates), and by the parallel form the GPU pack
// takes (frame_pack.hip): prefix sums of exactly n_items + 1 words, one hop per item, the chain of starts,
// their ranks, the stop predicate evaluated at every item of the flush, the records from hop and stop.  Both
// must agree in every frame and every result field, and F(i) must never decrease along a flush.
// Then the same flushes go through a third form, the kernels' own tiling written out lane by lane (tile_chain
// and hops_staged below): the hops from a workgroup's 256 + 128 staged prefix sums, the chain in tiles of 256
// items over four slots of 64 lanes, the starts marked by pointer doubling in two LDS rows that keep the flush
// before's garbage, the ranks from one ballot per slot and the count carried from slot to slot, the stop by
// find-first, the exit carried into the next tile; once with the lanes of a phase forwards and once backwards.
// directed_cases() places starts, stops and frame ends on lane 63, on lane 0 of the next slot and on item 0 of
// the next tile (tests/pack_expect.py lane_cases, the same numbers) and compares with literals as well.
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

// ---- the kernels' tiling, lane by lane ----

constexpr uint32_t kTile = 256, kSlots = kTile / 64, kHopThreads = 256, kHopWindow = 128;

// pack_hops_kernel over the whole batch: every workgroup stages kHopThreads + kHopWindow prefix sums, the index
// capped at n_items, and its items' hops read the staged ones alone (an index past them is a sanitizer report).
void hops_staged(const uint64_t* P, uint64_t n_items, uint8_t* out) {
  for (uint64_t base = 0; base < n_items; base += kHopThreads) {
    uint64_t* sP = new uint64_t[kHopThreads + kHopWindow];
    for (uint32_t t = 0; t < kHopThreads + kHopWindow; t++) sP[t] = P[base + t < n_items ? base + t : n_items];
    for (uint32_t t = 0; t < kHopThreads && base + t < n_items; t++) {
      const uint64_t i = base + t;
      out[i] = (uint8_t)ufc_codec::pack_data_hop([&](uint64_t k) -> uint64_t { return sP[k - base]; }, i, n_items);
    }
    delete[] sP;
  }
}

struct Lds {  // one wave's rows; never cleared between flushes, as on the device
  uint16_t nx[kTile];
  uint8_t mk[kTile];
};

struct Tiled {
  uint32_t frame_count;
  uint64_t stop;
  uint32_t why;
  int64_t alloc_left;
};

int popc(uint64_t m) { return __builtin_popcountll(m); }

// pack_chain_kernel<kEmit> for one flush.  kEmit: end = first + items_packed, infos the flush's own records
// (exactly frame_count of them).
template <bool kEmit>
Tiled tile_chain(const ufc_flush& fl, uint64_t first, uint64_t end, const uint64_t* P, const uint8_t* hops, bool backwards,
                 Lds& lds, ufc_frame_info* infos) {
  auto lanes = [&](auto&& f) {
    if (backwards)
      for (uint32_t l = 64; l-- > 0;) f(l);
    else
      for (uint32_t l = 0; l < 64; l++) f(l);
  };
  uint16_t* nx = lds.nx;
  uint8_t* mk = lds.mk;
  const bool ack = ufc_codec::pack_is_ack(fl);
  const uint32_t H = ufc_codec::pack_overhead(ack);
  const uint64_t P0 = ack ? 0 : P[first];
  uint64_t cur = first, stop = end;
  uint32_t k = 0, why = UFC_PACK_DONE;
  bool stopped = false;
  for (uint64_t t0 = first; t0 < end && !stopped; t0 += kTile) {
    const uint32_t nv = (uint32_t)(end - t0 < kTile ? end - t0 : kTile);
    if (cur < t0 || cur - t0 > nv) fail("cur outside the tile", (long)first, (long)t0, (long)cur);
    const uint32_t cur_rel = (uint32_t)(cur - t0);
    uint32_t hop[kSlots][64], nj[kSlots][64];
    lanes([&](uint32_t lane) {
      for (uint32_t r = 0; r < kSlots; r++) {
        const uint32_t jj = r * 64 + lane;
        hop[r][lane] = 0;
        if (jj < nv) {
          hop[r][lane] = ack ? ufc_codec::kAckFrameMaxGroups : (uint32_t)hops[t0 + jj];
          nx[jj] = (uint16_t)(jj + hop[r][lane]);
          mk[jj] = jj == cur_rel ? 1 : 0;
        }
      }
    });
    for (uint32_t span = 1; span < nv; span <<= 1) {
      lanes([&](uint32_t lane) {
        for (uint32_t r = 0; r < kSlots; r++) {
          const uint32_t jj = r * 64 + lane;
          nj[r][lane] = 0;
          if (jj < nv) {
            const uint32_t J = nx[jj];
            nj[r][lane] = J;
            if (J < nv) {
              if (mk[jj]) mk[J] = 1;
              nj[r][lane] = nx[J];
            }
          }
        }
      });
      lanes([&](uint32_t lane) {
        for (uint32_t r = 0; r < kSlots; r++) {
          const uint32_t jj = r * 64 + lane;
          if (jj < nv) nx[jj] = (uint16_t)nj[r][lane];
        }
      });
    }
    const uint32_t exit_rel = cur_rel < nv ? nx[cur_rel] : cur_rel;
    for (uint32_t r = 0; r < kSlots; r++) {
      uint64_t mask = 0, smask = 0;
      uint32_t kk[64], y[64];
      lanes([&](uint32_t lane) {
        const uint32_t jj = r * 64 + lane;
        if (jj < nv && mk[jj] != 0) mask |= 1ull << lane;
      });
      lanes([&](uint32_t lane) {
        const uint32_t jj = r * 64 + lane;
        const uint64_t i = t0 + jj;
        const bool valid = jj < nv, m = (mask >> lane) & 1;
        kk[lane] = k + (uint32_t)popc(mask & ((1ull << lane) - 1));
        y[lane] = UFC_PACK_DONE;
        if (!kEmit) {
          if (valid && !stopped) {
            const uint64_t bytes = ack ? (uint64_t)UFC_ACK_GROUP_SIZE * (i - first) : P[i] - P0;
            y[lane] = ufc_codec::pack_stop(fl, ack, (uint64_t)H * kk[lane] + bytes, m, kk[lane]);
          }
          if (y[lane] != UFC_PACK_DONE) smask |= 1ull << lane;
        } else if (m) {
          const uint64_t next = i + hop[r][lane] < end ? i + hop[r][lane] : end;
          infos[kk[lane]] = ufc_codec::pack_frame_info(fl, ack, kk[lane], kk[lane], nullptr, i, (uint32_t)(next - i));
        }
      });
      if (!kEmit && smask != 0 && !stopped) {
        const uint32_t l = (uint32_t)__builtin_ctzll(smask);
        stop = t0 + r * 64 + l;
        why = y[l];
        k = kk[l];
        stopped = true;
      }
      if (!stopped) k += (uint32_t)popc(mask);
    }
    cur = t0 + exit_rel < end ? t0 + exit_rel : end;
  }
  const uint64_t bytes = ack ? (uint64_t)UFC_ACK_GROUP_SIZE * (stop - first) : P[stop] - P0;
  return Tiled{k, stop, why, fl.flush_alloc - (int64_t)((uint64_t)H * k + bytes)};
}

Lds lds_rows[2];  // [lanes backwards]: garbage at first, then whatever the flush before left

void init_lds() {
  for (Lds& l : lds_rows)
    for (uint32_t t = 0; t < kTile; t++) l.nx[t] = (uint16_t)rnd(), l.mk[t] = (uint8_t)rnd();
}

// One flush [a, b) of the batch through both launches of the tiled form, lanes forwards and backwards, against
// the emitters' loop.
void check_tiled(const ufc_flush& fl, uint64_t a, uint64_t b, const uint64_t* P, const uint8_t* hops, const Packed& ref) {
  for (int backwards = 0; backwards < 2; backwards++) {
    Lds& lds = lds_rows[backwards];
    const Tiled t = tile_chain<false>(fl, a, b, P, hops, backwards != 0, lds, nullptr);
    if (t.why != ref.stop || t.stop - a != ref.pushed || t.frame_count != ref.frames.size() || t.alloc_left != ref.alloc)
      fail("tiled result", (long)t.why, (long)(t.stop - a), (long)t.frame_count);
    checks++;
    if (t.frame_count == 0) continue;
    ufc_frame_info* infos = new ufc_frame_info[t.frame_count];  // exact: a rank past the count is a report
    for (uint32_t k = 0; k < t.frame_count; k++) infos[k] = ufc_frame_info{};
    tile_chain<true>(fl, a, t.stop, P, hops, backwards != 0, lds, infos);
    const bool ack = ufc_codec::pack_is_ack(fl);
    for (uint32_t k = 0; k < t.frame_count; k++) {
      if (infos[k].ok != 1 || infos[k].item_first != a + ref.frames[k].first || infos[k].item_count != ref.frames[k].count ||
          infos[k].f[0] != (ack ? fl.id0 : fl.id0 + k))
        fail("tiled frame", (long)k, (long)(infos[k].item_first - a), (long)infos[k].item_count);
      checks++;
    }
    delete[] infos;
  }
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
  uint8_t* staged = new uint8_t[n_items ? n_items : 1];
  hops_staged(P, n_items, staged);
  for (uint64_t i = 0; i < n_items; i++)
    if (staged[i] != hops[i]) fail("staged hop", (long)i, staged[i], hops[i]);
  delete[] staged;
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
    check_tiled(fl, a, b, P, hops, ref);
    g += frame_count;
    checks++;
  }
  delete[] items;
  delete[] P;
  delete[] hops;
  delete[] sizes;
}

// ---- directed cases (tests/pack_expect.py lane_cases, the same numbers) ----

ufc_item dgram(uint32_t len) {
  ufc_item d{};
  d.data_len = len;
  return d;
}
std::vector<ufc_item> rep(const ufc_item& d, size_t n) { return std::vector<ufc_item>(n, d); }
std::vector<ufc_item> operator+(std::vector<ufc_item> a, const std::vector<ufc_item>& b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

// One flush of `mine` behind `at` items of 800 bytes (another flush's) and in front of `tail`, in exactly-sized
// arrays: the emitters' loop, and the tiled form checked against it.  The hops are the staged ones.
Packed directed(const std::vector<ufc_item>& mine, bool ack, int64_t flush_alloc, uint32_t window_room, uint32_t at,
                const std::vector<ufc_item>& tail = {}) {
  const std::vector<ufc_item> all = rep(dgram(800), at) + mine + tail;
  const uint64_t n_items = all.size(), a = at, b = at + mine.size(), n = mine.size();
  uint64_t* P = new uint64_t[n_items + 1];
  uint8_t* hops = new uint8_t[n_items ? n_items : 1];
  uint64_t* sizes = new uint64_t[n ? n : 1];
  P[0] = 0;
  for (uint64_t i = 0; i < n_items; i++) P[i + 1] = P[i] + ufc_codec::datagram_encoded_size(all[i]);
  for (uint64_t i = 0; i < n; i++) sizes[i] = ack ? 9 : P[a + i + 1] - P[a + i];
  hops_staged(P, n_items, hops);
  for (uint64_t i = 0; i < n_items; i++)
    if (hops[i] != ufc_codec::pack_data_hop([&](uint64_t k) -> uint64_t { return P[k]; }, i, n_items))
      fail("directed: staged hop", (long)i, hops[i], (long)n_items);
  ufc_flush fl{};
  fl.kind = ack ? UFC_FRAME_ACK : UFC_FRAME_DATA;
  fl.flush_alloc = flush_alloc;
  fl.window_room = window_room;
  fl.id0 = 0xFFFFFF00u + at;
  const Packed ref = reference_pack(sizes, n, ack, flush_alloc, window_room);
  check_tiled(fl, a, b, P, hops, ref);
  delete[] P;
  delete[] hops;
  delete[] sizes;
  return ref;
}

// The literals: the stop, the items pushed, and the frames as (first start, stride, count of all but the
// last, frames, count of the last).
void want(const char* what, long tag, const Packed& r, uint32_t stop, uint64_t pushed, size_t frames) {
  if (r.stop != stop || r.pushed != pushed || r.frames.size() != frames) fail(what, tag, (long)r.stop, (long)r.pushed);
  checks++;
}
void want_frames(const char* what, long tag, const Packed& r, const std::vector<Frame>& f) {
  if (r.frames.size() != f.size()) fail(what, tag, (long)r.frames.size(), (long)f.size());
  for (size_t k = 0; k < f.size(); k++)
    if (r.frames[k].first != f[k].first || r.frames[k].count != f[k].count)
      fail(what, tag, (long)k, (long)r.frames[k].first);
  checks++;
}
std::vector<Frame> ones(uint32_t n) {
  std::vector<Frame> f;
  for (uint32_t i = 0; i < n; i++) f.push_back({i, 1});
  return f;
}
// Frames at the given starts, each up to the next start, the last up to `end`.
std::vector<Frame> upto(const std::vector<uint64_t>& starts, size_t n, uint64_t end) {
  std::vector<Frame> f;
  for (size_t k = 0; k < n; k++) f.push_back({starts[k], (uint32_t)((k + 1 < n ? starts[k + 1] : end) - starts[k])});
  return f;
}

void directed_cases() {
  const int64_t kNoLimit = (int64_t)1 << 40;
  const uint32_t kRoom = 1u << 20;
  const ufc_item big = dgram(800), five = dgram(5);
  const uint64_t sz[] = {ufc_codec::datagram_encoded_size(big), ufc_codec::datagram_encoded_size(five),
                         ufc_codec::datagram_encoded_size(dgram(16)), ufc_codec::datagram_encoded_size(dgram(67)),
                         ufc_codec::datagram_encoded_size(dgram(0))};
  if (sz[0] != 814 || sz[1] != 11 || sz[2] != 22 || sz[3] != 76 || sz[4] != 6) fail("directed: sizes", (long)sz[0], (long)sz[1], 0);
  std::vector<ufc_item> sixty_four;
  for (int f = 0; f < 9; f++) sixty_four = sixty_four + rep(dgram(16), 63) + rep(dgram(67), 1);
  const std::vector<uint64_t> data_starts = {0, 127, 254, 381, 508}, ack_starts = {0, 161, 322, 483};
  for (uint32_t at : {0u, 7u}) {
    for (uint32_t n : {64u, 128u, 255u, 256u, 257u, 512u, 513u}) {  // every_item_a_start
      const Packed r = directed(rep(big, n), false, kNoLimit, kRoom, at);
      want("every_item_a_start", n, r, UFC_PACK_DONE, n, n);
      want_frames("every_item_a_start", n, r, ones(n));
    }
    for (uint32_t room : {63u, 64u, 65u, 127u, 128u, 191u, 192u, 255u, 256u, 257u, 511u, 512u}) {  // window_stop_at
      const Packed r = directed(rep(big, 600), false, kNoLimit, room, at);
      want("window_stop_at", room, r, UFC_PACK_WINDOW_LIMITED, room, room);
      want_frames("window_stop_at", room, r, ones(room));
    }
    for (int ack = 0; ack < 2; ack++) {  // size_stop_at, ack_stops
      const std::vector<uint64_t>& starts = ack ? ack_starts : data_starts;
      const uint64_t unit = ack ? 9 : 11, H = ack ? 15 : 10;
      const std::vector<uint32_t> stops = ack ? std::vector<uint32_t>{63, 64, 161, 255, 256, 322}
                                              : std::vector<uint32_t>{63, 64, 127, 128, 191, 192, 254, 255, 256, 257, 381, 511, 512};
      for (uint32_t i : stops) {
        size_t before = 0, through = 0;
        for (uint64_t s : starts) before += s < i, through += s <= i;
        const int64_t F = (int64_t)(H * before + unit * i);
        const Packed r = directed(rep(five, 600), ack != 0, F - 1, kRoom, at);
        want(ack ? "ack_stops" : "size_stop_at", i, r, UFC_PACK_SIZE_LIMITED, i, before);
        want_frames(ack ? "ack_stops" : "size_stop_at", i, r, upto(starts, before, i));
        const Packed r1 = directed(rep(five, 600), ack != 0, F, kRoom, at);
        want(ack ? "ack_stops + 1" : "size_stop_at + 1", i, r1, UFC_PACK_SIZE_LIMITED, i + 1, through);
        want_frames(ack ? "ack_stops + 1" : "size_stop_at + 1", i, r1, upto(starts, through, i + 1));
      }
    }
    {
      const Packed r = directed(rep(five, 322), true, kNoLimit, kRoom, at);  // ack_stops: exactly 2 * 161 groups
      want_frames("ack 2 x 161", at, r, {{0, 161}, {161, 161}});
    }
    for (uint32_t n : {576u, 256u, 257u}) {  // frames_of_64_exact, whole and cut at a tile's end and one past it
      const Packed r = directed(std::vector<ufc_item>(sixty_four.begin(), sixty_four.begin() + n), false, kNoLimit, kRoom, at);
      std::vector<uint64_t> starts;
      for (uint64_t s = 0; s < n; s += 64) starts.push_back(s);
      want("frames_of_64_exact", n, r, UFC_PACK_DONE, n, starts.size());
      want_frames("frames_of_64_exact", n, r, upto(starts, starts.size(), n));
    }
    {  // start_at_255_straddles, and the frame that covers the part-tile
      Packed r = directed(rep(big, 255) + rep(dgram(700), 1) + rep(five, 39) + rep(big, 5), false, kNoLimit, kRoom, at);
      std::vector<Frame> f = ones(255);
      f.push_back({255, 40});
      for (uint32_t i = 295; i < 300; i++) f.push_back({i, 1});
      want_frames("start_at_255_straddles", at, r, f);
      r = directed(rep(big, 230) + rep(dgram(700), 1) + rep(five, 65), false, kNoLimit, kRoom, at);
      f = ones(230);
      f.push_back({230, 66});
      want_frames("start_at_255_straddles, covers", at, r, f);
    }
  }
  // hop_window_seams: zero-length datagrams, hop 127 by count
  const ufc_item zero = dgram(0);
  for (uint32_t at : {129u, 255u}) {
    const Packed r = directed(rep(zero, 300), false, kNoLimit, kRoom, at, rep(big, 3));
    want_frames("hop_window_seams", at, r, {{0, 127}, {127, 127}, {254, 46}});
  }
  {
    const Packed r = directed(rep(zero, 100), false, kNoLimit, kRoom, 156, rep(big, 5));  // the follower starts at 256
    want_frames("hop_window_seams, followed", 156, r, {{0, 100}});
    const Packed l = directed(rep(zero, 130), false, kNoLimit, kRoom, 127);  // last in the batch: 257 items
    want_frames("hop_window_seams, last", 127, l, {{0, 127}, {127, 3}});
  }
  want_frames("batch_ends_on_size", 255, directed(rep(big, 2), false, kNoLimit, kRoom, 255), {{0, 1}, {1, 1}});
  {  // short_beside_long: the four flushes one after the other on the same LDS rows
    want_frames("short_beside_long 0", 0, directed(rep(five, 3), false, kNoLimit, kRoom, 0), {{0, 3}});
    want_frames("short_beside_long 1", 0, directed(rep(big, 513), false, kNoLimit, kRoom, 3), ones(513));
    want_frames("short_beside_long 2", 0, directed({}, false, kNoLimit, kRoom, 4), {});
    want_frames("short_beside_long 3", 0, directed(std::vector<ufc_item>(sixty_four.begin(), sixty_four.begin() + 257), false,
                                                   kNoLimit, kRoom, 4),
                {{0, 64}, {64, 64}, {128, 64}, {192, 64}, {256, 1}});
  }
}

}  // namespace

int main() {
  init_lds();
  directed_cases();
  check_batch(0, 3);
  check_batch(1, 1);
  for (int r = 0; r < 60; r++) check_batch(1 + rnd() % 3000, 1 + rnd() % 40);
  std::printf("ok: %ld\n", checks);
  return 0;
}
