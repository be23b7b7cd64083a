// The frame window's core (uflow_amd/csrc/frame_codec_core.hpp: fw_walk_tiles, the form the device runs, one wave
// per connection in tiles of 64 frames) as host code under AddressSanitizer and UBSan, driven the way the GPU form
// drives it (frame_window.hip): a counting walk per connection, the exclusive sum of the counts, a writing walk;
// the lanes of a phase run one after the other, the shared block starts as garbage.  Checked against the serial
// walk (fw_walk_serial, the reference's step frame by frame) driven the same way: frame_accept, groups,
// group_first, results and windows_out must be equal byte for byte.  Seeded traffic: ordinary connections (ids in
// order with gaps of 1 to 40, duplicates and late frames, frames with ok = 0 and other kinds, syncs that advance
// and syncs that do not, packet syncs, bases near 2^32, carried tails in reach), hostile ones (ids around the
// base and all over the id space, window sizes 0 to 2^31 and beyond, syncs that let ids come back) and 24 random
// bytes of state; 0 to 200 frames per connection; frame ranges reversed or past the batch now and then.  All
// buffers have their exact sizes, the groups' once the always-enough cap and once one below the need.
// Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../uflow_amd/csrc/frame_codec_core.hpp"

namespace {

using namespace ufc_codec;

long checks = 0;

void fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  std::exit(1);
}

uint64_t rng_state = 0xF7A3E11Du;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Out {
  std::vector<uint8_t> accept;
  std::vector<ufc_item> groups;
  std::vector<uint64_t> group_first;
  std::vector<ufc_frame_window_result> results;
  std::vector<ufc_frame_window> windows_out;
  uint64_t used = 0;
};

// One call the way the device form runs it; tiled or serial.
void run(bool tiled, const std::vector<ufc_frame_info>& infos, const std::vector<uint64_t>& frame_first,
         const std::vector<ufc_frame_window>& windows, size_t cap, Out& o) {
  const size_t n = windows.size();
  o.accept.assign(infos.size(), 0xA5);
  o.groups.resize(cap);
  if (cap) std::memset((void*)o.groups.data(), 0xA5, cap * sizeof(ufc_item));
  o.group_first.assign(n + 1, 0);
  o.results.resize(n);
  o.windows_out.resize(n);
  std::memset((void*)o.results.data(), 0xA5, n * sizeof(ufc_frame_window_result));
  std::memset((void*)o.windows_out.data(), 0xA5, n * sizeof(ufc_frame_window));
  const FwArgs a{infos.data(), infos.size(), frame_first.data(), windows.data(), n, o.accept.data(), o.groups.data(), cap,
                 o.group_first.data(), &o.used, o.results.data(), o.windows_out.data()};
  std::vector<uint64_t> counts(n + 1, 0);
  auto walk = [&](uint64_t r, bool write, uint64_t gfirst) {
    if (!tiled) return fw_walk_serial(a, r, write, gfirst);
    FwWaveShared sh;
    std::memset((void*)&sh, 0xCD, sizeof sh);
    return fw_walk_tiles(SerialWave{}, sh, a, r, write, gfirst);
  };
  for (uint64_t r = 0; r < n; r++) counts[r] = walk(r, false, 0);
  uint64_t total = 0;
  for (uint64_t r = 0; r <= n; r++) {
    o.group_first[r] = total;
    total += counts[r];
  }
  o.used = total;
  for (uint64_t r = n; r-- > 0;)  // (the connections in any order: last first here)
    if (walk(r, true, o.group_first[r]) != counts[r]) fail("the two walks count differently", (long)r, tiled, 0);
}

ufc_frame_info data_frame(uint32_t id, uint32_t aux, bool ok) {
  ufc_frame_info f{};
  f.kind = UFC_FRAME_DATA;
  f.ok = ok;
  f.aux = (uint8_t)aux;
  f.f[0] = id;
  return f;
}
ufc_frame_info sync_frame(bool has_frame, uint32_t nfi, bool has_packet) {
  ufc_frame_info f{};
  f.kind = UFC_FRAME_SYNC;
  f.ok = 1;
  f.aux = (uint8_t)((has_frame ? 1 : 0) | (has_packet ? 2 : 0));
  f.f[0] = nfi;
  f.f[1] = rnd() & 0xFFFFF;
  return f;
}

void make_connection(bool hostile, uint32_t nframes, ufc_frame_window& w, std::vector<ufc_frame_info>& infos) {
  static const uint32_t sizes[] = {0, 1, 2, 7, 33, 64, 4096, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFFu};
  if (hostile) {
    for (size_t k = 0; k < sizeof w; k++) ((uint8_t*)&w)[k] = (uint8_t)rnd();
    w.size = rnd() % 8 ? sizes[rnd() % 9] : sizes[rnd() % 11];
    if (rnd() % 3 == 0) w.tail_base_id = w.base_id - rnd() % 40;
  } else {
    w = ufc_frame_window{};
    static const uint32_t tame[] = {64, 256, 4096};
    w.size = tame[rnd() % 3];
    w.base_id = rnd() % 3 == 0 ? 0xFFFFFFFFu - rnd() % 50 : (rnd() << 16) ^ rnd();
    if (rnd() % 4) {
      const uint32_t back = 1 + rnd() % 19;
      w.tail_base_id = w.base_id - back;
      w.tail_bitfield = 1u | (1u << (back - 1)) | (rnd() & ((1u << (back - 1)) - 1));
      w.tail_nonce = (uint8_t)(rnd() & 1);
      w.has_tail = 1;
    }
  }
  uint32_t next = w.base_id;
  std::vector<uint32_t> sent;
  for (uint32_t k = 0; k < nframes; k++) {
    const uint32_t u = rnd() % 100;
    if (hostile) {
      if (u < 40) {
        infos.push_back(data_frame(next + rnd() % 9 - 3, rnd() % 4, u % 11 != 0));
      } else if (u < 55) {
        infos.push_back(data_frame((rnd() << 16) ^ rnd(), rnd() & 1, true));
      } else if (u < 70) {
        infos.push_back(data_frame(next + w.size - 1 + rnd() % 3 - 1, rnd() & 1, true));
      } else if (u < 90) {
        static const int32_t steps[] = {0, 1, -1, 2};
        const uint32_t nfi = rnd() % 6 == 0 ? ((rnd() << 16) ^ rnd()) : next + (rnd() % 2 ? w.size : 0) + (uint32_t)steps[rnd() % 4];
        infos.push_back(sync_frame(u % 5 != 0, nfi, u % 2));
      } else {
        ufc_frame_info f{};
        f.kind = (uint8_t)rnd();
        f.ok = rnd() & 1;
        f.f[0] = next;
        infos.push_back(f);
      }
      // (follow the base roughly: what matters is that ids land on both sides of it)
      const ufc_frame_info& f = infos.back();
      if (f.ok && f.kind == UFC_FRAME_DATA && (uint32_t)(f.f[0] - next) < w.size) next = f.f[0] + 1;
      if (f.ok && f.kind == UFC_FRAME_SYNC && (f.aux & 1) && f.f[0] - next > 0 && f.f[0] - next <= w.size) next = f.f[0];
      continue;
    }
    if (u < 70) {
      const uint32_t gap = u < 6 ? 1 + rnd() % 40 : 0;
      infos.push_back(data_frame(next + gap, rnd() & 1, true));
      sent.push_back(next + gap);
      next += gap + 1;
    } else if (u < 78 && !sent.empty()) {
      infos.push_back(data_frame(u < 74 ? sent.back() : sent[rnd() % sent.size()], rnd() & 1, true));
    } else if (u < 82) {
      infos.push_back(data_frame(next, 1, false));
    } else if (u < 86) {
      ufc_frame_info f{};
      f.kind = UFC_FRAME_ACK;
      f.ok = 1;
      f.f[0] = next;
      infos.push_back(f);
    } else if (u < 91) {
      next += 1 + rnd() % 50;
      infos.push_back(sync_frame(true, next, u % 2));
    } else if (u < 96) {
      infos.push_back(sync_frame(true, next - rnd() % 9, false));
    } else {
      infos.push_back(sync_frame(false, 0, true));
    }
  }
}

}  // namespace

int main() {
  static const uint32_t frame_counts[] = {0, 1, 2, 63, 64, 65, 127, 128, 130, 200};
  long accepted = 0, refused = 0, groups = 0, bad = 0, syncs = 0;
  {  // size = 2^31: a sync lets id 6 in twice, into the same group; its bit is set the second time, the nonce stays
    std::vector<ufc_frame_window> w(1);
    w[0] = ufc_frame_window{};
    w[0].base_id = 5;
    w[0].size = 0x80000000u;
    const std::vector<ufc_frame_info> infos = {data_frame(5, 1, true), data_frame(6, 1, true), sync_frame(true, 7u + 0x80000000u, false),
                                               data_frame(6, 1, true), data_frame(7, 1, true), data_frame(4, 1, true)};
    const std::vector<uint64_t> ff = {0, 6};
    for (int tiled = 0; tiled < 2; tiled++) {
      Out o;
      run(tiled != 0, infos, ff, w, 7, o);
      static const uint8_t want[6] = {1, 1, 0, 1, 1, 0};
      if (std::memcmp(o.accept.data(), want, 6)) fail("ids that come back: frame_accept", tiled, 0, 0);
      if (o.used != 1 || o.groups[0].id != 5 || o.groups[0].data_offset != 7 || o.groups[0].channel_id != 1)
        fail("ids that come back: group", tiled, (long)o.groups[0].data_offset, o.groups[0].channel_id);
      checks++;
    }
  }
  for (int round = 0; round < 600; round++) {
    const uint32_t n = 1 + rnd() % 6;
    std::vector<ufc_frame_window> windows(n);
    std::vector<ufc_frame_info> infos;
    std::vector<uint64_t> frame_first(n + 1, 0);
    for (uint32_t r = 0; r < n; r++) {
      make_connection(round % 3 == 2 || rnd() % 4 == 0, frame_counts[rnd() % 10], windows[r], infos);
      frame_first[r + 1] = infos.size();
    }
    if (round % 3 == 1) {  // 24 random bytes of state on ordinary traffic
      ufc_frame_window& w = windows[rnd() % n];
      const uint32_t base = w.base_id;
      for (size_t k = 0; k < sizeof w; k++) ((uint8_t*)&w)[k] = (uint8_t)rnd();
      if (rnd() % 2) w.base_id = base, w.size = 1u << (rnd() % 32);
    }
    if (rnd() % 16 == 0) {
      // a range reversed, or past the batch (its neighbour then begins beyond the end as well)
      if (rnd() % 2) frame_first[n] = infos.size() + 1 + rnd() % 3;
      else if (n > 1) frame_first[1 + rnd() % (n - 1)] = infos.size() + 2;
    }
    Out serial, tiled;
    run(false, infos, frame_first, windows, n + infos.size(), serial);
    const size_t caps[2] = {n + infos.size(), serial.used ? (size_t)(serial.used - 1 - rnd() % serial.used) : 0};
    for (int c = 0; c < 2; c++) {
      run(false, infos, frame_first, windows, caps[c], serial);
      run(true, infos, frame_first, windows, caps[c], tiled);
      if (serial.used != tiled.used || serial.group_first != tiled.group_first) fail("tiled: group_first", round, c, 0);
      if (serial.accept != tiled.accept) fail("tiled: frame_accept", round, c, 0);
      if (caps[c] && std::memcmp((void*)serial.groups.data(), (void*)tiled.groups.data(), caps[c] * sizeof(ufc_item)))
        fail("tiled: groups", round, c, 0);
      if (std::memcmp((void*)serial.results.data(), (void*)tiled.results.data(), n * sizeof(ufc_frame_window_result)))
        fail("tiled: results", round, c, 0);
      if (std::memcmp((void*)serial.windows_out.data(), (void*)tiled.windows_out.data(), n * sizeof(ufc_frame_window)))
        fail("tiled: windows_out", round, c, 0);
      checks++;
    }
    for (uint32_t r = 0; r < n; r++) {
      const ufc_frame_window_result& q = serial.results[r];
      if (q.stop != UFC_FW_DONE) {
        bad++;
        continue;
      }
      // the verdict bytes against the counts; every group's first bit
      uint32_t ones = 0;
      for (uint64_t i = frame_first[r]; i < frame_first[r + 1]; i++) {
        if (serial.accept[i] > 1) fail("frame_accept not 0 or 1", round, r, (long)i);
        ones += serial.accept[i];
      }
      if (ones != q.accepted) fail("accepted", round, r, ones);
      if (q.advanced != serial.windows_out[r].base_id - windows[r].base_id) fail("advanced", round, r, q.advanced);
      accepted += q.accepted, refused += q.refused, groups += q.group_count, syncs += q.syncs;
      checks++;
    }
  }
  if (accepted < 20000 || refused < 5000 || groups < 2000 || bad < 20 || syncs < 3000)
    fail("too little of some kind of traffic", accepted, refused, groups);
  std::printf("ok: %ld\n", checks);
  return 0;
}
