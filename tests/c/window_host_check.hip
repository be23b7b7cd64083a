// The frame window's core (uflow_amd/csrc/frame_codec_core.hpp: fw_walk_tiles, the form the device runs, one wave
// per connection in tiles of 64 frames) as host code under AddressSanitizer and UBSan, driven the way the GPU form
// drives it (frame_window.hip): a counting walk per connection, the exclusive sum of the counts, a writing walk;
// the lanes of a phase run one after the other -- forwards, backwards and in a fresh seeded permutation per phase
// (lane_orders.hpp) -- and the shared block starts as garbage, fresh for every walk or, in a fourth pass, one block
// carried from connection to connection as the kernel's grid-stride loop carries it.  Checked against the serial
// walk (fw_walk_serial, the reference's step frame by frame) driven the same way: frame_accept, groups,
// group_first, results and windows_out must be equal byte for byte.  Seeded traffic: ordinary connections (ids in
// order with gaps of 1 to 40, duplicates and late frames, frames with ok = 0 and other kinds, syncs that advance
// and syncs that do not, packet syncs, bases near 2^32, carried tails in reach), hostile ones (ids around the
// base and all over the id space, window sizes 0 to 2^31 and beyond, syncs that let ids come back) and 24 random
// bytes of state; 0 to 200 frames per connection; frame ranges reversed or past the batch now and then.  All
// buffers have their exact sizes, the groups' once the always-enough cap and once one below the need.  In front of
// the seeded traffic, directed cases that put a cross-lane read on lane 0, on lane 63 and across a tile seam
// (tests/test_window_cpu.py has the same cases as scenarios), each with its expectation spelled out.
// Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../uflow_amd/csrc/frame_codec_core.hpp"
#include "lane_orders.hpp"

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

// The forms a call runs in: the serial walk, and the tiled walk under three lane orders and with a carried block.
enum Form { kWalkSerial, kForwards, kBackwards, kShuffled, kCarried, kForms };
FwWaveShared carried_block;  // (garbage once, in main)

// One call the way the device form runs it.
void run(int form, const std::vector<ufc_frame_info>& infos, const std::vector<uint64_t>& frame_first,
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
    if (form == kWalkSerial) return fw_walk_serial(a, r, write, gfirst);
    FwWaveShared fresh;
    std::memset((void*)&fresh, 0xCD, sizeof fresh);
    FwWaveShared& sh = form == kCarried ? carried_block : fresh;
    if (form == kBackwards) return fw_walk_tiles(lane_orders::ReverseWave{}, sh, a, r, write, gfirst);
    if (form == kShuffled) return fw_walk_tiles(lane_orders::ShuffledWave{}, sh, a, r, write, gfirst);
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
    if (walk(r, true, o.group_first[r]) != counts[r]) fail("the two walks count differently", (long)r, form, 0);
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

// The serial walk, then the tiled walk in every form: every output of each equal to the serial walk's, byte for byte.
void all_forms(const char* what, long where, const std::vector<ufc_frame_info>& infos, const std::vector<uint64_t>& frame_first,
               const std::vector<ufc_frame_window>& windows, size_t cap, Out& serial) {
  const size_t n = windows.size();
  run(kWalkSerial, infos, frame_first, windows, cap, serial);
  for (int form = kForwards; form < kForms; form++) {
    Out tiled;
    run(form, infos, frame_first, windows, cap, tiled);
    if (serial.used != tiled.used || serial.group_first != tiled.group_first) fail(what, where, form, 1);
    if (serial.accept != tiled.accept) fail(what, where, form, 2);
    if (cap && std::memcmp((void*)serial.groups.data(), (void*)tiled.groups.data(), cap * sizeof(ufc_item))) fail(what, where, form, 3);
    if (std::memcmp((void*)serial.results.data(), (void*)tiled.results.data(), n * sizeof(ufc_frame_window_result)))
      fail(what, where, form, 4);
    if (std::memcmp((void*)serial.windows_out.data(), (void*)tiled.windows_out.data(), n * sizeof(ufc_frame_window)))
      fail(what, where, form, 5);
    checks++;
  }
}

ufc_frame_info filler(uint32_t k) {  // frames that are nothing to the window: a data frame not ok, an ack frame
  if (k % 2) return data_frame(6, 1, false);
  ufc_frame_info f{};
  f.kind = UFC_FRAME_ACK;
  f.ok = 1;
  f.f[0] = 6;
  return f;
}

// The cross-lane reads of fw_walk_tiles on lane 0, on lane 63 and across the tile seam (the same cases, with the
// same numbers, are scenarios of tests/test_window_cpu.py).  One connection each; the expectation is written out
// here and must also be what the serial walk gives.
void directed_cases() {
  struct Want {
    uint32_t accepted, refused, base_out, groups;
  };
  const auto one = [&](const char* what, uint32_t size, uint32_t base, const std::vector<ufc_frame_info>& infos, const Want& want,
                       Out& o, bool tail = false) {
    std::vector<ufc_frame_window> w(1);
    w[0] = ufc_frame_window{};
    w[0].base_id = base;
    w[0].size = size;
    if (tail) w[0].has_tail = 1, w[0].tail_base_id = base - 100, w[0].tail_bitfield = 1, w[0].tail_nonce = 1;
    const std::vector<uint64_t> ff = {0, infos.size()};
    all_forms(what, 0, infos, ff, w, infos.size() + 1, o);
    const ufc_frame_window_result& q = o.results[0];
    if (q.stop != UFC_FW_DONE || q.accepted != want.accepted || q.refused != want.refused || q.group_count != want.groups ||
        o.windows_out[0].base_id != want.base_out)
      fail(what, q.accepted, q.refused, (long)o.windows_out[0].base_id);
  };
  Out o;
  {  // a duplicate refused at lane 63, and once more at lane 0 of the next tile against the base carried over the seam
    std::vector<ufc_frame_info> f;
    for (uint32_t k = 0; k < 63; k++) f.push_back(data_frame(1000 + k, k & 1, true));
    f.push_back(data_frame(1062, 1, true));
    f.push_back(data_frame(1062, 1, true));
    f.push_back(data_frame(1063, 1, true));
    one("duplicate at lane 63 and over the seam", 4096, 1000, f, Want{64, 2, 1064, 2}, o);
    if (o.accept[62] != 1 || o.accept[63] != 0 || o.accept[64] != 0 || o.accept[65] != 1) fail("duplicate at lane 63: verdicts", 0, 0, 0);
  }
  {  // lane 63 folds into the open group and carries its only nonce; lane 0 of the next tile is 32 ids from the
     // group's base: it closes the group and opens the next
    std::vector<ufc_frame_info> f;
    for (uint32_t k = 0; k < 64; k++) f.push_back(data_frame(1000 + k, k == 63, true));
    f.push_back(data_frame(1064, 1, true));
    one("fold at lane 63", 4096, 1000, f, Want{65, 0, 1065, 3}, o);
    static const uint32_t want[3][3] = {{1000, 0xFFFFFFFFu, 0}, {1032, 0xFFFFFFFFu, 1}, {1064, 1, 1}};
    for (uint32_t g = 0; g < 3; g++)
      if (o.groups[g].id != want[g][0] || o.groups[g].data_offset != want[g][1] || o.groups[g].channel_id != want[g][2])
        fail("fold at lane 63: groups", g, (long)o.groups[g].data_offset, o.groups[g].channel_id);
  }
  {  // a sync at lane 63 moves the base that lane 0 of the next tile is tested against; packet syncs at lanes 5, 63
     // and at lane 1 of the next tile
    std::vector<ufc_frame_info> f;
    uint32_t next = 1000;
    for (uint32_t k = 0; k < 63; k++) {
      if (k == 5) f.push_back(sync_frame(false, 0, true));
      else f.push_back(data_frame(next++, k & 1, true));
    }
    f.push_back(sync_frame(true, next + 100, true));  // lane 63
    f.push_back(data_frame(next + 50, 1, true));      // behind the moved base: refused
    f.push_back(sync_frame(false, 0, true));
    f.push_back(data_frame(next + 100, 1, true));
    one("sync at lane 63", 4096, 1000, f, Want{63, 1, next + 101, 3}, o);
    const ufc_frame_window_result& q = o.results[0];
    if (o.accept[64] != 0 || o.accept[66] != 1 || q.first_packet_sync != 5 || q.packet_syncs != 3 || q.syncs != 3)
      fail("sync at lane 63: verdicts", o.accept[64], q.first_packet_sync, q.packet_syncs);
  }
  {  // all 64 candidates of a tile refused (65 rounds: the 65th reads fail[64]), then a tile with one refusal
    std::vector<ufc_frame_info> f;
    for (uint32_t k = 0; k < 64; k++) f.push_back(data_frame(999, k & 1, true));
    f.push_back(data_frame(1000, 1, true));
    f.push_back(data_frame(1000, 0, true));
    f.push_back(data_frame(1001, 1, true));
    one("64 refused", 64, 1000, f, Want{2, 65, 1002, 1}, o);
    if (o.accept[63] != 0 || o.accept[64] != 1 || o.accept[65] != 0 || o.accept[66] != 1) fail("64 refused: verdicts", 0, 0, 0);
    if (o.groups[0].id != 1000 || o.groups[0].data_offset != 3 || o.groups[0].channel_id != 0) fail("64 refused: group", 0, 0, 0);
  }
  {  // a carried tail out of reach and 64 accepted frames 40 ids apart: every lane closes the group before it, 64
     // group rounds with a stop test each, the most a tile takes (round k opens lane k - 1's group; stop[64] is
     // never reached)
    std::vector<ufc_frame_info> f;
    for (uint32_t k = 0; k < 64; k++) f.push_back(data_frame(1000 + 40 * k, k & 1, true));
    f.push_back(data_frame(1000 + 40 * 63 + 31, 1, true));  // lane 0 of the next tile folds into lane 63's group
    one("64 groups", 4096, 1000, f, Want{65, 0, 1000 + 40 * 63 + 32, 65}, o, true);
    const ufc_item &t = o.groups[0], &g = o.groups[64];
    if (t.id != 900 || t.data_offset != 1 || t.channel_id != 1) fail("64 groups: the tail", t.id, (long)t.data_offset, t.channel_id);
    if (g.id != 1000 + 40 * 63 || g.data_offset != 0x80000001u || g.channel_id != 0) fail("64 groups: the last", g.id, (long)g.data_offset, g.channel_id);
  }
  // size = 2^31: a sync lets id 6 in twice, into the same group; its bit is set the second time and the nonce stays.
  // The fold's stop test "a lane whose bit is not above the bit of the lane before it" is what keeps the nonce: with
  // both 6s in one fold both would count as "bit was clear".  (The bits are an OR either way: the clause decides the
  // nonce alone.)  The returning frame sits at lane 3 of a short step, at lane 63 with the lane before it (61) in
  // the same open group, and at lane 0 of the next tile.
  for (int where = 0; where < 3; where++) {
    std::vector<ufc_frame_info> f;
    if (where == 0) {
      f = {data_frame(5, 1, true), data_frame(6, 1, true), sync_frame(true, 7u + 0x80000000u, false), data_frame(6, 1, true),
           data_frame(7, 1, true), data_frame(4, 1, true)};
      one("ids that come back", 0x80000000u, 5, f, Want{4, 1, 8, 1}, o);
      static const uint8_t want[6] = {1, 1, 0, 1, 1, 0};
      if (std::memcmp(o.accept.data(), want, 6)) fail("ids that come back: frame_accept", 0, 0, 0);
      if (o.groups[0].id != 5 || o.groups[0].data_offset != 7 || o.groups[0].channel_id != 1)
        fail("ids that come back: group", 0, (long)o.groups[0].data_offset, o.groups[0].channel_id);
      continue;
    }
    // where == 1: data 5 | fillers | data 6 at 61 | the sync at 62 | data 6 at 63 | data 3 (refused) at 64
    // where == 2: data 5 | fillers | data 6 at 62 | the sync at 63 | data 6 at 64 (lane 0) | data 3 (refused) at 65
    const uint32_t first6 = where == 1 ? 61 : 62;
    f.push_back(data_frame(5, 0, true));
    for (uint32_t k = 1; k < first6; k++) f.push_back(filler(k));
    f.push_back(data_frame(6, 1, true));
    f.push_back(sync_frame(true, 7u + 0x80000000u, false));
    f.push_back(data_frame(6, 1, true));
    f.push_back(data_frame(3, 1, true));
    one(where == 1 ? "comes back at lane 63" : "comes back at lane 0", 0x80000000u, 5, f, Want{3, 1, 7, 1}, o);
    if (o.accept[first6] != 1 || o.accept[first6 + 2] != 1 || o.accept[first6 + 3] != 0) fail("comes back: verdicts", where, 0, 0);
    if (o.groups[0].id != 5 || o.groups[0].data_offset != 3 || o.groups[0].channel_id != 1)
      fail("comes back: group", where, (long)o.groups[0].data_offset, o.groups[0].channel_id);
  }
}

}  // namespace

int main() {
  static const uint32_t frame_counts[] = {0, 1, 2, 63, 64, 65, 127, 128, 130, 200};
  long accepted = 0, refused = 0, groups = 0, bad = 0, syncs = 0;
  std::memset((void*)&carried_block, 0xCD, sizeof carried_block);
  directed_cases();
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
    Out serial;
    run(kWalkSerial, infos, frame_first, windows, n + infos.size(), serial);
    const size_t caps[2] = {n + infos.size(), serial.used ? (size_t)(serial.used - 1 - rnd() % serial.used) : 0};
    for (int c = 0; c < 2; c++) all_forms("tiled", round, infos, frame_first, windows, caps[c], serial);
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
