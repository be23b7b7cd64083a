// The flush control's core (uflow_amd/csrc/frame_codec_core.hpp: fa_plan / fa_write and fs_decide_tile /
// fs_write_tile, the forms the device runs) as host code under AddressSanitizer and UBSan, driven the way the GPU
// form drives it (flush_ctl.hip): a count per connection, the exclusive sums, a writing wave per connection; the
// decisions tile by tile, the exclusive sum over the tiles, the writing tiles.  The lanes of a phase run one after the
// other -- forwards, backwards and in a fresh seeded permutation per phase (lane_orders.hpp) -- and the ack flush's
// shared block starts as garbage, fresh for every connection or, in a fourth pass, one block carried from connection
// to connection as the kernel's grid-stride loop carries it.  Checked against a serial restatement written here from
// the reference's text, push by push (AckFrameEmitter, emit.rs:137-211; emit_ack_frames, mod.rs:296-333;
// emit_sync_frame, mod.rs:234-294): every output must be equal byte for byte.  All buffers have their exact sizes, the
// caps once always-enough and once below the need; the carry rooms are updated in place and windows_out / ctl_out are
// the inputs.  In front of the seeded traffic, directed cases with their expectations written out as literals: the
// dud frame at alloc 0 and 15, the 161 / 162 group seam, a carry whose last group sits at lane 63 and at lane 0 of the
// next tile, a carry one over its room, and sync frames from lane 63 alone and from lane 0 of the second tile alone.
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

uint64_t rng_state = 0xF1A5C7u;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

enum Form { kRestated, kForwards, kBackwards, kShuffled, kCarried, kForms };
FaWaveShared carried_block;  // (garbage once, in main)

ufc_item group(uint32_t id, uint32_t bits, uint32_t nonce) {
  ufc_item g{};
  g.id = id;
  g.form = 3;
  g.channel_id = (uint8_t)nonce;
  g.data_offset = bits;
  return g;
}

// ---- the ack flush ----
struct AckIn {
  std::vector<ufc_flush_ctl> ctl;
  std::vector<ufc_frame_window> windows;
  std::vector<ufc_item> groups;
  std::vector<uint64_t> group_first;
  std::vector<ufc_receiver> receivers;
  std::vector<ufc_rate_result> rate;
  std::vector<ufc_item> carry;
};
struct AckOut {
  std::vector<ufc_flush_ctl> ctl;          // in place
  std::vector<ufc_frame_window> windows;   // in place
  std::vector<ufc_item> carry, merged;     // carry in place
  std::vector<uint64_t> merged_first;
  std::vector<ufc_frame_info> infos;
  std::vector<ufc_flush_result> results;
  std::vector<ufc_flush_acks_result> ack_results;
  std::vector<ufc_flush> flushes;
  std::vector<uint32_t> flags;
  uint64_t merged_used = 0, frames_used = 0;
};

void add_connection(AckIn& in, const std::vector<ufc_item>& carry, uint32_t cap, const std::vector<ufc_item>& groups,
                    int64_t alloc, uint8_t sync_reply) {
  ufc_flush_ctl c{};
  in.carry.push_back(group(0xDEAD0000u, 0xFFFFFFFFu, 1));  // a guard in front of every room
  c.carry_first = in.carry.size();
  c.carry_cap = cap;
  c.carry_count = (uint32_t)carry.size();
  c.reserved0 = 0xA5, c.reserved1 = 0xBEEF, c.reserved2 = rnd();
  c.sync_timeout_base_ms = rnd();
  for (uint32_t k = 0; k < cap || k < carry.size(); k++) in.carry.push_back(k < carry.size() ? carry[k] : group(0xFEED0000u + k, rnd(), 1));
  in.ctl.push_back(c);
  ufc_frame_window w{};
  w.base_id = rnd(), w.size = 64, w.sync_reply = sync_reply, w.reserved = 0x3C, w.reserved2 = rnd();
  if (!groups.empty()) w.has_tail = 1, w.tail_base_id = groups.back().id, w.tail_bitfield = groups.back().data_offset;
  in.windows.push_back(w);
  if (in.group_first.empty()) in.group_first.push_back(0);
  in.groups.insert(in.groups.end(), groups.begin(), groups.end());
  in.group_first.push_back(in.groups.size());
  ufc_receiver r{};
  r.base_id = rnd() & 0xFFFFF;
  in.receivers.push_back(r);
  ufc_rate_result q{};
  q.flush_alloc = alloc;
  in.rate.push_back(q);
}

// The reference's text, push by push, for one connection.
void restated_connection(const AckIn& in, AckOut& o, size_t c, std::vector<ufc_item>& merged_all,
                         std::vector<ufc_frame_info>& infos_all) {
  const ufc_flush_ctl& C = in.ctl[c];
  const ufc_frame_window& W = in.windows[c];
  const uint64_t g0 = in.group_first[c], g1 = in.group_first[c + 1];
  ufc_flush_result& r = o.results[c];
  ufc_flush_acks_result& ar = o.ack_results[c];
  r = ufc_flush_result{};
  ar = ufc_flush_acks_result{};
  r.frame_first = (uint32_t)infos_all.size();
  ar.merged_first = (uint32_t)merged_all.size();
  o.merged_first[c] = merged_all.size();
  int64_t alloc = in.rate[c].flush_alloc;
  bool ok = g0 <= g1 && g1 <= in.groups.size() && C.carry_count <= C.carry_cap && C.carry_first <= in.carry.size() &&
            in.carry.size() - C.carry_first >= C.carry_cap;
  if (ok && C.carry_count) ok = g1 > g0 && in.groups[g0].id == in.carry[C.carry_first + C.carry_count - 1].id;
  if (!ok) {
    r.stop = UFC_PACK_BAD_RANGE, r.alloc_left = alloc, ar.stop = UFC_FA_BAD_STATE;
    o.flushes[c].flush_alloc = alloc;
    o.flags[c] &= ~1u;
    return;
  }
  std::vector<ufc_item> deque;
  for (uint32_t k = 0; k + 1 < C.carry_count; k++) deque.push_back(in.carry[C.carry_first + k]);
  for (uint64_t g = g0; g < g1; g++) deque.push_back(in.groups[g]);
  const size_t at0 = merged_all.size();
  merged_all.insert(merged_all.end(), deque.begin(), deque.end());
  // AckFrameEmitter
  bool in_progress = false, sync_reply = W.sync_reply != 0, err = false;
  uint32_t count = 0, first = 0, popped = 0, frames = 0;
  const auto finalize = [&] {
    if (!in_progress) return;
    ufc_frame_info f{};
    f.kind = UFC_FRAME_ACK, f.ok = 1, f.f[0] = W.base_id, f.f[1] = in.receivers[c].base_id;
    f.item_first = (uint32_t)(at0 + first), f.item_count = count;
    infos_all.push_back(f);
    alloc -= 15 + 9 * (int64_t)count;
    frames++;
    in_progress = false;
    sync_reply = false;
  };
  if (sync_reply) {  // push_dud
    if (alloc < 0) err = true;
    else in_progress = true, count = 0, first = 0, ar.dud = 1;
  }
  while (!err && popped < deque.size()) {
    bool pushed = false;
    if (in_progress) {
      const int64_t size = 15 + 9 * (int64_t)count;
      if (alloc - size < 0) {
        finalize();
        err = true;
        break;
      } else if (size + 9 > 1472) {
        finalize();
      } else {
        count++;
        pushed = true;
      }
    }
    if (!pushed) {
      if (alloc < 0) {
        err = true;
        break;
      }
      in_progress = true, first = popped, count = 1;
    }
    popped++;
  }
  if (!err) finalize();
  const uint32_t left = (uint32_t)deque.size() - popped, kept = left < C.carry_cap ? left : C.carry_cap;
  for (uint32_t k = 0; k < kept; k++) o.carry[C.carry_first + k] = deque[deque.size() - kept + k];
  r.frame_count = frames, r.items_packed = popped, r.stop = err ? UFC_PACK_SIZE_LIMITED : UFC_PACK_DONE, r.alloc_left = alloc;
  ar.merged_count = (uint32_t)deque.size(), ar.carried = kept, ar.dropped = left - kept;
  ar.stop = left > kept ? UFC_FA_CARRY_FULL : UFC_FA_DONE;
  if (frames) o.windows[c].sync_reply = 0;
  if (!left) o.windows[c].has_tail = 0;
  o.ctl[c].carry_count = kept;
  o.flushes[c].flush_alloc = alloc;
  o.flags[c] = (o.flags[c] & ~1u) | (err ? 1u : 0u);
}

void run_acks(int form, const AckIn& in, size_t merged_cap, size_t frames_cap, AckOut& o) {
  const size_t n = in.ctl.size();
  o.ctl = in.ctl, o.windows = in.windows, o.carry = in.carry;
  o.merged.resize(merged_cap), o.infos.resize(frames_cap);
  if (merged_cap) std::memset((void*)o.merged.data(), 0xA5, merged_cap * sizeof(ufc_item));
  if (frames_cap) std::memset((void*)o.infos.data(), 0xA5, frames_cap * sizeof(ufc_frame_info));
  o.merged_first.assign(n + 1, 0);
  o.results.resize(n), o.ack_results.resize(n), o.flushes.resize(n), o.flags.resize(n);
  std::memset((void*)o.results.data(), 0xA5, n * sizeof(ufc_flush_result));
  std::memset((void*)o.ack_results.data(), 0xA5, n * sizeof(ufc_flush_acks_result));
  for (size_t c = 0; c < n; c++) {
    o.flushes[c] = ufc_flush{-777, UFC_FRAME_DATA, 5, (uint32_t)c, 9};
    o.flags[c] = (uint32_t)(c * 0x9E3779B1u) | 2u;
  }
  if (form == kRestated) {
    std::vector<ufc_item> merged_all;
    std::vector<ufc_frame_info> infos_all;
    for (size_t c = 0; c < n; c++) restated_connection(in, o, c, merged_all, infos_all);
    o.merged_first[n] = o.merged_used = merged_all.size();
    o.frames_used = infos_all.size();
    for (size_t k = 0; k < merged_all.size() && k < merged_cap; k++) o.merged[k] = merged_all[k];
    for (size_t k = 0; k < infos_all.size() && k < frames_cap; k++) o.infos[k] = infos_all[k];
    return;
  }
  const FaArgs a{o.ctl.data(), o.windows.data(), in.groups.data(), in.groups.size(), in.group_first.data(),
                 in.receivers.data(), in.rate.data(), n, o.carry.data(), o.carry.size(), o.merged.data(), merged_cap,
                 o.merged_first.data(), &o.merged_used, o.infos.data(), frames_cap, &o.frames_used, o.results.data(),
                 o.ack_results.data(), o.windows.data(), o.ctl.data(), o.flushes.data(), o.flags.data()};
  if (!fa_args_ok(a)) fail("fa_args_ok", form, 0, 0);
  std::vector<uint64_t> frame_first(n + 1, 0);
  uint64_t m = 0, f = 0;
  for (size_t c = 0; c < n; c++) {
    const FaPlan p = fa_plan(a, c);
    o.merged_first[c] = m, frame_first[c] = f;
    m += p.merged, f += p.frames;
  }
  o.merged_first[n] = o.merged_used = m;
  frame_first[n] = o.frames_used = f;
  for (size_t c = n; c-- > 0;) {  // (the connections in any order: last first here)
    FaWaveShared fresh;
    std::memset((void*)&fresh, 0xCD, sizeof fresh);
    FaWaveShared& sh = form == kCarried ? carried_block : fresh;
    if (form == kBackwards) fa_write(lane_orders::ReverseWave{}, sh, a, c, frame_first[c]);
    else if (form == kShuffled) fa_write(lane_orders::ShuffledWave{}, sh, a, c, frame_first[c]);
    else fa_write(SerialWave{}, sh, a, c, frame_first[c]);
  }
}

template <class T>
bool same(const std::vector<T>& x, const std::vector<T>& y) {
  return x.size() == y.size() && (x.empty() || !std::memcmp((const void*)x.data(), (const void*)y.data(), x.size() * sizeof(T)));
}

void acks_all_forms(const char* what, long where, const AckIn& in, size_t merged_cap, size_t frames_cap, AckOut& want) {
  run_acks(kRestated, in, merged_cap, frames_cap, want);
  for (int form = kForwards; form < kForms; form++) {
    AckOut got;
    run_acks(form, in, merged_cap, frames_cap, got);
    if (got.merged_used != want.merged_used || got.frames_used != want.frames_used) fail(what, where, form, 1);
    if (!same(got.merged_first, want.merged_first)) fail(what, where, form, 2);
    if (!same(got.merged, want.merged)) fail(what, where, form, 3);
    if (!same(got.infos, want.infos)) fail(what, where, form, 4);
    if (!same(got.results, want.results)) fail(what, where, form, 5);
    if (!same(got.ack_results, want.ack_results)) fail(what, where, form, 6);
    if (!same(got.windows, want.windows)) fail(what, where, form, 7);
    if (!same(got.ctl, want.ctl)) fail(what, where, form, 8);
    if (!same(got.carry, want.carry)) fail(what, where, form, 9);
    if (!same(got.flushes, want.flushes) || !same(got.flags, want.flags)) fail(what, where, form, 10);
    checks++;
  }
}

std::vector<ufc_item> seq(uint32_t n, uint32_t start) {
  std::vector<ufc_item> v;
  for (uint32_t k = 0; k < n; k++) v.push_back(group(start + 40 * k, 1u | (k * 2654435761u), k & 1));
  return v;
}

void directed_acks() {
  AckOut o;
  {  // the dud frame: finalized empty at alloc 0, takes the group at 15; without a dud alloc 0 packs one group
    AckIn in;
    add_connection(in, {}, 8, seq(2, 100), 0, 1);
    add_connection(in, {}, 8, seq(2, 100), 15, 1);
    add_connection(in, {}, 8, seq(2, 100), 0, 0);
    add_connection(in, {}, 8, seq(2, 100), -1, 7);
    add_connection(in, {}, 8, {}, 14, 1);
    acks_all_forms("dud", 0, in, in.carry.size() + in.groups.size(), 5 + in.carry.size() + in.groups.size(), o);
    static const long want[5][5] = {{1, 0, UFC_PACK_SIZE_LIMITED, -15, 2}, {1, 1, UFC_PACK_SIZE_LIMITED, -9, 1},
                                    {1, 1, UFC_PACK_SIZE_LIMITED, -24, 1}, {0, 0, UFC_PACK_SIZE_LIMITED, -1, 2},
                                    {1, 0, UFC_PACK_DONE, -1, 0}};
    for (int c = 0; c < 5; c++) {
      const ufc_flush_result& r = o.results[c];
      if (r.frame_count != want[c][0] || r.items_packed != want[c][1] || r.stop != want[c][2] || r.alloc_left != want[c][3] ||
          o.ctl[c].carry_count != want[c][4])
        fail("dud: result", c, r.items_packed, (long)r.alloc_left);
    }
    if (o.windows[0].sync_reply || o.windows[3].sync_reply != 7 || o.windows[4].sync_reply || o.windows[4].has_tail)
      fail("dud: sync_reply", o.windows[0].sync_reply, o.windows[3].sync_reply, 0);
    if (o.frames_used != 4 || o.infos[0].item_count != 0 || o.infos[1].item_count != 1 || o.infos[3].item_count != 0)
      fail("dud: frames", (long)o.frames_used, o.infos[0].item_count, 0);
  }
  {  // 161 groups are one frame of 1464 bytes; the 162nd starts a second one only with 1464 bytes to spend
    AckIn in;
    add_connection(in, {}, 200, seq(161, 7), 1463, 0);
    add_connection(in, {}, 200, seq(162, 7), 1463, 0);
    add_connection(in, {}, 200, seq(162, 7), 1464, 1);
    add_connection(in, {}, 200, seq(323, 7), 1 << 20, 0);
    acks_all_forms("seam", 0, in, in.carry.size() + in.groups.size(), 4 + in.carry.size() + in.groups.size(), o);
    static const long want[4][4] = {{1, 161, UFC_PACK_DONE, -1}, {1, 161, UFC_PACK_SIZE_LIMITED, -1},
                                    {2, 162, UFC_PACK_DONE, -24}, {3, 323, UFC_PACK_DONE, (1 << 20) - 45 - 9 * 323}};
    for (int c = 0; c < 4; c++) {
      const ufc_flush_result& r = o.results[c];
      if (r.frame_count != want[c][0] || r.items_packed != want[c][1] || r.stop != want[c][2] || r.alloc_left != want[c][3])
        fail("seam: result", c, r.items_packed, (long)r.alloc_left);
    }
    if (o.ctl[1].carry_count != 1 || o.carry[in.ctl[1].carry_first].id != 7 + 40 * 161) fail("seam: carry", o.ctl[1].carry_count, 0, 0);
    const ufc_frame_info& f = o.infos[o.results[3].frame_first + 2];
    if (f.item_count != 1 || f.item_first != o.merged_first[3] + 322) fail("seam: third frame", f.item_count, f.item_first, 0);
  }
  for (uint32_t m = 63; m <= 66; m++) {  // nothing is sent: the carry's last group is merged group m - 1, at lane 63
    AckIn in;                            // (m = 64), at lane 0 of the next tile (m = 65), and beside them
    const std::vector<ufc_item> all = seq(m, 11);
    std::vector<ufc_item> carry(all.begin(), all.begin() + 60), groups(all.begin() + 59, all.end());
    carry.back().data_offset = 1;  // (the stale copy of the tail as carried)
    add_connection(in, carry, 80, groups, -5, 0);
    add_connection(in, {}, 4, seq(3, 9), 100, 0);
    acks_all_forms("carry at the lane seam", m, in, in.carry.size() + in.groups.size(), 9, o);
    if (o.results[0].stop != UFC_PACK_SIZE_LIMITED || o.ctl[0].carry_count != m || o.ack_results[0].merged_count != m)
      fail("carry at the lane seam: counts", m, o.ctl[0].carry_count, 0);
    for (uint32_t k = 0; k < m; k++)
      if (std::memcmp((const void*)&o.carry[in.ctl[0].carry_first + k], (const void*)&all[k], sizeof(ufc_item)))
        fail("carry at the lane seam: group", m, k, 0);
    // the same list into a room one short: the oldest group goes, the tail stays
    AckIn tight;
    add_connection(tight, carry, m - 1, groups, -5, 0);
    if (m - 1 >= 60) {
      acks_all_forms("carry one over", m, tight, tight.carry.size() + tight.groups.size(), 9, o);
      if (o.ack_results[0].stop != UFC_FA_CARRY_FULL || o.ack_results[0].dropped != 1 || o.ctl[0].carry_count != m - 1 ||
          o.carry[tight.ctl[0].carry_first].id != all[1].id || o.carry[tight.ctl[0].carry_first + m - 2].id != all[m - 1].id)
        fail("carry one over", m, o.ack_results[0].dropped, o.ctl[0].carry_count);
    }
  }
  {  // BAD_STATE: a carry and no window group; ids that differ
    AckIn in;
    add_connection(in, seq(2, 5), 8, {}, 100, 1);
    add_connection(in, seq(2, 5), 8, seq(1, 46), 100, 1);
    add_connection(in, seq(2, 5), 8, seq(1, 45), 100, 1);
    acks_all_forms("bad state", 0, in, 20, 20, o);
    if (o.ack_results[0].stop != UFC_FA_BAD_STATE || o.ack_results[1].stop != UFC_FA_BAD_STATE || o.ack_results[2].stop != UFC_FA_DONE ||
        o.frames_used != 1 || o.ctl[0].carry_count != 2 || o.windows[1].sync_reply != 1 || o.ack_results[2].merged_count != 2)
      fail("bad state", o.ack_results[0].stop, o.ack_results[1].stop, (long)o.frames_used);
  }
}

void seeded_acks(int round) {
  AckIn in;
  const uint32_t n = 1 + rnd() % 6;
  static const uint32_t counts[] = {0, 1, 2, 5, 63, 64, 65, 130, 161, 162, 200, 330};
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t n_groups = counts[rnd() % 12], n_carry = rnd() % 3 ? 0 : rnd() % 70;
    std::vector<ufc_item> all = seq(n_carry + n_groups, rnd()), carry, groups;
    uint32_t cap = n_carry + rnd() % 5;
    if (n_carry && n_groups) {
      carry.assign(all.begin(), all.begin() + n_carry);
      groups.assign(all.begin() + n_carry - 1, all.end() - 1);
      carry.back().data_offset ^= 0xF0;
    } else {
      groups.assign(all.begin(), all.begin() + n_groups);
      if (rnd() % 8 == 0) cap = rnd() % 3;
    }
    if (rnd() % 16 == 0) {  // records that are no ack groups: carried through as they are
      for (auto& g : groups)
        for (size_t k = 4; k < sizeof g; k++) ((uint8_t*)&g)[k] = (uint8_t)rnd();
    }
    static const int64_t allocs[] = {-1, 0, 14, 15, 23, 24, 1463, 1464, 1465, INT64_MAX, INT64_MIN, 3000};
    const int64_t alloc = rnd() % 3 ? allocs[rnd() % 12] : (int64_t)(rnd() % 4000) - 10;
    add_connection(in, carry, cap, groups, alloc, rnd() % 3 ? 0 : (uint8_t)(1 + rnd() % 255));
  }
  in.carry.push_back(group(0xDEADFFFFu, 0, 0));
  if (rnd() % 16 == 0) in.ctl[rnd() % n].carry_count += 1 + rnd() % 100;  // BAD_STATE, one way or another
  if (rnd() % 16 == 0) in.group_first[rnd() % (n + 1)] = in.groups.size() + rnd() % 3;
  if (rnd() % 32 == 0) in.ctl[rnd() % n].carry_first = in.carry.size() + 1 + rnd() % 3;  // a room outside the arena
  AckOut want;
  const size_t always = in.carry.size() + in.groups.size();
  acks_all_forms("seeded", round, in, always, n + always, want);
  const size_t mc = want.merged_used ? want.merged_used - 1 - rnd() % want.merged_used : 0;
  const size_t fc = want.frames_used ? want.frames_used - 1 - rnd() % want.frames_used : 0;
  acks_all_forms("seeded, short caps", round, in, mc, fc, want);
}

// ---- the sync frame ----
struct SyncIn {
  std::vector<ufc_flush_ctl> ctl;
  std::vector<ufc_rate_result> rate;
  std::vector<ufc_flush_result> ack, pack;
  std::vector<ufc_resend_result> begin;
  std::vector<ufc_resend_commit_result> commit;
  std::vector<ufc_frame_queue> queues;
  std::vector<ufc_sender> senders;
};
struct SyncOut {
  std::vector<ufc_flush_ctl> ctl;  // in place
  std::vector<ufc_frame_info> infos;
  std::vector<uint32_t> index;
  std::vector<ufc_flush_sync_result> results;
  std::vector<ufc_rate_tick> ticks;
  uint64_t used = 0;
};

void add_sync(SyncIn& in, bool sends, bool random) {
  ufc_flush_ctl c{};
  ufc_rate_result r{};
  ufc_flush_result a{}, p{};
  ufc_resend_result b{};
  ufc_resend_commit_result m{};
  ufc_frame_queue q{};
  ufc_sender s{};
  r.now_ms = 100000, r.rto_ms = 600, c.sync_timeout_base_ms = 1000, p.alloc_left = 100;
  q.log_next_id = q.window_base_id = 500;
  s.base_id = 30, s.next_id = sends ? 31 : 30;
  c.reserved2 = rnd();
  if (random) {
    static const uint64_t rtos[] = {600, 1999, 2000, 2001, 5000};
    r.now_ms = ((uint64_t)rnd() << 8) ^ rnd(), r.rto_ms = rtos[rnd() % 5];
    const uint64_t timeout = r.rto_ms > 2000 ? r.rto_ms : 2000;
    const uint64_t elapsed = rnd() % 4 == 0 ? timeout - 1 : rnd() % 3 == 0 ? timeout : rnd() % 20000;
    c.sync_timeout_base_ms = r.now_ms - elapsed;
    const uint32_t u = rnd() % 16;
    if (u == 0) a.stop = UFC_PACK_SIZE_LIMITED;
    if (u == 1) b.stop = 1 + rnd() % 5;
    if (u == 2) p.stop = 1 + rnd() % 3;
    if (u == 3) m.stop = rnd() % 2 ? UFC_RS_BAD_STATE : UFC_RS_HEAP_FULL;
    if (rnd() % 4 == 0) p.frame_count = 1 + rnd() % 3;
    q.log_next_id = rnd(), q.window_base_id = rnd() % 2 ? q.log_next_id + p.frame_count : q.log_next_id - rnd() % 3;
    s.base_id = rnd() & 0xFFFFF, s.next_id = (s.base_id + rnd() % 3) & 0xFFFFF;
    m.heap_len = rnd() % 4 == 0, m.pending_count = rnd() % 4 == 0;
    if (rnd() % 2) c.has_keepalive = (uint8_t)(1 + rnd() % 255), c.keepalive_interval_ms = elapsed + rnd() % 3 - 1;
    else if (rnd() % 2) c.keepalive_interval_ms = rnd();
    static const int64_t left[] = {-1, 0, 13, 14, 5000, INT64_MIN};
    p.alloc_left = left[rnd() % 6];
  }
  in.ctl.push_back(c), in.rate.push_back(r), in.ack.push_back(a), in.pack.push_back(p), in.begin.push_back(b);
  in.commit.push_back(m), in.queues.push_back(q), in.senders.push_back(s);
}

void restated_sync(const SyncIn& in, size_t cap, SyncOut& o) {
  const size_t n = in.ctl.size();
  std::vector<ufc_frame_info> frames;
  for (size_t c = 0; c < n; c++) {
    ufc_flush_ctl& C = o.ctl[c];
    const ufc_rate_result& R = in.rate[c];
    const ufc_flush_result& P = in.pack[c];
    const ufc_resend_commit_result& M = in.commit[c];
    ufc_flush_sync_result res{};
    res.heap_len = M.heap_len, res.pending_count = M.pending_count;
    res.is_send_pending = M.heap_len || M.pending_count;
    uint32_t reason = UFC_FS_SENT;
    bool go = true;
    if (in.ack[c].stop == UFC_PACK_SIZE_LIMITED) reason = UFC_FS_ACK_LIMITED, go = false;  // mod.rs:218-221
    if (go && P.frame_count) C.sync_timeout_base_ms = R.now_ms;                            // :346
    if (go && (in.begin[c].stop == UFC_RS_SIZE_LIMITED || P.stop == UFC_PACK_SIZE_LIMITED)) reason = UFC_FS_DATA_LIMITED, go = false;
    if (go && (in.begin[c].stop == UFC_RS_REF_HANG || in.begin[c].stop == UFC_RS_BAD_STATE || M.stop == UFC_RS_REF_HANG ||
               M.stop == UFC_RS_BAD_STATE || M.stop == UFC_RS_HEAP_FULL))
      reason = UFC_FS_UPSTREAM, go = false;
    if (go) {  // emit_sync_frame
      const uint64_t elapsed_ms = R.now_ms - C.sync_timeout_base_ms;
      const uint64_t sync_timeout_ms = R.rto_ms > 2000 ? R.rto_ms : 2000;
      if (elapsed_ms >= sync_timeout_ms) {
        const uint32_t fq_next = in.queues[c].log_next_id + P.frame_count;
        const bool has_frame = fq_next != in.queues[c].window_base_id;
        const bool has_packet = in.senders[c].next_id != in.senders[c].base_id && M.heap_len == 0 && M.pending_count == 0;
        bool ret = false;
        if (!has_frame && !has_packet) {
          if (C.has_keepalive) {
            if (elapsed_ms < C.keepalive_interval_ms) ret = true;
          } else {
            ret = true;
          }
        }
        if (ret) {
          reason = UFC_FS_IDLE;
        } else if (P.alloc_left < 0) {
          reason = UFC_FS_NO_ALLOC;
        } else {
          ufc_frame_info f{};
          f.kind = UFC_FRAME_SYNC, f.ok = 1, f.aux = (uint8_t)((has_frame ? 1 : 0) | (has_packet ? 2 : 0));
          f.f[0] = has_frame ? fq_next : 0, f.f[1] = has_packet ? in.senders[c].next_id : 0;
          o.index[c] = (uint32_t)frames.size();
          frames.push_back(f);
          res.mode = f.aux;
          C.sync_timeout_base_ms = R.now_ms;
        }
      } else {
        reason = UFC_FS_NOT_DUE;
      }
    }
    if (C.has_keepalive) C.has_keepalive = 1;
    else C.keepalive_interval_ms = 0;
    res.reason = reason, res.sent = reason == UFC_FS_SENT;
    if (!res.sent) o.index[c] = UFC_NO_PARENT;
    o.results[c] = res;
    o.ticks[c].alloc_adjust = res.sent ? -14 : 0;
  }
  o.used = frames.size();
  for (size_t k = 0; k < frames.size() && k < cap; k++) o.infos[k] = frames[k];
}

void run_sync(int form, const SyncIn& in, size_t cap, SyncOut& o) {
  const size_t n = in.ctl.size();
  o.ctl = in.ctl;
  o.infos.resize(cap), o.index.assign(n, 0xA5A5A5A5u), o.results.resize(n), o.ticks.resize(n);
  if (cap) std::memset((void*)o.infos.data(), 0xA5, cap * sizeof(ufc_frame_info));
  std::memset((void*)o.results.data(), 0xA5, n * sizeof(ufc_flush_sync_result));
  std::memset((void*)o.ticks.data(), 0x5A, n * sizeof(ufc_rate_tick));
  if (form == kRestated) return restated_sync(in, cap, o);
  const FsArgs a{o.ctl.data(), in.rate.data(), in.ack.data(), in.begin.data(), in.pack.data(), in.commit.data(),
                 in.queues.data(), in.senders.data(), n, o.infos.data(), cap, o.index.data(), &o.used, o.results.data(),
                 o.ctl.data(), o.ticks.data()};
  if (!fs_args_ok(a)) fail("fs_args_ok", form, 0, 0);
  const size_t tiles = (n + 63) / 64;
  std::vector<uint64_t> first(tiles + 1, 0);
  for (size_t t = tiles; t-- > 0;) {
    if (form == kBackwards) first[t + 1] = fs_decide_tile(lane_orders::ReverseWave{}, a, t);
    else if (form == kShuffled) first[t + 1] = fs_decide_tile(lane_orders::ShuffledWave{}, a, t);
    else first[t + 1] = fs_decide_tile(SerialWave{}, a, t);
  }
  for (size_t t = 0; t < tiles; t++) first[t + 1] += first[t];
  o.used = first[tiles];
  for (size_t t = tiles; t-- > 0;) {
    if (form == kBackwards) fs_write_tile(lane_orders::ReverseWave{}, a, t, first[t]);
    else if (form == kShuffled) fs_write_tile(lane_orders::ShuffledWave{}, a, t, first[t]);
    else fs_write_tile(SerialWave{}, a, t, first[t]);
  }
}

void sync_all_forms(const char* what, long where, const SyncIn& in, size_t cap, SyncOut& want) {
  run_sync(kRestated, in, cap, want);
  for (int form = kForwards; form < kCarried; form++) {  // (the stage has no shared block to carry)
    SyncOut got;
    run_sync(form, in, cap, got);
    if (got.used != want.used || !same(got.index, want.index)) fail(what, where, form, 1);
    if (!same(got.infos, want.infos)) fail(what, where, form, 2);
    if (!same(got.results, want.results)) fail(what, where, form, 3);
    if (!same(got.ctl, want.ctl)) fail(what, where, form, 4);
    if (!same(got.ticks, want.ticks)) fail(what, where, form, 5);
    checks++;
  }
}

void directed_sync() {
  static const uint32_t sizes[] = {1, 63, 64, 65, 130};
  for (uint32_t n : sizes)
    for (int pattern = 0; pattern < 5; pattern++) {  // lane 63 alone, lane 0 of the second tile alone, all, none, thirds
      SyncIn in;
      uint32_t want_used = 0;
      for (uint32_t c = 0; c < n; c++) {
        const bool sends = pattern == 0 ? c == 63 : pattern == 1 ? c == 64 : pattern == 2 ? true : pattern == 3 ? false : c % 3 == 0;
        add_sync(in, sends, false);
        in.queues[c].log_next_id = in.queues[c].window_base_id = c;
        want_used += sends;
      }
      SyncOut o;
      sync_all_forms("compaction", n, in, n, o);
      if (o.used != want_used) fail("compaction: used", n, pattern, (long)o.used);
      uint32_t k = 0;
      for (uint32_t c = 0; c < n; c++) {
        const bool sends = o.results[c].sent != 0;
        if (o.index[c] != (sends ? k : UFC_NO_PARENT)) fail("compaction: index", n, pattern, c);
        if (sends && (o.infos[k].kind != UFC_FRAME_SYNC || o.infos[k].aux != 2 || o.infos[k].f[1] != 31 || o.infos[k].f[0] != 0 ||
                      o.ctl[c].sync_timeout_base_ms != 100000 || o.ticks[c].alloc_adjust != -14))
          fail("compaction: frame", n, pattern, c);
        if (!sends && (o.ctl[c].sync_timeout_base_ms != 1000 || o.ticks[c].alloc_adjust != 0)) fail("compaction: idle", n, pattern, c);
        k += sends;
      }
      if (want_used) sync_all_forms("compaction, short cap", n, in, want_used - 1, o);
    }
}

}  // namespace

int main() {
  std::memset((void*)&carried_block, 0xCD, sizeof carried_block);
  directed_acks();
  directed_sync();
  for (int round = 0; round < 400; round++) seeded_acks(round);
  long reasons[7] = {0};
  for (int round = 0; round < 200; round++) {
    SyncIn in;
    const uint32_t n = 1 + rnd() % 200;
    for (uint32_t c = 0; c < n; c++) add_sync(in, rnd() % 2, true);
    SyncOut want;
    sync_all_forms("seeded sync", round, in, n, want);
    for (uint32_t c = 0; c < n; c++) reasons[want.results[c].reason]++;
    sync_all_forms("seeded sync, short cap", round, in, want.used ? want.used - 1 - rnd() % want.used : 0, want);
  }
  for (int k = 0; k < 7; k++)
    if (reasons[k] < 50) fail("too little of some reason", k, reasons[k], 0);
  std::printf("ok: %ld\n", checks);
  return 0;
}
