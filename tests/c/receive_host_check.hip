// The receive core (uflow_amd/csrc/frame_codec_core.hpp: rx_walk, rx_finish, the duplicate table, the plan and
// segment records) as host code under AddressSanitizer and UBSan, driven the way the GPU form drives it
// (packet_receive.hip): one walk per receiver, exclusive sums of the three counts, one finish per receiver, then
// the copies as the kernels make them: the slots' segments split into chunks of 2048 bytes, every chunk finding
// its segment by binary search in the chunk prefix, then the datagrams' segments, each side of a copy at any
// byte alignment.  Seeded senders (sequence ids wrapping through 0xFFFFF, reliable packets on three channels,
// 0 to 65 fragments) feed receivers over many steps; every step delivers a random part of what is in flight,
// shuffled, some of it twice, the carry swapped each time.  All buffers have their exact sizes: every step runs
// once with caps of zero on a copy of the state to learn the used counts, then with buffers of exactly those.
// Checked against the senders' own record, with none of the core's functions: per receiver and channel the
// delivered packets are the sent ones, in order and byte for byte, and at the end every packet has arrived, the
// carry is empty and the allocation count is back at zero.  Hostile datagrams ride along (mismatching twins,
// invalid ones, ids and payload ranges out of bounds) and must leave no trace.  A second part runs steps on
// headers, slots and items of random bytes: no expectation but that every access stays inside the buffers.
// Every step of both parts also runs the device form's parts as host code -- rx_walk_begin, the item-parallel
// verdicts (rx_frame_verdicts, frames in reverse order), rx_walk_items on what they let through, and
// rx_receive_tiles (the per-channel delivery prefixes and the window-advance prefix over 64-lane masks, the
// lanes of a phase run one after the other: forwards, backwards and in a fresh seeded permutation per phase,
// lane_orders.hpp; the shared block garbage, fresh for every receiver or, in a fourth pass, one block carried from
// receiver to receiver) -- against the serial rx_walk: headers, slots, results, records, delivered bytes and the
// carry must be equal byte for byte, on hostile state too.  In front of all that, directed cases that put every
// cross-lane read of rx_receive_tiles on lane 63 and on lane 0 of the second tile (DESIGN.md 5.15;
// tests/test_receive_cpu.py has the same cases as scenarios), each with its expectation spelled out.
// Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
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

uint64_t rng_state = 0x5EC317EDu;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

constexpr uint32_t kMask = 0xFFFFF, kFrag = 1448, kChunk = 2048, kNone = 0xFFFFFFFFu;

struct Dg {  // a datagram in flight; its bytes are data[at .. at + len) of the sender's record
  ufc_item it;
  size_t packet;  // index in the sender's record
  uint32_t frag = 0;  // the fragment whose bytes it carries (a hostile twin may name another)
  bool bad_src = false;
};
struct Sent {
  uint32_t seq, channel;
  std::vector<uint8_t> data;
};
struct Peer {  // one sender and what it has in flight
  uint32_t next_id, window_parent = kNone, channel_parent[3] = {kNone, kNone, kNone};
  std::vector<Sent> sent;
  std::vector<Dg> flight;
  size_t delivered[3] = {0, 0, 0};  // per channel: packets of `sent` on that channel delivered so far
};

void send_packet(Peer& p, uint32_t len) {
  Sent s;
  s.seq = p.next_id;
  s.channel = rnd() % 3;
  s.data.resize(len);
  for (auto& b : s.data) b = (uint8_t)rnd();
  const uint32_t wl = p.window_parent == kNone ? 0 : ((s.seq - p.window_parent) & kMask) & 0xFFFF;
  const uint32_t cl = p.channel_parent[s.channel] == kNone ? 0 : ((s.seq - p.channel_parent[s.channel]) & kMask) & 0xFFFF;
  p.window_parent = p.channel_parent[s.channel] = s.seq;
  p.next_id = (p.next_id + 1) & kMask;
  const uint32_t last = (len ? (len + kFrag - 1) / kFrag : 1) - 1;
  for (uint32_t f = 0; f <= last; f++) {
    Dg d{};
    d.it.id = s.seq;
    d.it.channel_id = (uint8_t)s.channel;
    d.it.window_parent_lead = (uint16_t)wl;
    d.it.channel_parent_lead = (uint16_t)cl;
    d.it.fragment_id = (uint16_t)f;
    d.it.fragment_id_last = (uint16_t)last;
    d.it.data_len = f == last ? len - f * kFrag : kFrag;
    d.packet = p.sent.size();
    d.frag = f;
    p.flight.push_back(d);
  }
  p.sent.push_back(std::move(s));
}

struct Counts {
  uint64_t packets, out, carry;
};

// The forms run_step runs in: the serial walk, or the device form's parts with rx_receive_tiles under three lane
// orders on a fresh garbage block, and forwards on a carried one.
enum Form { kWalkSerial, kForwards, kBackwards, kShuffled, kCarried, kForms };
int g_form = kWalkSerial;
RxWaveShared carried_block;  // (garbage once, in main)

// One step the way the device form runs it; the caps are the vectors' sizes.
Counts run_step(const std::vector<ufc_frame_info>& infos, const std::vector<ufc_item>& items, const std::vector<uint8_t>& payload,
                const std::vector<uint64_t>& frame_first, std::vector<ufc_receiver>& receivers, std::vector<ufc_rx_slot>& slots,
                const std::vector<uint64_t>& slot_first, const std::vector<uint8_t>& carry_in, std::vector<uint8_t>& carry_out,
                std::vector<ufc_rx_packet>& packets, std::vector<uint8_t>& out_bytes, std::vector<ufc_receiver_result>& results) {
  const uint64_t nr = receivers.size(), ni = items.size(), ns = slots.size();
  std::vector<uint64_t> carry_first(nr + 1), packet_first(nr + 1), out_first(nr + 1);
  std::vector<uint8_t> status(ni);
  uint64_t used[3];
  // (the carries live in uint64 storage: the core reads and writes their bit words as such)
  std::vector<uint64_t> cin((carry_in.size() + 7) / 8), cout((carry_out.size() + 7) / 8);
  if (!carry_in.empty()) std::memcpy(cin.data(), carry_in.data(), carry_in.size());
  RxArgs a{infos.data(), infos.size(), nullptr, items.data(), ni, nullptr, payload.data(), payload.size(),
           frame_first.data(), receivers.data(), nr, slots.data(), slot_first.data(), ns, (const uint8_t*)cin.data(),
           carry_in.size(), (uint8_t*)cout.data(), carry_out.size(), carry_first.data(), &used[0], packets.data(),
           packets.size(), packet_first.data(), &used[1], out_bytes.data(), out_bytes.size(), &used[2], status.data(),
           results.data(), receivers.data()};
  std::vector<RxPlan> plans(ns);
  std::vector<unsigned long long> table(rx_dup_entries(ni), 0ull);
  const RxDupSet dups{table.data(), table.size() - 1};
  std::vector<uint64_t> c0(nr + 1, 0), c1(nr + 1, 0), c2(nr + 1, 0);
  if (g_form == kWalkSerial) {
    for (uint64_t r = 0; r < nr; r++) {
      uint64_t c[3];
      rx_walk(a, r, plans.data(), status.data(), dups, c);
      c0[r] = c[0], c1[r] = c[1], c2[r] = c[2];
    }
  } else {
    // the device form's launches: begin; the item-parallel verdicts (frames in any order: last first here); the
    // items the verdicts let through; receive in tiles of 64 ids; end
    std::vector<uint8_t> verdicts(ni, 0xEE);
    for (uint64_t r = 0; r < nr; r++) rx_walk_begin(a, r, plans.data());
    for (uint64_t r = nr; r-- > 0;)
      if (results[r].stop == UFC_RX_DONE)
        for (uint64_t i = frame_first[r + 1]; i-- > frame_first[r];) rx_frame_verdicts(a, r, i, verdicts.data());
    for (uint64_t r = 0; r < nr; r++) rx_walk_items(a, r, plans.data(), status.data(), dups, verdicts.data());
    for (uint64_t r = 0; r < nr; r++) {
      RxWaveShared fresh;
      std::memset((void*)&fresh, 0xCD, sizeof fresh);
      RxWaveShared& sh = g_form == kCarried ? carried_block : fresh;
      uint32_t d;
      uint64_t o, c[3];
      if (g_form == kBackwards) rx_receive_tiles(lane_orders::ReverseWave{}, sh, a, r, plans.data(), d, o);
      else if (g_form == kShuffled) rx_receive_tiles(lane_orders::ShuffledWave{}, sh, a, r, plans.data(), d, o);
      else rx_receive_tiles(SerialWave{}, sh, a, r, plans.data(), d, o);
      rx_walk_end(a, r, d, o, c);
      c0[r] = c[0], c1[r] = c[1], c2[r] = c[2];
    }
  }
  uint64_t s0 = 0, s1 = 0, s2 = 0;
  for (uint64_t r = 0; r <= nr; r++) {
    packet_first[r] = s0, out_first[r] = s1, carry_first[r] = s2;
    s0 += c0[r], s1 += c1[r], s2 += c2[r];
  }
  std::vector<RxSegment> segs(2 * ns + ni);
  std::memset((void*)segs.data(), 0, segs.size() * sizeof(RxSegment));
  for (uint64_t r = 0; r < nr; r++) rx_finish(a, r, plans.data(), status.data(), out_first[r], segs.data(), nullptr);
  auto ends = [&](const RxSegment& sg, uint8_t*& dst, const uint8_t*& src, uint64_t& len) {
    const bool to_carry = (sg.kinds & kRxDstCarry) != 0;
    const uint64_t cap = to_carry ? a.carry_cap : a.out_cap;
    if (sg.len == 0 || sg.dst >= cap) return false;
    len = std::min<uint64_t>(sg.len, cap - sg.dst);
    dst = (to_carry ? a.carry_out : a.out_bytes) + sg.dst;
    src = ((sg.kinds & kRxSrcCarry) ? a.carry_in : a.payload) + sg.src;
    return true;
  };
  // the slot copy: chunk counts, their prefix, a binary search per chunk
  const uint64_t n_segs = 2 * ns;
  std::vector<uint32_t> first(n_segs + 1, 0);
  for (uint64_t k = 0; k < n_segs; k++) first[k + 1] = first[k] + (segs[k].len + kChunk - 1) / kChunk;
  for (uint64_t c = 0; c < first[n_segs]; c++) {
    uint64_t lo = 0, hi = n_segs - 1;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    uint8_t* dst;
    const uint8_t* src;
    uint64_t len;
    if (!ends(segs[lo], dst, src, len)) continue;
    const uint64_t at = (c - first[lo]) * kChunk;
    if (at < len) std::memcpy(dst + at, src + at, std::min<uint64_t>(kChunk, len - at));
    checks++;
  }
  for (uint64_t g = 0; g < ni; g++) {
    uint8_t* dst;
    const uint8_t* src;
    uint64_t len;
    if (ends(segs[n_segs + g], dst, src, len)) std::memcpy(dst, src, len);
  }
  if (!carry_out.empty()) std::memcpy(carry_out.data(), cout.data(), carry_out.size());
  return Counts{s0, s1, s2};
}

// The same step by the serial walk and by the device form's parts: every output byte for byte.
void both_ways(int where, const std::vector<ufc_frame_info>& infos, const std::vector<ufc_item>& items,
               const std::vector<uint8_t>& payload, const std::vector<uint64_t>& frame_first,
               const std::vector<ufc_receiver>& receivers, const std::vector<ufc_rx_slot>& slots,
               const std::vector<uint64_t>& slot_first, const std::vector<uint8_t>& carry, size_t carry_cap, size_t packets_cap,
               size_t out_cap) {
  std::vector<ufc_receiver> r1 = receivers;
  std::vector<ufc_rx_slot> s1 = slots;
  std::vector<ufc_receiver_result> q1(receivers.size());
  std::vector<uint8_t> c1(carry_cap), o1(out_cap);
  std::vector<ufc_rx_packet> p1(packets_cap);
  if (!p1.empty()) std::memset((void*)p1.data(), 0, p1.size() * sizeof(ufc_rx_packet));
  g_form = kWalkSerial;
  const Counts a = run_step(infos, items, payload, frame_first, r1, s1, slot_first, carry, c1, p1, o1, q1);
  for (int form = kForwards; form < kForms; form++) {
    std::vector<ufc_receiver> r2 = receivers;
    std::vector<ufc_rx_slot> s2 = slots;
    std::vector<ufc_receiver_result> q2(receivers.size());
    std::vector<uint8_t> c2(carry_cap), o2(out_cap);
    std::vector<ufc_rx_packet> p2(packets_cap);
    if (!p2.empty()) std::memset((void*)p2.data(), 0, p2.size() * sizeof(ufc_rx_packet));
    g_form = form;
    const Counts b = run_step(infos, items, payload, frame_first, r2, s2, slot_first, carry, c2, p2, o2, q2);
    g_form = kWalkSerial;
    if (a.packets != b.packets || a.out != b.out || a.carry != b.carry) fail("tiled: used counts", where, form, (long)b.out);
    if (std::memcmp((void*)r1.data(), (void*)r2.data(), r1.size() * sizeof(ufc_receiver))) fail("tiled: headers", where, form, 0);
    if (!s1.empty() && std::memcmp((void*)s1.data(), (void*)s2.data(), s1.size() * sizeof(ufc_rx_slot))) fail("tiled: slots", where, form, 0);
    if (std::memcmp((void*)q1.data(), (void*)q2.data(), q1.size() * sizeof(ufc_receiver_result))) fail("tiled: results", where, form, 0);
    if (!p1.empty() && std::memcmp((void*)p1.data(), (void*)p2.data(), p1.size() * sizeof(ufc_rx_packet))) fail("tiled: records", where, form, 0);
    if (c1 != c2 || o1 != o2) fail("tiled: bytes", where, form, 0);
    checks++;
  }
}

// ---- the cross-lane reads of rx_receive_tiles on lane 63 and on lane 0 of the second tile ----
// One fresh receiver of window W at `base` (the ids wrap inside the window), one-fragment packets at the given
// leads, one step: every form against the serial walk (both_ways), then the expectation written out here.  The same
// cases, with the same numbers, are scenarios of tests/test_receive_cpu.py.
struct Dgm {
  uint32_t lead, ch, wl, cl, len;
};
struct Got {
  std::vector<uint32_t> leads, lens, offsets;  // the delivered packets, in order
  ufc_receiver out;
  ufc_receiver_result res;
};
Got directed(int where, uint32_t W, uint32_t base, const std::vector<Dgm>& dgs) {
  std::vector<ufc_receiver> receivers(1);
  ufc_receiver h{};
  h.base_id = h.end_id = base;
  h.window_size = W;
  h.deliver = 1;
  h.resync_id = kNone;
  h.max_alloc = 1ull << 40;
  for (auto& c : h.channel_base_id) c = kNone;
  receivers[0] = h;
  std::vector<ufc_rx_slot> slots(W);
  std::memset((void*)slots.data(), 0, slots.size() * sizeof(ufc_rx_slot));
  const std::vector<uint64_t> slot_first = {0, W}, frame_first = {0, 1};
  std::vector<ufc_item> items;
  std::vector<uint8_t> payload(3);
  for (const Dgm& d : dgs) {
    ufc_item it{};
    it.id = (base + d.lead) & kMask;
    it.channel_id = (uint8_t)d.ch;
    it.window_parent_lead = (uint16_t)d.wl;
    it.channel_parent_lead = (uint16_t)d.cl;
    it.data_len = d.len;
    it.data_offset = (uint32_t)payload.size();
    for (uint32_t k = 0; k < d.len; k++) payload.push_back((uint8_t)(d.lead + k));
    items.push_back(it);
  }
  ufc_frame_info f{};
  f.kind = UFC_FRAME_DATA;
  f.ok = 1;
  f.item_count = (uint32_t)items.size();
  const std::vector<ufc_frame_info> infos(1, f);
  const std::vector<uint8_t> carry;
  std::vector<ufc_receiver> rc = receivers;
  std::vector<ufc_rx_slot> sc = slots;
  std::vector<ufc_receiver_result> results(1);
  std::vector<uint8_t> none8;
  std::vector<ufc_rx_packet> nonep;
  const Counts need = run_step(infos, items, payload, frame_first, rc, sc, slot_first, carry, none8, nonep, none8, results);
  both_ways(where, infos, items, payload, frame_first, receivers, slots, slot_first, carry, need.carry, need.packets, need.out);
  std::vector<uint8_t> carry_out(need.carry), out_bytes(need.out);
  std::vector<ufc_rx_packet> packets(need.packets);
  run_step(infos, items, payload, frame_first, receivers, slots, slot_first, carry, carry_out, packets, out_bytes, results);
  Got g;
  g.out = receivers[0];
  g.res = results[0];
  if (g.res.stop != UFC_RX_DONE || g.res.packet_count != need.packets) fail("directed: stop", where, g.res.stop, 0);
  for (const ufc_rx_packet& p : packets) {
    const uint32_t lead = (p.sequence_id - base) & kMask;
    g.leads.push_back(lead), g.lens.push_back(p.len), g.offsets.push_back((uint32_t)p.out_offset);
    for (uint32_t k = 0; k < p.len; k++)
      if (out_bytes[p.out_offset + k] != (uint8_t)(lead + k)) fail("directed: bytes", where, lead, k);
  }
  return g;
}

void directed_cases() {
  const uint32_t base = 0xFFFFF - 20;  // (the ids wrap at lead 21)
  const auto want_leads = [](int where, const Got& g, const std::vector<uint32_t>& want) {
    if (g.leads != want) fail("directed: delivered", where, (long)g.leads.size(), g.leads.empty() ? -1 : (long)g.leads.back());
  };
  for (int seam = 0; seam < 2; seam++) {
    // the event's lead: 63, the last lane of a full tile (window 64), or 64, lane 0 of the second tile (window 128);
    // the lane before it in its channel or among the entries is lead 60
    const uint32_t W = seam ? 128 : 64, ev = seam ? 64 : 63, gap = ev - 60;
    {  // DATA: delivered only against the base lead 60 leaves (61: ev - 61 < gap); against the carried base, none
       // (measured from the window's base: ev >= gap), it would fail.  (Its window parent, the id before it, never
       // came: the window stops in front of it.)
      const Got g = directed(10 + seam, W, base, {{60, 4, 0, 0, 5}, {ev, 4, 1, gap, 6}});
      want_leads(10 + seam, g, {60, ev});
      if (g.out.channel_packet_count[4] != 0 || g.out.channel_ready_flags != 0 || g.out.base_id != ((base + 61) & kMask))
        fail("directed: channel base from the lane before", seam, g.out.channel_packet_count[4], (long)g.out.base_id);
    }
    {  // ENTRY: the advance passes only against the new base lead 60 leaves
      const Got g = directed(20 + seam, W, base, {{60, 4, 0, 0, 5}, {ev, 5, gap, 0, 6}});
      want_leads(20 + seam, g, {60, ev});
      if (g.out.base_id != ((base + ev + 1) & kMask) || g.res.advanced != ev + 1 || g.out.alloc != 0)
        fail("directed: entry prefix from the lane before", seam, (long)g.out.base_id, g.res.advanced);
    }
    {  // the event's lane is the only failing lane of its channel (its parent, two before it, never came): not
       // delivered, the ready flag cleared, one packet left; the window stops in front of it too
      const Got g = directed(30 + seam, W, base, {{10, 4, 0, 0, 5}, {20, 4, 0, 0, 7}, {ev, 4, 2, 2, 6}, {5, 9, 0, 0, 1}});
      want_leads(30 + seam, g, {5, 10, 20});
      if (g.out.channel_packet_count[4] != 1 || g.out.channel_ready_flags != 0 || g.out.base_id != ((base + 21) & kMask) ||
          g.out.channel_base_id[4] != kNone)
        fail("directed: the only failing lane", seam, g.out.channel_packet_count[4], (long)g.out.channel_ready_flags);
    }
  }
  {  // 128 ids delivered, lengths 1 but 200 at lead 63 and 77 at lead 64: tile 2's offsets carry lane 63's length
    std::vector<Dgm> d;
    for (uint32_t k = 0; k < 128; k++) d.push_back(Dgm{k, 4, k ? 1u : 0u, k ? 1u : 0u, k == 63 ? 200u : k == 64 ? 77u : 1u});
    const Got g = directed(40, 128, base, d);
    uint32_t at = 0;
    for (uint32_t k = 0; k < 128; k++) {
      if (g.leads.size() != 128 || g.leads[k] != k || g.offsets[k] != at || g.lens[k] != d[k].len) fail("directed: offsets", k, at, 0);
      at += d[k].len;
    }
    if (at != 126 + 277 || g.out.base_id != ((base + 128) & kMask)) fail("directed: 128 delivered", at, 0, 0);
  }
}

}  // namespace

int main() {
  std::memset((void*)&carried_block, 0xCD, sizeof carried_block);
  directed_cases();
  const uint32_t W = 16, R = 5;
  static const uint32_t sizes[] = {0, 1, 77, kFrag - 1, kFrag, kFrag + 1, 3000, 64 * kFrag, 65 * kFrag - 3};
  std::vector<Peer> peers(R);
  std::vector<ufc_receiver> receivers(R);
  std::vector<ufc_rx_slot> slots(R * W);
  std::memset((void*)slots.data(), 0, slots.size() * sizeof(ufc_rx_slot));
  std::vector<uint64_t> slot_first(R + 1);
  for (uint32_t r = 0; r <= R; r++) slot_first[r] = (uint64_t)r * W;
  for (uint32_t r = 0; r < R; r++) {
    ufc_receiver h{};
    h.base_id = h.end_id = (0xFFFFF - 7 * r) & kMask;
    h.window_size = W;
    h.deliver = 1;
    h.resync_id = kNone;
    h.max_alloc = 1ull << 40;
    for (auto& c : h.channel_base_id) c = kNone;
    receivers[r] = h;
    peers[r].next_id = h.base_id;
  }
  std::vector<uint8_t> carry;
  const int steps = 60, feed = 40;
  for (int step = 0; step < steps; step++) {
    std::vector<ufc_frame_info> infos;
    std::vector<ufc_item> items;
    std::vector<uint8_t> payload(1 + rnd() % 7);  // an odd start
    std::vector<uint64_t> frame_first(R + 1, 0);
    for (uint32_t r = 0; r < R; r++) {
      Peer& p = peers[r];
      if (step < feed)
        for (uint32_t k = rnd() % 6; k > 0 && ((p.next_id - receivers[r].base_id) & kMask) < W; k--)
          send_packet(p, sizes[rnd() % (sizeof(sizes) / sizeof(sizes[0]))]);
      // a random part of what is in flight (everything in the last steps), shuffled, some of it twice
      std::vector<Dg> now, later;
      for (const Dg& d : p.flight) {
        const bool take = step >= steps - 3 || rnd() % 3 != 0;
        (take ? now : later).push_back(d);
        if (take && rnd() % 8 == 0) now.push_back(d);
      }
      p.flight.swap(later);
      for (size_t k = now.size(); k > 1; k--) std::swap(now[k - 1], now[rnd() % k]);
      // datagrams the receiver must drop without a trace: right behind a fragment of the same packet one that
      // names other leads or another fragment count (MISMATCH, or CLOSED once the packet is whole), and anywhere
      // invalid ones, ids past 2^20 or past the window, and payload ranges outside the arena
      for (size_t k = 0; k < now.size(); k++) {
        const uint32_t u = rnd() % 16;
        if (u > 4) continue;
        Dg j = now[k];
        if (u == 0 && j.it.fragment_id_last > 0) j.it.fragment_id_last++, j.it.fragment_id = 0;
        else if (u == 0 || u == 1) j.it.window_parent_lead = j.it.channel_parent_lead = 0xFFFF;
        else if (u == 2) j.it.fragment_id = (uint16_t)(j.it.fragment_id_last + 1);
        else if (u == 3) j.it.id = (rnd() & 1) ? (j.it.id | 0x100000u) : ((receivers[r].base_id + W + rnd() % 900) & kMask);
        else j.bad_src = true;
        if (u <= 1 && j.it.fragment_id_last == 0) continue;  // (a one-fragment twin could open the slot itself)
        now.insert(now.begin() + (long)k + 1, j);
        k++;
      }
      for (size_t k = 0; k < now.size(); k++) {
        if (k % 5 == 0) {
          ufc_frame_info f{};
          f.kind = UFC_FRAME_DATA;
          f.ok = 1;
          f.item_first = (uint32_t)items.size();
          infos.push_back(f);
        }
        Dg d = now[k];
        const Sent& s = p.sent[d.packet];
        d.it.data_offset = (uint32_t)payload.size();
        payload.insert(payload.end(), s.data.begin() + (size_t)d.frag * kFrag,
                       s.data.begin() + (size_t)d.frag * kFrag + d.it.data_len);
        if (d.bad_src) d.it.data_offset = 0xFFFFFF00u + rnd() % 255;
        items.push_back(d.it);
        infos.back().item_count++;
      }
      frame_first[r + 1] = infos.size();
    }
    // caps of zero on a copy of the state: the used counts
    std::vector<ufc_receiver> rc = receivers;
    std::vector<ufc_rx_slot> sc = slots;
    std::vector<ufc_receiver_result> results(R);
    std::vector<uint8_t> none8;
    std::vector<ufc_rx_packet> nonep;
    const Counts need = run_step(infos, items, payload, frame_first, rc, sc, slot_first, carry, none8, nonep, none8, results);
    std::vector<uint8_t> carry_out(need.carry), out_bytes(need.out);
    std::vector<ufc_rx_packet> packets(need.packets);
    both_ways(step, infos, items, payload, frame_first, receivers, slots, slot_first, carry, need.carry, need.packets, need.out);
    const Counts got = run_step(infos, items, payload, frame_first, receivers, slots, slot_first, carry, carry_out, packets,
                                out_bytes, results);
    if (got.packets != need.packets || got.out != need.out || got.carry != need.carry)
      fail("used counts differ between the dry and the real pass", step, (long)got.out, (long)need.out);
    if (std::memcmp((void*)rc.data(), (void*)receivers.data(), R * sizeof(ufc_receiver)) != 0)
      fail("the state depends on the caps", step, 0, 0);
    // the delivered packets against the senders' record
    for (uint32_t r = 0; r < R; r++) {
      Peer& p = peers[r];
      if (results[r].stop != UFC_RX_DONE) fail("stop", step, r, results[r].stop);
      for (uint32_t k = 0; k < results[r].packet_count; k++) {
        const ufc_rx_packet& rec = packets[results[r].packet_first + k];
        const uint32_t ch = rec.channel_id;
        if (ch > 2 || rec.flags != 0) fail("record", step, r, k);
        size_t j = 0, seen = 0;  // the delivered[ch]-th packet sent on this channel
        for (; j < p.sent.size(); j++)
          if (p.sent[j].channel == ch && seen++ == p.delivered[ch]) break;
        if (j == p.sent.size()) fail("more delivered than sent", step, r, ch);
        const Sent& s = p.sent[j];
        if (s.seq != rec.sequence_id || s.data.size() != rec.len) fail("order or length", step, (long)s.seq, (long)rec.sequence_id);
        if (rec.len && std::memcmp(out_bytes.data() + rec.out_offset, s.data.data(), rec.len) != 0)
          fail("bytes", step, r, (long)rec.sequence_id);
        p.delivered[ch]++;
        checks++;
      }
    }
    carry.swap(carry_out);
  }
  for (uint32_t r = 0; r < R; r++) {
    const Peer& p = peers[r];
    if (p.delivered[0] + p.delivered[1] + p.delivered[2] != p.sent.size() || !p.flight.empty())
      fail("packets missing at the end", r, (long)p.sent.size(), (long)p.delivered[0]);
    if (receivers[r].alloc != 0 || receivers[r].base_id != p.next_id) fail("final state", r, (long)receivers[r].alloc, 0);
  }
  if (!carry.empty()) fail("carry left", (long)carry.size(), 0, 0);
  // Hostile state: headers, slots and items of random bytes (window sizes, ids and carry offsets kept near
  // what passes the state check, so that the walk and the finish run on them).  Nothing is expected but that
  // every access stays inside the exact-size buffers.
  long wide_done = 0, wide_delivered = 0, wide_advanced = 0;
  for (int round = 0; round < 400; round++) {
    const uint32_t Wf = 1u << (rnd() % 9), Rf = 1 + rnd() % 3;  // (up to four tiles of ids)
    std::vector<uint8_t> cin(8 * (rnd() % 600));
    for (auto& b : cin) b = (uint8_t)rnd();
    std::vector<ufc_receiver> rv(Rf);
    std::vector<ufc_rx_slot> sl(Rf * Wf + rnd() % 2);
    std::vector<uint64_t> sf(Rf + 1), ff(Rf + 1);
    std::vector<ufc_frame_info> fi(Rf * 2);
    std::vector<ufc_item> it(fi.size() * 4);
    std::vector<uint8_t> pay(rnd() % 3000);
    auto fill = [&](void* p, size_t n) { for (size_t k = 0; k < n; k++) ((uint8_t*)p)[k] = (uint8_t)rnd(); };
    fill(rv.data(), rv.size() * sizeof(ufc_receiver));
    fill(sl.data(), sl.size() * sizeof(ufc_rx_slot));
    fill(it.data(), it.size() * sizeof(ufc_item));
    fill(pay.data(), pay.size());
    for (uint32_t r = 0; r <= Rf; r++) sf[r] = (uint64_t)r * Wf, ff[r] = (uint64_t)r * 2;
    if (rnd() % 16 == 0) std::swap(ff[0], ff[Rf]);
    for (uint32_t r = 0; r < Rf; r++) {
      ufc_receiver& h = rv[r];
      h.window_size = rnd() % 8 ? Wf : rnd() % 9;
      h.base_id &= rnd() % 8 ? kMask : 0x1FFFFFu;
      h.end_id = (h.base_id + rnd() % (2 * Wf + 2)) & kMask;
      h.resync_id = rnd() % 2 ? kNone : h.base_id + rnd() % (Wf + 3);
      h.max_alloc = rnd() % 2 ? rnd() % 20000 : ~0ull;
      h.alloc = rnd() % 4 ? rnd() % 9000 : h.alloc;
      for (auto& c : h.channel_base_id)
        if (rnd() % 2) c = kNone; else c = (h.base_id + rnd() % (Wf + 2)) & kMask;
    }
    for (auto& s : sl) {
      s.asm_state %= (rnd() % 16 ? 3 : 4);
      s.asm_channel_id %= (rnd() % 16 ? 64 : 65);
      s.rx_channel_id %= 64;
      s.asm_last_fragment_id %= 4;
      s.data_len %= 700;
      s.data_offset = cin.empty() ? 0 : 8 * (rnd() % (cin.size() / 8 + 1)) + (rnd() % 32 ? 0 : 1);
      if (rnd() % 64) {  // most slots tame, so that wide windows pass the state check and run several tiles
        s.asm_state %= 2, s.asm_channel_id %= 64, s.data_len %= 40, s.data_offset = 0;
        if (cin.size() < 40) s.rx_flags &= (uint8_t)~UFC_RX_SLOT_DATA;
      }
    }
    bool shared = false;  // (what frames that share items give is unspecified: such rounds only have to stay in bounds)
    for (size_t f = 0; f < fi.size(); f++) {
      ufc_frame_info x{};
      x.kind = rnd() % 8 ? UFC_FRAME_DATA : UFC_FRAME_ACK;
      x.ok = rnd() % 8 != 0;
      x.item_first = (uint32_t)(f * 4) + (rnd() % 32 ? 0 : 3);  // (frames that share items, or leave the array)
      shared = shared || x.item_first != f * 4;
      x.item_count = rnd() % 5;
      fi[f] = x;
    }
    for (size_t g = 0; g < it.size(); g++) {
      ufc_item& x = it[g];
      const ufc_receiver& h = rv[(g / 8) % Rf];
      x.id = rnd() % 8 ? (h.base_id + rnd() % (Wf + 1)) & kMask : x.id;
      x.channel_id %= (rnd() % 16 ? 4 : 70);
      x.fragment_id_last %= 4;
      x.fragment_id %= 5;
      x.window_parent_lead %= 4, x.channel_parent_lead %= 4;
      x.data_len = x.fragment_id < x.fragment_id_last || rnd() % 4 == 0 ? kFrag : rnd() % 1500;
      x.data_offset = rnd() % 8 ? rnd() % (uint32_t)(pay.size() + 1) : x.data_offset;
    }
    std::vector<ufc_receiver_result> res(Rf);
    std::vector<ufc_receiver> rc = rv;
    std::vector<ufc_rx_slot> sc = sl;
    std::vector<uint8_t> none8;
    std::vector<ufc_rx_packet> nonep;
    const Counts need = run_step(fi, it, pay, ff, rc, sc, sf, cin, none8, nonep, none8, res);
    // (a region a hostile slot claims may be huge: such rounds run with clipped buffers, as a caller's caps would)
    std::vector<uint8_t> co(8 * (std::min<uint64_t>(need.carry, 1 << 22) / 8)), ob(std::min<uint64_t>(need.out, 1 << 22));
    std::vector<ufc_rx_packet> pk(need.packets);
    if (!shared) both_ways(1000 + round, fi, it, pay, ff, rv, sl, sf, cin, co.size(), pk.size(), ob.size());
    const Counts got = run_step(fi, it, pay, ff, rv, sl, sf, cin, co, pk, ob, res);
    if (got.packets != need.packets || got.out != need.out || got.carry != need.carry) fail("fuzz: used counts", round, 0, 0);
    for (uint32_t r = 0; r < Rf; r++)
      if (res[r].stop == UFC_RX_DONE && Wf > 64) wide_done++, wide_delivered += res[r].packet_count, wide_advanced += res[r].advanced;
    checks++;
  }
  if (wide_done < 30 || wide_delivered < 500 || wide_advanced < 500)
    fail("fuzz: too few steps over several tiles", wide_done, wide_delivered, wide_advanced);
  std::printf("ok: %ld\n", checks);
  return 0;
}
