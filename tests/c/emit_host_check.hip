// The emit core (uflow_amd/csrc/frame_codec_core.hpp: emit_alloc_size, emit_fragment_count, emit_lead,
// emit_packet_class, emit_max_alloc, emit_window_room, emit_alloc_fails, emit_item) as host code under
// AddressSanitizer and UBSan.  Seeded senders are emitted twice: by the serial walk of
// src/half_connection/packet_sender.rs:149-238 and pending_packet.rs:23-42, 84-103, restated here packet by
// packet with plain arithmetic (none of the core's functions), and by the tile form the GPU emit takes
// (packet_emit.hip): 64 packets at a time, ballots as 64-bit masks, ranks and prefix sums over the lanes, the
// stop by find-first, the window parent from the reliable lanes below, the channel parent from 64 per-channel
// lane masks and a 64-entry table carried across tiles, then the item search (the sender in flush_first, the
// packet among the sender's first items) for every item slot.  All buffers have their exact sizes.  Both must
// agree in every item, result and state field.  The tile form keeps the kernel's shape where a lane reads
// another's value: the three carries are lane 63's inclusive sums, the item search is narrowed to the senders
// of a workgroup's 256 slots first, and the finish pass runs in both of its lane widths.
// directed_cases() places stops, parents and carried sums on lane 63 and on lane 0 of the next tile, and
// senders on the seams of the item search (tests/emit_expect.py lane_cases, the same numbers), and compares
// with literals as well.
// Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../uflow_amd/csrc/frame_codec_core.hpp"

namespace {

long checks = 0;

void fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  std::exit(1);
}

uint64_t rng_state = 0xE317C0DEu;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

constexpr uint32_t kMask = 0xFFFFF, kFrag = 1448;

struct Out {
  std::vector<ufc_item> items;  // reserved slots: id = 0xFFFFFFFF marks "untouched"
  std::vector<ufc_packet_result> pres;
  ufc_sender_result res;
  ufc_sender state;
};

ufc_item untouched() {
  ufc_item it;
  std::memset(&it, 0xA5, sizeof it);
  return it;
}

// packet_sender.rs and pending_packet.rs, packet by packet.
Out serial_walk(const ufc_packet* q, uint64_t n_range, const ufc_sender& sd) {
  Out o{};
  o.state = sd;
  o.pres.assign(n_range, ufc_packet_result{});
  for (uint32_t k = 0; k < sd.reserve_items; k++) o.items.push_back(untouched());
  const uint64_t max_alloc = sd.max_alloc % kFrag ? sd.max_alloc + (kFrag - sd.max_alloc % kFrag) : sd.max_alloc;
  const uint64_t n = n_range < sd.take ? n_range : sd.take;
  ufc_sender& st = o.state;
  uint64_t i = 0;
  o.res.stop = UFC_EMIT_DONE;
  for (; i < n; i++) {
    const ufc_packet& p = q[i];
    if (p.channel_id >= 64 || p.mode > 3 || p.data_len > kFrag * 65536u) {
      o.res.stop = UFC_EMIT_BAD_PACKET;
      break;
    }
    if (p.mode == 0 && p.flush_id != sd.flush_id) {
      o.res.packets_dropped++;
      o.res.bytes_dropped += p.data_len;
      o.pres[i].status = UFC_PACKET_DROPPED;
      continue;
    }
    if (((st.next_id - st.base_id) & kMask) >= st.window_size) {
      o.res.stop = UFC_EMIT_WINDOW_LIMITED;
      break;
    }
    const uint64_t len = p.data_len;
    const uint64_t a = len > kFrag ? (len + kFrag - 1) / kFrag * kFrag : len;
    if (st.alloc + a > max_alloc) {
      o.res.stop = UFC_EMIT_ALLOC_LIMITED;
      break;
    }
    const uint32_t seq = st.next_id;
    const uint32_t wp = st.window_parent_id, cp = st.channel_parent_id[p.channel_id];
    const uint16_t wl = wp == UFC_NO_PARENT ? 0 : (uint16_t)((seq - wp) & kMask);
    const uint16_t cl = cp == UFC_NO_PARENT ? 0 : (uint16_t)((seq - cp) & kMask);
    st.next_id = (st.next_id + 1) & kMask;
    st.alloc += a;
    if (p.mode == 3) st.window_parent_id = st.channel_parent_id[p.channel_id] = seq;
    const uint32_t num = (uint32_t)((len + kFrag - 1) / kFrag) + (len == 0 ? 1 : 0);
    o.pres[i].sequence_id = seq;
    o.pres[i].item_first = (uint32_t)o.items.size();
    o.pres[i].item_count = num;
    o.pres[i].status = UFC_PACKET_EMITTED;
    o.pres[i].resend = p.mode >= 2;
    for (uint32_t f = 0; f < num; f++) {
      ufc_item it{};
      it.id = seq;
      it.channel_id = p.channel_id;
      it.window_parent_lead = wl;
      it.channel_parent_lead = cl;
      it.fragment_id = (uint16_t)f;
      it.fragment_id_last = (uint16_t)(num - 1);
      it.data_offset = p.data_offset + kFrag * f;
      it.data_len = f == num - 1 ? (uint32_t)(len - (uint64_t)kFrag * f) : kFrag;
      it.form = num > 1 ? 2 : (it.data_len < 64 && wl < 128 && cl < 256) ? 0 : it.data_len < 256 ? 1 : 2;  // build.rs:81-122
      const bool valid = !(cl != 0 && (wl == 0 || cl < wl));  // packet_receiver/mod.rs:12-30, the rest holds
      it.flags = valid ? UFC_ITEM_VALID : 0;
      o.items.push_back(it);
    }
    o.res.packets_emitted++;
  }
  o.res.packets_consumed = (uint32_t)i;
  o.res.item_count = (uint32_t)o.items.size();
  return o;
}

int popc(uint64_t m) { return __builtin_popcountll(m); }
uint32_t high_bit(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }

// packet_emit.hip's sender kernel for one sender: rel_first and meta are the sender's slices of the scratch
// (exactly n_range entries), pres its slice of the packet results.
void tile_form(const ufc_packet* q, uint64_t n_range, const ufc_sender& sd, uint32_t* rel_first, uint64_t* meta,
               ufc_packet_result* pres, ufc_sender_result& res, ufc_sender& state, uint64_t& count) {
  uint64_t mask[64];
  uint32_t parent[64];
  for (int c = 0; c < 64; c++) mask[c] = 0, parent[c] = sd.channel_parent_id[c];
  const uint64_t n = n_range < sd.take ? n_range : sd.take;
  const uint32_t room = ufc_codec::emit_window_room(sd.base_id, sd.next_id, sd.window_size);
  const uint64_t max_alloc = ufc_codec::emit_max_alloc(sd.max_alloc);
  uint32_t rank_base = 0, dropped = 0, wparent = sd.window_parent_id, why = UFC_EMIT_DONE;
  uint64_t A_base = 0, made = sd.reserve_items, dropped_bytes = 0, stop = n, done = 0;
  bool stopped = false;
  for (uint64_t t0 = 0; t0 < n && !stopped; t0 += 64) {
    const uint32_t nv = (uint32_t)(n - t0 < 64 ? n - t0 : 64);
    ufc_packet pk[64];
    uint32_t cls[64], rank[64], y[64], fc[64];
    uint64_t a_sz[64], A_incl[64], A_ex[64], f_incl[64], f_ex[64], d_incl[64];
    uint64_t live_mask = 0;
    for (uint32_t l = 0; l < 64; l++) {
      pk[l] = ufc_packet{};
      cls[l] = ufc_codec::kEmitStale;
      if (l < nv) {
        pk[l] = q[t0 + l];
        cls[l] = ufc_codec::emit_packet_class(pk[l], sd.flush_id);
      }
      if (cls[l] == ufc_codec::kEmitLive) live_mask |= 1ull << l;
    }
    uint64_t run = 0, fail_mask = 0;
    for (uint32_t l = 0; l < 64; l++) {
      const bool live = (live_mask >> l) & 1;
      rank[l] = rank_base + (uint32_t)popc(live_mask & ((1ull << l) - 1));
      a_sz[l] = live ? ufc_codec::emit_alloc_size(pk[l].data_len) : 0;
      run += a_sz[l];
      A_incl[l] = run;
      A_ex[l] = A_base + A_incl[l] - a_sz[l];
      y[l] = UFC_EMIT_DONE;
      if (l < nv) {
        if (cls[l] == ufc_codec::kEmitBad)
          y[l] = UFC_EMIT_BAD_PACKET;
        else if (live && rank[l] >= room)
          y[l] = UFC_EMIT_WINDOW_LIMITED;
        else if (live && ufc_codec::emit_alloc_fails(sd.alloc, A_ex[l], a_sz[l], max_alloc))
          y[l] = UFC_EMIT_ALLOC_LIMITED;
      }
      if (y[l] != UFC_EMIT_DONE) fail_mask |= 1ull << l;
    }
    uint32_t limit = nv;
    if (fail_mask) {
      const uint32_t l = (uint32_t)__builtin_ctzll(fail_mask);
      limit = l;
      stop = t0 + l;
      why = y[l];
      A_base = A_ex[l];
      stopped = true;
    } else {
      A_base += A_incl[63];
    }
    uint64_t emit_mask = 0, drop_mask = 0, rel_mask = 0, frun = 0, drun = 0;
    for (uint32_t l = 0; l < 64; l++) {
      const bool in_prefix = l < limit;
      if (in_prefix && ((live_mask >> l) & 1)) emit_mask |= 1ull << l;
      if (in_prefix && cls[l] == ufc_codec::kEmitStale) drop_mask |= 1ull << l;
      fc[l] = (emit_mask >> l) & 1 ? ufc_codec::emit_fragment_count(pk[l].data_len) : 0;
      frun += fc[l];
      f_incl[l] = frun;
      f_ex[l] = made + (f_incl[l] - fc[l]);
      drun += (drop_mask >> l) & 1 ? (uint64_t)pk[l].data_len : 0;
      d_incl[l] = drun;
      if (((emit_mask >> l) & 1) && pk[l].mode == UFC_SEND_RELIABLE) rel_mask |= 1ull << l;
    }
    auto seq_of = [&](uint32_t h) -> uint32_t {
      return (sd.next_id + rank_base + (uint32_t)popc(live_mask & ((1ull << h) - 1))) & kMask;
    };
    for (uint32_t l = 0; l < 64; l++)
      if ((rel_mask >> l) & 1) mask[pk[l].channel_id] |= 1ull << l;
    for (uint32_t l = 0; l < nv; l++) {
      const uint64_t below = (1ull << l) - 1;
      const bool emitted = (emit_mask >> l) & 1;
      if (l < limit) rel_first[t0 + l] = (uint32_t)f_ex[l];
      pres[t0 + l] = ufc_packet_result{};
      if (emitted) {
        const uint32_t seq = (sd.next_id + rank[l]) & kMask;
        const uint32_t wp = rel_mask & below ? seq_of(high_bit(rel_mask & below)) : wparent;
        const uint64_t m = mask[pk[l].channel_id] & below;
        const uint32_t cp = m ? seq_of(high_bit(m)) : parent[pk[l].channel_id];
        meta[t0 + l] = seq | ((uint64_t)ufc_codec::emit_lead(seq, wp) << 32) | ((uint64_t)ufc_codec::emit_lead(seq, cp) << 48);
        pres[t0 + l].sequence_id = seq;
        pres[t0 + l].item_first = (uint32_t)f_ex[l];
        pres[t0 + l].item_count = fc[l];
        pres[t0 + l].status = UFC_PACKET_EMITTED;
        pres[t0 + l].resend = pk[l].mode >= UFC_SEND_PERSISTENT ? 1 : 0;
      } else if ((drop_mask >> l) & 1) {
        pres[t0 + l].status = UFC_PACKET_DROPPED;
      }
    }
    for (int c = 0; c < 64; c++)
      if (mask[c]) parent[c] = seq_of(high_bit(mask[c])), mask[c] = 0;
    if (rel_mask) wparent = seq_of(high_bit(rel_mask));
    rank_base += (uint32_t)popc(emit_mask);
    made += f_incl[63];
    if (drop_mask != 0) {
      dropped += (uint32_t)popc(drop_mask);
      dropped_bytes += d_incl[63];
    }
    done = t0 + nv;
  }
  for (uint64_t k = done; k < n_range; k++) pres[k] = ufc_packet_result{};
  res = ufc_sender_result{};
  res.item_count = (uint32_t)made;
  res.packets_consumed = (uint32_t)stop;
  res.packets_emitted = rank_base;
  res.packets_dropped = dropped;
  res.stop = why;
  res.bytes_dropped = dropped_bytes;
  state = sd;
  state.next_id = (sd.next_id + rank_base) & kMask;
  state.alloc = sd.alloc + A_base;
  state.window_parent_id = wparent;
  for (int c = 0; c < 64; c++) state.channel_parent_id[c] = parent[c];
  count = made;
}

ufc_packet random_packet(uint32_t flush_id, uint32_t& arena, bool allow_bad) {
  ufc_packet p{};
  const uint32_t t = rnd() % 16;
  p.data_len = t == 0 ? 0 : t < 6 ? rnd() % 64 : t < 10 ? rnd() % 300 : t < 12 ? 1446 + rnd() % 5 : t < 15 ? rnd() % 9000
               : 100000 + rnd() % 100000;
  p.mode = (uint8_t)(rnd() % 5 == 0 ? 0 : rnd() % 4);
  p.flush_id = rnd() % 3 ? flush_id : flush_id + 1 + rnd() % 2;
  p.channel_id = (uint8_t)(rnd() % 3 ? rnd() % 4 : rnd() % 64);
  if (allow_bad && rnd() % 400 == 0) {
    const uint32_t k = rnd() % 3;
    if (k == 0) p.channel_id = (uint8_t)(64 + rnd() % 192);
    if (k == 1) p.mode = (uint8_t)(4 + rnd() % 200);
    if (k == 2) p.data_len = 1448u * 65536u + 1 + rnd() % 5;
  }
  p.data_offset = arena;
  if (p.data_len <= 1448u * 65536u) arena += p.data_len;
  return p;
}

// The emit's launches over one batch in exactly-sized arrays (a read or write past an end is a sanitizer
// report), checked against the serial walk, whose outputs are returned.
std::vector<Out> run_batch(const std::vector<uint64_t>& first, const ufc_packet* packets_in, const ufc_sender* senders_in) {
  const uint32_t n_senders = (uint32_t)first.size() - 1;
  const uint64_t n_packets = first[n_senders];
  ufc_packet* packets = new ufc_packet[n_packets ? n_packets : 1];
  ufc_sender* senders = new ufc_sender[n_senders];
  for (uint64_t i = 0; i < n_packets; i++) packets[i] = packets_in[i];
  for (uint32_t s = 0; s < n_senders; s++) senders[s] = senders_in[s];
  uint32_t* rel_first = new uint32_t[n_packets ? n_packets : 1];
  uint64_t* meta = new uint64_t[n_packets ? n_packets : 1];
  ufc_packet_result* pres = new ufc_packet_result[n_packets ? n_packets : 1];
  ufc_sender_result* sres = new ufc_sender_result[n_senders];
  ufc_sender* sout = new ufc_sender[n_senders];
  uint64_t* flush_first = new uint64_t[n_senders + 1];
  std::vector<Out> ref(n_senders);
  for (uint32_t s = 0; s < n_senders; s++) ref[s] = serial_walk(packets + first[s], first[s + 1] - first[s], senders[s]);
  // launch 1, per sender; the scan
  flush_first[0] = 0;
  for (uint32_t s = 0; s < n_senders; s++) {
    uint64_t count = 0;
    tile_form(packets + first[s], first[s + 1] - first[s], senders[s], rel_first + first[s], meta + first[s],
              pres + first[s], sres[s], sout[s], count);
    flush_first[s + 1] = flush_first[s] + count;
  }
  const uint64_t total = flush_first[n_senders];
  ufc_item* items = new ufc_item[total ? total : 1];
  for (uint64_t g = 0; g < total; g++) items[g] = untouched();
  // launch 4: every item slot on its own
  auto sender_of = [&](uint64_t g, uint64_t lo, uint64_t hi) -> uint64_t {
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (flush_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  for (uint64_t g = 0; g < total; g++) {
    const uint64_t g0 = g / 256 * 256;  // the workgroup's slots: its senders first, then the slot's among them
    const uint64_t s_lo = sender_of(g0, 0, n_senders - 1);
    const uint64_t s_hi = sender_of((g0 + 256 < total ? g0 + 256 : total) - 1, s_lo, n_senders - 1);
    const uint64_t s = sender_of(g, s_lo, s_hi);
    if (!(flush_first[s] <= g && g < flush_first[s + 1])) fail("sender search", (long)g, (long)s, 0);
    const uint32_t consumed = sres[s].packets_consumed;
    if (consumed == 0) continue;
    const uint32_t r = (uint32_t)(g - flush_first[s]);
    const uint32_t* rf = rel_first + first[s];
    if (rf[0] > r) continue;
    uint32_t a = 0, b = consumed - 1;
    while (a < b) {
      const uint32_t mid = a + (b - a + 1) / 2;
      if (rf[mid] <= r) a = mid; else b = mid - 1;
    }
    const ufc_packet pk = packets[first[s] + a];
    const uint32_t f = r - rf[a], last = ufc_codec::emit_fragment_count(pk.data_len) - 1;
    if (f > last) fail("fragment past the packet", (long)g, (long)f, (long)last);
    const uint64_t m = meta[first[s] + a];
    items[g] = ufc_codec::emit_item(pk, (uint32_t)m, (uint16_t)(m >> 32), (uint16_t)(m >> 48), f, last);
  }
  // launch 3 in both widths, on copies: the emitted packets' first items made absolute
  for (uint32_t lanes : {8u, 64u}) {
    ufc_packet_result* abs_pres = new ufc_packet_result[n_packets ? n_packets : 1];
    for (uint64_t i = 0; i < n_packets; i++) abs_pres[i] = pres[i];
    for (uint32_t s = 0; s < n_senders; s++)
      for (uint32_t lane = 0; lane < lanes; lane++)
        for (uint32_t q = lane; q < sres[s].packets_consumed; q += lanes) {
          ufc_packet_result* pr = abs_pres + first[s] + q;
          if (pr->status == UFC_PACKET_EMITTED) pr->item_first += (uint32_t)flush_first[s];
        }
    for (uint32_t s = 0; s < n_senders; s++)
      for (uint64_t i = 0; i < first[s + 1] - first[s]; i++) {
        const ufc_packet_result& a = ref[s].pres[i];
        const ufc_packet_result& b = abs_pres[first[s] + i];
        if (b.status != a.status || b.item_first != a.item_first + (a.status == UFC_PACKET_EMITTED ? (uint32_t)flush_first[s] : 0u))
          fail("finish", (long)lanes, (long)s, (long)i);
      }
    checks++;
    delete[] abs_pres;
  }
  // against the serial walk
  for (uint32_t s = 0; s < n_senders; s++) {
    const Out& o = ref[s];
    const uint64_t n = first[s + 1] - first[s];
    ufc_sender_result want = o.res;
    if (std::memcmp(&want.item_count, &sres[s].item_count, sizeof want - sizeof want.item_first) != 0)
      fail("sender result", (long)s, (long)want.stop, (long)sres[s].stop);
    if (std::memcmp(&o.state, &sout[s], sizeof(ufc_sender)) != 0) fail("sender state", (long)s, 0, 0);
    if (flush_first[s + 1] - flush_first[s] != o.items.size()) fail("item count", (long)s, 0, 0);
    for (uint64_t i = 0; i < n; i++) {
      const ufc_packet_result& a = o.pres[i];
      const ufc_packet_result& b = pres[first[s] + i];
      if (a.sequence_id != b.sequence_id || a.item_first != b.item_first || a.item_count != b.item_count ||
          a.status != b.status || a.resend != b.resend)
        fail("packet result", (long)s, (long)i, (long)b.status);
      checks++;
    }
    for (uint64_t k = 0; k < o.items.size(); k++) {
      if (std::memcmp(&o.items[k], &items[flush_first[s] + k], sizeof(ufc_item)) != 0) fail("item", (long)s, (long)k, 0);
      checks++;
    }
  }
  delete[] packets;
  delete[] senders;
  delete[] rel_first;
  delete[] meta;
  delete[] pres;
  delete[] sres;
  delete[] sout;
  delete[] flush_first;
  delete[] items;
  return ref;
}

void check_batch(uint32_t n_senders, uint32_t max_queue) {
  std::vector<uint64_t> first(n_senders + 1, 0);
  for (uint32_t s = 0; s < n_senders; s++) first[s + 1] = first[s] + (rnd() % 4 == 0 ? 0 : rnd() % (max_queue + 1));
  const uint64_t n_packets = first[n_senders];
  std::vector<ufc_packet> packets(n_packets ? n_packets : 1);
  std::vector<ufc_sender> senders(n_senders);
  uint32_t arena = 0;
  for (uint32_t s = 0; s < n_senders; s++) {
    ufc_sender sd{};
    const uint64_t n = first[s + 1] - first[s];
    sd.base_id = rnd() & kMask;
    sd.next_id = (sd.base_id + rnd() % 50) & kMask;
    sd.flush_id = rnd() % 4;
    const uint32_t kind = rnd() % 3;
    sd.window_size = kind == 1 ? 1u << (rnd() % 9) : 4096;
    sd.alloc = rnd() % 100000;
    sd.max_alloc = kind == 2 ? sd.alloc + rnd() % 80000 : (uint64_t)1 << 40;
    if (rnd() % 16 == 0) sd.max_alloc = sd.alloc / 2;
    sd.window_parent_id = rnd() % 2 ? (sd.next_id - 1 - rnd() % 50) & kMask : UFC_NO_PARENT;
    for (int c = 0; c < 64; c++)
      sd.channel_parent_id[c] = rnd() % 4 == 0 ? (sd.next_id - 1 - rnd() % 70) & kMask : UFC_NO_PARENT;
    sd.take = rnd() % 5 ? 0xFFFFFFFFu : rnd() % (uint32_t)(n + 2);
    sd.reserve_items = rnd() % 3 ? 0 : rnd() % 5;
    sd.reserved = rnd();
    senders[s] = sd;
    for (uint64_t i = 0; i < n; i++) packets[first[s] + i] = random_packet(sd.flush_id, arena, true);
  }
  run_batch(first, packets.data(), senders.data());
}

void check_arithmetic() {
  const uint32_t lens[] = {0, 1, 1447, 1448, 1449, 2895, 2896, 2897, 1448u * 65536u - 1, 1448u * 65536u, 0xFFFFFFFFu};
  for (uint32_t len : lens) {
    const uint64_t frags = len == 0 ? 1 : ((uint64_t)len + 1447) / 1448;
    if (ufc_codec::emit_fragment_count(len) != frags) fail("fragment count", (long)len, 0, 0);
    if (ufc_codec::emit_alloc_size(len) != (len > 1448 ? frags * 1448 : len)) fail("alloc size", (long)len, 0, 0);
    checks++;
  }
  const uint64_t maxes[] = {0, 1, 1447, 1448, 1449, ~0ull - 1448, ~0ull - 100, ~0ull};
  for (uint64_t m : maxes) {
    const uint64_t r = ufc_codec::emit_max_alloc(m);
    if (r < m || (r % 1448 != 0 && r != ~0ull) || r - m >= 1448) fail("max alloc", (long)m, (long)r, 0);
    if (!ufc_codec::emit_alloc_fails(m, 0, 1, m) || ufc_codec::emit_alloc_fails(m, 0, 0, m)) fail("alloc fails", (long)m, 0, 0);
    checks++;
  }
  // the window room against the check it stands for, around every edge
  for (uint32_t ws : {0u, 1u, 2u, 4096u, 0xFFFFFu, 0x100000u, 0xFFFFFFFFu})
    for (uint32_t d : {0u, 1u, 2u, 4095u, 4096u, 4097u, 0xFFFFEu, 0xFFFFFu}) {
      const uint32_t base = 0xFFFF0u, next = (base + d) & kMask;
      const uint32_t room = ufc_codec::emit_window_room(base, next, ws);
      for (uint32_t r : {0u, 1u, 2u, 4094u, 4095u, 4096u, 0xFFFFFu, 0x100000u, 0x7FFFFFFEu}) {
        const bool limited = ((next + r - base) & kMask) >= ws;
        // (from the first limited rank on the walk has stopped: ranks past it need not agree)
        if (r <= room && limited != (r >= room)) fail("window room", (long)ws, (long)d, (long)r);
        checks++;
      }
    }
}

// ---- directed cases (tests/emit_expect.py lane_cases, the same numbers) ----

constexpr uint8_t kT = 0, kU = 1, kR = 3;  // SendMode: time-sensitive, unreliable, reliable

ufc_packet pkt(uint32_t len, uint8_t channel = 0, uint8_t mode = kU, uint32_t flush_id = 0) {
  ufc_packet p{};
  p.data_len = len;
  p.channel_id = channel;
  p.mode = mode;
  p.flush_id = flush_id;
  return p;
}
ufc_packet stale(uint32_t len = 7, uint8_t channel = 2) { return pkt(len, channel, kT, 1); }  // under flush_id 0
std::vector<ufc_packet> rep(const ufc_packet& p, size_t n) { return std::vector<ufc_packet>(n, p); }
std::vector<ufc_packet> operator+(std::vector<ufc_packet> a, const std::vector<ufc_packet>& b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

struct Directed {
  std::vector<ufc_packet> packets;
  std::vector<uint64_t> first{0};
  std::vector<ufc_sender> senders;
  uint32_t arena = 0;
  // A sender with nothing in flight, no parents and no limits; the caller sets what the case needs.
  ufc_sender& add(const std::vector<ufc_packet>& q) {
    for (ufc_packet p : q) {
      p.data_offset = arena;
      if (p.data_len <= kFrag * 65536u) arena += p.data_len;
      packets.push_back(p);
    }
    first.push_back(packets.size());
    ufc_sender sd{};
    sd.window_size = 4096;
    sd.max_alloc = (uint64_t)1 << 40;
    sd.window_parent_id = UFC_NO_PARENT;
    for (int c = 0; c < 64; c++) sd.channel_parent_id[c] = UFC_NO_PARENT;
    sd.take = 0xFFFFFFFFu;
    senders.push_back(sd);
    return senders.back();
  }
};

void want(const char* what, long tag, uint64_t got, uint64_t lit) {
  if (got != lit) fail(what, tag, (long)got, (long)lit);
  checks++;
}
// The leads of emitted packet i, from its first item.
uint32_t wlead(const Out& o, uint32_t i) { return o.items[o.pres[i].item_first].window_parent_lead; }
uint32_t clead(const Out& o, uint32_t i) { return o.items[o.pres[i].item_first].channel_parent_lead; }

void directed_cases() {
  Directed d;
  // the item search: a packet on slots 254, 255 | 256; reserved slots 510, 511 | 512; a range that starts at
  // slot 768 behind two empty senders; a range that starts at slot 1023
  const size_t seams = d.senders.size();
  d.add(rep(pkt(1), 254) + rep(pkt(3000), 1) + rep(pkt(1), 253));
  d.add(rep(pkt(1, 1, kR), 255)).reserve_items = 3;
  d.add({});
  d.add({});
  d.add(rep(pkt(3000, 2, kR), 1) + rep(pkt(1, 2), 252));
  d.add(rep(pkt(1, 4, kR), 2));  // starts on the last slot of a workgroup, 1023
  // stop_at[p] x {window, alloc, bad} x {all live, the even packets but p stale}
  const uint32_t ps[] = {63, 64, 65, 127, 128}, rank_lit[2][5] = {{63, 64, 65, 127, 128}, {31, 32, 32, 63, 64}},
                 frags_lit[2][5] = {{84, 86, 87, 170, 171}, {41, 43, 43, 84, 85}};  // alloc sizes before p, in fragments
  const uint32_t base = 0xFFFC0;
  const size_t stops = d.senders.size();
  for (int pi = 0; pi < 5; pi++)
    for (int form = 0; form < 2; form++) {
      const uint32_t p = ps[pi], rank = rank_lit[form][pi];
      std::vector<ufc_packet> q;
      for (uint32_t k = 0; k < p + 10; k++) {
        const bool live = form == 0 || k % 2 == 1 || k == p;
        q.push_back(live ? pkt(kFrag * (1 + (k % 3 == 0)), (uint8_t)(k % 5), k % 7 == 3 ? kR : kU) : stale(9, (uint8_t)(k % 5)));
      }
      for (int why = 0; why < 3; why++) {
        std::vector<ufc_packet> qq = q;
        if (why == 2) qq[p] = pkt(1, 70);
        ufc_sender& sd = d.add(qq);
        sd.base_id = base;
        sd.next_id = why == 0 ? (base + 256 - rank) & kMask : base;
        sd.window_size = why == 0 ? 256 : 4096;
        sd.alloc = 500 * kFrag;
        if (why == 1) sd.max_alloc = (500 + (uint64_t)frags_lit[form][pi]) * kFrag;
      }
    }
  // the window parent on lane 63, on lanes 62 and 63, on lane 0 of tile 2
  const size_t wp = d.senders.size();
  for (int v = 0; v < 3; v++) {
    std::vector<ufc_packet> q = rep(pkt(2, 1), 130);
    if (v == 0) q[63].mode = kR;
    if (v == 1) q[62].mode = q[63].mode = kR;
    if (v == 2) q[64].mode = kR;
    ufc_sender& sd = d.add(q);
    sd.next_id = 100, sd.window_parent_id = 90, sd.channel_parent_id[1] = 80;
  }
  // the channel parent through parent[5], two tiles on; lane 63 moves mask[63] into parent[63]
  const size_t cp = d.senders.size();
  {
    std::vector<ufc_packet> q = rep(pkt(2, 1), 130);
    q[63] = pkt(2, 5, kR), q[64] = pkt(2, 5), q[128] = pkt(2, 5);
    ufc_sender& sd = d.add(q);
    sd.next_id = 100, sd.channel_parent_id[5] = 70;
    q = rep(pkt(2, 1), 70);
    q[0] = pkt(2, 63, kR), q[63] = pkt(2, 63), q[64] = pkt(2, 63);
    d.add(q).next_id = 100;
  }
  // what only lane 63 carries: the fragment count, the alloc size, the dropped bytes
  const size_t only = d.senders.size();
  d.add(rep(stale(), 63) + rep(pkt(3000), 1) + rep(pkt(kFrag), 10)).next_id = 500;
  d.add(rep(stale(), 63) + rep(pkt(3000), 1) + rep(pkt(kFrag), 10)).max_alloc = 3 * kFrag;
  d.add(rep(stale(), 63) + rep(pkt(3000), 1) + rep(pkt(kFrag), 10)).max_alloc = 4 * kFrag;
  d.add(rep(pkt(5), 63) + rep(stale(777), 1) + rep(pkt(5), 10));
  d.add(rep(pkt(5, 3, kR), 63) + rep(stale(11), 1) + rep(pkt(1, 70), 1) + rep(pkt(5), 5));  // stale_63_then_stop_64
  // take at 63, 64, 65, 128 of 200
  const size_t takes = d.senders.size();
  const uint32_t take_lit[] = {63, 64, 65, 128};
  {
    std::vector<ufc_packet> q;
    const uint32_t lens[] = {0, 5, 300, 1448, 1449, 4000};
    for (int k = 0; k < 200; k++) q.push_back(pkt(lens[rnd() % 6], (uint8_t)(rnd() % 4), (uint8_t)(rnd() % 4), rnd() % 3 == 0));
    for (uint32_t t : take_lit) d.add(q).take = t;
  }
  d.add(rep(pkt(3000, 1, kR), 8)).reserve_items = 1;  // the finish's 8 lanes: one pass, and a second for the 9th
  d.add(rep(pkt(3000, 1, kR), 9)).reserve_items = 1;

  const std::vector<Out> o = run_batch(d.first, d.packets.data(), d.senders.data());
  std::vector<uint64_t> ff(o.size() + 1, 0);
  for (size_t s = 0; s < o.size(); s++) ff[s + 1] = ff[s] + o[s].items.size();

  want("seams: straddle", 0, ff[seams] + o[seams].pres[254].item_first, 254);
  want("seams: straddle", 1, o[seams].pres[254].item_count, 3);
  want("seams: straddle", 2, ff[seams] + o[seams].pres[255].item_first, 257);
  want("seams: reserved", 0, ff[seams + 1], 510);
  want("seams: reserved", 1, ff[seams + 1] + o[seams + 1].pres[0].item_first, 513);
  want("seams: empty", 0, ff[seams + 2], 768);
  want("seams: empty", 1, ff[seams + 3], 768);
  want("seams: range start", 0, ff[seams + 4], 768);
  want("seams: range start", 1, ff[seams + 4] + o[seams + 4].pres[1].item_first, 771);
  want("seams: range start", 2, clead(o[seams + 4], 5), 5);
  want("seams: last slot", 0, ff[seams + 5], 1023);
  want("seams: last slot", 1, ff[seams + 5] + o[seams + 5].pres[1].item_first, 1024);
  for (int pi = 0; pi < 5; pi++)
    for (int form = 0; form < 2; form++)
      for (int why = 0; why < 3; why++) {
        const Out& x = o[stops + (pi * 2 + form) * 3 + why];
        const uint32_t p = ps[pi], rank = rank_lit[form][pi];
        const uint32_t why_lit[] = {UFC_EMIT_WINDOW_LIMITED, UFC_EMIT_ALLOC_LIMITED, UFC_EMIT_BAD_PACKET};
        want("stop_at: consumed", p, x.res.packets_consumed, p);
        want("stop_at: stop", p, x.res.stop, why_lit[why]);
        want("stop_at: emitted", p, x.res.packets_emitted, rank);
        want("stop_at: dropped", p, x.res.packets_dropped, p - rank);
        want("stop_at: bytes dropped", p, x.res.bytes_dropped, 9 * (uint64_t)(p - rank));
        want("stop_at: alloc", p, x.state.alloc, (500 + (uint64_t)frags_lit[form][pi]) * kFrag);
        want("stop_at: next_id", p, x.state.next_id, why == 0 ? 192 : (base + rank) & kMask);
      }
  want("window parent at 63", 0, wlead(o[wp], 0), 10);
  want("window parent at 63", 62, wlead(o[wp], 62), 72);
  want("window parent at 63", 63, wlead(o[wp], 63), 73);
  want("window parent at 63", 64, wlead(o[wp], 64), 1);
  want("window parent at 63", 129, wlead(o[wp], 129), 66);
  want("window parent at 63", 1, clead(o[wp], 63), 83);
  want("window parent at 63", 2, o[wp].state.window_parent_id, 163);
  want("window parents at 62 and 63", 63, wlead(o[wp + 1], 63), 1);
  want("window parents at 62 and 63", 64, wlead(o[wp + 1], 64), 1);
  want("window parents at 62 and 63", 0, o[wp + 1].state.window_parent_id, 163);
  want("window parent at 64", 63, wlead(o[wp + 2], 63), 73);
  want("window parent at 64", 64, wlead(o[wp + 2], 64), 74);
  want("window parent at 64", 65, wlead(o[wp + 2], 65), 1);
  want("window parent at 64", 129, wlead(o[wp + 2], 129), 65);
  want("window parent at 64", 0, o[wp + 2].state.window_parent_id, 164);
  want("channel parent at 63", 63, clead(o[cp], 63), 93);
  want("channel parent at 63", 64, clead(o[cp], 64), 1);
  want("channel parent at 63", 128, clead(o[cp], 128), 65);
  want("channel parent at 63", 0, o[cp].state.channel_parent_id[5], 163);
  want("channel 63", 63, clead(o[cp + 1], 63), 63);
  want("channel 63", 64, clead(o[cp + 1], 64), 64);
  want("channel 63", 0, o[cp + 1].state.channel_parent_id[63], 100);
  want("only lane 63: fragments", 64, o[only].pres[64].item_first, 3);
  want("only lane 63: fragments", 0, o[only].res.item_count, 13);
  want("only lane 63: fragments", 1, o[only].res.packets_emitted, 11);
  want("only lane 63: fragments", 2, o[only].pres[64].sequence_id, 501);
  want("only lane 63: alloc", 0, o[only + 1].res.packets_consumed, 64);
  want("only lane 63: alloc", 1, o[only + 1].res.stop, UFC_EMIT_ALLOC_LIMITED);
  want("only lane 63: alloc", 2, o[only + 2].res.packets_consumed, 65);
  want("only lane 63: alloc", 3, o[only + 2].state.alloc, 4 * kFrag);
  want("only lane 63: dropped", 0, o[only + 3].res.packets_dropped, 1);
  want("only lane 63: dropped", 1, o[only + 3].res.bytes_dropped, 777);
  want("stale 63 then stop 64", 0, o[only + 4].res.packets_consumed, 64);
  want("stale 63 then stop 64", 1, o[only + 4].res.stop, UFC_EMIT_BAD_PACKET);
  want("stale 63 then stop 64", 2, o[only + 4].res.packets_dropped, 1);
  want("stale 63 then stop 64", 3, o[only + 4].pres[63].status, UFC_PACKET_DROPPED);
  want("stale 63 then stop 64", 4, o[only + 4].pres[64].status, 0);
  for (int k = 0; k < 4; k++) {
    const Out& x = o[takes + k];
    want("take_at", take_lit[k], x.res.packets_consumed, take_lit[k]);
    for (uint32_t i = take_lit[k]; i < 200; i++) want("take_at: zero past", i, x.pres[i].status | x.pres[i].item_count | x.pres[i].sequence_id, 0);
  }
  want("finish 8", 0, o[takes + 4].res.packets_consumed, 8);
  want("finish 9", 0, o[takes + 5].res.packets_consumed, 9);
}

}  // namespace

int main() {
  check_arithmetic();
  directed_cases();
  check_batch(1, 0);
  check_batch(3, 1);
  for (int r = 0; r < 40; r++) check_batch(1 + rnd() % 60, rnd() % 4 ? 1 + rnd() % 300 : 1 + rnd() % 8);
  std::printf("ok: %ld\n", checks);
  return 0;
}
