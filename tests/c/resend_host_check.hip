// The resend core (uflow_amd/csrc/frame_codec_core.hpp: rs_begin, rs_place, rs_commit, the form the device runs, one
// wave per connection) as host code under AddressSanitizer and UBSan, over buffers of exactly the regions' sizes, the
// shared block starting as garbage.  Three checks:
//   - the heap (rs_heap_push / rs_heap_pop) against a plain scalar oracle: every pop returns an entry of the least
//     time and the multiset is kept; and the tie order std's BinaryHeap gives six equal entries that are popped and
//     pushed back one at a time (0, 2, 5, 1, 4, 3), or popped in a row (0, 2, 5, 4, 1, 3);
//   - pack_push / pack_finalize item by item against the closed form the packs use (pack_stop over F = H * starts +
//     bytes);
//   - chained ticks of one connection, begin -> a scalar emit -> place -> a scalar pack -> commit, with random acks
//     of sent refs, packet window acks (some beyond the span, some of next_id while fragments are pending), random
//     flush allocations, a small frame window, rings that wrap, ids through 2^20: run four times, the lanes of every
//     phase forwards (SerialWave), backwards (ReverseWave) and in a fresh seeded permutation per phase (ShuffledWave,
//     tests/c/lane_orders.hpp) on a shared block of fresh garbage, and forwards on one block carried from call to call
//     as the kernels' grid-stride loops and the host entries carry it; every state, result, arena byte and output
//     compared;
//   - directed ticks that put the wave form's cross-lane reads on lane 63 and on lane 0 of the next tile (DESIGN.md
//     5.15; tests/test_resend_cpu.py has the same cases on the model): the ack frames' ballot, the freed ids' window
//     and channel parents, the stopping packet of commit; in the same four forms, the expectation written out.
// Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <algorithm>
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

uint64_t rng_state = 0x7E5E2D11u;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

void check_heap() {
  {  // the tie order
    std::vector<ufc_resend_entry> d(6);
    uint32_t len = 0;
    for (uint32_t k = 0; k < 6; k++) rs_heap_push(d.data(), len, rs_entry(100, k, 0, 1));
    const uint32_t want[6] = {0, 2, 5, 1, 4, 3};
    for (uint32_t k = 0; k < 6; k++) {
      if (d[0].resend_time_ms != 100) fail("tie: top time", k, (long)d[0].resend_time_ms, 0);
      ufc_resend_entry x = rs_heap_pop(d.data(), len);
      if (x.sequence_id != want[k]) fail("tie: resend order", k, x.sequence_id, want[k]);
      x.resend_time_ms = 300;
      rs_heap_push(d.data(), len, x);
    }
    len = 0;
    for (uint32_t k = 0; k < 6; k++) rs_heap_push(d.data(), len, rs_entry(100, k, 0, 1));
    const uint32_t want2[6] = {0, 2, 5, 4, 1, 3};
    for (uint32_t k = 0; k < 6; k++)
      if (rs_heap_pop(d.data(), len).sequence_id != want2[k]) fail("tie: pop order", k, 0, 0);
    checks += 12;
  }
  for (uint32_t cap : {1u, 2u, 3u, 63u, 64u, 65u, 1000u}) {  // exact-size arrays, filled to the brim
    std::vector<ufc_resend_entry> d(cap);
    std::vector<uint64_t> oracle;
    uint32_t len = 0;
    for (uint32_t step = 0; step < 6 * cap + 20; step++) {
      const bool push = len == 0 || (len < cap && rnd() % 3 != 0);
      if (push) {
        const uint64_t t = rnd() % (cap < 8 ? 3 : cap / 2);
        rs_heap_push(d.data(), len, rs_entry(t, step, 0, 1));
        oracle.push_back(t);
      } else {
        const auto least = std::min_element(oracle.begin(), oracle.end());
        if (d[0].resend_time_ms != *least) fail("heap: peek is not the least", cap, step, 0);
        const ufc_resend_entry x = rs_heap_pop(d.data(), len);
        if (x.resend_time_ms != *least) fail("heap: pop is not the least", cap, step, 0);
        oracle.erase(least);
      }
      if (len != oracle.size()) fail("heap: length", cap, step, len);
      checks++;
    }
  }
}

void check_pack_rule() {
  for (uint32_t round = 0; round < 4000; round++) {
    ufc_flush fl{};
    fl.kind = UFC_FRAME_DATA;
    fl.window_room = rnd() % 5;
    fl.flush_alloc = (int64_t)(rnd() % 6000) - 5;
    PackRun run = pack_run_begin(fl);
    uint64_t bytes = 0, s = 0;
    uint32_t starts = 0, cnt = 0;
    for (uint32_t i = 0; i < 40; i++) {
      const uint64_t e = 6 + rnd() % (rnd() % 4 ? 300 : 1463);
      // the closed form: would the frame in progress take the item, and what has been spent
      const bool is_start = s == 0 || !pack_frame_takes(s, cnt, e, pack_max_count(false));
      const uint32_t want = pack_stop(fl, false, (uint64_t)kDataFrameOverhead * starts + bytes, is_start, starts);
      const uint32_t got = pack_push(run, fl, false, e);
      if (got != want) fail("pack rule", round, i, got * 10 + want);
      checks++;
      if (got != UFC_PACK_DONE) break;
      if (is_start) {
        starts++;
        s = kDataFrameOverhead + e;
        cnt = 1;
      } else {
        s += e;
        cnt++;
      }
      bytes += e;
    }
  }
}

// One connection's whole world, every buffer of its exact size.
struct World {
  ufc_resend st;
  ufc_sender sd;
  ufc_frame_queue q;
  std::vector<ufc_resend_entry> heap;
  std::vector<ufc_sent_packet> pkts;
  std::vector<uint8_t> frag, ref_acked;
  std::vector<ufc_tx_ref> tx;
  std::vector<ufc_item> stage;
  std::vector<ufc_sent_frame> log;
  uint32_t extra;
  std::vector<uint32_t> kept;  // ref_first of the frames of the last ticks, oldest first

  World(uint32_t window, uint32_t base, uint32_t heap_cap, uint32_t stage_cap) : extra(0) {
    std::memset(&st, 0, sizeof st);
    std::memset(&sd, 0, sizeof sd);
    std::memset(&q, 0, sizeof q);
    sd.base_id = sd.next_id = base;
    sd.window_size = window;
    sd.max_alloc = 20000;
    sd.window_parent_id = UFC_NO_PARENT;
    for (auto& c : sd.channel_parent_id) c = UFC_NO_PARENT;
    st.heap_cap = heap_cap;
    st.pkt_cap = window;
    st.frag_cap = window <= 16 ? 32 : 256;  // >= ceil(20000 / 1448) + window = 14 + window
    st.tx_cap = 512;   // >= (2 + 1 + 1) * 127
    st.stage_cap = stage_cap;
    q.window_size = 2;
    q.tail_size = 1;
    q.log_cap = 4;
    heap.resize(st.heap_cap);
    pkts.resize(st.pkt_cap);
    frag.assign(st.frag_cap, 0x5A);
    tx.resize(st.tx_cap);
    ref_acked.assign(st.tx_cap, 0);
    stage.resize(st.stage_cap);
    log.resize(q.log_cap);
  }
};

struct Tick {
  std::vector<ufc_frame_info> acks;
  std::vector<ufc_packet> packets;
  std::vector<uint32_t> ack_refs;  // tx positions the peer acknowledges
  int64_t alloc;
  uint32_t room, flags;
  uint64_t now, rtt;
};

using lane_orders::ReverseWave;
using lane_orders::ShuffledWave;

RsWaveShared carried_block;  // (garbage once, in main)

// What a tick's calls said, for the directed cases.
struct Said {
  ufc_resend_result begin;
  ufc_resend_commit_result commit;
  uint32_t frames;
};

template <class Wv>
Said run_tick(World& w, const Tick& t, std::vector<uint8_t>& trace, bool carried = false) {
  const auto put = [&](const void* p, size_t n) { trace.insert(trace.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
  RsWaveShared fresh;
  std::memset(&fresh, 0xA5, sizeof fresh);
  RsWaveShared& sh = carried ? carried_block : fresh;
  for (uint32_t r : t.ack_refs) w.ref_acked[r] = 1;
  // the frame queue's part that begin reads: the log's base frame
  w.q.log_base_id = 0;
  w.q.log_next_id = w.kept.empty() ? 0 : 1;
  if (!w.kept.empty()) w.log[0].ref_first = w.kept.front();
  const uint64_t frame_first[2] = {0, t.acks.size()};
  ufc_rate_result rate{};
  rate.now_ms = t.now;
  rate.rtt_ms = t.rtt;
  ufc_flush fl{};
  fl.flush_alloc = t.alloc;
  fl.kind = UFC_FRAME_DATA;
  fl.window_room = t.room;
  fl.id0 = 77;
  ufc_resend_result br;
  w.sd.take = 0xFFFFFFFFu;
  w.sd.reserve_items = 0;
  const RsBeginArgs ba{t.acks.data(), t.acks.size(), frame_first, &w.q, w.log.data(), w.log.size(), &rate, &t.flags, &fl, &w.st,
                       &w.sd, 1, w.heap.data(), w.heap.size(), w.pkts.data(), w.pkts.size(), w.frag.data(), w.frag.size(),
                       w.tx.data(), w.tx.size(), w.ref_acked.data(), w.ref_acked.size(), w.stage.data(), w.stage.size(), &br,
                       &w.st, &w.sd};
  rs_begin(Wv{}, sh, ba, 0);
  put(&br, sizeof br);
  // a scalar emit: the packets the window and the allocation take, fragment by fragment
  std::vector<ufc_item> items(w.sd.reserve_items);
  std::vector<ufc_packet_result> pres(t.packets.size());
  ufc_sender_result sres{};
  ufc_sender after = w.sd;
  for (size_t i = 0; i < t.packets.size() && i < w.sd.take; i++) {
    const ufc_packet& p = t.packets[i];
    if (emit_window_room(after.base_id, after.next_id, after.window_size) == 0) break;
    if (emit_alloc_fails(after.alloc, 0, emit_alloc_size(p.data_len), emit_max_alloc(after.max_alloc))) break;
    const uint32_t seq = after.next_id, last = emit_fragment_count(p.data_len) - 1;
    ufc_packet_result& r = pres[i];
    std::memset(&r, 0, sizeof r);
    r.sequence_id = seq;
    r.item_first = (uint32_t)items.size();
    r.item_count = last + 1;
    r.status = UFC_PACKET_EMITTED;
    r.resend = p.mode >= UFC_SEND_PERSISTENT;
    for (uint32_t f = 0; f <= last; f++)
      items.push_back(emit_item(p, seq, emit_lead(seq, after.window_parent_id), emit_lead(seq, after.channel_parent_id[p.channel_id]), f, last));
    after.next_id = packet_id_add(after.next_id, 1);
    after.alloc += emit_alloc_size(p.data_len);
    if (p.mode == UFC_SEND_RELIABLE) after.window_parent_id = after.channel_parent_id[p.channel_id] = seq;
    sres.packets_consumed++;
    sres.packets_emitted++;
  }
  sres.item_count = (uint32_t)items.size();
  const uint64_t flush_first[2] = {0, items.size()}, packet_first[2] = {0, t.packets.size()};
  const RsPlaceArgs pa{&w.st, &br, 1, w.stage.data(), w.stage.size(), flush_first, items.data(), items.size()};
  rs_place(Wv{}, pa, 0);
  // a scalar pack
  std::vector<ufc_frame_info> infos;
  std::vector<uint64_t> out_offsets(1, 0);
  ufc_flush_result fres{};
  PackRun run = pack_run_begin(fl);
  uint32_t first = 0;
  const auto frame = [&](uint32_t upto, uint64_t size) {
    ufc_frame_info info{};
    info.kind = UFC_FRAME_DATA;
    info.ok = 1;
    info.f[0] = fl.id0 + (uint32_t)infos.size();
    info.item_first = first;
    info.item_count = upto - first;
    infos.push_back(info);
    out_offsets.push_back(out_offsets.back() + size);
  };
  uint32_t i = 0;
  for (; i < items.size(); i++) {
    const uint64_t s0 = run.s;
    const uint32_t frames0 = run.frames;
    const uint32_t st = pack_push(run, fl, false, datagram_encoded_size(items[i]));
    if (run.frames != frames0) frame(i, s0);  // the push closed the frame in progress
    if (st != UFC_PACK_DONE) {
      fres.stop = st;
      break;
    }
    if (run.cnt == 1) first = i;
  }
  if (fres.stop == UFC_PACK_DONE && run.s) {
    const uint64_t s0 = run.s;
    pack_finalize(run);
    frame(i, s0);
  }
  fres.frame_count = (uint32_t)infos.size();
  fres.items_packed = i;
  fres.alloc_left = run.alloc;
  const uint64_t frames_used = infos.size();
  std::vector<ufc_sent_frame> sent(infos.size());
  uint64_t sent_first[2];
  ufc_resend_commit_result cr;
  ufc_sender retake;
  const ufc_sender pre = w.sd;
  const RsCommitArgs ca{&fres, infos.data(), infos.size(), out_offsets.data(), &frames_used, items.data(), items.size(),
                        flush_first, t.packets.data(), t.packets.size(), packet_first, pres.data(), &sres, &br, &rate, &w.st,
                        &pre, 1, w.heap.data(), w.heap.size(), w.pkts.data(), w.pkts.size(), w.frag.data(), w.frag.size(),
                        w.tx.data(), w.tx.size(), sent.data(), sent.size(), sent_first, &w.extra, &cr, &w.st, &retake};
  rs_commit(Wv{}, sh, ca, 0);
  put(&cr, sizeof cr);
  put(sent_first, sizeof sent_first);
  if (!sent.empty()) put(sent.data(), sent.size() * sizeof sent[0]);
  if (!items.empty()) put(items.data(), items.size() * sizeof items[0]);
  if (cr.stop == UFC_RS_BAD_STATE || br.stop == UFC_RS_BAD_STATE) fail("bad state on generated traffic", br.stop, cr.stop, 0);
  if (cr.take > t.packets.size()) fail("take beyond the queue", cr.take, (long)t.packets.size(), 0);
  // the second emit: the state after the first `take` packets
  ufc_sender second = pre;
  for (uint32_t k = 0; k < cr.take; k++) {
    const ufc_packet& p = t.packets[k];
    const uint32_t seq = second.next_id;
    second.next_id = packet_id_add(second.next_id, 1);
    second.alloc += emit_alloc_size(p.data_len);
    if (p.mode == UFC_SEND_RELIABLE) second.window_parent_id = second.channel_parent_id[p.channel_id] = seq;
  }
  w.sd = second;
  for (const ufc_sent_frame& f : sent) w.kept.push_back(f.ref_first);
  while (w.kept.size() > 3) w.kept.erase(w.kept.begin());
  put(&w.st, sizeof w.st);
  put(&w.sd, sizeof w.sd);
  put(w.heap.data(), w.st.heap_len * sizeof(ufc_resend_entry));
  put(w.pkts.data(), w.pkts.size() * sizeof(ufc_sent_packet));
  put(w.frag.data(), w.frag.size());
  put(w.ref_acked.data(), w.ref_acked.size());
  put(w.tx.data(), w.tx.size() * sizeof(ufc_tx_ref));
  put(&w.extra, sizeof w.extra);
  return Said{br, cr, (uint32_t)infos.size()};
}

// One tick in the four forms, on four worlds in the same state; every form's trace must be the first's.
struct Worlds {
  World a, b, c, d;
  Worlds(uint32_t window, uint32_t base, uint32_t heap_cap, uint32_t stage_cap)
      : a(window, base, heap_cap, stage_cap), b(window, base, heap_cap, stage_cap), c(window, base, heap_cap, stage_cap),
        d(window, base, heap_cap, stage_cap) {}
  Said tick(const Tick& t, long where, long when, std::vector<uint8_t>& ta) {
    std::vector<uint8_t> tb, tc, td;
    ta.clear();
    const Said said = run_tick<SerialWave>(a, t, ta);
    run_tick<ReverseWave>(b, t, tb);
    run_tick<ShuffledWave>(c, t, tc);
    run_tick<SerialWave>(d, t, td, true);
    if (ta != tb) fail("lane order changes the result: backwards", where, when, (long)ta.size());
    if (ta != tc) fail("lane order changes the result: shuffled", where, when, (long)ta.size());
    if (ta != td) fail("a carried shared block changes the result", where, when, (long)ta.size());
    checks += 3;
    return said;
  }
};

void check_ticks() {
  long stops[8] = {0}, commit_stops[8] = {0};
  for (uint32_t conn = 0; conn < 12; conn++) {
    const uint32_t window = conn % 2 ? 8 : 4, base = conn % 3 ? 0xFFFF8u + conn : conn * 1000;
    const uint32_t heap_cap = conn % 4 == 3 ? 5 : 24, stage_cap = conn % 4 == 2 ? 4 : 40;  // (small ones fill)
    Worlds ws(window, base, heap_cap, stage_cap);
    World& a = ws.a;
    uint64_t now = 1000;
    for (uint32_t tick = 0; tick < 120; tick++) {
      Tick t;
      t.now = now;
      t.rtt = conn == 5 ? 0 : 30;
      const uint32_t ak = rnd() % 4;
      t.alloc = ak == 0 ? (int64_t)(rnd() % 300) - 3 : ak == 1 ? (int64_t)(rnd() % 3000) : (int64_t)1 << 30;
      t.room = rnd() % 3;
      t.flags = rnd() % 16 == 0 ? UFC_RS_NO_DATA_FLUSH : 0;
      const uint32_t np = rnd() % 3;
      for (uint32_t k = 0; k < np; k++) {
        ufc_packet p{};
        p.data_offset = rnd();
        p.data_len = rnd() % 3 ? rnd() % 300 : 1000 + rnd() % 4000;
        p.channel_id = (uint8_t)(rnd() % 3);
        p.mode = (uint8_t)(1 + rnd() % 3);
        t.packets.push_back(p);
      }
      // acks: some of the live refs, and a packet window base somewhere in [base, next], now and then beyond
      const uint32_t live = a.st.tx_head - a.st.tx_tail;
      for (uint32_t j = 0; j < live; j++)
        if (rnd() % 3 == 0) t.ack_refs.push_back((a.st.tx_tail + j) & (a.st.tx_cap - 1));
      const uint32_t span = packet_id_sub(a.sd.next_id, a.sd.base_id);
      for (uint32_t k = rnd() % 3; k > 0; k--) {
        ufc_frame_info f{};
        f.kind = UFC_FRAME_ACK;
        f.ok = 1;
        const uint32_t r = tick < 100 ? 1 + rnd() % 19 : rnd() % 4;  // (a connection that hangs stays hung: late)
        f.f[1] = r == 0 ? a.sd.next_id : r == 1 ? packet_id_add(a.sd.next_id, 3) : r == 2 ? 0x7FFFFFFFu
                        : packet_id_add(a.sd.base_id, span ? rnd() % (span + 1) / 2 : 0);
        t.acks.push_back(f);
      }
      std::vector<uint8_t> ta;
      ws.tick(t, conn, tick, ta);
      ufc_resend_result br;
      std::memcpy(&br, ta.data(), sizeof br);
      ufc_resend_commit_result cr;
      std::memcpy(&cr, ta.data() + sizeof br, sizeof cr);
      stops[br.stop]++;
      commit_stops[cr.stop]++;
      checks++;
      now += 20;
    }
  }
  for (uint32_t s : {UFC_RS_DONE, UFC_RS_SIZE_LIMITED, UFC_RS_WINDOW_LIMITED, UFC_RS_REF_HANG, UFC_RS_STAGE_FULL})
    if (stops[s] == 0) fail("the traffic never reached begin stop", s, 0, 0);
  if (commit_stops[UFC_RS_HEAP_FULL] == 0) fail("the traffic never filled the heap", 0, 0, 0);
}

// ---- the wave form's cross-lane reads on lane 63 and on lane 0 of the next tile ----
Tick quiet_tick(uint64_t now, uint32_t room) {
  Tick t;
  t.alloc = (int64_t)1 << 30;
  t.room = room;
  t.flags = 0;
  t.now = now;
  t.rtt = 30;
  return t;
}
ufc_packet a_packet(uint32_t len, uint32_t channel, uint32_t mode) {
  ufc_packet p{};
  p.data_offset = 7 * len;
  p.data_len = len;
  p.channel_id = (uint8_t)channel;
  p.mode = (uint8_t)mode;
  return p;
}
ufc_frame_info an_ack(uint32_t packet_window_base) {
  ufc_frame_info f{};
  f.kind = UFC_FRAME_ACK;
  f.ok = 1;
  f.f[1] = packet_window_base;
  return f;
}

void check_directed() {
  const uint32_t base = 0xFFFF0;  // (the ids pass 2^20 inside every case)
  const auto id = [&](uint32_t k) { return packet_id_add(base, k); };
  std::vector<uint8_t> trace;
  // begin, the freed ids' parents: the window's parent and channel 63's are the id at lane 63 of a tile of freed ids
  // (64 freed), then at lane 0 of the next (65 freed); that id's packet is the only long one (the sums' lane too)
  for (uint32_t at : {63u, 64u}) {
    Worlds ws(128, base, 256, 300);
    Tick t = quiet_tick(1000, 3);
    uint64_t bytes = 0;
    for (uint32_t k = 0; k < 70; k++) {
      t.packets.push_back(k == at ? a_packet(1000, 63, UFC_SEND_RELIABLE) : a_packet(1 + k % 5, k % 3, UFC_SEND_UNRELIABLE));
      if (k <= at) bytes += t.packets.back().data_len;
    }
    Said said = ws.tick(t, 100 + at, 0, trace);
    if (said.commit.take != 70 || ws.a.sd.window_parent_id != id(at) || ws.a.sd.channel_parent_id[63] != id(at))
      fail("directed: the parents' packet", at, said.commit.take, ws.a.sd.window_parent_id);
    t = quiet_tick(1020, 3);
    t.acks.push_back(an_ack(id(at + 1)));
    said = ws.tick(t, 100 + at, 1, trace);
    if (said.begin.packets_freed != at + 1 || said.begin.bytes_freed != bytes || ws.a.sd.base_id != id(at + 1) ||
        ws.a.sd.window_parent_id != UFC_NO_PARENT || ws.a.sd.channel_parent_id[63] != UFC_NO_PARENT)
      fail("directed: parents freed", at, said.begin.packets_freed, ws.a.sd.window_parent_id);
  }
  {  // begin, the ack frames' ballot: the ack that frees sits at frame 63; the one behind it is stale only if it ran.
     // Then at frame 64 (lane 0 of the second tile), and a last one at 129 (lane 1 of the third).
    Worlds ws(128, base, 256, 300);
    Tick t = quiet_tick(1000, 3);
    for (uint32_t k = 0; k < 20; k++) t.packets.push_back(a_packet(2 + k, k % 3, UFC_SEND_UNRELIABLE));
    ws.tick(t, 200, 0, trace);
    t = quiet_tick(1020, 3);
    for (uint32_t i = 0; i < 70; i++) t.acks.push_back(an_ack(i == 63 ? id(5) : i == 64 ? id(3) : base));
    t.acks[10].kind = UFC_FRAME_DATA;  // (not an ack: whatever it names)
    t.acks[10].f[1] = id(9);
    Said said = ws.tick(t, 200, 1, trace);
    if (said.begin.packets_freed != 5 || said.begin.acks_ignored != 6 || ws.a.sd.base_id != id(5))
      fail("directed: the ack at frame 63", said.begin.packets_freed, said.begin.acks_ignored, ws.a.sd.base_id);
    t = quiet_tick(1040, 3);
    for (uint32_t i = 0; i < 130; i++) t.acks.push_back(an_ack(i == 64 ? id(9) : i == 65 ? id(7) : i == 129 ? id(11) : i < 64 ? id(5) : base));
    said = ws.tick(t, 200, 2, trace);
    if (said.begin.packets_freed != 6 || said.begin.acks_ignored != 64 || ws.a.sd.base_id != id(11))
      fail("directed: the acks at frames 64 and 129", said.begin.packets_freed, said.begin.acks_ignored, ws.a.sd.base_id);
  }
  // commit, the stopping packet: one frame's room; the packets in front of `at` fit it, packet `at` does not, and is
  // the first whose items lie past the packed ones: lane 63 of the first tile of packets, then lane 0 of the second
  for (uint32_t at : {63u, 64u}) {
    Worlds ws(128, base, 256, 300);
    Tick t = quiet_tick(1000, 1);
    for (uint32_t k = 0; k < 70; k++) t.packets.push_back(a_packet(k == at ? 1400 : 1, k % 3, UFC_SEND_PERSISTENT));
    Said said = ws.tick(t, 300 + at, 0, trace);
    const ufc_resend_commit_result& cr = said.commit;
    if (said.frames != 1 || cr.take != at + 1 || cr.packets_entered != at + 1 || cr.pending_count != 1 || cr.heap_pushed != at ||
        ws.a.st.pending_seq != id(at) || ws.a.st.window_bytes != at + 1400 || ws.a.sd.next_id != id(at + 1))
      fail("directed: the stopping packet", at, cr.take, cr.packets_entered);
    t.packets.erase(t.packets.begin(), t.packets.begin() + cr.take);
    t.now = 1010, t.room = 3;
    said = ws.tick(t, 300 + at, 1, trace);
    if (said.commit.pending_packed != 1 || said.commit.take != 69 - at || said.commit.pending_count != 0 || ws.a.st.heap_len != 70)
      fail("directed: behind the stopping packet", at, said.commit.take, ws.a.st.heap_len);
  }
}

}  // namespace

int main() {
  std::memset(&carried_block, 0xA5, sizeof carried_block);
  check_heap();
  check_pack_rule();
  check_ticks();
  check_directed();
  std::printf("ok: %ld checks\n", checks);
  return 0;
}
