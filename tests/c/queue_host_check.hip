// The frame queue's core (uflow_amd/csrc/frame_codec_core.hpp: fq_step, the form the device runs, one wave per
// connection with a lane per log entry) as host code under AddressSanitizer and UBSan: the lanes of a phase run one
// after the other -- forwards, backwards and in a fresh seeded permutation per phase (lane_orders.hpp) -- and the
// shared block starts as garbage, fresh for every step or, in a fourth pass, one block carried from connection to
// connection as the kernel's grid-stride loop and the host entry carry it.  Checked against a scalar loop in this file that follows the
// reference entry by entry (push, acknowledge_group, ReorderBuffer::put and advance with a callback per id,
// push_ack and push_nack one at a time, find_expiration_cutoff frame by frame) and stops where the reference would
// panic: results, states, every log byte and ref_acked must be equal byte for byte.  Seeded traffic: connections
// chained over several calls (frames pushed at rising times or at times all over, a receiver that loses frames and
// acknowledges in groups, in order or not, twice, with a bad nonce, empty or far away; window bases that advance;
// forgets, feedbacks, resets), windows of 1 to 4096 with rings that wrap, ids through 2^32, random states that pass
// the check, and states that do not.  All buffers have their exact sizes.  In front of the seeded traffic, directed
// cases that put every ballot's deciding lane on lane 0, on lane 63 and across a tile seam (DESIGN.md 5.15;
// tests/test_queue_cpu.py has the same cases as scenarios), each with its expectation spelled out.
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

uint64_t rng_state = 0x51ED270Bu;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
uint32_t rnd32() { return (rnd() << 16) ^ rnd(); }

// ---- the scalar loop ----
struct Scalar {
  ufc_frame_queue q;
  ufc_sent_frame* log;
  uint8_t* refs;
  uint64_t refs_cap, rtt;
  ufc_frame_queue_result r;

  uint32_t len() const { return q.log_next_id - q.log_base_id; }
  bool in_log(uint32_t id) const { return id - q.log_base_id < len(); }
  ufc_sent_frame& at(uint32_t id) { return log[q.log_first + (id & (q.log_cap - 1))]; }
  void push_ack() {
    r.li_acks++;
    if (q.li_count && q.li_length[0] != 0xFFFFFFFFu) q.li_length[0]++;
  }
  void open(uint64_t end) {
    const uint32_t held = q.li_count < 9 ? q.li_count : 8;
    for (uint32_t k = held; k > 0; k--) {
      q.li_end_time_ms[k] = q.li_end_time_ms[k - 1];
      q.li_length[k] = q.li_length[k - 1];
    }
    q.li_end_time_ms[0] = end;
    q.li_length[0] = 1;
    q.li_count = held + 1;
  }
  void push_nack(uint64_t t) {
    r.li_nacks++;
    if (q.li_count == 0 || t >= q.li_end_time_ms[0]) open(t + rtt);
    else if (q.li_length[0] != 0xFFFFFFFFu) q.li_length[0]++;
  }
  void callback(uint32_t id, bool seen) {
    if (!in_log(id)) fail("the reference would panic: callback outside the log", id, q.log_base_id, q.log_next_id);
    if (seen) push_ack();
    else push_nack(at(id).send_time_ms);
  }
  void put(uint32_t id) {
    uint32_t* f = q.rb_frames;
    if (q.rb_count == 0) {
      if (id == q.rb_base_id) callback(id, true), q.rb_base_id++;
      else f[0] = id, q.rb_count = 1;
    } else if (q.rb_count == 1) {
      if (id == q.rb_base_id) {
        callback(id, true), q.rb_base_id++;
        if (f[0] == q.rb_base_id) callback(f[0], true), q.rb_base_id++, q.rb_count = 0;
      } else {
        if (id - q.rb_base_id < f[0] - q.rb_base_id) f[1] = f[0], f[0] = id;
        else f[1] = id;
        q.rb_count = 2;
      }
    } else if (q.rb_count == 2) {
      uint32_t m = id, dm = id - q.rb_base_id;
      if (f[1] - q.rb_base_id < dm) {
        dm = f[1] - q.rb_base_id;
        const uint32_t t = f[1];
        f[1] = m, m = t;
      }
      if (f[0] - q.rb_base_id < dm) {
        const uint32_t t = f[0];
        f[0] = m, m = t;
      }
      while (q.rb_base_id != m) callback(q.rb_base_id, false), q.rb_base_id++;
      callback(m, true), q.rb_base_id++;
      consume();
    }
  }
  void consume() {  // the tail both put and advance end with, for two held frames
    uint32_t* f = q.rb_frames;
    if (f[0] == q.rb_base_id) {
      callback(f[0], true), q.rb_base_id++, q.rb_count--;
      if (f[1] == q.rb_base_id) callback(f[1], true), q.rb_base_id++, q.rb_count--;
      else f[0] = f[1];
    }
  }
  void advance(uint32_t nb) {
    uint32_t* f = q.rb_frames;
    while (q.rb_count > 0 && f[0] - q.rb_base_id < nb - q.rb_base_id) {
      while (q.rb_base_id != f[0]) callback(q.rb_base_id, false), q.rb_base_id++;
      callback(f[0], true), q.rb_base_id++;
      if (q.rb_count == 2) f[0] = f[1];
      q.rb_count--;
    }
    while (q.rb_base_id != nb) callback(q.rb_base_id, false), q.rb_base_id++;
    if (q.rb_count == 1) {
      if (f[0] == q.rb_base_id) callback(f[0], true), q.rb_base_id++, q.rb_count = 0;
    } else if (q.rb_count == 2) {
      consume();
    }
  }
  void cull(uint32_t nb) {
    const uint32_t d = nb - q.rb_base_id;
    if (d >= 1 && d <= q.rb_max_span) advance(nb);
    if (nb - q.log_base_id > len()) fail("the reference would panic: drain past the end", nb, 0, 0);
    r.log_culled += nb - q.log_base_id;
    q.log_base_id = nb;
  }
  void group(const ufc_item& g) {
    r.groups++;
    uint32_t n = 0;
    for (int i = 31; i >= 0; i--)
      if (g.data_offset & (1u << i)) {
        n = (uint32_t)i + 1;
        break;
      }
    if (!n) {
      r.groups_dud++;
      return;
    }
    bool nonce = false;
    for (uint32_t i = 0; i < n; i++) {
      if (!in_log(g.id + i)) {
        r.groups_unknown++;
        return;
      }
      if ((g.data_offset >> i) & 1u) nonce ^= (at(g.id + i).flags & UFC_SENT_NONCE) != 0;
    }
    if (nonce != ((g.channel_id & 1) != 0)) {
      r.groups_bad_nonce++;
      return;
    }
    uint64_t last = 0, total = 0;
    bool limited = false;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t id = g.id + i;
      ufc_sent_frame& e = at(id);
      limited |= (e.flags & UFC_SENT_RATE_LIMITED) != 0;
      if (((g.data_offset >> i) & 1u) && !(e.flags & UFC_SENT_ACKED)) {
        e.flags |= UFC_SENT_ACKED;
        r.frames_acked++;
        for (uint64_t j = e.ref_first; j < (uint64_t)e.ref_first + e.ref_count && j < refs_cap; j++) refs[j] = 1;
        if (e.send_time_ms > last) last = e.send_time_ms;
        total += e.size;
        if (id - q.rb_base_id < q.rb_max_span) put(id);
      }
    }
    if (q.has_ack_data) {
      if (last > q.ack_last_send_time_ms) q.ack_last_send_time_ms = last;
      q.ack_total_size += total;
      q.ack_rate_limited |= limited ? 1 : 0;
    } else {
      q.has_ack_data = 1;
      q.ack_last_send_time_ms = last;
      q.ack_total_size = total;
      q.ack_rate_limited = limited ? 1 : 0;
    }
  }
};

void scalar_step(const FqArgs& a, uint64_t c, ufc_sent_frame* log, uint8_t* refs) {
  const ufc_frame_queue Q = a.queues[c];
  const ufc_frame_queue_step S = a.steps[c];
  const uint64_t ff0 = a.frame_first[c], ff1 = a.frame_first[c + 1], sf0 = a.sent_first[c], sf1 = a.sent_first[c + 1];
  bool ok = fq_state_ok(a, Q, S, ff0, ff1, sf0, sf1);
  for (uint64_t i = ff0; ok && i < ff1; i++)
    if (a.infos[i].ok && a.infos[i].kind == UFC_FRAME_ACK && (uint64_t)a.infos[i].item_first + a.infos[i].item_count > a.n_items)
      ok = false;
  if (!ok) {
    ufc_frame_queue_result r{};
    r.stop = UFC_FQ_BAD_STATE;
    a.results[c] = r;
    a.queues_out[c] = Q;
    return;
  }
  Scalar s{Q, log, refs, refs ? a.refs_cap : 0, (S.flags & UFC_FQ_HAS_RTT) ? S.rtt_ms : 100, ufc_frame_queue_result{}};
  ufc_frame_queue& q = s.q;
  if (S.flags & UFC_FQ_RESET_LOSS) {
    q.li_count = 1;
    q.li_length[0] = fq_reset_length(S.reset_loss_rate);
  }
  for (uint64_t j = sf0; j < sf1; j++) {
    if (q.log_next_id - q.window_base_id >= q.window_size) {
      s.r.pushes_refused++;
      continue;
    }
    const ufc_sent_frame in = a.sent[j];
    if (in.flags & UFC_SENT_MARK) q.rate_limited = 1;
    ufc_sent_frame e{};
    e.send_time_ms = in.send_time_ms, e.size = in.size, e.ref_first = in.ref_first, e.ref_count = in.ref_count;
    e.flags = (uint8_t)((in.flags & UFC_SENT_NONCE) | (q.rate_limited ? UFC_SENT_RATE_LIMITED : 0));
    s.at(q.log_next_id) = e;
    q.rate_limited = 0;
    q.log_next_id++;
    s.r.pushes_taken++;
  }
  if (S.flags & UFC_FQ_MARK_RATE_LIMITED) q.rate_limited = 1;
  for (uint64_t i = ff0; i < ff1; i++) {
    const ufc_frame_info f = a.infos[i];
    if (!f.ok || f.kind != UFC_FRAME_ACK) continue;
    s.r.ack_frames++;
    for (uint32_t g = 0; g < f.item_count; g++) s.group(a.items[(uint64_t)f.item_first + g]);
    const uint32_t d = f.f[0] - q.window_base_id;
    if (d != 0 && d <= q.log_next_id - q.window_base_id) {
      q.window_base_id = f.f[0];
      s.r.window_advanced += d;
      const uint32_t mb = q.window_base_id - q.tail_size, cut = mb - q.log_base_id;
      if (cut != 0 && cut <= s.len()) s.cull(mb);
    }
  }
  if (S.flags & UFC_FQ_FORGET) {
    uint32_t cut = q.log_base_id;
    for (uint32_t k = 0, n = s.len(); k < n && s.at(q.log_base_id + k).send_time_ms < S.thresh_ms; k++) cut++;
    if (cut != q.log_base_id) s.cull(cut);
  }
  if ((S.flags & UFC_FQ_FEEDBACK) && q.has_ack_data) {
    s.r.has_feedback = 1;
    s.r.rtt_ms = S.now_ms - q.ack_last_send_time_ms;
    s.r.receive_rate = q.has_last_feedback ? fq_receive_rate(q.ack_total_size, S.now_ms - q.last_feedback_ms) : 0;
    s.r.loss_rate = fq_loss_rate(q.li_length, q.li_count);
    s.r.rate_limited = q.ack_rate_limited;
    q.has_last_feedback = 1;
    q.last_feedback_ms = S.now_ms;
    q.has_ack_data = 0;
  }
  if (!q.has_ack_data) q.ack_rate_limited = 0, q.ack_last_send_time_ms = 0, q.ack_total_size = 0;
  for (uint32_t k = q.li_count; k < 9; k++) q.li_end_time_ms[k] = 0, q.li_length[k] = 0;
  const uint32_t ahead = q.log_next_id - q.window_base_id;
  s.r.window_room = ahead < q.window_size ? q.window_size - ahead : 0;
  a.results[c] = s.r;
  a.queues_out[c] = q;
}

// ---- one batch, both ways ----
struct Batch {
  std::vector<ufc_frame_info> infos;
  std::vector<ufc_item> items;
  std::vector<uint64_t> frame_first, sent_first;
  std::vector<ufc_sent_frame> sent;
  std::vector<ufc_frame_queue> queues;
  std::vector<ufc_frame_queue_step> steps;
  std::vector<ufc_sent_frame> log;
  std::vector<uint8_t> refs;
};

long total_nacks = 0, total_acked = 0, total_bad = 0, total_unknown = 0, total_badnonce = 0, total_feedback = 0, total_culled = 0;

// The forms the wave step runs in: three lane orders on a fresh garbage block, and forwards on a carried one.
enum Form { kForwards, kBackwards, kShuffled, kCarried, kForms };
FqWaveShared carried_block;  // (garbage once, in main)
ufc_frame_queue_result last_result;  // connection 0's, of the last batch

// Runs the batch in every wave form and scalar, compares, and moves the batch's state on (queues, log, refs).
void run_both(Batch& b, bool with_refs) {
  const size_t n = b.queues.size();
  std::vector<ufc_frame_queue_result> r1(n), r2(n);
  std::vector<ufc_frame_queue> q1(n), q2(n);
  std::memset((void*)r2.data(), 0xA5, n * sizeof r2[0]);
  std::memset((void*)q2.data(), 0xA5, n * sizeof q2[0]);
  std::vector<ufc_sent_frame> log1, log2 = b.log;
  std::vector<uint8_t> refs1, refs2 = b.refs;
  FqArgs a{b.infos.data(), b.infos.size(), b.items.data(), b.items.size(), b.frame_first.data(), b.sent.data(), b.sent.size(),
           b.sent_first.data(), b.queues.data(), b.steps.data(), n, log2.data(), log2.size(),
           with_refs ? refs2.data() : nullptr, refs2.size(), r2.data(), q2.data()};
  for (uint64_t c = 0; c < n; c++) scalar_step(a, c, log2.data(), with_refs ? refs2.data() : nullptr);
  for (int form = 0; form < kForms; form++) {
    std::memset((void*)r1.data(), 0xA5, n * sizeof r1[0]);
    std::memset((void*)q1.data(), 0xA5, n * sizeof q1[0]);
    log1 = b.log, refs1 = b.refs;
    a.log = log1.data(), a.ref_acked = with_refs ? refs1.data() : nullptr, a.results = r1.data(), a.queues_out = q1.data();
    for (uint64_t c = n; c-- > 0;) {  // (the connections in any order: last first here)
      FqWaveShared fresh;
      std::memset((void*)&fresh, 0xCD, sizeof fresh);
      FqWaveShared& sh = form == kCarried ? carried_block : fresh;
      if (form == kBackwards) fq_step(lane_orders::ReverseWave{}, sh, a, c);
      else if (form == kShuffled) fq_step(lane_orders::ShuffledWave{}, sh, a, c);
      else fq_step(SerialWave{}, sh, a, c);
    }
    if (std::memcmp((void*)r1.data(), (void*)r2.data(), n * sizeof r1[0])) {
      for (size_t c = 0; c < n; c++)
        if (std::memcmp((void*)&r1[c], (void*)&r2[c], sizeof r1[0])) fail("results", (long)c, form, r1[c].li_nacks * 100000L + r2[c].li_nacks);
    }
    if (std::memcmp((void*)q1.data(), (void*)q2.data(), n * sizeof q1[0])) fail("queues_out", form, 0, 0);
    if (!log1.empty() && std::memcmp((void*)log1.data(), (void*)log2.data(), log1.size() * sizeof log1[0])) fail("log", form, 0, 0);
    if (refs1 != refs2) fail("ref_acked", form, 0, 0);
    checks++;
  }
  for (size_t c = 0; c < n; c++) {
    total_nacks += r1[c].li_nacks, total_acked += r1[c].frames_acked, total_bad += r1[c].stop == UFC_FQ_BAD_STATE;
    total_unknown += r1[c].groups_unknown, total_badnonce += r1[c].groups_bad_nonce, total_feedback += r1[c].has_feedback;
    total_culled += r1[c].log_culled;
    checks++;
  }
  if (n) last_result = r1[0];
  b.queues = q1;
  b.log = log1;
  b.refs = refs1;
}

ufc_frame_queue new_queue(uint32_t size, uint32_t tail, uint32_t base, uint32_t cap, uint64_t first) {
  ufc_frame_queue q{};
  q.log_base_id = q.log_next_id = q.window_base_id = q.rb_base_id = base;
  q.window_size = size, q.tail_size = tail, q.rb_max_span = size + tail, q.log_cap = cap, q.log_first = first;
  return q;
}
ufc_item group_item(uint32_t id, uint32_t bits, uint32_t nonce) {
  ufc_item g{};
  g.id = id, g.data_offset = bits, g.channel_id = (uint8_t)nonce, g.form = 3;
  return g;
}

// A connection's peer: what was pushed (as the queue would take it) and what the receiver has not answered yet.
struct Peer {
  uint32_t size, next, window_base, rx_base;
  uint64_t now;
  std::vector<uint8_t> nonce;  // by id - first
  uint32_t first;
  uint32_t ref_next;
};

void add_traffic(Batch& b, Peer& p, bool acks, bool monotone, uint32_t max_sends) {
  if (acks) {
    std::vector<ufc_item> groups;
    uint32_t base = p.rx_base;
    bool open = false;
    ufc_item cur{};
    for (uint32_t id = p.rx_base; id != p.next; id++) {
      if (rnd() % 100 < 15) continue;  // lost
      const uint32_t nn = p.nonce[id - p.first];
      base = id + 1;
      if (open && id - cur.id < 32) {
        cur.data_offset |= 1u << (id - cur.id);
        cur.channel_id ^= (uint8_t)nn;
      } else {
        if (open) groups.push_back(cur);
        cur = group_item(id, 1, nn);
        open = true;
      }
    }
    if (open) groups.push_back(cur);
    p.rx_base = p.next;
    if (groups.size() > 1 && rnd() % 3 == 0) std::swap(groups[rnd() % (groups.size() - 1)], groups.back());
    const size_t ng = groups.size();
    for (size_t k = 0; k < ng; k++) {
      const uint32_t u = rnd() % 40;
      if (u == 0) groups.push_back(group_item(groups[k].id, groups[k].data_offset, groups[k].channel_id ^ 1));
      else if (u == 1) groups.push_back(group_item(groups[k].id, 0, 1));
      else if (u == 2) groups.push_back(group_item(rnd32(), rnd32() | 1, 0));
      else if (u == 3) groups.push_back(groups[k]);
      else if (u == 4) groups.push_back(group_item(p.next - 3, 0xFF, 0));  // runs past the log's end
    }
    const uint32_t frames = 1 + rnd() % 2;
    const uint32_t new_base = rnd() % 10 ? base : rnd32();
    for (uint32_t f = 0; f < frames; f++) {
      const size_t g0 = groups.size() * f / frames, g1 = groups.size() * (f + 1) / frames;
      ufc_frame_info info{};
      info.kind = UFC_FRAME_ACK, info.ok = 1, info.crc_ok = 1;
      info.f[0] = f + 1 == frames ? new_base : p.window_base;
      info.item_first = (uint32_t)b.items.size(), info.item_count = (uint32_t)(g1 - g0);
      b.infos.push_back(info);
      for (size_t g = g0; g < g1; g++) b.items.push_back(groups[g]);
      if (rnd() % 5 == 0) {  // a frame that is not an ack, or not ok: its item range is never looked at
        ufc_frame_info other{};
        other.kind = rnd() % 2 ? UFC_FRAME_DATA : UFC_FRAME_ACK;
        other.ok = other.kind == UFC_FRAME_DATA;
        other.item_first = 0xFFFFFFF0u, other.item_count = 100;
        b.infos.push_back(other);
      }
    }
    if (new_base - p.window_base <= p.next - p.window_base) p.window_base = new_base;
  }
  const uint32_t sends = rnd() % (max_sends + 1);
  for (uint32_t k = 0; k < sends; k++) {
    p.now += rnd() % 40;
    ufc_sent_frame s{};
    s.send_time_ms = monotone ? p.now : rnd() % (p.now + 200);
    s.size = 1 + rnd() % 1472;
    static const uint32_t counts[] = {0, 1, 1, 2, 3, 5, 16, 17, 70};
    s.ref_first = p.ref_next, s.ref_count = counts[rnd() % 9];
    p.ref_next += s.ref_count;
    s.flags = (uint8_t)((rnd() & 1) | (rnd() % 20 == 0 ? UFC_SENT_MARK : 0) | (rnd() % 7 == 0 ? UFC_SENT_ACKED : 0));
    b.sent.push_back(s);
    if (p.next - p.window_base < p.size) {
      p.nonce.push_back(s.flags & 1);
      p.next++;
    }
  }
}

void chained(uint32_t n, uint32_t size, uint32_t tail, uint32_t cap, uint32_t base, int rounds, bool monotone, uint32_t max_sends) {
  Batch b;
  std::vector<Peer> peers(n);
  for (uint32_t c = 0; c < n; c++) {
    b.queues.push_back(new_queue(size, tail, base, cap, (uint64_t)c * cap));
    peers[c] = Peer{size, base, base, base, 1000ull * c, {}, base, 0};
  }
  b.log.assign((size_t)n * cap, ufc_sent_frame{});
  std::memset((void*)b.log.data(), 0x5A, b.log.size() * sizeof b.log[0]);
  uint32_t ref_total = 0;
  for (int r = 0; r < rounds; r++) {
    b.infos.clear(), b.items.clear(), b.sent.clear();
    b.frame_first.assign(1, 0), b.sent_first.assign(1, 0);
    b.steps.assign(n, ufc_frame_queue_step{});
    for (uint32_t c = 0; c < n; c++) {
      peers[c].ref_next = ref_total;
      add_traffic(b, peers[c], r > 0, monotone, max_sends);
      ref_total = peers[c].ref_next;
      b.frame_first.push_back(b.infos.size());
      b.sent_first.push_back(b.sent.size());
      ufc_frame_queue_step& s = b.steps[c];
      s.flags = rnd() & 31u;
      if (rnd() % 8 || b.queues[c].li_count == 0) s.flags &= ~(uint32_t)UFC_FQ_RESET_LOSS;
      s.rtt_ms = rnd() % 300;
      s.thresh_ms = peers[c].now > rnd() % 3000 ? peers[c].now - rnd() % 3000 : 0;
      s.now_ms = peers[c].now + rnd() % 50;
      static const double ps[] = {0.5, 0.01, 1e-12, 3.0, 0.0, -1.0};
      s.reset_loss_rate = ps[rnd() % 6];
    }
    b.refs.resize(ref_total, 0);  // (exact size: a mark past the end is a sanitizer report)
    run_both(b, r % 4 != 3);
  }
}

// A random state that passes the check, with a random log, and a random call for it.
void random_state(int seed) {
  Batch b;
  const uint32_t cap = 1u << (rnd() % 8);
  const uint32_t size = rnd() % (cap + 1), tail = rnd() % (cap - size + 1);
  const uint32_t ahead = rnd() % (size + 1), len = rnd() % (ahead + tail + 1);
  ufc_frame_queue q{};
  q.log_next_id = rnd() % 2 ? rnd32() : 0xFFFFFFFFu - rnd() % 100;
  q.log_base_id = q.log_next_id - len, q.window_base_id = q.log_next_id - ahead;
  q.window_size = size, q.tail_size = tail, q.log_cap = cap, q.log_first = rnd() % 3;
  const uint32_t spans[] = {size + tail, size + tail + 1, 0x80000000u, cap};
  q.rb_max_span = spans[rnd() % 4];
  if (q.rb_max_span < size + tail) q.rb_max_span = size + tail;
  const uint32_t rb = rnd() % (len + 1);
  q.rb_base_id = q.log_base_id + rb;
  const uint32_t room = len - rb > 0 ? len - rb - 1 : 0;
  q.rb_count = rnd() % 3;
  if (q.rb_count > room) q.rb_count = room;
  if (q.rb_count == 1) q.rb_frames[0] = q.rb_base_id + 1 + rnd() % room;
  if (q.rb_count == 2) {
    const uint32_t d0 = 1 + rnd() % (room - 1);
    q.rb_frames[0] = q.rb_base_id + d0;
    q.rb_frames[1] = q.rb_base_id + d0 + 1 + rnd() % (room - d0);
  }
  q.rate_limited = rnd() & 1, q.has_ack_data = rnd() & 1, q.ack_rate_limited = rnd() & 1, q.has_last_feedback = rnd() & 1;
  q.ack_last_send_time_ms = rnd() % 5000, q.ack_total_size = rnd() % 2 ? rnd() : ~0ull - rnd() % 100, q.last_feedback_ms = rnd() % 5000;
  q.li_count = rnd() % 10;
  for (uint32_t k = 0; k < q.li_count; k++) {
    q.li_end_time_ms[k] = rnd() % 3000;
    static const uint32_t lens[] = {1, 2, 50, 0xFFFFFFFEu, 0xFFFFFFFFu, 0};
    q.li_length[k] = lens[rnd() % 6];
  }
  b.queues.push_back(q);
  b.log.resize(cap + 2);
  for (auto& e : b.log) {
    e = ufc_sent_frame{};
    e.send_time_ms = rnd() % 3000, e.size = rnd32(), e.ref_first = rnd() % 40, e.ref_count = rnd() % 30, e.flags = rnd() & 7;
  }
  b.refs.assign(48, 0);
  for (int call = 0; call < 3; call++) {
    const ufc_frame_queue& s = b.queues[0];
    b.infos.clear(), b.items.clear(), b.sent.clear();
    const uint32_t frames = rnd() % 4;
    for (uint32_t f = 0; f < frames; f++) {
      ufc_frame_info info{};
      info.kind = UFC_FRAME_ACK, info.ok = 1;
      info.f[0] = rnd() % 5 ? s.log_next_id - rnd() % (2 * size + 2) : s.window_base_id;
      info.item_first = (uint32_t)b.items.size();
      info.item_count = rnd() % 4;
      for (uint32_t g = 0; g < info.item_count; g++)
        b.items.push_back(group_item(s.log_base_id + rnd() % (s.log_next_id - s.log_base_id + 6) - 3, rnd32() >> (rnd() % 32), rnd() & 1));
      b.infos.push_back(info);
    }
    const uint32_t sends = rnd() % 6;
    for (uint32_t k = 0; k < sends; k++) {
      ufc_sent_frame e{};
      e.send_time_ms = rnd() % 3000, e.size = rnd32(), e.ref_first = rnd() % 40, e.ref_count = rnd() % 30;
      e.flags = (uint8_t)(rnd() & 15);
      b.sent.push_back(e);
    }
    b.frame_first = {0, b.infos.size()};
    b.sent_first = {0, b.sent.size()};
    ufc_frame_queue_step st{};
    st.flags = rnd() & 31u;
    if (s.li_count == 0) st.flags &= ~(uint32_t)UFC_FQ_RESET_LOSS;
    st.rtt_ms = rnd() % 2 ? rnd() % 300 : ~0ull - rnd() % 50;
    st.thresh_ms = rnd() % 3000, st.now_ms = rnd() % 3000;
    static const double ps[] = {0.0, 0.3, 1e-12, -1.0, 0.4};
    st.reset_loss_rate = ps[rnd() % 5];
    b.steps.assign(1, st);
    const long bad_before = total_bad;
    run_both(b, true);
    if (call == 0 && total_bad != bad_before) fail("a generated state did not pass the check", seed, 0, 0);
    if (total_bad != bad_before) break;  // (a held frame acked twice)
  }
}

// States that do not pass, beside one that does: nothing of theirs may be touched.
void bad_states() {
  for (int k = 0; k < 12; k++) {
    Batch b;
    for (int c = 0; c < 3; c++) b.queues.push_back(new_queue(4, 4, 100, 8, 8 * c));
    b.log.assign(24, ufc_sent_frame{});
    ufc_frame_queue& q = b.queues[1];
    b.frame_first = {0, 0, 1, 1};
    b.sent_first = {0, 1, 2, 3};
    b.steps.assign(3, ufc_frame_queue_step{});
    ufc_frame_info info{};
    info.kind = UFC_FRAME_ACK, info.ok = 1, info.f[0] = 100, info.item_count = 1;
    b.infos.push_back(info);
    b.items.push_back(group_item(100, 1, 0));
    b.sent.assign(3, ufc_sent_frame{});
    b.refs.assign(4, 0);
    switch (k) {
      case 0: q.log_cap = 12; break;
      case 1: q.tail_size = 5; break;
      case 2: q.log_first = 17; break;
      case 3: q.log_base_id = 90; break;
      case 4: q.rb_base_id = 101; break;
      case 5: q.rb_count = 3; break;
      case 6: q.rb_count = 1, q.rb_frames[0] = 100; break;
      case 7: q.li_count = 10; break;
      case 8: b.steps[1].flags = UFC_FQ_RESET_LOSS; break;
      case 9: b.frame_first = {0, 1, 0, 1}; break;
      case 10: b.infos[0].item_count = 2; break;
      case 11: q.rb_max_span = 7; break;
    }
    const long before = total_bad;
    run_both(b, true);
    if (total_bad - before < 1) fail("a bad state passed", k, 0, 0);
    if (b.queues[0].log_next_id != 101) fail("the good neighbour did not run", k, 0, 0);
  }
}

// The ballots of fq_step with their deciding lane on lane 0, on lane 63 and across a tile seam (the same cases, with
// the same numbers, are scenarios of tests/test_queue_cpu.py).  One connection, window 256 / tail 256 / a ring of 512
// at ids through 2^32; a first call pushes 200 frames, the second is the case.  The expectation is written out here
// and must also be what the scalar loop gives (run_both).
constexpr uint32_t kBase = 0xFFFFFFC0u;

Batch pushed(const std::vector<uint64_t>& times) {
  Batch b;
  b.queues.push_back(new_queue(256, 256, kBase, 512, 0));
  b.log.assign(512, ufc_sent_frame{});
  std::memset((void*)b.log.data(), 0x5A, b.log.size() * sizeof b.log[0]);
  for (size_t k = 0; k < times.size(); k++) {
    ufc_sent_frame s{};
    s.send_time_ms = times[k], s.size = 100 + (uint32_t)k, s.ref_first = (uint32_t)k, s.ref_count = 1, s.flags = (uint8_t)(k & 1);
    b.sent.push_back(s);
  }
  b.frame_first = {0, 0}, b.sent_first = {0, times.size()};
  b.steps.assign(1, ufc_frame_queue_step{});
  b.refs.assign(times.size(), 0);
  run_both(b, true);
  if (last_result.pushes_taken != times.size()) fail("directed: the pushes", last_result.pushes_taken, 0, 0);
  b.sent.clear(), b.sent_first = {0, 0};
  return b;
}

// 130 frames of which the ok ack frames sit at 63, 64 and 129, three ids each; the others are not acks or not ok
// and carry item ranges that must never be looked at.  bad_at: that ack frame's item range runs past the items.
void ack_frames_at_63_64_129(int bad_at) {
  std::vector<uint64_t> times;
  for (uint32_t k = 0; k < 200; k++) times.push_back(10 * k);
  Batch b = pushed(times);
  b.infos.clear();
  for (uint32_t i = 0; i < 130; i++) {
    ufc_frame_info f{};
    if (i == 63 || i == 64 || i == 129) {
      const uint32_t g = i == 63 ? 0 : i == 64 ? 1 : 2;
      f.kind = UFC_FRAME_ACK, f.ok = 1, f.crc_ok = 1;
      f.f[0] = i == 129 ? kBase + 9 : kBase;
      f.item_first = g, f.item_count = (int)i == bad_at ? 4 - g : 1;
      b.items.push_back(group_item(kBase + 3 * g, 7, g == 1 ? 0 : 1));  // (nonces k & 1: 0 1 0 | 1 0 1 | 0 1 0)
    } else {
      f.kind = i % 2 ? UFC_FRAME_DATA : UFC_FRAME_ACK;
      f.ok = f.kind == UFC_FRAME_DATA;
      f.item_first = 0xFFFFFFF0u, f.item_count = 100;
    }
    b.infos.push_back(f);
  }
  b.frame_first = {0, 130};
  run_both(b, true);
  const ufc_frame_queue_result& r = last_result;
  if (bad_at >= 0) {
    if (r.stop != UFC_FQ_BAD_STATE || b.queues[0].window_base_id != kBase) fail("directed: a bad item range", bad_at, r.stop, 0);
    return;
  }
  if (r.stop != UFC_FQ_DONE || r.ack_frames != 3 || r.groups != 3 || r.frames_acked != 9 || r.li_acks != 9 || r.window_advanced != 9)
    fail("directed: ack frames at 63, 64, 129", r.ack_frames, r.frames_acked, r.window_advanced);
  for (uint32_t k = 0; k < 200; k++)
    if (b.refs[k] != (k < 9)) fail("directed: ack frames at 63, 64, 129: ref_acked", k, 0, 0);
}

// A nack run of 140 ids over a log whose send times go up and down (a forget whose first kept entry is `lead` + 140,
// the first `lead` ids acknowledged in the same call so that the run starts there).  rtt 50: the run's entry 0 opens
// an interval (none is open), entries 1..62 fall under it, entry 63 (number 63 of the first nack tile) is the first
// at or after its end and opens the next, entry 64 (number 0 of the next tile) the next, entry 128 (number 0 of the
// third) the last.
void nack_run(uint32_t lead) {
  std::vector<uint64_t> times;
  for (uint32_t k = 0; k < lead; k++) times.push_back(500 + k);
  for (uint32_t k = 0; k < 140; k++) {
    const uint64_t wobble = (k * 7) % 50;
    times.push_back(k == 0 ? 1000 : k < 63 ? 1049 - wobble : k == 63 ? 1050 : k == 64 ? 1100 : k < 128 ? 1149 - wobble
                    : k == 128 ? 1150 : 1199 - wobble);
  }
  while (times.size() < 200) times.push_back(3000);
  Batch b = pushed(times);
  ufc_frame_info f{};
  f.kind = UFC_FRAME_ACK, f.ok = 1, f.f[0] = kBase;
  f.item_first = 0, f.item_count = lead;
  for (uint32_t k = 0; k < lead; k++) b.items.push_back(group_item(kBase + k, 1, k & 1));
  b.infos.assign(1, f);
  b.frame_first = {0, 1};
  b.steps[0].flags = UFC_FQ_FORGET | UFC_FQ_HAS_RTT;
  b.steps[0].rtt_ms = 50, b.steps[0].thresh_ms = 2000;
  run_both(b, true);
  const ufc_frame_queue_result& r = last_result;
  const ufc_frame_queue& q = b.queues[0];
  static const uint32_t want_len[4] = {12, 64, 1, 63};
  static const uint64_t want_end[4] = {1200, 1150, 1100, 1050};
  if (r.stop != UFC_FQ_DONE || r.li_nacks != 140 || r.li_acks != lead || r.log_culled != lead + 140 || q.li_count != 4)
    fail("directed: the nack run", r.li_nacks, r.log_culled, q.li_count);
  for (uint32_t k = 0; k < 4; k++)
    if (q.li_length[k] != want_len[k] || q.li_end_time_ms[k] != want_end[k]) fail("directed: the nack run's intervals", lead, k, q.li_length[k]);
}

// A forget whose first kept entry is log index `kept`: 63 (the last lane of the first expiry tile) or 64 (the first
// of the next).
void forget_kept_at(uint32_t kept) {
  std::vector<uint64_t> times;
  for (uint32_t k = 0; k < 200; k++) times.push_back(10 * k);
  Batch b = pushed(times);
  b.steps[0].flags = UFC_FQ_FORGET;
  b.steps[0].thresh_ms = 10 * kept;
  run_both(b, true);
  if (last_result.log_culled != kept || last_result.li_nacks != kept || b.queues[0].log_base_id != kBase + kept)
    fail("directed: forget", kept, last_result.log_culled, last_result.li_nacks);
}

void directed_cases() {
  ack_frames_at_63_64_129(-1);
  for (int bad_at : {63, 64, 129}) ack_frames_at_63_64_129(bad_at);
  for (uint32_t lead : {0u, 5u}) nack_run(lead);
  for (uint32_t kept : {63u, 64u, 128u}) forget_kept_at(kept);
}

}  // namespace

int main() {
  std::memset((void*)&carried_block, 0xCD, sizeof carried_block);
  directed_cases();
  bad_states();
  chained(3, 4, 4, 8, 0xFFFFFFF0u, 40, true, 6);        // the ring wraps every other call; ids through 2^32
  chained(2, 1, 1, 2, 5, 30, true, 3);
  chained(4, 64, 64, 128, 0xFFFFFF00u, 12, true, 90);
  chained(3, 256, 256, 512, 7, 8, false, 300);         // times all over: the nack tiles entry by entry
  chained(2, 4096, 4096, 8192, 0xFFFFF800u, 5, true, 4200);  // nack runs over many tiles
  chained(2, 100, 28, 128, 0, 10, true, 130);
  for (int seed = 0; seed < 3000; seed++) random_state(seed);
  if (total_nacks < 5000 || total_acked < 5000 || total_bad < 12 || total_unknown < 20 || total_badnonce < 20 ||
      total_feedback < 100 || total_culled < 5000)
    fail("too little of some kind of traffic", total_nacks, total_acked, total_culled);
  std::printf("ok: %ld\n", checks);
  return 0;
}
