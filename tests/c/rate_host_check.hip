// rate_host_check.hip -- the send rate control's core (frame_codec_core.hpp: rate_step, rate_begin) as host code
// under AddressSanitizer and UBSan: the shapes of tests/golden/send_rate_cases.json with their hand-traced numbers,
// the named cases of tests/rate_expect.py's set_cases() (sets longer than the kRateHeld entries a step holds in
// registers) against literals over a heap arena of exactly the rooms' bytes, with the same numbers as there,
// then a random batch over buffers of exactly the sizes the states name (rooms of up to 24 entries), so that an entry written outside a
// connection's room, a gather past its array or a float cast with undefined behaviour stops the run.
// A stand-alone program; tests/test_rate_cpu.py builds and runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../uflow_amd/csrc/frame_codec_core.hpp"

using namespace ufc_codec;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                     \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static uint64_t rnd_below(uint64_t n) { return rnd() % n; }
static double rnd_unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static ufc_rate_state new_state(uint32_t max_send_rate, uint32_t cap) {
  ufc_rate_state s;
  std::memset(&s, 0, sizeof s);
  s.send_rate = UFC_MAX_FRAME_SIZE;
  s.max_send_rate = max_send_rate;
  s.recv_cap = cap;
  return s;
}
static ufc_frame_queue_result feedback(uint64_t rtt_ms, uint32_t rate, double loss, bool limited) {
  ufc_frame_queue_result f;
  std::memset(&f, 0, sizeof f);
  f.has_feedback = 1;
  f.rtt_ms = rtt_ms;
  f.receive_rate = rate;
  f.loss_rate = loss;
  f.rate_limited = limited;
  return f;
}
static ufc_rate_tick tick(uint64_t now, double delta, int64_t adjust, uint32_t flags) {
  ufc_rate_tick t;
  std::memset(&t, 0, sizeof t);
  t.now_ms = now;
  t.delta_time_s = delta;
  t.alloc_adjust = adjust;
  t.flags = flags;
  return t;
}

// One connection over a heap arena of exactly `cap` entries.
struct One {
  std::vector<ufc_recv_rate_entry> arena;
  ufc_rate_state s;
  ufc_rate_result r;
  One(uint32_t max_send_rate, uint32_t cap) : arena(cap), s(new_state(max_send_rate, cap)) {
    std::memset(arena.data(), 0, cap * sizeof(ufc_recv_rate_entry));
  }
  void step(const ufc_rate_tick& t, const ufc_frame_queue_result& f) {
    RateArgs a{};
    a.n = 1;
    a.entries = arena.data();
    a.n_entries = arena.size();
    rate_step(a, 0, s, t, f, r);
  }
};


// ---- rate_expect.set_cases(): sets past the held entries ----
struct Ent {
  uint64_t t;
  uint32_t v;
  bool initial;
};
static bool operator==(const ufc_recv_rate_entry& e, const Ent& w) {
  return e.timestamp_ms == w.t && e.value == w.v && e.is_initial == (w.initial ? 1 : 0) && e.reserved[0] == 0 &&
         e.reserved[1] == 0 && e.reserved[2] == 0;
}
struct SetCase {
  const char* name;
  uint32_t cap;
  std::vector<Ent> in;
  uint32_t stop;
  std::vector<Ent> want;  // the set afterwards (DONE)
  uint32_t send_rate;
  bool limited = true, feedback = true, arena_last = false;
  double prev_loss = 1e-9;
  uint64_t now = 10000;
};
static const uint64_t kNow = 10000, kF = 9950, kX = 9000;  // with rtt_ms 50: ages 50 (kept) and 1000 (dropped)
static const uint32_t kFed = 50000;
static uint32_t val(uint32_t k) { return 100000 + 1000 * k; }
static std::vector<Ent> set_of(const std::vector<uint64_t>& stamps, const std::vector<uint32_t>& values = {}) {
  std::vector<Ent> e;
  for (size_t k = 0; k < stamps.size(); k++) e.push_back({stamps[k], values.empty() ? val((uint32_t)k) : values[k], false});
  return e;
}
static std::vector<Ent> kept(const std::vector<Ent>& e, const std::vector<int>& idx, uint64_t now = kNow) {
  std::vector<Ent> w;
  for (int k : idx) w.push_back(e[k]);
  w.push_back({now, kFed, false});
  return w;
}
static std::vector<uint64_t> stamps(std::initializer_list<std::pair<int, uint64_t>> runs) {
  std::vector<uint64_t> s;
  for (auto& r : runs) s.insert(s.end(), r.first, r.second);
  return s;
}
static std::vector<int> upto(int n) {
  std::vector<int> v(n);
  for (int k = 0; k < n; k++) v[k] = k;
  return v;
}
static std::vector<SetCase> set_cases() {
  std::vector<SetCase> c;
  auto add = [&](const char* name, uint32_t cap, std::vector<Ent> in, uint32_t stop, std::vector<Ent> want, uint32_t rate) {
    SetCase s;
    s.name = name, s.cap = cap, s.in = in, s.stop = stop, s.want = want, s.send_rate = rate;
    c.push_back(s);
    return &c.back();
  };
  const uint32_t DONE = UFC_RATE_DONE, FULL = UFC_RATE_RECV_FULL;
  std::vector<Ent> e = set_of(stamps({{5, kF}}));
  add("five_all_kept", 8, e, DONE, kept(e, upto(5)), 2 * val(4));
  e = set_of(stamps({{4, kX}, {4, kF}}));
  add("tail_only_kept", 8, e, DONE, kept(e, {4, 5, 6, 7}), 2 * val(7));
  e = set_of(stamps({{4, kF}, {4, kX}}));
  add("head_only_kept", 8, e, DONE, kept(e, {0, 1, 2, 3}), 2 * val(3));
  e = set_of({kF, kX, kF, kX, kF, kX, kF, kX});
  add("alternate_kept", 8, e, DONE, kept(e, {0, 2, 4, 6}), 2 * val(6));
  e = set_of(stamps({{8, kX}}));
  add("none_kept", 8, e, DONE, kept(e, {}), 2 * kFed);
  e = set_of(stamps({{5, kF}}));
  add("full_by_the_tail", 5, e, FULL, {}, 0);
  e = set_of(stamps({{4, kF}, {1, kX}}));
  add("room_by_the_tail", 5, e, DONE, kept(e, upto(4)), 2 * val(3));
  e = set_of(stamps({{23, kF}}));
  add("cap24_fills", 24, e, DONE, kept(e, upto(23)), 2 * val(22));
  e = set_of(stamps({{24, kF}}));
  add("cap24_full", 24, e, FULL, {}, 0);
  const std::vector<uint32_t> desc = {val(5), val(4), val(3), val(2), val(1), 900000};
  e = set_of(stamps({{6, kF}}), desc);
  add("max_in_tail", 8, e, DONE, kept(e, upto(6)), 1800000);
  e = set_of(stamps({{5, kF}, {1, kX}}), desc);
  add("max_in_tail_expired", 8, e, DONE, kept(e, upto(5)), 2 * val(5));
  // now 40: ~0 - 10 and ~0 wrap to the ages 51 and 41 (kept); 45 and 1000 lie ahead of now (ages near 2^64)
  e = set_of({10, 10, 10, 10, ~0ull - 10, 45, ~0ull, 1000});
  add("wrapped_ages_in_tail", 8, e, DONE, kept(e, {0, 1, 2, 3, 4, 6}, 40), 2 * val(6))->now = 40;
  e = set_of(stamps({{8, kF}}), {val(0), val(1), val(2), val(3), val(4), val(5), 900000, val(7)});
  add("replace_max_tail", 8, e, DONE, {{kNow, 900000, false}}, 1800000)->limited = false;
  SetCase* li = add("replace_max_tail_loss_increase", 8, e, DONE, {{kNow, 450000, false}}, 450000);
  li->limited = false, li->prev_loss = 0.0;
  e = set_of(stamps({{6, kF}}), {0xFFFFFFFFu, val(1), val(2), val(3), val(4), 900000});
  e[0].initial = true;
  add("initial_skipped_with_tail", 8, e, DONE, {{kNow, 900000, false}}, 1800000)->limited = false;
  e = set_of(stamps({{8, kF}}), {val(0), val(1), val(2), val(3), val(4), val(5), val(6), 900000});
  add("nofeedback_max_in_tail", 8, e, DONE, {{kNow, 450000, false}}, 900000)->feedback = false;
  e = set_of(stamps({{5, kF}}));
  add("room_at_arena_end", 6, e, DONE, kept(e, upto(5)), 2 * val(4))->arena_last = true;
  return c;
}
// Every case between two neighbours of one entry, the rooms adjoining in a heap arena of exactly the rooms' bytes
// (room_at_arena_end's room last, the last neighbour's first): an entry written outside a room is a changed
// neighbour or, past the arena, AddressSanitizer's.
static void run_set_cases() {
  const std::vector<SetCase> cases = set_cases();
  const size_t n = 2 * cases.size() + 1;
  std::vector<const SetCase*> conn(n, nullptr);
  for (size_t k = 0; k < cases.size(); k++) conn[2 * k + 1] = &cases[k];
  CHECK(cases.size() == 17 && cases.back().arena_last);
  std::vector<uint32_t> cap(n), first(n);
  size_t total = 0;
  for (size_t c = 0; c < n; c++) total += cap[c] = conn[c] ? conn[c]->cap : 1;
  first[n - 1] = 0;  // the neighbour behind the last case
  uint32_t at = 1;
  for (size_t c = 0; c + 1 < n; c++) {
    first[c] = at;
    at += cap[c];
  }
  CHECK(at == total && first[n - 2] + cap[n - 2] == total);
  ufc_recv_rate_entry* arena = (ufc_recv_rate_entry*)std::malloc(total * sizeof(ufc_recv_rate_entry));
  std::vector<ufc_rate_state> states(n);
  std::vector<ufc_rate_tick> ticks(n);
  std::vector<ufc_frame_queue_result> fq(n);
  std::vector<ufc_flush> flushes(n);
  std::vector<uint32_t> fi(n);
  std::memset(flushes.data(), 0, n * sizeof(ufc_flush));
  for (size_t c = 0; c < n; c++) {
    const SetCase* k = conn[c];
    const uint64_t now = k ? k->now : kNow;
    ufc_rate_state s = new_state(0xFFFFFFFFu, cap[c]);
    s.mode = UFC_RATE_THROUGHPUT_EQN;
    s.send_rate = s.send_rate_tcp = 100000;
    s.has_rtt_s = s.has_rtt_ms = s.has_rto_ms = s.nofeedback_idle = s.has_nofeedback_exp = 1;
    s.rtt_s = 0.05;
    s.rtt_ms = 50;
    s.rto_ms = 200;
    s.nofeedback_exp_ms = now + 5000;
    s.prev_loss_rate = k ? k->prev_loss : 1e-9;
    s.now_ms = now - 10;
    s.recv_first = first[c];
    if (k && !k->feedback) {
      s.nofeedback_exp_ms = now;
      s.nofeedback_idle = 0;
      s.send_rate_tcp = 1000000000;
    }
    const std::vector<Ent> one = {{kF, 30000 + (uint32_t)(c / 2), false}};
    const std::vector<Ent>& in = k ? k->in : one;
    s.recv_count = (uint32_t)in.size();
    for (uint32_t j = 0; j < cap[c]; j++) {
      ufc_recv_rate_entry& e = arena[first[c] + j];
      std::memset(&e, 0x5A, sizeof e);  // (behind the count: rubbish)
      if (j < in.size()) e = rate_entry(in[j].t, in[j].v, in[j].initial);
    }
    states[c] = s;
    ticks[c] = tick(now, 0.01, 0, 0);
    fq[c] = (!k || k->feedback) ? feedback(50, kFed, 1e-9, k ? k->limited : false) : ufc_frame_queue_result{};
    flushes[c].flush_alloc = -7;
    fi[c] = (uint32_t)c;
  }
  std::vector<ufc_recv_rate_entry> before(arena, arena + total);
  RateArgs a{};
  a.n = n;
  a.entries = arena;
  a.n_entries = total;
  a.flushes = flushes.data();
  a.n_flushes = n;
  a.flush_index = fi.data();
  for (size_t c = 0; c < n; c++) {
    const SetCase* k = conn[c];
    ufc_rate_state S = states[c];
    ufc_rate_result R;
    rate_step(a, c, S, ticks[c], fq[c], R);
    const ufc_recv_rate_entry* room = arena + first[c];
    if (!k) {  // a neighbour: its one entry replaced by the maximum of itself and the feedback
      CHECK(R.stop == UFC_RATE_DONE && S.recv_count == 1 && (room[0] == Ent{kNow, kFed, false}));
      continue;
    }
    if (R.stop != k->stop) std::printf("FAIL %s: stop %u\n", k->name, R.stop), failures++;
    if (k->stop != UFC_RATE_DONE) {
      CHECK(std::memcmp(&S, &states[c], sizeof S) == 0 && flushes[c].flush_alloc == -7);
      CHECK(std::memcmp(room, &before[first[c]], cap[c] * sizeof *room) == 0);
      continue;
    }
    bool ok = S.rtt_ms == 50 && S.recv_count == k->want.size() && R.recv_count == S.recv_count && R.send_rate == k->send_rate &&
              S.send_rate == k->send_rate && flushes[c].flush_alloc == R.flush_alloc;
    for (size_t j = 0; ok && j < k->want.size(); j++) ok = room[j] == k->want[j];
    const size_t behind = std::max<size_t>(k->want.size(), k->in.size());  // what no entry reached is what it was
    ok = ok && std::memcmp(room + behind, &before[first[c] + behind], (cap[c] - behind) * sizeof *room) == 0;
    if (k->arena_last) ok = ok && first[c] + cap[c] == total && (arena[total - 1] == Ent{kNow, kFed, false});
    if (!ok) std::printf("FAIL %s: count %u, send_rate %u\n", k->name, S.recv_count, R.send_rate), failures++;
  }
  std::free(arena);
}

int main() {
  // ---- the goldens' shapes, numbers traced by hand ----
  const ufc_frame_queue_result none{};
  {
    One c(1000000, 4);
    c.step(tick(1000, 0.5, 0, 0), feedback(100, 50000, 0.0, false));  // AwaitSend ignores a step
    CHECK(c.r.stop == UFC_RATE_DONE && c.r.mode == UFC_RATE_AWAIT_SEND && c.r.flags == 0 && c.r.send_rate == 1472);
    CHECK(c.s.has_last_flush == 1 && c.r.flush_alloc == 0 && c.r.rtt_ms == 150 && c.r.rto_ms == 600);
    // a frame of 1000 bytes went out at 1000; the first feedback, without loss, at 1100: 4380 / 0.1 s
    c.step(tick(1100, 0.1, -1000, UFC_RATE_FRAME_SENT), feedback(100, 50000, 0.0, false));
    CHECK(c.r.mode == UFC_RATE_SLOW_START && c.r.send_rate == 43800 && c.r.flags == UFC_RATE_FEEDBACK);
    CHECK(c.r.flush_alloc == -853);  // -1000 + round(1472 * 0.1), below alloc_max = 0 (no RTT before the step)
    CHECK(c.s.has_time_last_doubled && c.s.time_last_doubled_ms == 1100 && c.s.rtt_ms == 100 && c.s.rtt_s == 0.1);
    CHECK(c.s.recv_count == 1 && c.arena[0].value == 50000 && c.arena[0].timestamp_ms == 1100 && !c.arena[0].is_initial);
    // rto = max(0.4, 2944 / 1472 = 2.0) = 2 s, taken with the rate before the step
    CHECK(c.s.rto_ms == 2000 && c.s.nofeedback_exp_ms == 3100 && c.s.nofeedback_idle == 1);
    // doubling is gated by rtt_ms: 50 ms later nothing, 100 ms later 2 * 43800 limited by 2 * 50000
    c.step(tick(1150, 0.05, 0, 0), feedback(100, 50000, 0.0, false));
    CHECK(c.r.send_rate == 43800 && c.s.time_last_doubled_ms == 1100);
    c.step(tick(1200, 0.05, 0, 0), feedback(100, 50000, 0.0, false));
    CHECK(c.r.send_rate == 87600 && c.s.time_last_doubled_ms == 1200);
    // loss after doubling: target = send_rate / 2, limit = max(50000 / 2, 0.85 * 50000) = 42500
    c.step(tick(1300, 0.1, 0, 0), feedback(100, 50000, 0.01, false));
    CHECK(c.r.mode == UFC_RATE_THROUGHPUT_EQN && c.s.send_rate_tcp == 43800 && c.r.send_rate == 42500);
    CHECK(c.r.flags == (UFC_RATE_FEEDBACK | UFC_RATE_RESET_ISSUED | UFC_RATE_ENTERED_EQN) && c.s.has_reset == 1);
    CHECK(c.r.inv_iterations >= 1 && c.s.reset_loss_rate > 0.0 && c.s.reset_loss_rate < 1.0);
    CHECK(!c.s.has_time_last_doubled && c.s.time_last_doubled_ms == 0);
  }
  {  // the two stalls: rtt 0.01 s with target 5 (first loss: 736 / rtt is far above, so through send_rate / 2)
    uint32_t it;
    bool stalled;
    double p = rate_tcp_throughput_inv(0.01, 5, it, stalled);
    CHECK(stalled && p == 1.0 && it == 54);
    p = rate_tcp_throughput_inv(0.05, 11, it, stalled);
    CHECK(stalled && p == 1.0 && it == 54);
    p = rate_tcp_throughput_inv(0.1, 7360, it, stalled);
    CHECK(!stalled && it < 64 && p > 0.0 && p < 1.0);
    p = rate_tcp_throughput_inv(std::numeric_limits<double>::quiet_NaN(), 100, it, stalled);
    CHECK(stalled && p == 0.0 && it > 1000 && it < 1200);
  }
  {  // the empty set: an updated rtt of 0 ms with a rate-limited feedback; nothing changes
    One c(1000000, 2);
    c.step(tick(10, 0.0, 0, UFC_RATE_FRAME_SENT), none);
    const ufc_rate_state before = c.s;
    const ufc_recv_rate_entry e0 = c.arena[0];
    c.step(tick(20, 0.01, 0, 0), feedback(0, 1000, 0.0, true));
    CHECK(c.r.stop == UFC_RATE_REF_PANIC && c.r.mode == 0 && c.r.send_rate == 0 && c.r.flags == 0);
    CHECK(std::memcmp(&before, &c.s, sizeof before) == 0 && std::memcmp(&e0, &c.arena[0], sizeof e0) == 0);
    // the initial entry survives a rate-limited update: limit = u32::MAX saturating
    c.step(tick(20, 0.01, 0, 0), feedback(100, 1000, 0.0, true));
    CHECK(c.r.stop == UFC_RATE_DONE && c.r.recv_count == 2 && c.arena[0].is_initial && c.arena[1].value == 1000);
    CHECK(c.r.send_rate == 43800);
    const ufc_rate_state full = c.s;
    c.step(tick(30, 0.01, 0, 0), feedback(100, 1000, 0.0, true));  // a third entry has no room
    CHECK(c.r.stop == UFC_RATE_RECV_FULL && std::memcmp(&full, &c.s, sizeof full) == 0);
  }
  {  // nofeedback without an RTT: the RTO doubles from 2 s as the rate halves
    One c(1000000, 1);
    c.step(tick(0, 0.0, 0, UFC_RATE_FRAME_SENT), none);
    CHECK(c.s.mode == UFC_RATE_SLOW_START && c.s.nofeedback_exp_ms == 2000 && c.r.flags == 0);
    c.step(tick(1999, 1.0, 0, 0), none);
    CHECK(c.r.flags == 0 && c.r.send_rate == 1472);
    c.step(tick(2000, 1.0, 0, 0), none);
    CHECK(c.r.flags == UFC_RATE_NOFEEDBACK && c.r.send_rate == 736 && c.s.rto_ms == 4000 && c.s.nofeedback_exp_ms == 6000);
    c.step(tick(6000, 1.0, 0, 0), none);
    CHECK(c.r.send_rate == 368 && c.s.rto_ms == 8000 && c.s.nofeedback_exp_ms == 14000);
  }
  {  // the fill: cap by alloc_max, a negative allocation, saturation
    One c(1000000, 1);
    c.s.has_last_flush = 1;
    c.s.has_rtt_s = 1;
    c.s.rtt_s = 0.1;
    c.s.send_rate = 10000;
    c.s.flush_alloc = 500;
    c.step(tick(5, 1.0, 0, 0), none);
    CHECK(c.r.flush_alloc == 1000);  // 500 + 10000 capped by 10000 * 0.1
    c.step(tick(6, 0.0105, -3000, 0), none);
    CHECK(c.r.flush_alloc == -1895);  // 1000 - 3000 + round(105.0)
    c.s.flush_alloc = INT64_MAX;
    c.s.rtt_s = 1e300;
    c.step(tick(7, 1.0, 0, 0), none);
    CHECK(c.r.flush_alloc == INT64_MAX);
    c.s.flush_alloc = INT64_MIN;
    c.step(tick(8, -1.0, 0, 0), none);
    CHECK(c.r.flush_alloc == INT64_MIN);
    c.step(tick(9, std::numeric_limits<double>::quiet_NaN(), -1, 0), none);
    CHECK(c.r.flush_alloc == INT64_MAX);  // the adjustment wraps; a NaN adds 0
  }
  {  // begin: the step record and the pending reset
    ufc_rate_state s = new_state(1, 1);
    ufc_frame_queue_step q;
    rate_begin(s, 500, UFC_FQ_MARK_RATE_LIMITED, q);
    CHECK(q.flags == (UFC_FQ_FORGET | UFC_FQ_FEEDBACK | UFC_FQ_MARK_RATE_LIMITED) && q.thresh_ms == 0 && q.rtt_ms == 0);
    s.has_rtt_ms = 1;
    s.rtt_ms = 20;
    s.has_reset = 1;
    s.reset_loss_rate = 0.25;
    rate_begin(s, 500, 0, q);
    CHECK(q.flags == (UFC_FQ_FORGET | UFC_FQ_FEEDBACK | UFC_FQ_HAS_RTT | UFC_FQ_RESET_LOSS) && q.thresh_ms == 420);
    CHECK(q.rtt_ms == 20 && q.now_ms == 500 && q.reset_loss_rate == 0.25 && !s.has_reset && s.reset_loss_rate == 0.0);
  }

  run_set_cases();

  // ---- a random batch over exact-size buffers ----
  const double edge_f[] = {0.0, -0.0, 1.0, 1e-9, 5e-324, 1e-310, INFINITY, -INFINITY, NAN, -1.0, 1e300, 0.5};
  const uint64_t edge_u[] = {0, 1, 150, 1ull << 32, (1ull << 63) - 1, 1ull << 63, ~0ull - 2000, ~0ull};
  const uint32_t edge_r[] = {0, 1, 23, 46, 1472, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
  auto f64 = [&]() { return rnd_below(5) == 0 ? edge_f[rnd_below(12)] : std::pow(10.0, -6.0 * rnd_unit()); };
  auto u64 = [&](uint64_t near) { return rnd_below(6) == 0 ? edge_u[rnd_below(8)] : near + rnd_below(4000) - 2000; };
  auto u32 = [&]() { return rnd_below(5) == 0 ? edge_r[rnd_below(8)] : (uint32_t)std::pow(10.0, 9.6 * rnd_unit()); };
  size_t stops[4] = {0, 0, 0, 0}, stalled = 0;
  for (int round = 0; round < 40; round++) {
    const size_t n = 1 + rnd_below(300);
    const uint32_t cap = 1 + (uint32_t)(round % 3 == 2 ? rnd_below(24) : rnd_below(5));
    std::vector<ufc_rate_state> states(n), out(n);
    std::vector<ufc_rate_tick> ticks(n);
    std::vector<ufc_frame_queue_result> fq(n);
    std::vector<ufc_rate_result> results(n);
    std::vector<ufc_recv_rate_entry> entries(n * cap);
    std::vector<ufc_flush_result> fres(n / 2 + 1);
    std::vector<ufc_flush> flushes(n);
    std::vector<uint32_t> ri(n), fi(n);
    std::memset(entries.data(), 0, entries.size() * sizeof(ufc_recv_rate_entry));
    std::memset(fres.data(), 0, fres.size() * sizeof(ufc_flush_result));
    std::memset(flushes.data(), 0, flushes.size() * sizeof(ufc_flush));
    for (size_t c = 0; c < n; c++) {
      ufc_rate_state s = new_state(rnd_below(2) ? 0xFFFFFFFFu : u32(), cap);
      const uint64_t base = u64(1000000);
      s.mode = (uint32_t)rnd_below(3);
      s.send_rate = u32();
      s.send_rate_tcp = u32();
      s.has_time_last_doubled = rnd_below(2);
      s.has_nofeedback_exp = rnd_below(2);
      s.nofeedback_idle = rnd_below(2);
      s.has_rtt_s = s.mode == UFC_RATE_THROUGHPUT_EQN ? 1 : rnd_below(2);
      s.has_rtt_ms = rnd_below(2);
      s.has_rto_ms = rnd_below(2);
      s.has_last_flush = rnd_below(2);
      s.has_reset = rnd_below(2);
      s.time_last_doubled_ms = u64(base);
      s.prev_loss_rate = f64();
      s.nofeedback_exp_ms = u64(base);
      s.rtt_s = f64();
      s.rtt_ms = u64(100);
      s.rto_ms = u64(400);
      s.now_ms = base;
      s.flush_alloc = rnd_below(8) == 0 ? (rnd_below(2) ? INT64_MAX : INT64_MIN) : (int64_t)rnd_below(200000) - 100000;
      s.reset_loss_rate = f64();
      s.recv_first = c * cap;
      s.recv_count = (uint32_t)(s.mode == UFC_RATE_AWAIT_SEND ? rnd_below(cap + 1) : 1 + rnd_below(cap));
      if (rnd_below(25) == 0) {  // one broken rule
        switch (rnd_below(5)) {
          case 0: s.mode = 3 + (uint32_t)rnd_below(100); break;
          case 1: s.recv_cap = 0; break;
          case 2: s.recv_count = cap + 1; break;
          case 3: s.recv_first = rnd_below(2) ? n * (uint64_t)cap - cap + 1 : ~0ull; break;
          default: s.mode = UFC_RATE_THROUGHPUT_EQN; s.has_rtt_s = 0; break;
        }
      }
      for (uint32_t k = 0; k < cap; k++) {
        ufc_recv_rate_entry& e = entries[c * cap + k];
        e.timestamp_ms = u64(base);
        e.value = u32();
        e.is_initial = k == 0 && rnd_below(3) == 0;
      }
      states[c] = s;
      ticks[c] = tick(rnd_below(10) ? base + rnd_below(3000) : u64(base), rnd_below(5) ? 10.0 * rnd_unit() : f64(),
                      rnd_below(6) == 0 ? (rnd_below(2) ? INT64_MAX : INT64_MIN) : -(int64_t)rnd_below(3000),
                      (uint32_t)rnd_below(2));
      fq[c] = rnd_below(5) < 3 ? feedback(rnd_below(4) ? rnd_below(2000) : u64(0), u32(), f64(), rnd_below(5) < 2) : none;
      ri[c] = rnd_below(3) == 0 ? UFC_NO_PARENT : (uint32_t)rnd_below(fres.size() + 2);
      fi[c] = rnd_below(4) == 0 ? UFC_NO_PARENT : (uint32_t)c;
    }
    for (auto& f : fres) {
      f.alloc_left = (int64_t)rnd_below(100000) - 3000;
      f.frame_count = (uint32_t)rnd_below(3);
    }
    const std::vector<ufc_recv_rate_entry> entries_in = entries;
    RateArgs a{states.data(), ticks.data(), fq.data(), n, entries.data(), entries.size(), fres.data(), fres.size(),
               ri.data(), flushes.data(), flushes.size(), fi.data(), results.data(), out.data()};
    for (size_t c = 0; c < n; c++) {
      ufc_rate_state S = states[c];
      ufc_rate_result R;
      rate_step(a, c, S, ticks[c], fq[c], R);
      results[c] = R;
      out[c] = S;
      CHECK(R.stop <= UFC_RATE_RECV_FULL);
      stops[R.stop & 3]++;
      stalled += (R.flags & UFC_RATE_INV_STALLED) != 0;
      if (R.stop != UFC_RATE_DONE) {  // nothing changed
        CHECK(std::memcmp(&S, &states[c], sizeof S) == 0);
        CHECK(R.mode == 0 && R.flags == 0 && R.send_rate == 0 && R.flush_alloc == 0 && R.recv_count == 0);
        if (R.stop != UFC_RATE_BAD_STATE)
          CHECK(std::memcmp(&entries[c * cap], &entries_in[c * cap], cap * sizeof(ufc_recv_rate_entry)) == 0);
        if (fi[c] < n) CHECK(flushes[fi[c]].flush_alloc == 0);
      } else {  // the state that comes out passes the check, and its set is what the result says
        CHECK(rate_state_ok(S, entries.size()) && S.recv_count == R.recv_count && S.recv_count <= cap);
        CHECK(S.flush_alloc == R.flush_alloc && S.now_ms == ticks[c].now_ms && S.has_last_flush == 1);
        CHECK(R.inv_iterations <= 1200 && S.send_rate == R.send_rate && S.mode == R.mode);
        if (R.flags & UFC_RATE_FEEDBACK) CHECK(S.send_rate <= S.max_send_rate);
        if (fi[c] < n) CHECK(flushes[fi[c]].flush_alloc == R.flush_alloc);
        // a second step from the new state, in place, stays inside the room too
        ufc_rate_state S2 = S;
        ufc_rate_result R2;
        RateArgs b = a;
        b.flush_results = nullptr;
        b.flushes = nullptr;
        rate_step(b, c, S2, tick(S.now_ms + rnd_below(500), 0.02, 0, 1), fq[(c + 1) % n], R2);
        CHECK(R2.stop != UFC_RATE_BAD_STATE);
      }
    }
  }
  CHECK(stops[0] > 1000 && stops[1] > 20 && stops[2] > 20 && stops[3] > 5 && stalled > 5);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok: done %zu, bad state %zu, ref panic %zu, recv full %zu, stalled %zu\n", stops[0], stops[1], stops[2],
              stops[3], stalled);
  return 0;
}
