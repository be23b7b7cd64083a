// The frame routing's host calls (ufc_route_table_build_host, ufc_route_frames_host: uflow_amd/csrc/frame_codec.cpp
// over the lane functions of frame_codec_core.hpp, rt_lookup / rt_classify / rt_bucket, which the device runs too) as
// host code under AddressSanitizer and UBSan, over seeded random batches, with 1 and 3 threads.  Checked against a
// plain sequential restatement written here from the reference's text (Server::handle_frames, src/server/mod.rs:
// 591-602: the pairs one after the other, a std::map keyed by the 32 key bytes, an address stopped at its first
// control frame), with the hash, the insertion and the bounded probe restated beside it: every output must be equal
// byte for byte.  All buffers have their exact sizes.  Tables: built ones from 0 to 700 connections at loads up to
// n_conns + 1 slots (long wrapping chains), a max_probe below the longest displacement, and arbitrary bytes with no
// empty slot.  The routing kernels take no wave policy (a lane works on its own frame; the placement is a function of
// the keys), so there is no lane order to vary here.  Prints "ok: <checks>" and exits 0; any difference or sanitizer
// report stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/uflow_frame_codec.h"

namespace {

long checks = 0;

void fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  std::exit(1);
}

uint64_t rng_state = 0x5EEDF00Du;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

std::string key_of(const ufc_addr& a) { return std::string((const char*)&a, 32); }

uint32_t hash_key(uint32_t seed, const std::string& k) {
  uint32_t h = seed;
  for (int j = 0; j < 8; j++) {
    const uint32_t w = (uint8_t)k[4 * j] | ((uint32_t)(uint8_t)k[4 * j + 1] << 8) |
                       ((uint32_t)(uint8_t)k[4 * j + 2] << 16) | ((uint32_t)(uint8_t)k[4 * j + 3] << 24);
    h = (h ^ w) * 0x9E3779B1u;
    h ^= h >> 15;
  }
  h *= 0x85EBCA77u;
  h ^= h >> 13;
  return h;
}

uint32_t probe(const std::vector<ufc_route_slot>& slots, uint32_t seed, uint32_t max_probe, size_t n_conns,
               const std::string& k) {
  const size_t mask = slots.size() - 1;
  const size_t home = hash_key(seed, k) & mask;
  const size_t last = max_probe < mask ? max_probe : mask;
  for (size_t p = 0; p <= last; p++) {
    const ufc_route_slot& s = slots[(home + p) & mask];
    if (!s.used) return UFC_NO_PARENT;
    if (s.conn < n_conns && key_of(s.key) == k) return s.conn;
  }
  return UFC_NO_PARENT;
}

ufc_addr addr_of(uint32_t id, bool v6) {
  ufc_addr a{};
  a.family = v6 ? 6 : 4;
  a.ip[0] = 10;
  a.ip[1] = (uint8_t)(id >> 16);
  a.ip[2] = (uint8_t)(id >> 8);
  a.ip[3] = (uint8_t)id;
  if (v6) a.ip[15] = 1;
  a.port = (uint16_t)(1000 + id % 13);
  if (v6) a.scope_id = id & 1;
  return a;
}

struct Out {
  std::vector<uint32_t> route, order;
  std::vector<uint8_t> cls;
  std::vector<uint64_t> bucket_first, src_base, timeout;
  std::vector<ufc_frame_info> infos;
  std::vector<ufc_route_result> results;
  uint32_t fuc;
};

template <class T>
void same(const char* what, const std::vector<T>& a, const std::vector<T>& b, long tag) {
  if (a.size() != b.size()) fail(what, tag, (long)a.size(), (long)b.size());
  for (size_t i = 0; i < a.size(); i++)
    if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) fail(what, tag, (long)i, -1);
  checks++;
}

// One round: a table, a batch, the call against the restatement.
void round(long tag, size_t n, size_t n_conns, size_t n_slots, bool garbage, bool short_probe, bool with_offsets) {
  const uint32_t seed = rnd();
  std::vector<ufc_addr> conn(n_conns);
  for (size_t c = 0; c < n_conns; c++) conn[c] = addr_of((uint32_t)(c * 37 + 1), c % 3 == 0);
  std::vector<ufc_route_slot> slots(n_slots);
  uint32_t max_probe = 0;
  std::map<std::string, uint32_t> clients;
  if (garbage) {
    for (auto& s : slots) {
      uint32_t w[12];
      for (auto& x : w) x = rnd() | (rnd() << 16);
      std::memcpy(&s, w, 48);
      s.used = (uint8_t)(1 + rnd() % 255);
      s.conn = rnd() % (uint32_t)(2 * n_conns + 1);
    }
    for (size_t c = 0; c < n_conns; c += 2) slots[rnd() % n_slots].key = conn[c];
    max_probe = rnd() % 2 ? 0xFFFFFFFFu : rnd() % (uint32_t)n_slots;
  } else {
    uint64_t dup = 12345;
    std::memset(slots.data(), 0xAB, n_slots * sizeof(ufc_route_slot));  // the build clears them
    const int rc = ufc_route_table_build_host(conn.data(), n_conns, seed, slots.data(), n_slots, &max_probe, &dup);
    if (rc != UFC_OK || dup != 12345) fail("build", tag, rc, (long)dup);
    // the restated insertion
    std::vector<ufc_route_slot> want(n_slots);
    std::memset(want.data(), 0, n_slots * sizeof(ufc_route_slot));
    uint32_t longest = 0;
    for (size_t c = 0; c < n_conns; c++) {
      const size_t home = hash_key(seed, key_of(conn[c])) & (n_slots - 1);
      uint32_t p = 0;
      while (want[(home + p) & (n_slots - 1)].used) p++;
      ufc_route_slot& s = want[(home + p) & (n_slots - 1)];
      s.key = conn[c];
      s.conn = (uint32_t)c;
      s.used = 1;
      if (p > longest) longest = p;
      clients[key_of(conn[c])] = (uint32_t)c;
    }
    same("slots", slots, want, tag);
    if (max_probe != longest) fail("max_probe", tag, max_probe, longest);
    if (short_probe && max_probe) max_probe--;
  }
  const bool by_map = !garbage && !short_probe;

  std::vector<ufc_frame_info> infos(n);
  std::vector<ufc_addr> addrs(n);
  std::vector<uint64_t> offsets(with_offsets ? n : 0), timeout_in(n_conns);
  std::vector<uint8_t> active(n_conns);
  for (auto& t : timeout_in) t = ((uint64_t)rnd() << 32) | rnd();
  for (auto& x : active) x = rnd() % 5 ? (uint8_t)(1 + rnd() % 255) : 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t w[8];
    for (auto& x : w) x = rnd() | (rnd() << 16);
    std::memcpy(&infos[i], w, 32);
    const uint32_t r = rnd() % 100;
    infos[i].kind = r < 4 ? (uint8_t)(rnd() % 6) : r < 8 ? (uint8_t)rnd() : (uint8_t)(10 + rnd() % 3);
    infos[i].ok = rnd() % 20 ? (uint8_t)(1 + rnd() % 255) : 0;
    addrs[i] = n_conns && rnd() % 8 ? conn[rnd() % n_conns] : addr_of(0x800000u + rnd() % 5, false);
    if (with_offsets) offsets[i] = ((uint64_t)rnd() << 32) | rnd();
  }
  const uint64_t now = rnd() % 4 ? rnd() : ~(uint64_t)0 - rnd() % 8, tmo = rnd() % 64;

  // the restatement
  Out w;
  w.route.assign(n, UFC_NO_PARENT);
  w.cls.assign(n, UFC_ROUTE_DROP);
  w.results.assign(n_conns, ufc_route_result{0, UFC_NO_PARENT, 0, 0});
  w.timeout = timeout_in;
  w.fuc = UFC_NO_PARENT;
  std::vector<std::vector<uint32_t>> buckets(n_conns + 2);
  std::vector<uint8_t> stopped(n_conns, 0);
  bool unknown_stopped = false;
  for (size_t i = 0; i < n; i++) {
    const std::string k = key_of(addrs[i]);
    uint32_t c;
    if (by_map) {
      auto it = clients.find(k);
      c = it == clients.end() ? UFC_NO_PARENT : it->second;
    } else {
      c = probe(slots, seed, max_probe, n_conns, k);
    }
    w.route[i] = c;
    const ufc_frame_info& f = infos[i];
    const bool control = f.ok && f.kind <= 5;
    const bool session = f.ok && (f.kind == UFC_FRAME_DATA || f.kind == UFC_FRAME_SYNC || f.kind == UFC_FRAME_ACK);
    uint8_t cls = UFC_ROUTE_DROP;
    if (control) {
      cls = UFC_ROUTE_CONTROL;
      if (c == UFC_NO_PARENT) {
        if (!unknown_stopped) w.fuc = (uint32_t)i;
        unknown_stopped = true;
      } else {
        if (!stopped[c]) w.results[c].first_control = (uint32_t)i;
        stopped[c] = 1;
      }
    } else if (session) {
      if (c == UFC_NO_PARENT) {
        cls = unknown_stopped ? UFC_ROUTE_DEFERRED : UFC_ROUTE_DROP;
      } else if (stopped[c]) {
        cls = UFC_ROUTE_DEFERRED;
        w.results[c].deferred++;
      } else if (active[c]) {
        cls = UFC_ROUTE_CONN;
        w.results[c].frames++;
        w.timeout[c] = now + tmo;
      }
    }
    w.cls[i] = cls;
    buckets[cls == UFC_ROUTE_CONN ? c : n_conns + (cls == UFC_ROUTE_DROP ? 1 : 0)].push_back((uint32_t)i);
  }
  w.bucket_first.assign(n_conns + 3, 0);
  for (size_t b = 0; b < n_conns + 2; b++) {
    w.bucket_first[b + 1] = w.bucket_first[b] + buckets[b].size();
    for (uint32_t i : buckets[b]) {
      w.order.push_back(i);
      w.infos.push_back(infos[i]);
      w.src_base.push_back(with_offsets ? offsets[i] : 0);
    }
  }

  for (int nthreads : {1, 3}) {
    Out g;
    g.route.assign(n, 0x55555555u);
    g.order.assign(n, 0x55555555u);
    g.cls.assign(n, 0x55);
    g.bucket_first.assign(n_conns + 3, 0x5555555555555555ull);
    g.src_base.assign(n, 0x5555555555555555ull);
    g.infos.resize(n);
    g.results.resize(n_conns);
    if (n) std::memset(g.infos.data(), 0x55, n * sizeof(ufc_frame_info));
    if (n_conns) std::memset(g.results.data(), 0x55, n_conns * sizeof(ufc_route_result));
    g.timeout = timeout_in;  // in place
    g.fuc = 0x55555555u;
    const int rc = ufc_route_frames_host(infos.data(), addrs.data(), with_offsets ? offsets.data() : nullptr, n,
                                         slots.data(), n_slots, seed, max_probe, n_conns, active.data(), now, tmo,
                                         g.timeout.data(), g.route.data(), g.cls.data(), g.bucket_first.data(),
                                         g.order.data(), g.infos.data(), g.src_base.data(), g.results.data(),
                                         g.timeout.data(), &g.fuc, nthreads);
    if (rc != UFC_OK) fail("route", tag, rc, nthreads);
    same("route", g.route, w.route, tag);
    same("cls", g.cls, w.cls, tag);
    same("bucket_first", g.bucket_first, w.bucket_first, tag);
    same("order", g.order, w.order, tag);
    same("infos_out", g.infos, w.infos, tag);
    same("src_base_out", g.src_base, w.src_base, tag);
    same("results", g.results, w.results, tag);
    same("timeout_out", g.timeout, w.timeout, tag);
    if (g.fuc != w.fuc) fail("first_unknown_control", tag, g.fuc, w.fuc);
  }
}

}  // namespace

int main() {
  // a duplicate address: the second occurrence is reported
  {
    std::vector<ufc_addr> a = {addr_of(1, false), addr_of(2, false), addr_of(3, true), addr_of(2, false)};
    std::vector<ufc_route_slot> s(8);
    uint32_t mp = 0;
    uint64_t dup = 99;
    if (ufc_route_table_build_host(a.data(), 4, 7, s.data(), 8, &mp, &dup) != UFC_ERR_INVALID_ARG || dup != 3)
      fail("dup", 0, (long)dup, 0);
    if (ufc_route_table_build_host(a.data(), 3, 7, s.data(), 3, &mp, &dup) != UFC_ERR_INVALID_ARG) fail("n_slots", 0, 0, 0);
    checks += 2;
  }
  const size_t conns[] = {0, 1, 2, 7, 63, 64, 255, 256, 700};
  long tag = 0;
  for (size_t n_conns : conns) {
    size_t tight = 1;
    while (tight <= n_conns) tight *= 2;  // the smallest table: full but for a few slots when n_conns = 2^k - 1
    for (size_t n_slots : {tight, tight * 4}) {
      for (size_t n : {(size_t)0, (size_t)1, (size_t)65, (size_t)1500, (size_t)2100}) {
        round(++tag, n, n_conns, n_slots, false, false, tag % 2 == 0);
        round(++tag, n, n_conns, n_slots, false, true, tag % 2 == 0);
        if (n_conns) round(++tag, n, n_conns, n_slots, true, false, tag % 2 == 0);
      }
    }
  }
  std::printf("ok: %ld checks\n", checks);
  return 0;
}
