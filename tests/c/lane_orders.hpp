// lane_orders.hpp -- test only: wave policies with the whole interface of wave.hpp's SerialWave (lanes, one,
// ballot, sum, sync, or64, add64) that run the 64 lanes of a phase in another order.  The result of a step must
// not depend on the order: a lane that reads what another lane writes in the same phase is a race on the device,
// where the lanes of a phase run at once.  The host checks run every round under SerialWave, ReverseWave and
// ShuffledWave and want the same bytes from all three.
#pragma once
#include <cstdint>

namespace lane_orders {

// The lanes 63..0.
struct ReverseWave {
  template <class F>
  void lanes(const F& f) const {
    for (uint32_t l = 64; l-- > 0;) f(l);
  }
  template <class F>
  void one(const F& f) const {
    f();
  }
  template <class F>
  unsigned long long ballot(const F& f) const {
    unsigned long long m = 0;
    for (uint32_t l = 64; l-- > 0;)
      if (f(l)) m |= 1ull << l;
    return m;
  }
  template <class F>
  uint64_t sum(const F& f) const {
    uint64_t s = 0;
    for (uint32_t l = 64; l-- > 0;) s += f(l);
    return s;
  }
  void sync() const {}
  static void or64(unsigned long long* p, unsigned long long v) { *p |= v; }
  static void add64(unsigned long long* p, unsigned long long v) { *p += v; }
};

// A fresh permutation of 0..63 for every phase (lanes, ballot and sum each draw one), from one seeded generator
// that all instances share, so a run is the same every time and no two phases of it see the same order.
struct ShuffledWave {
  struct Order {
    uint8_t at[64];
  };
  static uint64_t& state() {
    static uint64_t s = 0x1A9E0DE5u;
    return s;
  }
  static void seed(uint64_t s) { state() = s; }
  static uint32_t draw() {  // splitmix64
    uint64_t z = (state() += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
  }
  static Order order() {  // Fisher-Yates
    Order o;
    for (uint32_t k = 0; k < 64; k++) o.at[k] = (uint8_t)k;
    for (uint32_t k = 64; k > 1; k--) {
      const uint32_t j = draw() % k;
      const uint8_t t = o.at[k - 1];
      o.at[k - 1] = o.at[j];
      o.at[j] = t;
    }
    return o;
  }
  template <class F>
  void lanes(const F& f) const {
    const Order o = order();
    for (uint32_t k = 0; k < 64; k++) f((uint32_t)o.at[k]);
  }
  template <class F>
  void one(const F& f) const {
    f();
  }
  template <class F>
  unsigned long long ballot(const F& f) const {
    const Order o = order();
    unsigned long long m = 0;
    for (uint32_t k = 0; k < 64; k++)
      if (f((uint32_t)o.at[k])) m |= 1ull << o.at[k];
    return m;
  }
  template <class F>
  uint64_t sum(const F& f) const {
    const Order o = order();
    uint64_t s = 0;
    for (uint32_t k = 0; k < 64; k++) s += f((uint32_t)o.at[k]);
    return s;
  }
  void sync() const {}
  static void or64(unsigned long long* p, unsigned long long v) { *p |= v; }
  static void add64(unsigned long long* p, unsigned long long v) { *p += v; }
};

}  // namespace lane_orders
