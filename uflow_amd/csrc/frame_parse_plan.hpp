// frame_parse_plan.hpp -- the index arithmetic of the GPU batch parse (frame_parse.hip) that its host check
// (tests/c/parse_host_check.hip) runs thread by thread: frame lengths, the mode a frame's items take, the
// header-slot pool, the slot segment's capacity, the emit's owner search, header offsets and the plan of the
// emit's header fetch.  Nothing here touches memory except through what the caller hands in.
#pragma once
#include <cstdint>

#include "frame_codec_core.hpp"

namespace ufc_parse_plan {

constexpr int kParseThreads = 256;
#ifndef UFC_POS_SLOTS
#define UFC_POS_SLOTS 64
#endif
constexpr uint32_t kPosSlots = UFC_POS_SLOTS;  // datagram headers recorded per frame (a data frame holds <= 127)
constexpr uint64_t kSegWords = (uint64_t)kPosSlots * kParseThreads;  // u16 per workgroup segment
enum : uint8_t { kItemsNone = 0, kItemsPos = 1, kItemsAck = 2, kItemsWalk = 3 };
constexpr uint32_t kNoSegment = 0xFFFFFFFFu;  // a workgroup that found no room for its slots

// Length of frame i, its start in `a`: offsets that go backwards give 0, lengths saturate at 2^32 - 1.
UFC_HD uint32_t frame_len32(const uint64_t* offsets, uint64_t i, uint64_t& a) {
  a = offsets[i];
  const uint64_t b = offsets[i + 1];
  const uint64_t len64 = b >= a ? b - a : 0;
  return len64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len64;
}

// How the emit finds the cnt (> 0) items of an accepted frame: ack groups sit at fixed offsets; a data
// frame's headers are in u16 slots when there are at most kPosSlots of them, every offset fits 16 bits and
// the pool did not run out; else the frame is walked again.  (This condition and UFC_PARSE_SEG_NO_ROOM are
// macros: as inline functions they changed the walk kernel's code, profiles/EXPERIMENTS.md "parse plan hoist".)
#define UFC_PARSE_SLOTS_HOLD(cnt, len, full) ((cnt) <= kPosSlots && (len) <= 0xFFFFu && !(full))
inline uint8_t items_mode(bool ack, uint32_t cnt, uint32_t len, bool full) {
  if (ack) return kItemsAck;
  return UFC_PARSE_SLOTS_HOLD(cnt, len, full) ? kItemsPos : kItemsWalk;
}

// u16 header slots of a call: min(64 n, items_cap), at least 1, below 2^32 - 1 so that every segment fits
// 32-bit offsets and no segment base can equal kNoSegment.
inline uint64_t seg_cap(uint64_t n, uint64_t items_cap) {
  const uint64_t want = n * kPosSlots, room = items_cap > 1 ? items_cap : 1;
  const uint64_t c = want < room ? want : room;
  return c < 0xFFFFFFFEull - kSegWords ? c : 0xFFFFFFFEull - kSegWords;
}
// Whether a workgroup of `total` slots, given the cursor's value before its add, finds no room.
#define UFC_PARSE_SEG_NO_ROOM(b64, total, cap) ((total) && (b64) + (total) > (cap))

// The walk's header slots: kInlineSlots slots per frame, and the headers past them in a per-workgroup pool
// of linked entries (offset | next << 16) taken one at a time with `add` (the workgroup's counter + 1,
// returning the value before).  A frame that finds the pool full is walked again by the emit.
constexpr uint32_t kInlineSlots = 16;
constexpr uint32_t kPoolSlots = 2048;
constexpr uint32_t kPoolNil = 0xFFFFu;

template <class Add>
struct PoolSink {
  static constexpr bool kDecode = false;
  uint16_t* slot;     // this thread's inline slots (slot k at k * kParseThreads)
  uint32_t* pool;     // the workgroup's pool
  uint32_t* ctr;      // its allocation counter
  uint32_t* head;     // this thread's list (registers, through pointers: the sink is const)
  uint32_t* tail;
  bool* full;
  UFC_HD bool on() const { return true; }
  UFC_HD void operator()(uint32_t, const ufc_item&) const {}
  UFC_HD void header(uint32_t k, uint32_t off) const {
    if (k < kInlineSlots) {
      slot[k * kParseThreads] = (uint16_t)off;
      return;
    }
    if (*full) return;
    const uint32_t idx = Add::add(ctr);
    if (idx >= kPoolSlots) {
      *full = true;
      return;
    }
    pool[idx] = off | (kPoolNil << 16);
    if (k == kInlineSlots)
      *head = idx;
    else
      pool[*tail] = (pool[*tail] & 0xFFFFu) | (idx << 16);
    *tail = idx;
  }
};

// Owner of item g among the workgroup's nb frames: the last frame whose first item is <= g (frames without
// items share their successor's first item, and are passed over).
template <class First>
UFC_HD uint32_t owner_of(const First& lfirst, uint32_t nb, uint32_t g) {
  uint32_t lo_f = 0, hi_f = nb - 1;
  while (lo_f < hi_f) {
    const uint32_t mid = (lo_f + hi_f + 1) >> 1;
    if (lfirst(mid) <= g)
      lo_f = mid;
    else
      hi_f = mid - 1;
  }
  return lo_f;
}

// Frame offset of ack group k.
UFC_HD uint32_t ack_hoff(uint32_t k) { return 1u + ufc_codec::kAckPayloadHeader + UFC_ACK_GROUP_SIZE * k; }

// The workgroup's buffer range over [span_lo, span_hi) at byte address base_addr: 4-byte aligned base
// (delta bytes before base_addr), rounded up to whole dwords.  Spans that go backwards or reach 4 GiB
// take byte loads instead (ok false).
struct SpanRange {
  uint32_t delta;
  uint64_t range;
  bool ok;
};
UFC_HD SpanRange span_range(uint64_t span_lo, uint64_t span_hi, uint64_t base_addr) {
  SpanRange r;
  r.delta = (uint32_t)(base_addr & 3u);
  r.range = (span_hi - span_lo + r.delta + 3) & ~(uint64_t)3;
  r.ok = span_hi >= span_lo && r.range < 0xFFFFFFF0ull;
  return r;
}
// A header's byte offset in the range, and whether one unaligned 16-byte load at it stays inside the range
// (else an aligned 16-byte load at ex & ~3 and the dword behind it, shifted by ex & 3).
UFC_HD uint32_t fetch_ex(uint64_t frame_start, uint64_t span_lo, uint32_t delta, uint32_t hoff) {
  return (uint32_t)(frame_start - span_lo) + delta + hoff;
}
UFC_HD bool fetch_exact(uint32_t ex, uint64_t range) { return ex + 16 <= (uint32_t)range; }

// Bytes the byte-load path reads of a header whose first byte is b0: the header and no more (a micro header
// with no payload ends 4 bytes before its frame does).
UFC_HD uint32_t fallback_bytes(bool ack, uint32_t b0) {
  if (ack) return UFC_ACK_GROUP_SIZE;
  return (b0 & 0x80u) == 0 ? 6u : (b0 & 0x40u) == 0 ? 9u : 14u;
}

}  // namespace ufc_parse_plan
