// The GPU batch parse (uflow_amd/csrc/frame_parse.hip) thread by thread on the host, under AddressSanitizer and
// UBSan: walk -> scan -> emit per workgroup of 256 frames, with the arithmetic the kernels take from
// frame_parse_plan.hpp (frame lengths, the mode decision, the slot pool, the segment cursor, the owner search,
// header offsets, the fetch plan) and the rest of the kernels' bodies restated here line by line.  The 256
// threads of a phase, and the workgroups of a launch, run forwards, backwards and shuffled (lane_orders.hpp's
// generator): the pool's allocation order and the segment bases change, infos and items must not.  Every
// result is compared with the codec core's serial read_frame, frame by frame.
//
// Frame bytes live in heap blocks of exactly the bytes the call may read.  The emit's buffer loads are modelled
// with the hardware's range check (bytes past the range read as 0; the rounding bytes of the range's first and
// last dword are never fetched from the block); the walk's loads, the re-walk's and the byte-load fallback's
// are plain reads of the block, so a read past the caller's bytes is an AddressSanitizer report.
// Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../uflow_amd/csrc/frame_codec_core.hpp"
#include "../../uflow_amd/csrc/frame_parse_plan.hpp"
#include "lane_orders.hpp"

namespace {

using namespace ufc_parse_plan;

long checks = 0;

void fail(const char* what, const char* name, long a, long b, long c) {
  std::printf("FAIL %s [%s] (%ld, %ld, %ld)\n", what, name, a, b, c);
  std::exit(1);
}

struct Lcg {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

// ---- frames ----
typedef std::vector<uint8_t> Frame;
struct Dg { uint32_t form, dl; };  // 0 micro (dl < 64), 1 small (dl < 256), 2 large

Frame data_frame(Lcg& r, const std::vector<Dg>& dgs) {
  Frame f{10, (uint8_t)r.next(), (uint8_t)r.next(), (uint8_t)r.next(), (uint8_t)r.next(),
          (uint8_t)((r.next() & 0x80) | dgs.size())};
  for (const Dg& d : dgs) {
    const uint32_t hs = d.form == 0 ? 6 : d.form == 1 ? 9 : 14;
    const size_t at = f.size();
    for (uint32_t k = 0; k < hs + d.dl; k++) f.push_back((uint8_t)r.next());
    if (d.form == 0) f[at] = (uint8_t)((f[at] & 0x40) | d.dl);
    if (d.form == 1) f[at] = (uint8_t)(0x80 | (f[at] & 0x3F)), f[at + 1] = (uint8_t)d.dl;
    if (d.form == 2) f[at] = (uint8_t)(0xC0 | (f[at] & 0x3F)), f[at + 1] = (uint8_t)(d.dl >> 8), f[at + 2] = (uint8_t)d.dl;
  }
  for (int k = 0; k < 4; k++) f.push_back((uint8_t)r.next());  // the trailer: the gate's verdict comes with the batch
  return f;
}
Frame micros(Lcg& r, uint32_t n, uint32_t dl = 0) { return data_frame(r, std::vector<Dg>(n, Dg{0, dl})); }
Frame ack_frame(Lcg& r, uint32_t groups) {
  Frame f{12};
  for (int k = 0; k < 8; k++) f.push_back((uint8_t)r.next());
  f.push_back((uint8_t)(groups >> 8)), f.push_back((uint8_t)groups);
  for (uint32_t k = 0; k < 9 * groups + 4; k++) f.push_back((uint8_t)r.next());
  return f;
}
Frame sync_frame(Lcg& r) {
  Frame f{11};
  for (int k = 0; k < 13; k++) f.push_back((uint8_t)r.next());
  return f;
}

// A batch: frames in the order of their indices; where each lies in the caller's buffer is the layout's business.
struct Batch {
  std::string name;
  std::vector<Frame> frames;
  std::vector<uint8_t> valid;
  void add(const Frame& f, bool ok = true) { frames.push_back(f), valid.push_back(ok ? 1 : 0); }
  // frames without items until the next frame sits on thread `at` of its workgroup
  void pad_to(Lcg& r, uint32_t at) {
    while (frames.size() % kParseThreads != at) filler(r);
  }
  void filler(Lcg& r) {
    switch (frames.size() % 4) {
      case 0: add(sync_frame(r)); break;
      case 1: add(micros(r, 3, 2), false); break;  // rejected by the gate
      case 2: add(micros(r, 0)); break;
      default: add(ack_frame(r, 0)); break;
    }
  }
};

// ---- the caller's bytes: blocks of exactly the bytes the call may read ----
struct Block {
  uint64_t lo, len;
  uint8_t* p;  // malloc(len): byte lo + k at p[k]
};
struct Memory {
  std::vector<Block> blocks;  // ascending lo
  uint64_t lead = 0;          // the buffer's byte address modulo 4
  ~Memory() { for (Block& b : blocks) std::free(b.p); }
  void add(uint64_t lo, const std::vector<uint8_t>& bytes) {
    Block b{lo, bytes.size(), (uint8_t*)std::malloc(bytes.size() ? bytes.size() : 1)};
    if (!bytes.empty()) std::memcpy(b.p, bytes.data(), bytes.size());
    blocks.push_back(b);
  }
  const Block& block_of(uint64_t off) const {
    size_t k = blocks.size() - 1;
    while (k > 0 && blocks[k].lo > off) k--;
    return blocks[k];
  }
  // a plain load of byte `off`: past its block's end the sanitizer reports it
  uint32_t byte(uint64_t off) const {
    const Block& b = block_of(off);
    return b.p[off - b.lo];
  }
  bool holds(uint64_t off) const {
    const Block& b = block_of(off);
    return off >= b.lo && off - b.lo < b.len;
  }
};

// The walk's and the re-walk's readers (frame_parse.hip DevBytesHead, DevBytes): the extents of their loads.
struct WalkBytes {
  const Memory* m;
  uint64_t a;
  uint32_t held;  // the frame's first 8 bytes come from one load when the frame has 8
  uint32_t operator()(uint32_t i) const { return m->byte(a + i); }
  uint32_t head3(uint32_t i) const {
    if (i + 3 <= held) return (*this)(i) | ((*this)(i + 1) << 8) | ((*this)(i + 2) << 16);
    const uint32_t v = (*this)(i) | ((*this)(i + 1) << 8) | ((*this)(i + 2) << 16) | ((*this)(i + 3) << 24);  // one dword load
    return v & 0xFFFFFFu;
  }
};

struct HostAdd {
  static uint32_t add(uint32_t* ctr) { return (*ctr)++; }
};

// ---- thread orders ----
enum Order { kForward = 0, kBackward = 1, kShuffled = 2 };
std::vector<uint32_t> order_of(Order o, uint32_t n) {
  std::vector<uint32_t> v(n);
  for (uint32_t k = 0; k < n; k++) v[k] = o == kBackward ? n - 1 - k : k;
  if (o == kShuffled)
    for (uint32_t k = n; k > 1; k--) std::swap(v[k - 1], v[lane_orders::ShuffledWave::draw() % k]);
  return v;
}

struct Result {
  std::vector<ufc_frame_info> infos;
  std::vector<ufc_item> items;  // cap entries, 0xA5 where nothing was stored
  uint64_t items_used = ~0ull;
  std::vector<uint8_t> modes;
  std::vector<uint32_t> pool_demand;  // per workgroup: pool entries asked for (with no frame giving up)
  long fallback_items = 0, exact_loads = 0, pair_loads = 0, rewalks = 0;
};

// One call of ufc_parse_batch_varlen as the kernels run it.
Result emulate(const Batch& b, const std::vector<uint64_t>& offsets, const Memory& mem, uint64_t items_cap, bool items_null,
               Order order) {
  const uint64_t n = b.frames.size();
  const uint32_t blocks = (uint32_t)((n + kParseThreads - 1) / kParseThreads);
  const uint64_t cap = items_null ? 0 : items_cap;  // (ufc_parse_batch_varlen: no item array, no room)
  Result R;
  R.infos.resize(n);
  R.modes.assign(n, 0xEE);
  R.pool_demand.assign(blocks, 0);
  std::vector<uint32_t> counts(n), wg_counts(blocks), wg_firsts(blocks), seg_base(blocks);
  const uint64_t scap = seg_cap(n, cap);
  uint16_t* pos_seg = (uint16_t*)std::malloc(scap * 2);  // exactly the call's slots
  unsigned long long cursor = 0;
  // (the item array: exactly cap records)
  ufc_item* items = items_null ? nullptr : (ufc_item*)std::malloc(cap ? cap * sizeof(ufc_item) : 1);
  if (items) std::memset(items, 0xA5, cap * sizeof(ufc_item));

  // ---- parse_walk_pool_kernel ----
  for (uint32_t blk : order_of(order, blocks)) {
    std::vector<uint16_t> slots(kInlineSlots * kParseThreads, 0xDEAD);
    std::vector<uint32_t> pool(kPoolSlots, 0xDEADDEADu);
    uint32_t pool_ctr = 0;
    uint32_t npos[kParseThreads] = {0}, head[kParseThreads], tail[kParseThreads], cnt_all[kParseThreads] = {0};
    bool full[kParseThreads] = {false};
    uint8_t mode[kParseThreads] = {0};
    for (uint32_t t : order_of(order, kParseThreads)) {
      head[t] = tail[t] = kPoolNil;
      const uint64_t i = (uint64_t)blk * kParseThreads + t;
      if (i >= n) continue;
      uint64_t a;
      const uint32_t len = frame_len32(offsets.data(), i, a);
      ufc_frame_info info;
      const WalkBytes rd{&mem, a, len >= 8 ? 8u : 0u};
      if (len >= 8) (void)rd(7);  // the head's 8-byte load
      const bool ok = ufc_codec::read_frame_to(
          rd, len, b.valid[i] != 0, info,
          PoolSink<HostAdd>{slots.data() + t, pool.data(), &pool_ctr, &head[t], &tail[t], &full[t]}, kPosSlots);
      const uint32_t cnt = ok ? info.item_count : 0u;
      if (cnt) {
        mode[t] = items_mode(info.kind == UFC_FRAME_ACK, cnt, len, full[t]);
        if (mode[t] == kItemsPos) npos[t] = cnt;
        if (info.kind == UFC_FRAME_DATA && cnt > kInlineSlots) R.pool_demand[blk] += (cnt < kPosSlots ? cnt : kPosSlots) - kInlineSlots;
      }
      info.item_first = 0;
      R.infos[i] = info;
      counts[i] = cnt;
      cnt_all[t] = cnt;
    }
    uint32_t lo[kParseThreads], total = 0, total_items = 0;
    for (uint32_t t = 0; t < (uint32_t)kParseThreads; t++) lo[t] = total, total += npos[t], total_items += cnt_all[t];
    wg_counts[blk] = total_items;
    const unsigned long long b64 = total ? cursor : 0ull;
    if (total) cursor += total;
    const uint32_t base = UFC_PARSE_SEG_NO_ROOM(b64, total, scap) ? kNoSegment : (uint32_t)b64;
    seg_base[blk] = base;
    for (uint32_t t : order_of(order, kParseThreads)) {
      const uint64_t i = (uint64_t)blk * kParseThreads + t;
      if (i < n) R.modes[i] = (mode[t] == kItemsPos && base == kNoSegment) ? (uint8_t)kItemsWalk : mode[t];
      if (base != kNoSegment) {
        uint16_t* seg = pos_seg + base;
        const uint32_t ni = npos[t] < kInlineSlots ? npos[t] : kInlineSlots;
        for (uint32_t k = 0; k < ni; k++) seg[lo[t] + k] = slots[k * kParseThreads + t];
        uint32_t idx = head[t];
        for (uint32_t k = kInlineSlots; k < npos[t]; k++) {
          if (idx >= kPoolSlots) fail("pool list runs out", b.name.c_str(), blk, t, k);
          const uint32_t v = pool[idx];
          seg[lo[t] + k] = (uint16_t)(v & 0xFFFFu);
          idx = v >> 16;
        }
      }
    }
  }
  // ---- the scan over the workgroups ----
  for (uint32_t blk = 0, s = 0; blk < blocks; blk++) wg_firsts[blk] = s, s += wg_counts[blk];

  // ---- parse_emit_kernel<1, 2> ----
  for (uint32_t blk : order_of(order, blocks)) {
    const uint64_t i0 = (uint64_t)blk * kParseThreads;
    const uint32_t nb = (uint32_t)(n - i0 < (uint64_t)kParseThreads ? n - i0 : kParseThreads);
    uint32_t lfirst[kParseThreads], lseg[kParseThreads], lend = 0xDEADBEEFu, cnt[kParseThreads] = {0};
    uint64_t lstart[kParseThreads];
    uint8_t lmode[kParseThreads];
    uint32_t lo = 0, sum = 0;
    for (uint32_t t = 0; t < (uint32_t)kParseThreads; t++) {  // (the scan)
      const uint64_t i = i0 + t;
      uint8_t mode = kItemsNone;
      uint64_t a = 0;
      if (i < n) cnt[t] = counts[i], mode = R.modes[i], a = offsets[i];
      lfirst[t] = wg_firsts[blk] + sum, lseg[t] = lo, lstart[t] = a, lmode[t] = mode;
      lo += mode == kItemsPos ? cnt[t] : 0u, sum += cnt[t];
    }
    for (uint32_t t : order_of(order, kParseThreads)) {
      const uint64_t i = i0 + t;
      if (i < n) {
        R.infos[i].item_first = lfirst[t];
        if (i == n - 1) R.items_used = (uint64_t)lfirst[t] + cnt[t];
      }
      if (t == nb - 1) lend = lfirst[t] + cnt[t];
    }
    const uint64_t span_lo = lstart[0], span_hi = offsets[i0 + nb];
    const uint64_t base_addr = mem.lead + span_lo;  // (the buffer's address modulo 4 is all the plan uses of it)
    const SpanRange sr = span_range(span_lo, span_hi, base_addr);
    // a buffer load's byte: past the range 0; the range's rounding bytes (before the span's first byte, behind its
    // last) share a dword with a span byte and are not fetched here
    auto buf_byte = [&](uint32_t off) -> uint32_t {
      if (off >= sr.range) return 0;
      if (off < sr.delta || off - sr.delta >= span_hi - span_lo) {
        if (off >= sr.delta && off - sr.delta >= span_hi - span_lo + 3) fail("range rounding", b.name.c_str(), blk, off, 0);
        return 0xCD;  // (whatever lies there: never part of a header)
      }
      return mem.byte(span_lo + (off - sr.delta));
    };
    auto buf_dword = [&](uint32_t off) -> uint32_t {
      return buf_byte(off) | (buf_byte(off + 1) << 8) | (buf_byte(off + 2) << 16) | (buf_byte(off + 3) << 24);
    };
    const uint32_t g0 = lfirst[0], g1 = lend;
    const uint32_t sb = seg_base[blk];
    const uint16_t* seg = pos_seg + (sb == kNoSegment ? 0u : sb);
    if (!items) continue;
    const uint64_t g_end = (uint64_t)g1 < cap ? g1 : cap;
    for (uint32_t t : order_of(order, kParseThreads)) {
      for (uint64_t gb = (uint64_t)g0 + t; gb < g_end; gb += kParseThreads) {
        const uint32_t f = owner_of([&](uint32_t m) -> uint32_t { return lfirst[m]; }, nb, (uint32_t)gb);
        const uint32_t k = (uint32_t)gb - lfirst[f];
        const uint8_t m = lmode[f];
        if (m != kItemsPos && m != kItemsAck) continue;
        if (k >= cnt[f]) fail("owner without the item", b.name.c_str(), blk, (long)gb, f);
        const uint32_t hoff = m == kItemsPos ? (uint32_t)seg[lseg[f] + k] : ack_hoff(k);
        uint32_t w[4] = {0, 0, 0, 0};
        if (sr.ok) {
          const uint32_t ex = fetch_ex(lstart[f], span_lo, sr.delta, hoff);
          uint32_t x[5];
          if (fetch_exact(ex, sr.range)) {  // one unaligned 16-byte load at the header
            for (int q = 0; q < 4; q++) x[q] = buf_dword(ex + 4 * q);
            x[4] = 0;
            for (int q = 0; q < 4; q++) w[q] = x[q];
            R.exact_loads++;
          } else {  // an aligned 16-byte load + one dword, shifted
            const uint32_t al = ex & ~3u, sh = ex & 3u;
            for (int q = 0; q < 5; q++) x[q] = buf_dword(al + 4 * q);
            for (int q = 0; q < 4; q++) w[q] = (uint32_t)((((uint64_t)x[q + 1] << 32) | x[q]) >> (8 * sh));
            R.pair_loads++;
          }
        } else {
          const uint64_t at = lstart[f] + hoff;
          w[0] = mem.byte(at);
          const uint32_t nbytes = fallback_bytes(m == kItemsAck, w[0]);
          for (uint32_t c = 1; c < nbytes; c++) w[c >> 2] |= mem.byte(at + c) << (8 * (c & 3));
          R.fallback_items++;
        }
        auto h = [&](uint32_t c) -> uint32_t { return (w[c >> 2] >> (8 * (c & 3))) & 0xFFu; };
        ufc_item it{};
        if (m == kItemsPos) {
          uint32_t hs, dl;
          ufc_codec::datagram_size(h, hs, dl);
          ufc_codec::decode_datagram(h, hs, it);
          it.data_offset = hoff + hs;
        } else {
          ufc_codec::decode_ack_group(h, it);
        }
        items[gb] = it;  // (gb < cap: the array holds exactly cap records)
      }
      // frames whose headers did not fit the slots: walked again, items stored directly
      const uint64_t i = i0 + t;
      if (i < n && lmode[t] == kItemsWalk && (uint64_t)lfirst[t] < cap) {
        uint64_t aa;
        const uint32_t len = frame_len32(offsets.data(), i, aa);
        const uint64_t left = cap - lfirst[t];
        const uint32_t room = (uint32_t)((uint64_t)cnt[t] < left ? cnt[t] : left);
        ufc_frame_info info;
        ufc_codec::read_frame_to(WalkBytes{&mem, aa, 0}, len, b.valid[i] != 0, info, ufc_codec::PtrSink{items + lfirst[t]}, room);
        R.rewalks++;
      }
    }
  }
  if (items) R.items.assign(items, items + cap);
  std::free(items);
  std::free(pos_seg);
  return R;
}

// ---- expected: the codec core's serial parse, frame by frame ----
struct VecBytes {
  const uint8_t* p;
  uint32_t operator()(uint32_t i) const { return p[i]; }
  uint32_t head3(uint32_t i) const { return p[i] | (p[i + 1] << 8) | (p[i + 2] << 16); }
};
void expected(const Batch& b, const std::vector<uint32_t>& lens, std::vector<ufc_frame_info>& infos, std::vector<ufc_item>& items) {
  infos.resize(b.frames.size());
  items.clear();
  for (size_t i = 0; i < b.frames.size(); i++) {
    const Frame& f = b.frames[i];
    std::vector<ufc_item> own(f.size() / 6 + 1);
    std::memset(own.data(), 0, own.size() * sizeof(ufc_item));
    ufc_codec::read_frame(VecBytes{f.data()}, lens[i], b.valid[i] != 0, infos[i], own.data(), (uint32_t)own.size());
    infos[i].item_first = (uint32_t)items.size();
    items.insert(items.end(), own.begin(), own.begin() + infos[i].item_count);
  }
}

bool same_item(const ufc_item& a, const ufc_item& b) { return std::memcmp(&a, &b, sizeof(ufc_item)) == 0; }
bool same_info(const ufc_frame_info& a, const ufc_frame_info& b) {
  return a.kind == b.kind && a.ok == b.ok && a.aux == b.aux && a.crc_ok == b.crc_ok && a.item_count == b.item_count &&
         a.item_first == b.item_first && std::memcmp(a.f, b.f, sizeof(a.f)) == 0;
}

// What a case says of itself, asserted on the serial parse's records and the emulation's counters.
struct Facts {
  long total_items = -1;                 // the batch's items
  long wg_items[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // items of workgroups 0..7
  long pool_demand = -1;                 // largest pool demand of a workgroup
  long walk_frames = -1;                 // frames walked again in the uncapped run (-1: depends on the order)
  long min_fallback = 0;                 // at least this many items through the byte loads
  long pair_loads = -1;                  // headers fetched with the aligned pair (not the one exact 16-byte load)
  bool pool_overflows = false;           // some frame finds the pool full: which one depends on the order
};

// layout: where frame i lies.  kPacked: one block of exactly the frames' bytes, in order.
struct Layout {
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> lens;
  Memory mem;
};
void packed(const Batch& b, uint32_t lead, Layout& L) {
  std::vector<uint8_t> all;
  L.offsets.assign(1, 0);
  for (const Frame& f : b.frames) {
    all.insert(all.end(), f.begin(), f.end());
    L.offsets.push_back(all.size());
    L.lens.push_back((uint32_t)f.size());
  }
  L.mem.lead = lead;
  L.mem.add(0, all);
}

void run_case(const Batch& b, Layout& L, const Facts& facts, const std::vector<uint64_t>& caps, bool null_items) {
  const uint64_t n = b.frames.size();
  std::vector<ufc_frame_info> e_infos;
  std::vector<ufc_item> e_items;
  expected(b, L.lens, e_infos, e_items);
  // facts first: a generator that drifted stops here
  if (facts.total_items >= 0 && (long)e_items.size() != facts.total_items)
    fail("fact: total items", b.name.c_str(), (long)e_items.size(), facts.total_items, 0);
  for (uint32_t w = 0; w < 8; w++)
    if (facts.wg_items[w] >= 0) {
      long s = 0;
      for (uint64_t i = (uint64_t)w * kParseThreads; i < n && i < (uint64_t)(w + 1) * kParseThreads; i++) s += e_infos[i].item_count;
      if (s != facts.wg_items[w]) fail("fact: workgroup items", b.name.c_str(), w, s, facts.wg_items[w]);
    }
  Result first_run;
  for (int o = 0; o < 3; o++) {
    const Result R = emulate(b, L.offsets, L.mem, e_items.size() + 7, false, (Order)o);
    if (R.items_used != e_items.size()) fail("items_used", b.name.c_str(), o, (long)R.items_used, (long)e_items.size());
    for (uint64_t i = 0; i < n; i++, checks++)
      if (!same_info(R.infos[i], e_infos[i])) fail("info", b.name.c_str(), o, (long)i, R.infos[i].item_first);
    for (uint64_t g = 0; g < e_items.size(); g++, checks++)
      if (!same_item(R.items[g], e_items[g])) fail("item", b.name.c_str(), o, (long)g, 0);
    for (uint64_t g = e_items.size(); g < R.items.size(); g++)
      for (size_t k = 0; k < sizeof(ufc_item); k++)
        if (((const uint8_t*)&R.items[g])[k] != 0xA5) fail("store past the items", b.name.c_str(), o, (long)g, 0);
    long demand = 0;
    for (uint32_t d : R.pool_demand) demand = d > demand ? d : demand;
    if (facts.pool_demand >= 0 && demand != facts.pool_demand) fail("fact: pool demand", b.name.c_str(), o, demand, facts.pool_demand);
    if (facts.walk_frames >= 0 && R.rewalks != facts.walk_frames) fail("fact: frames walked again", b.name.c_str(), o, R.rewalks, facts.walk_frames);
    if ((R.rewalks > 0) != (facts.walk_frames != 0)) fail("fact: re-walk", b.name.c_str(), o, R.rewalks, 0);
    if (R.fallback_items < facts.min_fallback) fail("fact: byte-load items", b.name.c_str(), o, R.fallback_items, facts.min_fallback);
    if (facts.pair_loads >= 0 && R.pair_loads != facts.pair_loads) fail("fact: pair loads", b.name.c_str(), o, R.pair_loads, facts.pair_loads);
    if (o == 0) first_run = R;
    if (!facts.pool_overflows && R.modes != first_run.modes) fail("modes differ between orders", b.name.c_str(), o, 0, 0);
  }
  // caps: infos and items_used as uncapped, items below the cap, nothing stored from the cap on (the item array
  // holds exactly cap records)
  for (size_t c = 0; c <= caps.size(); c++) {
    const bool null_run = c == caps.size();
    if (null_run && !null_items) break;
    const uint64_t cap = null_run ? 5 : caps[c];
    for (int o = 0; o < 3; o++) {
      const Result R = emulate(b, L.offsets, L.mem, cap, null_run, (Order)o);
      if (R.items_used != e_items.size()) fail("capped items_used", b.name.c_str(), o, (long)cap, (long)R.items_used);
      for (uint64_t i = 0; i < n; i++, checks++)
        if (!same_info(R.infos[i], e_infos[i])) fail("capped info", b.name.c_str(), o, (long)cap, (long)i);
      for (uint64_t g = 0; g < R.items.size(); g++, checks++)
        if (g < e_items.size() ? !same_item(R.items[g], e_items[g]) : false) fail("capped item", b.name.c_str(), o, (long)cap, (long)g);
    }
  }
}

void run_packed(const Batch& b, const Facts& facts, const std::vector<uint64_t>& caps = {}, bool null_items = false) {
  for (uint32_t lead : {0u, 3u}) {
    Layout L;
    packed(b, lead, L);
    run_case(b, L, facts, caps, null_items);
  }
}

Batch named(const char* name) {
  Batch b;
  b.name = name;
  return b;
}

// ---- the cases (tests/parse_expect.py lane_cases, the same numbers) ----
void lone_owners(Lcg& r) {
  {
    Batch b = named("only_frame_0");
    b.add(micros(r, 5, 1));
    b.pad_to(r, 0);
    Facts f;
    f.total_items = 5, f.wg_items[0] = 5, f.walk_frames = 0;
    run_packed(b, f);
  }
  {
    Batch b = named("only_frame_255");
    b.pad_to(r, 255);
    b.add(ack_frame(r, 3));
    Facts f;
    f.total_items = 3, f.wg_items[0] = 3, f.walk_frames = 0;
    run_packed(b, f);
  }
  {
    Batch b = named("frames_0_and_255");
    b.add(micros(r, 2));
    for (int k = 0; k < 254; k++) b.filler(r);
    b.add(micros(r, 4, 3));
    Facts f;
    f.total_items = 6, f.wg_items[0] = 6, f.walk_frames = 0;
    run_packed(b, f);
  }
}

void empty_workgroups_and_ends(Lcg& r) {
  {
    Batch b = named("empty_workgroup_between");
    for (int k = 0; k < 256; k++) b.add(micros(r, 1 + k % 3));
    for (int k = 0; k < 256; k++) b.filler(r);
    for (int k = 0; k < 256; k++) b.add(k % 2 ? ack_frame(r, 2) : micros(r, 1));
    Facts f;
    f.wg_items[0] = 86 * 1 + 85 * 2 + 85 * 3, f.wg_items[1] = 0, f.wg_items[2] = 128 * 3, f.walk_frames = 0;
    run_packed(b, f);
  }
  {
    Batch b = named("last_workgroup_empty");
    for (int k = 0; k < 256; k++) b.add(micros(r, 2));
    for (int k = 0; k < 100; k++) b.filler(r);
    Facts f;
    f.total_items = 512, f.wg_items[0] = 512, f.wg_items[1] = 0, f.walk_frames = 0;
    run_packed(b, f);
  }
  {
    Batch b = named("last_frame_empty");
    for (int k = 0; k < 299; k++) b.add(micros(r, 1 + k % 2));
    b.add(micros(r, 0));
    Facts f;
    f.total_items = 150 * 1 + 149 * 2, f.walk_frames = 0;
    run_packed(b, f);
  }
  {
    Batch b = named("last_frame_alone");
    for (int k = 0; k < 256; k++) b.add(k % 5 ? micros(r, 1) : sync_frame(r));
    b.add(micros(r, 7, 1));
    Facts f;
    f.wg_items[0] = 204, f.wg_items[1] = 7, f.total_items = 211, f.walk_frames = 0;
    run_packed(b, f);
  }
}

// A batch without a single item (items_used is written by the batch's last frame, whatever it holds), and a
// header that ends exactly with its workgroup's range: the one exact 16-byte load still takes it.
void no_items_and_range_end(Lcg& r) {
  {
    Batch b = named("no_items_at_all");
    for (int k = 0; k < 300; k++) b.filler(r);
    Facts f;
    f.total_items = 0, f.walk_frames = 0;
    run_packed(b, f, {0, 1}, true);
  }
  {
    Batch b = named("header_16_before_span_end");
    b.add(micros(r, 1, 2));  // 18 bytes
    b.add(micros(r, 1, 6));  // 22 bytes: header, 6 bytes, trailer = the span's last 16 bytes
    Facts f;
    f.total_items = 2, f.walk_frames = 0, f.pair_loads = 0;
    run_packed(b, f);
  }
}

void items_in_workgroup(Lcg& r) {
  for (uint32_t want : {255u, 256u, 257u, 513u}) {
    {
      Batch b = named("items_in_workgroup[small]");
      b.name += std::to_string(want);
      // many small frames: 1..3 micro datagrams each (2..4 for 513) until the count is reached, the rest of the
      // workgroup empty
      uint32_t have = 0;
      const uint32_t least = want > 300 ? 2 : 1;
      while (have < want) {
        const uint32_t c = want - have < least + 2 ? want - have : least + (uint32_t)b.frames.size() % 3;
        b.add(micros(r, c, 1));
        have += c;
      }
      b.pad_to(r, 0);
      b.add(micros(r, 2));  // the next workgroup starts behind them
      Facts f;
      f.wg_items[0] = want, f.wg_items[1] = 2, f.walk_frames = 0;
      run_packed(b, f);
    }
    {
      Batch b = named("items_in_workgroup[ack]");
      b.name += std::to_string(want);
      for (int k = 0; k < 100; k++) b.filler(r);
      b.add(ack_frame(r, want));  // one frame owning every round
      b.pad_to(r, 0);
      b.add(ack_frame(r, 1));
      Facts f;
      f.wg_items[0] = want, f.wg_items[1] = 1, f.walk_frames = 0;
      run_packed(b, f);
    }
  }
  {
    Batch b = named("ack_groups_65535");
    b.add(sync_frame(r));
    b.add(ack_frame(r, 65535));
    if (b.frames[1].size() != 589830) fail("fact: frame bytes", b.name.c_str(), (long)b.frames[1].size(), 0, 0);
    b.add(micros(r, 1));
    Facts f;
    f.total_items = 65536, f.walk_frames = 0;
    run_packed(b, f);
  }
}

void slot_boundaries(Lcg& r) {
  for (uint32_t k : {16u, 17u, 64u, 65u}) {
    Batch b = named("slots");
    b.name += std::to_string(k);
    for (uint32_t at : {0u, 77u, 255u}) {
      b.pad_to(r, at);
      b.add(micros(r, k, at % 3));
    }
    Facts f;
    f.total_items = 3 * k, f.walk_frames = k > kPosSlots ? 3 : 0;
    f.pool_demand = 3 * (k <= kInlineSlots ? 0 : k > kPosSlots ? (long)(kPosSlots - kInlineSlots) : (long)(k - kInlineSlots));
    run_packed(b, f);
  }
}

void pool_limits(Lcg& r) {
  {
    Batch b = named("pool_exact");
    for (int k = 0; k < 256; k++) b.add(k % 2 ? micros(r, 32) : micros(r, k % 17));
    Facts f;
    f.pool_demand = 2048, f.walk_frames = 0;
    run_packed(b, f);
  }
  {
    Batch b = named("pool_plus_one");
    for (int k = 0; k < 256; k++) b.add(k % 2 ? micros(r, 32) : micros(r, k == 100 ? 17 : k % 17));
    Facts f;
    f.pool_demand = 2049, f.walk_frames = 1, f.pool_overflows = true;
    run_packed(b, f);
  }
  {
    Batch b = named("pool_all_want_48");
    for (int k = 0; k < 256; k++) b.add(micros(r, 64));
    Facts f;
    f.pool_demand = 256 * 48, f.pool_overflows = true;  // (how many frames give up depends on the order)
    run_packed(b, f);
  }
}

void u16_limit(Lcg& r) {
  for (uint32_t len : {65535u, 65536u}) {
    Batch b = named("len_");
    b.name += std::to_string(len);
    b.add(micros(r, 1));
    // one large datagram and a trailing micro with no payload: 6 + (14 + dl) + 6 + 4 bytes
    b.add(data_frame(r, {Dg{2, len - 30}, Dg{0, 0}}));
    if (b.frames[1].size() != len) fail("fact: frame bytes", b.name.c_str(), (long)b.frames[1].size(), len, 0);
    b.add(micros(r, 2));
    Facts f;
    f.total_items = 5, f.walk_frames = len > 65535 ? 1 : 0;
    run_packed(b, f);
  }
}

// slot, ack, re-walked and empty frames on adjacent threads; a re-walked frame on thread 0 of workgroup 1 and on
// thread 255 of workgroup 0
Batch mode_mix(Lcg& r) {
  Batch b = named("mode_mix");
  for (int k = 0; k < 255; k++) {
    switch (k % 4) {
      case 0: b.add(micros(r, 3, 1)); break;
      case 1: b.add(ack_frame(r, 2)); break;
      case 2: b.add(micros(r, 70)); break;
      default: b.filler(r); break;
    }
  }
  b.add(micros(r, 66));  // thread 255
  b.add(micros(r, 65));  // thread 0 of workgroup 1
  for (int k = 0; k < 40; k++) b.add(k % 2 ? micros(r, 20, 2) : ack_frame(r, 5));
  return b;
}

void mode_mix_and_caps(Lcg& r) {
  const Batch b = mode_mix(r);
  Facts f;
  // workgroup 0: threads 0..254: 64 x 3, 64 x 2, 64 x 70 (k % 4 == 2: k = 2..254 -> 64 frames), + 66
  f.wg_items[0] = 64 * 3 + 64 * 2 + 64 * 70 + 66;
  f.wg_items[1] = 65 + 20 * 20 + 20 * 5;
  f.walk_frames = 64 + 1 + 1;
  const uint64_t wg1 = (uint64_t)f.wg_items[0], total = wg1 + (uint64_t)f.wg_items[1];
  // 0, 1, workgroup 1's first item, inside a slot frame (frame 0 holds items 0..2), inside a re-walked frame
  // (frame 2 holds items 5..74; frame 256 holds wg1 .. wg1 + 64), exactly the total
  run_packed(b, f, {0, 1, wg1, 2, 40, wg1 + 30, wg1 + 65 + 7, total}, true);
}

// Workgroup 0's frames lie behind workgroup 1's in the buffer: offsets[256] < offsets[0], frame 255 gets length 0,
// and workgroup 0's 255 frames take the byte loads.  The buffer's used bytes end with frame 254: a micro datagram
// with no payload in front of its trailer.
void fallback_backward_offsets(Lcg& r) {
  Batch b = named("fallback_backward_offsets");
  for (int k = 0; k < 254; k++) {
    switch (k % 5) {
      case 0: b.add(data_frame(r, {Dg{0, 3}, Dg{1, 70}, Dg{2, 300}})); break;
      case 1: b.add(ack_frame(r, 1 + k % 4)); break;
      case 2: b.add(data_frame(r, {Dg{2, 0}, Dg{1, 0}, Dg{0, 0}})); break;
      case 3: b.add(micros(r, 70)); break;  // re-walked
      default: b.filler(r); break;
    }
  }
  b.add(data_frame(r, {Dg{1, 5}, Dg{0, 0}}));  // frame 254: ends the buffer
  b.add(Frame{});                              // frame 255: length 0 by frame_len32
  for (int k = 0; k < 60; k++) b.add(k % 2 ? micros(r, 2, 1) : ack_frame(r, 2));
  Layout L;
  std::vector<uint8_t> all;
  std::vector<uint64_t> off(b.frames.size() + 1);
  for (size_t i = 256; i < b.frames.size(); i++) {  // workgroup 1 first
    off[i] = all.size();
    all.insert(all.end(), b.frames[i].begin(), b.frames[i].end());
  }
  off[b.frames.size()] = all.size();
  for (size_t i = 0; i < 255; i++) {
    off[i] = all.size();
    all.insert(all.end(), b.frames[i].begin(), b.frames[i].end());
  }
  off[255] = all.size();
  if (!(off[256] < off[0]) || off[256] != 0) fail("fact: offsets go backwards", b.name.c_str(), 0, 0, 0);
  L.offsets = off;
  for (const Frame& f : b.frames) L.lens.push_back((uint32_t)f.size());
  for (uint32_t lead : {0u, 3u}) {
    Layout M;
    M.offsets = L.offsets, M.lens = L.lens;
    M.mem.lead = lead;
    M.mem.add(0, all);
    Facts f;
    f.min_fallback = 51 * 3 + 51 * 3 + 2 + 50;  // (at least the data frames' datagrams)
    f.walk_frames = 51;
    run_case(b, M, f, {}, false);
  }
}

// A workgroup whose span reaches 4 GiB: a hundred frames at the buffer's start, one 4-GiB "frame" that the gate
// rejected, a hundred frames at its end.  Only the two ends exist.
void fallback_span_4gib(Lcg& r) {
  Batch b = named("fallback_span_4gib");
  std::vector<uint8_t> front, back;
  std::vector<uint64_t> off;
  Layout L;
  for (int k = 0; k < 100; k++) {
    b.add(k % 3 == 0 ? ack_frame(r, 1 + k % 3) : k % 3 == 1 ? data_frame(r, {Dg{0, 0}, Dg{2, 20}, Dg{0, 0}}) : micros(r, 66));
    off.push_back(front.size());
    front.insert(front.end(), b.frames.back().begin(), b.frames.back().end());
    L.lens.push_back((uint32_t)b.frames.back().size());
  }
  // the gap: the gate rejected it, so the walk reads its first 8 bytes (the head) and no more; the caller's
  // buffer goes on there, so the front block holds 16 of its bytes
  b.add(Frame(16, 0x5A), false);
  off.push_back(front.size());
  front.insert(front.end(), 16, 0x5A);
  L.lens.push_back(16);
  const uint64_t far = (1ull << 32) + 4096;
  for (int k = 0; k < 100; k++) {
    b.add(k % 2 ? data_frame(r, {Dg{1, 9}, Dg{0, 0}}) : ack_frame(r, 2));
    off.push_back(far + back.size());
    back.insert(back.end(), b.frames.back().begin(), b.frames.back().end());
    L.lens.push_back((uint32_t)b.frames.back().size());
  }
  off.push_back(far + back.size());
  L.offsets = off;
  L.mem.lead = 1;
  L.mem.add(0, front);
  L.mem.add(far, back);
  Facts f;
  f.walk_frames = 33;
  f.min_fallback = 34 + 33 * 3 + 50 * 2 + 50 * 2;
  run_case(b, L, f, {}, false);
}

}  // namespace

int main(int argc, char** argv) {
  Lcg r{20260101};
  const std::string only = argc > 1 ? argv[1] : "";
  auto want = [&](const char* group) { return only.empty() || only == group; };
  if (want("lone")) lone_owners(r);
  if (want("ends")) empty_workgroups_and_ends(r);
  if (want("ends")) no_items_and_range_end(r);
  if (want("rounds")) items_in_workgroup(r);
  if (want("slots")) slot_boundaries(r);
  if (want("pool")) pool_limits(r);
  if (want("u16")) u16_limit(r);
  if (want("mix")) mode_mix_and_caps(r);
  if (want("backward")) fallback_backward_offsets(r);
  if (want("span")) fallback_span_4gib(r);
  std::printf("ok: %ld checks\n", checks);
  return 0;
}
