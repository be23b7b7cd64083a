// The encode core of the batched build (uflow_amd/csrc/frame_codec_core.hpp: datagram_header_size,
// encode_datagram_header, encode_ack_group, encode_frame_head, check_frame, packed_byte) as host code under
// AddressSanitizer and UBSan: swept over the header-form boundaries of build.rs:81-122 and the count limits,
// each result compared with a byte-wise restatement written here (arrays and plain stores, no packed
// words).  Then the GPU write's own piece assembly (frame_build_piece.hpp: span owners, frame and item
// searches, assemble_piece), run piece by piece on the host over seeded batches at every alignment of the
// output and the payload, into buffers of exactly the bytes the call may touch, against a sequential
// writer built from the restatement.  Prints "ok: <checks>" and exits 0; any difference or sanitizer report stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../uflow_amd/csrc/frame_build_piece.hpp"
#include "../../uflow_amd/csrc/frame_codec_core.hpp"

namespace {

long checks = 0;

void fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  std::exit(1);
}

void be32(uint8_t* p, uint32_t v) { p[0] = v >> 24, p[1] = v >> 16, p[2] = v >> 8, p[3] = v; }
void be16(uint8_t* p, uint32_t v) { p[0] = v >> 8, p[1] = v; }

// build.rs:81-143, byte by byte.
uint32_t ref_datagram_header(const ufc_item& d, uint8_t* h) {
  const uint32_t dl = d.data_len, ch = d.channel_id, seq = d.id;
  if (d.fragment_id_last == 0 && dl < 64 && d.window_parent_lead < 128 && d.channel_parent_lead < 256) {
    h[0] = (uint8_t)(dl | ((ch & 0x10) << 2));
    h[1] = (uint8_t)(((seq >> 12) & 0xF0) | (ch & 0x0F));
    h[2] = (uint8_t)(seq >> 8);
    h[3] = (uint8_t)seq;
    h[4] = (uint8_t)(d.window_parent_lead | ((ch & 0x20) << 2));
    h[5] = (uint8_t)d.channel_parent_lead;
    return 6;
  }
  if (d.fragment_id_last == 0 && dl < 256) {
    h[0] = (uint8_t)(ch | 0x80);
    h[1] = (uint8_t)dl;
    h[2] = (uint8_t)(seq >> 16), h[3] = (uint8_t)(seq >> 8), h[4] = (uint8_t)seq;
    be16(h + 5, d.window_parent_lead);
    be16(h + 7, d.channel_parent_lead);
    return 9;
  }
  h[0] = (uint8_t)(ch | 0xC0);
  be16(h + 1, dl);
  h[3] = (uint8_t)(seq >> 16), h[4] = (uint8_t)(seq >> 8), h[5] = (uint8_t)seq;
  be16(h + 6, d.window_parent_lead);
  be16(h + 8, d.channel_parent_lead);
  be16(h + 10, d.fragment_id);
  be16(h + 12, d.fragment_id_last);
  return 14;
}

// serial/mod.rs:437-657 and the builders' frame headers, byte by byte.
uint32_t ref_frame_head(const ufc_frame_info& in, uint8_t* h) {
  h[0] = in.kind;
  switch (in.kind) {
    case UFC_FRAME_HANDSHAKE_SYN:
      h[1] = in.aux;
      for (int i = 0; i < 4; i++) be32(h + 2 + 4 * i, in.f[i]);
      return 18;
    case UFC_FRAME_HANDSHAKE_SYN_ACK:
      for (int i = 0; i < 5; i++) be32(h + 1 + 4 * i, in.f[i]);
      return 21;
    case UFC_FRAME_HANDSHAKE_ACK: be32(h + 1, in.f[0]); return 5;
    case UFC_FRAME_HANDSHAKE_ERROR: be32(h + 1, in.f[0]); h[5] = in.aux; return 6;
    case UFC_FRAME_DATA: be32(h + 1, in.f[0]); h[5] = (uint8_t)((in.aux << 7) | in.item_count); return 6;
    case UFC_FRAME_SYNC:
      h[1] = in.aux;
      be32(h + 2, (in.aux & 1) ? in.f[0] : 0);
      be32(h + 6, (in.aux & 2) ? in.f[1] : 0);
      return 10;
    case UFC_FRAME_ACK: be32(h + 1, in.f[0]); be32(h + 5, in.f[1]); be16(h + 9, in.item_count); return 11;
    default: return 1;
  }
}

void unpack(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t n, uint8_t* out) {
  for (uint32_t j = 0; j < n; j++) out[j] = (uint8_t)ufc_codec::packed_byte(w0, w1, w2, j);
}


// ---- the write's piece assembly, emulated workgroup by workgroup ----
struct Lcg {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  uint32_t below(uint32_t n) { return next() % n; }
};

struct HostBatch {
  std::vector<ufc_frame_info> infos;
  std::vector<ufc_item> items;
  std::vector<uint64_t> src_base;
  std::vector<uint8_t> payload;
};

// Frames of every kind; datagrams of 0..40 bytes (every piece boundary position), some long ones; rejected
// frames (ok = 0, bad fields, bad sources) singly, in runs, first and last.
HostBatch make_batch(uint32_t seed, uint32_t nframes, uint32_t shift) {
  Lcg r{seed};
  HostBatch b;
  b.payload.resize(shift);
  for (uint32_t i = 0; i < nframes; i++) {
    ufc_frame_info in{};
    const uint8_t kinds[] = {10, 10, 10, 12, 11, 0, 1, 2, 3, 4, 5, 10};
    in.kind = kinds[r.below(12)];
    in.ok = 1;
    for (int k = 0; k < 5; k++) in.f[k] = r.next() * 2654435761u;
    in.aux = in.kind == 0 ? (uint8_t)r.below(256) : in.kind == 11 ? (uint8_t)r.below(4) : in.kind == 3 ? (uint8_t)r.below(3)
                                                                                                      : (uint8_t)r.below(2);
    in.item_first = (uint32_t)b.items.size();
    b.src_base.push_back(b.payload.size());
    if (in.kind == 10) {
      const uint32_t shape = r.below(8);
      in.item_count = shape == 0 ? 65 + r.below(63) : shape == 1 ? 0 : 1 + r.below(12);
      uint32_t off = 0;
      for (uint32_t k = 0; k < in.item_count; k++) {
        ufc_item d{};
        d.id = r.below(1u << 20), d.channel_id = (uint8_t)r.below(64);
        const uint32_t t = r.below(3);
        d.window_parent_lead = (uint16_t)(t == 0 ? r.below(128) : r.below(65536));
        d.channel_parent_lead = (uint16_t)(t == 0 ? r.below(256) : r.below(65536));
        d.fragment_id = (uint16_t)(t == 2 ? r.below(65536) : r.below(2) * 7);
        d.fragment_id_last = (uint16_t)(t == 2 ? 1 + r.below(65535) : 0);
        d.data_len = shape == 0 ? r.below(3) : (r.below(40) == 0 ? 200 + r.below(20000) : r.below(41));
        d.data_offset = off + r.below(5);
        off = d.data_offset + d.data_len;
        b.items.push_back(d);
      }
      for (uint32_t k = 0; k < off; k++) b.payload.push_back((uint8_t)r.next());
    } else if (in.kind == 12) {
      in.item_count = r.below(4) == 0 ? 162 : r.below(20);
      for (uint32_t k = 0; k < in.item_count; k++) {
        ufc_item g{};
        g.id = r.next() * 2654435761u, g.data_offset = r.next() * 40503u, g.channel_id = (uint8_t)r.below(3), g.form = 3;
        b.items.push_back(g);
      }
    }
    // rejected frames: the first, the last, singles and runs
    const bool run = (i / 7) % 5 == 3;
    if (i == 0 || i + 1 == nframes || run || r.below(9) == 0) {
      const uint32_t how = r.below(3);
      if (how == 0) in.ok = 0;
      else if (how == 1) in.kind = 9;
      else if (in.kind == 10 && in.item_count) b.src_base.back() = b.payload.size() + 1;  // a range past the payload's end
      else in.ok = 0;
    }
    b.infos.push_back(in);
  }
  return b;
}

// The frame, byte by byte, from the restatement.
void ref_write_frame(const HostBatch& b, size_t i, std::vector<uint8_t>& out) {
  const ufc_frame_info& in = b.infos[i];
  uint8_t h[24] = {0};
  const uint32_t hn = ref_frame_head(in, h);
  out.insert(out.end(), h, h + hn);
  if (in.kind == 10) {
    for (uint32_t k = 0; k < in.item_count; k++) {
      const ufc_item& d = b.items[in.item_first + k];
      uint8_t dh[14];
      const uint32_t hs = ref_datagram_header(d, dh);
      out.insert(out.end(), dh, dh + hs);
      const uint8_t* src = b.payload.data() + b.src_base[i] + d.data_offset;
      out.insert(out.end(), src, src + d.data_len);
    }
  } else if (in.kind == 12) {
    for (uint32_t k = 0; k < in.item_count; k++) {
      const ufc_item& g = b.items[in.item_first + k];
      uint8_t gh[9];
      be32(gh, g.id), be32(gh + 4, g.data_offset), gh[8] = g.channel_id ? 1 : 0;
      out.insert(out.end(), gh, gh + 9);
    }
  } else if (in.kind == 0) {
    out.insert(out.end(), 1468 - hn, 0);
  }
  out.insert(out.end(), 4, 0);  // the write leaves the trailer zero
}

// What a write call's workgroups did with their tables.
struct WriteStats {
  long spans = 0, frames_staged = 0, items_staged = 0, max_nf = 0, max_window = 0;
};
WriteStats last_write;

// One write call as the kernels run it: item destinations, flags and span owners, then every piece of
// every workgroup span, each workgroup with its LDS tables where the kernel stages them (arrays of the kernel's
// sizes on the heap, poisoned where no thread stored: a read of an entry that was not staged shows as a wrong
// byte, an index past a table as a sanitizer report).  out_bytes = buf + lead with exactly out_len bytes behind it.
void emulate_write(const HostBatch& b, const std::vector<uint64_t>& off, uint8_t* out_bytes, uint64_t out_len,
                   const uint8_t* payload, uint64_t payload_len) {
  using namespace ufc_dev;
  const uint64_t n = b.infos.size(), n_items = b.items.size();
  std::vector<uint64_t> dst(n_items + 1, 0);
  for (uint64_t g = 0; g < n_items; g++) dst[g + 1] = dst[g] + ufc_codec::datagram_encoded_size(b.items[g]);
  const uint64_t spans = write_spans(out_len);
  std::vector<uint8_t> flags(n);
  std::vector<uint32_t> owner(spans + 1, 0xFFFFFFFFu);
  BuildArgs a{b.infos.data(), b.items.data(), n_items, b.src_base.data(), payload, payload_len, n,
              const_cast<uint64_t*>(off.data()), nullptr, out_bytes, out_len};
  const uint64_t base = (uint64_t)(uintptr_t)out_bytes;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t size;
    const uint8_t st = ufc_codec::check_frame(b.infos[i], b.items.data(), n_items, b.src_base[i], payload_len, size);
    flags[i] = ufc_codec::span_matches(st, size, off[i], off[i + 1], off[0], off[n], out_len) ? 1 : 0;
    note_span_owner(base, off[0], off[i], off[i + 1], (uint32_t)i, owner.data(), spans);
  }
  const uint64_t lo = off[0], hi = off[n] < out_len ? off[n] : out_len;
  last_write = WriteStats{};
  if (hi <= lo) return;
  const uint64_t addr_lo = base + lo, addr_hi = base + hi;
  for (uint64_t blk = 0; blk < spans; blk++) {
    const uint64_t span0 = first_span_addr(addr_lo) + blk * kSpanBytes;
    if (span0 >= addr_hi) continue;
    const uint64_t span1 = span0 + kSpanBytes;
    if (owner[blk] == 0xFFFFFFFFu) fail("span owner missing", (long)blk, 0, 0);
    const uint32_t f_a = owner[blk] < n - 1 ? owner[blk] : (uint32_t)n - 1;
    uint32_t f_b = (uint32_t)n - 1;
    if (span1 < addr_hi) {
      if (owner[blk + 1] == 0xFFFFFFFFu) fail("next span owner missing", (long)blk, 0, 0);
      f_b = owner[blk + 1] < n - 1 ? owner[blk + 1] : (uint32_t)n - 1;
      if (f_b < f_a) f_b = f_a;
    }
    // the workgroup's tables (frame_build.hip build_write_kernel)
    const uint32_t nf = f_b - f_a + 1;
    const bool staged = UFC_BUILD_FRAMES_STAGED(nf);
    uint64_t* tab = (uint64_t*)std::malloc((kTabFrames + 1) * sizeof(uint64_t));
    ufc_frame_info* sinfo = (ufc_frame_info*)std::malloc(kTabFrames * sizeof(ufc_frame_info));
    uint8_t* sflag = (uint8_t*)std::malloc(kTabFrames);
    uint64_t* sdst = (uint64_t*)std::malloc((kTabItems + 1) * sizeof(uint64_t));
    std::memset(tab, 0xEE, (kTabFrames + 1) * sizeof(uint64_t));
    std::memset(sinfo, 0xEE, kTabFrames * sizeof(ufc_frame_info));
    std::memset(sflag, 0xEE, kTabFrames);
    std::memset(sdst, 0xEE, (kTabItems + 1) * sizeof(uint64_t));
    uint32_t item_lo = 0xFFFFFFFFu, item_hi = 0;
    if (staged) {
      for (uint32_t j = 0; j <= nf; j++) tab[j] = off[f_a + j];
      for (uint32_t j = 0; j < nf; j++) {
        const ufc_frame_info info = b.infos[f_a + j];
        const uint8_t fl = flags[f_a + j];
        sinfo[j] = info;
        sflag[j] = fl;
        if (fl && info.kind == UFC_FRAME_DATA && info.item_count) {
          if (info.item_first < item_lo) item_lo = info.item_first;
          if (info.item_first + info.item_count > item_hi) item_hi = info.item_first + info.item_count;
        }
      }
    }
    const bool items_staged = UFC_BUILD_ITEMS_STAGED(staged, item_lo, item_hi);
    if (items_staged)
      for (uint32_t j = 0; j <= item_hi - item_lo; j++) sdst[j] = dst[item_lo + j];
    const SpanTables tb{tab, sinfo, sflag, sdst, GlobalTables{off.data(), flags.data(), b.infos.data(), dst.data()},
                        f_a, item_lo, staged, items_staged};
    last_write.spans++, last_write.frames_staged += staged, last_write.items_staged += items_staged;
    if ((long)nf > last_write.max_nf) last_write.max_nf = nf;
    if (item_lo < item_hi && (long)(item_hi - item_lo) > last_write.max_window) last_write.max_window = item_hi - item_lo;
    for (int r = 0; r < kPiecesPerLane; r++)
      for (uint32_t t = 0; t < (uint32_t)kBuildThreads; t++) {
        const uint64_t addr = span0 + ((uint64_t)r * kBuildThreads + t) * kPiece;
        const uint64_t pa = addr > addr_lo ? addr : addr_lo, pb = addr + kPiece < addr_hi ? addr + kPiece : addr_hi;
        if (pa >= pb) continue;
        Piece pc;
        assemble_piece(a, tb, f_a, f_b, addr, pa, pb, pc);
        for (uint32_t j = 0; j < kPiece; j++)
          if (pc.set & (1u << j)) {
            if (addr + j < pa || addr + j >= pb) fail("byte outside the piece's range", (long)blk, t, j);
            *(uint8_t*)(uintptr_t)(addr + j) = (uint8_t)pc.byte(j);
          }
        checks++;
      }
    std::free(tab), std::free(sinfo), std::free(sflag), std::free(sdst);
  }
}

void check_write(uint32_t seed, uint32_t nframes, uint32_t lead, uint32_t shift, uint64_t first_off, bool mismatch) {
  const HostBatch b = make_batch(seed, nframes, shift);
  const uint64_t n = b.infos.size();
  // expected frames and offsets
  std::vector<std::vector<uint8_t>> frames(n);
  std::vector<uint64_t> off(n + 1);
  off[0] = first_off;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t size;
    const uint8_t st = ufc_codec::check_frame(b.infos[i], b.items.data(), b.items.size(), b.src_base[i], b.payload.size(), size);
    if (st == UFC_BUILD_OK) {
      ref_write_frame(b, i, frames[i]);
      if (frames[i].size() != size) fail("frame size", (long)i, (long)size, (long)frames[i].size());
    }
    off[i + 1] = off[i] + frames[i].size();
  }
  const uint64_t victim = n / 2;
  if (mismatch) {  // one span a byte too long: that frame stays untouched
    for (uint64_t i = victim + 1; i <= n; i++) off[i] += 1;
  }
  const uint64_t out_len = off[n];
  // buffers of exactly the bytes the call may touch (heap: the sanitizer sees any access outside them)
  uint8_t* buf = (uint8_t*)std::malloc(lead + out_len + 1);
  std::memset(buf, 0xA5, lead + out_len + 1);
  uint8_t* pay = (uint8_t*)std::malloc(b.payload.size() + 1);
  std::memcpy(pay, b.payload.data(), b.payload.size());
  emulate_write(b, off, buf + lead, out_len, pay, b.payload.size());
  for (uint64_t p = 0; p < lead + first_off; p++)
    if (buf[p] != 0xA5) fail("write before the batch", (long)p, 0, 0);
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* got = buf + lead + off[i];
    const uint64_t len = off[i + 1] - off[i];
    if (mismatch && i == victim) {
      for (uint64_t k = 0; k < len; k++)
        if (got[k] != 0xA5) fail("mismatched span touched", (long)i, (long)k, 0);
    } else if (len != frames[i].size() || (len && std::memcmp(got, frames[i].data(), len) != 0)) {
      uint64_t k = 0;
      while (k < len && got[k] == frames[i][k]) k++;
      fail("frame bytes", (long)i, (long)k, (long)len);
    }
  }
  std::free(buf);
  std::free(pay);
}

// ---- table limits and caller-made layouts (tests/build_expect.py table_cases, the same numbers) ----
ufc_item poison_item() {
  ufc_item p{};
  p.id = 0xFFFFFFFFu, p.channel_id = 255, p.form = 9, p.flags = 0xFFFF, p.data_offset = 0xFFFFFF00u, p.data_len = 60000;
  return p;
}
HostBatch layout_batch(uint32_t n_items) {
  HostBatch b;
  b.items.assign(n_items, poison_item());
  return b;
}
// A frame whose items go to item_first: a data frame of cnt datagrams of dl + k bytes (form by k % 3), or an ack
// frame of cnt groups.  src >= 0: the frame takes its payload from that source base (a frame that names another's items).
size_t add_frame(HostBatch& b, Lcg& r, uint8_t kind, uint32_t item_first, uint32_t cnt, uint32_t dl, long src = -1) {
  ufc_frame_info in{};
  in.kind = kind, in.ok = 1, in.aux = (uint8_t)r.below(2), in.item_first = item_first, in.item_count = cnt;
  for (int k = 0; k < 5; k++) in.f[k] = r.next() * 2654435761u;
  b.src_base.push_back(src >= 0 ? (uint64_t)src : b.payload.size());
  if (src < 0) {
    uint32_t off = 0;
    for (uint32_t k = 0; k < cnt; k++) {
      ufc_item d{};
      if (kind == UFC_FRAME_DATA) {
        const uint32_t t = k % 3;
        d.id = r.below(1u << 20), d.channel_id = (uint8_t)r.below(64);
        d.window_parent_lead = (uint16_t)(t == 0 ? r.below(128) : r.below(65536));
        d.channel_parent_lead = (uint16_t)(t == 0 ? r.below(256) : r.below(65536));
        d.fragment_id_last = (uint16_t)(t == 2 ? 1 + r.below(65535) : 0);
        d.fragment_id = (uint16_t)(t == 2 ? r.below(65536) : 0);
        d.data_len = dl + (dl ? k : 0), d.data_offset = off;
        off += d.data_len;
      } else {
        d.id = r.next() * 2654435761u, d.data_offset = r.next() * 40503u, d.channel_id = (uint8_t)r.below(2), d.form = 3;
      }
      b.items[item_first + k] = d;
    }
    for (uint32_t k = 0; k < off; k++) b.payload.push_back((uint8_t)r.next());
  }
  b.infos.push_back(in);
  return b.infos.size() - 1;
}

struct LayoutFacts {
  long spans = -1, frames_staged = -1, items_staged = -1, max_nf = -1, max_window = -1;
};

// The write over b at the given offsets (empty: the sizes' running sum from first_off).  In-order offsets: every
// frame's bytes where its span is, guard bytes everywhere else.  backward: the rule for offsets that go backwards.
void check_layout(const char* name, const HostBatch& b, std::vector<uint64_t> off, uint32_t lead, uint64_t first_off,
                  const LayoutFacts& facts, bool backward) {
  const uint64_t n = b.infos.size();
  std::vector<std::vector<uint8_t>> frames(n);
  std::vector<uint64_t> sizes(n + 1, first_off);
  for (uint64_t i = 0; i < n; i++) {
    uint64_t size;
    if (ufc_codec::check_frame(b.infos[i], b.items.data(), b.items.size(), b.src_base[i], b.payload.size(), size) != UFC_BUILD_OK)
      fail(name, (long)i, -1, 0);
    ref_write_frame(b, i, frames[i]);
    if (frames[i].size() != size) fail("frame size", (long)i, (long)size, (long)frames[i].size());
    sizes[i + 1] = sizes[i] + size;
  }
  if (off.empty()) off = sizes;
  uint64_t out_len = 0;
  for (uint64_t o : off) out_len = o > out_len ? o : out_len;
  uint8_t* buf = (uint8_t*)std::malloc(lead + out_len + 1);
  std::memset(buf, 0xA5, lead + out_len + 1);
  uint8_t* pay = (uint8_t*)std::malloc(b.payload.size() + 1);
  std::memcpy(pay, b.payload.data(), b.payload.size());
  emulate_write(b, off, buf + lead, out_len, pay, b.payload.size());
  const WriteStats& w = last_write;
  if ((facts.spans >= 0 && w.spans != facts.spans) || (facts.frames_staged >= 0 && w.frames_staged != facts.frames_staged) ||
      (facts.items_staged >= 0 && w.items_staged != facts.items_staged))
    fail(name, w.spans, w.frames_staged, w.items_staged);
  if ((facts.max_nf >= 0 && w.max_nf != facts.max_nf) || (facts.max_window >= 0 && w.max_window != facts.max_window))
    fail(name, w.max_nf, w.max_window, -2);
  const uint8_t* out = buf + lead;
  std::vector<uint8_t> allowed(out_len, 0);
  for (uint64_t p = 0; p < lead; p++)
    if (buf[p] != 0xA5) fail("write before the buffer", (long)p, 0, 0);
  for (uint64_t p = 0; p < out_len; p++)
    if ((p < off[0] || p >= off[n]) && out[p] != 0xA5) fail("write outside the batch", (long)p, 0, 0);
  for (uint64_t p = 0; p < out_len; p++) allowed[p] = out[p] == 0xA5;
  for (uint64_t i = 0; i < n; i++) {
    if (off[i + 1] < off[i] || off[i + 1] - off[i] != frames[i].size()) continue;
    bool whole = true;
    for (uint64_t k = 0; k < frames[i].size(); k++) {
      const bool same = out[off[i] + k] == frames[i][k];
      allowed[off[i] + k] |= same;
      whole &= same;
    }
    uint64_t floor = ~0ull;  // the lowest offset from the first backward step on
    for (uint64_t j = 0; j < n; j++)
      if (off[j + 1] < off[j])
        for (uint64_t q = j + 1; q <= n; q++) floor = off[q] < floor ? off[q] : floor;
    if (!whole && (!backward || off[i + 1] <= floor)) fail("frame bytes", (long)i, (long)off[i], backward);
    checks++;
  }
  for (uint64_t p = 0; p < out_len; p++)
    if (!allowed[p]) fail("a byte that is neither guard nor its span's frame's", (long)p, 0, 0);
  std::free(buf);
  std::free(pay);
}

void table_cases() {
  Lcg r{515};
  {  // frames of 32 bytes: the kernel counts 512 frames for span 0 one byte past a 16-byte boundary, 513 at it
    for (uint32_t lead : {1u, 0u}) {
      HostBatch b = layout_batch(1100);
      for (uint32_t i = 0; i < 1100; i++) add_frame(b, r, UFC_FRAME_DATA, i, 1, 16);
      LayoutFacts f;
      f.spans = 3, f.max_nf = 513, f.frames_staged = lead == 1 ? 2 : 1, f.items_staged = f.frames_staged;
      check_layout(lead ? "frames_per_span[512]" : "frames_per_span[513]", b, {}, lead, 0, f, false);
    }
  }
  for (uint32_t window : {1024u, 1025u}) {  // two frames whose items lie a window apart, poison between
    HostBatch b = layout_batch(window);
    add_frame(b, r, UFC_FRAME_DATA, 0, 3, 40);
    add_frame(b, r, UFC_FRAME_DATA, window - 3, 3, 30);
    LayoutFacts f;
    f.spans = 1, f.frames_staged = 1, f.items_staged = window <= 1024, f.max_window = window, f.max_nf = 2;
    check_layout(window == 1024 ? "item_window[1024]" : "item_window[1025]", b, {}, 0, 0, f, false);
  }
  {  // a resent frame: the same records named twice in one span and once in the next
    HostBatch b = layout_batch(400);
    const size_t a = add_frame(b, r, UFC_FRAME_DATA, 7, 5, 50);
    add_frame(b, r, UFC_FRAME_DATA, 7, 5, 50, (long)b.src_base[a]);
    for (uint32_t k = 0; k < 50; k++) add_frame(b, r, UFC_FRAME_DATA, 20 + 4 * k, 4, 90);
    add_frame(b, r, UFC_FRAME_DATA, 7, 5, 50, (long)b.src_base[a]);
    LayoutFacts f;
    f.spans = 2, f.frames_staged = 2, f.items_staged = 2;
    check_layout("shared_items", b, {}, 0, 0, f, false);
  }
  {  // frame i's items lie behind frame i + 1's
    HostBatch b = layout_batch(200);
    uint32_t at = 200;
    for (uint32_t k = 0; k < 60; k++) {
      const uint32_t cnt = 1 + k % 4;
      at -= cnt;
      add_frame(b, r, k % 7 == 3 ? UFC_FRAME_ACK : UFC_FRAME_DATA, at, cnt, 100 + k);
    }
    LayoutFacts f;
    f.spans = 2, f.frames_staged = 2, f.items_staged = 2;
    check_layout("items_reversed", b, {}, 0, 0, f, false);
  }
  for (uint32_t lead = 0; lead < 4; lead++) {  // the batch starts 37 bytes into the buffer
    HostBatch b = layout_batch(240);
    for (uint32_t k = 0; k < 60; k++) add_frame(b, r, UFC_FRAME_DATA, 4 * k, 4, 60 + k);
    LayoutFacts f;
    f.spans = 2;
    check_layout("lo_nonzero", b, {}, lead, 37, f, false);
  }
  {  // one backward step in the middle of 40 frames: frame 20 starts 500 bytes before frame 19 does
    HostBatch b = layout_batch(160);
    for (uint32_t k = 0; k < 40; k++) add_frame(b, r, UFC_FRAME_DATA, 4 * k, 4, 30 + k);
    std::vector<uint64_t> off(41, 0);
    for (uint32_t i = 0; i < 40; i++) {
      uint64_t size;
      ufc_codec::check_frame(b.infos[i], b.items.data(), b.items.size(), b.src_base[i], b.payload.size(), size);
      off[i + 1] = off[i] + size;
    }
    const uint64_t back = off[20] - off[19] + 500;
    for (uint32_t i = 20; i <= 40; i++) off[i] -= back;
    if (!(off[20] < off[19])) fail("offsets_backwards", 0, 0, 0);
    check_layout("offsets_backwards", b, off, 3, 0, LayoutFacts{}, true);
  }
}

}  // namespace

int main() {
  // packed_byte over every byte of three words
  {
    const uint64_t w[3] = {0x0706050403020100ull, 0x0F0E0D0C0B0A0908ull, 0x1716151413121110ull};
    for (uint32_t j = 0; j < 24; j++, checks++)
      if (ufc_codec::packed_byte(w[0], w[1], w[2], j) != j) fail("packed_byte", j, 0, 0);
  }
  // datagram headers across the form boundaries
  const uint32_t dls[] = {0, 1, 62, 63, 64, 65, 254, 255, 256, 257, 1448, 65534, 65535};
  const uint32_t ws[] = {0, 1, 126, 127, 128, 129, 255, 256, 65535};
  const uint32_t hs_[] = {0, 1, 254, 255, 256, 257, 65535};
  const uint32_t chs[] = {0, 15, 16, 31, 32, 47, 48, 63};
  const uint32_t seqs[] = {0, 1, 0xFFFFF, 0x45678, 0x80001};
  const uint32_t frags[][2] = {{0, 0}, {7, 0}, {0, 1}, {1, 1}, {0x4789, 0x478A}, {65535, 65535}};
  for (uint32_t dl : dls)
    for (uint32_t w : ws)
      for (uint32_t h : hs_)
        for (uint32_t ch : chs)
          for (uint32_t seq : seqs)
            for (const auto& fr : frags) {
              ufc_item d{};
              d.id = seq, d.channel_id = (uint8_t)ch, d.window_parent_lead = (uint16_t)w;
              d.channel_parent_lead = (uint16_t)h, d.fragment_id = (uint16_t)fr[0], d.fragment_id_last = (uint16_t)fr[1];
              d.data_len = dl;
              d.form = 3, d.flags = 0xFFFF;  // ignored by the encode
              uint8_t ref[14] = {0}, got[14] = {0};
              const uint32_t rhs = ref_datagram_header(d, ref);
              const uint32_t hs = ufc_codec::datagram_header_size(d);
              if (hs != rhs) fail("header size", dl, w, h);
              if (ufc_codec::datagram_encoded_size(d) != (uint64_t)hs + dl) fail("encoded size", dl, w, h);
              if (!ufc_codec::datagram_fields_ok(d)) fail("fields_ok", ch, seq, dl);
              uint64_t w0, w1;
              ufc_codec::encode_datagram_header(d, hs, w0, w1);
              unpack(w0, w1, 0, hs, got);
              if (std::memcmp(ref, got, 14) != 0) fail("header bytes", dl, w, h);
              checks++;
            }
  {  // what build.rs:74-77 asserts
    ufc_item d{};
    d.channel_id = 64;
    if (ufc_codec::datagram_fields_ok(d)) fail("channel 64", 0, 0, 0);
    d.channel_id = 63, d.id = 1u << 20;
    if (ufc_codec::datagram_fields_ok(d)) fail("id 2^20", 0, 0, 0);
    d.id = (1u << 20) - 1, d.data_len = 65536;
    if (ufc_codec::datagram_fields_ok(d)) fail("data_len 65536", 0, 0, 0);
    d.data_len = 65535;
    if (!ufc_codec::datagram_fields_ok(d)) fail("limits", 0, 0, 0);
    checks += 4;
  }
  // ack groups
  for (uint32_t id : {0u, 1u, 0x28475809u, 0xFFFFFFFFu})
    for (uint32_t bits : {0u, 0x089EED35u, 0xFFFFFFFFu})
      for (uint32_t nonce : {0u, 1u, 255u}) {
        ufc_item g{};
        g.id = id, g.data_offset = bits, g.channel_id = (uint8_t)nonce;
        uint8_t ref[9], got[9];
        be32(ref, id), be32(ref + 4, bits), ref[8] = nonce ? 1 : 0;
        uint64_t w0, w1;
        ufc_codec::encode_ack_group(g, w0, w1);
        unpack(w0, w1, 0, 9, got);
        if (std::memcmp(ref, got, 9) != 0) fail("ack group", id, bits, nonce);
        checks++;
      }
  // frame heads and sizes of every kind
  const uint8_t kinds[] = {0, 1, 2, 3, 4, 5, 10, 11, 12};
  const uint32_t sizes[] = {1472, 25, 9, 10, 5, 5, 0, 14, 0};
  for (int ki = 0; ki < 9; ki++)
    for (uint32_t aux = 0; aux < 4; aux++)
      for (uint32_t cnt : {0u, 1u, 127u}) {
        ufc_frame_info in{};
        in.kind = kinds[ki], in.ok = 1, in.aux = (uint8_t)aux;
        in.f[0] = 0x01020304u, in.f[1] = 0x98765432u, in.f[2] = 0xA1B2C3D4u, in.f[3] = 0xABCDEF01u, in.f[4] = 0x18273645u;
        in.item_count = cnt;
        const bool data = in.kind == UFC_FRAME_DATA, ack = in.kind == UFC_FRAME_ACK;
        if ((data && aux > 1) || (in.kind == UFC_FRAME_HANDSHAKE_ERROR && aux > 2)) {
          std::vector<ufc_item> none(cnt);
          uint64_t size = 99;
          if (ufc_codec::check_frame(in, none.data(), cnt, 0, 0, size) != UFC_BUILD_BAD_FIELD || size != 0)
            fail("aux", in.kind, aux, cnt);
          checks++;
          continue;
        }
        uint8_t ref[24] = {0}, got[24] = {0};
        ufc_frame_info masked = in;  // the restatement's data header takes the count as given
        const uint32_t rn = ref_frame_head(masked, ref);
        uint64_t w0, w1, w2;
        const uint32_t n = ufc_codec::encode_frame_head(in, w0, w1, w2);
        if (n != rn || ufc_codec::frame_head_size(in.kind) != rn) fail("head size", in.kind, n, rn);
        unpack(w0, w1, w2, n, got);
        if (std::memcmp(ref, got, 24) != 0) fail("head bytes", in.kind, aux, cnt);
        std::vector<ufc_item> items(cnt);  // zero datagrams: micro, 6 bytes each
        uint64_t size = 0;
        const uint8_t st = ufc_codec::check_frame(in, items.data(), cnt, 0, 0, size);
        const uint64_t want = data ? 6 + 6ull * cnt + 4 : ack ? 11 + 9ull * cnt + 4 : sizes[ki];
        if (st != UFC_BUILD_OK || size != want) fail("size", in.kind, (long)size, (long)want);
        checks++;
      }
  // count limits, item range, source range, unknown kinds, ok == 0
  {
    std::vector<ufc_item> items(65536);
    ufc_frame_info in{};
    uint64_t size;
    in.ok = 1, in.kind = UFC_FRAME_DATA;
    for (uint32_t cnt : {0u, 127u, 128u}) {
      in.item_count = cnt;
      const uint8_t st = ufc_codec::check_frame(in, items.data(), items.size(), 0, 0, size);
      if (st != (cnt <= 127 ? UFC_BUILD_OK : UFC_BUILD_BAD_FIELD)) fail("data count", cnt, st, 0);
      checks++;
    }
    in.kind = UFC_FRAME_ACK;
    for (uint32_t cnt : {0u, 1u, 162u, 65535u, 65536u}) {
      in.item_count = cnt;
      const uint8_t st = ufc_codec::check_frame(in, items.data(), items.size(), 0, 0, size);
      if (st != (cnt <= 65535 ? UFC_BUILD_OK : UFC_BUILD_BAD_FIELD)) fail("ack count", cnt, st, 0);
      if (st == UFC_BUILD_OK && size != 11 + 9ull * cnt + 4) fail("ack size", cnt, (long)size, 0);
      checks++;
    }
    in.item_count = 3, in.item_first = 65534;  // one past the items
    if (ufc_codec::check_frame(in, items.data(), items.size(), 0, 0, size) != UFC_BUILD_BAD_FIELD) fail("item range", 0, 0, 0);
    in.item_first = 0xFFFFFFFFu;  // (no 32-bit wrap)
    if (ufc_codec::check_frame(in, items.data(), items.size(), 0, 0, size) != UFC_BUILD_BAD_FIELD) fail("item wrap", 0, 0, 0);
    in.kind = UFC_FRAME_DATA, in.item_first = 10, in.item_count = 2;
    items[11].data_offset = 90, items[11].data_len = 10;
    if (ufc_codec::check_frame(in, items.data(), items.size(), 0, 100, size) != UFC_BUILD_OK || size != 6 + 6 + 16 + 4)
      fail("src at end", (long)size, 0, 0);
    if (ufc_codec::check_frame(in, items.data(), items.size(), 0, 99, size) != UFC_BUILD_BAD_SRC) fail("src past end", 0, 0, 0);
    if (ufc_codec::check_frame(in, items.data(), items.size(), 1, 100, size) != UFC_BUILD_BAD_SRC) fail("src base", 0, 0, 0);
    if (ufc_codec::check_frame(in, items.data(), items.size(), ~0ull, 100, size) != UFC_BUILD_BAD_SRC) fail("src wrap", 0, 0, 0);
    items[11].data_offset = 0xFFFFFFFFu, items[11].data_len = 0xFFFFu;
    if (ufc_codec::check_frame(in, items.data(), items.size(), 0, ~0ull, size) != UFC_BUILD_OK) fail("src wide", 0, 0, 0);
    items[10].channel_id = 64;  // a bad field outranks a bad source
    if (ufc_codec::check_frame(in, items.data(), items.size(), 0, 0, size) != UFC_BUILD_BAD_FIELD) fail("field first", 0, 0, 0);
    for (uint32_t kind : {6u, 9u, 13u, 255u}) {
      in.kind = (uint8_t)kind;
      if (ufc_codec::check_frame(in, items.data(), items.size(), 0, 0, size) != UFC_BUILD_BAD_FIELD) fail("kind", kind, 0, 0);
    }
    in.ok = 0;
    if (ufc_codec::check_frame(in, items.data(), items.size(), 0, 0, size) != UFC_BUILD_SKIPPED) fail("skipped", 0, 0, 0);
    checks += 12;
  }
  // Piece::put_packed (two word shifts) against a byte loop, every (from, at, nb)
  for (uint32_t from = 0; from < 24; from++)
    for (uint32_t at = 0; at < 16; at++)
      for (uint32_t nb = 1; from + nb <= 24 && at + nb <= 16; nb++, checks++) {
        const uint64_t h0 = 0x8877665544332211ull, h1 = 0x00FFEEDDCCBBAA99ull, h2 = 0x1817161514131211ull;
        ufc_dev::Piece a, b;
        a.put_packed(at, nb, h0, h1, h2, from);
        for (uint32_t j = 0; j < nb; j++) b.put(at + j, ufc_codec::packed_byte(h0, h1, h2, from + j));
        if (a.w0 != b.w0 || a.w1 != b.w1 || a.set != b.set) fail("put_packed", from, at, nb);
      }
  // the write, piece by piece: every alignment of the output, payload shifts, a batch that does not start
  // at offset 0, a mismatched span
  for (uint32_t lead = 0; lead < 16; lead++) check_write(100 + lead, 160, lead, lead % 5, lead % 3 ? 0 : 5, lead == 7);
  check_write(7, 900, 3, 1, 0, false);
  check_write(8, 900, 11, 0, 7, true);
  table_cases();
  std::printf("ok: %ld checks\n", checks);
  return 0;
}
