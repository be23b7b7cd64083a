// frame_build_piece.hpp -- the write step of the GPU batch build (frame_build.hip) below the kernel:
// how the output stream is cut into spans and 16-byte pieces, and the assembly of one piece.  Everything
// here is __host__ __device__, so the same index arithmetic runs as host code under sanitizers
// (tests/c/build_host_check.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "frame_build.hpp"
#include "frame_codec_core.hpp"

namespace ufc_dev {

constexpr int kBuildThreads = 256;
constexpr int kPiecesPerLane = 4;
constexpr uint32_t kPiece = 16;
constexpr uint64_t kSpanBytes = (uint64_t)kBuildThreads * kPiecesPerLane * kPiece;  // 16 KiB per workgroup

#define UFC_BHD __host__ __device__ __forceinline__

// Pieces and spans are cut by address: the first span starts at the 16-byte boundary at or before the
// batch's first byte.
UFC_BHD uint64_t first_span_addr(uint64_t addr_lo) { return addr_lo & ~(uint64_t)(kPiece - 1); }
// Workgroups of the write over a buffer of out_len bytes.
UFC_BHD uint64_t write_spans(uint64_t out_len) { return (out_len + (kPiece - 1) + kSpanBytes - 1) / kSpanBytes; }

// Frame i with span [oa, ob) of a batch that starts at offset lo of the buffer at address `base`: it owns
// the first byte of span 0 if it holds byte lo, and of each span s in 1..spans that starts inside it
// (span s starts at first_span_addr(base + lo) + s * kSpanBytes).
UFC_BHD void note_span_owner(uint64_t base, uint64_t lo, uint64_t oa, uint64_t ob, uint32_t i, uint32_t* span_owner,
                             uint64_t spans) {
  if (ob <= oa || oa < lo) return;
  const uint64_t a0 = first_span_addr(base + lo);
  if (oa == lo) span_owner[0] = i;
  uint64_t s = (base + oa - a0 + kSpanBytes - 1) / kSpanBytes;
  if (s == 0) s = 1;
  for (; s <= spans && a0 + s * kSpanBytes < base + ob; s++) span_owner[s] = i;
}

// The last index k in [lo, hi] with get(k) <= key (get(lo) <= key is the caller's).
template <class Get>
UFC_BHD uint32_t last_le(const Get& get, uint32_t lo, uint32_t hi, uint64_t key) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (get(mid) <= key)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// The bytes [a, b) of an 8-byte word as a mask (0 <= a, b <= 8; every shift amount in range).
UFC_BHD uint64_t byte_mask(uint32_t a, uint32_t b) {
  if (b <= a) return 0;
  const uint32_t nb = b - a;
  const uint64_t m = nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1);
  return m << (8 * a);
}

// 8 bytes at any address.
UFC_BHD uint64_t load_u64_unaligned(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (a byte-aligned global view, as frame_parse.hip: one global_load_dwordx2 in gfx950's unaligned access mode)
  typedef const __attribute__((address_space(1), aligned(1))) uint64_t g_u64_a1;
  return *(g_u64_a1*)p;
#else
  uint64_t v;
  std::memcpy(&v, p, 8);
  return v;
#endif
}

// A piece being assembled: 16 bytes in two little-endian words, and which of them are set.
struct Piece {
  uint64_t w0 = 0, w1 = 0;
  uint32_t set = 0;  // bit j: byte j is to be stored
  UFC_BHD void put(uint32_t at, uint32_t v) {
    const uint64_t b = (uint64_t)(v & 0xFFu) << (8 * (at & 7u));
    if (at < 8)
      w0 |= b;
    else
      w1 |= b;
    set |= 1u << at;
  }
  // bytes [at, at + nb) of the piece = bytes [from, from + nb) of the packed words (h0, h1, h2); at < 16,
  // from < 24.  Two word-wide shifts (the 24 header bytes down by `from`, then up by `at`) instead of a
  // loop over the bytes: every shift amount is 8 .. 56 or the shift is skipped.
  UFC_BHD void put_packed(uint32_t at, uint32_t nb, uint64_t h0, uint64_t h1, uint64_t h2, uint32_t from) {
    const uint32_t q = from >> 3, s = 8 * (from & 7u);
    const uint64_t a0 = q == 0 ? h0 : (q == 1 ? h1 : h2), a1 = q == 0 ? h1 : (q == 1 ? h2 : 0ull), a2 = q == 0 ? h2 : 0ull;
    const uint64_t r0 = s ? (a0 >> s) | (a1 << (64 - s)) : a0;  // header bytes from, from + 1, ... as bytes 0, 1, ...
    const uint64_t r1 = s ? (a1 >> s) | (a2 << (64 - s)) : a1;
    const uint32_t u = 8 * (at & 7u);
    uint64_t v0, v1;
    if (at < 8) {
      v0 = r0 << u;
      v1 = u ? (r1 << u) | (r0 >> (64 - u)) : r1;
    } else {
      v0 = 0;
      v1 = r0 << u;
    }
    merge(at, nb, v0, v1);
  }
  UFC_BHD void zeros(uint32_t at, uint32_t nb) { set |= ((1u << nb) - 1u) << at; }  // (at + nb <= 16)
  // bytes [at, at + nb) = the same bytes of (v0, v1)
  UFC_BHD void merge(uint32_t at, uint32_t nb, uint64_t v0, uint64_t v1) {
    const uint32_t end = at + nb;
    w0 |= v0 & byte_mask(at, end < 8u ? end : 8u);
    w1 |= v1 & byte_mask(at > 8 ? at - 8 : 0u, end > 8 ? end - 8 : 0u);
    zeros(at, nb);
  }
  UFC_BHD uint32_t byte(uint32_t j) const { return ufc_codec::packed_byte(w0, w1, 0, j); }
};

// The piece at address `addr` (a multiple of 16): its bytes [pa, pb) (addresses inside the piece and the
// batch's stream) from the frames toff(k) = out_offsets[k] describes, k in [f_a, f_b + 1], where frames
// f_a..f_b hold every frame that owns a byte of the piece.  dst: the items' destinations (exclusive sum of
// their encoded sizes), flag: which frames are written.  Bytes of frames that are not written, and bytes
// no frame in f_a..f_b owns (offsets out of order), stay unset.
// The tables come through `tb` (in global memory, or a workgroup's copies in LDS): tb.off(k), tb.flag(f),
// tb.info(f) for frames f_a..f_b (off also f_b + 1), tb.dst(k) for the items of their written data frames.
struct GlobalTables {
  const uint64_t* offs;
  const uint8_t* flags;
  const ufc_frame_info* infos;
  const uint64_t* dsts;
  UFC_BHD uint64_t off(uint32_t k) const { return offs[k]; }
  UFC_BHD bool flag(uint32_t f) const { return flags[f] != 0; }
  UFC_BHD ufc_frame_info info(uint32_t f) const { return infos[f]; }
  UFC_BHD uint64_t dst(uint32_t k) const { return dsts[k]; }
};

constexpr uint32_t kTabFrames = 512;   // frames whose offsets, flags and infos a workgroup stages in LDS
constexpr uint32_t kTabItems = 1024;   // item destinations it stages
// Whether a span's nf frames, and the item window [lo, hi) of its written data frames, are staged (the kernel
// and tests/c/build_host_check.hip take both switches from here).
#define UFC_BUILD_FRAMES_STAGED(nf) ((nf) <= kTabFrames)
#define UFC_BUILD_ITEMS_STAGED(staged, lo, hi) ((staged) && (lo) < (hi) && (hi) - (lo) <= kTabItems)

// The write kernel's tables for one workgroup span, in LDS when they fit: the offsets, flags and infos of
// the frames that touch the span, and the destinations of the items of its written data frames (the
// window from the lowest first item to the highest last one, wherever the frames keep their items).
// What does not fit is read from global memory: more than kTabFrames frames (tiny or empty frames), or
// an item window over kTabItems.
struct SpanTables {
  const uint64_t* tab;          // LDS: out_offsets[f_a ..]
  const ufc_frame_info* sinfo;  // LDS: infos[f_a ..]
  const uint8_t* sflag;         // LDS: flags[f_a ..]
  const uint64_t* sdst;         // LDS: dst[item_lo ..]
  GlobalTables g;
  uint32_t f_a, item_lo;
  bool frames_staged, items_staged;
  UFC_BHD uint64_t off(uint32_t k) const { return frames_staged ? tab[k - f_a] : g.off(k); }
  UFC_BHD bool flag(uint32_t f) const { return frames_staged ? sflag[f - f_a] != 0 : g.flag(f); }
  UFC_BHD ufc_frame_info info(uint32_t f) const { return frames_staged ? sinfo[f - f_a] : g.info(f); }
  UFC_BHD uint64_t dst(uint32_t k) const { return items_staged ? sdst[k - item_lo] : g.dst(k); }
};

template <class Tables>
UFC_BHD void assemble_piece(const BuildArgs& a, const Tables& tb, uint32_t f_a, uint32_t f_b, uint64_t addr, uint64_t pa,
                            uint64_t pb, Piece& pc) {
  auto toff = [&](uint32_t k) -> uint64_t { return tb.off(k); };
  const uint64_t base = (uint64_t)(uintptr_t)a.out_bytes;
  uint64_t p = pa;  // the next byte's address
  while (p < pb) {
    const uint64_t pos = p - base;
    // its frame: the last that starts at or before it (length-0 frames before that one start there too)
    const uint32_t f = last_le(toff, f_a, f_b, pos);
    const uint64_t fs = toff(f), fe = toff(f + 1);
    if (!(fs <= pos && pos < fe)) break;  // (offsets out of order: nothing of this piece from here on)
    const uint64_t seg_end = base + fe < pb ? base + fe : pb;
    if (!tb.flag(f)) {  // a frame that is not written: its bytes stay as they are
      p = seg_end;
      continue;
    }
    const ufc_frame_info info = tb.info(f);
    const uint32_t size = (uint32_t)(fe - fs);  // (span_matches: the frame's size, < 2^32)
    const uint32_t head = ufc_codec::frame_head_size(info.kind);  // (encoded only by the pieces that hold it)
    uint64_t dst_first = 0, sbase = 0;
    if (info.kind == UFC_FRAME_DATA && info.item_count) {
      dst_first = tb.dst(info.item_first);
      sbase = a.src_base ? a.src_base[f] : 0ull;
    }
    while (p < seg_end) {
      const uint32_t fr = (uint32_t)(p - base - fs);  // byte of the frame
      const uint32_t at = (uint32_t)(p - addr);       // byte of the piece
      const uint32_t room = (uint32_t)(seg_end - p);
      uint32_t nb;
      if (fr < head) {
        uint64_t h0, h1, h2;
        ufc_codec::encode_frame_head(info, h0, h1, h2);
        nb = head - fr < room ? head - fr : room;
        pc.put_packed(at, nb, h0, h1, h2, fr);
      } else if (fr >= size - 4) {  // trailer: zeros (the seal that follows writes the CRC)
        nb = room;
        pc.zeros(at, nb);
      } else if (info.kind == UFC_FRAME_ACK) {
        const uint32_t k = (fr - ufc_codec::kAckHead) / UFC_ACK_GROUP_SIZE;
        const uint32_t c = (fr - ufc_codec::kAckHead) % UFC_ACK_GROUP_SIZE;
        uint64_t g0, g1;
        ufc_codec::encode_ack_group(a.items[(uint64_t)info.item_first + k], g0, g1);
        nb = UFC_ACK_GROUP_SIZE - c < room ? UFC_ACK_GROUP_SIZE - c : room;
        pc.put_packed(at, nb, g0, g1, 0, c);
      } else if (info.kind == UFC_FRAME_DATA) {
        // the datagram that holds frame byte fr: the last whose destination is <= fr's
        const uint64_t key = dst_first + (fr - ufc_codec::kDataHead);
        auto gdst = [&](uint32_t k) -> uint64_t { return tb.dst(k); };
        const uint32_t k = last_le(gdst, info.item_first, info.item_first + info.item_count - 1, key);
        const ufc_item d = a.items[k];
        const uint32_t o = (uint32_t)(key - tb.dst(k));  // byte of the encoded datagram
        const uint32_t hs = ufc_codec::datagram_header_size(d);
        if (o < hs) {
          uint64_t g0, g1;
          ufc_codec::encode_datagram_header(d, hs, g0, g1);
          nb = hs - o < room ? hs - o : room;
          pc.put_packed(at, nb, g0, g1, 0, o);
        } else {
          const uint32_t q = o - hs;  // byte of the payload
          nb = d.data_len - q < room ? d.data_len - q : room;
          const uint64_t s = sbase + d.data_offset + q;  // its offset in the payload buffer
          if (s >= at && s - at + kPiece <= a.payload_len) {
            // one unaligned 16-byte load placed so that source byte s falls on piece byte `at`
            const uint8_t* src = a.payload + (s - at);
            pc.merge(at, nb, load_u64_unaligned(src), load_u64_unaligned(src + 8));
          } else {  // within 16 bytes of the payload buffer's ends
            for (uint32_t j = 0; j < nb; j++) pc.put(at + j, a.payload[s + j]);
          }
        }
      } else {  // handshake_syn's zero padding
        nb = size - 4 - fr < room ? size - 4 - fr : room;
        pc.zeros(at, nb);
      }
      p += nb;
    }
  }
}

}  // namespace ufc_dev
