// frame_codec_core.hpp -- the payload parse of Frame::read (everything after the CRC gate), written
// once for the host codec (frame_codec.cpp) and the GPU batch parse (frame_parse.hip); further down the
// encode for the batched builds (frame_build.hip), the emitters' arithmetic for the batched packs
// (frame_pack.hip) and the packet sender's for the batched packet emits (packet_emit.hip).
//
// Restates src/frame/serial/mod.rs:694-705 (dispatch on the frame id) and read_*_payload :54-434,
// read_datagram :183-309.  A byte reader abstracts the frame: rd(i) = frame byte i (i < len).
// Only bytes the reference reads are read, in the order it checks lengths, so a rejected frame
// never reads past its end.  rd.head3(i) = bytes i, i + 1, i + 2 packed little-endian (the caller has
// checked that at least 6 bytes remain from i; a reader may read byte i + 3 with them).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/uflow_frame_codec.h"

namespace ufc_codec {

#define UFC_HD __host__ __device__ __forceinline__

constexpr uint32_t kMaxFrameSize = 1472;                  // src/lib.rs:286-294
constexpr uint32_t kSynPayload = kMaxFrameSize - 5;       // serial/mod.rs:25
constexpr uint32_t kDataPayloadHeader = 5;                // serial/mod.rs:41
constexpr uint32_t kAckPayloadHeader = 10;                // serial/mod.rs:49

template <class Rd>
UFC_HD uint32_t be32(const Rd& rd, uint32_t i) {
  return (rd(i) << 24) | (rd(i + 1) << 16) | (rd(i + 2) << 8) | rd(i + 3);
}
template <class Rd>
UFC_HD uint32_t be16(const Rd& rd, uint32_t i) {
  return (rd(i) << 8) | rd(i + 1);
}

// src/half_connection/packet_receiver/mod.rs:12-30 `datagram_is_valid` on a decoded datagram
// (CHANNEL_COUNT = MAX_CHANNELS = 64, src/lib.rs:278; MAX_FRAGMENT_SIZE, src/lib.rs:297).
UFC_HD bool datagram_is_valid(const ufc_item& d) {
  if (d.channel_id >= UFC_MAX_CHANNELS) return false;
  if (d.channel_parent_lead != 0 && (d.window_parent_lead == 0 || d.channel_parent_lead < d.window_parent_lead))
    return false;
  if (d.fragment_id > d.fragment_id_last) return false;
  if (d.fragment_id < d.fragment_id_last && d.data_len != UFC_MAX_FRAGMENT_SIZE) return false;
  if (d.data_len > UFC_MAX_FRAGMENT_SIZE) return false;
  return true;
}

// A datagram header (read_datagram, serial/mod.rs:183-309) from a header reader h(c) = byte c of
// the header: its size hs (micro 6, small 9, large 14) and payload length dl (bytes 0..2) ...
// The three bytes are read together (one dependent step per datagram in a walk, not two): the
// callers have checked that at least 6 header bytes remain.
template <class H>
UFC_HD void datagram_size(const H& h, uint32_t& hs, uint32_t& dl) {
  const uint32_t b0 = h(0), b1 = h(1), b2 = h(2);
  if ((b0 & 0x80) == 0) {  // micro (:190-229)
    hs = 6;
    dl = b0 & 0x3F;
  } else if ((b0 & 0x40) == 0) {  // small (:230-268)
    hs = 9;
    dl = b1;
  } else {  // large (:269-308)
    hs = 14;
    dl = (b1 << 8) | b2;
  }
}

// ... and its fields, once the frame is known to hold hs + dl bytes from the header on.
// data_offset is left to the caller (the header's frame offset + hs).
template <class H>
UFC_HD void decode_datagram(const H& h, uint32_t hs, ufc_item& it) {
  const uint32_t b0 = h(0);
  if (hs == 6) {  // micro
    const uint32_t b1 = h(1), b4d = h(4);
    it.channel_id = (uint8_t)(((b4d >> 2) & 0x20) | ((b0 >> 2) & 0x10) | (b1 & 0x0F));
    it.id = ((b1 & 0xF0) << 12) | (h(2) << 8) | h(3);
    it.window_parent_lead = (uint16_t)(b4d & 0x7F);
    it.channel_parent_lead = (uint16_t)h(5);
    it.form = 0;
    it.data_len = b0 & 0x3F;
  } else if (hs == 9) {  // small
    it.channel_id = (uint8_t)(b0 & 0x3F);
    it.id = ((h(2) & 0x0F) << 16) | (h(3) << 8) | h(4);
    it.window_parent_lead = (uint16_t)((h(5) << 8) | h(6));
    it.channel_parent_lead = (uint16_t)((h(7) << 8) | h(8));
    it.form = 1;
    it.data_len = h(1);
  } else {  // large
    it.channel_id = (uint8_t)(b0 & 0x3F);
    it.id = ((h(3) & 0x0F) << 16) | (h(4) << 8) | h(5);
    it.window_parent_lead = (uint16_t)((h(6) << 8) | h(7));
    it.channel_parent_lead = (uint16_t)((h(8) << 8) | h(9));
    it.fragment_id = (uint16_t)((h(10) << 8) | h(11));
    it.fragment_id_last = (uint16_t)((h(12) << 8) | h(13));
    it.form = 2;
    it.data_len = (h(1) << 8) | h(2);
  }
  it.flags = datagram_is_valid(it) ? UFC_ITEM_VALID : 0;
}

// An ack group (serial/mod.rs:395-417) from h(c) = byte c of the group.
template <class H>
UFC_HD void decode_ack_group(const H& h, ufc_item& it) {
  it.id = (h(0) << 24) | (h(1) << 16) | (h(2) << 8) | h(3);
  it.data_offset = (h(4) << 24) | (h(5) << 16) | (h(6) << 8) | h(7);  // bitfield
  it.channel_id = (uint8_t)(h(8) != 0 ? 1 : 0);
  it.form = 3;
}

// Where the items go: sink(k, item) for k < cap, when sink.on().  PtrSink: a plain array.
// kDecode false: the sink only takes each datagram header's frame offset, header(k, off).
struct PtrSink {
  static constexpr bool kDecode = true;
  ufc_item* p;
  UFC_HD bool on() const { return p != nullptr; }
  UFC_HD void operator()(uint32_t k, const ufc_item& it) const { p[k] = it; }
  UFC_HD void header(uint32_t, uint32_t) const {}
};

// Parse the payload of a frame of `len` bytes (len >= 5) whose CRC gate passed.  Fills `info`
// (kind, aux, f[], item_count) and, when the sink is on, the first `cap` items.  Returns
// whether Frame::read returns Some.
template <class Rd, class Sink>
UFC_HD bool parse_payload(const Rd& rd, uint32_t len, ufc_frame_info& info, const Sink& items, uint32_t cap) {
  const uint32_t plen = len - 5;  // payload = frame[1 .. len - 4]
  auto p = [&](uint32_t i) -> uint32_t { return rd(1 + i); };
  auto p32 = [&](uint32_t i) -> uint32_t { return be32(rd, 1 + i); };
  auto p16 = [&](uint32_t i) -> uint32_t { return be16(rd, 1 + i); };
  info.item_count = 0;
  switch (info.kind) {
    case UFC_FRAME_HANDSHAKE_SYN:  // :54-87
      if (plen != kSynPayload) return false;
      info.aux = (uint8_t)p(0);
      info.f[0] = p32(1); info.f[1] = p32(5); info.f[2] = p32(9); info.f[3] = p32(13);
      return true;
    case UFC_FRAME_HANDSHAKE_SYN_ACK:  // :89-126
      if (plen != 20) return false;
      info.f[0] = p32(0); info.f[1] = p32(4); info.f[2] = p32(8); info.f[3] = p32(12); info.f[4] = p32(16);
      return true;
    case UFC_FRAME_HANDSHAKE_ACK:  // :128-141
      if (plen != 4) return false;
      info.f[0] = p32(0);
      return true;
    case UFC_FRAME_HANDSHAKE_ERROR: {  // :143-165
      if (plen != 5) return false;
      const uint32_t e = p(4);
      if (e > 2) return false;
      info.f[0] = p32(0);
      info.aux = (uint8_t)e;
      return true;
    }
    case UFC_FRAME_DISCONNECT:      // :167-173
    case UFC_FRAME_DISCONNECT_ACK:  // :175-181
      return plen == 0;
    case UFC_FRAME_DATA: {  // :311-340
      if (plen < kDataPayloadHeader) return false;
      info.f[0] = p32(0);
      const uint32_t b4 = p(4);
      info.aux = (uint8_t)(b4 >> 7);
      const uint32_t cnt = b4 & 0x7F;
      uint32_t pos = kDataPayloadHeader;
      for (uint32_t k = 0; k < cnt; k++) {  // read_datagram, :183-309
        const uint32_t rem = plen - pos;
        if (rem < 6) return false;
        auto h = [&](uint32_t c) -> uint32_t { return p(pos + c); };
        // the header's first three bytes at once (rd.head3: one read where the reader can, so the
        // sizes of small and large datagrams do not wait on a second read after the first byte's)
        const uint32_t h3 = rd.head3(1 + pos);
        uint32_t hs, dl;
        datagram_size([&](uint32_t c) -> uint32_t { return (h3 >> (8 * c)) & 0xFFu; }, hs, dl);
        if (rem < hs + dl) return false;
        if (items.on() && k < cap) {
          if (Sink::kDecode) {
            ufc_item it{};
            decode_datagram(h, hs, it);
            it.data_offset = 1 + pos + hs;
            items(k, it);
          } else {
            items.header(k, 1 + pos);  // the header's frame offset only
          }
        }
        pos += hs + dl;
      }
      if (pos != plen) return false;  // :335-337
      info.item_count = cnt;
      return true;
    }
    case UFC_FRAME_SYNC: {  // :342-367
      if (plen != 9) return false;
      const uint32_t mode = p(0);
      info.aux = (uint8_t)(mode & 3u);
      info.f[0] = (mode & 1u) ? p32(1) : 0u;
      info.f[1] = (mode & 2u) ? p32(5) : 0u;
      return true;
    }
    case UFC_FRAME_ACK: {  // :369-434
      if (plen < kAckPayloadHeader) return false;
      const uint32_t cnt = p16(8);
      // each group needs 9 bytes (:395-397, :412-417) and nothing may remain (:425-427)
      if (plen - kAckPayloadHeader != UFC_ACK_GROUP_SIZE * cnt) return false;
      info.f[0] = p32(0);
      info.f[1] = p32(4);
      if (items.on() && Sink::kDecode) {  // (ack groups sit at fixed offsets: no header hook)
        for (uint32_t k = 0; k < cnt && k < cap; k++) {
          const uint32_t o = kAckPayloadHeader + UFC_ACK_GROUP_SIZE * k;
          ufc_item it{};
          decode_ack_group([&](uint32_t c) -> uint32_t { return p(o + c); }, it);
          items(k, it);
        }
      }
      info.item_count = cnt;
      return true;
    }
    default:
      return false;  // unknown id (:704)
  }
}

// Frame::read given the CRC gate's verdict for the frame (crc_ok = len >= 5 && trailer matches).
template <class Rd, class Sink>
UFC_HD bool read_frame_to(const Rd& rd, uint32_t len, bool crc_ok, ufc_frame_info& info, const Sink& items,
                          uint32_t cap) {
  info.kind = len >= 1 ? (uint8_t)rd(0) : (uint8_t)0xFF;
  info.ok = 0;
  info.aux = 0;
  info.crc_ok = (crc_ok && len >= 5) ? 1 : 0;
  for (int i = 0; i < 5; i++) info.f[i] = 0;
  info.item_count = 0;
  if (!info.crc_ok) return false;
  const bool ok = parse_payload(rd, len, info, items, cap);
  if (!ok) info.item_count = 0;
  info.ok = ok ? 1 : 0;
  return ok;
}

template <class Rd>
UFC_HD bool read_frame(const Rd& rd, uint32_t len, bool crc_ok, ufc_frame_info& info, ufc_item* items,
                       uint32_t cap) {
  return read_frame_to(rd, len, crc_ok, info, PtrSink{items}, cap);
}

// ---- encode: Frame::write from the parse's records, for the batched builds (host and GPU) ----
//
// Restates write_* (serial/mod.rs:437-657), DataFrameBuilder::{new, add, encoded_size} (build.rs:55-143,
// 172-183) and AckFrameBuilder::{new, add} (build.rs:192-228).  A header is produced as packed
// little-endian words (byte j of the header = bits 8 (j & 7) of word j >> 3), so that a writer that owns
// an arbitrary byte range of the output (the GPU's 16-byte pieces) takes any byte of it without a buffer.
constexpr uint32_t kPacketIdMask = (1u << 20) - 1;  // src/packet_id.rs
constexpr uint32_t kDataHead = 1 + kDataPayloadHeader;  // frame id + sequence id + nonce | count
constexpr uint32_t kAckHead = 1 + kAckPayloadHeader;    // frame id + two base ids + count

// Byte j (j < 24) of three packed words; every shift amount in range.
UFC_HD uint32_t packed_byte(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t j) {
  const uint32_t q = (j >> 3) & 3u;
  const uint64_t w = q == 0 ? w0 : (q == 1 ? w1 : w2);
  return (uint32_t)(w >> (8 * (j & 7u))) & 0xFFu;
}
UFC_HD uint64_t pk(uint32_t j, uint32_t v) { return (uint64_t)(v & 0xFFu) << (8 * (j & 7u)); }
UFC_HD uint64_t pk_be32(uint32_t j, uint32_t v) {  // four bytes inside one word (j & 7 <= 4)
  return pk(j, v >> 24) | pk(j + 1, v >> 16) | pk(j + 2, v >> 8) | pk(j + 3, v);
}
UFC_HD uint64_t pk_be16(uint32_t j, uint32_t v) { return pk(j, v >> 8) | pk(j + 1, v); }

// The header form DataFrameBuilder::add chooses (build.rs:81-122): 6 micro, 9 small, 14 large.
// ufc_item.form and .flags play no part.
UFC_HD uint32_t datagram_header_size(const ufc_item& d) {
  if (d.fragment_id_last == 0) {
    if (d.data_len < 64 && d.window_parent_lead < 128 && d.channel_parent_lead < 256) return 6;
    if (d.data_len < 256) return 9;
  }
  return 14;
}
// DataFrameBuilder::encoded_size (build.rs:172-183).
UFC_HD uint64_t datagram_encoded_size(const ufc_item& d) { return (uint64_t)datagram_header_size(d) + d.data_len; }
// What build.rs:74-77 debug-asserts of a datagram.
UFC_HD bool datagram_fields_ok(const ufc_item& d) {
  return d.channel_id < UFC_MAX_CHANNELS && d.id <= kPacketIdMask && d.data_len <= 0xFFFFu;
}

// The datagram header of hs = datagram_header_size(d) bytes (build.rs:84-143).
UFC_HD void encode_datagram_header(const ufc_item& d, uint32_t hs, uint64_t& w0, uint64_t& w1) {
  const uint32_t dl = d.data_len, ch = d.channel_id, seq = d.id;
  const uint32_t w = d.window_parent_lead, h = d.channel_parent_lead;
  if (hs == 6) {  // micro, :84-100
    w0 = pk(0, dl | ((ch & 0x10) << 2)) | pk(1, ((seq >> 12) & 0xF0) | (ch & 0x0F)) | pk(2, seq >> 8) | pk(3, seq) |
         pk(4, w | ((ch & 0x20) << 2)) | pk(5, h);
    w1 = 0;
  } else if (hs == 9) {  // small, :101-119
    w0 = pk(0, ch | 0x80) | pk(1, dl) | pk(2, seq >> 16) | pk(3, seq >> 8) | pk(4, seq) | pk_be16(5, w) | pk(7, h >> 8);
    w1 = pk(8, h);
  } else {  // large, :123-143
    w0 = pk(0, ch | 0xC0) | pk_be16(1, dl) | pk(3, seq >> 16) | pk(4, seq >> 8) | pk(5, seq) | pk_be16(6, w);
    w1 = pk_be16(8, h) | pk_be16(10, d.fragment_id) | pk_be16(12, d.fragment_id_last);
  }
}

// An ack group's UFC_ACK_GROUP_SIZE bytes (build.rs:213-228): id = base_id, data_offset = bitfield,
// channel_id != 0 = nonce.
UFC_HD void encode_ack_group(const ufc_item& g, uint64_t& w0, uint64_t& w1) {
  w0 = pk_be32(0, g.id) | pk_be32(4, g.data_offset);
  w1 = pk(8, g.channel_id != 0 ? 1u : 0u);
}

// How many bytes encode_frame_head gives for a frame of this kind.
UFC_HD uint32_t frame_head_size(uint32_t kind) {
  switch (kind) {
    case UFC_FRAME_HANDSHAKE_SYN: return 18;
    case UFC_FRAME_HANDSHAKE_SYN_ACK: return 21;
    case UFC_FRAME_HANDSHAKE_ACK: return 5;
    case UFC_FRAME_HANDSHAKE_ERROR: return 6;
    case UFC_FRAME_DATA: return kDataHead;
    case UFC_FRAME_SYNC: return 10;
    case UFC_FRAME_ACK: return kAckHead;
    default: return 1;
  }
}

// The bytes a frame starts with: the whole body of a fixed-size frame (handshake_syn: the 18 bytes
// before its zero padding), the data frame's 6 and the ack frame's 11.  Returns their count.
UFC_HD uint32_t encode_frame_head(const ufc_frame_info& info, uint64_t& w0, uint64_t& w1, uint64_t& w2) {
  const uint32_t* f = info.f;
  w0 = pk(0, info.kind);
  w1 = w2 = 0;
  switch (info.kind) {
    case UFC_FRAME_HANDSHAKE_SYN:  // :437-473
      w0 |= pk(1, info.aux) | pk_be32(2, f[0]) | pk_be16(6, f[1] >> 16);
      w1 = pk_be16(8, f[1]) | pk_be32(10, f[2]) | pk_be16(14, f[3] >> 16);
      w2 = pk_be16(16, f[3]);
      return 18;
    case UFC_FRAME_HANDSHAKE_SYN_ACK:  // :475-514
      w0 |= pk_be32(1, f[0]) | pk(5, f[1] >> 24) | pk(6, f[1] >> 16) | pk(7, f[1] >> 8);
      w1 = pk(8, f[1]) | pk_be32(9, f[2]) | pk(13, f[3] >> 24) | pk(14, f[3] >> 16) | pk(15, f[3] >> 8);
      w2 = pk(16, f[3]) | pk_be32(17, f[4]);
      return 21;
    case UFC_FRAME_HANDSHAKE_ACK:  // :516-539
      w0 |= pk_be32(1, f[0]);
      return 5;
    case UFC_FRAME_HANDSHAKE_ERROR:  // :541-569
      w0 |= pk_be32(1, f[0]) | pk(5, info.aux);
      return 6;
    case UFC_FRAME_DATA:  // DataFrameBuilder::new and the count patched by build, build.rs:56-66, 148-149
      w0 |= pk_be32(1, f[0]) | pk(5, ((info.aux & 1u) << 7) | (info.item_count & 0x7Fu));
      return kDataHead;
    case UFC_FRAME_SYNC: {  // :623-657
      const uint32_t mode = info.aux & 3u;
      const uint32_t a = (mode & 1u) ? f[0] : 0u, b = (mode & 2u) ? f[1] : 0u;
      w0 |= pk(1, mode) | pk_be32(2, a) | pk_be16(6, b >> 16);
      w1 = pk_be16(8, b);
      return 10;
    }
    case UFC_FRAME_ACK:  // AckFrameBuilder::new and the count patched by build, build.rs:192-205, 231-234
      w0 |= pk_be32(1, f[0]) | pk(5, f[1] >> 24) | pk(6, f[1] >> 16) | pk(7, f[1] >> 8);
      w1 = pk(8, f[1]) | pk_be16(9, info.item_count);
      return kAckHead;
    default:  // disconnect, disconnect_ack (:571-611)
      return 1;
  }
}

// Status and encoded size (trailer included) of the frame `info` describes; `items` is the batch's item
// array of n_items records, src_base the offset in the payload buffer (payload_len bytes) that the
// frame's data_offsets are relative to.  size is 0 unless the status is UFC_BUILD_OK.
UFC_HD uint8_t check_frame(const ufc_frame_info& info, const ufc_item* items, uint64_t n_items, uint64_t src_base,
                           uint64_t payload_len, uint64_t& size) {
  size = 0;
  if (!info.ok) return UFC_BUILD_SKIPPED;
  switch (info.kind) {
    case UFC_FRAME_HANDSHAKE_SYN: size = kMaxFrameSize; return UFC_BUILD_OK;
    case UFC_FRAME_HANDSHAKE_SYN_ACK: size = 25; return UFC_BUILD_OK;
    case UFC_FRAME_HANDSHAKE_ACK: size = 9; return UFC_BUILD_OK;
    case UFC_FRAME_HANDSHAKE_ERROR:  // HandshakeErrorType has three values (:551-555)
      if (info.aux > 2) return UFC_BUILD_BAD_FIELD;
      size = 10;
      return UFC_BUILD_OK;
    case UFC_FRAME_DISCONNECT:
    case UFC_FRAME_DISCONNECT_ACK: size = 5; return UFC_BUILD_OK;
    case UFC_FRAME_SYNC:
      if (info.aux > 3) return UFC_BUILD_BAD_FIELD;
      size = 14;
      return UFC_BUILD_OK;
    case UFC_FRAME_ACK:
      if (info.item_count > 0xFFFFu || (uint64_t)info.item_first + info.item_count > n_items) return UFC_BUILD_BAD_FIELD;
      size = kAckHead + (uint64_t)UFC_ACK_GROUP_SIZE * info.item_count + 4;
      return UFC_BUILD_OK;
    case UFC_FRAME_DATA: {
      if (info.item_count > UFC_DATA_FRAME_MAX_DATAGRAM_COUNT || info.aux > 1 ||
          (uint64_t)info.item_first + info.item_count > n_items)
        return UFC_BUILD_BAD_FIELD;
      bool bad_field = false, bad_src = false;
      uint64_t s = kDataHead + 4;
      for (uint32_t k = 0; k < info.item_count; k++) {
        const ufc_item d = items[(uint64_t)info.item_first + k];
        bad_field = bad_field || !datagram_fields_ok(d);
        // the payload range [src_base + data_offset, + data_len) inside [0, payload_len)
        bad_src = bad_src || src_base > payload_len || (uint64_t)d.data_offset + d.data_len > payload_len - src_base;
        s += datagram_encoded_size(d);
      }
      if (bad_field) return UFC_BUILD_BAD_FIELD;
      if (bad_src) return UFC_BUILD_BAD_SRC;
      size = s;
      return UFC_BUILD_OK;
    }
    default:
      return UFC_BUILD_BAD_FIELD;  // unknown kind
  }
}

// Whether the build writes frame i: its status is OK, its span has the frame's size and lies inside
// both the batch's range [first, last) and the output buffer.
UFC_HD bool span_matches(uint8_t status, uint64_t size, uint64_t a, uint64_t b, uint64_t first, uint64_t last,
                         uint64_t out_len) {
  return status == UFC_BUILD_OK && b >= a && b - a == size && a >= first && b <= last && b <= out_len;
}

// ---- pack: DataFrameEmitter / AckFrameEmitter push and finalize (src/half_connection/emit.rs:47-125,
// 170-211), for the batched packs (host and GPU) ----
//
// A flush's frames are a greedy chain over its items' encoded sizes; flush_alloc and the frame window only
// cut that chain at one item, the stop.  With `starts` = the frames begun before item i and `bytes` = the
// encoded sizes of the flush's items before i, the emitter has spent (or, for the frame in progress, will
// have spent once it is finalized)
//   F(i) = H * starts + bytes
// when item i is pushed: `flush_alloc - frame_size < 0` of emit.rs:64, 176 and `flush_alloc < 0` of :83, 191
// are both flush_alloc < F(i).  F never decreases along a flush.
constexpr uint32_t kDataFrameOverhead = kDataHead + 4;  // DATA_FRAME_OVERHEAD: head + trailer
constexpr uint32_t kAckFrameOverhead = kAckHead + 4;    // ACK_FRAME_OVERHEAD
// Groups in a full ack frame, the ack chain's constant hop.
constexpr uint32_t kAckFrameMaxGroups = (kMaxFrameSize - kAckFrameOverhead) / UFC_ACK_GROUP_SIZE;

UFC_HD bool pack_is_ack(const ufc_flush& fl) { return fl.kind == UFC_FRAME_ACK; }  // any other kind packs as data
UFC_HD uint32_t pack_overhead(bool ack) { return ack ? kAckFrameOverhead : kDataFrameOverhead; }
// max_packet_count of emit.rs:61-62 (packet_id::SPAN / (2 MAX_FRAME_WINDOW_SIZE) = 2^20 / 8192 = 128, so
// DataFrameBuilder::MAX_COUNT decides); the ack emitter counts nothing.
UFC_HD uint32_t pack_max_count(bool ack) { return ack ? 0xFFFFFFFFu : (uint32_t)UFC_DATA_FRAME_MAX_DATAGRAM_COUNT; }
// Whether the frame in progress (size s with its overhead, c items) takes an item of e more bytes
// (emit.rs:69, 180).
UFC_HD bool pack_frame_takes(uint64_t s, uint32_t c, uint64_t e, uint32_t max_count) {
  return s + e <= kMaxFrameSize && c < max_count;
}
// The push of item i: UFC_PACK_DONE when it goes through, else why the flush stops there.  is_start: the item
// would begin a frame (the first item, or the frame in progress does not take it); F as above.
UFC_HD uint32_t pack_stop(const ufc_flush& fl, bool ack, uint64_t F, bool is_start, uint32_t starts) {
  if (fl.flush_alloc < (int64_t)F) return UFC_PACK_SIZE_LIMITED;                       // :64-68, :83-87, :176-179, :191-194
  if (is_start && !ack && starts >= fl.window_room) return UFC_PACK_WINDOW_LIMITED;  // :89-92, frame_queue.can_push()
  return UFC_PACK_DONE;
}
// The items a data frame that starts at item i takes when the flush does not end first: the largest m in
// 1..127 (and <= n_items - i) whose items fit a frame, at least the first item alone (emit.rs:94-109 makes no
// size check on it).  P(k) = the encoded sizes of items [0, k) summed, k <= n_items.
template <class Psum>
UFC_HD uint32_t pack_data_hop(const Psum& P, uint64_t i, uint64_t n_items) {
  const uint64_t left = n_items - i;
  uint32_t lo = 1, hi = left < UFC_DATA_FRAME_MAX_DATAGRAM_COUNT ? (uint32_t)left : (uint32_t)UFC_DATA_FRAME_MAX_DATAGRAM_COUNT;
  const uint64_t limit = P(i) + (kMaxFrameSize - kDataFrameOverhead);
  while (lo < hi) {  // at most 7 steps
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (P(i + mid) <= limit) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// The record of a flush's k-th frame, g-th of the batch, holding items [item_first, item_first + item_count).
UFC_HD ufc_frame_info pack_frame_info(const ufc_flush& fl, bool ack, uint32_t k, uint64_t g, const uint32_t* nonce_bits,
                                      uint64_t item_first, uint32_t item_count) {
  ufc_frame_info info{};
  info.kind = ack ? UFC_FRAME_ACK : UFC_FRAME_DATA;
  info.ok = 1;
  if (ack) {
    info.f[0] = fl.id0;
    info.f[1] = fl.id1;
  } else {
    info.f[0] = fl.id0 + k;  // frame_queue.next_id() of each frame in turn
    info.aux = nonce_bits ? (uint8_t)((nonce_bits[g >> 5] >> (g & 31u)) & 1u) : (uint8_t)0;
  }
  info.item_count = item_count;
  info.item_first = (uint32_t)item_first;
  return info;
}

// ---- emit: PacketSender::emit_packet (src/half_connection/packet_sender.rs:149-238) and PendingPacket::new /
// datagram (pending_packet.rs:23-42, 84-103), for the batched packet emits (host and GPU) ----
//
// Along one sender's queue, over its live packets (neither bad nor stale): the sequence id is next_id + rank
// (rank = live packets before it) and the allocation in front of it alloc + A (A = their alloc sizes summed).
// The window check fails from rank = room on and the allocation check from the first packet with
// A + a > max_alloc - alloc on; both never pass again further on, so the stop is the first packet that is bad
// or fails either.
enum EmitClass : uint32_t { kEmitBad = 0, kEmitStale = 1, kEmitLive = 2 };

// alloc_size (:16-22).
UFC_HD uint64_t emit_alloc_size(uint32_t len) {
  const uint64_t F = UFC_MAX_FRAGMENT_SIZE;
  return len > F ? (len + F - 1) / F * F : (uint64_t)len;
}
// num_fragments of PendingPacket::new (pending_packet.rs:25): an empty packet is one empty fragment.
UFC_HD uint32_t emit_fragment_count(uint32_t len) {
  return len ? (uint32_t)(((uint64_t)len + UFC_MAX_FRAGMENT_SIZE - 1) / UFC_MAX_FRAGMENT_SIZE) : 1u;
}
// A parent lead (:180-196): packet_id::sub, then `as u16`; 0 without a parent.
UFC_HD uint16_t emit_lead(uint32_t seq, uint32_t parent) {
  return parent == UFC_NO_PARENT ? (uint16_t)0 : (uint16_t)((seq - parent) & kPacketIdMask);
}
// Bad (what enqueue_packet debug-asserts, :139-141) before stale (:150-162).
UFC_HD uint32_t emit_packet_class(const ufc_packet& p, uint32_t flush_id) {
  if (p.channel_id >= UFC_MAX_CHANNELS || p.mode > UFC_SEND_RELIABLE || p.data_len > UFC_MAX_PACKET_SIZE) return kEmitBad;
  if (p.mode == UFC_SEND_TIME_SENSITIVE && p.flush_id != flush_id) return kEmitStale;
  return kEmitLive;
}
// max_alloc_ceil of PacketSender::new (:100), saturating.
UFC_HD uint64_t emit_max_alloc(uint64_t max_alloc) {
  const uint64_t r = max_alloc % UFC_MAX_FRAGMENT_SIZE;
  if (r == 0) return max_alloc;
  const uint64_t up = UFC_MAX_FRAGMENT_SIZE - r;
  return max_alloc > ~(uint64_t)0 - up ? ~(uint64_t)0 : max_alloc + up;
}
// Live packets the window still takes (:165-167): the check of the packet of rank r,
// ((next_id + r - base_id) & mask) >= window_size, fails exactly from r = room on (r < 2^31).  A window_size
// above the id mask never limits.
UFC_HD uint32_t emit_window_room(uint32_t base_id, uint32_t next_id, uint32_t window_size) {
  if (window_size > kPacketIdMask) return 0xFFFFFFFFu;
  const uint32_t d = (next_id - base_id) & kPacketIdMask;
  return d >= window_size ? 0u : window_size - d;
}
// alloc + A + a > max_alloc (:171), max_alloc already rounded, without overflow.
UFC_HD bool emit_alloc_fails(uint64_t alloc, uint64_t A, uint64_t a, uint64_t max_alloc) {
  if (alloc > max_alloc) return true;
  const uint64_t left = max_alloc - alloc;
  return A > left || a > left - A;
}
// Fragment f (<= last = emit_fragment_count(data_len) - 1) of an emitted packet (pending_packet.rs:84-103).
UFC_HD ufc_item emit_item(const ufc_packet& p, uint32_t seq, uint16_t window_parent_lead, uint16_t channel_parent_lead,
                          uint32_t f, uint32_t last) {
  ufc_item it{};
  it.id = seq;
  it.channel_id = p.channel_id;
  it.window_parent_lead = window_parent_lead;
  it.channel_parent_lead = channel_parent_lead;
  it.fragment_id = (uint16_t)f;
  it.fragment_id_last = (uint16_t)last;
  it.data_offset = p.data_offset + UFC_MAX_FRAGMENT_SIZE * f;
  it.data_len = f == last ? p.data_len - UFC_MAX_FRAGMENT_SIZE * f : (uint32_t)UFC_MAX_FRAGMENT_SIZE;
  const uint32_t hs = datagram_header_size(it);
  it.form = (uint8_t)(hs == 6 ? 0 : (hs == 9 ? 1 : 2));
  it.flags = datagram_is_valid(it) ? UFC_ITEM_VALID : 0;
  return it;
}

}  // namespace ufc_codec
