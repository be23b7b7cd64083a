// frame_codec_core.hpp -- the payload parse of Frame::read (everything after the CRC gate), written
// once for the host codec (frame_codec.cpp) and the GPU batch parse (frame_parse.hip); further down the
// encode for the batched builds (frame_build.hip), the emitters' arithmetic for the batched packs
// (frame_pack.hip), the packet sender's for the batched packet emits (packet_emit.hip), the packet receiver's
// step for the batched packet receives (packet_receive.hip), the frame window's for the batched frame windows
// (frame_window.hip), the sender's frame queue's for the batched frame queues (frame_queue.hip), the send rate
// control's (send_rate.hip), the resend's (resend.hip) and the flush control's (flush_ctl.hip).
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
#include "wave.hpp"

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

// ---- receive: PacketReceiver (src/half_connection/packet_receiver/mod.rs:142-435), AssemblyWindow
// (assembly_window/mod.rs:69-199) and FragmentBuffer (fragment_buffer.rs:12-57), for the batched packet receives
// (host: frame_codec.cpp; GPU: packet_receive.hip) ----
//
// Both forms run the same three passes over caller-owned state:
//   walk    per receiver, serial: the step (resynchronize, handle_datagram per item, receive) on the header and
//           the slots in place; a plan record per slot remembers what the copy needs (where the slot's bytes
//           were on entry, whether its packet was assembled in this step, its place in the delivery order); three
//           counts per receiver: delivered packets, delivered bytes, carry bytes;
//   (exclusive sums of the counts over the receivers: packet_first, the out offsets, carry_first)
//   finish  per receiver: the records, the slots' new data_offset, the received-bits words, and one copy segment
//           per stored datagram and two per slot (held packet, fragment buffer) with absolute offsets;
//   copy    the slots' segments, then the datagrams' (a new fragment overwrites the unspecified bytes a carried
//           fragment buffer has in its place).

// packet_id::sub / add (src/packet_id.rs).
UFC_HD uint32_t packet_id_sub(uint32_t a, uint32_t b) { return (a - b) & kPacketIdMask; }
UFC_HD uint32_t packet_id_add(uint32_t a, uint32_t b) { return (a + b) & kPacketIdMask; }
// packet_alloc_size (assembly_window/mod.rs:53-60).
UFC_HD uint64_t packet_alloc_size(uint32_t fragment_id_last, uint32_t data_len) {
  return fragment_id_last ? ((uint64_t)fragment_id_last + 1) * UFC_MAX_FRAGMENT_SIZE : (uint64_t)data_len;
}
// "The parent is not in the way": lead == 0 || lead > delta (mod.rs:206, 214, 336, 385).
UFC_HD bool lead_clears(uint32_t lead, uint32_t delta) { return lead == 0 || lead > delta; }
// alloc + a > max_alloc (assembly_window/mod.rs:95), max_alloc already rounded, without overflow.
UFC_HD bool rx_alloc_fails(uint64_t alloc, uint64_t a, uint64_t max_alloc) {
  return alloc > max_alloc || a > max_alloc - alloc;
}
UFC_HD uint64_t align8(uint64_t v) { return (v + 7) & ~(uint64_t)7; }
// A FragmentBuffer of n fragments in the carry: n * 1448 data bytes, then ceil(n / 64) words.
UFC_HD uint64_t rx_frag_data_bytes(uint32_t n) { return (uint64_t)n * UFC_MAX_FRAGMENT_SIZE; }
UFC_HD uint64_t rx_frag_bytes(uint32_t n) { return rx_frag_data_bytes(n) + 8ull * ((n + 63) / 64); }
UFC_HD uint32_t rx_slot_held(const ufc_rx_slot& s) {
  return (s.rx_flags & (UFC_RX_SLOT_DATA | UFC_RX_SLOT_DUD)) == UFC_RX_SLOT_DATA ? s.data_len : 0u;
}
UFC_HD uint32_t rx_slot_nfrag(const ufc_rx_slot& s) {
  return s.asm_state == UFC_RX_ASM_ACTIVE ? (uint32_t)s.asm_last_fragment_id + 1 : 0u;
}
// A slot's region in the carry.
UFC_HD uint64_t rx_slot_region(const ufc_rx_slot& s) {
  const uint32_t n = rx_slot_nfrag(s);
  return align8(rx_slot_held(s)) + (n ? rx_frag_bytes(n) : 0);
}

struct RxArgs {
  const ufc_frame_info* infos;
  uint64_t n_frames;
  const uint8_t* frame_accept;  // nullable
  const ufc_item* items;
  uint64_t n_items;
  const uint64_t* src_base;  // nullable
  const uint8_t* payload;
  uint64_t payload_len;
  const uint64_t* frame_first;
  const ufc_receiver* receivers;
  uint64_t n_receivers;
  ufc_rx_slot* slots;
  const uint64_t* slot_first;
  uint64_t n_slots;
  const uint8_t* carry_in;
  uint64_t carry_in_len;
  uint8_t* carry_out;
  uint64_t carry_cap;
  uint64_t* carry_first;
  uint64_t* carry_used;
  ufc_rx_packet* packets;
  uint64_t packets_cap;
  uint64_t* packet_first;
  uint64_t* packets_used;
  uint8_t* out_bytes;
  uint64_t out_cap;
  uint64_t* out_used;
  uint8_t* item_status;  // nullable
  ufc_receiver_result* results;
  ufc_receiver* receivers_out;
};
// The argument contracts of the batched calls from here on, each stated once for its host entry (frame_codec.cpp)
// and its device entry (ufc_api.cpp): a required pointer is set, an array with a non-zero count is set, and every
// count that is scanned or indexed with 32 bits lies below kCountLim.  Host code.  An entry asks after its own two
// answers: a missing context is an error (device entries), and an empty batch is UFC_OK whatever the pointers.
constexpr uint64_t kCountLim = ((uint64_t)1 << 31) - 1;
inline bool rx_args_ok(const RxArgs& a) {
  const bool bad = !a.frame_first || !a.receivers || !a.receivers_out || !a.slot_first || !a.carry_first ||
                   !a.carry_used || !a.packet_first || !a.packets_used || !a.out_used || !a.results ||
                   (!a.infos && a.n_frames) || (!a.items && a.n_items) || (!a.payload && a.payload_len) ||
                   (!a.slots && a.n_slots) || (!a.carry_in && a.carry_in_len) || (!a.carry_out && a.carry_cap) ||
                   (!a.packets && a.packets_cap) || (!a.out_bytes && a.out_cap) || a.n_frames >= kCountLim ||
                   a.n_items >= kCountLim || a.n_receivers >= kCountLim || a.n_slots >= kCountLim ||
                   ((uintptr_t)a.carry_in & 7) || ((uintptr_t)a.carry_out & 7);  // (the bit words are read as uint64)
  return !bad;
}

// What the copy needs to know of a slot (48 bytes).
enum RxPlanFlags : uint32_t {
  kRxHeldIn = 1,        // the receive-window packet's bytes are the ones held in carry_in
  kRxAsmCarry = 2,      // the fragment buffer in carry_in feeds this step's assembly
  kRxCompletedNow = 4,  // the receive-window packet was assembled in this step
  kRxPktOut = 8,        // finish: the packet's bytes go to out_bytes at pkt_dst ...
  kRxPktCarry = 16,     // ... or to carry_out
  kRxFrag = 32          // finish: ACTIVE afterwards, its buffer at frag_dst in carry_out
};
constexpr uint32_t kRxNotDelivered = 0xFFFFFFFFu;
struct RxPlan {
  uint64_t in_offset;   // the slot's region in carry_in on entry
  uint64_t pkt_dst;     // walk: a delivered packet's bytes relative to the receiver's first; finish: absolute
  uint64_t frag_dst;
  uint32_t in_held_len, in_nfrag;
  uint32_t deliver_idx;  // place in the receiver's delivery order, or kRxNotDelivered
  uint32_t seq, len;     // the delivered packet
  uint8_t flags, channel, pkt_flags, pad;
};
static_assert(sizeof(RxPlan) == 48, "plan record");

// One copy: len bytes from payload (kRxSrcCarry clear) or carry_in to out_bytes (kRxDstCarry clear) or
// carry_out, clipped at the destination's cap by the copy.
constexpr uint32_t kRxSrcCarry = 1, kRxDstCarry = 2;
struct RxSegment {
  uint64_t src, dst;
  uint32_t len, kinds;
};
static_assert(sizeof(RxSegment) == 24, "segment record");
// Segment indices: two per slot first (they are copied first), then one per datagram.
UFC_HD uint64_t rx_slot_segment(uint64_t slot, uint32_t which) { return 2 * slot + which; }
UFC_HD uint64_t rx_item_segment(uint64_t n_slots, uint64_t g) { return 2 * n_slots + g; }

// First arrivals per (receiver, slot, fragment) within a step: an open-addressed table of at least twice as
// many entries as there are datagrams (a power of two), zeroed before the walk.  Receivers insert concurrently.
struct RxDupSet {
  unsigned long long* table;
  uint64_t mask;
  // true: the key was new.
  UFC_HD bool insert(uint64_t r, uint32_t slot, uint32_t fragment) const {
    const unsigned long long key = ((unsigned long long)r << 28 | (unsigned long long)slot << 16 | fragment) + 1;
    uint64_t h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    for (uint64_t i = h & mask;; i = (i + 1) & mask) {
#if defined(__HIP_DEVICE_COMPILE__)
      const unsigned long long old = atomicCAS(&table[i], 0ull, key);
#else
      unsigned long long old = 0;
      __atomic_compare_exchange_n(&table[i], &old, key, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
      if (old == 0) return true;
      if (old == key) return false;
    }
  }
};
UFC_HD uint64_t rx_dup_entries(uint64_t n_items) {
  uint64_t c = 64;
  while (c < 2 * n_items) c <<= 1;
  return c;
}

// Whether frame i of the batch counts (its datagrams are handled).
UFC_HD bool rx_frame_counts(const RxArgs& a, uint64_t i) {
  const ufc_frame_info& f = a.infos[i];
  return f.ok && f.kind == UFC_FRAME_DATA && (!a.frame_accept || a.frame_accept[i] != 0);
}

// AssemblyWindow::clear (assembly_window/mod.rs:185-198) of one slot.
UFC_HD void rx_clear_slot(ufc_rx_slot& s, RxPlan& p, uint64_t& alloc) {
  if (s.asm_state == UFC_RX_ASM_CLOSED) {
    alloc -= s.asm_size;
  } else if (s.asm_state == UFC_RX_ASM_ACTIVE) {
    alloc -= rx_frag_data_bytes((uint32_t)s.asm_last_fragment_id + 1);
    p.flags &= (uint8_t)~kRxAsmCarry;  // the buffer goes with it
  }
  s.asm_state = UFC_RX_ASM_OPEN;
  s.asm_size = 0;
  s.asm_window_parent_lead = s.asm_channel_parent_lead = s.asm_last_fragment_id = s.asm_received = 0;
  s.asm_channel_id = 0;
}

// advance_window (mod.rs:244-282) on the receiver's working header R (in receivers_out).
inline __host__ __device__ void rx_advance_window(ufc_receiver& R, ufc_rx_slot* slots, RxPlan* plan, uint32_t new_base,
                                                  uint32_t& advanced) {
  const uint32_t mask = R.window_size - 1;
  const uint32_t delta = packet_id_sub(new_base, R.base_id);
  if (packet_id_sub(R.end_id, R.base_id) < delta) R.end_id = new_base;
  uint64_t alloc = R.alloc;
  for (uint32_t id = R.base_id; id != new_base; id = packet_id_add(id, 1)) {
    ufc_rx_slot& s = slots[id & mask];
    s.rx_flags &= (uint8_t)~UFC_RX_SLOT_ENTRY;
    rx_clear_slot(s, plan[id & mask], alloc);
  }
  R.alloc = alloc;
  // try_unset_channel_base_id over (base, new_base]: the channels whose base lead is in 1..=delta.
  for (uint32_t c = 0; c < UFC_MAX_CHANNELS; c++) {
    const uint32_t cb = R.channel_base_id[c];
    if (cb == UFC_NO_PARENT) continue;
    const uint32_t lead = packet_id_sub(cb, R.base_id);
    if (lead >= 1 && lead <= delta) R.channel_base_id[c] = UFC_NO_PARENT;
  }
  advanced += delta;
  R.base_id = new_base;
}

// The step of receiver r in four parts, run one after the other by rx_walk (the host form, and the fallback of the
// device form) and by separate launches on the device: begin (the state check, the plan records, resynchronize),
// items (handle_datagram per item), receive (delivery and the window advance; serial here, in tiles of 64 ids in
// rx_receive_tiles below) and end (the carry size, the counts).  R = a.receivers_out[r] already holds a copy of
// the input header.  status: one byte per item (a.item_status or scratch of the same size).  begin returns false
// for BAD_STATE (nothing done but the result, and the other parts do nothing).
inline __host__ __device__ bool rx_walk_begin(const RxArgs& a, uint64_t r, RxPlan* plans) {
  ufc_receiver& R = a.receivers_out[r];
  ufc_receiver_result& res = a.results[r];  // (counted in place: no indexed array of the thread's own)
  res = ufc_receiver_result{};
  const uint32_t W = R.window_size;
  const uint64_t ff0 = a.frame_first[r], ff1 = a.frame_first[r + 1];
  const uint64_t s0 = a.slot_first[r], s1 = a.slot_first[r + 1];
  bool bad = W == 0 || W > 4096 || (W & (W - 1)) != 0 || R.base_id > kPacketIdMask || R.end_id > kPacketIdMask ||
             ff0 > ff1 || ff1 > a.n_frames || s0 > s1 || s1 > a.n_slots || s1 - s0 < W;
  for (uint64_t i = ff0; !bad && i < ff1; i++) {
    const ufc_frame_info& f = a.infos[i];
    if (f.ok && (uint64_t)f.item_first + f.item_count > a.n_items) bad = true;
  }
  ufc_rx_slot* slots = a.slots + s0;
  RxPlan* plan = plans + s0;
  for (uint32_t j = 0; !bad && j < W; j++) {
    const ufc_rx_slot& s = slots[j];
    const uint64_t region = rx_slot_region(s);
    if (s.asm_state > UFC_RX_ASM_ACTIVE || s.asm_channel_id >= UFC_MAX_CHANNELS || s.rx_channel_id >= UFC_MAX_CHANNELS ||
        (region && ((s.data_offset & 7) || s.data_offset > a.carry_in_len || region > a.carry_in_len - s.data_offset)))
      bad = true;
  }
  if (bad) {
    res.stop = UFC_RX_BAD_STATE;
    return false;
  }
  const uint32_t mask = W - 1;
  for (uint32_t j = 0; j < W; j++) {
    const ufc_rx_slot& s = slots[j];
    RxPlan p{};
    p.in_offset = s.data_offset;
    p.in_held_len = rx_slot_held(s);
    p.in_nfrag = rx_slot_nfrag(s);
    p.flags = (uint8_t)((p.in_held_len ? kRxHeldIn : 0) | (p.in_nfrag ? kRxAsmCarry : 0));
    p.deliver_idx = kRxNotDelivered;
    plan[j] = p;
  }

  // 1. resynchronize (mod.rs:408-435).
  if (R.resync_id != UFC_NO_PARENT) {
    const uint32_t next = R.resync_id & kPacketIdMask;
    if (packet_id_sub(next, R.base_id) <= W) {
      uint32_t id = R.base_id;
      while (id != next && !(slots[id & mask].rx_flags & UFC_RX_SLOT_ENTRY)) id = packet_id_add(id, 1);
      rx_advance_window(R, slots, plan, id, res.advanced);
    }
  }
  res.stop = UFC_RX_DONE;
  return true;
}

// The verdicts of handle_datagram that do not depend on the order of arrival: base_id and the channel bases are
// constant while a step's datagrams are handled (they change in receive() only), so validity, the payload
// range, the window test (mod.rs:162) and the channel test (:167) are a function of the item alone.  Returns the
// item's status, or kRxToAssembly for a datagram that goes on to try_add.
constexpr uint8_t kRxToAssembly = 0xFF;
UFC_HD uint8_t rx_item_verdict(const RxArgs& a, const ufc_receiver& R, const ufc_item& it, uint64_t sb) {
  if (!datagram_is_valid(it) || it.id > kPacketIdMask) return UFC_RX_DROPPED_INVALID;
  if (sb > a.payload_len || it.data_offset > a.payload_len - sb || it.data_len > a.payload_len - sb - it.data_offset)
    return UFC_RX_DROPPED_BAD_SRC;
  const uint32_t base = R.base_id, cb = R.channel_base_id[it.channel_id];
  const uint32_t cbid = cb != UFC_NO_PARENT ? cb : base;
  const uint32_t packet_lead = packet_id_sub(it.id, base);
  if (packet_lead >= R.window_size) return UFC_RX_DROPPED_WINDOW;
  if (packet_lead < packet_id_sub(cbid, base)) return UFC_RX_DROPPED_CHANNEL;
  return kRxToAssembly;
}
// The verdicts of frame i of receiver r, into status (the item-parallel pass of the device form: any lane may
// take any frame of a receiver whose begin passed).
UFC_HD void rx_frame_verdicts(const RxArgs& a, uint64_t r, uint64_t i, uint8_t* verdicts) {
  const ufc_frame_info& f = a.infos[i];
  if (!f.ok) return;
  const bool counts_ = rx_frame_counts(a, i);
  const uint64_t sb = a.src_base ? a.src_base[i] : 0;
  for (uint64_t g = f.item_first, ge = (uint64_t)f.item_first + f.item_count; g < ge; g++)
    verdicts[g] = counts_ ? rx_item_verdict(a, a.receivers_out[r], a.items[g], sb) : (uint8_t)UFC_RX_NOT_HANDLED;
}

// 2. handle_datagram (mod.rs:142-218) over try_add (assembly_window/mod.rs:83-183).  pre (nullable): one byte per
// item, rx_frame_verdicts' result for every item of the receiver's frames (its own array, not status: frames of
// one receiver that share items, which no parse produces, then still get the serial walk's answer).
inline __host__ __device__ void rx_walk_items(const RxArgs& a, uint64_t r, RxPlan* plans, uint8_t* status,
                                              const RxDupSet& dups, const uint8_t* pre) {
  ufc_receiver& R = a.receivers_out[r];
  ufc_receiver_result& res = a.results[r];
  if (res.stop != UFC_RX_DONE) return;
  const uint32_t W = R.window_size, mask = W - 1;
  const uint64_t ff0 = a.frame_first[r], ff1 = a.frame_first[r + 1];
  ufc_rx_slot* slots = a.slots + a.slot_first[r];
  RxPlan* plan = plans + a.slot_first[r];
  const uint64_t max_alloc = emit_max_alloc(R.max_alloc);
  const uint32_t base = R.base_id;
  for (uint64_t i = ff0; i < ff1; i++) {
    const ufc_frame_info& f = a.infos[i];
    if (!f.ok) continue;
    const bool counts_ = rx_frame_counts(a, i);
    const uint64_t sb = a.src_base ? a.src_base[i] : 0;
    for (uint64_t g = f.item_first, ge = (uint64_t)f.item_first + f.item_count; g < ge; g++) {
      if (!counts_) {
        status[g] = UFC_RX_NOT_HANDLED;
        res.status_count[UFC_RX_NOT_HANDLED]++;
        continue;
      }
      uint8_t st = pre ? pre[g] : kRxToAssembly;
      if (pre && st != kRxToAssembly) {  // dropped by the verdict pass: the item itself is not read again
        if (st >= UFC_RX_STATUS_COUNT) st = UFC_RX_NOT_HANDLED;  // (only where receivers share frames: unspecified)
        status[g] = st;
        res.status_count[st]++;
        continue;
      }
      const ufc_item it = a.items[g];
      if (!pre) st = rx_item_verdict(a, R, it, sb);
      bool packet = false, dud = false;
      uint32_t packet_len = 0;
      const uint32_t ch = it.channel_id;
      if (st == kRxToAssembly) {
        const uint32_t cbid = R.channel_base_id[ch] != UFC_NO_PARENT ? R.channel_base_id[ch] : base;
        const uint32_t packet_lead = packet_id_sub(it.id, base);
        {
          const uint32_t idx = it.id & mask;
          ufc_rx_slot& s = slots[idx];
          RxPlan& p = plan[idx];
          if (s.asm_state == UFC_RX_ASM_OPEN) {
            const uint64_t a_sz = packet_alloc_size(it.fragment_id_last, it.data_len);
            if (rx_alloc_fails(R.alloc, a_sz, max_alloc)) {
              s.asm_state = UFC_RX_ASM_CLOSED;
              s.asm_size = 0;
              st = UFC_RX_DUD;
              packet = dud = true;
            } else {
              R.alloc += a_sz;
              if (it.fragment_id_last == 0) {
                s.asm_state = UFC_RX_ASM_CLOSED;
                s.asm_size = (uint32_t)a_sz;
                st = UFC_RX_COMPLETED;
                packet = true;
                packet_len = it.data_len;
              } else {
                s.asm_state = UFC_RX_ASM_ACTIVE;
                s.asm_channel_id = it.channel_id;
                s.asm_window_parent_lead = it.window_parent_lead;
                s.asm_channel_parent_lead = it.channel_parent_lead;
                s.asm_last_fragment_id = it.fragment_id_last;
                s.asm_received = 1;
                s.asm_size = it.data_len;
                (void)dups.insert(r, idx, it.fragment_id);
                st = UFC_RX_STORED;
              }
            }
          } else if (s.asm_state == UFC_RX_ASM_CLOSED) {
            st = UFC_RX_DROPPED_CLOSED;
          } else if (it.channel_id != s.asm_channel_id || it.window_parent_lead != s.asm_window_parent_lead ||
                     it.channel_parent_lead != s.asm_channel_parent_lead ||
                     it.fragment_id_last != s.asm_last_fragment_id) {
            st = UFC_RX_DROPPED_MISMATCH;
          } else {
            const uint32_t n = (uint32_t)s.asm_last_fragment_id + 1;
            bool seen = false;
            if (p.flags & kRxAsmCarry) {  // the bits received before this step
              const uint64_t words = p.in_offset + align8(p.in_held_len) + rx_frag_data_bytes(n);
              const uint64_t w = *(const uint64_t*)(a.carry_in + words + 8ull * (it.fragment_id >> 6));
              seen = (w >> (it.fragment_id & 63u)) & 1u;
            }
            if (seen || !dups.insert(r, idx, it.fragment_id)) {
              st = UFC_RX_DROPPED_DUPLICATE;
            } else {
              const uint32_t received = (uint32_t)s.asm_received + 1;
              s.asm_size += it.data_len;
              if (received == n) {
                packet = true;
                packet_len = s.asm_size;
                s.asm_state = UFC_RX_ASM_CLOSED;  // Closed(alloc_size): the opener's fields go with the entry
                s.asm_size = (uint32_t)rx_frag_data_bytes(n);
                s.asm_window_parent_lead = s.asm_channel_parent_lead = s.asm_last_fragment_id = s.asm_received = 0;
                s.asm_channel_id = 0;
                st = UFC_RX_COMPLETED;
              } else {
                s.asm_received = (uint16_t)received;
                st = UFC_RX_STORED;
              }
            }
          }
          if (packet) {  // mod.rs:177-216
            s.rx_channel_id = it.channel_id;
            s.rx_channel_parent_lead = it.channel_parent_lead;
            s.rx_window_parent_lead = it.window_parent_lead;
            s.rx_flags = (uint8_t)(UFC_RX_SLOT_ENTRY | UFC_RX_SLOT_DATA | (dud ? UFC_RX_SLOT_DUD : 0));
            s.data_len = packet_len;
            p.flags = (uint8_t)((p.flags & ~(kRxHeldIn | kRxCompletedNow)) | (dud ? 0 : kRxCompletedNow));
            if (packet_id_sub(it.id, R.end_id) < W) R.end_id = packet_id_add(it.id, 1);
            R.channel_packet_count[ch]++;
            if (lead_clears(it.channel_parent_lead, packet_id_sub(it.id, cbid))) R.channel_ready_flags |= 1ull << ch;
            if (lead_clears(it.window_parent_lead, packet_lead)) R.window_ready = 1;
            if (dud) res.packets_dud++; else res.packets_completed++;
          }
        }
      }
      status[g] = st;
      res.status_count[st]++;
    }
  }

}

// 3. receive (mod.rs:286-402), id by id.  delivered and out_bytes: the packets and bytes it delivers.
inline __host__ __device__ void rx_receive_serial(const RxArgs& a, uint64_t r, RxPlan* plans, uint32_t& delivered,
                                                  uint64_t& out_bytes) {
  ufc_receiver& R = a.receivers_out[r];
  ufc_receiver_result& res = a.results[r];
  delivered = 0;
  out_bytes = 0;
  if (res.stop != UFC_RX_DONE) return;
  const uint32_t mask = R.window_size - 1, base = R.base_id;
  ufc_rx_slot* slots = a.slots + a.slot_first[r];
  RxPlan* plan = plans + a.slot_first[r];
  if (R.deliver) {
    const uint32_t end = R.end_id;
    for (uint32_t seq = base; seq != end && R.channel_ready_flags != 0; seq = packet_id_add(seq, 1)) {
      ufc_rx_slot& s = slots[seq & mask];
      if (!(s.rx_flags & UFC_RX_SLOT_DATA)) continue;
      const uint32_t ch = s.rx_channel_id;
      const uint64_t bit = 1ull << ch;
      if (!(R.channel_ready_flags & bit)) continue;
      const uint32_t cbid = R.channel_base_id[ch] != UFC_NO_PARENT ? R.channel_base_id[ch] : base;
      if (lead_clears(s.rx_channel_parent_lead, packet_id_sub(seq, cbid))) {
        RxPlan& p = plan[seq & mask];
        const bool dud = (s.rx_flags & UFC_RX_SLOT_DUD) != 0;
        p.deliver_idx = delivered++;
        p.seq = seq;
        p.len = dud ? 0u : s.data_len;
        p.channel = (uint8_t)ch;
        p.pkt_flags = dud ? UFC_RX_PACKET_DUD : 0;
        p.pkt_dst = out_bytes;
        out_bytes += p.len;
        s.rx_flags &= (uint8_t)~(UFC_RX_SLOT_DATA | UFC_RX_SLOT_DUD);
        s.data_len = 0;
        if (--R.channel_packet_count[ch] == 0) R.channel_ready_flags &= ~bit;
        R.channel_base_id[ch] = packet_id_add(seq, 1);  // set_channel_base_id
      } else {
        R.channel_ready_flags &= ~bit;
      }
    }
    if (R.window_ready) {
      R.window_ready = 0;
      uint32_t new_base = base;
      for (uint32_t seq = base; seq != end; seq = packet_id_add(seq, 1)) {
        const ufc_rx_slot& s = slots[seq & mask];
        if (s.rx_flags & UFC_RX_SLOT_ENTRY) {
          if (!lead_clears(s.rx_window_parent_lead, packet_id_sub(seq, new_base))) break;
          new_base = packet_id_add(seq, 1);
        }
      }
      rx_advance_window(R, slots, plan, new_base, res.advanced);
    }
  }
}

// 3. receive (mod.rs:286-402) in tiles of 64 consecutive ids, one lane per id: the form the device runs, one wave
// per receiver.  Written once against a wave policy Wv so that the same text runs as host code (a loop over the
// lanes per phase: tests/c/receive_host_check.hip, against rx_receive_serial) and on the device (every lane runs
// each phase, a wave barrier in between):
//   Wv::lanes(f)       f(lane) for the 64 lanes; what the lanes wrote to `sh` before is visible to all after
//   Wv::or64 / add64   atomic on the device (vector atomics on LDS), plain on the host
// Delivery: per channel the delivered packets are a prefix of its DATA slots in id order.  A lane evaluates its
// slot's test with the channel base taken as (the previous DATA lane of its channel) + 1, or the carried base
// for the first; the lanes of a channel meet in a 64-bit lane mask per channel (all DATA lanes, and the failing
// ones); a lane is delivered when its channel was ready, no lane of the channel at or below it fails, and the
// packet count has not run out before it (the k-th delivery clears the ready flag when it takes the count to
// zero).  Lane c then settles channel c: count, base, ready flag.  The delivery order is the id order: a rank
// among the delivered lanes, the bytes' offsets a sum over the lanes below.  The window advance is the same shape
// over the ENTRY slots with new_base in the place of the channel base, and stops at the first failing lane;
// advance_window then clears its slots lane by lane.  More ids than window_size between base and end (state
// no consistent run produces) go to rx_receive_serial, as does nothing else.
struct RxWaveShared {
  unsigned long long chan_mask[UFC_MAX_CHANNELS], chan_fail[UFC_MAX_CHANNELS];
  uint32_t chan_base[UFC_MAX_CHANNELS], chan_count[UFC_MAX_CHANNELS];
  uint32_t chan_ready[UFC_MAX_CHANNELS];
  uint32_t lane_len[64];
  unsigned long long deliv_mask, entry_mask, entry_fail, ready_bits, alloc_sub, out_bytes;
  uint32_t delivered, new_base, stop;
};
template <class Wv>
inline __host__ __device__ void rx_receive_tiles(const Wv& wv, RxWaveShared& sh, const RxArgs& a, uint64_t r, RxPlan* plans,
                                                 uint32_t& delivered, uint64_t& out_bytes) {
  ufc_receiver& R = a.receivers_out[r];
  ufc_receiver_result& res = a.results[r];
  delivered = 0;
  out_bytes = 0;
  if (res.stop != UFC_RX_DONE || !R.deliver) return;
  const uint32_t W = R.window_size, mask = W - 1, base = R.base_id, end = R.end_id;
  const uint32_t n = packet_id_sub(end, base);
  if (n > W) {  // (every lane takes this branch or none)
    wv.lanes([&](uint32_t lane) {
      if (lane == 0) {
        uint32_t d;
        uint64_t o;
        rx_receive_serial(a, r, plans, d, o);
        sh.delivered = d;
        sh.out_bytes = o;
      }
    });
    delivered = sh.delivered;
    out_bytes = sh.out_bytes;
    return;
  }
  ufc_rx_slot* slots = a.slots + a.slot_first[r];
  RxPlan* plan = plans + a.slot_first[r];
  const uint64_t ready_in = R.channel_ready_flags;
  const bool window_ready = R.window_ready != 0;
  wv.lanes([&](uint32_t c) {
    sh.chan_base[c] = R.channel_base_id[c];
    sh.chan_count[c] = R.channel_packet_count[c];
    sh.chan_ready[c] = (uint32_t)((ready_in >> c) & 1u);
    sh.chan_mask[c] = sh.chan_fail[c] = 0;
    if (c == 0) sh.deliv_mask = sh.ready_bits = sh.alloc_sub = sh.out_bytes = 0, sh.delivered = 0;
  });
  auto below = [](uint32_t lane) { return (1ull << lane) - 1; };
  for (uint32_t t0 = 0; t0 < n; t0 += 64) {
    const uint32_t nv = n - t0 < 64 ? n - t0 : 64;
    auto seq_of = [&](uint32_t lane) { return packet_id_add(base, t0 + lane); };
    wv.lanes([&](uint32_t lane) {
      sh.lane_len[lane] = 0;
      if (lane >= nv) return;
      const ufc_rx_slot& s = slots[seq_of(lane) & mask];
      if (s.rx_flags & UFC_RX_SLOT_DATA) Wv::or64(&sh.chan_mask[s.rx_channel_id], 1ull << lane);
    });
    wv.lanes([&](uint32_t lane) {
      if (lane >= nv) return;
      const ufc_rx_slot& s = slots[seq_of(lane) & mask];
      if (!(s.rx_flags & UFC_RX_SLOT_DATA)) return;
      const uint32_t c = s.rx_channel_id;
      const unsigned long long m = sh.chan_mask[c] & below(lane);
      const uint32_t cb = m ? packet_id_add(seq_of(high_bit(m)), 1) : (sh.chan_base[c] != UFC_NO_PARENT ? sh.chan_base[c] : base);
      if (!lead_clears(s.rx_channel_parent_lead, packet_id_sub(seq_of(lane), cb))) Wv::or64(&sh.chan_fail[c], 1ull << lane);
    });
    wv.lanes([&](uint32_t lane) {
      if (lane >= nv) return;
      const ufc_rx_slot& s = slots[seq_of(lane) & mask];
      if (!(s.rx_flags & UFC_RX_SLOT_DATA)) return;
      const uint32_t c = s.rx_channel_id, count = sh.chan_count[c];
      const uint32_t rank = popc(sh.chan_mask[c] & below(lane));
      if (sh.chan_ready[c] && !(sh.chan_fail[c] & (below(lane) | 1ull << lane)) && (count == 0 || rank < count)) {
        Wv::or64(&sh.deliv_mask, 1ull << lane);
        sh.lane_len[lane] = (s.rx_flags & UFC_RX_SLOT_DUD) ? 0u : s.data_len;
      }
    });
    wv.lanes([&](uint32_t lane) {
      if (!((sh.deliv_mask >> lane) & 1u)) return;
      ufc_rx_slot& s = slots[seq_of(lane) & mask];
      RxPlan& p = plan[seq_of(lane) & mask];
      const bool dud = (s.rx_flags & UFC_RX_SLOT_DUD) != 0;
      uint64_t at = sh.out_bytes;
      for (uint32_t l = 0; l < lane; l++) at += sh.lane_len[l];
      p.deliver_idx = sh.delivered + popc(sh.deliv_mask & below(lane));
      p.seq = seq_of(lane);
      p.len = sh.lane_len[lane];
      p.channel = s.rx_channel_id;
      p.pkt_flags = dud ? UFC_RX_PACKET_DUD : 0;
      p.pkt_dst = at;
      s.rx_flags &= (uint8_t)~(UFC_RX_SLOT_DATA | UFC_RX_SLOT_DUD);
      s.data_len = 0;
    });
    wv.lanes([&](uint32_t c) {  // lane c settles channel c
      const unsigned long long M = sh.chan_mask[c], F = sh.chan_fail[c];
      if (sh.chan_ready[c] && M) {
        const uint32_t count = sh.chan_count[c];
        const uint32_t clear = F ? popc(M & below(low_bit(F))) : popc(M);  // DATA lanes before the first failing one
        const uint32_t nd = (count != 0 && clear > count) ? count : clear;
        if ((count != 0 && nd == count) || (F && (count == 0 || clear < count))) sh.chan_ready[c] = 0;
        sh.chan_count[c] = count - nd;
        if (nd) {
          unsigned long long m = M;
          for (uint32_t k = 1; k < nd; k++) m &= m - 1;  // drop the nd - 1 lowest: the nd-th DATA lane is the lowest left
          sh.chan_base[c] = packet_id_add(seq_of(low_bit(m)), 1);
        }
      }
      sh.chan_mask[c] = sh.chan_fail[c] = 0;
    });
    wv.lanes([&](uint32_t lane) {
      if (lane != 0) return;
      sh.delivered += popc(sh.deliv_mask);
      for (uint32_t l = 0; l < 64; l++) sh.out_bytes += sh.lane_len[l];
      sh.deliv_mask = 0;
    });
  }
  wv.lanes([&](uint32_t c) {
    R.channel_base_id[c] = sh.chan_base[c];
    R.channel_packet_count[c] = sh.chan_count[c];
    if (sh.chan_ready[c]) Wv::or64(&sh.ready_bits, 1ull << c);
  });
  delivered = sh.delivered;
  out_bytes = sh.out_bytes;
  if (!window_ready) {
    wv.lanes([&](uint32_t lane) {
      if (lane == 0) R.channel_ready_flags = sh.ready_bits;
    });
    return;
  }
  // the window advance: the ENTRY slots' prefix, then advance_window (mod.rs:244-282) lane by lane
  wv.lanes([&](uint32_t lane) {
    if (lane == 0) sh.new_base = base, sh.stop = 0, sh.entry_mask = sh.entry_fail = 0;
  });
  for (uint32_t t0 = 0; t0 < n; t0 += 64) {
    const uint32_t nv = n - t0 < 64 ? n - t0 : 64;
    auto seq_of = [&](uint32_t lane) { return packet_id_add(base, t0 + lane); };
    wv.lanes([&](uint32_t lane) {
      if (lane < nv && (slots[seq_of(lane) & mask].rx_flags & UFC_RX_SLOT_ENTRY)) Wv::or64(&sh.entry_mask, 1ull << lane);
    });
    wv.lanes([&](uint32_t lane) {
      if (!((sh.entry_mask >> lane) & 1u)) return;
      const unsigned long long m = sh.entry_mask & below(lane);
      const uint32_t nb = m ? packet_id_add(seq_of(high_bit(m)), 1) : sh.new_base;
      if (!lead_clears(slots[seq_of(lane) & mask].rx_window_parent_lead, packet_id_sub(seq_of(lane), nb)))
        Wv::or64(&sh.entry_fail, 1ull << lane);
    });
    wv.lanes([&](uint32_t lane) {
      if (lane != 0) return;
      unsigned long long E = sh.entry_mask;
      if (sh.entry_fail) {
        E &= below(low_bit(sh.entry_fail));
        sh.stop = 1;
      }
      if (E) sh.new_base = packet_id_add(seq_of(high_bit(E)), 1);
      sh.entry_mask = sh.entry_fail = 0;
    });
    if (sh.stop) break;  // (read by every lane after the phase: uniform)
  }
  const uint32_t new_base = sh.new_base, delta = packet_id_sub(new_base, base);  // delta <= n <= W: every slot once
  for (uint32_t k0 = 0; k0 < delta; k0 += 64)
    wv.lanes([&](uint32_t lane) {
      if (k0 + lane >= delta) return;
      const uint32_t idx = packet_id_add(base, k0 + lane) & mask;
      ufc_rx_slot& s = slots[idx];
      s.rx_flags &= (uint8_t)~UFC_RX_SLOT_ENTRY;
      uint64_t alloc = 0;
      rx_clear_slot(s, plan[idx], alloc);  // (alloc counts down from zero: what the slot gives back, negated)
      if (alloc) Wv::add64(&sh.alloc_sub, 0 - alloc);
    });
  wv.lanes([&](uint32_t c) {  // try_unset_channel_base_id over (base, new_base]
    const uint32_t cb = sh.chan_base[c];
    if (cb != UFC_NO_PARENT) {
      const uint32_t lead = packet_id_sub(cb, base);
      if (lead >= 1 && lead <= delta) R.channel_base_id[c] = UFC_NO_PARENT;
    }
  });
  wv.lanes([&](uint32_t lane) {
    if (lane != 0) return;
    R.channel_ready_flags = sh.ready_bits;
    R.window_ready = 0;
    if (n < delta) R.end_id = new_base;
    R.alloc -= sh.alloc_sub;
    res.advanced += delta;
    R.base_id = new_base;
  });
}

// The end of the step: the result's delivery fields and the three counts ([0] delivered packets, [1] delivered
// bytes, [2] carry bytes; all zero after BAD_STATE).
inline __host__ __device__ void rx_walk_end(const RxArgs& a, uint64_t r, uint32_t delivered, uint64_t out_bytes,
                                            uint64_t counts[3]) {
  ufc_receiver_result& res = a.results[r];
  counts[0] = counts[1] = counts[2] = 0;
  if (res.stop != UFC_RX_DONE) return;
  const ufc_rx_slot* slots = a.slots + a.slot_first[r];
  uint64_t carry = 0;
  for (uint32_t j = 0; j < a.receivers_out[r].window_size; j++) carry += rx_slot_region(slots[j]);
  res.packet_count = delivered;
  res.bytes_delivered = out_bytes;
  counts[0] = delivered;
  counts[1] = out_bytes;
  counts[2] = carry;
}

// The whole step, serially.  Returns false for BAD_STATE.
inline __host__ __device__ bool rx_walk(const RxArgs& a, uint64_t r, RxPlan* plans, uint8_t* status,
                                        const RxDupSet& dups, uint64_t counts[3]) {
  const bool ok = rx_walk_begin(a, r, plans);
  rx_walk_items(a, r, plans, status, dups, nullptr);
  uint32_t delivered;
  uint64_t out_bytes;
  rx_receive_serial(a, r, plans, delivered, out_bytes);
  rx_walk_end(a, r, delivered, out_bytes, counts);
  return ok;
}

// After the sums: receiver r's records, carry layout, received-bits words and copy segments (zeroed before).
// packet_first[r], out_first and carry_first[r] are its firsts.
inline __host__ __device__ void rx_finish(const RxArgs& a, uint64_t r, RxPlan* plans, const uint8_t* status,
                                          uint64_t out_first, RxSegment* segs, uint32_t* seg_len_out) {
  const uint64_t pf = a.packet_first[r];
  a.results[r].packet_first = (uint32_t)pf;
  if (a.results[r].stop != UFC_RX_DONE) return;
  const ufc_receiver& R = a.receivers_out[r];
  const uint32_t W = R.window_size, mask = W - 1;
  const uint64_t s0 = a.slot_first[r];
  ufc_rx_slot* slots = a.slots + s0;
  RxPlan* plan = plans + s0;
  auto put = [&](uint64_t k, uint64_t src, uint64_t dst, uint32_t len, uint32_t kinds) {
    RxSegment sg;
    sg.src = src;
    sg.dst = dst;
    sg.len = len;
    sg.kinds = kinds;
    segs[k] = sg;
    if (seg_len_out) seg_len_out[k] = len;
  };
  uint64_t cursor = a.carry_first[r];
  for (uint32_t j = 0; j < W; j++) {
    ufc_rx_slot& s = slots[j];
    RxPlan& p = plan[j];
    const uint32_t held = rx_slot_held(s), n = rx_slot_nfrag(s);
    uint32_t pkt_len = 0;
    if (p.deliver_idx != kRxNotDelivered) {
      p.pkt_dst += out_first;
      p.flags |= kRxPktOut;
      pkt_len = p.len;
      if (pf + p.deliver_idx < a.packets_cap) {
        ufc_rx_packet rec{};
        rec.out_offset = p.pkt_dst;
        rec.sequence_id = p.seq;
        rec.len = p.len;
        rec.channel_id = p.channel;
        rec.flags = p.pkt_flags;
        a.packets[pf + p.deliver_idx] = rec;
      }
    } else if (held) {
      p.pkt_dst = cursor;
      p.flags |= kRxPktCarry;
      pkt_len = held;
    }
    const uint32_t dst_kind = (p.flags & kRxPktCarry) ? kRxDstCarry : 0u;
    const uint64_t in_frag = p.in_offset + align8(p.in_held_len);
    if (pkt_len && (p.flags & kRxHeldIn)) {
      put(rx_slot_segment(s0 + j, 0), p.in_offset, p.pkt_dst, pkt_len, kRxSrcCarry | dst_kind);
    } else if (pkt_len && (p.flags & kRxCompletedNow) && (p.flags & kRxAsmCarry)) {
      // the fragments received in earlier steps (what lies in between is overwritten by this step's)
      const uint64_t have = rx_frag_data_bytes(p.in_nfrag);
      put(rx_slot_segment(s0 + j, 1), in_frag, p.pkt_dst, have < pkt_len ? (uint32_t)have : pkt_len,
          kRxSrcCarry | dst_kind);
    }
    if (n) {
      p.frag_dst = cursor + align8(held);
      p.flags |= kRxFrag;
      const uint64_t data = rx_frag_data_bytes(n), words = p.frag_dst + data;
      const bool carried = (p.flags & kRxAsmCarry) != 0;
      if (carried) put(rx_slot_segment(s0 + j, 1), in_frag, p.frag_dst, (uint32_t)data, kRxSrcCarry | kRxDstCarry);
      for (uint32_t w = 0; w < (n + 63) / 64; w++)
        if (words + 8ull * w + 8 <= a.carry_cap)
          *(uint64_t*)(a.carry_out + words + 8ull * w) = carried ? *(const uint64_t*)(a.carry_in + in_frag + data + 8ull * w) : 0ull;
    }
    s.data_offset = cursor;
    cursor += rx_slot_region(s);
  }
  // This step's fragments: into the slot's buffer, or into the packet they completed.
  const uint64_t ff0 = a.frame_first[r], ff1 = a.frame_first[r + 1];
  for (uint64_t i = ff0; i < ff1; i++) {
    if (!rx_frame_counts(a, i)) continue;
    const ufc_frame_info& f = a.infos[i];
    const uint64_t sb = a.src_base ? a.src_base[i] : 0;
    for (uint64_t g = f.item_first, ge = (uint64_t)f.item_first + f.item_count; g < ge; g++) {
      if (status[g] != UFC_RX_STORED && status[g] != UFC_RX_COMPLETED) continue;
      const ufc_item it = a.items[g];
      const RxPlan& p = plan[it.id & mask];
      const uint64_t at = (uint64_t)it.fragment_id * UFC_MAX_FRAGMENT_SIZE;
      if (p.flags & kRxFrag) {
        // (a stored fragment's fragment_id_last is the slot's)
        const uint64_t word = p.frag_dst + rx_frag_data_bytes((uint32_t)it.fragment_id_last + 1) + 8ull * (it.fragment_id >> 6);
        if (word + 8 <= a.carry_cap) *(uint64_t*)(a.carry_out + word) |= 1ull << (it.fragment_id & 63u);
        if (it.data_len) put(rx_item_segment(a.n_slots, g), sb + it.data_offset, p.frag_dst + at, it.data_len, kRxDstCarry);
      } else if ((p.flags & kRxCompletedNow) && (p.flags & (kRxPktOut | kRxPktCarry)) && it.data_len) {
        put(rx_item_segment(a.n_slots, g), sb + it.data_offset, p.pkt_dst + at, it.data_len,
            (p.flags & kRxPktCarry) ? kRxDstCarry : 0u);
      }
    }
  }
}

// ---- the frame window: FrameAckQueue as handle_data_frame and handle_sync_frame drive it ----
// Restates src/half_connection/frame_ack_queue.rs (ReceiveWindow::contains / advance :14-26, mark_seen :58-84) and
// half_connection/mod.rs:132-152, for the batched frame windows (frame_window.hip, ufc_frame_window_host).  A
// connection's step is walked twice with the same code: once for its group count (write = false: nothing is
// stored), and after the exclusive sum of the counts once more with its first group index (write = true).
struct FwArgs {
  const ufc_frame_info* infos;
  uint64_t n_frames;
  const uint64_t* frame_first;
  const ufc_frame_window* windows;
  uint64_t n_windows;
  uint8_t* frame_accept;
  ufc_item* groups;
  uint64_t groups_cap;
  uint64_t* group_first;
  uint64_t* groups_used;
  ufc_frame_window_result* results;
  ufc_frame_window* windows_out;
};
inline bool fw_args_ok(const FwArgs& a) {  // (the n_windows + 1 group counts are scanned with a 32-bit count)
  const bool bad = !a.frame_first || !a.windows || !a.windows_out || !a.frame_accept || !a.group_first ||
                   !a.groups_used || !a.results || (!a.infos && a.n_frames) || (!a.groups && a.groups_cap) ||
                   a.n_frames >= kCountLim || a.n_windows >= kCountLim;
  return !bad;
}

constexpr uint32_t kFwMaxSize = 0x80000000u;
// What a frame is to the window.
constexpr uint32_t kFwData = 1, kFwFrameSync = 2, kFwSync = 4, kFwPacketSync = 8, kFwNonce = 16;

// The class of a frame and its target: the base it leaves behind when it passes (id + 1, or next_frame_id).
UFC_HD uint32_t fw_classify(const ufc_frame_info& f, uint32_t& target) {
  target = 0;
  if (!f.ok) return 0;
  if (f.kind == UFC_FRAME_DATA) {
    target = f.f[0] + 1;
    return kFwData | ((f.aux & 1u) ? kFwNonce : 0u);
  }
  if (f.kind == UFC_FRAME_SYNC) {
    target = f.f[0];
    return kFwSync | ((f.aux & 1u) ? kFwFrameSync : 0u) | ((f.aux & 2u) ? kFwPacketSync : 0u);
  }
  return 0;
}
// A candidate (a data frame, or a sync frame with a frame id) against base b: contains(id), or advance's
// 0 < delta <= size.
UFC_HD bool fw_passes(uint32_t cls, uint32_t target, uint32_t b, uint32_t size) {
  if (cls & kFwData) return (uint32_t)(target - 1 - b) < size;
  const uint32_t d = target - b;
  return d > 0 && d <= size;
}

// A connection's running state: the base, the open group (the deque's last entry) and the result's counts.
struct FwRun {
  uint32_t base, ge, gb, gn;
  bool has;
  uint32_t groups;  // groups closed so far (the open one comes after them)
  uint32_t accepted, refused, syncs, psyncs, first_psync, reply;
};
UFC_HD FwRun fw_run_begin(const ufc_frame_window& W) {
  FwRun s{};
  s.base = W.base_id;
  s.ge = W.tail_base_id;
  s.gb = W.tail_bitfield;
  s.gn = W.tail_nonce & 1u;
  s.has = W.has_tail != 0;
  s.first_psync = UFC_NO_PARENT;
  return s;
}
UFC_HD bool fw_range_ok(const FwArgs& a, uint64_t ff0, uint64_t ff1) { return ff0 <= ff1 && ff1 <= a.n_frames; }
UFC_HD void fw_put_group(const FwArgs& a, uint64_t at, uint32_t e, uint32_t b, uint32_t n) {
  if (at >= a.groups_cap) return;
  ufc_item g{};
  g.id = e;
  g.channel_id = (uint8_t)n;
  g.form = 3;
  g.data_offset = b;
  a.groups[at] = g;
}
// mark_seen's second half for an accepted frame.
UFC_HD void fw_mark(const FwArgs& a, FwRun& s, bool write, uint64_t gfirst, uint32_t id, uint32_t nonce) {
  const uint32_t off = id - s.ge;
  if (s.has && off < 32) {
    if (!(s.gb & (1u << off))) {
      s.gb |= 1u << off;
      s.gn ^= nonce;
    }
    return;
  }
  if (s.has) {
    if (write) fw_put_group(a, gfirst + s.groups, s.ge, s.gb, s.gn);
    s.groups++;
  }
  s.ge = id;
  s.gb = 1;
  s.gn = nonce;
  s.has = true;
}
// BAD_STATE: the state copied through, an empty result.
UFC_HD void fw_bad(const FwArgs& a, uint64_t r, const ufc_frame_window& W, uint64_t gfirst) {
  ufc_frame_window_result res{};
  res.group_first = (uint32_t)gfirst;
  res.first_packet_sync = UFC_NO_PARENT;
  res.stop = UFC_FW_BAD_STATE;
  a.results[r] = res;
  a.windows_out[r] = W;
}
// The end of a step: the open group as the connection's last, the result, the state.  Returns the group count.
UFC_HD uint64_t fw_end(const FwArgs& a, uint64_t r, const ufc_frame_window& W, const FwRun& s, bool write, uint64_t gfirst) {
  const uint32_t count = s.groups + (s.has ? 1u : 0u);
  if (!write) return count;
  if (s.has) fw_put_group(a, gfirst + s.groups, s.ge, s.gb, s.gn);
  ufc_frame_window_result res{};
  res.group_first = (uint32_t)gfirst;
  res.group_count = count;
  res.accepted = s.accepted;
  res.refused = s.refused;
  res.syncs = s.syncs;
  res.packet_syncs = s.psyncs;
  res.first_packet_sync = s.first_psync;
  res.advanced = s.base - W.base_id;  // (the wrapping sum of the moves)
  res.stop = UFC_FW_DONE;
  a.results[r] = res;
  ufc_frame_window O = W;
  O.base_id = s.base;
  if (s.has) {
    O.tail_base_id = s.ge;
    O.tail_bitfield = s.gb;
    O.tail_nonce = (uint8_t)s.gn;
  }
  O.has_tail = s.has ? 1 : 0;
  O.sync_reply = (uint8_t)(W.sync_reply | s.reply);
  a.windows_out[r] = O;
  return count;
}

// The step frame by frame, as the reference runs it.
inline __host__ __device__ uint64_t fw_walk_serial(const FwArgs& a, uint64_t r, bool write, uint64_t gfirst) {
  const ufc_frame_window W = a.windows[r];
  const uint64_t ff0 = a.frame_first[r], ff1 = a.frame_first[r + 1];
  const bool usable = fw_range_ok(a, ff0, ff1);
  if (!usable || W.size > kFwMaxSize) {
    if (write) {
      if (usable)
        for (uint64_t i = ff0; i < ff1; i++) a.frame_accept[i] = 0;
      fw_bad(a, r, W, gfirst);
    }
    return 0;
  }
  FwRun s = fw_run_begin(W);
  for (uint64_t i = ff0; i < ff1; i++) {
    uint32_t target;
    const uint32_t cls = fw_classify(a.infos[i], target);
    bool accepted = false;
    if (cls & kFwData) {
      accepted = fw_passes(cls, target, s.base, W.size);
      if (accepted) {
        s.base = target;
        s.accepted++;
        fw_mark(a, s, write, gfirst, target - 1, (cls & kFwNonce) ? 1u : 0u);
      } else {
        s.refused++;
      }
    } else if (cls & kFwSync) {
      if ((cls & kFwFrameSync) && fw_passes(cls, target, s.base, W.size)) s.base = target;
      if (cls & kFwPacketSync) {
        if (!s.psyncs) s.first_psync = (uint32_t)i;
        s.psyncs++;
      }
      s.syncs++;
      s.reply = 1;
    }
    if (write) a.frame_accept[i] = accepted ? 1 : 0;
  }
  return fw_end(a, r, W, s, write, gfirst);
}

// The same step in tiles of 64 consecutive frames, one lane per frame: the form the device runs, one wave per
// connection (frame_window.hip), written against a wave policy as rx_receive_tiles is, so that the same text runs
// as host code (tests/c/window_host_check.hip, against fw_walk_serial):
//   Wv::lanes(f)   f(lane) for the 64 lanes; what the lanes wrote to `sh` before is visible to all after
//   Wv::one(f)     f() once
//   Wv::or64       atomic on the device (vector atomics on LDS), plain on the host
// What is written outside a phase is the same for every lane (the running state, the masks read back from `sh`).
// The window: a candidate lane (a data frame, or a sync frame with a frame id) tests itself against the target of
// the candidate lane before it, the tile's base for the first.  If no lane fails, every verdict is final.
// Otherwise the first failing lane does fail (all before it passed, so its base was the true one): it drops out
// as a candidate, and the lanes after it test again.  Rounds per tile = 1 + the refused candidates.
// The groups, over the accepted lanes in order: the lanes whose id lies within 32 of the open group's base fold into
// it (an OR of their bits; the parity of the nonces of those whose bit was clear) up to the first lane that does
// not, which closes the group and opens the next.  A fold also stops in front of a lane whose bit is not above
// the bit of the lane before it (after a sync frame the ids may come back): that lane folds in the next round,
// against the bits as they are then, so the bits of one fold are distinct and "only if the bit was clear" stays
// literal.  A word of `sh` per round, zeroed once per tile: at most 65 window rounds and 64 group rounds.
struct FwWaveShared {
  unsigned long long fail[65], stop[65], bits[65], par[65];
  unsigned long long data_mask, cand_mask, sync_mask, psync_mask;
  uint32_t target[64];
  uint8_t cls[64];
};

template <class Wv>
inline __host__ __device__ uint64_t fw_walk_tiles(const Wv& wv, FwWaveShared& sh, const FwArgs& a, uint64_t r, bool write,
                                                  uint64_t gfirst) {
  const ufc_frame_window W = a.windows[r];
  const uint64_t ff0 = a.frame_first[r], ff1 = a.frame_first[r + 1];
  const bool usable = fw_range_ok(a, ff0, ff1);
  if (!usable || W.size > kFwMaxSize) {  // (every lane takes this branch or none)
    if (write) {
      if (usable)
        for (uint64_t t0 = ff0; t0 < ff1; t0 += 64)
          wv.lanes([&](uint32_t lane) {
            if (t0 + lane < ff1) a.frame_accept[t0 + lane] = 0;
          });
      wv.one([&]() { fw_bad(a, r, W, gfirst); });
    }
    return 0;
  }
  FwRun s = fw_run_begin(W);
  const uint32_t size = W.size;
  auto below = [](uint32_t lane) { return (1ull << lane) - 1; };
  for (uint64_t t0 = ff0; t0 < ff1; t0 += 64) {
    const uint32_t nv = ff1 - t0 < 64 ? (uint32_t)(ff1 - t0) : 64u;
    wv.lanes([&](uint32_t lane) {
      sh.fail[lane] = sh.stop[lane] = sh.bits[lane] = sh.par[lane] = 0;
      if (lane == 0) {
        sh.fail[64] = sh.stop[64] = sh.bits[64] = sh.par[64] = 0;
        sh.data_mask = sh.cand_mask = sh.sync_mask = sh.psync_mask = 0;
      }
    });
    wv.lanes([&](uint32_t lane) {
      uint32_t target = 0, cls = 0;
      if (lane < nv) cls = fw_classify(a.infos[t0 + lane], target);
      sh.target[lane] = target;
      sh.cls[lane] = (uint8_t)cls;
      const unsigned long long bit = 1ull << lane;
      if (cls & kFwData) Wv::or64(&sh.data_mask, bit);
      if (cls & (kFwData | kFwFrameSync)) Wv::or64(&sh.cand_mask, bit);
      if (cls & kFwSync) Wv::or64(&sh.sync_mask, bit);
      if (cls & kFwPacketSync) Wv::or64(&sh.psync_mask, bit);
    });
    const unsigned long long cand = sh.cand_mask, data = sh.data_mask, syncs = sh.sync_mask, psyncs = sh.psync_mask;
    // the window
    unsigned long long failed = 0;
    uint32_t from = 0;  // the lanes below are final
    for (uint32_t k = 0;; k++) {
      const unsigned long long live = cand & ~failed;
      wv.lanes([&](uint32_t lane) {
        if (lane < from || !((live >> lane) & 1u)) return;
        const unsigned long long m = live & below(lane);
        const uint32_t b = m ? sh.target[high_bit(m)] : s.base;
        if (!fw_passes(sh.cls[lane], sh.target[lane], b, size)) Wv::or64(&sh.fail[k], 1ull << lane);
      });
      const unsigned long long F = sh.fail[k];
      if (!F) break;
      const uint32_t f = low_bit(F);
      failed |= 1ull << f;
      from = f + 1;
    }
    const unsigned long long passing = cand & ~failed, acc = data & passing;
    if (passing) s.base = sh.target[high_bit(passing)];
    s.accepted += popc(acc);
    s.refused += popc(data & ~acc);
    s.syncs += popc(syncs);
    if (psyncs && !s.psyncs) s.first_psync = (uint32_t)(t0 + low_bit(psyncs));
    s.psyncs += popc(psyncs);
    if (syncs) s.reply = 1;
    if (write)
      wv.lanes([&](uint32_t lane) {
        if (lane < nv) a.frame_accept[t0 + lane] = (uint8_t)((acc >> lane) & 1u);
      });
    // the groups
    unsigned long long rem = acc;
    for (uint32_t k = 0; rem; k++) {
      if (!s.has) {  // the first lane left opens a group
        const uint32_t o = low_bit(rem);
        s.ge = sh.target[o] - 1;
        s.gb = 1;
        s.gn = (sh.cls[o] & kFwNonce) ? 1u : 0u;
        s.has = true;
        rem &= rem - 1;
        if (!rem) break;
      }
      wv.lanes([&](uint32_t lane) {
        if (!((rem >> lane) & 1u)) return;
        const uint32_t off = sh.target[lane] - 1 - s.ge;
        const unsigned long long m = rem & below(lane);
        if (off >= 32 || (m && sh.target[high_bit(m)] - 1 - s.ge >= off)) Wv::or64(&sh.stop[k], 1ull << lane);
      });
      const unsigned long long S = sh.stop[k];
      const unsigned long long fold = S ? rem & below(low_bit(S)) : rem;
      if (fold) {
        wv.lanes([&](uint32_t lane) {
          if (!((fold >> lane) & 1u)) return;
          const uint32_t bit = 1u << (sh.target[lane] - 1 - s.ge);
          Wv::or64(&sh.bits[k], bit);
          if (!(s.gb & bit) && (sh.cls[lane] & kFwNonce)) Wv::or64(&sh.par[k], 1ull << lane);
        });
        s.gb |= (uint32_t)sh.bits[k];
        s.gn ^= popc(sh.par[k]) & 1u;
        rem &= ~fold;
      }
      if (rem && sh.target[low_bit(rem)] - 1 - s.ge >= 32) {  // the next lane closes the group
        const uint64_t at = gfirst + s.groups;
        if (write) wv.one([&]() { fw_put_group(a, at, s.ge, s.gb, s.gn); });
        s.groups++;
        s.has = false;
      }
    }
  }
  if (write) wv.one([&]() { fw_end(a, r, W, s, true, gfirst); });
  return s.groups + (s.has ? 1u : 0u);
}

// ---- the sender's frame queue: FrameQueue as handle_ack_frame, step and the emitters drive it ----
// Restates src/half_connection/frame_queue.rs (FrameLog :24-84, FeedbackGen :96-195, FrameQueue :209-388),
// reorder_buffer.rs:2-179 and loss_rate.rs:19-110 for the batched frame queues (frame_queue.hip,
// ufc_frame_queue_host; the rules are in include/uflow_frame_codec.h).  Written once, against the wave policy of
// fw_walk_tiles with one addition:
//   Wv::ballot(f)  the 64-bit mask of the lanes for which f(lane) is true; what f wrote to `sh` is visible to all
//                  after (the device's wave ballot; a loop on the host)
// One wave runs a connection's step.  What is written outside a phase is the same for every lane: the running
// state FqRun (the log's and the window's ids, the reorder buffer, the pending AckData, the front interval's end
// time and the interval count).  The loss intervals themselves live in `sh` and are touched by Wv::one alone (lane 0
// on the device, in its program order).  Everything that touches a run of log entries takes a lane per entry:
//   group span     the <= 32 entries of a group: outside-the-log test, nonce parity, rate_limited OR and the newly
//                  acked lanes are ballots; ACKED and ref_acked are stored by the entries' lanes; the send times
//                  and sizes of the newly acked go through `sh` into the serial put()s;
//   nack runs      put's and advance's `while base_id != ...` loops, in tiles of 64 ids.  A ballot finds the first
//                  entry at or after the front interval's end; the lanes in front of it add to the front's length
//                  in one step, that entry opens the next interval, and the lanes behind it vote again against the
//                  new end.  That is push_nack entry by entry for any log, monotone or not; a monotone log with a
//                  positive rtt opens few intervals, so a tile takes one or two votes;
//   expiry cutoff  a ballot per tile of 64 entries for the first one at or after the threshold;
//   pushes         a copy of 64 records per phase;
//   frames         a ballot per tile of 64 frames finds the ok ack frames; only they are visited.
struct FqArgs {
  const ufc_frame_info* infos;
  uint64_t n_frames;
  const ufc_item* items;
  uint64_t n_items;
  const uint64_t* frame_first;
  const ufc_sent_frame* sent;
  uint64_t n_sent;
  const uint64_t* sent_first;
  const ufc_frame_queue* queues;
  const ufc_frame_queue_step* steps;
  uint64_t n_queues;
  ufc_sent_frame* log;
  uint64_t n_log;
  uint8_t* ref_acked;
  uint64_t refs_cap;
  ufc_frame_queue_result* results;
  ufc_frame_queue* queues_out;
};
inline bool fq_args_ok(const FqArgs& a) {
  const bool bad = !a.frame_first || !a.sent_first || !a.queues || !a.steps || !a.results || !a.queues_out ||
                   (!a.infos && a.n_frames) || (!a.items && a.n_items) || (!a.sent && a.n_sent) ||
                   (!a.log && a.n_log) || a.n_frames >= kCountLim || a.n_items >= kCountLim || a.n_sent >= kCountLim ||
                   a.n_queues >= kCountLim;
  return !bad;
}

constexpr uint64_t kFqInitialRttMs = 100;         // FeedbackGen::INITIAL_RTT_MS, frame_queue.rs:111
constexpr uint32_t kFqMaxIntervals = 9;           // loss_rate.rs:72
constexpr uint32_t kFqMaxSpan = 0x80000000u;
constexpr uint32_t kFqOwnRefs = 16;               // a lane marks up to this many fragments itself

struct FqWaveShared {
  uint64_t tile_time[64];                          // a nack or expiry tile's send times
  uint64_t group_time[32];                         // a group's entries
  uint32_t group_size[32], group_ref_first[32], group_ref_count[32];
  uint8_t group_flags[32];
  // Wv::one only from here on: the loss intervals, the pending AckData, the result's counters
  uint64_t li_end[kFqMaxIntervals];
  uint32_t li_len[kFqMaxIntervals];
  uint32_t has_ack, ack_rl;
  uint64_t ack_last, ack_total;
  ufc_frame_queue_result res;
};

struct FqRun {
  uint32_t log_base, log_next, window_base, rb_base, rb_f0, rb_f1, rb_count;
  uint32_t rb_max_span, window_size, tail_size, mask;
  uint64_t ring, rtt;
  bool pending;
  uint32_t li_count;
  uint64_t li_end;                                 // the front interval's end time, if li_count
};

UFC_HD uint32_t fq_sat_add(uint32_t v, uint32_t k) {  // k saturating_add(1)s
  const uint64_t s = (uint64_t)v + k;
  return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
}
// (1.0 / p).clamp(0.0, u32::MAX as f64).round() as u32, loss_rate.rs:53.
UFC_HD uint32_t fq_reset_length(double p) {
#pragma clang fp contract(off)
  double v = 1.0 / p;
  if (v != v) return 0;  // (clamp keeps a NaN, `as u32` makes it 0)
  if (v < 0.0) v = 0.0;
  if (v > 4294967295.0) v = 4294967295.0;
  uint64_t t = (uint64_t)v;
  if (v - (double)t >= 0.5) t++;  // round(): half away from zero; v - t is exact
  return (uint32_t)t;
}
// (total as f64 / ms_to_s(delta)).clamp(0.0, u32::MAX as f64) as u32, frame_queue.rs:131-132.
UFC_HD uint32_t fq_receive_rate(uint64_t total, uint64_t delta_ms) {
#pragma clang fp contract(off)
  const double s = (double)delta_ms / 1000.0;
  const double v = (double)total / s;
  if (v != v) return 0;
  if (v < 0.0) return 0;
  if (v > 4294967295.0) return 0xFFFFFFFFu;
  return (uint32_t)v;
}
// compute_loss_rate, loss_rate.rs:86-109, sum by sum.
UFC_HD double fq_loss_rate(const uint32_t* len, uint32_t n) {
#pragma clang fp contract(off)
  const double W[8] = {1.0, 1.0, 1.0, 1.0, 0.8, 0.6, 0.4, 0.2};
  if (n == 0) return 0.0;
  if (n == 1) return W[0] / ((double)len[0] * W[0]);
  double i0 = 0.0, i1 = 0.0, w = 0.0;
  for (uint32_t i = 0; i + 1 < n; i++) {
    const double term = (double)len[i] * W[i];
    i0 = i0 + term;
    w = w + W[i];
  }
  for (uint32_t i = 1; i < n; i++) {
    const double term = (double)len[i] * W[i - 1];
    i1 = i1 + term;
  }
  return w / (i0 > i1 ? i0 : i1);
}

// The checks of the header comment, in its order; the frames' item ranges are checked by the caller's tiles.
UFC_HD bool fq_state_ok(const FqArgs& a, const ufc_frame_queue& Q, const ufc_frame_queue_step& S, uint64_t ff0, uint64_t ff1,
                        uint64_t sf0, uint64_t sf1) {
  const uint64_t span = (uint64_t)Q.window_size + Q.tail_size;
  if (Q.log_cap == 0 || (Q.log_cap & (Q.log_cap - 1)) || Q.log_cap < span) return false;
  if (Q.log_first > a.n_log || a.n_log - Q.log_first < Q.log_cap) return false;
  const uint32_t len = Q.log_next_id - Q.log_base_id, ahead = Q.log_next_id - Q.window_base_id;
  if (len > Q.log_cap || ahead > Q.window_size || (uint64_t)len > (uint64_t)ahead + Q.tail_size) return false;
  if (Q.rb_max_span < span || Q.rb_max_span > kFqMaxSpan) return false;
  const uint32_t rb = Q.rb_base_id - Q.log_base_id;
  if (rb > len || Q.rb_count > 2) return false;
  const uint32_t d0 = Q.rb_frames[0] - Q.rb_base_id, d1 = Q.rb_frames[1] - Q.rb_base_id;
  if (Q.rb_count >= 1 && (d0 == 0 || (uint64_t)rb + d0 >= len)) return false;
  if (Q.rb_count == 2 && (d1 == 0 || (uint64_t)rb + d1 >= len || d0 >= d1)) return false;
  if (Q.li_count > kFqMaxIntervals || ((S.flags & UFC_FQ_RESET_LOSS) && Q.li_count == 0)) return false;
  return ff0 <= ff1 && ff1 <= a.n_frames && sf0 <= sf1 && sf1 <= a.n_sent;
}
UFC_HD bool fq_is_ack(const ufc_frame_info& f) { return f.ok && f.kind == UFC_FRAME_ACK; }
UFC_HD uint64_t fq_slot(const FqRun& s, uint32_t id) { return s.ring + (id & s.mask); }

// push_ack k times (loss_rate.rs:56-61).
template <class Wv>
UFC_HD void fq_acks(const Wv& wv, FqWaveShared& sh, FqRun& s, uint32_t k) {
  wv.one([&]() { sh.res.li_acks += k; });
  if (s.li_count) wv.one([&]() { sh.li_len[0] = fq_sat_add(sh.li_len[0], k); });
}
// push_nack (loss_rate.rs:63-84) for the ids from, from + 1, ... (count of them), with their send times.
template <class Wv>
inline __host__ __device__ void fq_nacks(const Wv& wv, FqWaveShared& sh, const FqArgs& a, FqRun& s, uint32_t from,
                                         uint32_t count) {
  wv.one([&]() { sh.res.li_nacks += count; });
  for (uint32_t t = 0; t < count; t += 64) {
    const uint32_t nv = count - t < 64 ? count - t : 64u;
    wv.lanes([&](uint32_t lane) {
      if (lane < nv) sh.tile_time[lane] = a.log[fq_slot(s, from + t + lane)].send_time_ms;
    });
    uint32_t pos = 0;
    while (pos < nv) {
      uint32_t f = pos;  // with no interval the entry opens one whatever its time (:77-83)
      if (s.li_count) {
        const uint64_t end = s.li_end;
        const unsigned long long M =
            wv.ballot([&](uint32_t lane) { return lane >= pos && lane < nv && sh.tile_time[lane] >= end; });
        f = M ? low_bit(M) : nv;
        const uint32_t adds = f - pos;  // they fall under the front interval (:75)
        if (adds) wv.one([&]() { sh.li_len[0] = fq_sat_add(sh.li_len[0], adds); });
        if (f >= nv) break;
      }
      const uint64_t end = sh.tile_time[f] + s.rtt;
      const uint32_t held = s.li_count < kFqMaxIntervals ? s.li_count : kFqMaxIntervals - 1;
      wv.one([&]() {  // push_front, truncate(9)
        for (uint32_t k = held; k > 0; k--) {
          sh.li_end[k] = sh.li_end[k - 1];
          sh.li_len[k] = sh.li_len[k - 1];
        }
        sh.li_end[0] = end;
        sh.li_len[0] = 1;
      });
      s.li_count = held + 1;
      s.li_end = end;
      pos = f + 1;
    }
  }
}

// ReorderBuffer::put (reorder_buffer.rs:28-115) with FeedbackGen's callback (frame_queue.rs:164-172).
template <class Wv>
inline __host__ __device__ void fq_rb_put(const Wv& wv, FqWaveShared& sh, const FqArgs& a, FqRun& s, uint32_t id) {
  if (s.rb_count == 0) {
    if (id == s.rb_base) {
      fq_acks(wv, sh, s, 1);
      s.rb_base++;
    } else {
      s.rb_f0 = id;
      s.rb_count = 1;
    }
  } else if (s.rb_count == 1) {
    if (id == s.rb_base) {
      fq_acks(wv, sh, s, 1);
      s.rb_base++;
      if (s.rb_f0 == s.rb_base) {
        fq_acks(wv, sh, s, 1);
        s.rb_base++;
        s.rb_count = 0;
      }
    } else {
      if (id - s.rb_base < s.rb_f0 - s.rb_base) {
        s.rb_f1 = s.rb_f0;
        s.rb_f0 = id;
      } else {
        s.rb_f1 = id;
      }
      s.rb_count = 2;
    }
  } else if (s.rb_count == 2) {
    uint32_t min_id = id, delta_min = id - s.rb_base;
    const uint32_t delta_1 = s.rb_f1 - s.rb_base;
    if (delta_1 < delta_min) {
      const uint32_t t = s.rb_f1;
      s.rb_f1 = min_id;
      min_id = t;
      delta_min = delta_1;
    }
    if (s.rb_f0 - s.rb_base < delta_min) {
      const uint32_t t = s.rb_f0;
      s.rb_f0 = min_id;
      min_id = t;
    }
    fq_nacks(wv, sh, a, s, s.rb_base, min_id - s.rb_base);
    fq_acks(wv, sh, s, 1);
    s.rb_base = min_id + 1;
    if (s.rb_f0 == s.rb_base) {
      fq_acks(wv, sh, s, 1);
      s.rb_base++;
      s.rb_count--;
      if (s.rb_f1 == s.rb_base) {
        fq_acks(wv, sh, s, 1);
        s.rb_base++;
        s.rb_count--;
      } else {
        s.rb_f0 = s.rb_f1;
      }
    }
  }
}
// ReorderBuffer::advance (:122-178) with the same callback (frame_queue.rs:184-192).
template <class Wv>
inline __host__ __device__ void fq_rb_advance(const Wv& wv, FqWaveShared& sh, const FqArgs& a, FqRun& s, uint32_t new_base) {
  while (s.rb_count > 0 && s.rb_f0 - s.rb_base < new_base - s.rb_base) {
    fq_nacks(wv, sh, a, s, s.rb_base, s.rb_f0 - s.rb_base);
    fq_acks(wv, sh, s, 1);
    s.rb_base = s.rb_f0 + 1;
    if (s.rb_count == 2) s.rb_f0 = s.rb_f1;
    s.rb_count--;
  }
  fq_nacks(wv, sh, a, s, s.rb_base, new_base - s.rb_base);
  s.rb_base = new_base;
  if (s.rb_count == 1) {
    if (s.rb_f0 == s.rb_base) {
      fq_acks(wv, sh, s, 1);
      s.rb_base++;
      s.rb_count = 0;
    }
  } else if (s.rb_count == 2) {
    if (s.rb_f0 == s.rb_base) {
      fq_acks(wv, sh, s, 1);
      s.rb_base++;
      s.rb_count--;
      if (s.rb_f1 == s.rb_base) {
        fq_acks(wv, sh, s, 1);
        s.rb_base++;
        s.rb_count--;
      } else {
        s.rb_f0 = s.rb_f1;
      }
    }
  }
}
// cull_log_entries (frame_queue.rs:382-387): notify_advancement (:179-194), then FrameLog::drain (:79-83).
template <class Wv>
inline __host__ __device__ void fq_cull(const Wv& wv, FqWaveShared& sh, const FqArgs& a, FqRun& s, uint32_t new_base) {
  const uint32_t delta = new_base - s.rb_base;
  if (delta >= 1 && delta <= s.rb_max_span) fq_rb_advance(wv, sh, a, s, new_base);
  wv.one([&]() { sh.res.log_culled += new_base - s.log_base; });
  s.log_base = new_base;
}

// acknowledge_group (frame_queue.rs:279-355).
template <class Wv>
inline __host__ __device__ void fq_group(const Wv& wv, FqWaveShared& sh, const FqArgs& a, FqRun& s, const ufc_item& g) {
  const uint32_t base = g.id, bits = g.data_offset, nonce = g.channel_id & 1u;
  wv.one([&]() { sh.res.groups++; });
  if (bits == 0) {  // a dud (:294)
    wv.one([&]() { sh.res.groups_dud++; });
    return;
  }
  const uint32_t n = 32u - (uint32_t)__builtin_clz(bits), len = s.log_next - s.log_base;
  const unsigned long long outside = wv.ballot([&](uint32_t lane) {
    if (lane >= n) return false;
    const uint32_t id = base + lane;
    if (id - s.log_base >= len) return true;
    const ufc_sent_frame e = a.log[fq_slot(s, id)];
    sh.group_time[lane] = e.send_time_ms;
    sh.group_size[lane] = e.size;
    sh.group_ref_first[lane] = e.ref_first;
    sh.group_ref_count[lane] = e.ref_count;
    sh.group_flags[lane] = e.flags;
    return false;
  });
  if (outside) {  // forgotten, or beyond the log (:307)
    wv.one([&]() { sh.res.groups_unknown++; });
    return;
  }
  const unsigned long long claimed = bits;
  const unsigned long long odd =
      wv.ballot([&](uint32_t lane) { return lane < n && ((claimed >> lane) & 1u) && (sh.group_flags[lane] & UFC_SENT_NONCE); });
  if ((popc(odd) & 1u) != nonce) {  // (:313)
    wv.one([&]() { sh.res.groups_bad_nonce++; });
    return;
  }
  const unsigned long long limited = wv.ballot([&](uint32_t lane) { return lane < n && (sh.group_flags[lane] & UFC_SENT_RATE_LIMITED); });
  const unsigned long long fresh =
      wv.ballot([&](uint32_t lane) { return lane < n && ((claimed >> lane) & 1u) && !(sh.group_flags[lane] & UFC_SENT_ACKED); });
  // acked = true, and the fragments of the frame (:328-339)
  auto ref_end = [&](uint32_t lane) {
    const uint64_t e = (uint64_t)sh.group_ref_first[lane] + sh.group_ref_count[lane];
    return a.ref_acked ? (e < a.refs_cap ? e : a.refs_cap) : 0;
  };
  const unsigned long long wide = wv.ballot([&](uint32_t lane) {
    if (lane >= n || !((fresh >> lane) & 1u)) return false;
    a.log[fq_slot(s, base + lane)].flags = (uint8_t)(sh.group_flags[lane] | UFC_SENT_ACKED);
    const uint64_t first = sh.group_ref_first[lane], end = ref_end(lane);
    if (end > first && end - first > kFqOwnRefs) return true;
    for (uint64_t j = first; j < end; j++) a.ref_acked[j] = 1;
    return false;
  });
  for (unsigned long long w = wide; w; w &= w - 1) {  // a frame with many fragments: all lanes mark them
    const uint32_t o = low_bit(w);
    const uint64_t first = sh.group_ref_first[o], end = ref_end(o);
    wv.lanes([&](uint32_t lane) {
      for (uint64_t j = first + lane; j < end; j += 64) a.ref_acked[j] = 1;
    });
  }
  uint64_t last = 0, total = 0;
  for (unsigned long long w = fresh; w; w &= w - 1) {
    const uint32_t o = low_bit(w), id = base + o;
    const uint64_t t = sh.group_time[o];
    last = last > t ? last : t;
    total += sh.group_size[o];
    wv.one([&]() { sh.res.frames_acked++; });
    if (id - s.rb_base < s.rb_max_span) fq_rb_put(wv, sh, a, s, id);  // notify_ack (:159-177)
  }
  // put_ack_data (:149-157)
  wv.one([&]() {
    if (sh.has_ack) {
      sh.ack_last = sh.ack_last > last ? sh.ack_last : last;
      sh.ack_total += total;
      sh.ack_rl |= limited != 0;
    } else {
      sh.has_ack = 1;
      sh.ack_last = last;
      sh.ack_total = total;
      sh.ack_rl = limited != 0;
    }
  });
}

// One connection's step.
template <class Wv>
inline __host__ __device__ void fq_step(const Wv& wv, FqWaveShared& sh, const FqArgs& a, uint64_t c) {
  // (read in place: queues_out[c], which may be queues[c], is written last, behind every read)
  const ufc_frame_queue& Q = a.queues[c];
  const ufc_frame_queue_step& S = a.steps[c];
  const uint64_t ff0 = a.frame_first[c], ff1 = a.frame_first[c + 1], sf0 = a.sent_first[c], sf1 = a.sent_first[c + 1];
  bool ok = fq_state_ok(a, Q, S, ff0, ff1, sf0, sf1);
  for (uint64_t t0 = ff0; ok && t0 < ff1; t0 += 64) {  // the ack frames' item ranges
    const uint32_t nv = ff1 - t0 < 64 ? (uint32_t)(ff1 - t0) : 64u;
    const unsigned long long bad = wv.ballot([&](uint32_t lane) {
      if (lane >= nv) return false;
      const ufc_frame_info f = a.infos[t0 + lane];
      return fq_is_ack(f) && (uint64_t)f.item_first + f.item_count > a.n_items;
    });
    if (bad) ok = false;
  }
  if (!ok) {  // (every lane takes this branch or none)
    wv.one([&]() {
      ufc_frame_queue_result res{};
      res.stop = UFC_FQ_BAD_STATE;
      a.results[c] = res;
      const ufc_frame_queue O = Q;
      a.queues_out[c] = O;
    });
    return;
  }
  FqRun s{};
  s.log_base = Q.log_base_id;
  s.log_next = Q.log_next_id;
  s.window_base = Q.window_base_id;
  s.window_size = Q.window_size;
  s.tail_size = Q.tail_size;
  s.rb_base = Q.rb_base_id;
  s.rb_max_span = Q.rb_max_span;
  s.rb_f0 = Q.rb_frames[0];
  s.rb_f1 = Q.rb_frames[1];
  s.rb_count = Q.rb_count;
  s.mask = Q.log_cap - 1;
  s.ring = Q.log_first;
  s.rtt = (S.flags & UFC_FQ_HAS_RTT) ? S.rtt_ms : kFqInitialRttMs;
  s.pending = Q.rate_limited != 0;
  s.li_count = Q.li_count;
  s.li_end = Q.li_end_time_ms[0];
  wv.one([&]() {
    for (uint32_t k = 0; k < kFqMaxIntervals; k++) {
      sh.li_end[k] = Q.li_end_time_ms[k];
      sh.li_len[k] = Q.li_length[k];
    }
    sh.has_ack = Q.has_ack_data != 0;
    sh.ack_rl = Q.ack_rate_limited != 0;
    sh.ack_last = Q.ack_last_send_time_ms;
    sh.ack_total = Q.ack_total_size;
    sh.res = ufc_frame_queue_result{};
  });
  // 1. reset_loss_rate
  if (S.flags & UFC_FQ_RESET_LOSS) {
    s.li_count = 1;
    wv.one([&]() { sh.li_len[0] = fq_reset_length(S.reset_loss_rate); });
  }
  // 2. push
  {
    const uint32_t ahead = s.log_next - s.window_base, count = (uint32_t)(sf1 - sf0);
    const uint32_t room = s.window_size - ahead, taken = count < room ? count : room;
    const uint32_t first_id = s.log_next;
    const bool pending = s.pending;
    for (uint32_t t = 0; t < taken; t += 64)
      wv.lanes([&](uint32_t lane) {
        const uint32_t j = t + lane;
        if (j >= taken) return;
        const ufc_sent_frame in = a.sent[sf0 + j];
        ufc_sent_frame e{};
        e.send_time_ms = in.send_time_ms;
        e.size = in.size;
        e.ref_first = in.ref_first;
        e.ref_count = in.ref_count;
        e.flags = (uint8_t)((in.flags & UFC_SENT_NONCE) |
                            (((in.flags & UFC_SENT_MARK) || (j == 0 && pending)) ? UFC_SENT_RATE_LIMITED : 0));
        a.log[fq_slot(s, first_id + j)] = e;
      });
    if (taken) s.pending = false;
    s.log_next += taken;
    wv.one([&]() {
      sh.res.pushes_taken = taken;
      sh.res.pushes_refused = count - taken;
    });
    if (S.flags & UFC_FQ_MARK_RATE_LIMITED) s.pending = true;
  }
  // 3. the ack frames
  for (uint64_t t0 = ff0; t0 < ff1; t0 += 64) {
    const uint32_t nv = ff1 - t0 < 64 ? (uint32_t)(ff1 - t0) : 64u;
    unsigned long long acks = wv.ballot([&](uint32_t lane) { return lane < nv && fq_is_ack(a.infos[t0 + lane]); });
    for (; acks; acks &= acks - 1) {
      const ufc_frame_info f = a.infos[t0 + low_bit(acks)];
      wv.one([&]() { sh.res.ack_frames++; });
      for (uint64_t g = f.item_first, ge = (uint64_t)f.item_first + f.item_count; g < ge; g++) fq_group(wv, sh, a, s, a.items[g]);
      // advance_transfer_window (:357-380)
      const uint32_t delta = f.f[0] - s.window_base;
      if (delta != 0 && delta <= s.log_next - s.window_base) {
        s.window_base = f.f[0];
        wv.one([&]() { sh.res.window_advanced += delta; });
        const uint32_t max_base = s.window_base - s.tail_size, cut = max_base - s.log_base;
        if (cut != 0 && cut <= s.log_next - s.log_base) fq_cull(wv, sh, a, s, max_base);
      }
    }
  }
  // 4. forget_frames (:261-269)
  if (S.flags & UFC_FQ_FORGET) {
    const uint32_t len = s.log_next - s.log_base;
    uint32_t expired = 0;
    for (uint32_t t = 0; t < len; t += 64) {
      const uint32_t nv = len - t < 64 ? len - t : 64u;
      const unsigned long long kept = wv.ballot(
          [&](uint32_t lane) { return lane < nv && a.log[fq_slot(s, s.log_base + t + lane)].send_time_ms >= S.thresh_ms; });
      if (kept) {
        expired += low_bit(kept);
        break;
      }
      expired += nv;
    }
    if (expired) fq_cull(wv, sh, a, s, s.log_base + expired);
  }
  // 5. get_feedback (:126-147), the result and the state
  wv.one([&]() {
    ufc_frame_queue O = Q;
    ufc_frame_queue_result res = sh.res;
    res.stop = UFC_FQ_DONE;
    bool has_ack = sh.has_ack != 0;
    if ((S.flags & UFC_FQ_FEEDBACK) && has_ack) {
      res.has_feedback = 1;
      res.rtt_ms = S.now_ms - sh.ack_last;
      res.receive_rate = Q.has_last_feedback ? fq_receive_rate(sh.ack_total, S.now_ms - Q.last_feedback_ms) : 0;
      res.loss_rate = fq_loss_rate(sh.li_len, s.li_count);
      res.rate_limited = sh.ack_rl ? 1 : 0;
      O.has_last_feedback = 1;
      O.last_feedback_ms = S.now_ms;
      has_ack = false;
    }
    const uint32_t ahead = s.log_next - s.window_base;
    res.window_room = ahead < s.window_size ? s.window_size - ahead : 0;
    O.log_base_id = s.log_base;
    O.log_next_id = s.log_next;
    O.window_base_id = s.window_base;
    O.rb_base_id = s.rb_base;
    O.rb_frames[0] = s.rb_f0;
    O.rb_frames[1] = s.rb_f1;
    O.rb_count = s.rb_count;
    O.rate_limited = s.pending ? 1 : 0;
    O.has_ack_data = has_ack ? 1 : 0;
    O.ack_rate_limited = (has_ack && sh.ack_rl) ? 1 : 0;
    O.ack_last_send_time_ms = has_ack ? sh.ack_last : 0;
    O.ack_total_size = has_ack ? sh.ack_total : 0;
    O.li_count = s.li_count;
    for (uint32_t k = 0; k < kFqMaxIntervals; k++) {  // (the entries behind the count: zero)
      O.li_end_time_ms[k] = k < s.li_count ? sh.li_end[k] : 0;
      O.li_length[k] = k < s.li_count ? sh.li_len[k] : 0;
    }
    a.results[c] = res;
    a.queues_out[c] = O;
  });
}

// ---- batched send rate control (ufc_rate_begin_*, ufc_rate_step_*) ----
// SendRateComp and RecvRateSet (src/half_connection/send_rate.rs, recv_rate_set.rs) with HalfConnection's
// fill_flush_alloc, one connection per call of rate_step: the host entry loops over it, the kernel gives it a lane.
// Every float operation is written out one per statement under fp contract(off), so host and device round alike.
struct RateArgs {
  const ufc_rate_state* states;
  const ufc_rate_tick* ticks;
  const ufc_frame_queue_result* fq;
  size_t n;
  ufc_recv_rate_entry* entries;
  size_t n_entries;
  const ufc_flush_result* flush_results;
  size_t n_flush_results;
  const uint32_t* result_index;
  ufc_flush* flushes;
  size_t n_flushes;
  const uint32_t* flush_index;
  ufc_rate_result* results;
  ufc_rate_state* states_out;
};
struct RateBeginArgs {
  const ufc_rate_state* states;
  const uint64_t* now_ms;
  const uint32_t* extra_flags;
  size_t n;
  ufc_frame_queue_step* steps;
  ufc_rate_state* states_out;
};
inline bool rate_begin_args_ok(const RateBeginArgs& a) {
  return a.states && a.now_ms && a.steps && a.states_out && a.n < kCountLim;
}
inline bool rate_args_ok(const RateArgs& a) {
  const bool bad = !a.states || !a.ticks || !a.fq || !a.results || !a.states_out || (!a.entries && a.n_entries) ||
                   (a.flush_results && !a.result_index) || (a.flushes && !a.flush_index) || a.n >= kCountLim;
  return !bad;
}

constexpr uint32_t kRateMinimum = UFC_MAX_FRAME_SIZE / 64;  // MINIMUM_RATE
constexpr uint32_t kRateInitialWindow = 4380;               // INITIAL_TCP_WINDOW

// Rust's float casts: saturating, NaN gives 0.
UFC_HD uint32_t rate_f64_u32(double v) {
  if (!(v > 0.0)) return 0;
  if (v >= 4294967296.0) return 0xFFFFFFFFu;
  return (uint32_t)v;
}
UFC_HD uint64_t rate_f64_u64(double v) {
  if (!(v > 0.0)) return 0;
  if (v >= 18446744073709551616.0) return ~0ull;
  return (uint64_t)v;
}
UFC_HD int64_t rate_f64_i64(double v) {
  if (v != v) return 0;
  if (v >= 9223372036854775808.0) return INT64_MAX;
  if (v <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)v;
}
// f64::round: half away from zero.  v - t is exact, so no second rounding enters.
UFC_HD double rate_round(double v) {
#pragma clang fp contract(off)
  const double t = __builtin_trunc(v);
  const double d = v - t;
  if (d >= 0.5) return t + 1.0;
  if (d <= -0.5) return t - 1.0;
  return t;  // (an infinity or a NaN gives d = NaN and comes back as it is)
}
// f64::max: a NaN operand gives the other one.
UFC_HD double rate_max(double x, double y) {
  if (x != x) return y;
  if (y != y) return x;
  return x > y ? x : y;
}
UFC_HD uint32_t rate_min_u32(uint32_t x, uint32_t y) { return x < y ? x : y; }
UFC_HD uint32_t rate_max_u32(uint32_t x, uint32_t y) { return x > y ? x : y; }
UFC_HD uint32_t rate_sat_mul2(uint32_t v) { return v > 0x7FFFFFFFu ? 0xFFFFFFFFu : 2 * v; }
UFC_HD uint64_t rate_s_to_ms(double v_s) {  // send_rate.rs:16-18
#pragma clang fp contract(off)
  const double ms = v_s * 1000.0;
  return rate_f64_u64(rate_round(rate_max(ms, 0.0)));
}
UFC_HD uint32_t rate_initial_send_rate(double rtt_s) {  // :110-112
#pragma clang fp contract(off)
  const double v = (double)kRateInitialWindow / rtt_s;
  return rate_f64_u32(v);
}
// The equation's value before its cast (tests/c/float_paths_gpu.hip compares it as 64 bits).
UFC_HD double rate_tcp_throughput_f64(double rtt, double p) {  // :24-28
#pragma clang fp contract(off)
  const double s = (double)UFC_MAX_FRAME_SIZE;
  const double p2 = p * 2.0;
  const double q0 = p2 / 3.0;
  const double r0 = __builtin_sqrt(q0);
  const double p3 = p * 3.0;
  const double q1 = p3 / 8.0;
  const double r1 = __builtin_sqrt(q1);
  const double t0 = 12.0 * r1;
  const double t1 = t0 * p;
  const double u0 = 32.0 * p;
  const double u1 = u0 * p;
  const double u2 = 1.0 + u1;
  const double t2 = t1 * u2;
  const double f_p = r0 + t2;
  const double den = rtt * f_p;
  const double v = s / den;
  return v;
}
UFC_HD uint32_t rate_tcp_throughput(double rtt, double p) { return rate_f64_u32(rate_tcp_throughput_f64(rtt, p)); }
// eval_tcp_throughput_inv (:30-59) with the stall rule of the header: a midpoint equal to an end of the interval
// is returned where the reference would go round for ever.
UFC_HD double rate_tcp_throughput_inv(double rtt, uint32_t target, uint32_t& iterations, bool& stalled) {
#pragma clang fp contract(off)
  const double d = (double)target * 0.05;
  const uint32_t delta = rate_f64_u32(d);
  double a = 0.0, b = 1.0;
  iterations = 0;
  stalled = false;
  for (;;) {
    const double sum = b + a;
    const double c = sum / 2.0;
    const uint32_t rate = rate_tcp_throughput(rtt, c);
    iterations++;
    if (rate > target) {
      if (rate - target <= delta) return c;
    } else if (rate < target) {
      if (target - rate <= delta) return c;
    } else {
      return c;
    }
    if (c == a || c == b) {  // (a, b and c are never negative or NaN: equal values are equal bits)
      stalled = true;
      return c;
    }
    if (rate > target)
      a = c;
    else
      b = c;
  }
}
UFC_HD double rate_update_rto(ufc_rate_state& S, double rtt_s, uint32_t send_rate) {  // :381-386
#pragma clang fp contract(off)
  const double x = 4.0 * rtt_s;
  const double y = (double)(2 * UFC_MAX_FRAME_SIZE) / (double)send_rate;
  const double rto_s = rate_max(x, y);
  S.has_rto_ms = 1;
  S.rto_ms = rate_s_to_ms(rto_s);
  return rto_s;
}
UFC_HD ufc_recv_rate_entry rate_entry(uint64_t t, uint32_t value, bool initial) {
  ufc_recv_rate_entry e;
  e.timestamp_ms = t;
  e.value = value;
  e.is_initial = initial ? 1 : 0;
  e.reserved[0] = e.reserved[1] = e.reserved[2] = 0;
  return e;
}

// The set a step works on: the connection's entries as they lie in the arena, or the single entry a reset put in
// their place earlier in the same step.  What the step leaves behind is described, not stored, until it commits.
// The first kRateHeld entries are loaded together when the step begins, so that the loops over the set do not wait
// for one load after the other (a lane has nothing else to hide them behind); longer sets go on from memory.
constexpr uint32_t kRateHeld = 4;
struct RateSet {
  const ufc_recv_rate_entry* base;
  uint32_t count;
  bool single;
  ufc_recv_rate_entry e0;
  uint64_t held_t[kRateHeld];
  uint32_t held_v[kRateHeld];
  bool held_i[kRateHeld];
  UFC_HD void load() {
#pragma unroll
    for (uint32_t k = 0; k < kRateHeld; k++)
      if (k < count) {
        held_t[k] = base[k].timestamp_ms;
        held_v[k] = base[k].value;
        held_i[k] = base[k].is_initial != 0;
      }
  }
  UFC_HD uint32_t size() const { return single ? 1u : count; }
  // f(timestamp_ms, value, is_initial) for every entry in Vec order.  f may store into the arena at or before the
  // entry it is given.
  template <class F>
  UFC_HD void each(const F& f) const {
    if (single) {
      f(e0.timestamp_ms, e0.value, e0.is_initial != 0);
      return;
    }
#pragma unroll
    for (uint32_t k = 0; k < kRateHeld; k++)
      if (k < count) f(held_t[k], held_v[k], held_i[k]);
    for (uint32_t k = kRateHeld; k < count; k++) f(base[k].timestamp_ms, base[k].value, base[k].is_initial != 0);
  }
  UFC_HD void reset(const ufc_recv_rate_entry& e) {
    single = true;
    e0 = e;
  }
};

inline __host__ __device__ bool rate_state_ok(const ufc_rate_state& S, uint64_t n_entries) {
  if (S.mode > UFC_RATE_THROUGHPUT_EQN || S.recv_cap == 0 || S.recv_count > S.recv_cap) return false;
  if (S.recv_first > n_entries || n_entries - S.recv_first < S.recv_cap) return false;
  if (S.mode != UFC_RATE_AWAIT_SEND && S.recv_count == 0) return false;
  if (S.mode == UFC_RATE_THROUGHPUT_EQN && !S.has_rtt_s) return false;
  return true;
}

// One connection's step.  `S` comes in as the state and goes out as states_out's record; the entries and the
// gathered flush are written here, once nothing can stop the step any more.
inline __host__ __device__ void rate_step(const RateArgs& a, uint64_t c, ufc_rate_state& S, const ufc_rate_tick& T,
                                          const ufc_frame_queue_result& F, ufc_rate_result& R) {
#pragma clang fp contract(off)
  R = ufc_rate_result{};
  if (!rate_state_ok(S, a.n_entries)) {
    R.stop = UFC_RATE_BAD_STATE;
    return;
  }
  const ufc_rate_state in = S;
  ufc_recv_rate_entry* const arena = a.entries + S.recv_first;
  RateSet set;
  set.base = arena;
  set.count = S.recv_count;
  set.single = false;
  set.load();
  // (the Option bits as 0 / 1, the values behind a clear bit as 0)
  S.has_time_last_doubled = S.mode == UFC_RATE_SLOW_START && S.has_time_last_doubled;
  S.has_nofeedback_exp = S.has_nofeedback_exp != 0;
  S.nofeedback_idle = S.nofeedback_idle != 0;
  S.has_rtt_s = S.has_rtt_s != 0;
  S.has_rtt_ms = S.has_rtt_ms != 0;
  S.has_rto_ms = S.has_rto_ms != 0;
  S.has_reset = S.has_reset != 0;
  if (!S.has_time_last_doubled) S.time_last_doubled_ms = 0;
  if (!S.has_nofeedback_exp) S.nofeedback_exp_ms = 0;
  if (!S.has_rtt_s) S.rtt_s = 0.0;
  if (!S.has_rtt_ms) S.rtt_ms = 0;
  if (!S.has_rto_ms) S.rto_ms = 0;
  if (!S.has_reset) S.reset_loss_rate = 0.0;
  if (S.mode != UFC_RATE_THROUGHPUT_EQN) S.send_rate_tcp = 0;

  // 1. the last flush's accounting
  int64_t alloc = S.flush_alloc;
  bool sent = (T.flags & UFC_RATE_FRAME_SENT) != 0;
  if (a.flush_results) {
    const uint32_t i = a.result_index[c];
    if (i < a.n_flush_results) {
      alloc = a.flush_results[i].alloc_left;
      sent = sent || a.flush_results[i].frame_count > 0;
    }
  }
  alloc = (int64_t)((uint64_t)alloc + (uint64_t)T.alloc_adjust);
  if (sent) {  // notify_frame_sent(now_ms of that flush), :155-168
    if (S.mode == UFC_RATE_AWAIT_SEND) {
      S.has_nofeedback_exp = 1;
      S.nofeedback_exp_ms = S.now_ms + 2000;
      S.mode = UFC_RATE_SLOW_START;
      set.reset(rate_entry(S.now_ms, 0xFFFFFFFFu, true));
    }
    S.nofeedback_idle = 0;
  }
  // 2. the values the coming flush uses
  const uint64_t now = T.now_ms;
  S.now_ms = now;
  const uint64_t flush_rtt_ms = S.has_rtt_ms ? S.rtt_ms : 150, flush_rto_ms = S.has_rto_ms ? S.rto_ms : 600;
  // 3. fill_flush_alloc, mod.rs:200-215
  if (S.has_last_flush) {
    const double rate = (double)S.send_rate;
    const double nb = rate * T.delta_time_s;
    const double am = rate * (S.has_rtt_s ? S.rtt_s : 0.0);
    const int64_t new_bytes = rate_f64_i64(rate_round(nb)), alloc_max = rate_f64_i64(rate_round(am));
    int64_t sum;
    if (__builtin_add_overflow(alloc, new_bytes, &sum)) sum = new_bytes < 0 ? INT64_MIN : INT64_MAX;
    alloc = sum < alloc_max ? sum : alloc_max;
  }
  S.has_last_flush = 1;
  S.flush_alloc = alloc;

  // 4. SendRateComp::step, :170-185
  uint32_t flags = 0, iterations = 0;
  bool append = false;       // a rate-limited update: the survivors of `set`, then `fresh`
  uint64_t two_rtt = 0;
  ufc_recv_rate_entry fresh = {};
  if (S.mode != UFC_RATE_AWAIT_SEND && F.has_feedback) {  // handle_feedback, :187-284
    flags |= UFC_RATE_FEEDBACK;
    const double rtt_sample_s = (double)F.rtt_ms / 1000.0;
    double rtt_s = rtt_sample_s;  // update_rtt, :367-379
    if (S.has_rtt_s) {
      const double keep = (1.0 - 0.1) * S.rtt_s;
      const double take = 0.1 * rtt_sample_s;
      rtt_s = keep + take;
    }
    const uint64_t rtt_ms = rate_s_to_ms(rtt_s);
    S.has_rtt_s = S.has_rtt_ms = 1;
    S.rtt_s = rtt_s;
    S.rtt_ms = rtt_ms;
    const double rto_s = rate_update_rto(S, rtt_s, S.send_rate);
    const double loss_rate = F.loss_rate;
    const bool loss_increase = loss_rate > S.prev_loss_rate;
    uint32_t recv_limit;
    if (F.rate_limited) {  // rate_limited_update, recv_rate_set.rs:55-65
      two_rtt = 2 * rtt_ms;
      uint32_t kept = 0, max_val = 0;
      set.each([&](uint64_t t, uint32_t value, bool) {
        if (now - t < two_rtt) {
          kept++;
          max_val = rate_max_u32(max_val, value);
        }
      });
      if (two_rtt == 0) {  // (not even the new entry, of age 0, stays: max() unwraps None)
        S = in;
        R.stop = UFC_RATE_REF_PANIC;
        return;
      }
      if (kept >= S.recv_cap) {
        S = in;
        R.stop = UFC_RATE_RECV_FULL;
        return;
      }
      append = true;
      fresh = rate_entry(now, F.receive_rate, false);
      max_val = rate_max_u32(max_val, F.receive_rate);
      recv_limit = rate_sat_mul2(max_val);
    } else {  // loss_increase_update / data_limited_update through replace_max, :31-43, :67-77
      uint32_t recv_rate = F.receive_rate;
      if (loss_increase) {
        const double scaled = (double)recv_rate * 0.85;
        recv_rate = rate_f64_u32(scaled);
      }
      uint32_t max_rate = recv_rate;
      set.each([&](uint64_t, uint32_t value, bool initial) {
        if (!initial) max_rate = rate_max_u32(max_rate, loss_increase ? value / 2 : value);
      });
      set.reset(rate_entry(now, max_rate, false));
      recv_limit = loss_increase ? max_rate : rate_sat_mul2(max_rate);
    }
    S.prev_loss_rate = loss_rate;
    if (S.mode == UFC_RATE_SLOW_START) {
      if (loss_increase) {  // section 6.3.1: into the throughput equation
        uint32_t target;
        if (!S.has_time_last_doubled) {
          const double v = (double)(UFC_MAX_FRAME_SIZE / 2) / rtt_s;  // compute_initial_loss_send_rate
          target = rate_f64_u32(v);
        } else {
          target = S.send_rate / 2;
        }
        bool stalled;
        const double initial_p = rate_tcp_throughput_inv(rtt_s, target, iterations, stalled);
        S.has_reset = 1;
        S.reset_loss_rate = initial_p;
        flags |= UFC_RATE_RESET_ISSUED | UFC_RATE_ENTERED_EQN | (stalled ? UFC_RATE_INV_STALLED : 0);
        S.send_rate = rate_max_u32(rate_min_u32(target, recv_limit), kRateMinimum);
        S.mode = UFC_RATE_THROUGHPUT_EQN;
        S.send_rate_tcp = target;
        S.has_time_last_doubled = 0;
        S.time_last_doubled_ms = 0;
      } else {
        const uint32_t initial_rate = rate_initial_send_rate(rtt_s);
        if (S.has_time_last_doubled) {
          if (now - S.time_last_doubled_ms >= rtt_ms) {
            S.time_last_doubled_ms = now;
            S.send_rate = rate_max_u32(rate_min_u32(2 * S.send_rate, recv_limit), initial_rate);
          }
        } else {
          S.has_time_last_doubled = 1;
          S.time_last_doubled_ms = now;
          S.send_rate = initial_rate;
        }
      }
    } else {
      S.send_rate_tcp = rate_tcp_throughput(rtt_s, loss_rate);
      S.send_rate = rate_max_u32(rate_min_u32(S.send_rate_tcp, recv_limit), kRateMinimum);
    }
    S.send_rate = rate_min_u32(S.send_rate, S.max_send_rate);
    S.has_nofeedback_exp = 1;
    S.nofeedback_exp_ms = now + rate_s_to_ms(rto_s);
    S.nofeedback_idle = 1;
  } else if (S.mode != UFC_RATE_AWAIT_SEND && S.has_nofeedback_exp && now >= S.nofeedback_exp_ms) {
    flags |= UFC_RATE_NOFEEDBACK;  // nofeedback_expired, :286-365
    if (S.mode == UFC_RATE_SLOW_START) {
      bool halve = true;
      if (S.has_rtt_s) {
        const uint32_t recover_rate = rate_initial_send_rate(S.rtt_s);
        halve = !(S.nofeedback_idle && S.send_rate < 2 * recover_rate);
      }
      if (halve) S.send_rate = rate_max_u32(S.send_rate / 2, kRateMinimum);
    } else {
      const uint32_t recover_rate = rate_initial_send_rate(S.rtt_s);
      uint32_t recv_rate = 0;  // max(), :79-87, of a set the state check found non-empty
      set.each([&](uint64_t, uint32_t value, bool) { recv_rate = rate_max_u32(recv_rate, value); });
      if (!(S.nofeedback_idle && recv_rate < recover_rate)) {
        const uint32_t current_limit = rate_min_u32(S.send_rate_tcp, rate_sat_mul2(recv_rate));
        const uint32_t new_limit = rate_max_u32(current_limit / 2, kRateMinimum);
        set.reset(rate_entry(now, new_limit / 2, false));
        S.send_rate = rate_min_u32(S.send_rate_tcp, new_limit);
      }
    }
    const double rto_s = rate_update_rto(S, S.has_rtt_s ? S.rtt_s : 0.0, S.send_rate);
    S.nofeedback_exp_ms = now + rate_s_to_ms(rto_s);
    S.nofeedback_idle = 1;
  }

  // 5. commit: the set, the flush, the result
  uint32_t count = 0;
  if (append) {
    set.each([&](uint64_t t, uint32_t value, bool initial) {  // (retain in place: never ahead of the entry read)
      if (now - t < two_rtt) arena[count++] = rate_entry(t, value, initial);
    });
    arena[count++] = fresh;
  } else if (set.single) {
    arena[0] = set.e0;
    count = 1;
  } else {
    count = set.count;
  }
  S.recv_count = count;
  if (a.flushes) {
    const uint32_t j = a.flush_index[c];
    if (j < a.n_flushes) a.flushes[j].flush_alloc = alloc;
  }
  R.mode = S.mode;
  R.now_ms = now;
  R.rtt_ms = flush_rtt_ms;
  R.rto_ms = flush_rto_ms;
  R.flush_alloc = alloc;
  R.send_rate = S.send_rate;
  R.flags = flags;
  R.inv_iterations = iterations;
  R.recv_count = count;
}

// One connection of ufc_rate_begin_*: the frame queue's step record, and the pending reset taken.
inline __host__ __device__ void rate_begin(ufc_rate_state& S, uint64_t now, uint32_t extra, ufc_frame_queue_step& Q) {
  const uint64_t rtt = S.has_rtt_ms ? S.rtt_ms : 150;
  const uint64_t back = rtt * 4;
  Q.flags = UFC_FQ_FORGET | UFC_FQ_FEEDBACK | (S.has_rtt_ms ? UFC_FQ_HAS_RTT : 0) | (S.has_reset ? UFC_FQ_RESET_LOSS : 0) |
            extra;
  Q.reserved = 0;
  Q.rtt_ms = S.has_rtt_ms ? S.rtt_ms : 0;
  Q.thresh_ms = now > back ? now - back : 0;
  Q.now_ms = now;
  Q.reset_loss_rate = S.has_reset ? S.reset_loss_rate : 0.0;
  S.has_reset = 0;
  S.reset_loss_rate = 0.0;
}

// ---- batched resend (ufc_resend_begin_*, ufc_resend_place_*, ufc_resend_commit_*) ----
// PacketSender::acknowledge (packet_sender.rs:242-275), the resend queue (resend_queue.rs over std's BinaryHeap),
// the pending queue and emit_data_frames (half_connection/mod.rs:335-432); the rules are in
// include/uflow_frame_codec.h.  Written once against a wave policy, as fq_step is, with two additions:
//   Wv::sum(f)   the sum of f(lane) over the 64 lanes, the same in every lane
//   Wv::sync()   what Wv::one wrote (to memory or to `sh`) is visible to every lane after it
// One wave runs a connection.  The running state (ids, alloc, counters) is the same in every lane; the heap and the
// pack rule are a dependent chain and run inside Wv::one; everything that touches a run of records takes a lane per
// record: the live refs, the slots acknowledge frees, the pending fragments' items, commit's table entries, ack
// bytes and refs.

// DataFrameEmitter::push and finalize as a state machine (emit.rs:47-125; steps 1-4 of the ufc_flush comment): what
// the batched packs compute in closed form, item by item, for a caller that has to decide after each push.
struct PackRun {
  int64_t alloc;   // flush_alloc
  uint64_t s;      // the frame in progress with its overhead; 0 = none
  uint32_t frames; // frames finalized
  uint32_t cnt;    // items in the frame in progress
};
UFC_HD PackRun pack_run_begin(const ufc_flush& fl) { return PackRun{fl.flush_alloc, 0, 0, 0}; }
UFC_HD void pack_finalize(PackRun& r) {
  if (r.s == 0) return;
  r.frames++;
  r.alloc = (int64_t)((uint64_t)r.alloc - r.s);
  r.s = 0;
  r.cnt = 0;
}
// UFC_PACK_DONE when the item (e encoded bytes) went in, else why the flush stops at it.
UFC_HD uint32_t pack_push(PackRun& r, const ufc_flush& fl, bool ack, uint64_t e) {
  if (r.s) {
    if (r.alloc < (int64_t)r.s) {  // :64-68
      pack_finalize(r);
      return UFC_PACK_SIZE_LIMITED;
    }
    if (pack_frame_takes(r.s, r.cnt, e, pack_max_count(ack))) {
      r.s += e;
      r.cnt++;
      return UFC_PACK_DONE;
    }
    pack_finalize(r);  // :69-71
  }
  if (r.alloc < 0) return UFC_PACK_SIZE_LIMITED;                       // :83-87
  if (!ack && r.frames >= fl.window_room) return UFC_PACK_WINDOW_LIMITED;  // :89-92
  r.s = pack_overhead(ack) + e;
  r.cnt = 1;
  return UFC_PACK_DONE;
}

// std's BinaryHeap over d[0 .. len), Ord reversed on resend_time (resend_queue.rs:20-38): "a <= b".
UFC_HD bool rs_le(const ufc_resend_entry& x, const ufc_resend_entry& y) { return x.resend_time_ms >= y.resend_time_ms; }
inline __host__ __device__ void rs_sift_up(ufc_resend_entry* d, uint32_t start, uint32_t pos) {
  const ufc_resend_entry elem = d[pos];
  while (pos > start) {
    const uint32_t parent = (pos - 1) / 2;
    if (rs_le(elem, d[parent])) break;
    d[pos] = d[parent];
    pos = parent;
  }
  d[pos] = elem;
}
inline __host__ __device__ void rs_heap_push(ufc_resend_entry* d, uint32_t& len, const ufc_resend_entry& x) {
  d[len] = x;
  len++;
  rs_sift_up(d, 0, len - 1);
}
inline __host__ __device__ ufc_resend_entry rs_heap_pop(ufc_resend_entry* d, uint32_t& len) {  // len > 0
  len--;
  ufc_resend_entry item = d[len];
  if (len > 0) {
    const ufc_resend_entry root = d[0];
    // sift_down_to_bottom(0) of the old last entry, then sift_up
    const uint32_t end = len;
    uint32_t pos = 0, child = 1;
    while (child + 1 < end) {
      child += rs_le(d[child], d[child + 1]) ? 1u : 0u;
      d[pos] = d[child];
      pos = child;
      child = 2 * pos + 1;
    }
    if (child == end - 1) {
      d[pos] = d[child];
      pos = child;
    }
    d[pos] = item;
    rs_sift_up(d, 0, pos);
    item = root;
  }
  return item;
}
UFC_HD ufc_resend_entry rs_entry(uint64_t t, uint32_t seq, uint32_t frag, uint8_t count) {
  ufc_resend_entry e{};
  e.resend_time_ms = t;
  e.sequence_id = seq;
  e.fragment_id = (uint16_t)frag;
  e.send_count = count;
  return e;
}

struct RsBeginArgs {
  const ufc_frame_info* infos;
  uint64_t n_frames;
  const uint64_t* frame_first;
  const ufc_frame_queue* queues;
  const ufc_sent_frame* log;
  uint64_t n_log;
  const ufc_rate_result* rate;
  const uint32_t* flags;
  const ufc_flush* flushes;
  const ufc_resend* states;
  const ufc_sender* senders;
  uint64_t n;
  ufc_resend_entry* heap;
  uint64_t n_heap;
  const ufc_sent_packet* pkts;
  uint64_t n_pkts;
  uint8_t* frag_acked;
  uint64_t n_frag;
  const ufc_tx_ref* tx;
  uint64_t n_tx;
  uint8_t* ref_acked;
  uint64_t refs_cap;
  ufc_item* stage;
  uint64_t n_stage;
  ufc_resend_result* results;
  ufc_resend* states_out;
  ufc_sender* senders_out;
};

struct RsPlaceArgs {
  const ufc_resend* states;
  const ufc_resend_result* begin_results;
  uint64_t n;
  const ufc_item* stage;
  uint64_t n_stage;
  const uint64_t* flush_first;
  ufc_item* items;
  uint64_t items_cap;
};

struct RsCommitArgs {
  const ufc_flush_result* flush_results;
  const ufc_frame_info* infos;
  uint64_t n_infos;
  const uint64_t* out_offsets;
  const uint64_t* frames_used;
  const ufc_item* items;
  uint64_t n_items;
  const uint64_t* flush_first;
  const ufc_packet* packets;
  uint64_t n_packets;
  const uint64_t* packet_first;
  const ufc_packet_result* packet_results;
  const ufc_sender_result* sender_results;
  const ufc_resend_result* begin_results;
  const ufc_rate_result* rate;
  const ufc_resend* states;
  const ufc_sender* senders;
  uint64_t n;
  ufc_resend_entry* heap;
  uint64_t n_heap;
  ufc_sent_packet* pkts;
  uint64_t n_pkts;
  uint8_t* frag_acked;
  uint64_t n_frag;
  ufc_tx_ref* tx;
  uint64_t n_tx;
  ufc_sent_frame* sent;
  uint64_t sent_cap;
  uint64_t* sent_first;
  uint32_t* next_extra_flags;
  ufc_resend_commit_result* results;
  ufc_resend* states_out;
  ufc_sender* retake;
};
inline bool rs_begin_args_ok(const RsBeginArgs& a) {
  const bool bad = !a.frame_first || !a.queues || !a.rate || !a.flushes || !a.states || !a.senders || !a.results ||
                   !a.states_out || !a.senders_out || (!a.infos && a.n_frames) || (!a.log && a.n_log) ||
                   (!a.heap && a.n_heap) || (!a.pkts && a.n_pkts) || (!a.frag_acked && a.n_frag) || (!a.tx && a.n_tx) ||
                   (!a.stage && a.n_stage) || a.n >= kCountLim || a.n_frames >= kCountLim;
  return !bad;
}
inline bool rs_place_args_ok(const RsPlaceArgs& a) {
  const bool bad = !a.states || !a.begin_results || !a.flush_first || (!a.stage && a.n_stage) ||
                   (!a.items && a.items_cap) || a.n >= kCountLim;
  return !bad;
}
inline bool rs_commit_args_ok(const RsCommitArgs& a) {
  const bool bad = !a.flush_results || !a.out_offsets || !a.frames_used || !a.flush_first || !a.packet_first ||
                   !a.sender_results || !a.begin_results || !a.rate || !a.states || !a.senders || !a.sent_first ||
                   !a.results || !a.states_out || !a.retake || (!a.infos && a.n_infos) || (!a.items && a.n_items) ||
                   (!a.packets && a.n_packets) || (!a.packet_results && a.n_packets) || (!a.heap && a.n_heap) ||
                   (!a.pkts && a.n_pkts) || (!a.frag_acked && a.n_frag) || (!a.tx && a.n_tx) ||
                   (!a.sent && a.sent_cap) || a.n >= kCountLim || a.n_packets >= kCountLim || a.n_items >= kCountLim ||
                   a.n_infos >= kCountLim;
  return !bad;
}

struct RsWaveShared {
  uint32_t chan_parent[UFC_MAX_CHANNELS];
  // written by Wv::one, read by all behind Wv::sync
  uint32_t stop, n_resent, dead, acked, heap_len, pushed, dropped;
};

UFC_HD bool rs_pow2(uint32_t v) { return v != 0 && (v & (v - 1)) == 0; }
UFC_HD bool rs_region_ok(uint64_t first, uint64_t cap, uint64_t n) { return first <= n && n - first >= cap; }
// The checks of the header comment that begin and commit share.
UFC_HD bool rs_state_ok(const ufc_resend& R, const ufc_sender& S, uint64_t n_heap, uint64_t n_pkts, uint64_t n_frag,
                        uint64_t n_tx, uint64_t n_stage, bool with_stage) {
  if (!rs_pow2(R.pkt_cap) || !rs_pow2(R.frag_cap) || !rs_pow2(R.tx_cap)) return false;
  if (S.window_size == 0 || S.window_size > kPacketIdMask + 1 || R.pkt_cap < S.window_size) return false;
  if (emit_max_alloc(S.max_alloc) / UFC_MAX_FRAGMENT_SIZE + S.window_size > R.frag_cap) return false;
  if (n_tx > 0x100000000ull) return false;
  if (!rs_region_ok(R.heap_first, R.heap_cap, n_heap) || !rs_region_ok(R.pkt_first, R.pkt_cap, n_pkts) ||
      !rs_region_ok(R.frag_first, R.frag_cap, n_frag) || !rs_region_ok(R.tx_first, R.tx_cap, n_tx) ||
      (with_stage && !rs_region_ok(R.stage_first, R.stage_cap, n_stage)))
    return false;
  if (R.heap_len > R.heap_cap || R.tx_head - R.tx_tail > R.tx_cap) return false;
  return true;
}
// One Entry of the frame log as commit hands it to the next tick's push (written field by field: no record on the
// stack).
UFC_HD void rs_put_sent(ufc_sent_frame& o, uint64_t now, uint32_t size, uint32_t ref_first, uint32_t ref_count, uint32_t aux) {
  o.send_time_ms = now;
  o.size = size;
  o.ref_first = ref_first;
  o.ref_count = ref_count;
  o.flags = (aux & 1) ? UFC_SENT_NONCE : 0;
  o.reserved[0] = 0;
  o.reserved[1] = 0;
  o.reserved[2] = 0;
}
// A state record written field by field (a whole-record copy keeps its untouched bytes on the stack).
UFC_HD void rs_put_state(ufc_resend& o, const ufc_resend& r) {
  o.heap_first = r.heap_first;
  o.heap_cap = r.heap_cap;
  o.heap_len = r.heap_len;
  o.pkt_first = r.pkt_first;
  o.pkt_cap = r.pkt_cap;
  o.frag_next = r.frag_next;
  o.frag_first = r.frag_first;
  o.frag_cap = r.frag_cap;
  o.tx_cap = r.tx_cap;
  o.tx_first = r.tx_first;
  o.tx_head = r.tx_head;
  o.tx_tail = r.tx_tail;
  o.stage_first = r.stage_first;
  o.stage_cap = r.stage_cap;
  o.pending_seq = r.pending_seq;
  o.pending_next = r.pending_next;
  o.pending_count = r.pending_count;
  o.pending_resend = r.pending_resend;
  o.reserved0 = r.reserved0;
  o.reserved1 = r.reserved1;
  o.reserved2 = r.reserved2;
  o.window_bytes = r.window_bytes;
}
// A ufc_sender without its channel parents (they go lane by lane).
struct RsSenderHead {
  uint32_t base_id, next_id, window_size, flush_id;
  uint64_t alloc, max_alloc;
  uint32_t window_parent_id, take, reserve_items, reserved;
};
UFC_HD void rs_put_sender(ufc_sender& O, const RsSenderHead& h) {
  O.base_id = h.base_id;
  O.next_id = h.next_id;
  O.window_size = h.window_size;
  O.flush_id = h.flush_id;
  O.alloc = h.alloc;
  O.max_alloc = h.max_alloc;
  O.window_parent_id = h.window_parent_id;
  O.take = h.take;
  O.reserve_items = h.reserve_items;
  O.reserved = h.reserved;
}
// PendingPacket::datagram of a table packet (pending_packet.rs:84-103), as the emit makes its items.
UFC_HD ufc_item rs_item(const ufc_sent_packet& k, uint32_t seq, uint32_t f) {
  ufc_packet p{};
  p.data_offset = k.data_offset;
  p.data_len = k.data_len;
  p.channel_id = k.channel_id;
  return emit_item(p, seq, k.window_parent_lead, k.channel_parent_lead, f, emit_fragment_count(k.data_len) - 1);
}

template <class Wv>
inline __host__ __device__ void rs_begin(const Wv& wv, RsWaveShared& sh, const RsBeginArgs& a, uint64_t c) {
  // (read in place: the outputs, which may be the inputs, are written last, behind every read)
  const ufc_resend R = a.states[c];
  const ufc_sender& S = a.senders[c];
  const ufc_frame_queue& Q = a.queues[c];
  const uint64_t ff0 = a.frame_first[c], ff1 = a.frame_first[c + 1];
  const uint32_t window_size = S.window_size, flush_id = S.flush_id, in_take = S.take, s_reserved = S.reserved;
  const uint64_t max_alloc = S.max_alloc;
  uint32_t base = S.base_id, wparent = S.window_parent_id;
  const uint32_t next = S.next_id;
  uint64_t alloc = S.alloc;
  wv.lanes([&](uint32_t lane) { sh.chan_parent[lane] = S.channel_parent_id[lane]; });
  bool ok = rs_state_ok(R, S, a.n_heap, a.n_pkts, a.n_frag, a.n_tx, a.n_stage, true) && ff0 <= ff1 && ff1 <= a.n_frames &&
            rs_pow2(Q.log_cap) && rs_region_ok(Q.log_first, Q.log_cap, a.n_log) &&
            ((uint64_t)Q.window_size + Q.tail_size + 1) * UFC_DATA_FRAME_MAX_DATAGRAM_COUNT <= R.tx_cap;
  if (!ok) {  // (every lane takes this branch or none)
    wv.lanes([&](uint32_t lane) { a.senders_out[c].channel_parent_id[lane] = sh.chan_parent[lane]; });
    wv.one([&]() {
      ufc_resend_result res{};
      res.stop = UFC_RS_BAD_STATE;
      a.results[c] = res;
      rs_put_state(a.states_out[c], R);
      rs_put_sender(a.senders_out[c], RsSenderHead{base, next, window_size, flush_id, alloc, max_alloc, wparent, 0, 0, s_reserved});
    });
    return;
  }
  const uint32_t pmask = R.pkt_cap - 1, fmask = R.frag_cap - 1, tmask = R.tx_cap - 1;
  const ufc_sent_packet* pk = a.pkts + R.pkt_first;
  uint8_t* fa = a.frag_acked + R.frag_first;
  // 1. ack propagation over the live refs, then the tail
  uint32_t refs_acked = 0;
  const uint32_t live = R.tx_head - R.tx_tail;
  if (a.ref_acked) {
    const uint32_t span0 = packet_id_sub(next, base);
    for (uint32_t t = 0; t < live; t += 64)
      refs_acked += (uint32_t)wv.sum([&](uint32_t lane) -> uint64_t {
        const uint32_t j = t + lane;
        if (j >= live) return 0;
        const uint64_t r = R.tx_first + ((R.tx_tail + j) & tmask);
        if (r >= a.refs_cap || a.ref_acked[r] == 0) return 0;
        a.ref_acked[r] = 0;
        const ufc_tx_ref ref = a.tx[r];
        if (!(ref.flags & UFC_TX_RESEND) || packet_id_sub(ref.sequence_id, base) >= span0) return 0;
        const ufc_sent_packet k = pk[ref.sequence_id & pmask];
        if (ref.fragment_id >= emit_fragment_count(k.data_len)) return 0;
        fa[(k.frag_first + ref.fragment_id) & fmask] = 1;
        return 1;
      });
  }
  uint32_t tail = R.tx_head;
  if (Q.log_next_id != Q.log_base_id) {
    const uint64_t rf = a.log[Q.log_first + (Q.log_base_id & (Q.log_cap - 1))].ref_first;
    tail = (rf >= R.tx_first && rf - R.tx_first < R.tx_cap) ? R.tx_head - ((R.tx_head - (uint32_t)(rf - R.tx_first)) & tmask)
                                                           : R.tx_tail;
  }
  // 2. acknowledge for the ack frames in arrival order
  uint32_t freed = 0, ignored = 0;
  uint64_t bytes_freed = 0, window_bytes = R.window_bytes;
  for (uint64_t t0 = ff0; t0 < ff1; t0 += 64) {
    const uint32_t nv = ff1 - t0 < 64 ? (uint32_t)(ff1 - t0) : 64u;
    unsigned long long acks = wv.ballot([&](uint32_t lane) { return lane < nv && fq_is_ack(a.infos[t0 + lane]); });
    for (; acks; acks &= acks - 1) {
      const uint32_t rb = a.infos[t0 + low_bit(acks)].f[1];
      const uint32_t delta = packet_id_sub(rb, base), span = packet_id_sub(next, base);
      if (rb > kPacketIdMask || delta > span) {  // :246
        ignored++;
        continue;
      }
      for (uint32_t t = 0; t < delta; t += 64) {
        const uint32_t m = delta - t < 64 ? delta - t : 64u, first = packet_id_add(base, t);
        if (wv.ballot([&](uint32_t lane) { return lane < m && wparent == packet_id_add(first, lane); })) wparent = UFC_NO_PARENT;
        alloc -= wv.sum([&](uint32_t lane) -> uint64_t {
          return lane < m ? emit_alloc_size(pk[packet_id_add(first, lane) & pmask].data_len) : 0;
        });
        const uint64_t len = wv.sum([&](uint32_t lane) -> uint64_t {
          return lane < m ? pk[packet_id_add(first, lane) & pmask].data_len : 0;
        });
        window_bytes -= len;
        bytes_freed += len;
        wv.lanes([&](uint32_t lane) {  // (one id matches a channel's parent at most)
          if (lane >= m) return;
          const uint32_t id = packet_id_add(first, lane), ch = pk[id & pmask].channel_id & (UFC_MAX_CHANNELS - 1);
          if (sh.chan_parent[ch] == id) sh.chan_parent[ch] = UFC_NO_PARENT;
        });
      }
      freed += delta;
      base = rb;
    }
  }
  // 3. the resend loop, in one lane
  const bool no_flush = a.flags && (a.flags[c] & UFC_RS_NO_DATA_FLUSH);
  const uint64_t now = a.rate[c].now_ms, rtt = a.rate[c].rtt_ms;
  const uint32_t span = packet_id_sub(next, base);
  ufc_item* stage = a.stage + R.stage_first;
  wv.one([&]() {
    ufc_resend_entry* d = a.heap + R.heap_first;
    const ufc_flush fl = a.flushes[c];
    PackRun run = pack_run_begin(fl);
    uint32_t len = R.heap_len, n = 0, stop = UFC_RS_DONE, dead = 0, acked = 0;
    while (!no_flush && len > 0) {
      const ufc_resend_entry e = d[0];
      if (packet_id_sub(e.sequence_id, base) >= span) {  // Weak::upgrade fails, :379-382
        rs_heap_pop(d, len);
        dead++;
        continue;
      }
      const ufc_sent_packet k = pk[e.sequence_id & pmask];
      if (fa[(k.frag_first + e.fragment_id) & fmask]) {  // :355-358
        rs_heap_pop(d, len);
        acked++;
        continue;
      }
      if (e.resend_time_ms > now) break;  // :360
      if (n >= R.stage_cap) {
        stop = UFC_RS_STAGE_FULL;
        break;
      }
      const ufc_item it = rs_item(k, e.sequence_id, e.fragment_id);
      const uint32_t st = pack_push(run, fl, false, datagram_encoded_size(it));
      if (st != UFC_PACK_DONE) {
        stop = st == UFC_PACK_SIZE_LIMITED ? UFC_RS_SIZE_LIMITED : UFC_RS_WINDOW_LIMITED;
        break;
      }
      stage[n++] = it;
      ufc_resend_entry x = rs_heap_pop(d, len);  // :371-378
      x.resend_time_ms = now + rtt * ((uint64_t)1 << (x.send_count & 63u));
      const uint8_t up = (uint8_t)(x.send_count + 1);
      x.send_count = up < 2 ? up : (uint8_t)2;
      rs_heap_push(d, len, x);
    }
    sh.stop = stop;
    sh.n_resent = n;
    sh.dead = dead;
    sh.acked = acked;
    sh.heap_len = len;
  });
  wv.sync();
  uint32_t stop = sh.stop, n_pending = 0;
  const uint32_t n_resent = sh.n_resent;
  // 4. the pending front, then the pending fragments' items
  if (stop == UFC_RS_DONE && !no_flush && R.pending_count) {
    const ufc_sent_packet k = pk[R.pending_seq & pmask];
    if (packet_id_sub(R.pending_seq, base) >= span || fa[(k.frag_first + R.pending_next) & fmask]) {
      stop = UFC_RS_REF_HANG;
    } else if ((uint64_t)n_resent + R.pending_count > R.stage_cap) {
      stop = UFC_RS_STAGE_FULL;
    } else {
      n_pending = R.pending_count;
      for (uint32_t t = 0; t < n_pending; t += 64)
        wv.lanes([&](uint32_t lane) {
          const uint32_t j = t + lane;
          if (j < n_pending) stage[n_resent + j] = rs_item(k, R.pending_seq, R.pending_next + j);
        });
    }
  }
  // 5. the outputs
  wv.lanes([&](uint32_t lane) { a.senders_out[c].channel_parent_id[lane] = sh.chan_parent[lane]; });
  wv.one([&]() {
    ufc_resend_result res{};
    res.stop = stop;
    res.n_resent = n_resent;
    res.n_pending_staged = n_pending;
    res.heap_popped_dead = sh.dead;
    res.heap_popped_acked = sh.acked;
    res.packets_freed = freed;
    res.refs_acked = refs_acked;
    res.heap_len = sh.heap_len;
    res.pending_count = R.pending_count;
    res.acks_ignored = ignored;
    res.bytes_freed = bytes_freed;
    a.results[c] = res;
    ufc_resend& O = a.states_out[c];
    rs_put_state(O, R);
    O.heap_len = sh.heap_len;
    O.tx_tail = tail;
    O.window_bytes = window_bytes;
    rs_put_sender(a.senders_out[c], RsSenderHead{base, next, window_size, flush_id, alloc, max_alloc, wparent,
                                                 (stop == UFC_RS_DONE && !no_flush) ? in_take : 0u, n_resent + n_pending,
                                                 s_reserved});
  });
}

// One connection's staged items into the slots the emit reserved; lanes over the items.
template <class Wv>
inline __host__ __device__ void rs_place(const Wv& wv, const RsPlaceArgs& a, uint64_t c) {
  const ufc_resend& R = a.states[c];
  const ufc_resend_result& B = a.begin_results[c];
  if (B.stop == UFC_RS_BAD_STATE || !rs_region_ok(R.stage_first, R.stage_cap, a.n_stage)) return;
  const uint64_t f0 = a.flush_first[c], f1 = a.flush_first[c + 1];
  if (f1 < f0) return;
  uint64_t n = (uint64_t)B.n_resent + B.n_pending_staged;
  if (n > R.stage_cap) n = R.stage_cap;
  if (n > f1 - f0) n = f1 - f0;
  for (uint64_t t = 0; t < n; t += 64)
    wv.lanes([&](uint32_t lane) {
      const uint64_t j = t + lane;
      if (j < n && f0 + j < a.items_cap) a.items[f0 + j] = a.stage[R.stage_first + j];
    });
}

template <class Wv>
inline __host__ __device__ void rs_commit(const Wv& wv, RsWaveShared& sh, const RsCommitArgs& a, uint64_t c) {
  const ufc_resend R = a.states[c];
  const ufc_sender& S = a.senders[c];
  const ufc_resend_result B = a.begin_results[c];
  // (scalars, not the record: a record that lambdas capture stays on the stack)
  const uint32_t f_first = a.flush_results[c].frame_first, f_count = a.flush_results[c].frame_count;
  const uint32_t f_packed = a.flush_results[c].items_packed, f_stop = a.flush_results[c].stop;
  const ufc_sender_result SR = a.sender_results[c];
  const uint64_t pf0 = a.packet_first[c], pf1 = a.packet_first[c + 1], if0 = a.flush_first[c], if1 = a.flush_first[c + 1];
  const uint64_t now = a.rate[c].now_ms, rtt = a.rate[c].rtt_ms;
  const uint32_t staged = B.n_resent + B.n_pending_staged;
  const bool frames_ok = (uint64_t)f_first + f_count <= a.n_infos;
  bool ok = rs_state_ok(R, S, a.n_heap, a.n_pkts, a.n_frag, a.n_tx, 0, false) && B.stop != UFC_RS_BAD_STATE && frames_ok &&
            pf0 <= pf1 && pf1 <= a.n_packets && SR.packets_consumed <= pf1 - pf0 && if0 <= if1 && if1 <= a.n_items &&
            staged <= if1 - if0 && f_packed >= B.n_resent && f_packed <= if1 - if0 &&
            B.n_pending_staged <= R.pending_count;
  const uint32_t m = ok ? f_packed - B.n_resent : 0;
  const uint32_t pp = m < B.n_pending_staged ? m : B.n_pending_staged, q = m - pp;
  const uint32_t pending_left = R.pending_count - (ok ? pp : 0);
  if (ok && pending_left && q) ok = false;  // new items packed behind unpacked pending ones
  // retake: the sender as begin left it, with the take the reference's loop got to
  wv.lanes([&](uint32_t lane) { sh.chan_parent[lane] = S.channel_parent_id[lane]; });
  // (the fixed fields; the parents go through sh)
  RsSenderHead T{S.base_id, S.next_id, S.window_size, S.flush_id, S.alloc, S.max_alloc, S.window_parent_id, 0, 0, S.reserved};
  const auto put_sender = [&]() {
    wv.lanes([&](uint32_t lane) { a.retake[c].channel_parent_id[lane] = sh.chan_parent[lane]; });
    wv.one([&]() { rs_put_sender(a.retake[c], T); });
  };
  wv.one([&]() {
    a.sent_first[c] = f_first;
    if (c + 1 == a.n) a.sent_first[a.n] = *a.frames_used;
  });
  const bool limited = f_stop == UFC_PACK_SIZE_LIMITED || B.stop == UFC_RS_SIZE_LIMITED;
  if (!ok) {
    if (frames_ok)
      for (uint32_t t = 0; t < f_count; t += 64)
        wv.lanes([&](uint32_t lane) {
          const uint64_t g = (uint64_t)f_first + t + lane;
          if (t + lane >= f_count || g >= a.sent_cap) return;
          rs_put_sent(a.sent[g], now, (uint32_t)(a.out_offsets[g + 1] - a.out_offsets[g]), 0, 0, a.infos[g].aux);
        });
    put_sender();
    wv.one([&]() {
      ufc_resend_commit_result res{};
      res.stop = UFC_RS_BAD_STATE;
      res.heap_len = R.heap_len;
      res.pending_count = R.pending_count;
      a.results[c] = res;
      rs_put_state(a.states_out[c], R);
      if (a.next_extra_flags)
        a.next_extra_flags[c] = (a.next_extra_flags[c] & ~(uint32_t)UFC_FQ_MARK_RATE_LIMITED) |
                                (limited ? (uint32_t)UFC_FQ_MARK_RATE_LIMITED : 0u);
    });
    return;
  }
  const uint32_t pmask = R.pkt_cap - 1, fmask = R.frag_cap - 1, tmask = R.tx_cap - 1;
  ufc_sent_packet* pk = a.pkts + R.pkt_first;
  uint8_t* fa = a.frag_acked + R.frag_first;
  const uint64_t new0 = if0 + staged, first_unpacked = new0 + q;
  // the stopping packet p and the packets that enter the table
  uint32_t take = 0, entered = 0, frag_next = R.frag_next;
  uint32_t pend_seq = R.pending_seq, pend_next = R.pending_next + pp, pend_count = pending_left;
  uint8_t pend_resend = R.pending_resend;
  uint64_t window_bytes = R.window_bytes;
  if (pending_left == 0) {
    take = SR.packets_consumed;
    uint64_t enter_end = if1;
    if (first_unpacked < if1) {
      for (uint32_t t = 0; t < SR.packets_consumed; t += 64) {
        const unsigned long long hit = wv.ballot([&](uint32_t lane) {
          if (t + lane >= SR.packets_consumed) return false;
          const ufc_packet_result r = a.packet_results[pf0 + t + lane];
          return r.status == UFC_PACKET_EMITTED && (uint64_t)r.item_first + r.item_count > first_unpacked;
        });
        if (hit) {
          const uint32_t p = t + low_bit(hit);
          const ufc_packet_result r = a.packet_results[pf0 + p];
          take = p + 1;
          enter_end = (uint64_t)r.item_first + r.item_count;
          pend_seq = r.sequence_id;
          pend_next = (uint32_t)(first_unpacked - r.item_first);
          pend_count = (uint32_t)(enter_end - first_unpacked);
          pend_resend = r.resend ? 1 : 0;
          break;
        }
      }
    }
    if (pend_count == 0) {
      pend_seq = 0;
      pend_next = 0;
      pend_resend = 0;
    }
    for (uint32_t t = 0; t < take; t += 64) {
      // (status NOT_REACHED = 0 marks a lane with no packet to enter)
      const auto emitted = [&](uint32_t lane) {
        ufc_packet_result r{};
        if (t + lane >= take) return r;
        r = a.packet_results[pf0 + t + lane];
        if (r.status != UFC_PACKET_EMITTED || r.item_first < new0 || (uint64_t)r.item_first + r.item_count > enter_end)
          r.status = UFC_PACKET_NOT_REACHED;
        return r;
      };
      entered += (uint32_t)wv.sum([&](uint32_t lane) -> uint64_t { return emitted(lane).status ? 1 : 0; });
      window_bytes += wv.sum([&](uint32_t lane) -> uint64_t {
        return emitted(lane).status ? a.packets[pf0 + t + lane].data_len : 0;
      });
      wv.lanes([&](uint32_t lane) {
        const ufc_packet_result r = emitted(lane);
        if (!r.status) return;
        const ufc_packet p = a.packets[pf0 + t + lane];
        const ufc_item& it = a.items[r.item_first];  // (read in place: only the leads are used)
        ufc_sent_packet& k = pk[r.sequence_id & pmask];  // (field by field: no record on the stack)
        k.data_offset = p.data_offset;
        k.data_len = p.data_len;
        k.frag_first = R.frag_next + (uint32_t)(r.item_first - new0);
        k.sequence_id = r.sequence_id;
        k.window_parent_lead = it.window_parent_lead;
        k.channel_parent_lead = it.channel_parent_lead;
        k.channel_id = p.channel_id;
        k.resend = r.resend ? 1 : 0;
        k.reserved = 0;
      });
    }
    const uint32_t nfrag = (uint32_t)(enter_end - new0);
    for (uint32_t t = 0; t < nfrag; t += 64)
      wv.lanes([&](uint32_t lane) {
        if (t + lane < nfrag) fa[(R.frag_next + t + lane) & fmask] = 0;
      });
    frag_next = R.frag_next + nfrag;
  } else {
    wv.sync();
  }
  // the pushes, in one lane: the packed pending fragments, then the packed new fragments of resend packets
  wv.one([&]() {
    ufc_resend_entry* d = a.heap + R.heap_first;
    uint32_t len = R.heap_len, pushed = 0, dropped = 0;
    const uint64_t due = now + rtt;
    const uint32_t from_pending = R.pending_resend ? pp : 0;
    for (uint64_t i = 0; i < (uint64_t)from_pending + q; i++) {  // (one loop: one copy of the push)
      uint32_t seq = R.pending_seq, f = R.pending_next + (uint32_t)i;
      if (i >= from_pending) {
        const ufc_item& it = a.items[new0 + (i - from_pending)];
        seq = it.id;
        f = it.fragment_id;
        if (!pk[seq & pmask].resend) continue;
      }
      if (len >= R.heap_cap) {
        dropped++;
        continue;
      }
      rs_heap_push(d, len, rs_entry(due, seq, f, 1));
      pushed++;
    }
    sh.heap_len = len;
    sh.pushed = pushed;
    sh.dropped = dropped;
  });
  wv.sync();
  // the refs and the sent records: the positions are a chain over the frames, every lane walks it
  uint32_t head = R.tx_head, refs_written = 0;
  for (uint32_t kf = 0; kf < f_count; kf++) {
    const uint64_t g = (uint64_t)f_first + kf;
    const uint32_t item_first = a.infos[g].item_first, aux = a.infos[g].aux;
    uint32_t cnt = a.infos[g].item_count;
    if (cnt > UFC_DATA_FRAME_MAX_DATAGRAM_COUNT || (uint64_t)item_first + cnt > a.n_items) cnt = 0;
    if ((head & tmask) + cnt > R.tx_cap) head += R.tx_cap - (head & tmask);
    const uint64_t ref_first = R.tx_first + (head & tmask);
    wv.lanes([&](uint32_t lane) {
      for (uint32_t j = lane; j < cnt; j += 64) {
        const ufc_item& it = a.items[(uint64_t)item_first + j];
        ufc_tx_ref& ref = a.tx[ref_first + j];
        ref.sequence_id = it.id;
        ref.fragment_id = it.fragment_id;
        ref.flags = pk[it.id & pmask].resend ? UFC_TX_RESEND : 0;
      }
    });
    wv.one([&]() {
      if (g >= a.sent_cap) return;
      rs_put_sent(a.sent[g], now, (uint32_t)(a.out_offsets[g + 1] - a.out_offsets[g]), (uint32_t)ref_first, cnt, aux);
    });
    head += cnt;
    refs_written += cnt;
  }
  T.take = take;
  put_sender();
  wv.one([&]() {
    ufc_resend_commit_result res{};
    res.stop = sh.dropped ? UFC_RS_HEAP_FULL : UFC_RS_DONE;
    res.pending_packed = pp;
    res.packets_entered = entered;
    res.heap_pushed = sh.pushed;
    res.heap_dropped = sh.dropped;
    res.refs_written = refs_written;
    res.frames = f_count;
    res.take = take;
    res.heap_len = sh.heap_len;
    res.pending_count = pend_count;
    a.results[c] = res;
    ufc_resend& O = a.states_out[c];
    rs_put_state(O, R);
    O.heap_len = sh.heap_len;
    O.frag_next = frag_next;
    O.tx_head = head;
    O.pending_seq = pend_seq;
    O.pending_next = pend_next;
    O.pending_count = pend_count;
    O.pending_resend = pend_resend;
    O.window_bytes = window_bytes;
    if (a.next_extra_flags)
      a.next_extra_flags[c] = (a.next_extra_flags[c] & ~(uint32_t)UFC_FQ_MARK_RATE_LIMITED) |
                              (limited ? (uint32_t)UFC_FQ_MARK_RATE_LIMITED : 0u);
  });
}

// ---- batched flush control (ufc_flush_acks_*, ufc_flush_sync_*) ----
// The glue of HalfConnection::flush around the data flush: emit_ack_frames (half_connection/mod.rs:296-333 over
// AckFrameEmitter, emit.rs:137-211, push_dud :149-166) with the deque carry of FrameAckQueue, and emit_sync_frame
// (mod.rs:234-294) with the early returns of emit_frames (:217-232); the rules are in include/uflow_flush_ctl.h.
// The ack flush is counted by a lane per connection (fa_plan: a loop over frames), and after the exclusive sums of
// the group and frame counts written by a wave per connection with a lane per group (fa_write).  The sync decision
// takes a lane per connection in tiles of 64 (fs_decide_tile), and after a scan over the tiles' ballot counts the
// same tiles write the frames' records in connection order (fs_write_tile).
struct FaArgs {
  const ufc_flush_ctl* ctl;
  const ufc_frame_window* windows;
  const ufc_item* groups;
  uint64_t n_groups;
  const uint64_t* group_first;
  const ufc_receiver* receivers;
  const ufc_rate_result* rate;
  uint64_t n;
  ufc_item* carry;
  uint64_t n_carry;
  ufc_item* merged;
  uint64_t merged_cap;
  uint64_t* merged_first;
  uint64_t* merged_used;
  ufc_frame_info* infos;
  uint64_t frames_cap;
  uint64_t* frames_used;
  ufc_flush_result* results;
  ufc_flush_acks_result* ack_results;
  ufc_frame_window* windows_out;
  ufc_flush_ctl* ctl_out;
  ufc_flush* flushes;
  uint32_t* flags;
};
// (The n + 1 group and frame counts are scanned with a 32-bit count; n_groups + n_carry < 2^32 keeps every merged
// count and every index into `merged` inside 32 bits.)
inline bool fa_args_ok(const FaArgs& a) {
  const bool bad = !a.ctl || !a.windows || !a.group_first || !a.receivers || !a.rate || !a.merged_first ||
                   !a.merged_used || !a.frames_used || !a.results || !a.ack_results || !a.windows_out || !a.ctl_out ||
                   (!a.groups && a.n_groups) || (!a.carry && a.n_carry) || (!a.merged && a.merged_cap) ||
                   (!a.infos && a.frames_cap) || a.n >= kCountLim || a.n_groups >= kCountLim || a.n_carry >= kCountLim;
  return !bad;
}

// What one connection's ack flush comes to: the merged list's length, and the emitter's run over it.
struct FaPlan {
  bool ok;           // false: BAD_STATE
  bool dud;          // push_dud opened the first frame
  uint32_t skip;     // carry groups in front of the window's (carry_count - 1, or 0)
  uint64_t g0;       // the window's first group
  uint32_t merged;   // groups in the merged list
  uint32_t frames, packed, stop;
  int64_t alloc_left;
};
// AckFrameEmitter over n groups of 9 bytes, frame by frame (emit.rs:170-211; steps 1, 2 and 4 of the ufc_flush
// comment with H = 15, e = 9, no count limit), behind an optional push_dud.  While a frame is in progress alloc
// stands still and its size grows by 9 a group, so the groups it takes are the least of what is left, what fits the
// frame, and the pushes that pass `alloc - size >= 0`.
UFC_HD void fa_pack(FaPlan& p, int64_t alloc, bool sync_reply, uint64_t n) {
  uint64_t s = 0, i = 0;
  p.frames = 0;
  p.stop = UFC_PACK_DONE;
  p.dud = false;
  if (sync_reply) {  // push_dud, emit.rs:149-166
    if (alloc < 0) {
      p.packed = 0;
      p.stop = UFC_PACK_SIZE_LIMITED;
      p.alloc_left = alloc;
      return;
    }
    p.dud = true;
    s = kAckFrameOverhead;
  }
  while (i < n) {
    if (s == 0) {  // :190-202
      if (alloc < 0) {
        p.stop = UFC_PACK_SIZE_LIMITED;
        break;
      }
      s = kAckFrameOverhead + UFC_ACK_GROUP_SIZE;
      i++;
    }
    const uint64_t k_size = (kMaxFrameSize - s) / UFC_ACK_GROUP_SIZE;
    const uint64_t k_alloc = alloc >= (int64_t)s ? (uint64_t)(alloc - (int64_t)s) / UFC_ACK_GROUP_SIZE + 1 : 0;
    uint64_t k = n - i;
    if (k > k_size) k = k_size;
    if (k > k_alloc) k = k_alloc;
    i += k;
    s += k * UFC_ACK_GROUP_SIZE;
    if (i == n) break;
    // the push of group i does not go into this frame: finalize (:176-182)
    p.frames++;
    alloc = (int64_t)((uint64_t)alloc - s);
    s = 0;
    if (k == k_alloc) {  // it was the allocation that refused it
      p.stop = UFC_PACK_SIZE_LIMITED;
      break;
    }
  }
  if (s) {  // finalize (:205-211)
    p.frames++;
    alloc = (int64_t)((uint64_t)alloc - s);
  }
  p.packed = (uint32_t)i;
  p.alloc_left = alloc;
}
UFC_HD FaPlan fa_plan(const FaArgs& a, uint64_t c) {
  const ufc_flush_ctl& C = a.ctl[c];
  const uint64_t g0 = a.group_first[c], g1 = a.group_first[c + 1];
  const uint32_t cc = C.carry_count;
  FaPlan p{};
  p.g0 = g0;
  p.alloc_left = a.rate[c].flush_alloc;
  p.stop = UFC_PACK_BAD_RANGE;
  p.ok = g0 <= g1 && g1 <= a.n_groups && cc <= C.carry_cap && rs_region_ok(C.carry_first, C.carry_cap, a.n_carry);
  // The window writes the carried tail first, as updated: the carry's own copy of it is dropped.
  if (p.ok && cc) p.ok = g1 > g0 && a.groups[g0].id == a.carry[C.carry_first + cc - 1].id;
  if (!p.ok) return p;
  p.skip = cc ? cc - 1 : 0;
  p.merged = p.skip + (uint32_t)(g1 - g0);
  fa_pack(p, a.rate[c].flush_alloc, a.windows[c].sync_reply != 0, p.merged);
  return p;
}

struct FaWaveShared {
  ufc_item tile[64];
};
// Frame k of a flush holds the groups [k * kAckFrameMaxGroups ..) of its merged list: every frame but the last is
// full, with or without a dud in front (a dud frame that takes no group is the flush's only one).
template <class Wv>
inline __host__ __device__ void fa_write(const Wv& wv, FaWaveShared& sh, const FaArgs& a, uint64_t c, uint64_t ffirst) {
  // (read in place: the outputs, which may be the inputs, are written last, behind every read)
  const ufc_flush_ctl C = a.ctl[c];
  const ufc_frame_window W = a.windows[c];
  const FaPlan p = fa_plan(a, c);
  const uint64_t mfirst = a.merged_first[c];
  const uint32_t id0 = W.base_id, id1 = a.receivers[c].base_id;
  const uint32_t left = p.merged - p.packed;                    // the groups no frame took
  const uint32_t kept = left < C.carry_cap ? left : C.carry_cap;  // the newest of them stay
  const uint32_t from = p.merged - kept;
  for (uint64_t t = 0; t < p.merged; t += 64) {
    wv.lanes([&](uint32_t lane) {
      const uint64_t j = t + lane;
      if (j < p.merged) sh.tile[lane] = j < p.skip ? a.carry[C.carry_first + j] : a.groups[p.g0 + (j - p.skip)];
    });
    wv.lanes([&](uint32_t lane) {
      const uint64_t j = t + lane;
      if (j >= p.merged) return;
      if (mfirst + j < a.merged_cap) a.merged[mfirst + j] = sh.tile[lane];
      if (j >= from) a.carry[C.carry_first + (j - from)] = sh.tile[lane];  // (j - from <= j: no later tile reads it)
    });
  }
  for (uint64_t t = 0; t < p.frames; t += 64)
    wv.lanes([&](uint32_t lane) {
      const uint64_t k = t + lane;
      if (k >= p.frames || ffirst + k >= a.frames_cap) return;
      const uint64_t first = k * kAckFrameMaxGroups;
      const uint64_t cnt = p.packed > first ? p.packed - first : 0;
      ufc_frame_info info{};
      info.kind = UFC_FRAME_ACK;
      info.ok = 1;
      info.f[0] = id0;
      info.f[1] = id1;
      info.item_count = cnt < kAckFrameMaxGroups ? (uint32_t)cnt : kAckFrameMaxGroups;
      info.item_first = (uint32_t)(mfirst + first);
      a.infos[ffirst + k] = info;
    });
  wv.one([&] {
    ufc_flush_result res{};
    res.frame_first = (uint32_t)ffirst;
    res.frame_count = p.frames;
    res.items_packed = p.packed;
    res.stop = p.stop;
    res.alloc_left = p.alloc_left;
    a.results[c] = res;
    ufc_flush_acks_result ar{};
    ar.stop = !p.ok ? UFC_FA_BAD_STATE : left > kept ? UFC_FA_CARRY_FULL : UFC_FA_DONE;
    ar.merged_first = (uint32_t)mfirst;
    ar.merged_count = p.merged;
    ar.carried = p.ok ? kept : 0;
    ar.dropped = left - kept;
    ar.dud = p.dud ? 1 : 0;
    a.ack_results[c] = ar;
    ufc_frame_window O = W;
    ufc_flush_ctl K = C;
    if (p.ok) {
      if (p.frames) O.sync_reply = 0;           // emit_cb, mod.rs:306-310
      if (p.packed == p.merged) O.has_tail = 0;  // the deque is empty
      K.carry_count = kept;
    }
    a.windows_out[c] = O;
    a.ctl_out[c] = K;
    if (a.flushes) a.flushes[c].flush_alloc = p.alloc_left;
    if (a.flags)
      a.flags[c] = (a.flags[c] & ~(uint32_t)UFC_RS_NO_DATA_FLUSH) |
                   (p.stop == UFC_PACK_SIZE_LIMITED ? (uint32_t)UFC_RS_NO_DATA_FLUSH : 0u);
  });
}

struct FsArgs {
  const ufc_flush_ctl* ctl;
  const ufc_rate_result* rate;
  const ufc_flush_result* ack_results;
  const ufc_resend_result* begin_results;
  const ufc_flush_result* pack_results;
  const ufc_resend_commit_result* commit_results;
  const ufc_frame_queue* queues;
  const ufc_sender* senders;
  uint64_t n;
  ufc_frame_info* infos;
  uint64_t syncs_cap;
  uint32_t* sync_index;
  uint64_t* syncs_used;
  ufc_flush_sync_result* results;
  ufc_flush_ctl* ctl_out;
  ufc_rate_tick* ticks_next;
};
inline bool fs_args_ok(const FsArgs& a) {
  const bool bad = !a.ctl || !a.rate || !a.ack_results || !a.begin_results || !a.pack_results || !a.commit_results ||
                   !a.queues || !a.senders || !a.sync_index || !a.syncs_used || !a.results || !a.ctl_out ||
                   (!a.infos && a.syncs_cap) || a.n >= kCountLim;
  return !bad;
}
constexpr uint64_t kMinSyncTimeoutMs = 2000;  // MIN_SYNC_TIMEOUT_MS
constexpr int64_t kSyncFrameSize = 14;        // write_sync: id, mode, two ids, trailer

// The ids a sync frame of connection c would carry: bit 0 / f0 next_frame_id (mod.rs:244-249), bit 1 / f1
// next_packet_id (:257-263).
UFC_HD uint32_t fs_ids(const FsArgs& a, uint64_t c, uint32_t& f0, uint32_t& f1) {
  const ufc_frame_queue& Q = a.queues[c];
  const ufc_sender& S = a.senders[c];
  const ufc_resend_commit_result& M = a.commit_results[c];
  const uint32_t next_frame = Q.log_next_id + a.pack_results[c].frame_count;
  uint32_t mode = 0;
  f0 = f1 = 0;
  if (next_frame != Q.window_base_id) {
    mode |= 1;
    f0 = next_frame;
  }
  if (S.next_id != S.base_id && M.heap_len == 0 && M.pending_count == 0) {
    mode |= 2;
    f1 = S.next_id;
  }
  return mode;
}
// emit_frames behind emit_ack_frames for one connection (rules 1-10 of the header); returns whether a frame goes out.
UFC_HD bool fs_decide(const FsArgs& a, uint64_t c) {
  ufc_flush_ctl C = a.ctl[c];
  const ufc_rate_result& R = a.rate[c];
  const ufc_flush_result& P = a.pack_results[c];
  const ufc_resend_commit_result& M = a.commit_results[c];
  const uint32_t bstop = a.begin_results[c].stop;
  ufc_flush_sync_result res{};
  res.heap_len = M.heap_len;
  res.pending_count = M.pending_count;
  res.is_send_pending = (M.heap_len != 0 || M.pending_count != 0) ? 1 : 0;
  uint32_t reason;
  if (a.ack_results[c].stop == UFC_PACK_SIZE_LIMITED) {
    reason = UFC_FS_ACK_LIMITED;  // mod.rs:218-221
  } else {
    if (P.frame_count) C.sync_timeout_base_ms = R.now_ms;  // emit_cb of emit_data_frames, :342-347
    const uint64_t elapsed = R.now_ms - C.sync_timeout_base_ms;
    uint32_t f0, f1;
    if (bstop == UFC_RS_SIZE_LIMITED || P.stop == UFC_PACK_SIZE_LIMITED) {
      reason = UFC_FS_DATA_LIMITED;  // :223-226
    } else if (bstop == UFC_RS_REF_HANG || bstop == UFC_RS_BAD_STATE || M.stop == UFC_RS_REF_HANG ||
               M.stop == UFC_RS_BAD_STATE || M.stop == UFC_RS_HEAP_FULL) {
      reason = UFC_FS_UPSTREAM;
    } else if (elapsed < (R.rto_ms > kMinSyncTimeoutMs ? R.rto_ms : kMinSyncTimeoutMs)) {
      reason = UFC_FS_NOT_DUE;  // :235-238
    } else if ((res.mode = (uint8_t)fs_ids(a, c, f0, f1)) == 0 &&
               (!C.has_keepalive || elapsed < C.keepalive_interval_ms)) {
      reason = UFC_FS_IDLE;  // :269-277
    } else if (P.alloc_left < 0) {
      reason = UFC_FS_NO_ALLOC;  // :279-281
    } else {
      reason = UFC_FS_SENT;
      C.sync_timeout_base_ms = R.now_ms;  // :290
    }
  }
  C.has_keepalive = C.has_keepalive ? 1 : 0;
  if (!C.has_keepalive) C.keepalive_interval_ms = 0;
  res.reason = reason;
  res.sent = reason == UFC_FS_SENT ? 1 : 0;
  if (!res.sent) res.mode = 0;
  a.results[c] = res;
  a.ctl_out[c] = C;
  if (a.ticks_next) a.ticks_next[c].alloc_adjust = res.sent ? -kSyncFrameSize : 0;
  return res.sent != 0;
}
// Connections [64 tile, 64 tile + 64): the decisions, a lane each; returns how many send a frame.
template <class Wv>
inline __host__ __device__ uint32_t fs_decide_tile(const Wv& wv, const FsArgs& a, uint64_t tile) {
  return popc(wv.ballot([&](uint32_t lane) {
    const uint64_t c = tile * 64 + lane;
    return c < a.n && fs_decide(a, c);
  }));
}
// The same tile behind the scan: `first` frames went out in the tiles before it.  The ballot over results[].sent is
// the stage's one cross-lane read: a sending lane's frame index is `first` + the sending lanes below it.
template <class Wv>
inline __host__ __device__ void fs_write_tile(const Wv& wv, const FsArgs& a, uint64_t tile, uint64_t first) {
  const unsigned long long m = wv.ballot([&](uint32_t lane) {
    const uint64_t c = tile * 64 + lane;
    return c < a.n && a.results[c].sent != 0;
  });
  wv.lanes([&](uint32_t lane) {
    const uint64_t c = tile * 64 + lane;
    if (c >= a.n) return;
    if (!((m >> lane) & 1)) {
      a.sync_index[c] = UFC_NO_PARENT;
      return;
    }
    const uint64_t at = first + popc(m & ((1ull << lane) - 1));
    a.sync_index[c] = (uint32_t)at;
    if (at >= a.syncs_cap) return;
    ufc_frame_info info{};
    info.kind = UFC_FRAME_SYNC;
    info.ok = 1;
    info.aux = (uint8_t)fs_ids(a, c, info.f[0], info.f[1]);
    a.infos[at] = info;
  });
}

// ---- batched frame routing (ufc_route_table_build_host, ufc_route_frames_*) ----
// The address lookup and dispatch of Server::handle_frames (server/mod.rs:591-602 over :492-589; client/mod.rs:
// 557-583) for the frames of State::Active clients; the rules are in include/uflow_route.h.  What a lane does for a
// frame is written here once: the hash (rt_hash), the bounded probe (rt_lookup), the frame's kind class
// (rt_kind_class) and, once every first control frame is known, its class and bucket (rt_classify, rt_bucket).  The
// grouping itself is a stable sort of the frames by bucket number, which has one answer: the host counts and places
// in arrival order (frame_codec.cpp), the device runs a radix placement (route.hip).
struct RtArgs {
  const ufc_frame_info* infos;
  const ufc_addr* addrs;
  const uint64_t* offsets;
  uint64_t n;
  const ufc_route_slot* slots;
  uint64_t n_slots;
  uint32_t seed, max_probe;
  uint64_t n_conns;
  const uint8_t* conn_active;
  uint64_t now_ms, active_timeout_ms;
  const uint64_t* timeout_in;
  uint32_t* route;
  uint8_t* cls;
  uint64_t* bucket_first;
  uint32_t* order;
  ufc_frame_info* infos_out;
  uint64_t* src_base_out;
  ufc_route_result* results;
  uint64_t* timeout_out;
  uint32_t* first_unknown_control;
};
constexpr uint64_t kRouteConnLim = kCountLim - 2;  // n_conns + 2 bucket numbers and UFC_NO_PARENT stay apart in 32 bits
// n_slots: a power of two above n_conns, and no more than 2^31 (the probe index is 32-bit).
inline bool rt_table_ok(uint64_t n_slots, uint64_t n_conns) {
  return n_conns < kRouteConnLim && n_slots > n_conns && (n_slots & (n_slots - 1)) == 0 &&
         n_slots <= ((uint64_t)1 << 31);
}
inline bool rt_args_ok(const RtArgs& a) {
  const bool bad = !a.slots || !a.bucket_first || !a.first_unknown_control || !rt_table_ok(a.n_slots, a.n_conns) ||
                   a.n >= kCountLim ||
                   (a.n && (!a.infos || !a.addrs || !a.route || !a.cls || !a.order || !a.infos_out || !a.src_base_out ||
                            a.infos_out == a.infos || a.src_base_out == a.offsets)) ||
                   (a.n_conns && (!a.conn_active || !a.timeout_in || !a.results || !a.timeout_out));
  return !bad;
}

// The key's eight little-endian words (the host and the GPU are little-endian; a key is 4-byte aligned).
struct RtKey {
  uint32_t w[8];
};
UFC_HD RtKey rt_key(const ufc_addr& a) {
  RtKey k;
  __builtin_memcpy(k.w, &a, 32);
  return k;
}
UFC_HD uint32_t rt_hash(uint32_t seed, const uint32_t* w) {
  uint32_t h = seed;
  for (int k = 0; k < 8; k++) {
    h = (h ^ w[k]) * 0x9E3779B1u;
    h ^= h >> 15;
  }
  h *= 0x85EBCA77u;
  h ^= h >> 13;
  return h;
}
UFC_HD bool rt_key_eq(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
  for (int k = 0; k < 8; k++) d |= a[k] ^ b[k];
  return d == 0;
}
// e(i): the connection of a key, or UFC_NO_PARENT.  At most min(max_probe, n_slots - 1) + 1 slots are read, all of
// them inside the table.
UFC_HD uint32_t rt_lookup(const ufc_route_slot* slots, uint64_t n_slots, uint32_t seed, uint32_t max_probe,
                          uint64_t n_conns, const ufc_addr& key) {
  const RtKey kw = rt_key(key);
  const uint32_t mask = (uint32_t)(n_slots - 1);
  const uint32_t home = rt_hash(seed, kw.w) & mask;
  const uint32_t last = max_probe < mask ? max_probe : mask;
  for (uint32_t p = 0;; p++) {
    const ufc_route_slot& s = slots[(home + p) & mask];
    if (!s.used) return UFC_NO_PARENT;
    if (s.conn < n_conns && rt_key_eq(rt_key(s.key).w, kw.w)) return s.conn;
    if (p == last) return UFC_NO_PARENT;
  }
}
// 1: control (handshake and disconnect frames), 2: session (data, sync, ack), 0: Frame::read gave None.
UFC_HD uint32_t rt_kind_class(const ufc_frame_info& f) {
  if (!f.ok) return 0;
  if (f.kind <= UFC_FRAME_DISCONNECT_ACK) return 1;
  return (f.kind == UFC_FRAME_DATA || f.kind == UFC_FRAME_SYNC || f.kind == UFC_FRAME_ACK) ? 2 : 0;
}
// Frame i's class, once route[] and every first control frame (results[].first_control, *first_unknown_control)
// are final.  k: rt_kind_class of the frame.
UFC_HD uint32_t rt_classify(const RtArgs& a, uint64_t i, uint32_t k) {
  if (k == 1) return UFC_ROUTE_CONTROL;
  if (k == 0) return UFC_ROUTE_DROP;
  const uint32_t c = a.route[i];
  if (c == UFC_NO_PARENT) return i > *a.first_unknown_control ? UFC_ROUTE_DEFERRED : UFC_ROUTE_DROP;
  if (i > a.results[c].first_control) return UFC_ROUTE_DEFERRED;  // (UFC_NO_PARENT is above every index)
  return a.conn_active[c] ? UFC_ROUTE_CONN : UFC_ROUTE_DROP;
}
UFC_HD uint32_t rt_bucket(const RtArgs& a, uint64_t i, uint32_t cls) {
  if (cls == UFC_ROUTE_CONN) return a.route[i];
  return (uint32_t)a.n_conns + (cls == UFC_ROUTE_DROP ? 1u : 0u);
}
// Grouped position k takes frame order[k]'s record and source offset.
UFC_HD uint64_t rt_src_base(const RtArgs& a, uint32_t i) { return a.offsets ? a.offsets[i] : 0; }
// Connection c behind the placement: its bucket's length, and the timeout refresh of handle_data / handle_sync /
// handle_ack (server/mod.rs:507, :529, :551).  timeout_out may be timeout_in: entry c is read before it is written.
UFC_HD void rt_finish_conn(const RtArgs& a, uint64_t c) {
  const uint32_t frames = (uint32_t)(a.bucket_first[c + 1] - a.bucket_first[c]);
  a.results[c].frames = frames;
  a.results[c].reserved = 0;
  const uint64_t t = a.timeout_in[c];
  a.timeout_out[c] = frames ? a.now_ms + a.active_timeout_ms : t;
}

}  // namespace ufc_codec
