// frame_codec.cpp -- host side of uflow's frame codec (include/uflow_frame_codec.h): Frame::read,
// the fixed-size writers, DataFrameBuilder / AckFrameBuilder, and the batched host parse that
// follows the batched CRC gate.  The payload parse is frame_codec_core.hpp (shared with the GPU).
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/uflow_frame_codec.h"
#include "crc_math.hpp"
#include "frame_codec_core.hpp"

namespace {

struct HostBytes {
  const uint8_t* p;
  uint32_t operator()(uint32_t i) const { return p[i]; }
  uint32_t head3(uint32_t i) const { return p[i] | (p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16); }
};

inline void put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

inline bool crc_gate(const uint8_t* f, size_t len) {  // serial/mod.rs:676-690
  if (len < 5) return false;
  const uint32_t rx = ((uint32_t)f[len - 4] << 24) | ((uint32_t)f[len - 3] << 16) | ((uint32_t)f[len - 2] << 8) |
                      (uint32_t)f[len - 1];
  return ufc::host_extend(0u, f, len - 4) == rx;
}

// Trailer: BE32 CRC of everything before it (serial/mod.rs:463-470, build.rs:151-159), or zeros
// for a later batched seal.
inline void trailer(uint8_t* f, size_t body, int seal) {
  put32(f + body, seal ? ufc::host_extend(0u, f, body) : 0u);
}

constexpr uint32_t kPacketIdMask = (1u << 20) - 1;  // src/packet_id.rs

// ---- batched host build (the encode of frame_codec_core.hpp, shared with frame_build.hip) ----
// body(a, b) over contiguous ranges of [0, n) on up to nthreads threads, and no more threads than n / grain
// rounded up: kRecordGrain where an element is a record's worth of work (a frame, a flush, a sender, a copy
// segment), kStepGrain where it is a connection's whole step, which is work enough for a thread.
constexpr size_t kRecordGrain = 1024, kStepGrain = 1;
template <class F>
void for_ranges(size_t n, int nthreads, size_t grain, const F& body) {
  size_t T = nthreads > 0 ? (size_t)nthreads : 1;
  T = std::max<size_t>(1, std::min(T, (n + grain - 1) / grain));
  std::vector<std::thread> th;
  for (size_t t = 1; t < T; t++) th.emplace_back([&, t] { body(n * t / T, n * (t + 1) / T); });
  body(0, n / T);
  for (auto& x : th) x.join();
}
// first[1 .. n] hold n counts: first[0 .. n] become their exclusive sum, first[n] the total, which is returned.
inline uint64_t counts_to_firsts(uint64_t* first, size_t n) {
  uint64_t total = 0;
  for (size_t r = 0; r < n; r++) {
    const uint64_t c = first[r + 1];
    first[r] = total;
    total += c;
  }
  return first[n] = total;
}
inline void put_packed(uint8_t* out, uint64_t w0, uint64_t w1, uint64_t w2, uint32_t nbytes) {
  for (uint32_t j = 0; j < nbytes; j++) out[j] = (uint8_t)ufc_codec::packed_byte(w0, w1, w2, j);
}
}  // namespace

extern "C" {

int ufc_frame_read(const uint8_t* frame, size_t len, ufc_frame_info* info, ufc_item* items, size_t items_cap) {
  if (!info || (!frame && len)) return UFC_ERR_INVALID_ARG;
  if (len > 0xFFFFFFFFu) len = 0xFFFFFFFFu;
  const bool gate = frame && crc_gate(frame, len);
  const bool ok = ufc_codec::read_frame(HostBytes{frame}, (uint32_t)len, gate, *info, items,
                                        (uint32_t)std::min<size_t>(items_cap, 0xFFFFFFFFu));
  info->item_first = 0;
  if (ok && info->item_count > items_cap && items) return UFC_ERR_NOMEM;
  return ok ? 1 : 0;
}

int ufc_frame_parse(const uint8_t* frame, size_t len, int crc_ok, ufc_frame_info* info, ufc_item* items,
                    size_t items_cap) {
  if (!info || (!frame && len)) return UFC_ERR_INVALID_ARG;
  if (len > 0xFFFFFFFFu) len = 0xFFFFFFFFu;
  const bool ok = ufc_codec::read_frame(HostBytes{frame}, (uint32_t)len, crc_ok != 0 && frame, *info, items,
                                        (uint32_t)std::min<size_t>(items_cap, 0xFFFFFFFFu));
  info->item_first = 0;
  if (ok && info->item_count > items_cap && items) return UFC_ERR_NOMEM;
  return ok ? 1 : 0;
}

int ufc_datagram_is_valid(const ufc_item* datagram) {  // packet_receiver/mod.rs:12-30
  if (!datagram) return UFC_ERR_INVALID_ARG;
  return ufc_codec::datagram_is_valid(*datagram) ? 1 : 0;
}

size_t ufc_frame_write_fixed(const ufc_frame_info* info, uint8_t* out, size_t cap, int seal) {
  if (!info || !out) return 0;
  size_t len;
  switch (info->kind) {
    case UFC_FRAME_HANDSHAKE_SYN: len = ufc_codec::kMaxFrameSize; break;  // :437-473, zero-padded
    case UFC_FRAME_HANDSHAKE_SYN_ACK: len = 25; break;                   // :475-514
    case UFC_FRAME_HANDSHAKE_ACK: len = 9; break;                        // :516-539
    case UFC_FRAME_HANDSHAKE_ERROR: len = 10; break;                     // :541-569
    case UFC_FRAME_DISCONNECT:                                           // :571-590
    case UFC_FRAME_DISCONNECT_ACK: len = 5; break;                       // :592-611
    case UFC_FRAME_SYNC: len = 14; break;                                // :623-657
    default: return 0;
  }
  if (cap < len) return 0;
  std::memset(out, 0, len);
  out[0] = info->kind;
  switch (info->kind) {
    case UFC_FRAME_HANDSHAKE_SYN:
      out[1] = info->aux;
      for (int i = 0; i < 4; i++) put32(out + 2 + 4 * i, info->f[i]);
      break;
    case UFC_FRAME_HANDSHAKE_SYN_ACK:
      for (int i = 0; i < 5; i++) put32(out + 1 + 4 * i, info->f[i]);
      break;
    case UFC_FRAME_HANDSHAKE_ACK:
      put32(out + 1, info->f[0]);
      break;
    case UFC_FRAME_HANDSHAKE_ERROR:
      if (info->aux > 2) return 0;  // HandshakeErrorType has three values (:551-555)
      put32(out + 1, info->f[0]);
      out[5] = info->aux;
      break;
    case UFC_FRAME_SYNC: {
      const uint8_t mode = info->aux & 3u;
      out[1] = mode;
      put32(out + 2, (mode & 1u) ? info->f[0] : 0u);
      put32(out + 6, (mode & 2u) ? info->f[1] : 0u);
      break;
    }
    default:
      break;
  }
  trailer(out, len - 4, seal);
  return len;
}

// ---- DataFrameBuilder (build.rs:47-181) ----
int ufc_data_frame_builder_init(ufc_builder* b, uint8_t* buf, size_t cap, uint32_t sequence_id, int nonce) {
  if (!b || !buf || cap < 6 + 4) return UFC_ERR_INVALID_ARG;
  b->buf = buf;
  b->cap = cap;
  buf[0] = UFC_FRAME_DATA;  // :56-66
  put32(buf + 1, sequence_id);
  buf[5] = (uint8_t)((nonce ? 1 : 0) << 7);
  b->len = 6;
  b->count = 0;
  b->kind = UFC_FRAME_DATA;
  return UFC_OK;
}

size_t ufc_data_frame_encoded_size(const ufc_datagram_ref* d) {  // :173-181
  if (!d) return 0;
  if (d->fragment_id_last == 0) {
    if (d->data_len < 64 && d->window_parent_lead < 128 && d->channel_parent_lead < 256) return 6 + d->data_len;
    if (d->data_len < 256) return 9 + d->data_len;
  }
  return 14 + d->data_len;
}

int ufc_data_frame_builder_add(ufc_builder* b, const ufc_datagram_ref* d) {
  if (!b || !d || b->kind != UFC_FRAME_DATA) return UFC_ERR_INVALID_ARG;
  // build.rs:74-77 (debug_assert!): channel, 20-bit sequence id, u16 length, count limit
  if (d->channel_id >= UFC_MAX_CHANNELS || d->sequence_id > kPacketIdMask || d->data_len > 0xFFFF ||
      b->count >= UFC_DATA_FRAME_MAX_DATAGRAM_COUNT || (d->data_len && !d->data))
    return UFC_ERR_INVALID_ARG;
  if (d->fragment_id_last == 0 && d->fragment_id != 0) return UFC_ERR_INVALID_ARG;  // :82
  const size_t need = ufc_data_frame_encoded_size(d);
  if (b->len + need + 4 > b->cap) return UFC_ERR_INVALID_ARG;
  uint8_t* h = b->buf + b->len;
  const uint32_t dl = (uint32_t)d->data_len, ch = d->channel_id, seq = d->sequence_id;
  const size_t hs = need - d->data_len;  // header form chosen as in :80-121
  if (hs == 6) {  // micro, :84-100
    h[0] = (uint8_t)(dl | ((ch & 0x10) << 2));
    h[1] = (uint8_t)(((seq >> 12) & 0xF0) | (ch & 0x0F));
    h[2] = (uint8_t)(seq >> 8);
    h[3] = (uint8_t)seq;
    h[4] = (uint8_t)(d->window_parent_lead | ((ch & 0x20) << 2));
    h[5] = (uint8_t)d->channel_parent_lead;
  } else if (hs == 9) {  // small, :101-119
    h[0] = (uint8_t)(ch | 0x80);
    h[1] = (uint8_t)dl;
    h[2] = (uint8_t)(seq >> 16);
    h[3] = (uint8_t)(seq >> 8);
    h[4] = (uint8_t)seq;
    h[5] = (uint8_t)(d->window_parent_lead >> 8);
    h[6] = (uint8_t)d->window_parent_lead;
    h[7] = (uint8_t)(d->channel_parent_lead >> 8);
    h[8] = (uint8_t)d->channel_parent_lead;
  } else {  // large, :123-143
    h[0] = (uint8_t)(ch | 0xC0);
    h[1] = (uint8_t)(dl >> 8);
    h[2] = (uint8_t)dl;
    h[3] = (uint8_t)(seq >> 16);
    h[4] = (uint8_t)(seq >> 8);
    h[5] = (uint8_t)seq;
    h[6] = (uint8_t)(d->window_parent_lead >> 8);
    h[7] = (uint8_t)d->window_parent_lead;
    h[8] = (uint8_t)(d->channel_parent_lead >> 8);
    h[9] = (uint8_t)d->channel_parent_lead;
    h[10] = (uint8_t)(d->fragment_id >> 8);
    h[11] = (uint8_t)d->fragment_id;
    h[12] = (uint8_t)(d->fragment_id_last >> 8);
    h[13] = (uint8_t)d->fragment_id_last;
  }
  if (dl) std::memcpy(h + hs, d->data, dl);
  b->len += hs + dl;
  b->count++;
  return UFC_OK;
}

// ---- AckFrameBuilder (build.rs:183-256) ----
int ufc_ack_frame_builder_init(ufc_builder* b, uint8_t* buf, size_t cap, uint32_t frame_window_base_id,
                               uint32_t packet_window_base_id) {
  if (!b || !buf || cap < 11 + 4) return UFC_ERR_INVALID_ARG;
  b->buf = buf;
  b->cap = cap;
  buf[0] = UFC_FRAME_ACK;  // :189-205
  put32(buf + 1, frame_window_base_id);
  put32(buf + 5, packet_window_base_id);
  buf[9] = buf[10] = 0;
  b->len = 11;
  b->count = 0;
  b->kind = UFC_FRAME_ACK;
  return UFC_OK;
}

int ufc_ack_frame_builder_add(ufc_builder* b, uint32_t base_id, uint32_t bitfield, int nonce) {
  if (!b || b->kind != UFC_FRAME_ACK || b->count >= 0xFFFF || b->len + 9 + 4 > b->cap) return UFC_ERR_INVALID_ARG;
  uint8_t* h = b->buf + b->len;  // :213-228
  put32(h, base_id);
  put32(h + 4, bitfield);
  h[8] = (uint8_t)(nonce ? 1 : 0);
  b->len += 9;
  b->count++;
  return UFC_OK;
}

size_t ufc_builder_size(const ufc_builder* b) { return b ? b->len + 4 : 0; }

size_t ufc_builder_build(ufc_builder* b, int seal) {
  if (!b || !b->buf || b->len + 4 > b->cap) return 0;
  if (b->kind == UFC_FRAME_DATA) {
    b->buf[5] |= (uint8_t)b->count;  // :148-149
  } else if (b->kind == UFC_FRAME_ACK) {
    b->buf[9] = (uint8_t)(b->count >> 8);  // :231-234
    b->buf[10] = (uint8_t)b->count;
  } else {
    return 0;
  }
  trailer(b->buf, b->len, seal);
  return b->len + 4;
}

// ---- batched host parse ----
int ufc_parse_batch_host(const uint8_t* bytes, const uint64_t* offsets, size_t n, const uint8_t* valid,
                         ufc_frame_info* infos, ufc_item* items, size_t items_cap, size_t* items_used,
                         int nthreads) {
  if (items_used) *items_used = 0;
  if (n == 0) return UFC_OK;
  if (!bytes || !offsets || !infos) return UFC_ERR_INVALID_ARG;
  for (size_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0xFFFFFFFFull) return UFC_ERR_INVALID_ARG;
  int T = nthreads > 0 ? nthreads : 1;
  T = (int)std::min<size_t>((size_t)T, (n + 1023) / 1024);
  if (T < 1) T = 1;
  // Pass 1 (parallel over contiguous frame ranges): gate + parse into infos, count items.
  std::vector<uint64_t> part(T + 1, 0);
  auto pass1 = [&](int t) {
    const size_t a = n * t / T, b = n * (t + 1) / T;
    uint64_t c = 0;
    for (size_t i = a; i < b; i++) {
      const uint8_t* f = bytes + offsets[i];
      const size_t len = (size_t)(offsets[i + 1] - offsets[i]);
      const bool gate = valid ? valid[i] != 0 : crc_gate(f, len);
      ufc_codec::read_frame(HostBytes{f}, (uint32_t)len, gate, infos[i], nullptr, 0);
      infos[i].item_first = (uint32_t)c;  // local, rebased in pass 2
      c += infos[i].item_count;
    }
    part[t + 1] = c;
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(pass1, t);
  pass1(0);
  for (auto& x : th) x.join();
  th.clear();
  for (int t = 0; t < T; t++) part[t + 1] += part[t];
  const uint64_t total = part[T];
  if (items_used) *items_used = (size_t)total;
  const bool fill = items && total <= items_cap;
  // Pass 2: global item indices, items written by re-parsing accepted frames.
  auto pass2 = [&](int t) {
    const size_t a = n * t / T, b = n * (t + 1) / T;
    for (size_t i = a; i < b; i++) {
      const uint64_t first = part[t] + infos[i].item_first;
      infos[i].item_first = (uint32_t)first;
      if (fill && infos[i].ok && infos[i].item_count) {
        ufc_frame_info tmp;
        const uint8_t* f = bytes + offsets[i];
        ufc_codec::read_frame(HostBytes{f}, (uint32_t)(offsets[i + 1] - offsets[i]), true, tmp, items + first,
                              infos[i].item_count);
      }
    }
  };
  for (int t = 1; t < T; t++) th.emplace_back(pass2, t);
  pass2(0);
  for (auto& x : th) x.join();
  return (items && !fill) ? UFC_ERR_NOMEM : UFC_OK;
}

// ---- batched host build ----
int ufc_build_sizes_host(const ufc_frame_info* infos, const ufc_item* items, size_t n_items, const uint64_t* src_base,
                         size_t payload_len, size_t n, uint64_t* out_offsets, uint8_t* status, int nthreads) {
  if (n == 0) return UFC_OK;
  if (!infos || !out_offsets || (!items && n_items) || n >= ((size_t)1 << 31) || n_items >= ((size_t)1 << 31))
    return UFC_ERR_INVALID_ARG;
  for_ranges(n, nthreads, kRecordGrain, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; i++) {
      uint64_t size;
      const uint8_t st = ufc_codec::check_frame(infos[i], items, n_items, src_base ? src_base[i] : 0, payload_len, size);
      out_offsets[i + 1] = size;  // lengths first, summed below
      if (status) status[i] = st;
    }
  });
  out_offsets[0] = 0;
  for (size_t i = 0; i < n; i++) out_offsets[i + 1] += out_offsets[i];
  return UFC_OK;
}

int ufc_build_batch_host(const ufc_frame_info* infos, const ufc_item* items, size_t n_items, const uint64_t* src_base,
                         const uint8_t* payload, size_t payload_len, size_t n, const uint64_t* out_offsets,
                         uint8_t* out_bytes, size_t out_len, int seal, uint32_t* crc_out, int nthreads) {
  if (n == 0) return UFC_OK;
  if (!infos || !out_offsets || (!items && n_items) || (!payload && payload_len) || (!out_bytes && out_len) ||
      n >= ((size_t)1 << 31) || n_items >= ((size_t)1 << 31))
    return UFC_ERR_INVALID_ARG;
  const uint64_t first = out_offsets[0], last = out_offsets[n];
  for_ranges(n, nthreads, kRecordGrain, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; i++) {
      const ufc_frame_info& info = infos[i];
      const uint64_t base = src_base ? src_base[i] : 0;
      uint64_t size;
      const uint8_t st = ufc_codec::check_frame(info, items, n_items, base, payload_len, size);
      if (!ufc_codec::span_matches(st, size, out_offsets[i], out_offsets[i + 1], first, last, out_len)) continue;
      uint8_t* f = out_bytes + out_offsets[i];
      uint64_t w0, w1, w2;
      const uint32_t head = ufc_codec::encode_frame_head(info, w0, w1, w2);
      put_packed(f, w0, w1, w2, head);
      size_t pos = head;
      if (info.kind == UFC_FRAME_DATA) {
        for (uint32_t k = 0; k < info.item_count; k++) {
          const ufc_item& d = items[(size_t)info.item_first + k];
          const uint32_t hs = ufc_codec::datagram_header_size(d);
          ufc_codec::encode_datagram_header(d, hs, w0, w1);
          put_packed(f + pos, w0, w1, 0, hs);
          if (d.data_len) std::memcpy(f + pos + hs, payload + base + d.data_offset, d.data_len);
          pos += hs + d.data_len;
        }
      } else if (info.kind == UFC_FRAME_ACK) {
        for (uint32_t k = 0; k < info.item_count; k++) {
          ufc_codec::encode_ack_group(items[(size_t)info.item_first + k], w0, w1);
          put_packed(f + pos, w0, w1, 0, UFC_ACK_GROUP_SIZE);
          pos += UFC_ACK_GROUP_SIZE;
        }
      } else if (pos < size - 4) {  // handshake_syn's zero padding (:463)
        std::memset(f + pos, 0, (size_t)size - 4 - pos);
        pos = (size_t)size - 4;
      }
      trailer(f, pos, seal);
      if (seal && crc_out) crc_out[i] = ufc::host_extend(0u, f, pos);
    }
  });
  return UFC_OK;
}

// ---- batched host pack ----
namespace {
// One flush, item by item (emit.rs:47-125, 170-211 through the core's predicates).  infos null: the result
// only; else its frames into infos[r.frame_first ..], those below frames_cap.
void pack_flush(const ufc_item* items, uint64_t n_items, uint64_t first, uint64_t end, const ufc_flush& fl,
                const uint32_t* nonce_bits, ufc_frame_info* infos, uint64_t frames_cap, ufc_flush_result& r) {
  const uint32_t frame_first = r.frame_first;
  r = ufc_flush_result{frame_first, 0, 0, UFC_PACK_DONE, fl.flush_alloc};
  if (first > end || end > n_items) {
    r.stop = UFC_PACK_BAD_RANGE;
    return;
  }
  const bool ack = ufc_codec::pack_is_ack(fl);
  const uint32_t H = ufc_codec::pack_overhead(ack), max_count = ufc_codec::pack_max_count(ack);
  uint64_t spent = 0, s = 0, start = first;  // finalized bytes; the frame in progress: size (0: none), first item
  uint32_t c = 0, frames = 0;
  auto finalize = [&](uint64_t upto) {
    if (s == 0) return;
    const uint64_t g = (uint64_t)frame_first + frames;
    if (infos && g < frames_cap)
      infos[g] = ufc_codec::pack_frame_info(fl, ack, frames, g, nonce_bits, start, (uint32_t)(upto - start));
    frames++;
    spent += s;
    s = 0;
  };
  uint64_t i = first;
  for (; i < end; i++) {
    const uint64_t e = ack ? (uint64_t)UFC_ACK_GROUP_SIZE : ufc_codec::datagram_encoded_size(items[i]);
    const bool is_start = s == 0 || !ufc_codec::pack_frame_takes(s, c, e, max_count);
    const uint32_t why = ufc_codec::pack_stop(fl, ack, spent + s, is_start, frames + (s ? 1u : 0u));
    if (why != UFC_PACK_DONE) {
      r.stop = why;
      break;
    }
    if (is_start) {
      finalize(i);
      start = i;
      s = H + e;
      c = 1;
    } else {
      s += e;
      c++;
    }
  }
  finalize(i);
  r.frame_count = frames;
  r.items_packed = (uint32_t)(i - first);
  r.alloc_left = fl.flush_alloc - (int64_t)spent;
}
}  // namespace

int ufc_pack_host(const ufc_item* items, size_t n_items, const uint64_t* flush_first, const ufc_flush* flushes,
                  size_t n_flushes, const uint32_t* nonce_bits, ufc_frame_info* infos, size_t frames_cap,
                  ufc_flush_result* results, uint64_t* frames_used, int nthreads) {
  if (n_flushes == 0) return UFC_OK;
  if (!flush_first || !flushes || !results || !frames_used || (!items && n_items) || (!infos && frames_cap) ||
      n_flushes >= ((size_t)1 << 31) - 1 || n_items >= ((size_t)1 << 31) - 1)
    return UFC_ERR_INVALID_ARG;
  // Pass 1: every flush's result; then frame_first, their exclusive sum; pass 2: the frames.
  for_ranges(n_flushes, nthreads, kRecordGrain, [&](size_t a, size_t b) {
    for (size_t j = a; j < b; j++) {
      results[j].frame_first = 0;
      pack_flush(items, n_items, flush_first[j], flush_first[j + 1], flushes[j], nullptr, nullptr, 0, results[j]);
    }
  });
  uint64_t total = 0;
  for (size_t j = 0; j < n_flushes; j++) {
    results[j].frame_first = (uint32_t)total;
    total += results[j].frame_count;
  }
  *frames_used = total;
  if (!infos) return UFC_OK;
  for_ranges(n_flushes, nthreads, kRecordGrain, [&](size_t a, size_t b) {
    for (size_t j = a; j < b; j++)
      if (results[j].frame_count)
        pack_flush(items, n_items, flush_first[j], flush_first[j + 1], flushes[j], nonce_bits, infos, frames_cap,
                   results[j]);
  });
  return UFC_OK;
}

// ---- batched host emit ----
namespace {
// One sender, packet by packet (packet_sender.rs:149-238 through the core's functions).  Returns its item count,
// reserved slots included.  out false: the count only; else every output of the sender, its items at
// items[item_base + reserve_items ..), those below items_cap.  `sd` is a copy: senders_out may be the input.
uint64_t emit_sender(const ufc_packet* packets, uint64_t n_packets, uint64_t first, uint64_t end, const ufc_sender sd,
                     bool out, uint64_t item_base, ufc_item* items, uint64_t items_cap, ufc_packet_result* packet_results,
                     ufc_sender_result* result, ufc_sender* sender_out) {
  ufc_sender st = sd;
  ufc_sender_result r{};
  r.item_first = (uint32_t)item_base;
  if (first > end || end > n_packets) {
    if (out) {
      r.stop = UFC_EMIT_BAD_RANGE;
      *result = r;
      if (sender_out) *sender_out = st;
    }
    return 0;
  }
  const uint64_t n = std::min<uint64_t>(end - first, sd.take);
  const uint64_t max_alloc = ufc_codec::emit_max_alloc(sd.max_alloc);
  uint64_t made = sd.reserve_items;  // the sender's items so far
  uint64_t i = 0;
  r.stop = UFC_EMIT_DONE;
  for (; i < n; i++) {
    const ufc_packet& p = packets[first + i];
    const uint32_t cls = ufc_codec::emit_packet_class(p, sd.flush_id);
    if (cls == ufc_codec::kEmitBad) {
      r.stop = UFC_EMIT_BAD_PACKET;
      break;
    }
    if (cls == ufc_codec::kEmitStale) {
      r.packets_dropped++;
      r.bytes_dropped += p.data_len;
      if (out && packet_results) {
        ufc_packet_result pr{};
        pr.status = UFC_PACKET_DROPPED;
        packet_results[first + i] = pr;
      }
      continue;
    }
    if (((st.next_id - st.base_id) & ufc_codec::kPacketIdMask) >= st.window_size) {
      r.stop = UFC_EMIT_WINDOW_LIMITED;
      break;
    }
    const uint64_t a = ufc_codec::emit_alloc_size(p.data_len);
    if (ufc_codec::emit_alloc_fails(st.alloc, 0, a, max_alloc)) {
      r.stop = UFC_EMIT_ALLOC_LIMITED;
      break;
    }
    const uint32_t seq = st.next_id;
    const uint16_t wl = ufc_codec::emit_lead(seq, st.window_parent_id);
    const uint16_t cl = ufc_codec::emit_lead(seq, st.channel_parent_id[p.channel_id]);
    st.next_id = (st.next_id + 1) & ufc_codec::kPacketIdMask;
    st.alloc += a;
    if (p.mode == UFC_SEND_RELIABLE) st.window_parent_id = st.channel_parent_id[p.channel_id] = seq;
    const uint32_t count = ufc_codec::emit_fragment_count(p.data_len);
    if (out) {
      if (packet_results) {
        ufc_packet_result pr{};
        pr.sequence_id = seq;
        pr.item_first = (uint32_t)(item_base + made);
        pr.item_count = count;
        pr.status = UFC_PACKET_EMITTED;
        pr.resend = p.mode >= UFC_SEND_PERSISTENT ? 1 : 0;
        packet_results[first + i] = pr;
      }
      for (uint32_t f = 0; f < count && item_base + made + f < items_cap; f++)
        items[item_base + made + f] = ufc_codec::emit_item(p, seq, wl, cl, f, count - 1);
    }
    made += count;
    r.packets_emitted++;
  }
  if (out) {
    if (packet_results)
      for (uint64_t k = first + i; k < end; k++) packet_results[k] = ufc_packet_result{};  // not reached
    r.packets_consumed = (uint32_t)i;
    r.item_count = (uint32_t)made;
    *result = r;
    if (sender_out) *sender_out = st;
  }
  return made;
}
}  // namespace

int ufc_emit_packets_host(const ufc_packet* packets, size_t n_packets, const uint64_t* packet_first,
                          const ufc_sender* senders, size_t n_senders, ufc_item* items, size_t items_cap,
                          uint64_t* flush_first, ufc_packet_result* packet_results, ufc_sender_result* sender_results,
                          ufc_sender* senders_out, uint64_t* items_used, int nthreads) {
  if (n_senders == 0) return UFC_OK;
  if (!packet_first || !senders || !flush_first || !sender_results || !items_used || (!packets && n_packets) ||
      (!items && items_cap) || n_senders >= ((size_t)1 << 31) - 1 || n_packets >= ((size_t)1 << 31) - 1)
    return UFC_ERR_INVALID_ARG;
  // Pass 1: every sender's item count, into flush_first; then their exclusive sum; pass 2: the outputs.
  for_ranges(n_senders, nthreads, kRecordGrain, [&](size_t a, size_t b) {
    for (size_t s = a; s < b; s++)
      flush_first[s + 1] = emit_sender(packets, n_packets, packet_first[s], packet_first[s + 1], senders[s], false, 0,
                                       nullptr, 0, nullptr, nullptr, nullptr);
  });
  const uint64_t total = *items_used = counts_to_firsts(flush_first, n_senders);
  if (total >= ((uint64_t)1 << 31) - 1) return UFC_ERR_INVALID_ARG;
  for_ranges(n_senders, nthreads, kRecordGrain, [&](size_t a, size_t b) {
    for (size_t s = a; s < b; s++)
      emit_sender(packets, n_packets, packet_first[s], packet_first[s + 1], senders[s], true, flush_first[s], items,
                  items_cap, packet_results, &sender_results[s], senders_out ? &senders_out[s] : nullptr);
  });
  return UFC_OK;
}

}  // extern "C"

// ---- batched host receive ----
namespace {
// One copy segment, clipped at its destination's cap.
void rx_copy(const ufc_codec::RxArgs& a, const ufc_codec::RxSegment& sg) {
  if (!sg.len) return;
  const bool to_carry = (sg.kinds & ufc_codec::kRxDstCarry) != 0;
  const uint64_t cap = to_carry ? a.carry_cap : a.out_cap;
  if (sg.dst >= cap) return;
  const uint64_t len = std::min<uint64_t>(sg.len, cap - sg.dst);
  const uint8_t* src = ((sg.kinds & ufc_codec::kRxSrcCarry) ? a.carry_in : a.payload) + sg.src;
  std::memcpy((to_carry ? a.carry_out : a.out_bytes) + sg.dst, src, len);
}
}  // namespace

extern "C" {

int ufc_receive_packets_host(const ufc_frame_info* infos, size_t n_frames, const uint8_t* frame_accept,
                             const ufc_item* items, size_t n_items, const uint64_t* src_base, const uint8_t* payload,
                             size_t payload_len, const uint64_t* frame_first, const ufc_receiver* receivers,
                             size_t n_receivers, ufc_rx_slot* slots, const uint64_t* slot_first, size_t n_slots,
                             const uint8_t* carry_in, size_t carry_in_len, uint8_t* carry_out, size_t carry_cap,
                             uint64_t* carry_first, uint64_t* carry_used, ufc_rx_packet* packets, size_t packets_cap,
                             uint64_t* packet_first, uint64_t* packets_used, uint8_t* out_bytes, size_t out_cap,
                             uint64_t* out_used, uint8_t* item_status, ufc_receiver_result* results,
                             ufc_receiver* receivers_out, int nthreads) {
  if (n_receivers == 0) return UFC_OK;
  const ufc_codec::RxArgs a{infos, n_frames, frame_accept, items, n_items, src_base, payload, payload_len, frame_first,
                            receivers, n_receivers, slots, slot_first, n_slots, carry_in, carry_in_len, carry_out,
                            carry_cap, carry_first, carry_used, packets, packets_cap, packet_first, packets_used,
                            out_bytes, out_cap, out_used, item_status, results, receivers_out};
  if (!ufc_codec::rx_args_ok(a)) return UFC_ERR_INVALID_ARG;
  std::vector<ufc_codec::RxPlan> plans(n_slots);
  std::vector<uint8_t> own_status(item_status ? 0 : n_items);
  uint8_t* status = item_status ? item_status : own_status.data();
  std::vector<unsigned long long> table(ufc_codec::rx_dup_entries(n_items), 0ull);
  const ufc_codec::RxDupSet dups{table.data(), table.size() - 1};
  std::vector<uint64_t> out_first(n_receivers + 1);
  // Pass 1: every receiver's step; its counts into the three CSR arrays, then their exclusive sums.
  for_ranges(n_receivers, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      if (receivers_out != receivers) receivers_out[r] = receivers[r];
      uint64_t c[3];
      ufc_codec::rx_walk(a, r, plans.data(), status, dups, c);
      packet_first[r + 1] = c[0];
      out_first[r + 1] = c[1];
      carry_first[r + 1] = c[2];
    }
  });
  *packets_used = counts_to_firsts(packet_first, n_receivers);
  *out_used = counts_to_firsts(out_first.data(), n_receivers);
  *carry_used = counts_to_firsts(carry_first, n_receivers);
  // Pass 2: records, layout, bits and segments; then the copies, the slots' before the datagrams'.
  std::vector<ufc_codec::RxSegment> segs(2 * n_slots + n_items);
  for_ranges(n_receivers, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) ufc_codec::rx_finish(a, r, plans.data(), status, out_first[r], segs.data(), nullptr);
  });
  for_ranges(2 * n_slots, nthreads, kRecordGrain, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) rx_copy(a, segs[k]);
  });
  for_ranges(n_items, nthreads, kRecordGrain, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) rx_copy(a, segs[2 * n_slots + k]);
  });
  return UFC_OK;
}

// ---- batched host frame window ----
int ufc_frame_window_host(const ufc_frame_info* infos, size_t n_frames, const uint64_t* frame_first,
                          const ufc_frame_window* windows, size_t n_windows, uint8_t* frame_accept,
                          ufc_item* groups, size_t groups_cap, uint64_t* group_first, uint64_t* groups_used,
                          ufc_frame_window_result* results, ufc_frame_window* windows_out, int nthreads) {
  if (n_windows == 0) return UFC_OK;
  const ufc_codec::FwArgs a{infos, n_frames, frame_first, windows, n_windows, frame_accept, groups, groups_cap,
                            group_first, groups_used, results, windows_out};
  if (!ufc_codec::fw_args_ok(a)) return UFC_ERR_INVALID_ARG;
  // Pass 1: every connection's group count, into group_first; then their exclusive sum; pass 2: the outputs.
  for_ranges(n_windows, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) group_first[r + 1] = ufc_codec::fw_walk_serial(a, r, false, 0);
  });
  *groups_used = counts_to_firsts(group_first, n_windows);
  for_ranges(n_windows, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) ufc_codec::fw_walk_serial(a, r, true, group_first[r]);
  });
  return UFC_OK;
}

// ---- batched host frame queue ----
int ufc_frame_queue_host(const ufc_frame_info* infos, size_t n_frames, const ufc_item* items, size_t n_items,
                         const uint64_t* frame_first, const ufc_sent_frame* sent, size_t n_sent,
                         const uint64_t* sent_first, const ufc_frame_queue* queues, const ufc_frame_queue_step* steps,
                         size_t n_queues, ufc_sent_frame* log, size_t n_log, uint8_t* ref_acked, size_t refs_cap,
                         ufc_frame_queue_result* results, ufc_frame_queue* queues_out, int nthreads) {
  if (n_queues == 0) return UFC_OK;
  const ufc_codec::FqArgs a{infos, n_frames, items, n_items, frame_first, sent, n_sent, sent_first, queues, steps,
                            n_queues, log, n_log, ref_acked, refs_cap, results, queues_out};
  if (!ufc_codec::fq_args_ok(a)) return UFC_ERR_INVALID_ARG;
  // The step the device runs, the lanes of a phase one after the other; a connection touches its own ring, its
  // own records and (with ranges that do not overlap) its own fragment marks, so the connections run in parallel.
  for_ranges(n_queues, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    ufc_codec::FqWaveShared sh;
    for (size_t c = lo; c < hi; c++) ufc_codec::fq_step(ufc_codec::SerialWave{}, sh, a, c);
  });
  return UFC_OK;
}

// ---- batched host send rate control ----
int ufc_rate_begin_host(const ufc_rate_state* states, const uint64_t* now_ms, const uint32_t* extra_flags, size_t n,
                        ufc_frame_queue_step* steps, ufc_rate_state* states_out, int nthreads) {
  if (n == 0) return UFC_OK;
  const ufc_codec::RateBeginArgs a{states, now_ms, extra_flags, n, steps, states_out};
  if (!ufc_codec::rate_begin_args_ok(a)) return UFC_ERR_INVALID_ARG;
  for_ranges(n, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; c++) {
      ufc_rate_state S = states[c];
      ufc_frame_queue_step Q;
      ufc_codec::rate_begin(S, now_ms[c], extra_flags ? extra_flags[c] : 0, Q);
      steps[c] = Q;
      states_out[c] = S;
    }
  });
  return UFC_OK;
}

int ufc_rate_step_host(const ufc_rate_state* states, const ufc_rate_tick* ticks, const ufc_frame_queue_result* fq,
                       size_t n, ufc_recv_rate_entry* entries, size_t n_entries, const ufc_flush_result* flush_results,
                       size_t n_flush_results, const uint32_t* result_index, ufc_flush* flushes, size_t n_flushes,
                       const uint32_t* flush_index, ufc_rate_result* results, ufc_rate_state* states_out, int nthreads) {
  if (n == 0) return UFC_OK;
  const ufc_codec::RateArgs a{states, ticks, fq, n, entries, n_entries, flush_results, n_flush_results, result_index,
                              flushes, n_flushes, flush_index, results, states_out};
  if (!ufc_codec::rate_args_ok(a)) return UFC_ERR_INVALID_ARG;
  // The step the device gives a lane; a connection touches its own records, its own entries and its own flush.
  for_ranges(n, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; c++) {
      ufc_rate_state S = states[c];
      ufc_rate_result R;
      ufc_codec::rate_step(a, c, S, ticks[c], fq[c], R);
      results[c] = R;
      states_out[c] = S;
    }
  });
  return UFC_OK;
}

// ---- batched host resend ----
int ufc_resend_begin_host(const ufc_frame_info* infos, size_t n_frames, const uint64_t* frame_first,
                          const ufc_frame_queue* queues, const ufc_sent_frame* log, size_t n_log,
                          const ufc_rate_result* rate, const uint32_t* flags, const ufc_flush* flushes,
                          const ufc_resend* states, const ufc_sender* senders, size_t n, ufc_resend_entry* heap,
                          size_t n_heap, const ufc_sent_packet* pkts, size_t n_pkts, uint8_t* frag_acked, size_t n_frag,
                          const ufc_tx_ref* tx, size_t n_tx, uint8_t* ref_acked, size_t refs_cap, ufc_item* stage,
                          size_t n_stage, ufc_resend_result* results, ufc_resend* states_out, ufc_sender* senders_out,
                          int nthreads) {
  if (n == 0) return UFC_OK;
  const ufc_codec::RsBeginArgs a{infos, n_frames, frame_first, queues, log, n_log, rate, flags, flushes, states, senders,
                                 n, heap, n_heap, pkts, n_pkts, frag_acked, n_frag, tx, n_tx, ref_acked, refs_cap, stage,
                                 n_stage, results, states_out, senders_out};
  if (!ufc_codec::rs_begin_args_ok(a)) return UFC_ERR_INVALID_ARG;
  // The step the device runs; a connection touches its own regions and records, so the connections run in parallel.
  for_ranges(n, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    ufc_codec::RsWaveShared sh;
    for (size_t c = lo; c < hi; c++) ufc_codec::rs_begin(ufc_codec::SerialWave{}, sh, a, c);
  });
  return UFC_OK;
}

int ufc_resend_place_host(const ufc_resend* states, const ufc_resend_result* begin_results, size_t n,
                          const ufc_item* stage, size_t n_stage, const uint64_t* flush_first, ufc_item* items,
                          size_t items_cap, int nthreads) {
  if (n == 0) return UFC_OK;
  const ufc_codec::RsPlaceArgs a{states, begin_results, n, stage, n_stage, flush_first, items, items_cap};
  if (!ufc_codec::rs_place_args_ok(a)) return UFC_ERR_INVALID_ARG;
  for_ranges(n, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; c++) ufc_codec::rs_place(ufc_codec::SerialWave{}, a, c);
  });
  return UFC_OK;
}

int ufc_resend_commit_host(const ufc_flush_result* flush_results, const ufc_frame_info* infos, size_t n_infos,
                           const uint64_t* out_offsets, const uint64_t* frames_used, const ufc_item* items,
                           size_t n_items, const uint64_t* flush_first, const ufc_packet* packets, size_t n_packets,
                           const uint64_t* packet_first, const ufc_packet_result* packet_results,
                           const ufc_sender_result* sender_results, const ufc_resend_result* begin_results,
                           const ufc_rate_result* rate, const ufc_resend* states, const ufc_sender* senders, size_t n,
                           ufc_resend_entry* heap, size_t n_heap, ufc_sent_packet* pkts, size_t n_pkts,
                           uint8_t* frag_acked, size_t n_frag, ufc_tx_ref* tx, size_t n_tx, ufc_sent_frame* sent,
                           size_t sent_cap, uint64_t* sent_first, uint32_t* next_extra_flags,
                           ufc_resend_commit_result* results, ufc_resend* states_out, ufc_sender* retake, int nthreads) {
  if (n == 0) return UFC_OK;
  const ufc_codec::RsCommitArgs a{flush_results, infos, n_infos, out_offsets, frames_used, items, n_items, flush_first,
                                  packets, n_packets, packet_first, packet_results, sender_results, begin_results, rate,
                                  states, senders, n, heap, n_heap, pkts, n_pkts, frag_acked, n_frag, tx, n_tx, sent,
                                  sent_cap, sent_first, next_extra_flags, results, states_out, retake};
  if (!ufc_codec::rs_commit_args_ok(a)) return UFC_ERR_INVALID_ARG;
  for_ranges(n, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    ufc_codec::RsWaveShared sh;
    for (size_t c = lo; c < hi; c++) ufc_codec::rs_commit(ufc_codec::SerialWave{}, sh, a, c);
  });
  return UFC_OK;
}

// ---- batched host flush control ----
int ufc_flush_acks_host(const ufc_flush_ctl* ctl, const ufc_frame_window* windows, const ufc_item* groups,
                        size_t n_groups, const uint64_t* group_first, const ufc_receiver* receivers,
                        const ufc_rate_result* rate, size_t n, ufc_item* carry, size_t n_carry, ufc_item* merged,
                        size_t merged_cap, uint64_t* merged_first, uint64_t* merged_used, ufc_frame_info* infos,
                        size_t frames_cap, uint64_t* frames_used, ufc_flush_result* results,
                        ufc_flush_acks_result* ack_results, ufc_frame_window* windows_out, ufc_flush_ctl* ctl_out,
                        ufc_flush* flushes, uint32_t* flags, int nthreads) {
  if (n == 0) return UFC_OK;
  const ufc_codec::FaArgs a{ctl, windows, groups, n_groups, group_first, receivers, rate, n, carry, n_carry, merged,
                            merged_cap, merged_first, merged_used, infos, frames_cap, frames_used, results, ack_results,
                            windows_out, ctl_out, flushes, flags};
  if (!ufc_codec::fa_args_ok(a)) return UFC_ERR_INVALID_ARG;
  // Pass 1: every connection's merged and frame counts; then their exclusive sums; pass 2: the outputs.
  std::vector<uint64_t> frame_first(n + 1);
  for_ranges(n, nthreads, kRecordGrain, [&](size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; c++) {
      const ufc_codec::FaPlan p = ufc_codec::fa_plan(a, c);
      merged_first[c + 1] = p.merged;
      frame_first[c + 1] = p.frames;
    }
  });
  *merged_used = counts_to_firsts(merged_first, n);
  *frames_used = counts_to_firsts(frame_first.data(), n);
  for_ranges(n, nthreads, kStepGrain, [&](size_t lo, size_t hi) {
    ufc_codec::FaWaveShared sh;
    for (size_t c = lo; c < hi; c++) ufc_codec::fa_write(ufc_codec::SerialWave{}, sh, a, c, frame_first[c]);
  });
  return UFC_OK;
}

int ufc_flush_sync_host(const ufc_flush_ctl* ctl, const ufc_rate_result* rate, const ufc_flush_result* ack_results,
                        const ufc_resend_result* begin_results, const ufc_flush_result* pack_results,
                        const ufc_resend_commit_result* commit_results, const ufc_frame_queue* queues,
                        const ufc_sender* senders, size_t n, ufc_frame_info* infos, size_t syncs_cap,
                        uint32_t* sync_index, uint64_t* syncs_used, ufc_flush_sync_result* results,
                        ufc_flush_ctl* ctl_out, ufc_rate_tick* ticks_next, int nthreads) {
  if (n == 0) return UFC_OK;
  const ufc_codec::FsArgs a{ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders, n,
                            infos, syncs_cap, sync_index, syncs_used, results, ctl_out, ticks_next};
  if (!ufc_codec::fs_args_ok(a)) return UFC_ERR_INVALID_ARG;
  // The tiles the device gives a wave each: the decisions, the exclusive sum of their counts, the frames.
  const size_t n_tiles = (n + 63) / 64;
  std::vector<uint64_t> tile_first(n_tiles + 1);
  for_ranges(n_tiles, nthreads, kRecordGrain / 64, [&](size_t lo, size_t hi) {
    for (size_t t = lo; t < hi; t++) tile_first[t + 1] = ufc_codec::fs_decide_tile(ufc_codec::SerialWave{}, a, t);
  });
  *syncs_used = counts_to_firsts(tile_first.data(), n_tiles);
  for_ranges(n_tiles, nthreads, kRecordGrain / 64, [&](size_t lo, size_t hi) {
    for (size_t t = lo; t < hi; t++) ufc_codec::fs_write_tile(ufc_codec::SerialWave{}, a, t, tile_first[t]);
  });
  return UFC_OK;
}

// ---- batched host frame routing ----
int ufc_route_table_build_host(const ufc_addr* addrs, size_t n_conns, uint32_t seed, ufc_route_slot* slots,
                               size_t n_slots, uint32_t* max_probe, uint64_t* dup_index) {
  if (!slots || !max_probe || (!addrs && n_conns) || !ufc_codec::rt_table_ok(n_slots, n_conns))
    return UFC_ERR_INVALID_ARG;
  std::memset(slots, 0, n_slots * sizeof(ufc_route_slot));
  const uint32_t mask = (uint32_t)(n_slots - 1);
  uint32_t longest = 0;
  for (size_t c = 0; c < n_conns; c++) {
    const ufc_codec::RtKey k = ufc_codec::rt_key(addrs[c]);
    const uint32_t home = ufc_codec::rt_hash(seed, k.w) & mask;
    // n_slots > n_conns: an empty slot is met before the probe comes round, and an equal key before that slot.
    uint32_t p = 0;
    for (;; p++) {
      ufc_route_slot& s = slots[(home + p) & mask];
      if (!s.used) {
        s.key = addrs[c];
        s.conn = (uint32_t)c;
        s.used = 1;
        break;
      }
      if (ufc_codec::rt_key_eq(ufc_codec::rt_key(s.key).w, k.w)) {
        if (dup_index) *dup_index = c;
        return UFC_ERR_INVALID_ARG;
      }
    }
    longest = std::max(longest, p);
  }
  *max_probe = longest;
  return UFC_OK;
}

int ufc_route_frames_host(const ufc_frame_info* infos, const ufc_addr* addrs, const uint64_t* offsets, size_t n,
                          const ufc_route_slot* slots, size_t n_slots, uint32_t seed, uint32_t max_probe,
                          size_t n_conns, const uint8_t* conn_active, uint64_t now_ms, uint64_t active_timeout_ms,
                          const uint64_t* timeout_in, uint32_t* route, uint8_t* cls, uint64_t* bucket_first,
                          uint32_t* order, ufc_frame_info* infos_out, uint64_t* src_base_out,
                          ufc_route_result* results, uint64_t* timeout_out, uint32_t* first_unknown_control,
                          int nthreads) {
  const ufc_codec::RtArgs a{infos, addrs, offsets, n, slots, n_slots, seed, max_probe, n_conns, conn_active, now_ms,
                            active_timeout_ms, timeout_in, route, cls, bucket_first, order, infos_out, src_base_out,
                            results, timeout_out, first_unknown_control};
  if (!ufc_codec::rt_args_ok(a)) return UFC_ERR_INVALID_ARG;
  for (size_t c = 0; c < n_conns; c++) results[c] = ufc_route_result{0, UFC_NO_PARENT, 0, 0};
  *first_unknown_control = UFC_NO_PARENT;
  std::fill(bucket_first, bucket_first + n_conns + 3, (uint64_t)0);
  // The lookups; then the first control frames, in arrival order (the device takes the same minima).
  for_ranges(n, nthreads, kRecordGrain, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) route[i] = ufc_codec::rt_lookup(slots, n_slots, seed, max_probe, n_conns, addrs[i]);
  });
  for (size_t i = 0; i < n; i++) {
    if (ufc_codec::rt_kind_class(infos[i]) != 1) continue;
    uint32_t& first = route[i] == UFC_NO_PARENT ? *first_unknown_control : results[route[i]].first_control;
    if (first == UFC_NO_PARENT) first = (uint32_t)i;
  }
  // The classes; the buckets' counts and their exclusive sum; the stable placement with a cursor per bucket.
  for_ranges(n, nthreads, kRecordGrain, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) cls[i] = (uint8_t)ufc_codec::rt_classify(a, i, ufc_codec::rt_kind_class(infos[i]));
  });
  for (size_t i = 0; i < n; i++) {
    bucket_first[ufc_codec::rt_bucket(a, i, cls[i]) + 1]++;
    if (cls[i] == UFC_ROUTE_DEFERRED && route[i] != UFC_NO_PARENT) results[route[i]].deferred++;
  }
  counts_to_firsts(bucket_first, n_conns + 2);
  {
    std::vector<uint64_t> cursor(bucket_first, bucket_first + n_conns + 2);
    for (size_t i = 0; i < n; i++) order[cursor[ufc_codec::rt_bucket(a, i, cls[i])]++] = (uint32_t)i;
  }
  for_ranges(n, nthreads, kRecordGrain, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      std::memcpy(&infos_out[k], &infos[order[k]], sizeof(ufc_frame_info));
      src_base_out[k] = ufc_codec::rt_src_base(a, order[k]);
    }
  });
  for (size_t c = 0; c < n_conns; c++) ufc_codec::rt_finish_conn(a, c);
  return UFC_OK;
}

}  // extern "C"
