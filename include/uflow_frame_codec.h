/*
 * uflow_frame_codec.h -- C ABI of libuflowcrc.so for uflow's frame codec around the CRC gate:
 * the rest of Frame::read (type dispatch and payload parse), the frame writers and builders, and
 * batched parses that consume the batched CRC gate's valid flags.
 *
 * Reference (lowquark/uflow v0.7.1, Rust) interfaces each entry point replaces:
 *   ufc_frame_read             <- src/frame/serial/mod.rs:674-706  `Frame::read` (Serialize::read), with
 *                                 read_*_payload :54-434 and read_datagram :183-309
 *   ufc_frame_write_fixed      <- src/frame/serial/mod.rs:437-611, 623-657  write_handshake_*,
 *                                 write_disconnect[_ack], write_sync
 *   ufc_data_frame_builder_*   <- src/frame/serial/build.rs:47-181  DataFrameBuilder::{new, add, build,
 *                                 count, size, encoded_size}
 *   ufc_ack_frame_builder_*    <- src/frame/serial/build.rs:183-256  AckFrameBuilder::{new, add, build, size}
 *   ufc_parse_batch_host       <- the receive loops' Frame::read of every datagram (src/server/mod.rs:
 *                                 591-602, src/client/mod.rs:615-623), after the batched CRC gate
 *   ufc_parse_batch_varlen     <- the same parse on the GPU, device-resident frames
 *   ufc_build_sizes_host, ufc_build_batch_host, ufc_build_sizes_varlen, ufc_build_batch_varlen
 *                              <- the emitters' Frame::write of every data and ack frame they send
 *                                 (src/half_connection/emit.rs:47-125, 170-211 over build.rs:55-162,
 *                                 192-247) and write_* (serial/mod.rs:437-657), batched from the parse's
 *                                 records, on the host and on the GPU
 *   ufc_pack_host, ufc_pack_varlen
 *                              <- the emitters' push / finalize loop that cuts a flush's datagrams or ack
 *                                 groups into frames (src/half_connection/emit.rs:47-125, 170-211), many
 *                                 flushes per call, on the host and on the GPU
 *   ufc_emit_packets_host, ufc_emit_packets_varlen
 *                              <- PacketSender::emit_packet (src/half_connection/packet_sender.rs:149-238),
 *                                 PendingPacket::new / datagram (pending_packet.rs:23-42, 84-103) and the
 *                                 new-packet loop of emit_data_frames (half_connection/mod.rs:385-427): queued
 *                                 packets into the datagram items the packs take, many senders per call, on
 *                                 the host and on the GPU
 *   ufc_receive_packets_host, ufc_receive_packets_varlen
 *                              <- PacketReceiver::handle_datagram, receive and resynchronize
 *                                 (src/half_connection/packet_receiver/mod.rs:142-218, 286-402, 408-435) over
 *                                 AssemblyWindow and FragmentBuffer (assembly_window/mod.rs:69-199,
 *                                 fragment_buffer.rs:12-57): the parses' datagram items into delivered packets,
 *                                 many receivers per call, on the host and on the GPU
 *   ufc_frame_window_host, ufc_frame_window_varlen
 *                              <- FrameAckQueue::window_contains, mark_seen, resynchronize and base_id
 *                                 (src/half_connection/frame_ack_queue.rs) as handle_data_frame and
 *                                 handle_sync_frame call them (src/half_connection/mod.rs:132-152): the parses'
 *                                 frames into the receive's frame_accept verdicts and the packs' ack groups,
 *                                 many connections per call, on the host and on the GPU
 *   ufc_frame_queue_*, ufc_rate_begin_*, ufc_rate_step_*
 *                              <- FrameQueue, SendRateComp and HalfConnection::step (their sections below)
 *   ufc_resend_begin_*, ufc_resend_place_*, ufc_resend_commit_*
 *                              <- PacketSender::acknowledge (packet_sender.rs:242-275), the resend queue
 *                                 (resend_queue.rs), the pending queue (pending_queue.rs) and emit_data_frames
 *                                 (half_connection/mod.rs:335-432) around the emit and the pack, many connections per
 *                                 call, on the host and on the GPU
 *   ufc_flush_acks_*, ufc_flush_sync_* (declared in uflow_flush_ctl.h, included at the end of this header)
 *                              <- emit_ack_frames with push_dud and the FrameAckQueue deque's carry
 *                                 (half_connection/mod.rs:296-333 over emit.rs:137-211), emit_sync_frame
 *                                 (mod.rs:234-294) and the early returns of emit_frames (:217-232), many
 *                                 connections per call, on the host and on the GPU
 *   ufc_route_table_build_host, ufc_route_frames_* (declared in uflow_route.h, included at the end of this header)
 *                              <- the address lookup and dispatch of Server::handle_frames (src/server/mod.rs:
 *                                 591-602 over :492-589, clients: HashMap<SocketAddr, ..> :118) and of
 *                                 Client::handle_frames (src/client/mod.rs:557-583) for State::Active clients:
 *                                 the parse's frames grouped by connection, on the host and on the GPU
 *   ufc_datagram_is_valid, UFC_ITEM_VALID
 *                              <- src/half_connection/packet_receiver/mod.rs:12-30 `datagram_is_valid`,
 *                                 applied by handle_datagram (:147-150) to every received datagram
 *
 * Conventions: as uflow_frame_crc.h.  A frame the reference would reject is data (ok = 0), never
 * an error; nothing is allocated per call except where stated (the device parse's scan scratch
 * grows inside the context).  Decoded datagrams point into the frame (data_offset, data_len);
 * nothing is copied.
 */
#ifndef UFLOW_FRAME_CODEC_H
#define UFLOW_FRAME_CODEC_H

#include <stddef.h>
#include <stdint.h>

#include "uflow_frame_crc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frame ids (src/frame/serial/mod.rs:15-23). */
#define UFC_FRAME_HANDSHAKE_SYN 0
#define UFC_FRAME_HANDSHAKE_SYN_ACK 1
#define UFC_FRAME_HANDSHAKE_ACK 2
#define UFC_FRAME_HANDSHAKE_ERROR 3
#define UFC_FRAME_DISCONNECT 4
#define UFC_FRAME_DISCONNECT_ACK 5
#define UFC_FRAME_DATA 10
#define UFC_FRAME_SYNC 11
#define UFC_FRAME_ACK 12
/* Wire constants (src/frame/serial/mod.rs:25-44). */
#define UFC_DATA_FRAME_MAX_DATAGRAM_COUNT 127
#define UFC_ACK_GROUP_SIZE 9
#define UFC_MAX_CHANNELS 64

/* One decoded frame (32 bytes).  Fields by kind (f[] in wire order):
 *   handshake_syn      aux = version; f = nonce, max_receive_rate, max_packet_size, max_receive_alloc
 *   handshake_syn_ack  f = nonce_ack, nonce, max_receive_rate, max_packet_size, max_receive_alloc
 *   handshake_ack      f = nonce_ack
 *   handshake_error    f = nonce_ack; aux = error (0 Version, 1 Config, 2 ServerFull)
 *   disconnect[_ack]   -
 *   data               f = sequence_id; aux = nonce (0/1); item_count = datagrams
 *   sync               aux = mode (bit 0: next_frame_id present, bit 1: next_packet_id present);
 *                      f = next_frame_id, next_packet_id (0 when absent)
 *   ack                f = frame_window_base_id, packet_window_base_id; item_count = ack groups
 * ok = 1 exactly when Frame::read returns Some; with ok = 0 the other fields are unspecified
 * except kind (byte 0 of the frame, or 0xFF for frames shorter than 1 byte). */
typedef struct ufc_frame_info {
  uint8_t kind;
  uint8_t ok;
  uint8_t aux;
  uint8_t crc_ok;      /* the CRC gate alone (len >= 5 and the trailer matches) */
  uint32_t f[5];
  uint32_t item_count;
  uint32_t item_first; /* batched parses: index of the frame's first item in the item array */
} ufc_frame_info;

/* One datagram of a data frame, or one ack group of an ack frame (24 bytes). */
typedef struct ufc_item {
  uint32_t id;                  /* datagram: sequence_id; ack group: base_id */
  uint8_t channel_id;           /* datagram: channel_id; ack group: nonce (0/1) */
  uint8_t form;                 /* datagram header: 0 micro, 1 small, 2 large; 3 = ack group */
  uint16_t window_parent_lead;
  uint16_t channel_parent_lead;
  uint16_t fragment_id;
  uint16_t fragment_id_last;
  uint16_t flags;               /* datagram: UFC_ITEM_VALID if datagram_is_valid (below); ack group: 0 */
  uint32_t data_offset;         /* datagram: payload offset in the frame; ack group: bitfield */
  uint32_t data_len;            /* datagram: payload bytes; ack group: 0 */
} ufc_item;

/* ufc_item.flags bit: the datagram passes the receive side's content check,
 * src/half_connection/packet_receiver/mod.rs:12-30 `datagram_is_valid` (channel < 64; a nonzero
 * channel_parent_lead needs window_parent_lead != 0 and channel_parent_lead >= window_parent_lead;
 * fragment_id <= fragment_id_last; every fragment but the last exactly UFC_MAX_FRAGMENT_SIZE bytes;
 * no payload over UFC_MAX_FRAGMENT_SIZE).  handle_datagram (:147-150) drops datagrams without it. */
#define UFC_ITEM_VALID 1
/* MAX_FRAGMENT_SIZE = MAX_FRAME_SIZE - DATA_FRAME_OVERHEAD - MAX_DATAGRAM_OVERHEAD (src/lib.rs:297). */
#define UFC_MAX_FRAGMENT_SIZE 1448

/* ---- scalar host entry points ---- */
/* Frame::read: 1 = Some, 0 = None.  info is always written; up to items_cap items are written
 * (info->item_count says how many the frame holds; UFC_ERR_NOMEM if items_cap is smaller). */
int ufc_frame_read(const uint8_t* frame, size_t len, ufc_frame_info* info, ufc_item* items, size_t items_cap);

/* The rest of Frame::read after an external CRC gate (e.g. the batched GPU gate): crc_ok is the
 * gate's verdict for this frame.  Returns and fills as ufc_frame_read. */
int ufc_frame_parse(const uint8_t* frame, size_t len, int crc_ok, ufc_frame_info* info, ufc_item* items,
                    size_t items_cap);

/* datagram_is_valid (src/half_connection/packet_receiver/mod.rs:12-30) of a decoded datagram
 * (form 0..2): 1 valid, 0 not (the parses store the same verdict in flags & UFC_ITEM_VALID). */
int ufc_datagram_is_valid(const ufc_item* datagram);

/* Fixed-size frames (every kind but data and ack) from info; writes the BE32 CRC trailer when
 * seal != 0, else 4 zero bytes (for a batched seal on the GPU).  Returns the frame length, 0 if
 * cap is too small or the kind is data/ack/unknown. */
size_t ufc_frame_write_fixed(const ufc_frame_info* info, uint8_t* out, size_t cap, int seal);

/* Builders over a caller-owned buffer. */
typedef struct ufc_builder {
  uint8_t* buf;
  size_t cap;
  size_t len;      /* bytes written so far (header + items, no trailer) */
  uint32_t count;  /* datagrams or ack groups added */
  uint32_t kind;   /* UFC_FRAME_DATA or UFC_FRAME_ACK */
} ufc_builder;

typedef struct ufc_datagram_ref {
  uint32_t sequence_id;
  uint8_t channel_id;
  uint8_t reserved;
  uint16_t window_parent_lead;
  uint16_t channel_parent_lead;
  uint16_t fragment_id;
  uint16_t fragment_id_last;
  const uint8_t* data;
  size_t data_len;
} ufc_datagram_ref;

int ufc_data_frame_builder_init(ufc_builder* b, uint8_t* buf, size_t cap, uint32_t sequence_id, int nonce);
/* UFC_ERR_INVALID_ARG for what build.rs debug_asserts (channel >= 64, sequence id >= 2^20,
 * data > 65535 B, already 127 datagrams) and when the buffer would overflow (trailer included). */
int ufc_data_frame_builder_add(ufc_builder* b, const ufc_datagram_ref* d);
size_t ufc_data_frame_encoded_size(const ufc_datagram_ref* d);
int ufc_ack_frame_builder_init(ufc_builder* b, uint8_t* buf, size_t cap, uint32_t frame_window_base_id,
                               uint32_t packet_window_base_id);
int ufc_ack_frame_builder_add(ufc_builder* b, uint32_t base_id, uint32_t bitfield, int nonce);
/* Frame size once built: len + 4 (build.rs:169-171, 249-251). */
size_t ufc_builder_size(const ufc_builder* b);
/* Patches the count (build.rs:148-149 / 231-234) and appends the trailer: BE32 CRC if seal != 0,
 * else 4 zero bytes.  Returns the frame length. */
size_t ufc_builder_build(ufc_builder* b, int seal);

/* ---- batched parses (CSR batch: frame i = bytes[offsets[i] .. offsets[i+1])) ----
 * valid: the batched CRC gate's flags (ufc_crc_batch_varlen / ufc_validate_host_varlen); NULL =
 * check the CRC here.  infos[n]; items in frame order, infos[i].item_first the first of frame i;
 * *items_used = total items of accepted frames (items of rejected frames are not emitted); if it
 * exceeds items_cap only infos are complete and UFC_ERR_NOMEM is returned. */
int ufc_parse_batch_host(const uint8_t* bytes, const uint64_t* offsets, size_t n, const uint8_t* valid,
                         ufc_frame_info* infos, ufc_item* items, size_t items_cap, size_t* items_used,
                         int nthreads);
/* Device-resident, asynchronous on `stream`: d_valid is required (the gate's output), d_items_used
 * is one device word.  Items beyond items_cap are dropped (compare *d_items_used with the cap). */
int ufc_parse_batch_varlen(ufc_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, size_t n,
                           const uint8_t* d_valid, ufc_frame_info* d_infos, ufc_item* d_items, size_t items_cap,
                           uint64_t* d_items_used, void* stream);

/* ---- batched builds: Frame::write of every frame of a batch, from the parse's records ----
 * The inverse of the batched parses.  Input is their output format:
 *   infos[n]        kind, ok, aux, f[], item_count and item_first are used; crc_ok is ignored.
 *   items[n_items]  datagram: id, channel_id, window_parent_lead, channel_parent_lead, fragment_id,
 *                   fragment_id_last, data_len, and data_offset = the payload's offset relative to the
 *                   frame's source base; ack group: id = base_id, data_offset = bitfield, channel_id != 0 =
 *                   nonce.  form and flags are ignored: the header form is chosen as DataFrameBuilder::add
 *                   does (build.rs:81-122), so a datagram with fragment_id_last == 0 takes the micro or
 *                   small form when its sizes allow and its fragment_id is then not encoded.
 *   src_base[n]     (nullable: all zero) the byte offset in `payload` that frame i's data_offsets are
 *                   relative to.  Passing a parsed batch's own offsets and bytes as src_base and payload
 *                   re-emits that batch with no copy in between.
 * Output is a CSR batch: frame i = out_bytes[out_offsets[i] .. out_offsets[i+1]), byte for byte what
 * Frame::write gives (handshake_syn zero-padded to UFC_MAX_FRAME_SIZE).  MAX_FRAME_SIZE is NOT enforced:
 * the reference enforces it in the emitter (emit.rs:69), not in the builder, and so does the caller here.
 *
 * Per-frame status: */
#define UFC_BUILD_OK 0
#define UFC_BUILD_SKIPPED 1   /* infos[i].ok == 0: nothing to write */
#define UFC_BUILD_BAD_FIELD 2 /* what build.rs:74-77, 146 debug-assert, and records that describe no frame: an
                                 unknown kind; item_first + item_count > n_items; data: item_count > 127, aux > 1,
                                 channel_id >= 64, id >= 2^20, data_len > 65535; ack: item_count > 65535; sync:
                                 aux > 3; handshake_error: aux > 2 */
#define UFC_BUILD_BAD_SRC 3   /* a payload range leaves [0, payload_len) */
/* Sizes: out_offsets[n + 1] (CSR: [0] = 0, [n] = total bytes) and status[n] (nullable).  Frames whose
 * status is not UFC_BUILD_OK get length 0. */
int ufc_build_sizes_host(const ufc_frame_info* infos, const ufc_item* items, size_t n_items, const uint64_t* src_base,
                         size_t payload_len, size_t n, uint64_t* out_offsets, uint8_t* status, int nthreads);
/* Write: frame i into out_bytes[out_offsets[i] .. out_offsets[i+1]), with the BE32 CRC as trailer if
 * seal != 0, else 4 zero bytes (for a later batched seal).  The call stands alone (it needs nothing a
 * sizes call left behind) and trusts out_offsets as the other CSR entry points trust theirs: frame i is
 * written only when its span's length equals the frame's size and the span lies inside
 * [out_offsets[0], out_offsets[n]) and ends at or before out_len; otherwise its span is left untouched (a
 * length-0 span is the way to skip a frame).  Nothing outside [out_offsets[0], out_offsets[n]) is written.
 * crc_out[n] (nullable, seal != 0 only): the CRC words of the frames written. */
int ufc_build_batch_host(const ufc_frame_info* infos, const ufc_item* items, size_t n_items, const uint64_t* src_base,
                         const uint8_t* payload, size_t payload_len, size_t n, const uint64_t* out_offsets,
                         uint8_t* out_bytes, size_t out_len, int seal, uint32_t* crc_out, int nthreads);
/* The same two on the GPU (gfx950 kernels, frame_build.hip): every pointer device memory, any alignment
 * of d_out_bytes and d_payload, asynchronous on `stream`, nothing allocated per call (scan temporaries and
 * the per-item destination offsets live in the context's per-stream scratch), n and n_items < 2^31 - 1,
 * n == 0 returns UFC_OK whatever the pointers.  With seal != 0 the write is followed, on the same stream, by
 * the variable-length seal of ufc_seal_batch_varlen over (d_out_bytes, d_out_offsets), which treats every
 * span of 4 bytes or more as a frame: give a frame that is to be skipped a length-0 span.  These replace the
 * per-frame assembly of the reference's emitters, src/half_connection/emit.rs:47-125, 170-211 over
 * src/frame/serial/build.rs:55-162, 192-247; packing datagrams into frames (emit.rs:47-112) is the
 * batched pack below, whose records these calls take as they are. */
int ufc_build_sizes_varlen(ufc_ctx* ctx, const ufc_frame_info* d_infos, const ufc_item* d_items, size_t n_items,
                           const uint64_t* d_src_base, size_t payload_len, size_t n, uint64_t* d_out_offsets,
                           uint8_t* d_status, void* stream);
int ufc_build_batch_varlen(ufc_ctx* ctx, const ufc_frame_info* d_infos, const ufc_item* d_items, size_t n_items,
                           const uint64_t* d_src_base, const uint8_t* d_payload, size_t payload_len, size_t n,
                           const uint64_t* d_out_offsets, uint8_t* d_out_bytes, size_t out_len, int seal,
                           uint32_t* d_crc_out, void* stream);

/* ---- batched pack: the emitters' push / finalize, many flushes per call ----
 * A flush is one connection's datagrams (or ack groups) in push order, with the limits its emitter was made
 * with; each flush is cut into frames exactly as DataFrameEmitter / AckFrameEmitter cut it
 * (src/half_connection/emit.rs:47-125, 170-211).  The output is the ufc_frame_info records of the frames,
 * ready for ufc_build_sizes_* / ufc_build_batch_* over the same item array with no step in between.
 *
 * Per flush: alloc = flush_alloc, no frame in progress, frames = 0; H = 10 and at most 127 items per frame
 * for data, H = 15 and no count limit for ack; e = the item's encoded size (a datagram's as
 * DataFrameBuilder::encoded_size, build.rs:172-183, from data_len, the leads and fragment_id_last; an ack
 * group's UFC_ACK_GROUP_SIZE).  For each item in order:
 *   1. with a frame in progress of size s (H + its items): if alloc - s < 0, finalize and stop
 *      SIZE_LIMITED; else if s + e > UFC_MAX_FRAME_SIZE or the frame holds its maximum count, finalize and
 *      go on with 2; else add the item and take the next one;
 *   2. if alloc < 0, stop SIZE_LIMITED;
 *   3. data only: if frames >= window_room, stop WINDOW_LIMITED;
 *   4. start a frame with this item (no size check: a datagram larger than a frame gets a frame of its own).
 * After the last item, finalize.  Finalize: emit the frame, frames += 1, alloc -= s.
 * The pack judges no field value (that stays UFC_BUILD_BAD_FIELD in the build); an ack flush with no groups
 * yields no frame (push_dud is ufc_flush_acks_*, uflow_flush_ctl.h); a kind other than UFC_FRAME_ACK packs as data. */
typedef struct ufc_flush {        /* 24 bytes */
  int64_t  flush_alloc;           /* the emitter's flush_alloc in bytes; may be negative */
  uint32_t kind;                  /* UFC_FRAME_DATA or UFC_FRAME_ACK */
  uint32_t window_room;           /* data: frames the frame queue still takes, window.size - (next_id - base_id);
                                     ack: ignored */
  uint32_t id0;                   /* data: frame_queue.next_id() of the first frame; ack: frame_window_base_id */
  uint32_t id1;                   /* ack: packet_window_base_id */
} ufc_flush;

#define UFC_PACK_DONE 0           /* every item packed */
#define UFC_PACK_SIZE_LIMITED 1   /* DataPushError::SizeLimited / the ack emitter's Err(()) */
#define UFC_PACK_WINDOW_LIMITED 2 /* DataPushError::WindowLimited */
#define UFC_PACK_BAD_RANGE 3      /* the flush's item range is reversed or leaves [0, n_items): nothing packed */
typedef struct ufc_flush_result { /* 24 bytes */
  uint32_t frame_first, frame_count; /* its frames: infos[frame_first .. frame_first + frame_count) */
  uint32_t items_packed;             /* items that went into those frames; the push of the next one failed */
  uint32_t stop;
  int64_t  alloc_left;               /* flush_alloc after the last finalize */
} ufc_flush_result;

/* Flush j owns items[flush_first[j] .. flush_first[j + 1]) (CSR, n_flushes + 1 entries).  Frames come out in flush order and within a flush in emit order:
 * frame_first is the exclusive sum of frame_count, *frames_used the total.  Frames at index >= frames_cap
 * are not written (compare *frames_used with frames_cap, as with the parse's items_cap); frames_cap =
 * n_items is always enough.  Every written info has kind set, ok = 1, crc_ok = 0, item_first and item_count
 * into the same item array (a frame's items are consecutive: nothing is permuted), f[] and aux zero except:
 *   data  f[0] = id0 + k (wrapping) for the flush's k-th frame; aux = bit g % 32 of nonce_bits[g / 32] for the
 *         batch's g-th frame (nonce_bits NULL: 0; else one bit per frame below frames_cap)
 *   ack   f[0] = id0, f[1] = id1
 * n_items and n_flushes < 2^31 - 1; n_flushes == 0 returns UFC_OK whatever the pointers; a NULL flush_first,
 * flushes, results or frames_used, NULL items with n_items != 0, or NULL infos with frames_cap != 0, is
 * UFC_ERR_INVALID_ARG. */
int ufc_pack_host(const ufc_item* items, size_t n_items, const uint64_t* flush_first, const ufc_flush* flushes,
                  size_t n_flushes, const uint32_t* nonce_bits, ufc_frame_info* infos, size_t frames_cap,
                  ufc_flush_result* results, uint64_t* frames_used, int nthreads);
/* The same on the GPU (gfx950 kernels, frame_pack.hip): every pointer device memory, asynchronous on
 * `stream`, nothing allocated per call (the items' size prefix sums, one hop byte per item, two words per
 * flush and the scan temporaries live in the context's per-stream scratch). */
int ufc_pack_varlen(ufc_ctx* ctx, const ufc_item* d_items, size_t n_items, const uint64_t* d_flush_first,
                    const ufc_flush* d_flushes, size_t n_flushes, const uint32_t* d_nonce_bits,
                    ufc_frame_info* d_infos, size_t frames_cap, ufc_flush_result* d_results,
                    uint64_t* d_frames_used, void* stream);

/* ---- batched packet emit: queued packets into datagram items, many senders per call ----
 * The step in front of the pack: PacketSender::emit_packet (src/half_connection/packet_sender.rs:149-238),
 * PendingPacket::new / datagram (pending_packet.rs:23-42, 84-103) and the new-packet loop of emit_data_frames
 * (half_connection/mod.rs:385-427).  A sender is one connection's PacketSender state plus its queued packets
 * in queue order; the output is the ufc_item records of the packets' fragments, ready for ufc_pack_* (with
 * the flush_first this call writes) and ufc_build_* (src_base NULL: data_offset is absolute in the payload
 * arena).
 *
 * Per sender, for the packets i = 0, 1, ... of its range, the first min(take, range) only:
 *   1. channel_id >= 64, mode > 3 or data_len > UFC_MAX_PACKET_SIZE: stop BAD_PACKET at i (what
 *      enqueue_packet debug-asserts, :139-141);
 *   2. mode == TIME_SENSITIVE and packet.flush_id != sender.flush_id: the packet is dropped (:150-162), its
 *      length counted in bytes_dropped; next packet;
 *   3. (next_id - base_id) & 0xFFFFF >= window_size: stop WINDOW_LIMITED (:165-167);
 *   4. a = the packet's alloc_size (:16-22: a length over 1448 rounded up to a multiple of 1448); alloc + a >
 *      max_alloc rounded up to a multiple of 1448 (PacketSender::new, :100; saturating): stop ALLOC_LIMITED
 *      (:169-173);
 *   5. emit: seq = next_id; each parent lead = (seq - parent) & 0xFFFFF truncated to 16 bits as the
 *      reference's `as u16`, 0 without a parent; next_id = (next_id + 1) & 0xFFFFF; alloc += a; a RELIABLE
 *      packet becomes the window parent and its channel's parent; resend = mode >= PERSISTENT; the packet
 *      yields last + 1 items, last = max(ceil(data_len / 1448), 1) - 1, fragment f with data_offset + 1448 f
 *      and 1448 bytes, the last one the rest (an empty packet: one empty datagram).
 * A stopped sender consumes nothing at or after the stopping packet; stale packets in front of it are
 * dropped.  When the range (or take) ends first the stop is DONE.
 *
 * Every item has id = seq, channel_id, the two leads, fragment_id, fragment_id_last, data_offset, data_len,
 * form = the header form DataFrameBuilder::add will choose (build.rs:81-122) and flags = UFC_ITEM_VALID when
 * datagram_is_valid holds (always for consistent sender state; parents the caller made up may break it, which
 * is data, not an error): what the parse gives back for the built frame, data_offset apart. */
#define UFC_SEND_TIME_SENSITIVE 0 /* SendMode order, src/lib.rs:304-323 */
#define UFC_SEND_UNRELIABLE 1
#define UFC_SEND_PERSISTENT 2
#define UFC_SEND_RELIABLE 3
#define UFC_NO_PARENT 0xFFFFFFFFu
#define UFC_MAX_PACKET_SIZE (UFC_MAX_FRAGMENT_SIZE * 65536u) /* MAX_PACKET_SIZE, src/lib.rs:300 */

typedef struct ufc_packet {          /* 16 bytes */
  uint32_t data_offset, data_len;    /* in the payload arena (< 2^32 bytes) */
  uint32_t flush_id;                 /* the flush it was enqueued in */
  uint8_t channel_id, mode;
  uint16_t reserved;
} ufc_packet;

typedef struct ufc_sender {          /* 304 bytes; in and out */
  uint32_t base_id, next_id, window_size, flush_id;
  uint64_t alloc, max_alloc;
  uint32_t window_parent_id;         /* UFC_NO_PARENT = None */
  uint32_t take;                     /* look at the first min(take, range) packets only */
  uint32_t reserve_items;            /* item slots left untouched in front of this sender's new items */
  uint32_t reserved;
  uint32_t channel_parent_id[UFC_MAX_CHANNELS]; /* UFC_NO_PARENT = None */
} ufc_sender;

#define UFC_PACKET_NOT_REACHED 0
#define UFC_PACKET_EMITTED 1
#define UFC_PACKET_DROPPED 2
typedef struct ufc_packet_result {   /* 16 bytes, one per packet; all zero unless emitted or dropped */
  uint32_t sequence_id;              /* emitted packets only, as item_first and item_count */
  uint32_t item_first, item_count;   /* its fragments: items[item_first .. item_first + item_count) */
  uint8_t status;                    /* UFC_PACKET_* */
  uint8_t resend;                    /* emitted: mode >= PERSISTENT (the fragments go to the resend queue) */
  uint16_t reserved;
} ufc_packet_result;

#define UFC_EMIT_DONE 0           /* the range (or take) ended */
#define UFC_EMIT_WINDOW_LIMITED 1 /* the transfer window is full */
#define UFC_EMIT_ALLOC_LIMITED 2  /* the receiver's allocation limit */
#define UFC_EMIT_BAD_PACKET 3     /* a record enqueue_packet would not have taken */
#define UFC_EMIT_BAD_RANGE 4      /* the packet range is reversed or leaves [0, n_packets): nothing done */
typedef struct ufc_sender_result {   /* 32 bytes */
  uint32_t item_first, item_count;   /* its item range, reserved slots included */
  uint32_t packets_consumed;         /* emitted + dropped: the stopping packet's index in the range */
  uint32_t packets_emitted, packets_dropped, stop;
  uint64_t bytes_dropped;
} ufc_sender_result;

/* Sender s owns packets[packet_first[s] .. packet_first[s + 1]) (CSR, n_senders + 1 entries).  Outputs:
 *   items, items_cap   sender s's items at items[flush_first[s] + reserve_items ..), packets in order and
 *                      each packet's fragments in order; items at an index >= items_cap are not written
 *                      (compare *items_used with items_cap, as with the parse; items_cap = 0 gives the records
 *                      and the state alone).  The reserve_items slots in front of a sender's new items are
 *                      never written: ufc_resend_place_* (below) puts the flush's resent and leftover fragments
 *                      there, as the reference sends them first (mod.rs:351-383 before :385).
 *   flush_first        [n_senders + 1], the exclusive sum of the senders' item counts, reserved slots
 *                      included: what ufc_pack_* takes as its flush_first.  *items_used = flush_first[n_senders].
 *   packet_results     [n_packets], nullable.  Every packet of a sender's range gets a record; packets that
 *                      no sender owns are left as they were.
 *   sender_results     [n_senders].
 *   senders_out        [n_senders], nullable, may be `senders` itself: the state after the consumed prefix
 *                      (next_id, alloc, window_parent_id, channel_parent_id updated, everything else copied).
 * A BAD_RANGE sender gets item_count 0 (no reserved slots either), an unchanged state and no packet records.
 * The ranges of the other senders must not overlap (in a CSR they cannot, unless an entry in between is out
 * of order); where they do, the records and items of the packets they share are unspecified.
 * n_packets, n_senders and the item total < 2^31 - 1 (the host call returns UFC_ERR_INVALID_ARG for an item
 * total beyond it, with flush_first and *items_used written; the device call leaves that to the caller);
 * n_senders == 0 returns UFC_OK whatever the pointers; a NULL packet_first, senders, flush_first,
 * sender_results or items_used, NULL packets with n_packets != 0, or NULL items with items_cap != 0, is
 * UFC_ERR_INVALID_ARG. */
int ufc_emit_packets_host(const ufc_packet* packets, size_t n_packets, const uint64_t* packet_first,
                          const ufc_sender* senders, size_t n_senders, ufc_item* items, size_t items_cap,
                          uint64_t* flush_first, ufc_packet_result* packet_results, ufc_sender_result* sender_results,
                          ufc_sender* senders_out, uint64_t* items_used, int nthreads);
/* The same on the GPU (gfx950 kernels, packet_emit.hip): every pointer device memory, asynchronous on
 * `stream`, nothing allocated per call (12 bytes per packet, 8 per sender and the scan temporaries live in
 * the context's per-stream scratch). */
int ufc_emit_packets_varlen(ufc_ctx* ctx, const ufc_packet* d_packets, size_t n_packets,
                            const uint64_t* d_packet_first, const ufc_sender* d_senders, size_t n_senders,
                            ufc_item* d_items, size_t items_cap, uint64_t* d_flush_first,
                            ufc_packet_result* d_packet_results, ufc_sender_result* d_sender_results,
                            ufc_sender* d_senders_out, uint64_t* d_items_used, void* stream);

/* ---- batched packet receive: datagram items into delivered packets, many receivers per call ----
 * The step behind the parse, and the mirror of the emit: PacketReceiver::handle_datagram, receive and
 * resynchronize (src/half_connection/packet_receiver/mod.rs:142-218, 286-402, 408-435), AssemblyWindow::try_add
 * and clear (assembly_window/mod.rs:69-199) and FragmentBuffer (fragment_buffer.rs:12-57).  A receiver is one
 * connection's PacketReceiver state; one call runs one *step* for every receiver:
 *   1. if resync_id != UFC_NO_PARENT: resynchronize(resync_id & 0xFFFFF);
 *   2. handle_datagram for every datagram of the receiver's frames, in frame order and then item order.
 *      Receiver r owns frames [frame_first[r], frame_first[r + 1]) (CSR; the caller groups frames by
 *      connection).  A frame counts when infos[i].ok, kind == UFC_FRAME_DATA and (frame_accept == NULL or
 *      frame_accept[i] != 0): frame_accept is where the frame window's verdict (FrameAckQueue) plugs in.  The
 *      items of a frame with ok != 0 that does not count get UFC_RX_NOT_HANDLED.  Per datagram, in this order:
 *        - datagram_is_valid recomputed from the fields (flags is not trusted), and id < 2^20: else
 *          DROPPED_INVALID;
 *        - its payload is payload[src_base[i] + data_offset ..+ data_len) (src_base NULL: zero, as in the build,
 *          so a parsed batch's offsets and bytes are passed as they are): a range that leaves [0, payload_len)
 *          is DROPPED_BAD_SRC;
 *        - (id - base_id) & 0xFFFFF >= window_size: DROPPED_WINDOW (:162); behind its channel's base:
 *          DROPPED_CHANNEL (:167);
 *        - try_add on slot id & (window_size - 1): an OPEN slot is opened by this datagram (refused by the
 *          allocation limit: DUD, the slot CLOSED with no allocation; one fragment: COMPLETED; else STORED, the
 *          slot ACTIVE); a CLOSED slot: DROPPED_CLOSED; an ACTIVE slot: DROPPED_MISMATCH if channel, either lead
 *          or fragment_id_last differ from the opener's, DROPPED_DUPLICATE if the fragment was already received
 *          (the first arrival's bytes win), else STORED, or COMPLETED when it was the last one missing.
 *      A COMPLETED or DUD datagram enters its packet into the receive window (:177-216).
 *   3. if deliver != 0: receive(): packets go out in sequence order, gated per channel, then the window advances.
 * The item ranges of a batch's frames must not overlap (a parse's never do): where they do, the status of the
 * shared items and what follows from them are unspecified, within every bound.
 * resync_id and deliver let a caller split a batch at a sync frame: a step with deliver = 0 for the datagrams in
 * front of it, then a step with resync_id set for the rest.
 *
 * The release build is the specification: debug asserts are not enforced, and every input has one answer,
 * hostile senders included (a window that passes an undelivered packet leaves a stale receive-window entry
 * behind, exactly as the reference does).  One deliberate difference: a packet refused by the allocation limit
 * (assembly_window/mod.rs:95-105) makes the reference panic when it is delivered (mod.rs:337, unwrap of None);
 * here it is delivered as a record with UFC_RX_PACKET_DUD and length 0, everything else as if sink.send had
 * happened.  channel_base_markers are not stored: a channel base is the id after a delivered packet, its lead
 * over base_id in 1..=window_size, so try_unset_channel_base_id over (base, new_base] unsets exactly the
 * channels whose base lead is in 1..=advance, and that is the rule here whatever the state. */
typedef struct ufc_receiver {        /* 560 bytes; in and out */
  uint32_t base_id, end_id, window_size;
  uint8_t window_ready;              /* window_ready_flag */
  uint8_t deliver;                   /* in: run receive() in this step */
  uint16_t reserved;
  uint32_t resync_id;                /* in: UFC_NO_PARENT = no resynchronize in this step */
  uint32_t reserved2;
  uint64_t alloc, max_alloc;         /* AssemblyWindow's; max_alloc is rounded up to a multiple of 1448 at use
                                        (assembly_window/mod.rs:73), saturating, as the emit does */
  uint64_t channel_ready_flags;
  uint32_t channel_base_id[UFC_MAX_CHANNELS];      /* UFC_NO_PARENT = None */
  uint32_t channel_packet_count[UFC_MAX_CHANNELS];
} ufc_receiver;

/* One window slot (32 bytes): the assembly window's entry and, apart from it, the receive window's (stale
 * receive-window entries outlive a cleared assembly entry in the reference).  All zero = empty.
 * Its bytes live in the carry arena at data_offset: first the held packet's data_len bytes when DATA is set
 * without DUD (a complete packet not yet delivered), then, 8-byte aligned, an ACTIVE slot's FragmentBuffer:
 * n * 1448 data bytes, fragment f at f * 1448, and ceil(n / 64) uint64 received-bits words (bit f % 64 of word
 * f / 64), n = asm_last_fragment_id + 1. */
#define UFC_RX_ASM_OPEN 0
#define UFC_RX_ASM_CLOSED 1
#define UFC_RX_ASM_ACTIVE 2
#define UFC_RX_SLOT_ENTRY 1 /* entry_flags bit */
#define UFC_RX_SLOT_DATA 2  /* data_flags bit */
#define UFC_RX_SLOT_DUD 4   /* with DATA: the packet has no bytes (data = None) */
typedef struct ufc_rx_slot {
  uint64_t data_offset;              /* the slot's region in the carry arena (8-byte aligned) */
  uint32_t data_len;                 /* the held packet's bytes (0 without DATA, or with DUD) */
  uint32_t asm_size;                 /* CLOSED: Closed(alloc_size); ACTIVE: the FragmentBuffer's total_size (its
                                        alloc_size is n * 1448) */
  uint16_t asm_window_parent_lead, asm_channel_parent_lead, asm_last_fragment_id;  /* ACTIVE: the opener's */
  uint16_t asm_received;             /* ACTIVE: fragments received (at most n - 1) */
  uint16_t rx_window_parent_lead, rx_channel_parent_lead; /* window_entries / channel_entries */
  uint8_t asm_state;                 /* UFC_RX_ASM_* */
  uint8_t asm_channel_id;            /* ACTIVE: the opener's */
  uint8_t rx_channel_id;             /* channel_entries */
  uint8_t rx_flags;                  /* UFC_RX_SLOT_ENTRY | _DATA | _DUD */
} ufc_rx_slot;

#define UFC_RX_PACKET_DUD 1
typedef struct ufc_rx_packet {       /* 24 bytes: one delivered packet */
  uint64_t out_offset;               /* its bytes: out_bytes[out_offset ..+ len) */
  uint32_t sequence_id, len;
  uint8_t channel_id;
  uint8_t flags;                     /* UFC_RX_PACKET_DUD: refused by the allocation limit, len 0 */
  uint16_t reserved;
  uint32_t reserved2;
} ufc_rx_packet;

/* item_status values, one byte per datagram. */
#define UFC_RX_NOT_HANDLED 0
#define UFC_RX_STORED 1
#define UFC_RX_COMPLETED 2
#define UFC_RX_DUD 3
#define UFC_RX_DROPPED_INVALID 4
#define UFC_RX_DROPPED_WINDOW 5
#define UFC_RX_DROPPED_CHANNEL 6
#define UFC_RX_DROPPED_CLOSED 7
#define UFC_RX_DROPPED_MISMATCH 8
#define UFC_RX_DROPPED_DUPLICATE 9
#define UFC_RX_DROPPED_BAD_SRC 10
#define UFC_RX_STATUS_COUNT 11

#define UFC_RX_DONE 0
#define UFC_RX_BAD_STATE 1 /* window_size not a power of two in 1..4096; base_id or end_id >= 2^20; the frame range,
                              a counted or ok frame's item range, the slot range (fewer than window_size slots) or a
                              slot's carry region reversed or out of bounds; a slot's channel id >= 64 or asm_state
                              > 2: nothing is done, state and slots stay as they are, no item status is written */
typedef struct ufc_receiver_result { /* 80 bytes */
  uint32_t packet_first, packet_count;            /* its records: packets[packet_first ..+ packet_count) */
  uint32_t status_count[UFC_RX_STATUS_COUNT];     /* datagrams per item_status value */
  uint32_t packets_completed, packets_dud;        /* packets that entered the receive window in this step */
  uint32_t advanced;                              /* ids the window moved, the resynchronize included */
  uint32_t stop;                                  /* UFC_RX_DONE or UFC_RX_BAD_STATE */
  uint32_t reserved;
  uint64_t bytes_delivered;
} ufc_receiver_result;

/* State: receivers[n_receivers] in, receivers_out[n_receivers] out (required; may be `receivers` itself);
 * slot j of receiver r is slots[slot_first[r] + j], j < window_size (slot_first: CSR, n_receivers + 1 entries,
 * inside [0, n_slots)), updated in place.  All-zero slots and a header with base_id = end_id, window_size,
 * max_alloc, resync_id = UFC_NO_PARENT, channel_base_id all UFC_NO_PARENT and the rest zero is
 * PacketReceiver::new.
 * Carry: carry_in[carry_in_len) is const and, like carry_out, 8-byte aligned; carry_out[carry_cap) must not overlap it; the caller swaps them
 * between steps.  carry_out holds every slot's region (above) laid down in receiver order, then slot-index
 * order over all window_size slots, each region 8-byte aligned: carry_first[n_receivers + 1] (CSR) and
 * *carry_used are outputs, the slots' data_offset point into carry_out afterwards.  Bytes of fragments not yet
 * received, and padding, are unspecified.  The layout is part of the ABI: a carry written by the host form is
 * read by the GPU form and the reverse.  Held bytes are copied once per step.
 * Outputs: packets[packets_cap], delivered packets in receiver order, then delivery order; their bytes packed
 * without gaps in out_bytes[out_cap); packet_first[n_receivers + 1] (CSR), *packets_used, *out_used;
 * item_status[n_items] (nullable); results[n_receivers].  Records at an index >= packets_cap and bytes at an
 * offset >= out_cap or carry_cap are not written; the used counts are exact and the state advances all the
 * same (compare the used counts with the caps, as with the parse and the emit): a step whose carry_used exceeds
 * carry_cap has lost held bytes.  Always enough: out_cap = carry_in_len + payload_len; packets_cap = n_items +
 * n_slots; carry_cap = carry_in_len + payload_len + 8 * n_slots + B, where B covers the fragment buffers opened
 * in this step: an ACTIVE slot's region is its whole FragmentBuffer, n * 1448 + 8 * ceil(n / 64) bytes with n =
 * fragment_id_last + 1, however few fragments have arrived, so one first fragment of a 64-fragment packet needs
 * 92 680 bytes.  B = that size summed over the step's datagrams with fragment_id_last != 0, one per (receiver,
 * sequence id); per receiver it is also at most (max_alloc rounded up - alloc) * (1 + 1 / 11584) + 8 *
 * window_size.  A caller that cannot bound B runs the step once on a copy of the state with caps of zero: the used
 * counts are exact whatever the caps (the Python wrappers do this when no caps are given).
 * n_frames, n_items, n_receivers and n_slots < 2^31 - 1; n_receivers == 0 returns UFC_OK whatever the pointers;
 * a NULL infos with n_frames != 0, items with n_items != 0, payload with payload_len != 0, slots with n_slots
 * != 0, carry_in with carry_in_len != 0, carry_out with carry_cap != 0, packets with packets_cap != 0, out_bytes
 * with out_cap != 0, or a NULL frame_first, receivers, receivers_out, slot_first, carry_first, carry_used,
 * packet_first, packets_used, out_used or results is UFC_ERR_INVALID_ARG.  frame_accept, src_base and
 * item_status are nullable. */
int ufc_receive_packets_host(const ufc_frame_info* infos, size_t n_frames, const uint8_t* frame_accept,
                             const ufc_item* items, size_t n_items, const uint64_t* src_base, const uint8_t* payload,
                             size_t payload_len, const uint64_t* frame_first, const ufc_receiver* receivers,
                             size_t n_receivers, ufc_rx_slot* slots, const uint64_t* slot_first, size_t n_slots,
                             const uint8_t* carry_in, size_t carry_in_len, uint8_t* carry_out, size_t carry_cap,
                             uint64_t* carry_first, uint64_t* carry_used, ufc_rx_packet* packets, size_t packets_cap,
                             uint64_t* packet_first, uint64_t* packets_used, uint8_t* out_bytes, size_t out_cap,
                             uint64_t* out_used, uint8_t* item_status, ufc_receiver_result* results,
                             ufc_receiver* receivers_out, int nthreads);
/* The same on the GPU (gfx950 kernels, packet_receive.hip): every pointer device memory, any alignment of
 * d_payload and d_out_bytes (d_carry_in and d_carry_out 8-byte aligned), asynchronous on `stream`, nothing
 * allocated per call.  The context's per-stream scratch holds, in bytes: 48 n_slots (a plan record per slot) +
 * 24 (n_items + 2 n_slots) (a copy segment per datagram and two per slot) + 8 (2 n_slots + 1) (a chunk count and
 * its prefix per slot segment) + 2 n_items (a status and a verdict byte) + 8 * the power of two at or above 2 n_items, at least 64
 * (the duplicate table) + 48 (n_receivers + 1) (six counts per receiver) + the scan temporaries, each part
 * rounded up to 256.  n_slots < 2^30 - 1 here. */
int ufc_receive_packets_varlen(ufc_ctx* ctx, const ufc_frame_info* d_infos, size_t n_frames,
                               const uint8_t* d_frame_accept, const ufc_item* d_items, size_t n_items,
                               const uint64_t* d_src_base, const uint8_t* d_payload, size_t payload_len,
                               const uint64_t* d_frame_first, const ufc_receiver* d_receivers, size_t n_receivers,
                               ufc_rx_slot* d_slots, const uint64_t* d_slot_first, size_t n_slots,
                               const uint8_t* d_carry_in, size_t carry_in_len, uint8_t* d_carry_out, size_t carry_cap,
                               uint64_t* d_carry_first, uint64_t* d_carry_used, ufc_rx_packet* d_packets,
                               size_t packets_cap, uint64_t* d_packet_first, uint64_t* d_packets_used,
                               uint8_t* d_out_bytes, size_t out_cap, uint64_t* d_out_used, uint8_t* d_item_status,
                               ufc_receiver_result* d_results, ufc_receiver* d_receivers_out, void* stream);

/* ---- batched frame window: accept verdicts and ack groups, many connections per call ----
 * The step between the parse and the receive, and the source of the ack flushes the pack takes: FrameAckQueue
 * (src/half_connection/frame_ack_queue.rs, whole file) as handle_data_frame and handle_sync_frame drive it
 * (src/half_connection/mod.rs:132-152).  The release build is the specification, wrapping u32 arithmetic
 * included.  A window is one connection's state: the ReceiveWindow (base_id, size), the last entry of the
 * deque of pending ack groups (the only entry mark_seen ever reads or changes) and sync_reply.  One call runs
 * every connection's frames, in arrival order:
 *   data frame (ok, kind == UFC_FRAME_DATA; id = f[0], nonce = aux & 1):
 *     if (id - base_id) < size (wrapping) it is accepted and base_id = id + 1; then, with a tail and
 *     bit = id - tail_base_id < 32: if that bit of tail_bitfield is clear it is set and tail_nonce ^= nonce (a set
 *     bit changes nothing: the rule is kept literal although consistent states never meet it); otherwise the
 *     tail is closed and (id, 1, nonce) is the new tail.  A frame that is not accepted changes nothing;
 *   sync frame (ok, kind == UFC_FRAME_SYNC): if aux bit 0 (next_frame_id = f[0] present), d = f[0] - base_id
 *     (wrapping), and 0 < d <= size: base_id = f[0].  next_packet_id (aux bit 1) belongs to the packet receiver:
 *     ufc_receive_packets_* takes it as resync_id.  sync_reply is set whatever aux holds;
 *   every other kind, and every frame with ok == 0: no effect. */
typedef struct ufc_frame_window {      /* 24 bytes; in and out */
  uint32_t base_id, size;              /* ReceiveWindow */
  uint32_t tail_base_id, tail_bitfield;/* the last pending ack group, if has_tail */
  uint8_t  tail_nonce, has_tail, sync_reply, reserved;
  uint32_t reserved2;
} ufc_frame_window;

#define UFC_FW_DONE 0
#define UFC_FW_BAD_STATE 1  /* size > 2^31, or the frame range reversed or outside [0, n_frames): nothing done,
                               state copied through, its frames' frame_accept written 0 only where the range is usable */
typedef struct ufc_frame_window_result { /* 40 bytes */
  uint32_t group_first, group_count;   /* its groups: groups[group_first ..+ group_count) */
  uint32_t accepted, refused;          /* ok data frames inside / outside the window */
  uint32_t syncs, packet_syncs;        /* ok sync frames; those with next_packet_id present */
  uint32_t first_packet_sync;          /* frame index of the first of those, UFC_NO_PARENT if none: where the caller
                                          splits the receive step (resync_id / deliver) */
  uint32_t advanced;                   /* ids base_id moved in this step (wrapping sum) */
  uint32_t stop, reserved;
} ufc_frame_window_result;

/* Connection r owns frames [frame_first[r], frame_first[r + 1]) (CSR, n_windows + 1 entries) in arrival order: the
 * CSR the receive takes, so one grouping serves both calls.  Outputs:
 *   frame_accept[n_frames]  written for every frame of every usable range: 1 exactly for accepted data frames, 0 for
 *                      everything else, so that it is passed to ufc_receive_packets_* unchanged.  Frames outside
 *                      every range are not touched.
 *   groups, groups_cap ufc_item records in the ack-group form of the parse and the pack: form = 3, id = base_id,
 *                      channel_id = nonce (0/1), data_offset = bitfield, everything else 0.  For connection r the
 *                      carried tail comes first if has_tail != 0, as updated, and is written even when unchanged;
 *                      the groups opened in this step follow in order.  Groups at an index >= groups_cap are not
 *                      written; *groups_used is exact and the state advances all the same (compare, as with the
 *                      parse).  groups_cap = n_windows + n_frames is always enough.
 *   group_first        [n_windows + 1], the exclusive sum of the connections' group counts: directly the
 *                      flush_first of ufc_pack_* (an ack flush per connection: kind = UFC_FRAME_ACK, id0 = the new
 *                      base_id, id1 = the packet receiver's base_id).  *groups_used = group_first[n_windows].
 *   results            [n_windows].  A BAD_STATE connection has no groups, zero counts and first_packet_sync =
 *                      UFC_NO_PARENT.
 *   windows_out        [n_windows], required, may be `windows` itself: the new base_id; the tail = the connection's
 *                      last output group, with has_tail = 1 if any group came out (else has_tail = 0 and the tail
 *                      fields as they came); sync_reply = the input OR'd with 1 if the range holds an ok sync frame;
 *                      size and the reserved fields copied.  tail_nonce is read as tail_nonce & 1.
 * A flush that sent every group clears has_tail: the reference's empty deque then opens a new group even
 * within 32 ids of the old one.  After a SIZE_LIMITED ack flush the unpacked groups are kept and the tail is left
 * as it is.  ufc_flush_acks_* (uflow_flush_ctl.h) does both, and clears sync_reply.  Any 24 bytes are a state, and
 * every input has one answer (size <= 2^31 is what makes the ids of one group strictly increasing, so that the
 * answer does not depend on the order in which a tile's lanes meet).  Ranges of different connections must not
 * overlap; where they do, the frame_accept of the shared frames is unspecified.
 * n_frames and n_windows < 2^31 - 1; n_windows == 0 returns UFC_OK whatever the pointers; a NULL infos with
 * n_frames != 0, groups with groups_cap != 0, or a NULL frame_first, windows, windows_out, frame_accept, group_first,
 * groups_used or results is UFC_ERR_INVALID_ARG. */
int ufc_frame_window_host(const ufc_frame_info* infos, size_t n_frames, const uint64_t* frame_first,
                          const ufc_frame_window* windows, size_t n_windows, uint8_t* frame_accept,
                          ufc_item* groups, size_t groups_cap, uint64_t* group_first, uint64_t* groups_used,
                          ufc_frame_window_result* results, ufc_frame_window* windows_out, int nthreads);
/* The same on the GPU (gfx950 kernels, frame_window.hip): every pointer device memory, asynchronous on `stream`,
 * nothing allocated per call.  One wave walks a connection in tiles of 64 frames, twice: once for the group
 * counts, and after their exclusive sum once more to write.  The context's per-stream scratch holds, in bytes:
 * 8 (n_windows + 1) (a group count per connection) + the scan's temporaries, each part rounded up to 256. */
int ufc_frame_window_varlen(ufc_ctx* ctx, const ufc_frame_info* d_infos, size_t n_frames, const uint64_t* d_frame_first,
                            const ufc_frame_window* d_windows, size_t n_windows, uint8_t* d_frame_accept,
                            ufc_item* d_groups, size_t groups_cap, uint64_t* d_group_first, uint64_t* d_groups_used,
                            ufc_frame_window_result* d_results, ufc_frame_window* d_windows_out, void* stream);

/* ---- batched sender frame queue: received acks into acked fragments, the transfer window and feedback ----
 * The step behind the parse on the sender's side: FrameQueue (src/half_connection/frame_queue.rs:209-388) with its
 * FrameLog (:24-84) and FeedbackGen (:96-195), ReorderBuffer (reorder_buffer.rs:2-179, whole file) and
 * LossIntervalQueue (loss_rate.rs:19-110, whole file), as HalfConnection::handle_ack_frame, step and the emitters
 * drive it.  The release build is the specification, wrapping u32 and u64 arithmetic included (send_time_ms +
 * rtt_ms, now_ms - last_send_time_ms and total_ack_size all wrap).  SendRateComp (send_rate.rs, recv_rate_set.rs)
 * is ufc_rate_begin_* / ufc_rate_step_* below; PacketSender::acknowledge (it needs the per-packet window table that
 * ufc_sender does not hold) and the resend and pending queues are ufc_resend_* further below.
 *
 * A log slot is one frame_queue::Entry (:14-21).  fragment_refs is the range [ref_first, ref_first + ref_count) of a
 * fragment table the caller owns: in the device pipeline the connection's transmission ring, which
 * ufc_resend_commit_* fills and whose marks ufc_resend_begin_* consumes. */
#define UFC_SENT_NONCE 1         /* Entry.nonce */
#define UFC_SENT_RATE_LIMITED 2  /* Entry.rate_limited; ignored on input to a push */
#define UFC_SENT_ACKED 4         /* Entry.acked; ignored on input to a push */
#define UFC_SENT_MARK 8          /* input to a push only: mark_rate_limited() (:240) was called since the push before */
typedef struct ufc_sent_frame {        /* 24 bytes */
  uint64_t send_time_ms;
  uint32_t size;
  uint32_t ref_first, ref_count;
  uint8_t flags;                       /* UFC_SENT_* */
  uint8_t reserved[3];                 /* stored as 0 */
} ufc_sent_frame;

/* One connection's FrameQueue, in and out.  Frame `id` of the log lives at log[log_first + (id & (log_cap - 1))],
 * a ring in the caller's log arena; the rings of different connections must not overlap. */
typedef struct ufc_frame_queue {       /* 192 bytes */
  uint32_t log_base_id, log_next_id;   /* FrameLog (:24-28); its length is log_next_id - log_base_id */
  uint32_t window_base_id, window_size, tail_size;  /* TransferWindow (:197-201) */
  uint32_t rb_base_id, rb_max_span, rb_frames[2], rb_count;  /* ReorderBuffer (reorder_buffer.rs:2-7) */
  uint8_t rate_limited;                /* FrameQueue.rate_limited (:214): the pending mark */
  uint8_t has_ack_data;                /* FeedbackGen.ack_data is Some (:101) */
  uint8_t ack_rate_limited;            /* AckData.rate_limited */
  uint8_t has_last_feedback;           /* FeedbackGen.last_feedback_ms is Some (:98) */
  uint32_t li_count;                   /* LossIntervalQueue.entries.len(), 0..9 */
  uint64_t ack_last_send_time_ms, ack_total_size;  /* AckData (:90-94); 0 when has_ack_data is 0 on output */
  uint64_t last_feedback_ms;
  uint64_t li_end_time_ms[9];          /* front (the latest interval) first; entries at li_count and beyond are
                                          ignored on input and written 0 */
  uint32_t li_length[9];
  uint32_t log_cap;                    /* a power of two, >= window_size + tail_size */
  uint64_t log_first;
} ufc_frame_queue;

#define UFC_FQ_HAS_RTT 1            /* rtt_ms is Some; otherwise FeedbackGen::INITIAL_RTT_MS = 100 is used (:111, :170) */
#define UFC_FQ_RESET_LOSS 2         /* reset_loss_rate(reset_loss_rate) first */
#define UFC_FQ_MARK_RATE_LIMITED 4  /* mark_rate_limited() behind the pushes */
#define UFC_FQ_FORGET 8             /* forget_frames(thresh_ms, rtt) behind the ack frames */
#define UFC_FQ_FEEDBACK 16          /* get_feedback(now_ms) last */
typedef struct ufc_frame_queue_step {  /* 40 bytes: what to do for one connection in this call */
  uint32_t flags, reserved;
  uint64_t rtt_ms;                     /* the Option<u64> handle_ack_frame and forget_frames pass, constant through the
                                          call as it is between two step()s of the reference */
  uint64_t thresh_ms, now_ms;
  double reset_loss_rate;
} ufc_frame_queue_step;

#define UFC_FQ_DONE 0
#define UFC_FQ_BAD_STATE 1
typedef struct ufc_frame_queue_result { /* 80 bytes */
  uint32_t stop;
  uint32_t pushes_taken, pushes_refused;
  uint32_t ack_frames, groups;         /* ok ack frames; their groups */
  uint32_t groups_dud, groups_unknown, groups_bad_nonce;  /* acknowledge_group's three silent returns */
  uint32_t frames_acked;               /* log entries newly acked */
  uint32_t li_acks, li_nacks;          /* push_ack / push_nack calls */
  uint32_t window_advanced, log_culled;/* ids the transfer window's and the log's base moved (wrapping sums) */
  uint32_t window_room;                /* window_size - (log_next_id - window_base_id) if positive, else 0: the pack's
                                          ufc_flush.window_room, with id0 = log_next_id */
  uint8_t has_feedback, rate_limited;  /* get_feedback returned Some; FeedbackData.rate_limited */
  uint16_t reserved;
  uint32_t receive_rate;
  uint64_t rtt_ms;
  double loss_rate;
} ufc_frame_queue_result;

/* One call runs one step for every connection c, in this order:
 *   1. UFC_FQ_RESET_LOSS: LossIntervalQueue::reset (loss_rate.rs:33-54): the queue is truncated to its front entry,
 *      whose length becomes (1.0 / p).clamp(0, u32::MAX).round() as u32 (half away from zero, NaN gives 0).
 *   2. FrameQueue::push (:244-259) for sent[sent_first[c] .. sent_first[c + 1]) in order: while (log_next_id -
 *      window_base_id) < window_size (can_push, :228) the record is stored with ACKED clear, NONCE as given,
 *      RATE_LIMITED = the pending mark OR the record's MARK, reserved 0; the pending mark is cleared and log_next_id
 *      += 1.  The window does not move during pushes, so the refused records are a suffix; they are only counted.
 *      Then UFC_FQ_MARK_RATE_LIMITED sets the pending mark.
 *   3. The frames infos[frame_first[c] .. frame_first[c + 1]) in arrival order (the CSR the frame window and the
 *      receive take).  A frame with ok and kind == UFC_FRAME_ACK: each of its groups items[item_first ..+ item_count)
 *      goes through acknowledge_group (:279-355) with base_id = id, bitfield = data_offset, nonce = channel_id & 1;
 *      then advance_transfer_window(f[0], rtt) (:357-380, cull_log_entries :382-387, notify_advancement :179-194).
 *      Every other frame has no effect.  acknowledge_group is literal: a bitfield of 0 is a dud (:294); a group
 *      with an id outside the log returns (:307); a nonce that is not the XOR of the claimed frames' returns (:313);
 *      rate_limited is OR-ed over every frame of the span, acked or not (:323); a frame newly acked gets ACKED, its
 *      size and send time enter the AckData, notify_ack (:159-177) runs, and ref_acked[ref_first ..+ ref_count) is
 *      set to 1 where the index is below refs_cap (the batched acknowledge_fragment; ref_acked is nullable and is
 *      never written 0); put_ack_data (:149-157) runs even when no frame was newly acked.  notify_ack's old-frame
 *      branch does nothing (:173-176).
 *   4. UFC_FQ_FORGET: forget_frames(thresh_ms, rtt) (:261-269, find_expiration_cutoff :67-77).
 *   5. UFC_FQ_FEEDBACK: get_feedback(now_ms) (:126-147).  receive_rate = (total_ack_size as f64 / ((now_ms -
 *      last_feedback_ms) as f64 / 1000.0)).clamp(0, u32::MAX) as u32 with Rust's casts: a difference of 0 gives
 *      u32::MAX, 0 / 0 gives NaN and so 0, and 0 without an earlier feedback.  loss_rate = compute_loss_rate
 *      (loss_rate.rs:86-109), the sums in the reference's order and never fused, so host and device agree in
 *      every bit.
 * queues_out[c] (required, may be `queues` itself) gets the new state; the log rings are updated in place.
 *
 * The reference unwrap()s and indexes without checks, so a state is checked first.  A connection stops
 * UFC_FQ_BAD_STATE, its state copied through, its result zero but for `stop`, its ring and ref_acked untouched, when:
 *   - log_cap is not a power of two, log_cap < window_size + tail_size, or the ring [log_first, log_first + log_cap)
 *     leaves [0, n_log);
 *   - log_next_id - log_base_id > log_cap;
 *   - log_next_id - window_base_id > window_size, or log_next_id - log_base_id > (log_next_id - window_base_id) +
 *     tail_size (all wrapping): the log then starts more than tail_size behind the window.  push and
 *     advance_transfer_window keep both true from FrameQueue::new on; without them a push would outgrow the ring;
 *   - rb_max_span < window_size + tail_size or rb_max_span > 2^31 (FrameQueue::new sets it to the sum, :221);
 *   - rb_base_id - log_base_id > log_next_id - log_base_id;
 *   - rb_count > 2; a reorder-buffer frame not strictly after rb_base_id, or not inside the log: with d = frame -
 *     rb_base_id, d == 0 or (rb_base_id - log_base_id) + d >= the log's length; two frames out of order (d0 >= d1);
 *   - li_count > 9; UFC_FQ_RESET_LOSS with li_count == 0 (the reference indexes entries[0], loss_rate.rs:53);
 *   - the frame or the sent range reversed or outside its array; an ok ack frame's item range outside [0, n_items).
 * A state that passes never reaches a failing unwrap or index of the reference, and the state that comes out
 * passes again unless a reorder-buffer frame was acked a second time.  The reasoning: with L = the log's length,
 * the rules give L <= window_size + tail_size <= rb_max_span <= 2^31 and keep it so (a push needs log_next_id -
 * window_base_id < window_size; an advance culls to window_base_id - tail_size whenever that lies ahead).
 * acknowledge_group unwraps only ids its first loop found (:302, :321).  notify_ack puts only ids inside the log:
 * one at or ahead of rb_base_id passes can_put since its distance is below L, one behind it is at a wrapped
 * distance of at least 2^32 - 2^31 and does not.  put and advance call back for rb_base_id up to the nearest of
 * the new id and the held frames, or up to the new log base, and then for held frames: all at or ahead of
 * rb_base_id and inside the log (:165, :185).  A cull's new base lies within L of log_base_id, so it is either at or
 * behind rb_base_id (can_advance fails at distance 0 or >= 2^31 + 1, and rb_base_id stays inside the log) or ahead of
 * it by at most L <= rb_max_span (can_advance holds, and rb_base_id ends at or ahead of it); drain (:79-83) gets
 * at most L.  A frame held twice (acked again from a state that held it unacked) stays behind as a stale entry at
 * a wrapped distance no put or advance ever selects.
 * Counts: n_frames, n_items, n_sent, n_queues < 2^31 - 1; n_queues == 0 returns UFC_OK whatever the pointers; a NULL
 * infos with n_frames != 0, items with n_items != 0, sent with n_sent != 0, log with n_log != 0, or a NULL
 * frame_first, sent_first, queues, steps, results or queues_out is UFC_ERR_INVALID_ARG.  ref_acked is nullable. */
int ufc_frame_queue_host(const ufc_frame_info* infos, size_t n_frames, const ufc_item* items, size_t n_items,
                         const uint64_t* frame_first, const ufc_sent_frame* sent, size_t n_sent,
                         const uint64_t* sent_first, const ufc_frame_queue* queues, const ufc_frame_queue_step* steps,
                         size_t n_queues, ufc_sent_frame* log, size_t n_log, uint8_t* ref_acked, size_t refs_cap,
                         ufc_frame_queue_result* results, ufc_frame_queue* queues_out, int nthreads);
/* The same on the GPU (gfx950 kernel, frame_queue.hip): every pointer device memory, asynchronous on `stream`,
 * nothing allocated per call.  One wave per connection and one launch: no output needs a scan.  Per-stream
 * scratch: none (0 bytes); the wave's working set is about 2 KiB of LDS. */
int ufc_frame_queue_varlen(ufc_ctx* ctx, const ufc_frame_info* d_infos, size_t n_frames, const ufc_item* d_items,
                           size_t n_items, const uint64_t* d_frame_first, const ufc_sent_frame* d_sent, size_t n_sent,
                           const uint64_t* d_sent_first, const ufc_frame_queue* d_queues,
                           const ufc_frame_queue_step* d_steps, size_t n_queues, ufc_sent_frame* d_log, size_t n_log,
                           uint8_t* d_ref_acked, size_t refs_cap, ufc_frame_queue_result* d_results,
                           ufc_frame_queue* d_queues_out, void* stream);

/* ---- batched send rate control: the TFRC step and the flush allocation ----
 * The two steps around the frame queue call that close a tick on the sender's side: SendRateComp
 * (src/half_connection/send_rate.rs, whole file) with its RecvRateSet (recv_rate_set.rs, whole file), as
 * HalfConnection::step (half_connection/mod.rs:165-193), fill_flush_alloc (:200-215) and the notify_frame_sent call
 * of emit_data_frames (:342-347) drive them.  The release build is the specification: u32 and u64 arithmetic wraps
 * (2*send_rate, 2*recover_rate, now_ms + 2000, now_ms - time_last_doubled_ms, now_ms - e.timestamp_ms, 2*rtt_ms,
 * rtt_ms*4, now_ms + s_to_ms(rto)), saturating_mul / saturating_sub / saturating_add apply where the reference
 * writes them, `as u32` / `as u64` / `as isize` on a float saturate with NaN giving 0, f64::round is half away from
 * zero, f64::max returns the other operand for a NaN, and debug_assert!s do not exist.  MSS = UFC_MAX_FRAME_SIZE,
 * MINIMUM_RATE = MSS / 64 = 23, INITIAL_TCP_WINDOW = 4380.  PacketSender::acknowledge and the resend and pending
 * queues are ufc_resend_* below; the sync frame's decision and push_dud are ufc_flush_sync_* and ufc_flush_acks_*
 * (uflow_flush_ctl.h).
 *
 * A tick of a device-resident sender is queued calls with no host code between them:
 *   ufc_rate_begin_varlen -> ufc_frame_queue_varlen -> ufc_rate_step_varlen -> (emit) -> ufc_pack_varlen,
 * the rate step writing the coming flush's flush_alloc and reading the last flush's alloc_left; with resends and
 * leftover fragments the ufc_resend_* calls go around the emit and the pack (their section has the full order). */
typedef struct ufc_recv_rate_entry {   /* 16 bytes: one RecvEntry (recv_rate_set.rs:3-7) */
  uint64_t timestamp_ms;
  uint32_t value;
  uint8_t is_initial;
  uint8_t reserved[3];                 /* stored as 0 */
} ufc_recv_rate_entry;

#define UFC_RATE_AWAIT_SEND 0
#define UFC_RATE_SLOW_START 1
#define UFC_RATE_THROUGHPUT_EQN 2
/* One connection's SendRateComp (send_rate.rs:83-108) and the HalfConnection fields that go with it, in and out.
 * Its RecvRateSet is entries[recv_first .. recv_first + recv_count) in Vec order, inside the room
 * [recv_first, recv_first + recv_cap) of the caller's entry arena; the rooms of different connections must not
 * overlap.  A has_* byte is an Option's Some bit: nonzero on input means Some, it is written 0 or 1, and a value
 * whose bit is 0 is ignored on input and written 0 (so are time_last_doubled_ms outside SLOW_START and
 * send_rate_tcp outside THROUGHPUT_EQN). */
typedef struct ufc_rate_state {        /* 112 bytes */
  uint32_t mode;                       /* UFC_RATE_* */
  uint32_t send_rate, max_send_rate;
  uint32_t send_rate_tcp;              /* ThroughputEqnState */
  uint8_t has_time_last_doubled;       /* SlowStartState.time_last_doubled_ms is Some */
  uint8_t has_nofeedback_exp;
  uint8_t nofeedback_idle;
  uint8_t has_rtt_s, has_rtt_ms, has_rto_ms;
  uint8_t has_last_flush;              /* HalfConnection.time_last_flushed is Some */
  uint8_t has_reset;                   /* a reset_loss_rate(reset_loss_rate) is pending for the next frame queue call */
  uint64_t time_last_doubled_ms;
  double prev_loss_rate;
  uint64_t nofeedback_exp_ms;
  double rtt_s;
  uint64_t rtt_ms, rto_ms;
  uint64_t now_ms;                     /* HalfConnection.now_ms: the time the next flush stamps on its frames */
  int64_t flush_alloc;                 /* HalfConnection.flush_alloc */
  double reset_loss_rate;
  uint64_t recv_first;
  uint32_t recv_count, recv_cap;
} ufc_rate_state;

#define UFC_RATE_FRAME_SENT 1          /* the last flush emitted at least one data frame (notify_frame_sent) */
typedef struct ufc_rate_tick {         /* 32 bytes: one connection's input to ufc_rate_step_* */
  uint64_t now_ms;
  double delta_time_s;                 /* (now - time_last_flushed).as_secs_f64(); ignored without has_last_flush */
  int64_t alloc_adjust;                /* added (wrapping) to flush_alloc first: bytes spent on frames the pack did
                                          not see, such as the sync frame, as a negative number */
  uint32_t flags, reserved;            /* UFC_RATE_FRAME_SENT */
} ufc_rate_tick;

#define UFC_RATE_DONE 0
#define UFC_RATE_BAD_STATE 1
#define UFC_RATE_REF_PANIC 2           /* the reference panics here: rate_limited_update emptied the set */
#define UFC_RATE_RECV_FULL 3           /* the set would outgrow recv_cap */
#define UFC_RATE_FEEDBACK 1            /* result flags: handle_feedback ran */
#define UFC_RATE_NOFEEDBACK 2          /*   nofeedback_expired ran */
#define UFC_RATE_RESET_ISSUED 4        /*   reset_loss_rate was called: has_reset is set in states_out */
#define UFC_RATE_ENTERED_EQN 8         /*   SLOW_START became THROUGHPUT_EQN */
#define UFC_RATE_INV_STALLED 16        /*   the bisection stopped by the stall rule below */
typedef struct ufc_rate_result {       /* 56 bytes */
  uint32_t stop, mode;                 /* mode after the step */
  uint64_t now_ms;                     /* the three values the coming flush uses (mod.rs:173-175, :197): */
  uint64_t rtt_ms, rto_ms;             /*   rtt_ms().unwrap_or(150) and rto_ms().unwrap_or(600) before the rate step */
  int64_t flush_alloc;                 /* after the fill */
  uint32_t send_rate;                  /* after the step */
  uint32_t flags;                      /* UFC_RATE_FEEDBACK .. UFC_RATE_INV_STALLED */
  uint32_t inv_iterations;             /* eval_tcp_throughput calls of the bisection, 0 when it did not run */
  uint32_t recv_count;
} ufc_rate_result;

/* ufc_rate_begin_*: opens a tick, in front of ufc_frame_queue_*.  For every connection c it writes steps[c]:
 *   flags = UFC_FQ_FORGET | UFC_FQ_FEEDBACK | (has_rtt_ms ? UFC_FQ_HAS_RTT : 0) | (has_reset ? UFC_FQ_RESET_LOSS : 0)
 *           | extra_flags[c] (nullable; the caller's UFC_FQ_MARK_RATE_LIMITED, emit.rs:67 and :85);
 *   rtt_ms = the state's rtt_ms or 0 for None; thresh_ms = now_ms.saturating_sub(rtt_ms.unwrap_or(150) * 4), the
 *   product wrapping (mod.rs:178); now_ms = now_ms[c]; reset_loss_rate = the pending value, or 0; reserved 0.
 * states_out[c] (required, may be `states`) is the state with has_reset and reset_loss_rate cleared and nothing
 * else changed, not even canonicalised.  The pending flag is equivalent to the reference's immediate callback: the
 * reference resets the loss intervals inside step(), before any later ack, and the frame queue call applies
 * UFC_FQ_RESET_LOSS first of all, so a reset issued in tick T and carried to tick T+1's call sees the same sequence
 * of operations.  No state is judged here.
 *
 * ufc_rate_step_*: closes the tick, behind ufc_frame_queue_*.  fq[c] is that call's result for the connection
 * (has_feedback, rtt_ms, receive_rate, loss_rate and rate_limited are read).  Per connection, in this order:
 *   1. Accounting of the last flush.  With flush_results != NULL and i = result_index[c] < n_flush_results:
 *      flush_alloc = flush_results[i].alloc_left, and frame_count > 0 counts as UFC_RATE_FRAME_SENT.  An index at or
 *      beyond n_flush_results (UFC_NO_PARENT is one) means no gather.  Then flush_alloc += alloc_adjust, wrapping.
 *      If a frame was sent, notify_frame_sent(state.now_ms) (send_rate.rs:155-168): AWAIT_SEND becomes SLOW_START
 *      with nofeedback_exp_ms = now_ms + 2000 and the set reset to its initial entry (u32::MAX); nofeedback_idle = 0.
 *   2. state.now_ms = tick.now_ms; the result's rtt_ms and rto_ms are taken, with their defaults.
 *   3. fill_flush_alloc with send_rate and rtt_s as they are now: new_bytes = (send_rate as f64 *
 *      delta_time_s).round() as isize, alloc_max = (send_rate as f64 * rtt_s.unwrap_or(0.0)).round() as isize,
 *      flush_alloc = flush_alloc.saturating_add(new_bytes).min(alloc_max); without has_last_flush only
 *      has_last_flush is set.
 *   4. SendRateComp::step(now_ms, feedback, reset) (:170-185) literally: nothing in AWAIT_SEND; handle_feedback
 *      (:187-284) if fq[c].has_feedback; else nofeedback_expired (:286-365) if the timer is set and now_ms has
 *      reached it.  reset_loss_rate(initial_p) sets has_reset and reset_loss_rate.
 *   5. results[c], states_out[c] (required, may be `states`), the set updated in place, and with flushes != NULL
 *      and j = flush_index[c] < n_flushes: flushes[j].flush_alloc = the new flush_alloc, no other field touched.
 *      Two connections must not name the same flush.
 *
 * Where the reference does not return, the batched call gives an answer:
 *   - eval_tcp_throughput_inv (:30-59) spins for ever when the target lies more than delta below
 *     eval_tcp_throughput(rtt, 1.0): the midpoint reaches 1.0 after 54 halvings and stays (rtt 0.01 s with target 5,
 *     rtt 0.05 s with target 11; a small max_send_rate or a small receive limit in front of send_rate/2 gets
 *     there).  The rule: when a new midpoint equals a or b bit for bit and no return condition holds, that
 *     midpoint is returned and UFC_RATE_INV_STALLED set.  Every interval step moves a or b to a new double
 *     strictly between them, so the loop ends after at most about 1,100 evaluations (a target no rate reaches walks
 *     b down through the denormals).
 *   - rate_limited_update (recv_rate_set.rs:55-65) can empty the set, and max() then unwraps None: an updated
 *     rtt_ms of 0 (a loopback RTT below 0.5 ms) makes 2 * rtt_ms zero, and no entry is younger than that.  The
 *     connection stops UFC_RATE_REF_PANIC.
 *   - The reference's Vec has no bound (feedback at every tick that saw an ack keeps about 2 * rtt / tick entries).
 *     Here the entries are retained first and the new one appended; if more than recv_cap survive, the connection
 *     stops UFC_RATE_RECV_FULL.
 *   - UFC_RATE_BAD_STATE for: mode > 2; recv_cap == 0; recv_count > recv_cap; the room outside [0, n_entries);
 *     mode != AWAIT_SEND with recv_count == 0; mode == THROUGHPUT_EQN without has_rtt_s (the unwrap at :340).
 * A stopped connection changes nothing: states_out[c] is the input state byte for byte, its entries and its flush
 * are untouched, and its result is zero but for `stop` (the step works on a copy and commits at the end).
 * A state that passes never reaches an unwrap or panic of the reference other than the REF_PANIC one: max()
 * (:79-87) is called by replace_max only behind its is_empty test, by rate_limited_update (REF_PANIC), and by
 * nofeedback_expired in THROUGHPUT_EQN on a set the rules keep non-empty; rtt_s.unwrap() (:340) has its rule; the
 * two `_ => panic!()` arms (:276, :354) stand behind the AWAIT_SEND return of step().  Every stop copies the state
 * through, so each leaves a passing state passing, and UFC_RATE_DONE does too: every set update ends with at least
 * one entry and at most recv_cap, and THROUGHPUT_EQN is entered only by handle_feedback, which sets rtt_s.
 *
 * Floats: every operation is an IEEE double operation in the reference's order, never fused; sqrt is correctly
 * rounded on both sides, so host and device agree in every bit.
 * Counts: n < 2^31 - 1; n == 0 returns UFC_OK whatever the pointers; a NULL states, now_ms / ticks, fq, steps /
 * results or states_out, a NULL entries with n_entries != 0, a NULL result_index with flush_results, or a NULL
 * flush_index with flushes is UFC_ERR_INVALID_ARG. */
int ufc_rate_begin_host(const ufc_rate_state* states, const uint64_t* now_ms, const uint32_t* extra_flags, size_t n,
                        ufc_frame_queue_step* steps, ufc_rate_state* states_out, int nthreads);
int ufc_rate_step_host(const ufc_rate_state* states, const ufc_rate_tick* ticks, const ufc_frame_queue_result* fq,
                       size_t n, ufc_recv_rate_entry* entries, size_t n_entries, const ufc_flush_result* flush_results,
                       size_t n_flush_results, const uint32_t* result_index, ufc_flush* flushes, size_t n_flushes,
                       const uint32_t* flush_index, ufc_rate_result* results, ufc_rate_state* states_out, int nthreads);
/* The same on the GPU (gfx950 kernels, send_rate.hip): every pointer device memory, asynchronous on `stream`,
 * nothing allocated per call, no scratch.  One lane per connection; a wave moves its 64 states, ticks and frame
 * queue results through 15 KiB of LDS with coalesced loads and stores. */
int ufc_rate_begin_varlen(ufc_ctx* ctx, const ufc_rate_state* d_states, const uint64_t* d_now_ms,
                          const uint32_t* d_extra_flags, size_t n, ufc_frame_queue_step* d_steps,
                          ufc_rate_state* d_states_out, void* stream);
int ufc_rate_step_varlen(ufc_ctx* ctx, const ufc_rate_state* d_states, const ufc_rate_tick* d_ticks,
                         const ufc_frame_queue_result* d_fq, size_t n, ufc_recv_rate_entry* d_entries, size_t n_entries,
                         const ufc_flush_result* d_flush_results, size_t n_flush_results, const uint32_t* d_result_index,
                         ufc_flush* d_flushes, size_t n_flushes, const uint32_t* d_flush_index,
                         ufc_rate_result* d_results, ufc_rate_state* d_states_out, void* stream);

/* ---- batched resend: packet acks, the resend queue and the pending queue ----
 * The last serial piece of HalfConnection's data path: PacketSender::acknowledge (packet_sender.rs:242-275), the ack
 * flags of PendingPacket (pending_packet.rs:64-78), the resend queue (resend_queue.rs: std's BinaryHeap ordered on
 * resend_time alone, reversed), the pending queue (pending_queue.rs) and emit_data_frames (half_connection/mod.rs:
 * 335-432: the resend loop :351-383, the pending / new-packet loop :385-427), as handle_ack_frame (:154-163) and flush
 * drive them.  The release build is the specification.  Three calls go around the emit and the pack, so that a tick of
 * a device-resident sender is queued with no host code in it:
 *   ufc_rate_begin -> ufc_frame_queue -> ufc_rate_step -> ufc_resend_begin -> ufc_emit_packets -> ufc_resend_place ->
 *   ufc_pack (the data flushes alone: flush c = connection c) -> ufc_build_sizes -> ufc_resend_commit ->
 *   ufc_emit_packets (senders = retake, items_cap = 0: the state after the packets the reference emitted) -> build.
 *
 * State, caller-owned like the frame queue's log arena: one ufc_resend per connection, in and out, with regions in
 * six arenas.  The regions of different connections must not overlap.
 *   heap      [heap_first, heap_first + heap_cap) of ufc_resend_entry: std's BinaryHeap array index for index, entry i
 *             with children 2i+1 and 2i+2; heap_len entries are live.  push appends and sifts up; pop swaps the last
 *             entry into the root, sifts it down to the bottom along the children chosen by `child += (d[child] <=
 *             d[child+1])`, and sifts it up again, "a <= b" meaning a.resend_time_ms >= b.resend_time_ms.  The order of
 *             entries with equal times is observable (all fragments of one flush share a time) and is std's: host and
 *             device agree on the region's bytes.
 *   packets   a ring of ufc_sent_packet, pkt_cap a power of two >= window_size, packet seq at slot seq & (pkt_cap - 1):
 *             the WindowEntry and the PendingPacket's header.  alloc_size is recomputed from data_len.
 *   ack flags one byte per fragment in the ring frag_acked[frag_first + (i & (frag_cap - 1))], frag_cap a power of two
 *             >= ceil(max_alloc / 1448) + window_size (the allocation limit bounds the live fragments and packets are
 *             freed in order, so a live byte is never overwritten).  A packet's fragment f is i = its frag_first + f,
 *             taken from the monotone frag_next and zeroed when the packet enters the table.
 *   tx ring   ufc_tx_ref records, tx_cap a power of two >= (window_size + tail_size + 1) * 127 of the connection's
 *             frame queue, positions from the monotone tx_head / tx_tail: the fragment table that
 *             ufc_sent_frame.ref_first / ref_count and ref_acked[] index (ref_first = tx_first + (position & (tx_cap -
 *             1)), an index into the arena, so the arena holds < 2^32 records).  A frame's refs are its items in
 *             order, contiguous, and never straddle the region's end: if they would, the head skips to its start.
 *   stage     [stage_first, stage_first + stage_cap) of ufc_item: what ufc_resend_begin found to send first.
 *   pending   the pending queue only ever holds fragments f..last of one packet (emit_packet is called only when it is
 *             empty, mod.rs:386), so it is pending_seq, pending_next (the front's fragment id), pending_count and
 *             pending_resend.
 *   window_bytes  the sum of data_len over the window: the part of total_size that acknowledge subtracts.
 * The ufc_sender stays the emit's record and is passed alongside (base_id, next_id, alloc and the parents).
 * All-zero counters with the regions set is HalfConnection::new. */
typedef struct ufc_resend_entry {      /* 16 bytes: resend_queue::Entry */
  uint64_t resend_time_ms;
  uint32_t sequence_id;
  uint16_t fragment_id;
  uint8_t send_count;
  uint8_t reserved;                    /* stored as 0 */
} ufc_resend_entry;

typedef struct ufc_sent_packet {       /* 24 bytes: one packet of the transfer window */
  uint32_t data_offset, data_len;      /* in the payload arena */
  uint32_t frag_first;                 /* its first ack byte's position in the ack ring (monotone, masked at use) */
  uint32_t sequence_id;
  uint16_t window_parent_lead, channel_parent_lead;
  uint8_t channel_id;
  uint8_t resend;                      /* mode >= PERSISTENT */
  uint16_t reserved;                   /* stored as 0 */
} ufc_sent_packet;

#define UFC_TX_RESEND 1                /* the fragment was pushed with resend = true (emit.rs:75, :104) */
typedef struct ufc_tx_ref {            /* 8 bytes: one sent fragment */
  uint32_t sequence_id;
  uint16_t fragment_id;
  uint16_t flags;                      /* UFC_TX_* */
} ufc_tx_ref;

typedef struct ufc_resend {            /* 104 bytes; in and out */
  uint64_t heap_first;
  uint32_t heap_cap, heap_len;
  uint64_t pkt_first;
  uint32_t pkt_cap, frag_next;
  uint64_t frag_first;
  uint32_t frag_cap, tx_cap;
  uint64_t tx_first;
  uint32_t tx_head, tx_tail;
  uint64_t stage_first;
  uint32_t stage_cap, pending_seq;
  uint32_t pending_next, pending_count;
  uint8_t pending_resend;
  uint8_t reserved0;                   /* the reserved fields are copied */
  uint16_t reserved1;
  uint32_t reserved2;
  uint64_t window_bytes;
} ufc_resend;

#define UFC_RS_NO_DATA_FLUSH 1         /* flags[c]: emit_ack_frames returned Err, the tick has no data flush */

#define UFC_RS_DONE 0
#define UFC_RS_SIZE_LIMITED 1          /* DataPushError::SizeLimited in the resend loop: the flush ends, mark_rate_limited */
#define UFC_RS_WINDOW_LIMITED 2        /* DataPushError::WindowLimited in the resend loop: the flush ends */
#define UFC_RS_REF_HANG 3              /* the reference never returns from mod.rs:405-407 / :422-424 (below) */
#define UFC_RS_BAD_STATE 4
#define UFC_RS_STAGE_FULL 5            /* the stage's capacity; ends the flush like WINDOW_LIMITED */
#define UFC_RS_HEAP_FULL 6             /* commit only: the heap's capacity */
typedef struct ufc_resend_result {     /* 48 bytes: ufc_resend_begin_* */
  uint32_t stop;
  uint32_t n_resent, n_pending_staged; /* the stage: resent fragments, then pending ones */
  uint32_t heap_popped_dead, heap_popped_acked;
  uint32_t packets_freed;              /* by acknowledge */
  uint32_t refs_acked;                 /* ack bytes set from ref_acked */
  uint32_t heap_len, pending_count;    /* after the call: with base_id != next_id, what the sync frame's decision
                                          (mod.rs:257-263) and is_send_pending (:120-122) need */
  uint32_t acks_ignored;               /* ack frames acknowledge returned from at :246 (or whose id is no packet id) */
  uint64_t bytes_freed;
} ufc_resend_result;

typedef struct ufc_resend_commit_result { /* 40 bytes: ufc_resend_commit_* */
  uint32_t stop;
  uint32_t pending_packed;             /* pending fragments that left the pending queue */
  uint32_t packets_entered;            /* new packets the reference emitted: entered into the table */
  uint32_t heap_pushed, heap_dropped;  /* dropped: pushes that found the heap full (HEAP_FULL) */
  uint32_t refs_written, frames;       /* tx refs and sent records written */
  uint32_t take;                       /* retake[c].take */
  uint32_t heap_len, pending_count;    /* after the call */
} ufc_resend_commit_result;

/* ufc_resend_begin_*: behind ufc_rate_step_*, in front of the emit.  Connection c owns the frames [frame_first[c],
 * frame_first[c + 1]) (the CSR the frame queue takes) and reads queues[c] and its log ring as ufc_frame_queue_* left
 * them, rate[c].now_ms and rate[c].rtt_ms (ufc_rate_step_*'s result: the flush's now_ms and rtt_ms, mod.rs:197),
 * flags[c] (nullable: 0) and flushes[c], the data flush the pack will get.  Per connection, in this order:
 *   1. Ack propagation.  For every position r in [tx_tail, tx_head) with ref_acked[r] != 0 (r < refs_cap; ref_acked
 *      nullable): ref_acked[r] = 0 (the frame queue never clears it: this call consumes it), and if the ref has
 *      UFC_TX_RESEND and its packet is in the window ((sequence_id - base_id) & 0xFFFFF < (next_id - base_id) &
 *      0xFFFFF: Weak::upgrade succeeds) its ack byte is set (acknowledge_fragment).  A ref is matched to its packet
 *      by id and window position alone: a ref still in the ring when its id has come round 2^20 packets later would
 *      mark the new packet.  The frame queue forgets a frame 4 RTTs after it was sent, so that takes 2^20 packets
 *      within 4 RTTs on one connection; the reference's weak pointer cannot be fooled this way.  Then tx_tail moves to the
 *      ref_first of the frame at the queue's log_base_id, or to tx_head if the log is empty.
 *   2. acknowledge(f[1]) for every ok UFC_FRAME_ACK frame of the range in arrival order, literally :242-275: ignored
 *      when delta > span; else alloc, window_bytes, the window parent and the channel parents are updated and
 *      base_id moves.  An f[1] above 0xFFFFF, which no sender writes, is ignored too (the reference walks past
 *      next_id and panics on an empty window slot).
 *      handle_ack_frame interleaves the frame queue's work and acknowledge frame by frame; the two states meet only
 *      through the ack flags and the weak pointers, and those are read at flush time only (a fragment marked on a
 *      packet that a later acknowledge of the same tick frees is never looked at again), so running all of
 *      ufc_frame_queue_* first and every acknowledge after it gives the same state.
 *   3. Unless UFC_RS_NO_DATA_FLUSH: the resend loop (:351-383).  While the heap is not empty, for its top entry:
 *      packet gone ((sequence_id - base_id) & 0xFFFFF >= (next_id - base_id) & 0xFFFFF): pop, continue; fragment
 *      acknowledged: pop, continue; resend_time_ms > now_ms: break; else dfe.push, which is the pack's rule (steps 1-4
 *      of the ufc_flush comment) run over flushes[c] as a state machine of four variables (alloc, frames, the size
 *      and count of the frame in progress): WINDOW_LIMITED and SIZE_LIMITED end the loop with that stop; on success
 *      the fragment becomes the stage's next item (as the emit makes items, from the packet table's slot), the entry
 *      is popped and pushed again as {now_ms + rtt_ms * (1 << send_count), min(send_count + 1, 2)} (wrapping u64, the
 *      shift amount & 63, a wrapping u8 add).  With rtt_ms == 0 the entry is due again at once and is resent until
 *      the flush is limited, as in the reference.  A full stage stops the loop STAGE_FULL.
 *   4. If the loop was not limited: a pending front whose packet is gone or whose ack byte is set stops REF_HANG: the
 *      reference pops the *resend* queue and `continue`s with the same pending front for ever (an ack frame with
 *      packet_window_base_id = next_id, from a hostile or broken peer, gets there).  The connection keeps what the
 *      reference had done when it entered that loop and the flush ends there: the frame in progress goes out, the
 *      heap is not drained, no pending fragment and no new packet is sent, and every later tick stops the same way
 *      until the caller gives the connection up.  Otherwise
 *      all pending fragments are staged behind the resent ones, unjudged: the pack decides how many go.  If they do
 *      not fit the stage none is staged and the stop is STAGE_FULL.
 *   5. senders_out[c] (required, may be `senders`) = the sender with acknowledge's changes, reserve_items = the
 *      staged count, and take = 0 unless the stop is DONE and a data flush takes place (the reference's flush ends
 *      there); states_out[c] (required, may be `states`); results[c].
 * Sizing the stage: with rtt_ms > 0 and times that do not wrap, an entry is resent once per tick, so heap_len + the
 * fragments of the longest packet the caller sends is enough, and that is the sizing to use (24 bytes an item);
 * heap_cap + 65536 covers any packet but is 1.5 MB a connection.  The exception is the u64 wrap: when now_ms +
 * rtt_ms * (1 << send_count) wraps, the re-pushed entry lies in the past, is due again at once and is resent until
 * the flush is limited, as with rtt_ms == 0; STAGE_FULL is then one of the ways that flush ends.
 * UFC_RS_BAD_STATE follows the frame queue's convention: the state is copied through and nothing else is touched; the
 * sender is copied with take = 0 and reserve_items = 0, so that the emit sends nothing for it.  It covers: pkt_cap,
 * frag_cap or tx_cap not a power of two, or below the bounds above (window_size 0 or above 2^20); a region outside its arena (n_tx > 2^32); heap_len > heap_cap; tx_head - tx_tail > tx_cap; the queue's
 * log_cap not a power of two or its ring outside [0, n_log); a reversed or outlying frame range.
 * Counts: n < 2^31 - 1; n == 0 returns UFC_OK whatever the pointers; a NULL frame_first, queues, rate, flushes,
 * states, senders, results, states_out or senders_out, a NULL infos with n_frames != 0, or a NULL arena with a nonzero
 * size is UFC_ERR_INVALID_ARG. */
int ufc_resend_begin_host(const ufc_frame_info* infos, size_t n_frames, const uint64_t* frame_first,
                          const ufc_frame_queue* queues, const ufc_sent_frame* log, size_t n_log,
                          const ufc_rate_result* rate, const uint32_t* flags, const ufc_flush* flushes,
                          const ufc_resend* states, const ufc_sender* senders, size_t n, ufc_resend_entry* heap,
                          size_t n_heap, const ufc_sent_packet* pkts, size_t n_pkts, uint8_t* frag_acked, size_t n_frag,
                          const ufc_tx_ref* tx, size_t n_tx, uint8_t* ref_acked, size_t refs_cap, ufc_item* stage,
                          size_t n_stage, ufc_resend_result* results, ufc_resend* states_out, ufc_sender* senders_out,
                          int nthreads);

/* ufc_resend_place_*: behind the emit.  Copies connection c's staged items (begin_results[c].n_resent +
 * n_pending_staged of them, from its stage) into items[flush_first[c] ..), the reserve_items slots the emit left, at
 * most flush_first[c + 1] - flush_first[c] of them and none at an index >= items_cap.  A copy: on the device one wave
 * per connection with a lane per staged item of that connection (not one lane per staged item over the whole batch
 * with the sender searched in flush_first, as the emit's item kernel does it: with less than one staged item a
 * connection most waves have one live lane; 0.06 ms for 250,000 connections, the smallest of the three calls).
 * n == 0 returns UFC_OK; a NULL states, begin_results or flush_first, NULL stage with n_stage != 0 or NULL items with
 * items_cap != 0 is UFC_ERR_INVALID_ARG. */
int ufc_resend_place_host(const ufc_resend* states, const ufc_resend_result* begin_results, size_t n,
                          const ufc_item* stage, size_t n_stage, const uint64_t* flush_first, ufc_item* items,
                          size_t items_cap, int nthreads);

/* ufc_resend_commit_*: behind the pack of the data flushes (flush c = connection c, over the emit's flush_first)
 * and the build's size pass.  Inputs per connection: flush_results[c] and its frames infos[frame_first ..+
 * frame_count) with their sizes out_offsets[g + 1] - out_offsets[g]; the first emit's packet_results and
 * sender_results[c] over packets[packet_first[c] .. packet_first[c + 1]); begin_results[c]; rate[c] as in begin;
 * senders[c] as begin wrote it.  In this order:
 *   - items_packed >= n_resent must hold, because begin ran the pack's rule; otherwise BAD_STATE.
 *   - The packed pending fragments leave the pending queue; with pending_resend each is pushed {now_ms + rtt_ms, 1},
 *     in order (:417-421).
 *   - If pending fragments are left, the reference emitted no new packet: take = 0.  Otherwise p = the packet that
 *     owns the first unpacked new item.  Packets 0..p were emitted by the reference (:387-395): they enter the packet
 *     table, their ack bytes are taken from frag_next and zeroed, window_bytes grows by their lengths; the packed
 *     fragments of resend packets are pushed {now_ms + rtt_ms, 1} in item order; p's unpacked fragments become the
 *     pending queue; take = p's index in the range + 1.  When every item was packed, take = the first emit's
 *     packets_consumed and every emitted packet enters.
 *   - retake[c] (required, may be `senders`) = senders[c] with that take and reserve_items = 0: the second emit's
 *     input.
 *   - Every packed item's ufc_tx_ref is appended (UFC_TX_RESEND from its packet's resend) and the frames' records are
 *     written to sent[g], g the frame's index in infos: send_time_ms = now_ms, size, ref_first / ref_count,
 *     UFC_SENT_NONCE from aux.  sent_first[c] = frame_first and sent_first[n] = *frames_used: the next tick's input
 *     to ufc_frame_queue_*.  Records at an index >= sent_cap are not written.
 *   - next_extra_flags[c] (nullable): UFC_FQ_MARK_RATE_LIMITED is set when the pack's stop or begin's stop was
 *     SIZE_LIMITED and cleared otherwise; the other bits stay.  It is the next tick's extra_flags of
 *     ufc_rate_begin_*: the frame queue sets its pending mark behind this tick's pushes, as emit.rs:67 and :85 do.
 *   - A push that finds heap_len == heap_cap is dropped and counted, and the stop is HEAP_FULL: that fragment is not
 *     resent.  Entries of departed packets leave only at the top of the heap, so no static bound on its length
 *     exists; the live fragments of Persistent and Reliable packets plus a margin for the departed is a sizing.
 * BAD_STATE (begin's rules, begin's stop BAD_STATE, items_packed < n_resent or beyond the flush, frames outside
 * [0, n_infos), items outside [0, n_items), a reversed or outlying packet range, fewer item slots than staged items):
 * the state is copied through, retake[c] has take = 0, and the flush's frames get records with ref_count = 0.
 * Counts and NULL rules as begin's; n_packets < 2^31 - 1. */
int ufc_resend_commit_host(const ufc_flush_result* flush_results, const ufc_frame_info* infos, size_t n_infos,
                           const uint64_t* out_offsets, const uint64_t* frames_used, const ufc_item* items,
                           size_t n_items, const uint64_t* flush_first, const ufc_packet* packets, size_t n_packets,
                           const uint64_t* packet_first, const ufc_packet_result* packet_results,
                           const ufc_sender_result* sender_results, const ufc_resend_result* begin_results,
                           const ufc_rate_result* rate, const ufc_resend* states, const ufc_sender* senders, size_t n,
                           ufc_resend_entry* heap, size_t n_heap, ufc_sent_packet* pkts, size_t n_pkts,
                           uint8_t* frag_acked, size_t n_frag, ufc_tx_ref* tx, size_t n_tx, ufc_sent_frame* sent,
                           size_t sent_cap, uint64_t* sent_first, uint32_t* next_extra_flags,
                           ufc_resend_commit_result* results, ufc_resend* states_out, ufc_sender* retake, int nthreads);

/* The same three on the GPU (gfx950 kernels, resend.hip): every pointer device memory, asynchronous on `stream`,
 * nothing allocated per call, no scratch.  One launch per call.  Below 16,384 connections one wave per connection (one
 * wave per workgroup, as the frame queue); from there on begin and commit give every connection a lane, 64 heap walks
 * in flight per wave (measured: DESIGN 5.14).  In the wave form the whole wave takes the
 * live refs (64 per pass), the slots acknowledge frees (wave sums of alloc_size and data_len, a ballot for the
 * window parent), the pending fragments' items, and commit's table entries, ack bytes and refs; the heap operations
 * and the pack rule are a dependent chain and run in one lane. */
int ufc_resend_begin_varlen(ufc_ctx* ctx, const ufc_frame_info* d_infos, size_t n_frames, const uint64_t* d_frame_first,
                            const ufc_frame_queue* d_queues, const ufc_sent_frame* d_log, size_t n_log,
                            const ufc_rate_result* d_rate, const uint32_t* d_flags, const ufc_flush* d_flushes,
                            const ufc_resend* d_states, const ufc_sender* d_senders, size_t n, ufc_resend_entry* d_heap,
                            size_t n_heap, const ufc_sent_packet* d_pkts, size_t n_pkts, uint8_t* d_frag_acked,
                            size_t n_frag, const ufc_tx_ref* d_tx, size_t n_tx, uint8_t* d_ref_acked, size_t refs_cap,
                            ufc_item* d_stage, size_t n_stage, ufc_resend_result* d_results, ufc_resend* d_states_out,
                            ufc_sender* d_senders_out, void* stream);
int ufc_resend_place_varlen(ufc_ctx* ctx, const ufc_resend* d_states, const ufc_resend_result* d_begin_results, size_t n,
                            const ufc_item* d_stage, size_t n_stage, const uint64_t* d_flush_first, ufc_item* d_items,
                            size_t items_cap, void* stream);
int ufc_resend_commit_varlen(ufc_ctx* ctx, const ufc_flush_result* d_flush_results, const ufc_frame_info* d_infos,
                             size_t n_infos, const uint64_t* d_out_offsets, const uint64_t* d_frames_used,
                             const ufc_item* d_items, size_t n_items, const uint64_t* d_flush_first,
                             const ufc_packet* d_packets, size_t n_packets, const uint64_t* d_packet_first,
                             const ufc_packet_result* d_packet_results, const ufc_sender_result* d_sender_results,
                             const ufc_resend_result* d_begin_results, const ufc_rate_result* d_rate,
                             const ufc_resend* d_states, const ufc_sender* d_senders, size_t n, ufc_resend_entry* d_heap,
                             size_t n_heap, ufc_sent_packet* d_pkts, size_t n_pkts, uint8_t* d_frag_acked, size_t n_frag,
                             ufc_tx_ref* d_tx, size_t n_tx, ufc_sent_frame* d_sent, size_t sent_cap,
                             uint64_t* d_sent_first, uint32_t* d_next_extra_flags, ufc_resend_commit_result* d_results,
                             ufc_resend* d_states_out, ufc_sender* d_retake, void* stream);

#ifdef __cplusplus
}
#endif

/* The batched flush control (ufc_flush_acks_*, ufc_flush_sync_*: the ack flush with dud and carry, the sync frame)
 * is declared in its own header, which this one brings along. */
#include "uflow_flush_ctl.h"

/* The batched frame routing (ufc_route_table_build_host, ufc_route_frames_*: a frame's source address to its
 * connection, the batch grouped by connection) is declared in its own header as well. */
#include "uflow_route.h"

#endif /* UFLOW_FRAME_CODEC_H */
