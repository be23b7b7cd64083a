/*
 * uflow_route.h -- C ABI of libuflowcrc.so for the batched frame routing: a received frame's source address to its
 * connection, and the batch grouped by connection.  The records and calls here work on the records of
 * uflow_frame_codec.h, which includes this header at its end: including either gives both.
 *
 * Reference (lowquark/uflow v0.7.1, Rust) interfaces each entry point replaces:
 *   ufc_route_table_build_host <- the keys of Server.clients: HashMap<SocketAddr, ...> (src/server/mod.rs:118)
 *   ufc_route_frames_host, ufc_route_frames_varlen
 *                              <- the address lookup and the dispatch of Server::handle_frames (src/server/mod.rs:
 *                                 591-602 over handle_frame :492-589) and of Client::handle_frames
 *                                 (src/client/mod.rs:557-583) for data, sync and ack frames of State::Active clients,
 *                                 with the timeout refresh of handle_data / handle_sync / handle_ack
 * Conventions: as uflow_frame_codec.h.
 */
#ifndef UFLOW_ROUTE_H
#define UFLOW_ROUTE_H

#include "uflow_frame_codec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched frame routing: source address -> connection, grouped ----
 * Every per-connection stage (ufc_frame_window_*, ufc_receive_packets_*, ufc_frame_queue_*) takes the parse's
 * ufc_frame_info records grouped by connection: connection r owns infos[frame_first[r] .. frame_first[r + 1]) in
 * arrival order.  A socket delivers (frame, SocketAddr) pairs interleaved across all clients; these calls make the
 * grouping from the addresses.  The handshake and disconnect state machine stays with the host: its frames are
 * handed back, together with the frames whose routing they may change.
 *
 * A key is a SocketAddr in 32 bytes.  V4 puts its 4 bytes in ip[0..4) and leaves the rest zero.  Equality is bytewise
 * over all 32 bytes and the caller zeroes what it does not use: as Rust's Eq and Hash of SocketAddr, V4 and V4-mapped
 * V6 differ and V6 includes flowinfo and scope_id.  Any 32 bytes are a key. */
typedef struct ufc_addr {              /* 32 bytes */
  uint8_t  ip[16];
  uint16_t port;
  uint8_t  family;                     /* 4 or 6 */
  uint8_t  reserved;
  uint32_t flowinfo;
  uint32_t scope_id;
  uint32_t reserved2;
} ufc_addr;

/* One open-addressing slot.  The table is slots[n_slots] plus three scalars passed by value: seed, max_probe and
 * n_conns.  n_slots is a power of two and > n_conns.
 *   h = seed;  for k in 0..7: w = little-endian u32 of key bytes [4k, 4k + 4);  h = (h ^ w) * 0x9E3779B1;  h ^= h >> 15
 *   h *= 0x85EBCA77;  h ^= h >> 13;  home = h & (n_slots - 1)                          (u32, wrapping)
 * Lookup: probe slots[(home + p) & (n_slots - 1)] for p = 0 .. min(max_probe, n_slots - 1).  A slot with used == 0
 * ends the search with "not found"; a used slot whose conn < n_conns and whose key is equal gives conn; any other used
 * slot is skipped; when the probes run out the result is "not found".  Any bytes are a table, every input has one
 * answer, and the loop is bounded whatever the table holds.
 * The seed is the caller's random number, drawn once per table and kept from the peers: it is the table's only guard
 * against addresses chosen to collide (the reference's HashMap is SipHash with random keys).  The hash is not
 * cryptographic: a peer that learns the seed can build long chains, which max_probe then bounds. */
typedef struct ufc_route_slot {        /* 48 bytes */
  ufc_addr key;
  uint32_t conn;
  uint8_t  used;
  uint8_t  reserved[11];
} ufc_route_slot;

/* Clears the slots and inserts connections 0 .. n_conns - 1 in order by linear probing from their home slot;
 * *max_probe is the longest displacement used (0 for an empty table).  A repeated address is UFC_ERR_INVALID_ARG
 * with *dup_index (nullable) set to the second occurrence; the slots are then unspecified.  Membership changes are
 * control plane and happen on the host: the table is plain data the caller uploads.  n_conns < 2^31 - 3; n_slots not a
 * power of two, n_slots <= n_conns, n_slots > 2^31, a NULL slots or max_probe, or a NULL addrs with n_conns != 0 is
 * UFC_ERR_INVALID_ARG. */
int ufc_route_table_build_host(const ufc_addr* addrs, size_t n_conns, uint32_t seed, ufc_route_slot* slots,
                               size_t n_slots, uint32_t* max_probe, uint64_t* dup_index);

#define UFC_ROUTE_DROP 0               /* cls[i] */
#define UFC_ROUTE_CONN 1               /* in its connection's bucket */
#define UFC_ROUTE_CONTROL 2            /* the host's handshake and disconnect code takes it */
#define UFC_ROUTE_DEFERRED 3           /* to be routed again once the host has handled the control frames before it */
typedef struct ufc_route_result {      /* 16 bytes */
  uint32_t frames;                     /* UFC_ROUTE_CONN frames of the connection: its bucket's length */
  uint32_t first_control;              /* first control frame from its address, UFC_NO_PARENT if none */
  uint32_t deferred;                   /* UFC_ROUTE_DEFERRED frames from its address */
  uint32_t reserved;                   /* 0 */
} ufc_route_result;

/* ufc_route_frames_*: behind the parse, in front of ufc_frame_window_*.  infos[n] are the parse's records in arrival
 * order, addrs[n] their source addresses, offsets[n] the parsed batch's CSR offsets or any per-frame src_base
 * (nullable: NULL is read as all zero).  The stages find a frame's items through infos[i].item_first and its payload
 * through src_base[i], so only the 32-byte infos and the 8-byte offsets are permuted: items and frame bytes stay
 * where the parse left them.  conn_active[c] != 0: client c is in State::Active (kept outside the table, so that an
 * activation does not rebuild it).
 *
 * Classification is what handle_frames does with the table as it stands at the start of the batch.  A frame is
 * control if ok != 0 and kind is 0..5, session if ok != 0 and kind is UFC_FRAME_DATA, UFC_FRAME_SYNC or UFC_FRAME_ACK,
 * and otherwise dropped (Frame::read gave None, server/mod.rs:598).  e(i) is the lookup of addrs[i];
 * first_control[c] the smallest control i with e(i) = c; first_unknown_control the smallest control i with e(i) not
 * found; each UFC_NO_PARENT when there is none.
 *   control                                            UFC_ROUTE_CONTROL
 *   session, e(i) = c, i > first_control[c]            UFC_ROUTE_DEFERRED
 *   session, e(i) = c, otherwise                       UFC_ROUTE_CONN if conn_active[c], else UFC_ROUTE_DROP
 *                                                      (`_ => ()`, server/mod.rs:509, :531, :553)
 *   session, not found, i > first_unknown_control      UFC_ROUTE_DEFERRED
 *   session, not found, otherwise                      UFC_ROUTE_DROP
 *   anything else                                      UFC_ROUTE_DROP
 * The rule is exact because inside handle_frames a client's state, and the table's membership, change only through
 * control frames (handle_handshake_syn / _ack, handle_disconnect / _ack, server/mod.rs:492-589 dispatching on the
 * frame kind; a data, sync or ack frame touches only its own client's half connection and timeout, :499-560), and a
 * control frame changes only the client of its own address: before an address' first control frame the batch sees
 * the state the table was built from.  A session frame from an unknown address is deferred behind any unknown
 * address' control frame (one word instead of a set of new addresses; a deferred frame routed again is never wrong,
 * only later).  The host handles the control frames in arrival order, then routes the deferred frames again, still in
 * arrival order, against the updated table; a deferred frame of connection c always follows all of c's
 * UFC_ROUTE_CONN frames of this batch.  INTEGRATION.md has the loop.
 *
 * Outputs (required unless marked):
 *   route[n]             e(i), or UFC_NO_PARENT.
 *   cls[n]               UFC_ROUTE_*.
 *   bucket_first[n_conns + 3]   a CSR over n_conns + 2 buckets: 0 .. n_conns - 1 the connections' UFC_ROUTE_CONN
 *                        frames, n_conns the CONTROL and DEFERRED frames together, n_conns + 1 the dropped frames;
 *                        the last entry is n.  Its first n_conns + 1 entries are, unchanged, the frame_first the frame
 *                        window, the receive and the frame queue take.
 *   order[n]             the source frame index of every grouped position; stable: within a bucket it ascends.
 *   infos_out[n]         infos_out[k] = infos[order[k]], byte for byte.
 *   src_base_out[n]      src_base_out[k] = offsets[order[k]] (0 without offsets).  These two are what the stages take
 *                        as infos and src_base, beside the parse's own items and payload.  Neither may be its input.
 *   results[n_conns]     above.
 *   timeout_out[n_conns] now_ms + active_timeout_ms (wrapping) where frames != 0, else timeout_in[c]; may be
 *                        timeout_in.  (server/mod.rs:507, :529, :551; client/mod.rs:561, :571, :581.)
 *   first_unknown_control   one word.
 * Every output is a function of the inputs alone.  n < 2^31 - 1 and n_conns < 2^31 - 3; n_slots as for the build.
 * n == 0 writes bucket_first all zero, results with no frames (first_control = UFC_NO_PARENT), first_unknown_control =
 * UFC_NO_PARENT, copies the timeouts through and returns UFC_OK.  A NULL slots, bucket_first or
 * first_unknown_control; a NULL infos, addrs, route, cls, order, infos_out or src_base_out with n != 0; a NULL
 * conn_active, timeout_in, results or timeout_out with n_conns != 0; infos_out == infos or src_base_out == offsets with
 * n != 0 is UFC_ERR_INVALID_ARG. */
int ufc_route_frames_host(const ufc_frame_info* infos, const ufc_addr* addrs, const uint64_t* offsets, size_t n,
                          const ufc_route_slot* slots, size_t n_slots, uint32_t seed, uint32_t max_probe,
                          size_t n_conns, const uint8_t* conn_active, uint64_t now_ms, uint64_t active_timeout_ms,
                          const uint64_t* timeout_in, uint32_t* route, uint8_t* cls, uint64_t* bucket_first,
                          uint32_t* order, ufc_frame_info* infos_out, uint64_t* src_base_out,
                          ufc_route_result* results, uint64_t* timeout_out, uint32_t* first_unknown_control,
                          int nthreads);
/* The same on the GPU (gfx950 kernels, route.hip): every pointer device memory, asynchronous on `stream`, nothing
 * allocated per call.  A lane per frame looks its address up and takes the minima (first_control,
 * first_unknown_control: minima do not depend on the order they are taken in); a lane per frame classifies and writes
 * its bucket number as a sort key; a stable least-significant-digit radix placement with 8-bit digits over the bytes
 * n_conns + 1 needs (per pass: a digit histogram per tile of 1024 frames, an exclusive sum over the digit-major
 * histograms, a scatter whose rank comes from wave ballots and per-digit cursors the tile's waves advance in wave
 * order) gives order; the placed keys' runs give the buckets' lengths, whose exclusive sum is bucket_first; a lane per
 * grouped position gathers; a lane per connection finishes results and timeouts.  No kernel waits on another
 * workgroup and no output depends on the order atomics land in (they take minima and sums).  The context's per-stream
 * scratch holds, each part rounded up to 256: 8 n bytes of keys, with P = the passes (P > 1 ? 8 n : 0) bytes of
 * indices in flight, 1024 ceil(n / 1024) bytes of histograms, and the temporaries of the two scans. */
int ufc_route_frames_varlen(ufc_ctx* ctx, const ufc_frame_info* d_infos, const ufc_addr* d_addrs,
                            const uint64_t* d_offsets, size_t n, const ufc_route_slot* d_slots, size_t n_slots,
                            uint32_t seed, uint32_t max_probe, size_t n_conns, const uint8_t* d_conn_active,
                            uint64_t now_ms, uint64_t active_timeout_ms, const uint64_t* d_timeout_in,
                            uint32_t* d_route, uint8_t* d_cls, uint64_t* d_bucket_first, uint32_t* d_order,
                            ufc_frame_info* d_infos_out, uint64_t* d_src_base_out, ufc_route_result* d_results,
                            uint64_t* d_timeout_out, uint32_t* d_first_unknown_control, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UFLOW_ROUTE_H */
