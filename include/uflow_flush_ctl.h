/*
 * uflow_flush_ctl.h -- C ABI of libuflowcrc.so for the batched flush control: the glue of HalfConnection::flush
 * around the data flush.  The records and calls here work on the records of uflow_frame_codec.h, which includes
 * this header at its end: including either gives both.
 *
 * Reference (lowquark/uflow v0.7.1, Rust) interfaces each entry point replaces:
 *   ufc_flush_acks_host, ufc_flush_acks_varlen
 *                              <- emit_ack_frames with push_dud and the FrameAckQueue deque's carry
 *                                 (src/half_connection/mod.rs:296-333 over emit.rs:137-211)
 *   ufc_flush_sync_host, ufc_flush_sync_varlen
 *                              <- emit_sync_frame (mod.rs:234-294), the early returns of emit_frames (:217-232) and
 *                                 is_send_pending (:120-122)
 * Conventions: as uflow_frame_codec.h.
 */
#ifndef UFLOW_FLUSH_CTL_H
#define UFLOW_FLUSH_CTL_H

#include "uflow_frame_codec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched flush control: the ack flush with dud and carry, the sync frame ----
 * The glue of HalfConnection::flush around the data flush: emit_ack_frames (src/half_connection/mod.rs:296-333 over
 * AckFrameEmitter, emit.rs:137-211) with the FrameAckQueue's deque as a carry, and emit_sync_frame (mod.rs:234-294) with
 * the early returns of emit_frames (:217-232) and is_send_pending (:120-122).  The release build is the specification,
 * wrapping arithmetic included.  With the two calls a full-duplex tick is queued with no host code in it:
 *   ... ufc_frame_window -> ... ufc_rate_step -> ufc_flush_acks -> ufc_build (the ack frames) -> ufc_resend_begin ->
 *   ... -> the second ufc_emit_packets -> ufc_flush_sync -> ufc_build (the sync frames); INTEGRATION.md has every call.
 *
 * State: one ufc_flush_ctl per connection, in and out.  The front of FrameAckQueue.entries that earlier flushes could
 * not send is carry[carry_first .. carry_first + carry_count), oldest first, its last group the window's tail, inside
 * the room [carry_first, carry_first + carry_cap) of the caller's arena of ufc_item ack groups; the rooms of different
 * connections must not overlap.  has_keepalive is an Option's Some byte (sync_keepalive_interval_ms): nonzero on input
 * means Some; ufc_flush_sync_* writes it 0 or 1 and an interval whose byte is 0 as 0; ufc_flush_acks_* copies both.
 * The reserved fields are copied.  All zero but for the room and the keepalive is HalfConnection::new. */
typedef struct ufc_flush_ctl {         /* 40 bytes; in and out */
  uint64_t sync_timeout_base_ms;
  uint64_t keepalive_interval_ms;
  uint64_t carry_first;
  uint32_t carry_cap, carry_count;
  uint8_t  has_keepalive, reserved0;
  uint16_t reserved1;
  uint32_t reserved2;
} ufc_flush_ctl;

#define UFC_FA_DONE 0
#define UFC_FA_BAD_STATE 1             /* below: the state copied through, nothing emitted */
#define UFC_FA_CARRY_FULL 2            /* unpacked groups outgrew carry_cap: the oldest were dropped */
typedef struct ufc_flush_acks_result { /* 24 bytes */
  uint32_t stop;                       /* UFC_FA_*; the emitter's own stop is ufc_flush_result.stop */
  uint32_t merged_first, merged_count; /* its merged list: merged[merged_first ..+ merged_count) */
  uint32_t carried, dropped;           /* groups in the new carry; groups that found no room in it */
  uint8_t  dud;                        /* push_dud opened the first frame */
  uint8_t  reserved[3];
} ufc_flush_acks_result;

/* ufc_flush_acks_*: behind this tick's ufc_frame_window_* and ufc_rate_step_*, in front of ufc_resend_begin_*.  The
 * window call runs every tick (with an empty frame range when nothing arrived), so a held tail is always re-emitted.
 * Connection c reads ctl[c] and its carry, windows[c] as the window call left it, that call's groups
 * [group_first[c], group_first[c + 1]) (n_groups: the records the array holds), receivers[c].base_id and
 * rate[c].flush_alloc.  Per connection:
 *   The merged list = the carry without its last group (the window writes the carried tail first, as updated: the
 *   carry's copy of it is stale) followed by the window's groups.  carry_count > 0 with no window group, or a first
 *   window group whose id differs from the carry's last id, is UFC_FA_BAD_STATE; so are carry_count > carry_cap, a room
 *   outside [0, n_carry) and a group range that is reversed or leaves [0, n_groups).
 *   1. alloc = flush_alloc, no frame in progress.
 *   2. If windows[c].sync_reply: push_dud (emit.rs:149-166).  With alloc < 0 the flush stops UFC_PACK_SIZE_LIMITED with
 *      no frame and nothing popped; otherwise a frame of size 15 with no groups is in progress.
 *   3. The pack's ack rule (steps 1, 2 and 4 of the ufc_flush comment, H = 15, e = 9, no count limit) over the merged
 *      list from that state, then finalize.  The rule is literal: a dud frame in progress with 0 <= alloc < 15 is
 *      finalized empty at the first push and the flush stops SIZE_LIMITED, where without a dud the same alloc packs
 *      one group first.
 * Outputs:
 *   merged, merged_cap   the merged groups; merged_first[n + 1] the exclusive sum of the merged counts, directly the
 *                        flush_first of an ack flush; *merged_used the total.  Groups at an index >= merged_cap are not
 *                        written (compare, as with the parse's items_cap); n_carry + n_groups is always enough.
 *   infos, frames_cap    the ack frames in connection order, in the pack's form, ready for ufc_build_* over `merged`:
 *                        kind = UFC_FRAME_ACK, ok = 1, f[0] = windows[c].base_id, f[1] = receivers[c].base_id,
 *                        item_first / item_count into merged (a dud frame that took no group has item_count = 0),
 *                        everything else 0.  *frames_used is exact; frames at an index >= frames_cap are not written;
 *                        n + n_carry + n_groups is always enough.
 *   results[c]           the ufc_flush_result ufc_pack_* gives an ack flush over the merged list (without sync_reply
 *                        they are equal record for record); UFC_FA_BAD_STATE: zero counts, stop = UFC_PACK_BAD_RANGE,
 *                        alloc_left = flush_alloc.
 *   ack_results[c]       above.
 *   windows_out[c]       (required, may be `windows`) sync_reply cleared iff a frame was emitted (emit_cb, mod.rs:
 *                        306-310); has_tail cleared iff every merged group was packed (the deque is empty: the next
 *                        frame opens a new group even within 32 ids of the old one); nothing else changed.
 *   ctl_out[c]           (required, may be `ctl`) carry_count = the new carry: the unpacked groups in order, copied into
 *                        the room.  The room may be read and written by the same call.
 *   flushes[c]           (nullable) flush_alloc = alloc_left, no other field touched: flush c is connection c's data
 *                        flush, as the resend calls take it.
 *   flags[c]             (nullable) UFC_RS_NO_DATA_FLUSH set on SIZE_LIMITED and cleared otherwise; other bits kept.
 * Where the reference has no bound: the deque is unbounded.  If the unpacked groups outgrow carry_cap, the oldest are
 * dropped and the newest carry_cap kept (so the tail always survives with carry_cap >= 1); `dropped` counts them and
 * the stop is UFC_FA_CARRY_FULL.  A dropped group is the same to the peer as a lost ack frame: the frames it named are
 * taken for lost by the sender's loss detection, as after any dropped datagram.  (UFC_RATE_RECV_FULL is the rate
 * section's answer to its own unbounded Vec.)  carry_cap = 0 carries nothing; a SIZE_LIMITED flush then drops its
 * unpacked groups, the tail included, and the window's has_tail stays set: give every connection a room.
 * n, n_groups and n_carry < 2^31 - 1 (the merged counts and the indices into `merged` are 32-bit); n == 0 returns
 * UFC_OK whatever the pointers; a NULL ctl, windows, group_first, receivers, rate, merged_first, merged_used,
 * frames_used, results, ack_results, windows_out or ctl_out, or a NULL groups, carry, merged or infos with a nonzero
 * size, is UFC_ERR_INVALID_ARG. */
int ufc_flush_acks_host(const ufc_flush_ctl* ctl, const ufc_frame_window* windows, const ufc_item* groups,
                        size_t n_groups, const uint64_t* group_first, const ufc_receiver* receivers,
                        const ufc_rate_result* rate, size_t n, ufc_item* carry, size_t n_carry, ufc_item* merged,
                        size_t merged_cap, uint64_t* merged_first, uint64_t* merged_used, ufc_frame_info* infos,
                        size_t frames_cap, uint64_t* frames_used, ufc_flush_result* results,
                        ufc_flush_acks_result* ack_results, ufc_frame_window* windows_out, ufc_flush_ctl* ctl_out,
                        ufc_flush* flushes, uint32_t* flags, int nthreads);
/* The same on the GPU (gfx950 kernels, flush_ctl.hip): every pointer device memory, asynchronous on `stream`, nothing
 * allocated per call.  A lane per connection counts its merged groups and its frames (a loop over frames: a full frame
 * is 161 groups); two exclusive sums; then a wave per connection with a lane per group copies (the shape of
 * ufc_resend_place_*).  The context's per-stream scratch holds 8 (n + 1) bytes of frame counts + the scan's
 * temporaries, each part rounded up to 256. */
int ufc_flush_acks_varlen(ufc_ctx* ctx, const ufc_flush_ctl* d_ctl, const ufc_frame_window* d_windows,
                          const ufc_item* d_groups, size_t n_groups, const uint64_t* d_group_first,
                          const ufc_receiver* d_receivers, const ufc_rate_result* d_rate, size_t n, ufc_item* d_carry,
                          size_t n_carry, ufc_item* d_merged, size_t merged_cap, uint64_t* d_merged_first,
                          uint64_t* d_merged_used, ufc_frame_info* d_infos, size_t frames_cap, uint64_t* d_frames_used,
                          ufc_flush_result* d_results, ufc_flush_acks_result* d_ack_results,
                          ufc_frame_window* d_windows_out, ufc_flush_ctl* d_ctl_out, ufc_flush* d_flushes,
                          uint32_t* d_flags, void* stream);

#define UFC_FS_SENT 0                  /* ufc_flush_sync_result.reason */
#define UFC_FS_ACK_LIMITED 1           /* rule 1 */
#define UFC_FS_DATA_LIMITED 2          /* rule 3 */
#define UFC_FS_UPSTREAM 3              /* rule 4 */
#define UFC_FS_NOT_DUE 4               /* rule 5 */
#define UFC_FS_IDLE 5                  /* rule 8 */
#define UFC_FS_NO_ALLOC 6              /* rule 9 */
typedef struct ufc_flush_sync_result { /* 24 bytes */
  uint32_t sent;                       /* 1: a sync frame went out */
  uint32_t reason;                     /* UFC_FS_*: why none did */
  uint32_t heap_len, pending_count;    /* ufc_resend_commit_*'s */
  uint8_t  mode;                       /* the frame's mode bits; 0 when none went out */
  uint8_t  is_send_pending;            /* heap_len != 0 || pending_count != 0: mod.rs:120-122 without
                                          packet_sender.pending_count(), the caller's packets not yet taken */
  uint16_t reserved;
  uint32_t reserved2;
} ufc_flush_sync_result;

/* ufc_flush_sync_*: behind the data flush's last call (the second ufc_emit_packets_*).  Connection c reads ctl[c];
 * rate[c].now_ms and rate[c].rto_ms (ufc_rate_step_*'s result: the flush's time and retransmit timeout);
 * ack_results[c].stop (ufc_flush_acks_*'s ufc_flush_result); begin_results[c].stop; pack_results[c] (the data pack's:
 * stop, frame_count, alloc_left); commit_results[c] (stop, heap_len, pending_count); queues[c].log_next_id and
 * window_base_id after this tick's frame queue call; senders[c].base_id and next_id as the second emit left them.
 * In this order:
 *   1. the ack flush stopped UFC_PACK_SIZE_LIMITED: nothing is done, the state is unchanged (mod.rs:218-221);
 *   2. if the data flush emitted a frame (frame_count > 0): sync_timeout_base_ms = now_ms (:346);
 *   3. UFC_RS_SIZE_LIMITED from begin or UFC_PACK_SIZE_LIMITED from the pack ends here (:223-226); WINDOW_LIMITED and
 *      STAGE_FULL go on;
 *   4. begin's REF_HANG or BAD_STATE, commit's REF_HANG, BAD_STATE or HEAP_FULL: no sync frame.  The reference never
 *      returns from a REF_HANG flush and has no such state as the other two, so nothing is specified there; a
 *      connection whose queues are in doubt does not vouch for them in a sync frame;
 *   5. elapsed = now_ms - sync_timeout_base_ms, wrapping; elapsed < max(rto_ms, 2000): no frame;
 *   6. next_frame_id = log_next_id + frame_count (wrapping: the queue's next_id once this flush's frames are pushed),
 *      present iff it differs from window_base_id;
 *   7. next_packet_id = next_id, present iff next_id != base_id && heap_len == 0 && pending_count == 0;
 *   8. with neither present: no frame without has_keepalive, or with elapsed < keepalive_interval_ms (:269-277);
 *   9. alloc_left < 0: no frame (:279-281);
 *  10. the frame goes out and sync_timeout_base_ms = now_ms.
 * Outputs: infos[syncs_cap], the sync frames compacted in connection order, ready for ufc_build_* (kind =
 * UFC_FRAME_SYNC, ok = 1, aux = the mode bits, f[0] / f[1] the ids with 0 where absent, item_count = 0: write_sync's 14
 * bytes); sync_index[c] the connection's frame or UFC_NO_PARENT; *syncs_used exact, frames at an index >= syncs_cap not
 * written (n is always enough); results[c]; ctl_out[c] (required, may be `ctl`); ticks_next[c].alloc_adjust (nullable)
 * = -14 or 0 and nothing else of the record touched, so that the next ufc_rate_step_* accounts for the frame.
 * n < 2^31 - 1; n == 0 returns UFC_OK whatever the pointers; a NULL ctl, rate, ack_results, begin_results,
 * pack_results, commit_results, queues, senders, sync_index, syncs_used, results or ctl_out, or a NULL infos with
 * syncs_cap != 0, is UFC_ERR_INVALID_ARG. */
int ufc_flush_sync_host(const ufc_flush_ctl* ctl, const ufc_rate_result* rate, const ufc_flush_result* ack_results,
                        const ufc_resend_result* begin_results, const ufc_flush_result* pack_results,
                        const ufc_resend_commit_result* commit_results, const ufc_frame_queue* queues,
                        const ufc_sender* senders, size_t n, ufc_frame_info* infos, size_t syncs_cap,
                        uint32_t* sync_index, uint64_t* syncs_used, ufc_flush_sync_result* results,
                        ufc_flush_ctl* ctl_out, ufc_rate_tick* ticks_next, int nthreads);
/* The same on the GPU (flush_ctl.hip): a lane per connection decides, in tiles of 64 whose ballot counts are scanned
 * over the batch; the same tiles then write the frames (a sending lane's index is the tile's first + the sending lanes
 * below it: the one cross-lane read).  Scratch: 8 (ceil(n / 64) + 1) bytes + the scan's temporaries. */
int ufc_flush_sync_varlen(ufc_ctx* ctx, const ufc_flush_ctl* d_ctl, const ufc_rate_result* d_rate,
                          const ufc_flush_result* d_ack_results, const ufc_resend_result* d_begin_results,
                          const ufc_flush_result* d_pack_results, const ufc_resend_commit_result* d_commit_results,
                          const ufc_frame_queue* d_queues, const ufc_sender* d_senders, size_t n,
                          ufc_frame_info* d_infos, size_t syncs_cap, uint32_t* d_sync_index, uint64_t* d_syncs_used,
                          ufc_flush_sync_result* d_results, ufc_flush_ctl* d_ctl_out, ufc_rate_tick* d_ticks_next,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UFLOW_FLUSH_CTL_H */
