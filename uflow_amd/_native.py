"""ctypes binding of libuflowcrc.so (the C ABI in include/uflow_frame_crc.h and
include/uflow_frame_codec.h).

This is the Python-side equivalent of the `extern "C"` block a Rust caller would declare
(see INTEGRATION.md).  Loading fails loudly when the in-tree library is missing: there is no
CPU fallback for the batched entry points.
"""
import ctypes
import os

from ._build import LIB_PATH as _DEFAULT_LIB

# Measurement tools only: with UFC_AB=1 set as well, UFC_LIB names another build of the library to
# load (in-process A/B runs under tools/).  Without the guard the in-tree library is the one loaded,
# whatever UFC_LIB says ("Test-only environment").
LIB_PATH = os.environ["UFC_LIB"] if os.environ.get("UFC_AB") == "1" and os.environ.get("UFC_LIB") else _DEFAULT_LIB

UFC_OK = 0
UFC_ERR_INVALID_ARG = -1
UFC_ERR_NO_DEVICE = -2
UFC_ERR_HIP = -3
UFC_ERR_NOMEM = -4
UFC_ERR_COMM = -5
UFC_ERR_PEER = -6
UFC_COMM_ID_BYTES = 128
UFC_MAX_RANKS = 64
UFC_OP_GATE, UFC_OP_SEND, UFC_OP_RECV = 0, 1, 2

# ufc_ctx_set_option (include/uflow_frame_crc.h)
UFC_OPT_FIXED_KERNEL, UFC_OPT_VARLEN_KERNEL, UFC_OPT_GENERIC_JC = 0, 1, 2
UFC_FIXED_AUTO, UFC_FIXED_GENERIC, UFC_FIXED_CLAIM16 = 0, 1, 2
UFC_VARLEN_AUTO, UFC_VARLEN_GENERIC, UFC_VARLEN_SORTED, UFC_VARLEN_BLOCKED8, UFC_VARLEN_CLAIM16 = 0, 1, 2, 3, 4
UFC_VARLEN_BLOCKSTREAM, UFC_VARLEN_SORTED8, UFC_VARLEN_STREAM = 5, 6, 7
UFC_OPT_SEAL_KERNEL, UFC_SEAL_INLINE, UFC_SEAL_TWO_PASS = 3, 0, 1
# per-frame status of the batched builds (include/uflow_frame_codec.h)
UFC_BUILD_OK, UFC_BUILD_SKIPPED, UFC_BUILD_BAD_FIELD, UFC_BUILD_BAD_SRC = 0, 1, 2, 3
# why a flush of the batched packs stopped (include/uflow_frame_codec.h)
UFC_PACK_DONE, UFC_PACK_SIZE_LIMITED, UFC_PACK_WINDOW_LIMITED, UFC_PACK_BAD_RANGE = 0, 1, 2, 3
# the batched packet emits (include/uflow_frame_codec.h): SendMode, why a sender stopped, a packet's status
UFC_SEND_TIME_SENSITIVE, UFC_SEND_UNRELIABLE, UFC_SEND_PERSISTENT, UFC_SEND_RELIABLE = 0, 1, 2, 3
UFC_NO_PARENT = 0xFFFFFFFF
UFC_EMIT_DONE, UFC_EMIT_WINDOW_LIMITED, UFC_EMIT_ALLOC_LIMITED, UFC_EMIT_BAD_PACKET, UFC_EMIT_BAD_RANGE = 0, 1, 2, 3, 4
UFC_PACKET_NOT_REACHED, UFC_PACKET_EMITTED, UFC_PACKET_DROPPED = 0, 1, 2
# the batched packet receives (include/uflow_frame_codec.h): a slot's assembly state and flags, a datagram's
# status, why a receiver stopped
UFC_RX_ASM_OPEN, UFC_RX_ASM_CLOSED, UFC_RX_ASM_ACTIVE = 0, 1, 2
UFC_RX_SLOT_ENTRY, UFC_RX_SLOT_DATA, UFC_RX_SLOT_DUD = 1, 2, 4
UFC_RX_PACKET_DUD = 1
(UFC_RX_NOT_HANDLED, UFC_RX_STORED, UFC_RX_COMPLETED, UFC_RX_DUD, UFC_RX_DROPPED_INVALID, UFC_RX_DROPPED_WINDOW,
 UFC_RX_DROPPED_CHANNEL, UFC_RX_DROPPED_CLOSED, UFC_RX_DROPPED_MISMATCH, UFC_RX_DROPPED_DUPLICATE,
 UFC_RX_DROPPED_BAD_SRC) = range(11)
UFC_RX_STATUS_COUNT = 11
UFC_RX_DONE, UFC_RX_BAD_STATE = 0, 1
# the batched frame windows (include/uflow_frame_codec.h): why a connection stopped
UFC_FW_DONE, UFC_FW_BAD_STATE = 0, 1
# the batched frame queues (include/uflow_frame_codec.h): a log slot's flags, a step's flags, why a connection stopped
UFC_SENT_NONCE, UFC_SENT_RATE_LIMITED, UFC_SENT_ACKED, UFC_SENT_MARK = 1, 2, 4, 8
UFC_FQ_HAS_RTT, UFC_FQ_RESET_LOSS, UFC_FQ_MARK_RATE_LIMITED, UFC_FQ_FORGET, UFC_FQ_FEEDBACK = 1, 2, 4, 8, 16
UFC_FQ_DONE, UFC_FQ_BAD_STATE = 0, 1
# the batched send rate control (include/uflow_frame_codec.h): modes, the tick's flag, stops, the result's flags
UFC_RATE_AWAIT_SEND, UFC_RATE_SLOW_START, UFC_RATE_THROUGHPUT_EQN = 0, 1, 2
UFC_RATE_FRAME_SENT = 1
UFC_RATE_DONE, UFC_RATE_BAD_STATE, UFC_RATE_REF_PANIC, UFC_RATE_RECV_FULL = 0, 1, 2, 3
UFC_RATE_FEEDBACK, UFC_RATE_NOFEEDBACK, UFC_RATE_RESET_ISSUED, UFC_RATE_ENTERED_EQN, UFC_RATE_INV_STALLED = 1, 2, 4, 8, 16
# the batched resend (include/uflow_frame_codec.h): a transmission record's flag, a connection's flag, why it stopped
UFC_TX_RESEND = 1
UFC_RS_NO_DATA_FLUSH = 1
(UFC_RS_DONE, UFC_RS_SIZE_LIMITED, UFC_RS_WINDOW_LIMITED, UFC_RS_REF_HANG, UFC_RS_BAD_STATE, UFC_RS_STAGE_FULL,
 UFC_RS_HEAP_FULL) = range(7)
# the batched flush control (include/uflow_flush_ctl.h): why an ack flush stopped, why no sync frame went out
UFC_FA_DONE, UFC_FA_BAD_STATE, UFC_FA_CARRY_FULL = 0, 1, 2
(UFC_FS_SENT, UFC_FS_ACK_LIMITED, UFC_FS_DATA_LIMITED, UFC_FS_UPSTREAM, UFC_FS_NOT_DUE, UFC_FS_IDLE,
 UFC_FS_NO_ALLOC) = range(7)
# the batched frame routing (include/uflow_route.h): a frame's class
UFC_ROUTE_DROP, UFC_ROUTE_CONN, UFC_ROUTE_CONTROL, UFC_ROUTE_DEFERRED = range(4)

# Every symbol the header declares, with its ctypes signature.
_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_V, _Z, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
# ufc_parse_batch_*: data, offsets, n, valid, infos, items, items_cap
_PARSE_ARGS = [_V, _V, _Z, _V, _V, _V, _Z]
# ufc_build_sizes_*: infos, items, n_items, src_base, payload_len, n, out_offsets, status
_BUILD_SIZES_ARGS = [_V, _V, _Z, _V, _Z, _Z, _V, _V]
# ufc_build_batch_*: infos, items, n_items, src_base, payload, payload_len, n, out_offsets, out, out_cap, seal, crc_out
_BUILD_ARGS = [_V, _V, _Z, _V, _V, _Z, _Z, _V, _V, _Z, _I, _V]
# ufc_pack_*: items, n_items, flush_first, flushes, n_flushes, nonce_bits, infos, frames_cap, results
_PACK_ARGS = [_V, _Z, _V, _V, _Z, _V, _V, _Z, _V]
# ufc_emit_packets_*: packets, n_packets, packet_first, senders, n_senders, items, items_cap, flush_first,
# packet_results, sender_results, senders_out
_EMIT_ARGS = [_V, _Z, _V, _V, _Z, _V, _Z, _V, _V, _V, _V]
_RX_ARGS = [_V, _Z, _V, _V, _Z, _V, _V, _Z, _V, _V, _Z, _V, _V, _Z, _V, _Z, _V, _Z, _V, _V, _V, _Z, _V, _V, _V, _Z, _V,
            _V, _V, _V]
_FW_ARGS = [_V, _Z, _V, _V, _Z, _V, _V, _Z, _V, _V, _V, _V]
_FQ_ARGS = [_V, _Z, _V, _Z, _V, _V, _Z, _V, _V, _V, _Z, _V, _Z, _V, _Z, _V, _V]
_RATE_BEGIN_ARGS = [_V, _V, _V, _Z, _V, _V]
# ufc_resend_begin_*: infos, n_frames, frame_first, queues, log, n_log, rate, flags, flushes, states, senders, n, heap,
# n_heap, pkts, n_pkts, frag_acked, n_frag, tx, n_tx, ref_acked, refs_cap, stage, n_stage, results, states_out,
# senders_out
_RS_BEGIN_ARGS = [_V, _Z, _V, _V, _V, _Z, _V, _V, _V, _V, _V, _Z, _V, _Z, _V, _Z, _V, _Z, _V, _Z, _V, _Z, _V, _Z, _V, _V,
                  _V]
# ufc_resend_place_*: states, begin_results, n, stage, n_stage, flush_first, items, items_cap
_RS_PLACE_ARGS = [_V, _V, _Z, _V, _Z, _V, _V, _Z]
# ufc_resend_commit_*: flush_results, infos, n_infos, out_offsets, frames_used, items, n_items, flush_first, packets,
# n_packets, packet_first, packet_results, sender_results, begin_results, rate, states, senders, n, heap, n_heap, pkts,
# n_pkts, frag_acked, n_frag, tx, n_tx, sent, sent_cap, sent_first, next_extra_flags, results, states_out, retake
_RS_COMMIT_ARGS = [_V, _V, _Z, _V, _V, _V, _Z, _V, _V, _Z, _V, _V, _V, _V, _V, _V, _V, _Z, _V, _Z, _V, _Z, _V, _Z, _V, _Z,
                   _V, _Z, _V, _V, _V, _V, _V]
_RATE_STEP_ARGS = [_V, _V, _V, _Z, _V, _Z, _V, _Z, _V, _V, _Z, _V, _V, _V]
# ufc_flush_acks_*: ctl, windows, groups, n_groups, group_first, receivers, rate, n, carry, n_carry, merged, merged_cap,
# merged_first, merged_used, infos, frames_cap, frames_used, results, ack_results, windows_out, ctl_out, flushes, flags
_FLUSH_ACKS_ARGS = [_V, _V, _V, _Z, _V, _V, _V, _Z, _V, _Z, _V, _Z, _V, _V, _V, _Z, _V, _V, _V, _V, _V, _V, _V]
# ufc_flush_sync_*: ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders, n, infos,
# syncs_cap, sync_index, syncs_used, results, ctl_out, ticks_next
_FLUSH_SYNC_ARGS = [_V, _V, _V, _V, _V, _V, _V, _V, _Z, _V, _Z, _V, _V, _V, _V, _V]
# ufc_route_frames_*: infos, addrs, offsets, n, slots, n_slots, seed, max_probe, n_conns, conn_active, now_ms,
# active_timeout_ms, timeout_in, route, cls, bucket_first, order, infos_out, src_base_out, results, timeout_out,
# first_unknown_control
_U32, _U64 = ctypes.c_uint32, ctypes.c_uint64
_ROUTE_ARGS = [_V, _V, _V, _Z, _V, _Z, _U32, _U32, _Z, _V, _U64, _U64, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]
_SIGNATURES = {
    "ufc_crc32_compute": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_size_t]),
    "ufc_crc32_extend": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "ufc_frame_validate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    "ufc_frame_seal": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    "ufc_device_count": (ctypes.c_int, []),
    "ufc_ctx_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    "ufc_ctx_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "ufc_ctx_release_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "ufc_ctx_last_hip_error": (ctypes.c_int, [ctypes.c_void_p]),
    "ufc_ctx_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "ufc_ctx_get_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "ufc_crc_batch_fixed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_crc_batch_varlen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_seal_batch_fixed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                            ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_seal_batch_varlen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_hbm_read_probe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                          ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]),
    "ufc_validate_host_varlen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_crc_batch_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_validate_host_slots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                               ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_validate_host_slots_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                     ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_seal_host_slots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p]),
    "ufc_seal_host_varlen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p]),
    "ufc_shard_range": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_uint64)]),
    "ufc_shard_chunk": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "ufc_shard_bounds_fixed": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]),
    "ufc_shard_bounds_varlen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]),
    "ufc_shard_nchunks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "ufc_shard_gather_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_int]),
    "ufc_comm_id_create": (ctypes.c_int, [ctypes.c_void_p]),
    "ufc_comm_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p]),
    "ufc_comm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "ufc_comm_last_error": (ctypes.c_int, [ctypes.c_void_p]),
    "ufc_comm_set_timeout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "ufc_crc_sharded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint64,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_crc_sharded_varlen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    # include/uflow_frame_codec.h
    "ufc_frame_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_size_t]),
    "ufc_frame_parse": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_size_t]),
    "ufc_datagram_is_valid": (ctypes.c_int, [ctypes.c_void_p]),
    "ufc_frame_write_fixed": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]),
    "ufc_data_frame_builder_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                                   ctypes.c_int]),
    "ufc_data_frame_builder_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "ufc_data_frame_encoded_size": (ctypes.c_size_t, [ctypes.c_void_p]),
    "ufc_ack_frame_builder_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                                  ctypes.c_uint32]),
    "ufc_ack_frame_builder_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]),
    "ufc_builder_size": (ctypes.c_size_t, [ctypes.c_void_p]),
    "ufc_builder_build": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int]),
    # each stage: the shared arguments, then its used count (where it has one), then nthreads (host) / ctx first and
    # stream last (device)
    "ufc_parse_batch_host": (_I, _PARSE_ARGS + [ctypes.POINTER(_Z), _I]),
    "ufc_parse_batch_varlen": (_I, [_V] + _PARSE_ARGS + [_V, _V]),
    "ufc_build_sizes_host": (_I, _BUILD_SIZES_ARGS + [_I]),
    "ufc_build_batch_host": (_I, _BUILD_ARGS + [_I]),
    "ufc_build_sizes_varlen": (_I, [_V] + _BUILD_SIZES_ARGS + [_V]),
    "ufc_build_batch_varlen": (_I, [_V] + _BUILD_ARGS + [_V]),
    "ufc_pack_host": (_I, _PACK_ARGS + [ctypes.POINTER(ctypes.c_uint64), _I]),
    "ufc_pack_varlen": (_I, [_V] + _PACK_ARGS + [_V, _V]),
    "ufc_emit_packets_host": (_I, _EMIT_ARGS + [ctypes.POINTER(ctypes.c_uint64), _I]),
    "ufc_emit_packets_varlen": (_I, [_V] + _EMIT_ARGS + [_V, _V]),
    # infos, n_frames, frame_accept, items, n_items, src_base, payload, payload_len, frame_first, receivers,
    # n_receivers, slots, slot_first, n_slots, carry_in, carry_in_len, carry_out, carry_cap, carry_first, carry_used,
    # packets, packets_cap, packet_first, packets_used, out_bytes, out_cap, out_used, item_status, results,
    # receivers_out, then nthreads (host) / ctx first and stream last (device)
    "ufc_receive_packets_host": (ctypes.c_int, _RX_ARGS + [ctypes.c_int]),
    "ufc_receive_packets_varlen": (ctypes.c_int, [ctypes.c_void_p] + _RX_ARGS + [ctypes.c_void_p]),
    # infos, n_frames, frame_first, windows, n_windows, frame_accept, groups, groups_cap, group_first, groups_used,
    # results, windows_out, then nthreads (host) / ctx first and stream last (device)
    "ufc_frame_window_host": (ctypes.c_int, _FW_ARGS + [ctypes.c_int]),
    "ufc_frame_window_varlen": (ctypes.c_int, [ctypes.c_void_p] + _FW_ARGS + [ctypes.c_void_p]),
    # infos, n_frames, items, n_items, frame_first, sent, n_sent, sent_first, queues, steps, n_queues, log, n_log,
    # ref_acked, refs_cap, results, queues_out, then nthreads (host) / ctx first and stream last (device)
    "ufc_frame_queue_host": (ctypes.c_int, _FQ_ARGS + [ctypes.c_int]),
    "ufc_frame_queue_varlen": (ctypes.c_int, [ctypes.c_void_p] + _FQ_ARGS + [ctypes.c_void_p]),
    # states, now_ms, extra_flags, n, steps, states_out, then nthreads (host) / ctx first and stream last (device)
    "ufc_rate_begin_host": (ctypes.c_int, _RATE_BEGIN_ARGS + [ctypes.c_int]),
    "ufc_rate_begin_varlen": (ctypes.c_int, [ctypes.c_void_p] + _RATE_BEGIN_ARGS + [ctypes.c_void_p]),
    # states, ticks, fq, n, entries, n_entries, flush_results, n_flush_results, result_index, flushes, n_flushes,
    # flush_index, results, states_out, then nthreads (host) / ctx first and stream last (device)
    "ufc_rate_step_host": (ctypes.c_int, _RATE_STEP_ARGS + [ctypes.c_int]),
    "ufc_rate_step_varlen": (ctypes.c_int, [ctypes.c_void_p] + _RATE_STEP_ARGS + [ctypes.c_void_p]),
    # then nthreads (host) / ctx first and stream last (device)
    "ufc_resend_begin_host": (ctypes.c_int, _RS_BEGIN_ARGS + [ctypes.c_int]),
    "ufc_resend_begin_varlen": (ctypes.c_int, [ctypes.c_void_p] + _RS_BEGIN_ARGS + [ctypes.c_void_p]),
    "ufc_resend_place_host": (ctypes.c_int, _RS_PLACE_ARGS + [ctypes.c_int]),
    "ufc_resend_place_varlen": (ctypes.c_int, [ctypes.c_void_p] + _RS_PLACE_ARGS + [ctypes.c_void_p]),
    "ufc_resend_commit_host": (ctypes.c_int, _RS_COMMIT_ARGS + [ctypes.c_int]),
    "ufc_resend_commit_varlen": (ctypes.c_int, [ctypes.c_void_p] + _RS_COMMIT_ARGS + [ctypes.c_void_p]),
}
SYMBOLS = tuple(_SIGNATURES)
# include/uflow_flush_ctl.h: the batched flush control's symbols, bound with the others in lib().
_FLUSH_SIGNATURES = {
    "ufc_flush_acks_host": (_I, _FLUSH_ACKS_ARGS + [_I]),
    "ufc_flush_acks_varlen": (_I, [_V] + _FLUSH_ACKS_ARGS + [_V]),
    "ufc_flush_sync_host": (_I, _FLUSH_SYNC_ARGS + [_I]),
    "ufc_flush_sync_varlen": (_I, [_V] + _FLUSH_SYNC_ARGS + [_V]),
}
FLUSH_SYMBOLS = tuple(_FLUSH_SIGNATURES)
# include/uflow_route.h: the batched frame routing's symbols, bound with the others in lib().
_ROUTE_SIGNATURES = {
    # addrs, n_conns, seed, slots, n_slots, max_probe, dup_index
    "ufc_route_table_build_host": (_I, [_V, _Z, _U32, _V, _Z, _V, _V]),
    "ufc_route_frames_host": (_I, _ROUTE_ARGS + [_I]),
    "ufc_route_frames_varlen": (_I, [_V] + _ROUTE_ARGS + [_V]),
}
ROUTE_SYMBOLS = tuple(_ROUTE_SIGNATURES)


# Structs of include/uflow_frame_codec.h the Python side instantiates (layouts checked against the
# header by tests/test_records_cpu.py; every other record is a numpy dtype in records.py).
class FrameInfo(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint8), ("ok", ctypes.c_uint8), ("aux", ctypes.c_uint8), ("crc_ok", ctypes.c_uint8),
                ("f", ctypes.c_uint32 * 5), ("item_count", ctypes.c_uint32), ("item_first", ctypes.c_uint32)]


class Item(ctypes.Structure):
    _fields_ = [("id", ctypes.c_uint32), ("channel_id", ctypes.c_uint8), ("form", ctypes.c_uint8),
                ("window_parent_lead", ctypes.c_uint16), ("channel_parent_lead", ctypes.c_uint16),
                ("fragment_id", ctypes.c_uint16), ("fragment_id_last", ctypes.c_uint16), ("flags", ctypes.c_uint16),
                ("data_offset", ctypes.c_uint32), ("data_len", ctypes.c_uint32)]


class Builder(ctypes.Structure):
    _fields_ = [("buf", ctypes.c_void_p), ("cap", ctypes.c_size_t), ("len", ctypes.c_size_t),
                ("count", ctypes.c_uint32), ("kind", ctypes.c_uint32)]


class Xfer(ctypes.Structure):
    """ufc_xfer: one operation of the multi-GPU gather plan (ufc_shard_gather_plan)."""
    _fields_ = [("op", ctypes.c_int32), ("peer", ctypes.c_int32), ("src", ctypes.c_uint64), ("dst", ctypes.c_uint64),
                ("count", ctypes.c_uint64)]


class DatagramRef(ctypes.Structure):
    _fields_ = [("sequence_id", ctypes.c_uint32), ("channel_id", ctypes.c_uint8), ("reserved", ctypes.c_uint8),
                ("window_parent_lead", ctypes.c_uint16), ("channel_parent_lead", ctypes.c_uint16),
                ("fragment_id", ctypes.c_uint16), ("fragment_id_last", ctypes.c_uint16),
                ("data", ctypes.c_void_p), ("data_len", ctypes.c_size_t)]

_lib = None


class NativeError(RuntimeError):
    def __init__(self, code, what=""):
        msg = _lib.ufc_error_string(code).decode() if _lib is not None else str(code)
        super().__init__(f"{what}: {msg} (code {code})" if what else f"{msg} (code {code})")
        self.code = code


def lib():
    """The loaded library (raises if libuflowcrc.so has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libuflowcrc.so not found at {LIB_PATH}: run `python -m uflow_amd._build` "
                              "(the native library is required; there is no CPU fallback)")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(_SIGNATURES.items()) + list(_FLUSH_SIGNATURES.items()) +
                                   list(_ROUTE_SIGNATURES.items())):
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what=""):
    if rc != UFC_OK:
        raise NativeError(rc, what)
    return rc
