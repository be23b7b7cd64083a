"""uflow's frame types and their Serialize surface, backed by libuflowcrc.so's native codec.

Mirrors the reference (lowquark/uflow v0.7.1):
    HandshakeSynFrame ... AckFrame, Frame      <- src/frame/mod.rs:4-148
    Frame.read(bytes) -> Frame | None          <- Serialize::read, src/frame/serial/mod.rs:674-706
    frame.write() -> bytes                     <- Serialize::write, src/frame/serial/mod.rs:708-720
    DataFrameBuilder, AckFrameBuilder          <- src/frame/serial/build.rs:47-256
and the batched receive-side parse that follows the batched CRC gate:
    parse_batch_host(bytes, offsets, valid)    <- Frame::read of every received datagram
    pack_host(items, flush_first, flushes)     <- DataFrameEmitter / AckFrameEmitter push + finalize,
                                                  src/half_connection/emit.rs:47-125, 170-211
    emit_packets_host(packets, packet_first, senders)
                                               <- PacketSender::emit_packet and fragmentation,
                                                  src/half_connection/packet_sender.rs:149-238
    receive_packets_host(infos, items, payload, frame_first, receivers, slots, slot_first, carry_in)
                                               <- PacketReceiver::handle_datagram / receive / resynchronize,
                                                  src/half_connection/packet_receiver/mod.rs:142-435
    frame_window_host(infos, frame_first, windows)
                                               <- FrameAckQueue::window_contains / mark_seen / resynchronize,
                                                  src/half_connection/frame_ack_queue.rs, as handle_data_frame and
                                                  handle_sync_frame call them (half_connection/mod.rs:132-152)
    frame_queue_host(infos, items, frame_first, sent, sent_first, queues, steps, log)
                                               <- FrameQueue::push / acknowledge_group / advance_transfer_window /
                                                  forget_frames / get_feedback, src/half_connection/frame_queue.rs
                                                  with reorder_buffer.rs and loss_rate.rs
    rate_begin_host(states, now_ms) / rate_step_host(states, ticks, fq_results, entries)
                                               <- SendRateComp::step / notify_frame_sent with RecvRateSet,
                                                  src/half_connection/send_rate.rs and recv_rate_set.rs, and
                                                  HalfConnection::step / fill_flush_alloc (mod.rs:165-215)
    resend_begin_host / resend_place_host / resend_commit_host
                                               <- PacketSender::acknowledge (packet_sender.rs:242-275), the resend and
                                                  pending queues and emit_data_frames (half_connection/mod.rs:335-432)
    (device-resident: uflow_amd.batch.FrameCrcEngine.parse_varlen)

None plays the role of Rust's None: a frame the reference rejects is returned as None, never
raised.  Decoding goes through ufc_frame_read (C++, frame_codec_core.hpp); there is no Python
fallback.
"""
import ctypes
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from ._native import (Builder, DatagramRef, Flush, FlushResult, FrameInfo, FrameQueue, FrameQueueResult, FrameQueueStep,
                      FrameWindow, FrameWindowResult, Item, Packet, PacketResult, RateResult, RateState, RateTick,
                      Receiver, ReceiverResult, RecvRateEntry, Resend, ResendCommitResult, ResendEntry, ResendResult,
                      RxPacket, RxSlot, SentFrame, SentPacket, Sender, SenderResult, TxRef, check, lib, UFC_ERR_NOMEM)

MAX_FRAME_SIZE = 1472  # src/lib.rs:286-294
DATA_FRAME_MAX_DATAGRAM_COUNT = 127  # serial/mod.rs:42
HANDSHAKE_SYN, HANDSHAKE_SYN_ACK, HANDSHAKE_ACK, HANDSHAKE_ERROR = 0, 1, 2, 3
DISCONNECT, DISCONNECT_ACK, DATA, SYNC, ACK = 4, 5, 10, 11, 12
HANDSHAKE_ERRORS = ("Version", "Config", "ServerFull")  # HandshakeErrorType, src/frame/mod.rs:30-35

# numpy views of ufc_frame_info / ufc_item (batched outputs)
FRAME_INFO_DTYPE = np.dtype([("kind", "u1"), ("ok", "u1"), ("aux", "u1"), ("crc_ok", "u1"), ("f", "<u4", (5,)),
                             ("item_count", "<u4"), ("item_first", "<u4")])
ITEM_DTYPE = np.dtype([("id", "<u4"), ("channel_id", "u1"), ("form", "u1"), ("window_parent_lead", "<u2"),
                       ("channel_parent_lead", "<u2"), ("fragment_id", "<u2"), ("fragment_id_last", "<u2"),
                       ("flags", "<u2"), ("data_offset", "<u4"), ("data_len", "<u4")])
assert FRAME_INFO_DTYPE.itemsize == ctypes.sizeof(FrameInfo) == 32
assert ITEM_DTYPE.itemsize == ctypes.sizeof(Item) == 24
# ufc_flush / ufc_flush_result (batched packs)
FLUSH_DTYPE = np.dtype([("flush_alloc", "<i8"), ("kind", "<u4"), ("window_room", "<u4"), ("id0", "<u4"), ("id1", "<u4")])
FLUSH_RESULT_DTYPE = np.dtype([("frame_first", "<u4"), ("frame_count", "<u4"), ("items_packed", "<u4"), ("stop", "<u4"),
                               ("alloc_left", "<i8")])
assert FLUSH_DTYPE.itemsize == ctypes.sizeof(Flush) == 24
assert FLUSH_RESULT_DTYPE.itemsize == ctypes.sizeof(FlushResult) == 24
PACK_DONE, PACK_SIZE_LIMITED, PACK_WINDOW_LIMITED, PACK_BAD_RANGE = 0, 1, 2, 3
# ufc_packet / ufc_sender / ufc_packet_result / ufc_sender_result (batched packet emits)
PACKET_DTYPE = np.dtype([("data_offset", "<u4"), ("data_len", "<u4"), ("flush_id", "<u4"), ("channel_id", "u1"),
                         ("mode", "u1"), ("reserved", "<u2")])
SENDER_DTYPE = np.dtype([("base_id", "<u4"), ("next_id", "<u4"), ("window_size", "<u4"), ("flush_id", "<u4"),
                         ("alloc", "<u8"), ("max_alloc", "<u8"), ("window_parent_id", "<u4"), ("take", "<u4"),
                         ("reserve_items", "<u4"), ("reserved", "<u4"), ("channel_parent_id", "<u4", (64,))])
PACKET_RESULT_DTYPE = np.dtype([("sequence_id", "<u4"), ("item_first", "<u4"), ("item_count", "<u4"), ("status", "u1"),
                                ("resend", "u1"), ("reserved", "<u2")])
SENDER_RESULT_DTYPE = np.dtype([("item_first", "<u4"), ("item_count", "<u4"), ("packets_consumed", "<u4"),
                                ("packets_emitted", "<u4"), ("packets_dropped", "<u4"), ("stop", "<u4"),
                                ("bytes_dropped", "<u8")])
assert PACKET_DTYPE.itemsize == ctypes.sizeof(Packet) == 16
assert SENDER_DTYPE.itemsize == ctypes.sizeof(Sender) == 304
assert PACKET_RESULT_DTYPE.itemsize == ctypes.sizeof(PacketResult) == 16
assert SENDER_RESULT_DTYPE.itemsize == ctypes.sizeof(SenderResult) == 32
SEND_TIME_SENSITIVE, SEND_UNRELIABLE, SEND_PERSISTENT, SEND_RELIABLE = 0, 1, 2, 3
NO_PARENT = 0xFFFFFFFF
EMIT_DONE, EMIT_WINDOW_LIMITED, EMIT_ALLOC_LIMITED, EMIT_BAD_PACKET, EMIT_BAD_RANGE = 0, 1, 2, 3, 4
PACKET_NOT_REACHED, PACKET_EMITTED, PACKET_DROPPED = 0, 1, 2
# ufc_receiver / ufc_rx_slot / ufc_rx_packet / ufc_receiver_result (batched packet receives)
RECEIVER_DTYPE = np.dtype([("base_id", "<u4"), ("end_id", "<u4"), ("window_size", "<u4"), ("window_ready", "u1"),
                           ("deliver", "u1"), ("reserved", "<u2"), ("resync_id", "<u4"), ("reserved2", "<u4"),
                           ("alloc", "<u8"), ("max_alloc", "<u8"), ("channel_ready_flags", "<u8"),
                           ("channel_base_id", "<u4", (64,)), ("channel_packet_count", "<u4", (64,))])
RX_SLOT_DTYPE = np.dtype([("data_offset", "<u8"), ("data_len", "<u4"), ("asm_size", "<u4"),
                          ("asm_window_parent_lead", "<u2"), ("asm_channel_parent_lead", "<u2"),
                          ("asm_last_fragment_id", "<u2"), ("asm_received", "<u2"), ("rx_window_parent_lead", "<u2"),
                          ("rx_channel_parent_lead", "<u2"), ("asm_state", "u1"), ("asm_channel_id", "u1"),
                          ("rx_channel_id", "u1"), ("rx_flags", "u1")])
RX_PACKET_DTYPE = np.dtype([("out_offset", "<u8"), ("sequence_id", "<u4"), ("len", "<u4"), ("channel_id", "u1"),
                            ("flags", "u1"), ("reserved", "<u2"), ("reserved2", "<u4")])
RECEIVER_RESULT_DTYPE = np.dtype([("packet_first", "<u4"), ("packet_count", "<u4"), ("status_count", "<u4", (11,)),
                                  ("packets_completed", "<u4"), ("packets_dud", "<u4"), ("advanced", "<u4"),
                                  ("stop", "<u4"), ("reserved", "<u4"), ("bytes_delivered", "<u8")])
assert RECEIVER_DTYPE.itemsize == ctypes.sizeof(Receiver) == 560
assert RX_SLOT_DTYPE.itemsize == ctypes.sizeof(RxSlot) == 32
assert RX_PACKET_DTYPE.itemsize == ctypes.sizeof(RxPacket) == 24
assert RECEIVER_RESULT_DTYPE.itemsize == ctypes.sizeof(ReceiverResult) == 80
RX_ASM_OPEN, RX_ASM_CLOSED, RX_ASM_ACTIVE = 0, 1, 2
RX_SLOT_ENTRY, RX_SLOT_DATA, RX_SLOT_DUD = 1, 2, 4
RX_PACKET_DUD = 1
(RX_NOT_HANDLED, RX_STORED, RX_COMPLETED, RX_DUD, RX_DROPPED_INVALID, RX_DROPPED_WINDOW, RX_DROPPED_CHANNEL,
 RX_DROPPED_CLOSED, RX_DROPPED_MISMATCH, RX_DROPPED_DUPLICATE, RX_DROPPED_BAD_SRC) = range(11)
RX_DONE, RX_BAD_STATE = 0, 1
# ufc_frame_window / ufc_frame_window_result (batched frame windows)
FRAME_WINDOW_DTYPE = np.dtype([("base_id", "<u4"), ("size", "<u4"), ("tail_base_id", "<u4"), ("tail_bitfield", "<u4"),
                               ("tail_nonce", "u1"), ("has_tail", "u1"), ("sync_reply", "u1"), ("reserved", "u1"),
                               ("reserved2", "<u4")])
FRAME_WINDOW_RESULT_DTYPE = np.dtype([("group_first", "<u4"), ("group_count", "<u4"), ("accepted", "<u4"),
                                      ("refused", "<u4"), ("syncs", "<u4"), ("packet_syncs", "<u4"),
                                      ("first_packet_sync", "<u4"), ("advanced", "<u4"), ("stop", "<u4"),
                                      ("reserved", "<u4")])
assert FRAME_WINDOW_DTYPE.itemsize == ctypes.sizeof(FrameWindow) == 24
assert FRAME_WINDOW_RESULT_DTYPE.itemsize == ctypes.sizeof(FrameWindowResult) == 40
FW_DONE, FW_BAD_STATE = 0, 1
# ufc_sent_frame / ufc_frame_queue / ufc_frame_queue_step / ufc_frame_queue_result (batched sender frame queues)
SENT_FRAME_DTYPE = np.dtype([("send_time_ms", "<u8"), ("size", "<u4"), ("ref_first", "<u4"), ("ref_count", "<u4"),
                             ("flags", "u1"), ("reserved", "u1", (3,))])
FRAME_QUEUE_DTYPE = np.dtype([("log_base_id", "<u4"), ("log_next_id", "<u4"), ("window_base_id", "<u4"),
                              ("window_size", "<u4"), ("tail_size", "<u4"), ("rb_base_id", "<u4"), ("rb_max_span", "<u4"),
                              ("rb_frames", "<u4", (2,)), ("rb_count", "<u4"), ("rate_limited", "u1"),
                              ("has_ack_data", "u1"), ("ack_rate_limited", "u1"), ("has_last_feedback", "u1"),
                              ("li_count", "<u4"), ("ack_last_send_time_ms", "<u8"), ("ack_total_size", "<u8"),
                              ("last_feedback_ms", "<u8"), ("li_end_time_ms", "<u8", (9,)), ("li_length", "<u4", (9,)),
                              ("log_cap", "<u4"), ("log_first", "<u8")])
FRAME_QUEUE_STEP_DTYPE = np.dtype([("flags", "<u4"), ("reserved", "<u4"), ("rtt_ms", "<u8"), ("thresh_ms", "<u8"),
                                   ("now_ms", "<u8"), ("reset_loss_rate", "<f8")])
FRAME_QUEUE_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("pushes_taken", "<u4"), ("pushes_refused", "<u4"),
                                     ("ack_frames", "<u4"), ("groups", "<u4"), ("groups_dud", "<u4"),
                                     ("groups_unknown", "<u4"), ("groups_bad_nonce", "<u4"), ("frames_acked", "<u4"),
                                     ("li_acks", "<u4"), ("li_nacks", "<u4"), ("window_advanced", "<u4"),
                                     ("log_culled", "<u4"), ("window_room", "<u4"), ("has_feedback", "u1"),
                                     ("rate_limited", "u1"), ("reserved", "<u2"), ("receive_rate", "<u4"),
                                     ("rtt_ms", "<u8"), ("loss_rate", "<f8")])
assert SENT_FRAME_DTYPE.itemsize == ctypes.sizeof(SentFrame) == 24
assert FRAME_QUEUE_DTYPE.itemsize == ctypes.sizeof(FrameQueue) == 192
assert FRAME_QUEUE_STEP_DTYPE.itemsize == ctypes.sizeof(FrameQueueStep) == 40
assert FRAME_QUEUE_RESULT_DTYPE.itemsize == ctypes.sizeof(FrameQueueResult) == 80
SENT_NONCE, SENT_RATE_LIMITED, SENT_ACKED, SENT_MARK = 1, 2, 4, 8
FQ_HAS_RTT, FQ_RESET_LOSS, FQ_MARK_RATE_LIMITED, FQ_FORGET, FQ_FEEDBACK = 1, 2, 4, 8, 16
FQ_DONE, FQ_BAD_STATE = 0, 1
# ufc_recv_rate_entry / ufc_rate_state / ufc_rate_tick / ufc_rate_result (batched send rate control)
RECV_RATE_ENTRY_DTYPE = np.dtype([("timestamp_ms", "<u8"), ("value", "<u4"), ("is_initial", "u1"),
                                  ("reserved", "u1", (3,))])
RATE_STATE_DTYPE = np.dtype([("mode", "<u4"), ("send_rate", "<u4"), ("max_send_rate", "<u4"), ("send_rate_tcp", "<u4"),
                             ("has_time_last_doubled", "u1"), ("has_nofeedback_exp", "u1"), ("nofeedback_idle", "u1"),
                             ("has_rtt_s", "u1"), ("has_rtt_ms", "u1"), ("has_rto_ms", "u1"), ("has_last_flush", "u1"),
                             ("has_reset", "u1"), ("time_last_doubled_ms", "<u8"), ("prev_loss_rate", "<f8"),
                             ("nofeedback_exp_ms", "<u8"), ("rtt_s", "<f8"), ("rtt_ms", "<u8"), ("rto_ms", "<u8"),
                             ("now_ms", "<u8"), ("flush_alloc", "<i8"), ("reset_loss_rate", "<f8"),
                             ("recv_first", "<u8"), ("recv_count", "<u4"), ("recv_cap", "<u4")])
RATE_TICK_DTYPE = np.dtype([("now_ms", "<u8"), ("delta_time_s", "<f8"), ("alloc_adjust", "<i8"), ("flags", "<u4"),
                            ("reserved", "<u4")])
RATE_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("mode", "<u4"), ("now_ms", "<u8"), ("rtt_ms", "<u8"), ("rto_ms", "<u8"),
                              ("flush_alloc", "<i8"), ("send_rate", "<u4"), ("flags", "<u4"), ("inv_iterations", "<u4"),
                              ("recv_count", "<u4")])
assert RECV_RATE_ENTRY_DTYPE.itemsize == ctypes.sizeof(RecvRateEntry) == 16
assert RATE_STATE_DTYPE.itemsize == ctypes.sizeof(RateState) == 112
assert RATE_TICK_DTYPE.itemsize == ctypes.sizeof(RateTick) == 32
assert RATE_RESULT_DTYPE.itemsize == ctypes.sizeof(RateResult) == 56
RATE_AWAIT_SEND, RATE_SLOW_START, RATE_THROUGHPUT_EQN = 0, 1, 2
RATE_FRAME_SENT = 1
RATE_DONE, RATE_BAD_STATE, RATE_REF_PANIC, RATE_RECV_FULL = 0, 1, 2, 3
RATE_FEEDBACK, RATE_NOFEEDBACK, RATE_RESET_ISSUED, RATE_ENTERED_EQN, RATE_INV_STALLED = 1, 2, 4, 8, 16
NO_INDEX = 0xFFFFFFFF  # UFC_NO_PARENT in result_index / flush_index: no gather for this connection
# ufc_resend_entry / ufc_sent_packet / ufc_tx_ref / ufc_resend / ufc_resend_result / ufc_resend_commit_result
RESEND_ENTRY_DTYPE = np.dtype([("resend_time_ms", "<u8"), ("sequence_id", "<u4"), ("fragment_id", "<u2"),
                               ("send_count", "u1"), ("reserved", "u1")])
SENT_PACKET_DTYPE = np.dtype([("data_offset", "<u4"), ("data_len", "<u4"), ("frag_first", "<u4"), ("sequence_id", "<u4"),
                              ("window_parent_lead", "<u2"), ("channel_parent_lead", "<u2"), ("channel_id", "u1"),
                              ("resend", "u1"), ("reserved", "<u2")])
TX_REF_DTYPE = np.dtype([("sequence_id", "<u4"), ("fragment_id", "<u2"), ("flags", "<u2")])
RESEND_DTYPE = np.dtype([("heap_first", "<u8"), ("heap_cap", "<u4"), ("heap_len", "<u4"), ("pkt_first", "<u8"),
                         ("pkt_cap", "<u4"), ("frag_next", "<u4"), ("frag_first", "<u8"), ("frag_cap", "<u4"),
                         ("tx_cap", "<u4"), ("tx_first", "<u8"), ("tx_head", "<u4"), ("tx_tail", "<u4"),
                         ("stage_first", "<u8"), ("stage_cap", "<u4"), ("pending_seq", "<u4"), ("pending_next", "<u4"),
                         ("pending_count", "<u4"), ("pending_resend", "u1"), ("reserved0", "u1"), ("reserved1", "<u2"),
                         ("reserved2", "<u4"), ("window_bytes", "<u8")])
RESEND_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("n_resent", "<u4"), ("n_pending_staged", "<u4"),
                                ("heap_popped_dead", "<u4"), ("heap_popped_acked", "<u4"), ("packets_freed", "<u4"),
                                ("refs_acked", "<u4"), ("heap_len", "<u4"), ("pending_count", "<u4"),
                                ("acks_ignored", "<u4"), ("bytes_freed", "<u8")])
RESEND_COMMIT_RESULT_DTYPE = np.dtype([("stop", "<u4"), ("pending_packed", "<u4"), ("packets_entered", "<u4"),
                                       ("heap_pushed", "<u4"), ("heap_dropped", "<u4"), ("refs_written", "<u4"),
                                       ("frames", "<u4"), ("take", "<u4"), ("heap_len", "<u4"), ("pending_count", "<u4")])
assert RESEND_ENTRY_DTYPE.itemsize == ctypes.sizeof(ResendEntry) == 16
assert SENT_PACKET_DTYPE.itemsize == ctypes.sizeof(SentPacket) == 24
assert TX_REF_DTYPE.itemsize == ctypes.sizeof(TxRef) == 8
assert RESEND_DTYPE.itemsize == ctypes.sizeof(Resend) == 104
assert RESEND_RESULT_DTYPE.itemsize == ctypes.sizeof(ResendResult) == 48
assert RESEND_COMMIT_RESULT_DTYPE.itemsize == ctypes.sizeof(ResendCommitResult) == 40
TX_RESEND = 1
RS_NO_DATA_FLUSH = 1
RS_DONE, RS_SIZE_LIMITED, RS_WINDOW_LIMITED, RS_REF_HANG, RS_BAD_STATE, RS_STAGE_FULL, RS_HEAP_FULL = range(7)
# The arenas of the resend state, in the order the C calls take them: name, record dtype.
RESEND_ARENAS = (("heap", RESEND_ENTRY_DTYPE), ("pkts", SENT_PACKET_DTYPE), ("frag_acked", np.dtype(np.uint8)),
                 ("tx", TX_REF_DTYPE), ("ref_acked", np.dtype(np.uint8)), ("stage", ITEM_DTYPE))


def _pow2_at_least(v: int) -> int:
    c = 1
    while c < v:
        c *= 2
    return c


def new_resend_states(n: int, window_size, max_alloc, frame_window_size, frame_tail_size, heap_cap: int,
                      stage_cap=None, pkt_cap=None, frag_cap=None, tx_cap=None):
    """n ufc_resend records of a new HalfConnection (empty heap, empty pending queue, nothing sent) and their arenas:
    returns (states, arenas), arenas a dict of numpy arrays heap, pkts, frag_acked, tx, ref_acked (one byte per tx
    record: what frame_queue marks) and stage.  Every connection's regions have the same capacities and lie back to
    back.  The defaults are the smallest capacities the header's bounds allow for a sender with window_size and
    max_alloc whose frame queue has frame_window_size and frame_tail_size.  stage_cap defaults to heap_cap + 65536,
    which covers a packet of any length but is 1.5 MB a connection: give heap_cap + the fragments of the longest
    packet that is sent (the header's sizing) wherever there are many connections."""
    frag = 1448
    rounded = (int(max_alloc) + frag - 1) // frag * frag
    pkt_cap = _pow2_at_least(int(window_size)) if pkt_cap is None else int(pkt_cap)
    frag_cap = _pow2_at_least(rounded // frag + int(window_size)) if frag_cap is None else int(frag_cap)
    tx_cap = _pow2_at_least((int(frame_window_size) + int(frame_tail_size) + 1) * 127) if tx_cap is None else int(tx_cap)
    stage_cap = int(heap_cap) + 65536 if stage_cap is None else int(stage_cap)
    s = np.zeros(n, dtype=RESEND_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    for name, cap in (("heap", heap_cap), ("pkt", pkt_cap), ("frag", frag_cap), ("tx", tx_cap), ("stage", stage_cap)):
        s[name + "_cap"] = cap
        s[name + "_first"] = idx * np.uint64(cap)
    arenas = {"heap": np.zeros(n * int(heap_cap), dtype=RESEND_ENTRY_DTYPE),
              "pkts": np.zeros(n * pkt_cap, dtype=SENT_PACKET_DTYPE),
              "frag_acked": np.zeros(n * frag_cap, dtype=np.uint8),
              "tx": np.zeros(n * tx_cap, dtype=TX_REF_DTYPE),
              "ref_acked": np.zeros(n * tx_cap, dtype=np.uint8),
              "stage": np.zeros(n * stage_cap, dtype=ITEM_DTYPE)}
    return s, arenas


def new_rate_states(n: int, max_send_rate, recv_cap: int):
    """n ufc_rate_state records equal to SendRateComp::new(max_send_rate) (send_rate.rs:119-137) inside a new
    HalfConnection (flush_alloc 0, now_ms 0, never flushed) and their entry arena: returns (states, entries).  Every
    connection's RecvRateSet has room for recv_cap entries; the rooms lie back to back, recv_first = c * recv_cap."""
    if int(recv_cap) < 1:
        raise ValueError("recv_cap must be at least 1")
    s = np.zeros(n, dtype=RATE_STATE_DTYPE)
    s["mode"] = RATE_AWAIT_SEND
    s["send_rate"] = MAX_FRAME_SIZE
    s["max_send_rate"] = max_send_rate
    s["recv_cap"] = recv_cap
    s["recv_first"] = np.arange(n, dtype=np.uint64) * np.uint64(recv_cap)
    return s, np.zeros(n * int(recv_cap), dtype=RECV_RATE_ENTRY_DTYPE)


def new_frame_queues(n: int, window_size, tail_size, base_id=0, log_cap=None):
    """n ufc_frame_queue records equal to FrameQueue::new(window_size, tail_size, base_id) (frame_queue.rs:218-226)
    and their log arena: returns (queues, log).  log_cap (a power of two, default the smallest one holding
    window_size + tail_size) is every connection's ring size; the rings lie back to back, log_first = c * log_cap."""
    span = int(window_size) + int(tail_size)
    if log_cap is None:
        log_cap = 1
        while log_cap < span:
            log_cap *= 2
    log_cap = int(log_cap)
    if log_cap < max(span, 1) or log_cap & (log_cap - 1) or log_cap > 1 << 31:
        raise ValueError("log_cap must be a power of two of at least window_size + tail_size")
    q = np.zeros(n, dtype=FRAME_QUEUE_DTYPE)
    for k in ("log_base_id", "log_next_id", "window_base_id", "rb_base_id"):
        q[k] = base_id
    q["window_size"] = window_size
    q["tail_size"] = tail_size
    q["rb_max_span"] = span
    q["log_cap"] = log_cap
    q["log_first"] = np.arange(n, dtype=np.uint64) * np.uint64(log_cap)
    return q, np.zeros(n * log_cap, dtype=SENT_FRAME_DTYPE)


def new_frame_windows(n: int, size, base_id=0) -> np.ndarray:
    """n ufc_frame_window records equal to FrameAckQueue::new(size, base_id) (frame_ack_queue.rs:39-44): no pending
    ack group, no sync reply owed."""
    w = np.zeros(n, dtype=FRAME_WINDOW_DTYPE)
    w["base_id"] = base_id
    w["size"] = size
    return w


def new_receivers(n: int, window_size, base_id=0, max_alloc=1 << 40) -> np.ndarray:
    """n ufc_receiver headers equal to PacketReceiver::new(window_size, base_id, max_alloc) (mod.rs:94-136), to
    go with all-zero slots: deliver = 1, no resynchronize."""
    r = np.zeros(n, dtype=RECEIVER_DTYPE)
    r["base_id"] = r["end_id"] = base_id
    r["window_size"] = window_size
    r["max_alloc"] = max_alloc
    r["deliver"] = 1
    r["resync_id"] = NO_PARENT
    r["channel_base_id"] = NO_PARENT
    return r


@dataclass
class HandshakeSynFrame:
    version: int
    nonce: int
    max_receive_rate: int
    max_packet_size: int
    max_receive_alloc: int


@dataclass
class HandshakeSynAckFrame:
    nonce_ack: int
    nonce: int
    max_receive_rate: int
    max_packet_size: int
    max_receive_alloc: int


@dataclass
class HandshakeAckFrame:
    nonce_ack: int


@dataclass
class HandshakeErrorFrame:
    nonce_ack: int
    error: str  # "Version" | "Config" | "ServerFull"


@dataclass
class DisconnectFrame:
    pass


@dataclass
class DisconnectAckFrame:
    pass


@dataclass
class Datagram:
    sequence_id: int
    channel_id: int
    window_parent_lead: int
    channel_parent_lead: int
    fragment_id: int
    fragment_id_last: int
    data: bytes


@dataclass
class DataFrame:
    sequence_id: int
    nonce: bool
    datagrams: List[Datagram] = field(default_factory=list)


@dataclass
class SyncFrame:
    next_frame_id: Optional[int]
    next_packet_id: Optional[int]


@dataclass
class AckGroup:
    base_id: int
    bitfield: int
    nonce: bool


@dataclass
class AckFrame:
    frame_window_base_id: int
    packet_window_base_id: int
    frame_acks: List[AckGroup] = field(default_factory=list)


MAX_FRAGMENT_SIZE = 1448  # src/lib.rs:297


def datagram_is_valid(dg: Datagram) -> bool:
    """src/half_connection/packet_receiver/mod.rs:12-30 (through ufc_datagram_is_valid)."""
    it = Item()
    it.channel_id = dg.channel_id & 0xFF
    it.window_parent_lead = dg.window_parent_lead & 0xFFFF
    it.channel_parent_lead = dg.channel_parent_lead & 0xFFFF
    it.fragment_id = dg.fragment_id & 0xFFFF
    it.fragment_id_last = dg.fragment_id_last & 0xFFFF
    it.data_len = len(dg.data)
    rc = lib().ufc_datagram_is_valid(ctypes.byref(it))
    if rc < 0:
        check(rc, "ufc_datagram_is_valid")
    return rc == 1


def _u8buf(data):
    data = bytes(data)
    return ctypes.create_string_buffer(data, len(data)), len(data)


def _frame_from_info(info, items, fb: bytes):
    k, f = info.kind, list(info.f)
    if k == HANDSHAKE_SYN:
        return HandshakeSynFrame(info.aux, f[0], f[1], f[2], f[3])
    if k == HANDSHAKE_SYN_ACK:
        return HandshakeSynAckFrame(*f)
    if k == HANDSHAKE_ACK:
        return HandshakeAckFrame(f[0])
    if k == HANDSHAKE_ERROR:
        return HandshakeErrorFrame(f[0], HANDSHAKE_ERRORS[info.aux])
    if k == DISCONNECT:
        return DisconnectFrame()
    if k == DISCONNECT_ACK:
        return DisconnectAckFrame()
    if k == DATA:
        return DataFrame(f[0], bool(info.aux), [
            Datagram(it.id, it.channel_id, it.window_parent_lead, it.channel_parent_lead, it.fragment_id,
                     it.fragment_id_last, fb[it.data_offset:it.data_offset + it.data_len]) for it in items])
    if k == SYNC:
        return SyncFrame(f[0] if info.aux & 1 else None, f[1] if info.aux & 2 else None)
    if k == ACK:
        return AckFrame(f[0], f[1], [AckGroup(it.id, it.data_offset, bool(it.channel_id)) for it in items])
    raise AssertionError(k)


class Frame:
    """Serialize for every frame kind (serial/mod.rs:669-721)."""

    @staticmethod
    def read(frame_bytes) -> Optional[object]:
        fb = bytes(frame_bytes)
        buf, n = _u8buf(fb)
        info = FrameInfo()
        cap = 1024
        items = (Item * cap)()
        rc = lib().ufc_frame_read(buf, n, ctypes.byref(info), items, cap)
        if rc == UFC_ERR_NOMEM:
            cap = info.item_count
            items = (Item * cap)()
            rc = lib().ufc_frame_read(buf, n, ctypes.byref(info), items, cap)
        if rc < 0:
            check(rc, "ufc_frame_read")
        if rc == 0:
            return None
        return _frame_from_info(info, list(items[:info.item_count]), fb)

    @staticmethod
    def write(frame) -> bytes:
        if isinstance(frame, DataFrame):
            b = DataFrameBuilder(frame.sequence_id, frame.nonce)
            for d in frame.datagrams:
                b.add(d)
            return b.build()
        if isinstance(frame, AckFrame):
            b = AckFrameBuilder(frame.frame_window_base_id, frame.packet_window_base_id)
            for a in frame.frame_acks:
                b.add(a)
            return b.build()
        info = FrameInfo()
        if isinstance(frame, HandshakeSynFrame):
            info.kind, info.aux = HANDSHAKE_SYN, frame.version
            info.f[:4] = [frame.nonce, frame.max_receive_rate, frame.max_packet_size, frame.max_receive_alloc]
        elif isinstance(frame, HandshakeSynAckFrame):
            info.kind = HANDSHAKE_SYN_ACK
            info.f[:] = [frame.nonce_ack, frame.nonce, frame.max_receive_rate, frame.max_packet_size,
                         frame.max_receive_alloc]
        elif isinstance(frame, HandshakeAckFrame):
            info.kind, info.f[0] = HANDSHAKE_ACK, frame.nonce_ack
        elif isinstance(frame, HandshakeErrorFrame):
            info.kind, info.f[0], info.aux = HANDSHAKE_ERROR, frame.nonce_ack, HANDSHAKE_ERRORS.index(frame.error)
        elif isinstance(frame, DisconnectFrame):
            info.kind = DISCONNECT
        elif isinstance(frame, DisconnectAckFrame):
            info.kind = DISCONNECT_ACK
        elif isinstance(frame, SyncFrame):
            info.kind = SYNC
            info.aux = (1 if frame.next_frame_id is not None else 0) | (2 if frame.next_packet_id is not None else 0)
            info.f[0], info.f[1] = frame.next_frame_id or 0, frame.next_packet_id or 0
        else:
            raise TypeError(type(frame))
        out = ctypes.create_string_buffer(MAX_FRAME_SIZE)
        n = lib().ufc_frame_write_fixed(ctypes.byref(info), out, MAX_FRAME_SIZE, 1)
        if n == 0:
            raise ValueError("unencodable frame")
        return out.raw[:n]


class DataFrameBuilder:
    """build.rs:47-181 over a native buffer (the caller's Vec<u8> of the reference)."""
    MAX_COUNT = DATA_FRAME_MAX_DATAGRAM_COUNT

    def __init__(self, sequence_id: int, nonce: bool, capacity: int = 1 << 17):
        self._buf = ctypes.create_string_buffer(capacity)
        self._b = Builder()
        check(lib().ufc_data_frame_builder_init(ctypes.byref(self._b), self._buf, capacity, sequence_id & 0xFFFFFFFF,
                                                1 if nonce else 0), "DataFrameBuilder.new")
        self._keep = []

    @staticmethod
    def _ref(d: Datagram):
        data = bytes(d.data)
        cbuf = ctypes.create_string_buffer(data, max(len(data), 1))
        r = DatagramRef(d.sequence_id, d.channel_id, 0, d.window_parent_lead, d.channel_parent_lead, d.fragment_id,
                        d.fragment_id_last, ctypes.cast(cbuf, ctypes.c_void_p), len(data))
        return r, cbuf

    def add(self, d: Datagram):
        r, cbuf = self._ref(d)
        check(lib().ufc_data_frame_builder_add(ctypes.byref(self._b), ctypes.byref(r)), "DataFrameBuilder.add")

    @staticmethod
    def encoded_size(d: Datagram) -> int:
        r, _ = DataFrameBuilder._ref(d)
        return lib().ufc_data_frame_encoded_size(ctypes.byref(r))

    def count(self) -> int:
        return self._b.count

    def size(self) -> int:
        return lib().ufc_builder_size(ctypes.byref(self._b))

    def build(self, seal: bool = True) -> bytes:
        n = lib().ufc_builder_build(ctypes.byref(self._b), 1 if seal else 0)
        return self._buf.raw[:n]


class AckFrameBuilder:
    """build.rs:183-256."""

    def __init__(self, frame_window_base_id: int, packet_window_base_id: int, capacity: int = 1 << 17):
        self._buf = ctypes.create_string_buffer(capacity)
        self._b = Builder()
        check(lib().ufc_ack_frame_builder_init(ctypes.byref(self._b), self._buf, capacity, frame_window_base_id,
                                               packet_window_base_id), "AckFrameBuilder.new")

    def add(self, a: AckGroup):
        check(lib().ufc_ack_frame_builder_add(ctypes.byref(self._b), a.base_id & 0xFFFFFFFF, a.bitfield & 0xFFFFFFFF,
                                              1 if a.nonce else 0), "AckFrameBuilder.add")

    def size(self) -> int:
        return lib().ufc_builder_size(ctypes.byref(self._b))

    def build(self, seal: bool = True) -> bytes:
        n = lib().ufc_builder_build(ctypes.byref(self._b), 1 if seal else 0)
        return self._buf.raw[:n]


def parse_batch_host(data: np.ndarray, offsets: np.ndarray, valid: Optional[np.ndarray] = None, nthreads: int = 1):
    """Frame::read of every frame of a CSR batch in host memory, after the batched CRC gate
    (`valid`, from the GPU; None = gate on the host).  Returns (infos[n], items) as numpy
    structured arrays (FRAME_INFO_DTYPE, ITEM_DTYPE); infos['item_first'] indexes items."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    infos = np.zeros(max(n, 0), dtype=FRAME_INFO_DTYPE)
    if valid is not None:
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
    used = ctypes.c_size_t(0)
    vp = valid.ctypes.data if valid is not None else None
    rc = lib().ufc_parse_batch_host(data.ctypes.data, offsets.ctypes.data, n, vp, infos.ctypes.data, None, 0,
                                    ctypes.byref(used), nthreads)
    check(rc, "ufc_parse_batch_host")
    items = np.zeros(used.value, dtype=ITEM_DTYPE)
    rc = lib().ufc_parse_batch_host(data.ctypes.data, offsets.ctypes.data, n, vp, infos.ctypes.data,
                                    items.ctypes.data, items.size, ctypes.byref(used), nthreads)
    check(rc, "ufc_parse_batch_host")
    return infos, items


def build_batch_host(infos: np.ndarray, items: np.ndarray, payload: np.ndarray, src_base: Optional[np.ndarray] = None,
                     seal: bool = True, nthreads: int = 1):
    """Frame::write of every frame the records describe (what parse_batch_host returns), in host memory:
    ufc_build_sizes_host then ufc_build_batch_host.  Datagram payloads come from `payload` at
    src_base[i] + data_offset (src_base uint64[n], default zeros; a parsed batch's own offsets and bytes
    re-emit it).  Returns (out_bytes uint8, out_offsets uint64[n + 1], status uint8[n], crc uint32[n]);
    frames whose status is not UFC_BUILD_OK have length 0; seal=False leaves 4 zero bytes as trailers."""
    infos = np.ascontiguousarray(infos, dtype=FRAME_INFO_DTYPE)
    items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    n = infos.size
    sb = None
    if src_base is not None:
        src_base = np.ascontiguousarray(src_base, dtype=np.uint64)
        if src_base.size < n:
            raise ValueError("src_base must hold one offset per frame")
        sb = src_base.ctypes.data
    offsets = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    crc = np.zeros(n, dtype=np.uint32)
    ip = items.ctypes.data if items.size else None
    check(lib().ufc_build_sizes_host(infos.ctypes.data, ip, items.size, sb, payload.size, n, offsets.ctypes.data,
                                     status.ctypes.data, nthreads), "ufc_build_sizes_host")
    out = np.zeros(int(offsets[n]), dtype=np.uint8)
    check(lib().ufc_build_batch_host(infos.ctypes.data, ip, items.size, sb, payload.ctypes.data if payload.size else None,
                                     payload.size, n, offsets.ctypes.data, out.ctypes.data if out.size else None, out.size,
                                     1 if seal else 0, crc.ctypes.data, nthreads), "ufc_build_batch_host")
    return out, offsets, status, crc


def pack_host(items: np.ndarray, flush_first: np.ndarray, flushes: np.ndarray, frames_cap: Optional[int] = None,
              nonce_bits: Optional[np.ndarray] = None, nthreads: int = 1, infos: Optional[np.ndarray] = None):
    """The emitters' push / finalize of many flushes in host memory (ufc_pack_host): flush j owns
    items[flush_first[j] : flush_first[j + 1]] (ITEM_DTYPE records in push order, flush_first uint64[n + 1]) with
    the limits of flushes[j] (FLUSH_DTYPE).  Returns (infos, results, frames_used): the frames' FRAME_INFO_DTYPE
    records in flush order, as build_batch_host takes them (rows from frames_used on stay as they were: zero,
    which the builds skip), one FLUSH_RESULT_DTYPE record per flush, and the number of frames.  frames_cap
    (default: the number of items, always enough) bounds the records written; nonce_bits: uint32 words, bit g
    the nonce of the batch's g-th frame (default 0); infos: an array to write into."""
    items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
    flush_first = np.ascontiguousarray(flush_first, dtype=np.uint64)
    flushes = np.ascontiguousarray(flushes, dtype=FLUSH_DTYPE)
    n = flushes.size
    if flush_first.size < n + 1:
        raise ValueError("flush_first must hold one more entry than there are flushes")
    if frames_cap is None:
        frames_cap = items.size if infos is None else infos.size
    if infos is None:
        infos = np.zeros(frames_cap, dtype=FRAME_INFO_DTYPE)
    elif infos.dtype != FRAME_INFO_DTYPE or not infos.flags.c_contiguous or infos.size < frames_cap:
        raise ValueError("infos must be a contiguous FRAME_INFO_DTYPE array of at least frames_cap records")
    nb = None
    if nonce_bits is not None:
        nonce_bits = np.ascontiguousarray(nonce_bits, dtype=np.uint32)
        if nonce_bits.size * 32 < frames_cap:
            raise ValueError("nonce_bits must hold one bit per frame below frames_cap")
        nb = nonce_bits.ctypes.data
    results = np.zeros(n, dtype=FLUSH_RESULT_DTYPE)
    used = ctypes.c_uint64(0)
    check(lib().ufc_pack_host(items.ctypes.data if items.size else None, items.size, flush_first.ctypes.data,
                              flushes.ctypes.data if n else None, n, nb, infos.ctypes.data if frames_cap else None,
                              frames_cap, results.ctypes.data if n else None, ctypes.byref(used), nthreads),
          "ufc_pack_host")
    return infos, results, used.value


def emit_packets_host(packets: np.ndarray, packet_first: np.ndarray, senders: np.ndarray, items_cap: Optional[int] = None,
                      nthreads: int = 1, items: Optional[np.ndarray] = None, senders_out: Optional[np.ndarray] = None,
                      want_packet_results: bool = True):
    """PacketSender::emit_packet and fragmentation for many senders in host memory (ufc_emit_packets_host): sender
    s (SENDER_DTYPE: its PacketSender state, take and reserve_items) owns packets[packet_first[s] :
    packet_first[s + 1]] (PACKET_DTYPE records in queue order, packet_first uint64[n + 1]).  Returns (items,
    flush_first, packet_results, sender_results, senders_out, items_used): the fragments' ITEM_DTYPE records with
    the uint64 CSR over them that pack_host takes as its flush_first (each sender's reserve_items slots in front
    of its new items are left as they were), one PACKET_RESULT_DTYPE record per packet (None without
    want_packet_results), one SENDER_RESULT_DTYPE record per sender, and the senders' state after the packets they
    consumed.  items_cap bounds the items written (default: what the call needs, found by a first call with
    none); items: an array to write into; senders_out: where the state goes (may be `senders` itself)."""
    packets = np.ascontiguousarray(packets, dtype=PACKET_DTYPE)
    packet_first = np.ascontiguousarray(packet_first, dtype=np.uint64)
    if senders.dtype != SENDER_DTYPE or not senders.flags.c_contiguous:
        senders = np.ascontiguousarray(senders, dtype=SENDER_DTYPE)
    n = senders.size
    if packet_first.size < n + 1:
        raise ValueError("packet_first must hold one more entry than there are senders")
    if senders_out is None:
        senders_out = np.zeros(n, dtype=SENDER_DTYPE)
    elif senders_out.dtype != SENDER_DTYPE or not senders_out.flags.c_contiguous or senders_out.size < n:
        raise ValueError("senders_out must be a contiguous SENDER_DTYPE array of one record per sender")
    flush_first = np.zeros(n + 1, dtype=np.uint64)
    packet_results = np.zeros(packets.size, dtype=PACKET_RESULT_DTYPE) if want_packet_results else None
    sender_results = np.zeros(n, dtype=SENDER_RESULT_DTYPE)
    used = ctypes.c_uint64(0)

    def call(items_p, cap):
        check(lib().ufc_emit_packets_host(packets.ctypes.data if packets.size else None, packets.size,
                                          packet_first.ctypes.data, senders.ctypes.data if n else None, n, items_p, cap,
                                          flush_first.ctypes.data, packet_results.ctypes.data
                                          if want_packet_results and packets.size else None,
                                          sender_results.ctypes.data if n else None,
                                          senders_out.ctypes.data if n else None, ctypes.byref(used), nthreads),
              "ufc_emit_packets_host")

    if items_cap is None:
        if items is not None:
            items_cap = items.size
        elif senders_out is senders or np.shares_memory(senders_out, senders):
            raise ValueError("give items_cap (or items) when the state is updated in place")
        else:
            call(None, 0)
            items_cap = used.value
    if items is None:
        items = np.zeros(items_cap, dtype=ITEM_DTYPE)
    elif items.dtype != ITEM_DTYPE or not items.flags.c_contiguous or items.size < items_cap:
        raise ValueError("items must be a contiguous ITEM_DTYPE array of at least items_cap records")
    call(items.ctypes.data if items_cap else None, items_cap)
    return items, flush_first, packet_results, sender_results, senders_out, used.value


def receive_packets_host(infos: np.ndarray, items: np.ndarray, payload: np.ndarray, frame_first: np.ndarray,
                         receivers: np.ndarray, slots: np.ndarray, slot_first: np.ndarray, carry_in: np.ndarray,
                         src_base: Optional[np.ndarray] = None, frame_accept: Optional[np.ndarray] = None,
                         carry_cap: Optional[int] = None, out_cap: Optional[int] = None,
                         packets_cap: Optional[int] = None, nthreads: int = 1, receivers_out: Optional[np.ndarray] = None,
                         want_item_status: bool = True, carry_out: Optional[np.ndarray] = None,
                         out_bytes: Optional[np.ndarray] = None, packets: Optional[np.ndarray] = None):
    """One step of PacketReceiver for many receivers in host memory (ufc_receive_packets_host): receiver r
    (RECEIVER_DTYPE: its state, resync_id and deliver) owns frames frame_first[r] : frame_first[r + 1] of infos
    (FRAME_INFO_DTYPE, with their ITEM_DTYPE items; src_base uint64[n_frames] and payload as in build_host) and the
    slots slot_first[r] : slot_first[r] + window_size (RX_SLOT_DTYPE, updated in place).  carry_in uint8: the carry
    arena the slots point into.  Returns a dict: packets (RX_PACKET_DTYPE), packet_first, packets_used, out_bytes,
    out_used, carry_out, carry_first, carry_used, item_status (uint8 per item, or None), results
    (RECEIVER_RESULT_DTYPE), receivers_out.  Caps that are not given are what the step needs, found by a first
    pass on a copy of the state with caps of zero (an ACTIVE slot holds its whole fragment buffer, so the carry
    has no small bound from the batch's sizes alone); arrays given for carry_out, out_bytes and packets are written
    into (their sizes are then the caps).  Pass carry_out as the next step's carry_in."""
    infos = np.ascontiguousarray(infos, dtype=FRAME_INFO_DTYPE)
    items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    carry_in = np.ascontiguousarray(carry_in, dtype=np.uint8)
    frame_first = np.ascontiguousarray(frame_first, dtype=np.uint64)
    slot_first = np.ascontiguousarray(slot_first, dtype=np.uint64)
    if receivers.dtype != RECEIVER_DTYPE or not receivers.flags.c_contiguous:
        receivers = np.ascontiguousarray(receivers, dtype=RECEIVER_DTYPE)
    if slots.dtype != RX_SLOT_DTYPE or not slots.flags.c_contiguous or not slots.flags.writeable:
        raise ValueError("slots must be a writable contiguous RX_SLOT_DTYPE array (it is updated in place)")
    n = receivers.size
    if frame_first.size < n + 1 or slot_first.size < n + 1:
        raise ValueError("frame_first and slot_first must hold one more entry than there are receivers")
    if src_base is not None:
        src_base = np.ascontiguousarray(src_base, dtype=np.uint64)
        if src_base.size < infos.size:
            raise ValueError("src_base must hold one entry per frame")
    if frame_accept is not None:
        frame_accept = np.ascontiguousarray(frame_accept, dtype=np.uint8)
        if frame_accept.size < infos.size:
            raise ValueError("frame_accept must hold one entry per frame")
    if receivers_out is None:
        receivers_out = np.zeros(n, dtype=RECEIVER_DTYPE)
    elif receivers_out.dtype != RECEIVER_DTYPE or not receivers_out.flags.c_contiguous or receivers_out.size < n:
        raise ValueError("receivers_out must be a contiguous RECEIVER_DTYPE array of one record per receiver")
    carry_first = np.zeros(n + 1, dtype=np.uint64)
    packet_first = np.zeros(n + 1, dtype=np.uint64)
    results = np.zeros(n, dtype=RECEIVER_RESULT_DTYPE)
    carry_used, packets_used, out_used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def p(a):
        return a.ctypes.data if a is not None and a.size else None

    def call(slots_, carry_out_, out_bytes_, packets_, status_, receivers_out_):
        size = lambda a: 0 if a is None else a.size  # noqa: E731
        check(lib().ufc_receive_packets_host(
            p(infos), infos.size, p(frame_accept), p(items), items.size, p(src_base), p(payload), payload.size,
            frame_first.ctypes.data, p(receivers), n, p(slots_), slot_first.ctypes.data, slots_.size, p(carry_in),
            carry_in.size, p(carry_out_), size(carry_out_), carry_first.ctypes.data, ctypes.addressof(carry_used),
            p(packets_), size(packets_), packet_first.ctypes.data, ctypes.addressof(packets_used), p(out_bytes_),
            size(out_bytes_), ctypes.addressof(out_used), p(status_), p(results), p(receivers_out_), nthreads),
            "ufc_receive_packets_host")

    need = [(carry_out, carry_cap), (out_bytes, out_cap), (packets, packets_cap)]
    if any(arr is None and cap is None for arr, cap in need):
        # the used counts are exact whatever the caps: a first pass on a copy of the state, with none
        call(slots.copy(), None, None, None, None, np.zeros(n, dtype=RECEIVER_DTYPE))
        carry_cap = carry_used.value if carry_cap is None else carry_cap
        out_cap = out_used.value if out_cap is None else out_cap
        packets_cap = packets_used.value if packets_cap is None else packets_cap
    if carry_out is None:
        carry_out = np.zeros(int(carry_cap), dtype=np.uint8)
    if out_bytes is None:
        out_bytes = np.zeros(int(out_cap), dtype=np.uint8)
    if packets is None:
        packets = np.zeros(int(packets_cap), dtype=RX_PACKET_DTYPE)
    for name, arr, dt in (("carry_out", carry_out, np.uint8), ("out_bytes", out_bytes, np.uint8),
                          ("packets", packets, RX_PACKET_DTYPE)):
        if arr.dtype != dt or not arr.flags.c_contiguous or not arr.flags.writeable:
            raise ValueError(f"{name} must be a writable contiguous {dt} array")
    if np.shares_memory(carry_out, carry_in):
        raise ValueError("carry_out must not overlap carry_in")
    item_status = np.zeros(items.size, dtype=np.uint8) if want_item_status else None
    call(slots, carry_out, out_bytes, packets, item_status, receivers_out)
    return {"packets": packets, "packet_first": packet_first, "packets_used": packets_used.value,
            "out_bytes": out_bytes, "out_used": out_used.value, "carry_out": carry_out, "carry_first": carry_first,
            "carry_used": carry_used.value, "item_status": item_status, "results": results,
            "receivers_out": receivers_out}


def frame_window_host(infos: np.ndarray, frame_first: np.ndarray, windows: np.ndarray, groups_cap: Optional[int] = None,
                      nthreads: int = 1, frame_accept: Optional[np.ndarray] = None, groups: Optional[np.ndarray] = None,
                      group_first: Optional[np.ndarray] = None, results: Optional[np.ndarray] = None,
                      windows_out: Optional[np.ndarray] = None):
    """One step of FrameAckQueue for many connections in host memory (ufc_frame_window_host): connection r
    (FRAME_WINDOW_DTYPE: its ReceiveWindow, the last pending ack group and sync_reply) owns frames frame_first[r] :
    frame_first[r + 1] of infos (FRAME_INFO_DTYPE, what the parse returns) in arrival order.  Returns a dict:
    frame_accept (uint8 per frame: 1 for the data frames inside the window, what receive_packets_host takes as
    its frame_accept), groups (ITEM_DTYPE ack groups, the carried tail first), group_first (uint64 CSR over them:
    pack_host's flush_first), groups_used, results (FRAME_WINDOW_RESULT_DTYPE), windows_out.  groups_cap bounds
    the groups written (default n_windows + n_frames, always enough); arrays given for frame_accept, groups,
    group_first, results and windows_out (which may be `windows`) are written into."""
    infos = np.ascontiguousarray(infos, dtype=FRAME_INFO_DTYPE)
    frame_first = np.ascontiguousarray(frame_first, dtype=np.uint64)
    if windows.dtype != FRAME_WINDOW_DTYPE or not windows.flags.c_contiguous:
        windows = np.ascontiguousarray(windows, dtype=FRAME_WINDOW_DTYPE)
    n = windows.size
    if frame_first.size < n + 1:
        raise ValueError("frame_first must hold one more entry than there are windows")
    if groups_cap is None:
        groups_cap = groups.size if groups is not None else n + infos.size
    groups_cap = int(groups_cap)

    def out(name, arr, size, dt):
        if arr is None:
            return np.zeros(size, dtype=dt)
        if arr.dtype != dt or not arr.flags.c_contiguous or not arr.flags.writeable or arr.size < size:
            raise ValueError(f"{name} must be a writable contiguous {dt} array of at least {size} entries")
        return arr

    frame_accept = out("frame_accept", frame_accept, infos.size, np.dtype(np.uint8))
    groups = out("groups", groups, groups_cap, ITEM_DTYPE)
    group_first = out("group_first", group_first, n + 1, np.dtype(np.uint64))
    results = out("results", results, n, FRAME_WINDOW_RESULT_DTYPE)
    windows_out = out("windows_out", windows_out, n, FRAME_WINDOW_DTYPE)
    used = ctypes.c_uint64(0)
    one = np.zeros(1, dtype=np.uint8)  # (frame_accept is required even when there are no frames)
    check(lib().ufc_frame_window_host(infos.ctypes.data if infos.size else None, infos.size, frame_first.ctypes.data,
                                      windows.ctypes.data if n else None, n,
                                      frame_accept.ctypes.data if frame_accept.size else one.ctypes.data,
                                      groups.ctypes.data if groups_cap else None, groups_cap, group_first.ctypes.data,
                                      ctypes.addressof(used), results.ctypes.data if n else None,
                                      windows_out.ctypes.data if n else None, nthreads), "ufc_frame_window_host")
    return {"frame_accept": frame_accept, "groups": groups, "group_first": group_first, "groups_used": used.value,
            "results": results, "windows_out": windows_out}


def frame_queue_host(infos: np.ndarray, items: np.ndarray, frame_first: np.ndarray, sent: np.ndarray,
                     sent_first: np.ndarray, queues: np.ndarray, steps: np.ndarray, log: np.ndarray,
                     ref_acked: Optional[np.ndarray] = None, nthreads: int = 1, results: Optional[np.ndarray] = None,
                     queues_out: Optional[np.ndarray] = None):
    """One step of the sender's FrameQueue for many connections in host memory (ufc_frame_queue_host): connection c
    (FRAME_QUEUE_DTYPE; what to do in FRAME_QUEUE_STEP_DTYPE) pushes sent[sent_first[c] : sent_first[c + 1]]
    (SENT_FRAME_DTYPE), then handles the ack frames among infos[frame_first[c] : frame_first[c + 1]] (their groups
    in items, as the parse returns them), then forgets and produces feedback as its step asks.  log (SENT_FRAME_DTYPE,
    the arena new_frame_queues returns) and ref_acked (uint8, optional: set to 1 for every fragment of a newly
    acked frame) are updated in place.  Returns a dict: results (FRAME_QUEUE_RESULT_DTYPE), queues_out (may be
    given as `queues`), log, ref_acked."""
    infos = np.ascontiguousarray(infos, dtype=FRAME_INFO_DTYPE)
    items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
    sent = np.ascontiguousarray(sent, dtype=SENT_FRAME_DTYPE)
    frame_first = np.ascontiguousarray(frame_first, dtype=np.uint64)
    sent_first = np.ascontiguousarray(sent_first, dtype=np.uint64)
    steps = np.ascontiguousarray(steps, dtype=FRAME_QUEUE_STEP_DTYPE)
    if queues.dtype != FRAME_QUEUE_DTYPE or not queues.flags.c_contiguous:
        queues = np.ascontiguousarray(queues, dtype=FRAME_QUEUE_DTYPE)
    n = queues.size
    if frame_first.size < n + 1 or sent_first.size < n + 1 or steps.size < n:
        raise ValueError("frame_first and sent_first must hold one more entry than there are queues, steps one each")

    def inout(name, arr, size, dt):
        if arr is None:
            return np.zeros(size, dtype=dt)
        if arr.dtype != dt or not arr.flags.c_contiguous or not arr.flags.writeable or arr.size < size:
            raise ValueError(f"{name} must be a writable contiguous {dt} array of at least {size} entries")
        return arr

    log = inout("log", log, 0, SENT_FRAME_DTYPE)
    if ref_acked is not None:
        ref_acked = inout("ref_acked", ref_acked, 0, np.dtype(np.uint8))
    results = inout("results", results, n, FRAME_QUEUE_RESULT_DTYPE)
    queues_out = inout("queues_out", queues_out, n, FRAME_QUEUE_DTYPE)
    refs_cap = ref_acked.size if ref_acked is not None else 0
    check(lib().ufc_frame_queue_host(infos.ctypes.data if infos.size else None, infos.size,
                                     items.ctypes.data if items.size else None, items.size, frame_first.ctypes.data,
                                     sent.ctypes.data if sent.size else None, sent.size, sent_first.ctypes.data,
                                     queues.ctypes.data if n else None, steps.ctypes.data if n else None, n,
                                     log.ctypes.data if log.size else None, log.size,
                                     ref_acked.ctypes.data if refs_cap else None, refs_cap,
                                     results.ctypes.data if n else None, queues_out.ctypes.data if n else None, nthreads),
          "ufc_frame_queue_host")
    return {"results": results, "queues_out": queues_out, "log": log, "ref_acked": ref_acked}


def _rate_inout(name, arr, size, dt):
    if arr is None:
        return np.zeros(size, dtype=dt)
    if arr.dtype != dt or not arr.flags.c_contiguous or not arr.flags.writeable or arr.size < size:
        raise ValueError(f"{name} must be a writable contiguous {dt} array of at least {size} entries")
    return arr


def rate_begin_host(states: np.ndarray, now_ms: np.ndarray, extra_flags: Optional[np.ndarray] = None,
                    nthreads: int = 1, steps: Optional[np.ndarray] = None, states_out: Optional[np.ndarray] = None):
    """Opens a tick for many connections in host memory (ufc_rate_begin_host): from every RATE_STATE_DTYPE record and
    its now_ms, the FRAME_QUEUE_STEP_DTYPE record the frame queue call of this tick takes (forget, feedback, the rtt
    and a pending reset_loss_rate, OR-ed with extra_flags: the caller's FQ_MARK_RATE_LIMITED).  Returns a dict:
    steps, states_out (the pending reset taken; may be given as `states`)."""
    if states.dtype != RATE_STATE_DTYPE or not states.flags.c_contiguous:
        states = np.ascontiguousarray(states, dtype=RATE_STATE_DTYPE)
    n = states.size
    now_ms = np.ascontiguousarray(now_ms, dtype=np.uint64)
    if extra_flags is not None:
        extra_flags = np.ascontiguousarray(extra_flags, dtype=np.uint32)
    if now_ms.size < n or (extra_flags is not None and extra_flags.size < n):
        raise ValueError("now_ms and extra_flags must hold one entry per state")
    steps = _rate_inout("steps", steps, n, FRAME_QUEUE_STEP_DTYPE)
    states_out = _rate_inout("states_out", states_out, n, RATE_STATE_DTYPE)
    check(lib().ufc_rate_begin_host(states.ctypes.data if n else None, now_ms.ctypes.data if n else None,
                                    extra_flags.ctypes.data if extra_flags is not None and n else None, n,
                                    steps.ctypes.data if n else None, states_out.ctypes.data if n else None, nthreads),
          "ufc_rate_begin_host")
    return {"steps": steps, "states_out": states_out}


def rate_step_host(states: np.ndarray, ticks: np.ndarray, fq_results: np.ndarray, entries: np.ndarray,
                   flush_results: Optional[np.ndarray] = None, result_index: Optional[np.ndarray] = None,
                   flushes: Optional[np.ndarray] = None, flush_index: Optional[np.ndarray] = None, nthreads: int = 1,
                   results: Optional[np.ndarray] = None, states_out: Optional[np.ndarray] = None):
    """Closes a tick for many connections in host memory (ufc_rate_step_host): the last flush's accounting
    (notify_frame_sent), fill_flush_alloc and SendRateComp::step on the frame queue's results (fq_results,
    FRAME_QUEUE_RESULT_DTYPE) for every RATE_STATE_DTYPE record with its RATE_TICK_DTYPE input.  entries
    (RECV_RATE_ENTRY_DTYPE, the arena new_rate_states returns) is updated in place.  flush_results
    (FLUSH_RESULT_DTYPE) with result_index (uint32 per connection, NO_INDEX for none) gathers the last flush's
    alloc_left and frame_count; flushes (FLUSH_DTYPE, updated in place) with flush_index receives the new
    flush_alloc.  Returns a dict: results (RATE_RESULT_DTYPE), states_out (may be given as `states`), entries,
    flushes."""
    if states.dtype != RATE_STATE_DTYPE or not states.flags.c_contiguous:
        states = np.ascontiguousarray(states, dtype=RATE_STATE_DTYPE)
    n = states.size
    ticks = np.ascontiguousarray(ticks, dtype=RATE_TICK_DTYPE)
    fq_results = np.ascontiguousarray(fq_results, dtype=FRAME_QUEUE_RESULT_DTYPE)
    if ticks.size < n or fq_results.size < n:
        raise ValueError("ticks and fq_results must hold one record per state")
    entries = _rate_inout("entries", entries, 0, RECV_RATE_ENTRY_DTYPE)
    n_fr = n_fl = 0
    if (flush_results is not None and result_index is None) or (flushes is not None and flush_index is None):
        raise ValueError("flush_results needs result_index, flushes needs flush_index")
    if flush_results is not None:
        flush_results = np.ascontiguousarray(flush_results, dtype=FLUSH_RESULT_DTYPE)
        result_index = np.ascontiguousarray(result_index, dtype=np.uint32)
        n_fr = flush_results.size
        if result_index.size < n:
            raise ValueError("result_index must hold one entry per state")
    if flushes is not None:
        flushes = _rate_inout("flushes", flushes, 0, FLUSH_DTYPE)
        flush_index = np.ascontiguousarray(flush_index, dtype=np.uint32)
        n_fl = flushes.size
        if flush_index.size < n:
            raise ValueError("flush_index must hold one entry per state")
    results = _rate_inout("results", results, n, RATE_RESULT_DTYPE)
    states_out = _rate_inout("states_out", states_out, n, RATE_STATE_DTYPE)
    check(lib().ufc_rate_step_host(states.ctypes.data if n else None, ticks.ctypes.data if n else None,
                                   fq_results.ctypes.data if n else None, n,
                                   entries.ctypes.data if entries.size else None, entries.size,
                                   flush_results.ctypes.data if n_fr else None, n_fr,
                                   result_index.ctypes.data if n_fr else None,
                                   flushes.ctypes.data if n_fl else None, n_fl,
                                   flush_index.ctypes.data if n_fl else None,
                                   results.ctypes.data if n else None, states_out.ctypes.data if n else None, nthreads),
          "ufc_rate_step_host")
    return {"results": results, "states_out": states_out, "entries": entries, "flushes": flushes}


def _rs_arenas(arenas):
    out = {}
    for name, dt in RESEND_ARENAS:
        a = arenas.get(name)
        if a is None:
            a = np.zeros(0, dtype=dt)
        if a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError(f"arena {name} must be a writable contiguous {dt} array")
        out[name] = a
    return out


def _rs_ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _rs_in(arr, dt):
    if arr.dtype != dt or not arr.flags.c_contiguous:
        arr = np.ascontiguousarray(arr, dtype=dt)
    return arr


def resend_begin_host(infos: np.ndarray, frame_first: np.ndarray, queues: np.ndarray, log: np.ndarray,
                      rate: np.ndarray, flushes: np.ndarray, states: np.ndarray, senders: np.ndarray, arenas: dict,
                      flags: Optional[np.ndarray] = None, nthreads: int = 1, results: Optional[np.ndarray] = None,
                      states_out: Optional[np.ndarray] = None, senders_out: Optional[np.ndarray] = None):
    """ufc_resend_begin_host: ack propagation, PacketSender::acknowledge for the ack frames among
    infos[frame_first[c] : frame_first[c + 1]], the resend loop and the pending fragments' staging for every
    connection (RESEND_DTYPE states with SENDER_DTYPE senders; queues and log as frame_queue_host left them; rate
    the RATE_RESULT_DTYPE records of rate_step_host; flushes the data FLUSH_DTYPE records the pack will get).  The
    arenas (the dict new_resend_states returns) are updated in place.  Returns a dict: results (RESEND_RESULT_DTYPE),
    states_out and senders_out (may be given as `states` and `senders`)."""
    infos = _rs_in(infos, FRAME_INFO_DTYPE)
    frame_first = _rs_in(frame_first, np.dtype(np.uint64))
    queues = _rs_in(queues, FRAME_QUEUE_DTYPE)
    log = _rs_in(log, SENT_FRAME_DTYPE)
    rate = _rs_in(rate, RATE_RESULT_DTYPE)
    flushes = _rs_in(flushes, FLUSH_DTYPE)
    states = _rs_in(states, RESEND_DTYPE)
    senders = _rs_in(senders, SENDER_DTYPE)
    n = states.size
    if min(queues.size, rate.size, flushes.size, senders.size) < n or frame_first.size < n + 1:
        raise ValueError("queues, rate, flushes and senders must hold one record per state, frame_first one more")
    if flags is not None:
        flags = _rs_in(flags, np.dtype(np.uint32))
        if flags.size < n:
            raise ValueError("flags must hold one entry per state")
    A = _rs_arenas(arenas)
    results = _rate_inout("results", results, n, RESEND_RESULT_DTYPE)
    states_out = _rate_inout("states_out", states_out, n, RESEND_DTYPE)
    senders_out = _rate_inout("senders_out", senders_out, n, SENDER_DTYPE)
    check(lib().ufc_resend_begin_host(_rs_ptr(infos), infos.size, frame_first.ctypes.data, _rs_ptr(queues), _rs_ptr(log),
                                      log.size, _rs_ptr(rate), _rs_ptr(flags), _rs_ptr(flushes), _rs_ptr(states),
                                      _rs_ptr(senders), n, _rs_ptr(A["heap"]), A["heap"].size, _rs_ptr(A["pkts"]),
                                      A["pkts"].size, _rs_ptr(A["frag_acked"]), A["frag_acked"].size, _rs_ptr(A["tx"]),
                                      A["tx"].size, _rs_ptr(A["ref_acked"]), A["ref_acked"].size, _rs_ptr(A["stage"]),
                                      A["stage"].size, _rs_ptr(results), _rs_ptr(states_out), _rs_ptr(senders_out),
                                      nthreads), "ufc_resend_begin_host")
    return {"results": results, "states_out": states_out, "senders_out": senders_out}


def resend_place_host(states: np.ndarray, begin_results: np.ndarray, arenas: dict, flush_first: np.ndarray,
                      items: np.ndarray, nthreads: int = 1):
    """ufc_resend_place_host: every connection's staged items into items[flush_first[c] ..], the slots the emit
    reserved; items (ITEM_DTYPE) is written in place and returned."""
    states = _rs_in(states, RESEND_DTYPE)
    begin_results = _rs_in(begin_results, RESEND_RESULT_DTYPE)
    flush_first = _rs_in(flush_first, np.dtype(np.uint64))
    n = states.size
    if begin_results.size < n or flush_first.size < n + 1:
        raise ValueError("begin_results must hold one record per state, flush_first one more")
    if items.dtype != ITEM_DTYPE or not items.flags.c_contiguous or not items.flags.writeable:
        raise ValueError("items must be a writable contiguous ITEM_DTYPE array")
    stage = _rs_arenas(arenas)["stage"]
    check(lib().ufc_resend_place_host(_rs_ptr(states), _rs_ptr(begin_results), n, _rs_ptr(stage), stage.size,
                                      flush_first.ctypes.data, _rs_ptr(items), items.size, nthreads),
          "ufc_resend_place_host")
    return items


def resend_commit_host(flush_results: np.ndarray, infos: np.ndarray, out_offsets: np.ndarray, frames_used: int,
                       items: np.ndarray, flush_first: np.ndarray, packets: np.ndarray, packet_first: np.ndarray,
                       packet_results: np.ndarray, sender_results: np.ndarray, begin_results: np.ndarray,
                       rate: np.ndarray, states: np.ndarray, senders: np.ndarray, arenas: dict,
                       sent: Optional[np.ndarray] = None, next_extra_flags: Optional[np.ndarray] = None,
                       nthreads: int = 1, results: Optional[np.ndarray] = None, states_out: Optional[np.ndarray] = None,
                       retake: Optional[np.ndarray] = None):
    """ufc_resend_commit_host: behind pack_host over the data flushes (flush c = connection c) and build_sizes_host:
    what the reference's flush did to the pending queue, the packet table, the resend heap and the transmission ring,
    the frames' SENT_FRAME_DTYPE records for the next frame_queue_host call, and the second emit's senders.  Returns a
    dict: results (RESEND_COMMIT_RESULT_DTYPE), states_out (may be given as `states`), retake (SENDER_DTYPE, may be
    given as `senders`), sent (one record per frame of infos unless given), sent_first, next_extra_flags."""
    flush_results = _rs_in(flush_results, FLUSH_RESULT_DTYPE)
    infos = _rs_in(infos, FRAME_INFO_DTYPE)
    out_offsets = _rs_in(out_offsets, np.dtype(np.uint64))
    items = _rs_in(items, ITEM_DTYPE)
    flush_first = _rs_in(flush_first, np.dtype(np.uint64))
    packets = _rs_in(packets, PACKET_DTYPE)
    packet_first = _rs_in(packet_first, np.dtype(np.uint64))
    packet_results = _rs_in(packet_results, PACKET_RESULT_DTYPE)
    sender_results = _rs_in(sender_results, SENDER_RESULT_DTYPE)
    begin_results = _rs_in(begin_results, RESEND_RESULT_DTYPE)
    rate = _rs_in(rate, RATE_RESULT_DTYPE)
    states = _rs_in(states, RESEND_DTYPE)
    senders = _rs_in(senders, SENDER_DTYPE)
    n = states.size
    if min(flush_results.size, sender_results.size, begin_results.size, rate.size, senders.size) < n or \
            min(flush_first.size, packet_first.size) < n + 1 or out_offsets.size < infos.size + 1 or \
            packet_results.size < packets.size:
        raise ValueError("one record per state (one more in the CSRs), out_offsets one more than infos")
    A = _rs_arenas(arenas)
    used = np.array([frames_used], dtype=np.uint64)
    sent = _rate_inout("sent", sent, infos.size, SENT_FRAME_DTYPE)
    sent_first = np.zeros(n + 1, dtype=np.uint64)
    if next_extra_flags is not None:
        next_extra_flags = _rate_inout("next_extra_flags", next_extra_flags, n, np.dtype(np.uint32))
    results = _rate_inout("results", results, n, RESEND_COMMIT_RESULT_DTYPE)
    states_out = _rate_inout("states_out", states_out, n, RESEND_DTYPE)
    retake = _rate_inout("retake", retake, n, SENDER_DTYPE)
    check(lib().ufc_resend_commit_host(_rs_ptr(flush_results), _rs_ptr(infos), infos.size, out_offsets.ctypes.data,
                                       used.ctypes.data, _rs_ptr(items), items.size, flush_first.ctypes.data,
                                       _rs_ptr(packets), packets.size, packet_first.ctypes.data, _rs_ptr(packet_results),
                                       _rs_ptr(sender_results), _rs_ptr(begin_results), _rs_ptr(rate), _rs_ptr(states),
                                       _rs_ptr(senders), n, _rs_ptr(A["heap"]), A["heap"].size, _rs_ptr(A["pkts"]),
                                       A["pkts"].size, _rs_ptr(A["frag_acked"]), A["frag_acked"].size, _rs_ptr(A["tx"]),
                                       A["tx"].size, _rs_ptr(sent), sent.size, sent_first.ctypes.data,
                                       _rs_ptr(next_extra_flags), _rs_ptr(results), _rs_ptr(states_out), _rs_ptr(retake),
                                       nthreads), "ufc_resend_commit_host")
    return {"results": results, "states_out": states_out, "retake": retake, "sent": sent, "sent_first": sent_first,
            "next_extra_flags": next_extra_flags}
