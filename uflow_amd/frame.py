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

from ._native import Builder, DatagramRef, FrameInfo, Item, check, lib, UFC_ERR_NOMEM
# The stages' constants without their prefix: each value is written once, in _native.
from ._native import (  # noqa: F401
    UFC_PACK_DONE as PACK_DONE, UFC_PACK_SIZE_LIMITED as PACK_SIZE_LIMITED, UFC_PACK_WINDOW_LIMITED as PACK_WINDOW_LIMITED,
    UFC_PACK_BAD_RANGE as PACK_BAD_RANGE,
    UFC_SEND_TIME_SENSITIVE as SEND_TIME_SENSITIVE, UFC_SEND_UNRELIABLE as SEND_UNRELIABLE,
    UFC_SEND_PERSISTENT as SEND_PERSISTENT, UFC_SEND_RELIABLE as SEND_RELIABLE, UFC_NO_PARENT as NO_PARENT,
    UFC_EMIT_DONE as EMIT_DONE, UFC_EMIT_WINDOW_LIMITED as EMIT_WINDOW_LIMITED, UFC_EMIT_ALLOC_LIMITED as EMIT_ALLOC_LIMITED,
    UFC_EMIT_BAD_PACKET as EMIT_BAD_PACKET, UFC_EMIT_BAD_RANGE as EMIT_BAD_RANGE,
    UFC_PACKET_NOT_REACHED as PACKET_NOT_REACHED, UFC_PACKET_EMITTED as PACKET_EMITTED, UFC_PACKET_DROPPED as PACKET_DROPPED,
    UFC_RX_ASM_OPEN as RX_ASM_OPEN, UFC_RX_ASM_CLOSED as RX_ASM_CLOSED, UFC_RX_ASM_ACTIVE as RX_ASM_ACTIVE,
    UFC_RX_SLOT_ENTRY as RX_SLOT_ENTRY, UFC_RX_SLOT_DATA as RX_SLOT_DATA, UFC_RX_SLOT_DUD as RX_SLOT_DUD,
    UFC_RX_PACKET_DUD as RX_PACKET_DUD,
    UFC_RX_NOT_HANDLED as RX_NOT_HANDLED, UFC_RX_STORED as RX_STORED, UFC_RX_COMPLETED as RX_COMPLETED, UFC_RX_DUD as RX_DUD,
    UFC_RX_DROPPED_INVALID as RX_DROPPED_INVALID, UFC_RX_DROPPED_WINDOW as RX_DROPPED_WINDOW,
    UFC_RX_DROPPED_CHANNEL as RX_DROPPED_CHANNEL, UFC_RX_DROPPED_CLOSED as RX_DROPPED_CLOSED,
    UFC_RX_DROPPED_MISMATCH as RX_DROPPED_MISMATCH, UFC_RX_DROPPED_DUPLICATE as RX_DROPPED_DUPLICATE,
    UFC_RX_DROPPED_BAD_SRC as RX_DROPPED_BAD_SRC, UFC_RX_DONE as RX_DONE, UFC_RX_BAD_STATE as RX_BAD_STATE,
    UFC_FW_DONE as FW_DONE, UFC_FW_BAD_STATE as FW_BAD_STATE,
    UFC_SENT_NONCE as SENT_NONCE, UFC_SENT_RATE_LIMITED as SENT_RATE_LIMITED, UFC_SENT_ACKED as SENT_ACKED,
    UFC_SENT_MARK as SENT_MARK,
    UFC_FQ_HAS_RTT as FQ_HAS_RTT, UFC_FQ_RESET_LOSS as FQ_RESET_LOSS, UFC_FQ_MARK_RATE_LIMITED as FQ_MARK_RATE_LIMITED,
    UFC_FQ_FORGET as FQ_FORGET, UFC_FQ_FEEDBACK as FQ_FEEDBACK, UFC_FQ_DONE as FQ_DONE, UFC_FQ_BAD_STATE as FQ_BAD_STATE,
    UFC_RATE_AWAIT_SEND as RATE_AWAIT_SEND, UFC_RATE_SLOW_START as RATE_SLOW_START,
    UFC_RATE_THROUGHPUT_EQN as RATE_THROUGHPUT_EQN, UFC_RATE_FRAME_SENT as RATE_FRAME_SENT,
    UFC_RATE_DONE as RATE_DONE, UFC_RATE_BAD_STATE as RATE_BAD_STATE, UFC_RATE_REF_PANIC as RATE_REF_PANIC,
    UFC_RATE_RECV_FULL as RATE_RECV_FULL,
    UFC_RATE_FEEDBACK as RATE_FEEDBACK, UFC_RATE_NOFEEDBACK as RATE_NOFEEDBACK, UFC_RATE_RESET_ISSUED as RATE_RESET_ISSUED,
    UFC_RATE_ENTERED_EQN as RATE_ENTERED_EQN, UFC_RATE_INV_STALLED as RATE_INV_STALLED,
    UFC_NO_PARENT as NO_INDEX,  # in result_index / flush_index: no gather for this connection
    UFC_TX_RESEND as TX_RESEND, UFC_RS_NO_DATA_FLUSH as RS_NO_DATA_FLUSH,
    UFC_RS_DONE as RS_DONE, UFC_RS_SIZE_LIMITED as RS_SIZE_LIMITED, UFC_RS_WINDOW_LIMITED as RS_WINDOW_LIMITED,
    UFC_RS_REF_HANG as RS_REF_HANG, UFC_RS_BAD_STATE as RS_BAD_STATE, UFC_RS_STAGE_FULL as RS_STAGE_FULL,
    UFC_RS_HEAP_FULL as RS_HEAP_FULL)
# The record layouts (numpy views of the header's structs) are declared in records.py.
from .records import (  # noqa: F401
    FRAME_INFO_DTYPE, ITEM_DTYPE, FLUSH_DTYPE, FLUSH_RESULT_DTYPE, PACKET_DTYPE, SENDER_DTYPE, PACKET_RESULT_DTYPE,
    SENDER_RESULT_DTYPE, RECEIVER_DTYPE, RX_SLOT_DTYPE, RX_PACKET_DTYPE, RECEIVER_RESULT_DTYPE, FRAME_WINDOW_DTYPE,
    FRAME_WINDOW_RESULT_DTYPE, SENT_FRAME_DTYPE, FRAME_QUEUE_DTYPE, FRAME_QUEUE_STEP_DTYPE, FRAME_QUEUE_RESULT_DTYPE,
    RECV_RATE_ENTRY_DTYPE, RATE_STATE_DTYPE, RATE_TICK_DTYPE, RATE_RESULT_DTYPE, RESEND_ENTRY_DTYPE, SENT_PACKET_DTYPE,
    TX_REF_DTYPE, RESEND_DTYPE, RESEND_RESULT_DTYPE, RESEND_COMMIT_RESULT_DTYPE)

MAX_FRAME_SIZE = 1472  # src/lib.rs:286-294
DATA_FRAME_MAX_DATAGRAM_COUNT = 127  # serial/mod.rs:42
HANDSHAKE_SYN, HANDSHAKE_SYN_ACK, HANDSHAKE_ACK, HANDSHAKE_ERROR = 0, 1, 2, 3
DISCONNECT, DISCONNECT_ACK, DATA, SYNC, ACK = 4, 5, 10, 11, 12
HANDSHAKE_ERRORS = ("Version", "Config", "ServerFull")  # HandshakeErrorType, src/frame/mod.rs:30-35

# The arenas of the resend state, in the order the C calls take them: name, record dtype.
RESEND_ARENAS = (("heap", RESEND_ENTRY_DTYPE), ("pkts", SENT_PACKET_DTYPE), ("frag_acked", np.dtype(np.uint8)),
                 ("tx", TX_REF_DTYPE), ("ref_acked", np.dtype(np.uint8)), ("stage", ITEM_DTYPE))
_RS_ARENA_DTYPE = dict(RESEND_ARENAS)


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


_U8, _U32, _U64 = np.dtype(np.uint8), np.dtype(np.uint32), np.dtype(np.uint64)


def _in(name, arr, dt, count=0):
    """An input argument: a C-contiguous array of dt (the array itself when it is one, else a coerced copy) holding
    at least count entries."""
    arr = np.ascontiguousarray(arr, dtype=dt)
    if arr.size < count:
        raise ValueError(f"{name} must hold at least {count} entries, holds {arr.size}")
    return arr


def _inout(name, arr, dt, size=0):
    """An argument the C call writes: allocated (zeroed, size entries) when None, else it must be exactly dt,
    C-contiguous, writable and hold at least size entries (nothing is coerced: a copy would take the writes)."""
    if arr is None:
        return np.zeros(size, dtype=dt)
    if arr.dtype != dt or not arr.flags.c_contiguous or not arr.flags.writeable or arr.size < size:
        raise ValueError(f"{name} must be a writable contiguous {dt} array of at least {size} entries")
    return arr


def _p(a):
    """The array's address for the C ABI; None (NULL) for no array and for an empty one."""
    return a.ctypes.data if a is not None and a.size else None


def parse_batch_host(data: np.ndarray, offsets: np.ndarray, valid: Optional[np.ndarray] = None, nthreads: int = 1):
    """Frame::read of every frame of a CSR batch in host memory, after the batched CRC gate
    (`valid`, from the GPU; None = gate on the host).  Returns (infos[n], items) as numpy
    structured arrays (FRAME_INFO_DTYPE, ITEM_DTYPE); infos['item_first'] indexes items."""
    data = _in("data", data, _U8)
    offsets = _in("offsets", offsets, _U64)
    n = offsets.size - 1
    infos = np.zeros(max(n, 0), dtype=FRAME_INFO_DTYPE)
    used = ctypes.c_size_t(0)
    vp = _in("valid", valid, _U8).ctypes.data if valid is not None else None
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
    infos = _in("infos", infos, FRAME_INFO_DTYPE)
    items = _in("items", items, ITEM_DTYPE)
    payload = _in("payload", payload, _U8)
    n = infos.size
    sb = _in("src_base", src_base, _U64, n).ctypes.data if src_base is not None else None
    offsets = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    crc = np.zeros(n, dtype=np.uint32)
    ip = _p(items)
    check(lib().ufc_build_sizes_host(infos.ctypes.data, ip, items.size, sb, payload.size, n, offsets.ctypes.data,
                                     status.ctypes.data, nthreads), "ufc_build_sizes_host")
    out = np.zeros(int(offsets[n]), dtype=np.uint8)
    check(lib().ufc_build_batch_host(infos.ctypes.data, ip, items.size, sb, _p(payload), payload.size, n,
                                     offsets.ctypes.data, _p(out), out.size,
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
    items = _in("items", items, ITEM_DTYPE)
    flushes = _in("flushes", flushes, FLUSH_DTYPE)
    n = flushes.size
    flush_first = _in("flush_first", flush_first, _U64, n + 1)
    if frames_cap is None:
        frames_cap = items.size if infos is None else infos.size
    infos = _inout("infos", infos, FRAME_INFO_DTYPE, frames_cap)
    nb = None
    if nonce_bits is not None:  # one bit per frame below frames_cap
        nb = _in("nonce_bits", nonce_bits, _U32, (frames_cap + 31) // 32).ctypes.data
    results = np.zeros(n, dtype=FLUSH_RESULT_DTYPE)
    used = ctypes.c_uint64(0)
    check(lib().ufc_pack_host(_p(items), items.size, flush_first.ctypes.data, _p(flushes), n, nb,
                              infos.ctypes.data if frames_cap else None, frames_cap, _p(results), ctypes.byref(used),
                              nthreads), "ufc_pack_host")
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
    packets = _in("packets", packets, PACKET_DTYPE)
    senders = _in("senders", senders, SENDER_DTYPE)
    n = senders.size
    packet_first = _in("packet_first", packet_first, _U64, n + 1)
    senders_out = _inout("senders_out", senders_out, SENDER_DTYPE, n)
    flush_first = np.zeros(n + 1, dtype=np.uint64)
    packet_results = np.zeros(packets.size, dtype=PACKET_RESULT_DTYPE) if want_packet_results else None
    sender_results = np.zeros(n, dtype=SENDER_RESULT_DTYPE)
    used = ctypes.c_uint64(0)

    def call(items_p, cap):
        check(lib().ufc_emit_packets_host(_p(packets), packets.size, packet_first.ctypes.data, _p(senders), n, items_p, cap,
                                          flush_first.ctypes.data, _p(packet_results), _p(sender_results),
                                          _p(senders_out) if n else None, ctypes.byref(used), nthreads),
              "ufc_emit_packets_host")

    if items_cap is None:
        if items is not None:
            items_cap = items.size
        elif senders_out is senders or np.shares_memory(senders_out, senders):
            raise ValueError("give items_cap (or items) when the state is updated in place")
        else:
            call(None, 0)
            items_cap = used.value
    items = _inout("items", items, ITEM_DTYPE, items_cap)
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
    infos = _in("infos", infos, FRAME_INFO_DTYPE)
    items = _in("items", items, ITEM_DTYPE)
    payload = _in("payload", payload, _U8)
    carry_in = _in("carry_in", carry_in, _U8)
    receivers = _in("receivers", receivers, RECEIVER_DTYPE)
    n = receivers.size
    frame_first = _in("frame_first", frame_first, _U64, n + 1)
    slot_first = _in("slot_first", slot_first, _U64, n + 1)
    slots = _inout("slots", slots, RX_SLOT_DTYPE)
    if src_base is not None:
        src_base = _in("src_base", src_base, _U64, infos.size)
    if frame_accept is not None:
        frame_accept = _in("frame_accept", frame_accept, _U8, infos.size)
    receivers_out = _inout("receivers_out", receivers_out, RECEIVER_DTYPE, n)
    carry_first = np.zeros(n + 1, dtype=np.uint64)
    packet_first = np.zeros(n + 1, dtype=np.uint64)
    results = np.zeros(n, dtype=RECEIVER_RESULT_DTYPE)
    carry_used, packets_used, out_used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    p = _p

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
    # (arrays that are given set the caps by their sizes)
    carry_out = _inout("carry_out", carry_out, _U8, 0 if carry_out is not None else int(carry_cap))
    out_bytes = _inout("out_bytes", out_bytes, _U8, 0 if out_bytes is not None else int(out_cap))
    packets = _inout("packets", packets, RX_PACKET_DTYPE, 0 if packets is not None else int(packets_cap))
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
    infos = _in("infos", infos, FRAME_INFO_DTYPE)
    windows = _in("windows", windows, FRAME_WINDOW_DTYPE)
    n = windows.size
    frame_first = _in("frame_first", frame_first, _U64, n + 1)
    if groups_cap is None:
        groups_cap = groups.size if groups is not None else n + infos.size
    groups_cap = int(groups_cap)
    frame_accept = _inout("frame_accept", frame_accept, _U8, infos.size)
    groups = _inout("groups", groups, ITEM_DTYPE, groups_cap)
    group_first = _inout("group_first", group_first, _U64, n + 1)
    results = _inout("results", results, FRAME_WINDOW_RESULT_DTYPE, n)
    windows_out = _inout("windows_out", windows_out, FRAME_WINDOW_DTYPE, n)
    used = ctypes.c_uint64(0)
    one = np.zeros(1, dtype=np.uint8)  # (frame_accept is required even when there are no frames)
    check(lib().ufc_frame_window_host(_p(infos), infos.size, frame_first.ctypes.data, _p(windows), n,
                                      _p(frame_accept) or one.ctypes.data, groups.ctypes.data if groups_cap else None,
                                      groups_cap, group_first.ctypes.data, ctypes.addressof(used),
                                      results.ctypes.data if n else None, windows_out.ctypes.data if n else None,
                                      nthreads), "ufc_frame_window_host")
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
    infos = _in("infos", infos, FRAME_INFO_DTYPE)
    items = _in("items", items, ITEM_DTYPE)
    sent = _in("sent", sent, SENT_FRAME_DTYPE)
    queues = _in("queues", queues, FRAME_QUEUE_DTYPE)
    n = queues.size
    frame_first = _in("frame_first", frame_first, _U64, n + 1)
    sent_first = _in("sent_first", sent_first, _U64, n + 1)
    steps = _in("steps", steps, FRAME_QUEUE_STEP_DTYPE, n)
    log = _inout("log", log, SENT_FRAME_DTYPE)
    if ref_acked is not None:
        ref_acked = _inout("ref_acked", ref_acked, _U8)
    results = _inout("results", results, FRAME_QUEUE_RESULT_DTYPE, n)
    queues_out = _inout("queues_out", queues_out, FRAME_QUEUE_DTYPE, n)
    refs_cap = ref_acked.size if ref_acked is not None else 0
    check(lib().ufc_frame_queue_host(_p(infos), infos.size, _p(items), items.size, frame_first.ctypes.data, _p(sent),
                                     sent.size, sent_first.ctypes.data, _p(queues), _p(steps) if n else None, n, _p(log),
                                     log.size, _p(ref_acked), refs_cap, results.ctypes.data if n else None,
                                     queues_out.ctypes.data if n else None, nthreads), "ufc_frame_queue_host")
    return {"results": results, "queues_out": queues_out, "log": log, "ref_acked": ref_acked}


def rate_begin_host(states: np.ndarray, now_ms: np.ndarray, extra_flags: Optional[np.ndarray] = None,
                    nthreads: int = 1, steps: Optional[np.ndarray] = None, states_out: Optional[np.ndarray] = None):
    """Opens a tick for many connections in host memory (ufc_rate_begin_host): from every RATE_STATE_DTYPE record and
    its now_ms, the FRAME_QUEUE_STEP_DTYPE record the frame queue call of this tick takes (forget, feedback, the rtt
    and a pending reset_loss_rate, OR-ed with extra_flags: the caller's FQ_MARK_RATE_LIMITED).  Returns a dict:
    steps, states_out (the pending reset taken; may be given as `states`)."""
    states = _in("states", states, RATE_STATE_DTYPE)
    n = states.size
    now_ms = _in("now_ms", now_ms, _U64, n)
    if extra_flags is not None:
        extra_flags = _in("extra_flags", extra_flags, _U32, n)
    steps = _inout("steps", steps, FRAME_QUEUE_STEP_DTYPE, n)
    states_out = _inout("states_out", states_out, RATE_STATE_DTYPE, n)
    check(lib().ufc_rate_begin_host(_p(states), _p(now_ms) if n else None, _p(extra_flags) if n else None, n,
                                    _p(steps) if n else None, _p(states_out) if n else None, nthreads),
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
    states = _in("states", states, RATE_STATE_DTYPE)
    n = states.size
    ticks = _in("ticks", ticks, RATE_TICK_DTYPE, n)
    fq_results = _in("fq_results", fq_results, FRAME_QUEUE_RESULT_DTYPE, n)
    entries = _inout("entries", entries, RECV_RATE_ENTRY_DTYPE)
    n_fr = n_fl = 0
    if (flush_results is not None and result_index is None) or (flushes is not None and flush_index is None):
        raise ValueError("flush_results needs result_index, flushes needs flush_index")
    if flush_results is not None:
        flush_results = _in("flush_results", flush_results, FLUSH_RESULT_DTYPE)
        result_index = _in("result_index", result_index, _U32, n)
        n_fr = flush_results.size
    if flushes is not None:
        flushes = _inout("flushes", flushes, FLUSH_DTYPE)
        flush_index = _in("flush_index", flush_index, _U32, n)
        n_fl = flushes.size
    results = _inout("results", results, RATE_RESULT_DTYPE, n)
    states_out = _inout("states_out", states_out, RATE_STATE_DTYPE, n)
    check(lib().ufc_rate_step_host(_p(states), _p(ticks) if n else None, _p(fq_results) if n else None, n, _p(entries),
                                   entries.size, _p(flush_results), n_fr, _p(result_index) if n_fr else None,
                                   _p(flushes), n_fl, _p(flush_index) if n_fl else None,
                                   _p(results) if n else None, _p(states_out) if n else None, nthreads),
          "ufc_rate_step_host")
    return {"results": results, "states_out": states_out, "entries": entries, "flushes": flushes}


def _rs_arenas(arenas, *names):
    """(pointer, count) of the named resend arenas, flat, as the C calls take them: each a writable array of its
    RESEND_ARENAS dtype (none: empty)."""
    out = []
    for name in names:
        a = _inout(f"arena {name}", arenas.get(name), _RS_ARENA_DTYPE[name])
        out += [_p(a), a.size]
    return out


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
    states = _in("states", states, RESEND_DTYPE)
    n = states.size
    infos = _in("infos", infos, FRAME_INFO_DTYPE)
    frame_first = _in("frame_first", frame_first, _U64, n + 1)
    queues = _in("queues", queues, FRAME_QUEUE_DTYPE, n)
    log = _in("log", log, SENT_FRAME_DTYPE)
    rate = _in("rate", rate, RATE_RESULT_DTYPE, n)
    flushes = _in("flushes", flushes, FLUSH_DTYPE, n)
    senders = _in("senders", senders, SENDER_DTYPE, n)
    if flags is not None:
        flags = _in("flags", flags, _U32, n)
    A = _rs_arenas(arenas, "heap", "pkts", "frag_acked", "tx", "ref_acked", "stage")
    results = _inout("results", results, RESEND_RESULT_DTYPE, n)
    states_out = _inout("states_out", states_out, RESEND_DTYPE, n)
    senders_out = _inout("senders_out", senders_out, SENDER_DTYPE, n)
    check(lib().ufc_resend_begin_host(_p(infos), infos.size, frame_first.ctypes.data, _p(queues), _p(log), log.size,
                                      _p(rate), _p(flags), _p(flushes), _p(states), _p(senders), n,
                                      *A, _p(results), _p(states_out), _p(senders_out), nthreads),
          "ufc_resend_begin_host")
    return {"results": results, "states_out": states_out, "senders_out": senders_out}


def resend_place_host(states: np.ndarray, begin_results: np.ndarray, arenas: dict, flush_first: np.ndarray,
                      items: np.ndarray, nthreads: int = 1):
    """ufc_resend_place_host: every connection's staged items into items[flush_first[c] ..], the slots the emit
    reserved; items (ITEM_DTYPE) is written in place and returned."""
    states = _in("states", states, RESEND_DTYPE)
    n = states.size
    begin_results = _in("begin_results", begin_results, RESEND_RESULT_DTYPE, n)
    flush_first = _in("flush_first", flush_first, _U64, n + 1)
    items = _inout("items", items, ITEM_DTYPE)
    check(lib().ufc_resend_place_host(_p(states), _p(begin_results), n, *_rs_arenas(arenas, "stage"),
                                      flush_first.ctypes.data, _p(items), items.size, nthreads), "ufc_resend_place_host")
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
    states = _in("states", states, RESEND_DTYPE)
    n = states.size
    flush_results = _in("flush_results", flush_results, FLUSH_RESULT_DTYPE, n)
    infos = _in("infos", infos, FRAME_INFO_DTYPE)
    out_offsets = _in("out_offsets", out_offsets, _U64, infos.size + 1)
    items = _in("items", items, ITEM_DTYPE)
    flush_first = _in("flush_first", flush_first, _U64, n + 1)
    packets = _in("packets", packets, PACKET_DTYPE)
    packet_first = _in("packet_first", packet_first, _U64, n + 1)
    packet_results = _in("packet_results", packet_results, PACKET_RESULT_DTYPE, packets.size)
    sender_results = _in("sender_results", sender_results, SENDER_RESULT_DTYPE, n)
    begin_results = _in("begin_results", begin_results, RESEND_RESULT_DTYPE, n)
    rate = _in("rate", rate, RATE_RESULT_DTYPE, n)
    senders = _in("senders", senders, SENDER_DTYPE, n)
    A = _rs_arenas(arenas, "heap", "pkts", "frag_acked", "tx")
    used = np.array([frames_used], dtype=np.uint64)
    sent = _inout("sent", sent, SENT_FRAME_DTYPE, infos.size)
    sent_first = np.zeros(n + 1, dtype=np.uint64)
    if next_extra_flags is not None:
        next_extra_flags = _inout("next_extra_flags", next_extra_flags, _U32, n)
    results = _inout("results", results, RESEND_COMMIT_RESULT_DTYPE, n)
    states_out = _inout("states_out", states_out, RESEND_DTYPE, n)
    retake = _inout("retake", retake, SENDER_DTYPE, n)
    check(lib().ufc_resend_commit_host(_p(flush_results), _p(infos), infos.size, out_offsets.ctypes.data, used.ctypes.data,
                                       _p(items), items.size, flush_first.ctypes.data, _p(packets), packets.size,
                                       packet_first.ctypes.data, _p(packet_results), _p(sender_results), _p(begin_results),
                                       _p(rate), _p(states), _p(senders), n, *A,
                                       _p(sent), sent.size, sent_first.ctypes.data, _p(next_extra_flags), _p(results),
                                       _p(states_out), _p(retake), nthreads), "ufc_resend_commit_host")
    return {"results": results, "states_out": states_out, "retake": retake, "sent": sent, "sent_first": sent_first,
            "next_extra_flags": next_extra_flags}
