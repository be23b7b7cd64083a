"""Batched, device-resident frame CRC on MI355X (the hot path).

`FrameCrcEngine` owns one libuflowcrc context per device and wraps the batched C-ABI entry
points on torch tensors (torch provides device memory and the current HIP stream only).
Per frame i:  crc[i] = compute(frame_i[:-4]),  valid[i] = len_i >= 5 and crc[i] == BE32(frame_i[-4:])
-- the CRC gate of Frame::read (src/frame/serial/mod.rs:675-690) -- and seal writes the trailer
(src/frame/serial/mod.rs:463-470, build.rs:151-159).

CRC words are returned as int32 tensors holding the uint32 bit patterns
(`crc.cpu().numpy().view(numpy.uint32)`).
"""
import contextlib
import ctypes

import numpy as np
import torch

from ._native import lib, check
from .frame import _RS_ARENA_DTYPE
from .records import (ADDR_DTYPE, FLUSH_ACKS_RESULT_DTYPE, FLUSH_CTL_DTYPE, FLUSH_DTYPE, FLUSH_RESULT_DTYPE,
                      FLUSH_SYNC_RESULT_DTYPE, FRAME_INFO_DTYPE, FRAME_QUEUE_DTYPE, FRAME_QUEUE_RESULT_DTYPE,
                      FRAME_QUEUE_STEP_DTYPE, FRAME_WINDOW_DTYPE, FRAME_WINDOW_RESULT_DTYPE, ITEM_DTYPE, PACKET_DTYPE,
                      PACKET_RESULT_DTYPE, RATE_RESULT_DTYPE, RATE_STATE_DTYPE, RATE_TICK_DTYPE, RECEIVER_DTYPE,
                      RECEIVER_RESULT_DTYPE, RECV_RATE_ENTRY_DTYPE, RESEND_COMMIT_RESULT_DTYPE, RESEND_DTYPE,
                      RESEND_RESULT_DTYPE, ROUTE_RESULT_DTYPE, ROUTE_SLOT_DTYPE, RX_PACKET_DTYPE, RX_SLOT_DTYPE,
                      SENDER_DTYPE, SENDER_RESULT_DTYPE, SENT_FRAME_DTYPE)


# Items of a flush whose frame chain one wave of the pack resolves in LDS at a time (kPackTile, csrc/frame_pack.hpp).
PACK_TILE = 256
# Packets of a sender that one wave of the packet emit resolves at a time (kEmitTile, csrc/packet_emit.hpp).
EMIT_TILE = 64


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _pn(t, count):
    """The stage calls' pointer rule: NULL for no tensor and when the count that goes with it is 0."""
    return _ptr(t) if count else None


def rows(a, device):
    """A numpy array as the device calls take it, on `device`: a structured (record) array becomes uint8[n, itemsize]
    rows, uint64 goes up as int64 and uint32 as int32 (the same bits), any other plain array as it is.  Always a
    fresh copy, never an alias of a's buffer (also on the CPU)."""
    a = np.ascontiguousarray(a)
    if a.dtype.names is not None:
        a = a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    device = torch.device(device)
    if device.type == "cpu" or not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a).to(device)


def records(t, dtype):
    """The tensor's bytes as a fresh, flat host array of `dtype` (a record dtype for rows, or a plain one: an int64
    CSR reads back as numpy.uint64)."""
    b = t.detach().contiguous().cpu().numpy().reshape(-1)
    return b.view(np.uint8).view(dtype).copy()


class FrameCrcEngine:
    def __init__(self, device=None):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._ctx = ctypes.c_void_p()
        check(lib().ufc_ctx_create(ctypes.byref(self._ctx), self.device.index or 0), "ufc_ctx_create")

    def _bytes_ptr(self, t):
        """The frame bytes' pointer for the C ABI, which wants a readable device buffer even when a
        batch holds only empty frames (torch gives an empty tensor a NULL data_ptr): a zeroed 256-B
        buffer of the engine's stands in then."""
        if t.numel():
            return _ptr(t)
        if getattr(self, "_no_bytes", None) is None:
            self._no_bytes = torch.zeros(256, dtype=torch.uint8, device=self.device)
        return _ptr(self._no_bytes)

    def close(self):
        if self._ctx:
            lib().ufc_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_stream(self, stream):
        """ufc_ctx_release_stream: free this context's scratch kept for `stream` (a torch.cuda.Stream)
        after the work queued on it; call before the stream goes away."""
        check(lib().ufc_ctx_release_stream(self._ctx, ctypes.c_void_p(stream.cuda_stream)), "ufc_ctx_release_stream")

    def set_option(self, option, value):
        """ufc_ctx_set_option (A/B kernel selection; results never depend on it)."""
        check(lib().ufc_ctx_set_option(self._ctx, int(option), int(value)), "ufc_ctx_set_option")

    def get_option(self, option):
        return lib().ufc_ctx_get_option(self._ctx, int(option))

    def _stream(self, stream):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def _check_dev(self, *ts):
        for t in ts:
            if t is not None and (t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"tensor must be contiguous on {self.device}")

    def _check(self, name, t, dtypes, min_numel):
        """Device, contiguity, dtype and size of an argument, checked before the C ABI sees its
        pointer (the kernels trust the sizes they are given)."""
        if t is None:
            return
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if t.dtype not in dtypes:
            raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        self._check_dev(t)
        if t.numel() < min_numel:
            raise ValueError(f"{name} holds {t.numel()} elements, needs at least {min_numel}")

    def _check_outputs(self, n, crc_out=None, valid_out=None):
        self._check("crc_out", crc_out, (torch.int32, torch.uint32), n)
        self._check("valid_out", valid_out, (torch.uint8,), n)

    # ---- fixed-stride batches ----
    def crc_fixed(self, frames, frame_len, stride=None, n=None, crc_out=None, valid_out=None,
                  want_crc=True, want_valid=True, stream=None):
        """frames: uint8 tensor; frame i at byte i*stride (stride defaults to frame_len)."""
        stride = frame_len if stride is None else stride
        if n is None:
            n = (frames.numel() - frame_len) // stride + 1 if frames.numel() >= frame_len else 0
        if crc_out is None and want_crc:
            crc_out = torch.empty(n, dtype=torch.int32, device=self.device)
        if valid_out is None and want_valid:
            valid_out = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._check("frames", frames, (torch.uint8,), (n - 1) * stride + frame_len if n else 0)
        self._check_outputs(n, crc_out, valid_out)
        check(lib().ufc_crc_batch_fixed(self._ctx, self._bytes_ptr(frames), stride, frame_len, n, _ptr(crc_out),
                                        _ptr(valid_out), self._stream(stream)), "ufc_crc_batch_fixed")
        return crc_out, valid_out

    def seal_fixed(self, frames, frame_len, stride=None, n=None, crc_out=None, stream=None):
        stride = frame_len if stride is None else stride
        if n is None:
            n = (frames.numel() - frame_len) // stride + 1 if frames.numel() >= frame_len else 0
        self._check("frames", frames, (torch.uint8,), (n - 1) * stride + frame_len if n else 0)
        self._check_outputs(n, crc_out)
        check(lib().ufc_seal_batch_fixed(self._ctx, self._bytes_ptr(frames), stride, frame_len, n, _ptr(crc_out),
                                         self._stream(stream)), "ufc_seal_batch_fixed")
        return crc_out

    # ---- variable-length (CSR) batches ----
    def crc_varlen(self, data, offsets, crc_out=None, valid_out=None, want_crc=True, want_valid=True,
                   stream=None):
        """data: uint8 tensor; offsets: int64 tensor of n+1 nondecreasing byte offsets."""
        n = offsets.numel() - 1
        if crc_out is None and want_crc:
            crc_out = torch.empty(max(n, 0), dtype=torch.int32, device=self.device)
        if valid_out is None and want_valid:
            valid_out = torch.empty(max(n, 0), dtype=torch.uint8, device=self.device)
        self._check("offsets", offsets, (torch.int64,), 1)
        self._check("data", data, (torch.uint8,), 0)
        self._check_outputs(n, crc_out, valid_out)
        check(lib().ufc_crc_batch_varlen(self._ctx, self._bytes_ptr(data), _ptr(offsets), n, _ptr(crc_out), _ptr(valid_out),
                                         self._stream(stream)), "ufc_crc_batch_varlen")
        return crc_out, valid_out

    def seal_varlen(self, data, offsets, crc_out=None, stream=None):
        n = offsets.numel() - 1
        self._check("offsets", offsets, (torch.int64,), 1)
        self._check("data", data, (torch.uint8,), 0)
        self._check_outputs(n, crc_out)
        check(lib().ufc_seal_batch_varlen(self._ctx, self._bytes_ptr(data), _ptr(offsets), n, _ptr(crc_out),
                                          self._stream(stream)), "ufc_seal_batch_varlen")
        return crc_out

    def crc_pairs(self, data, pairs, crc_out=None, valid_out=None, want_crc=True, want_valid=True, stream=None):
        """pairs: int64 tensor [n, 2] of (start, end) byte offsets into data (any gapped layout)."""
        if pairs.dim() != 2 or pairs.shape[1] != 2:
            raise ValueError("pairs must have shape [n, 2]")
        n = pairs.shape[0]
        if crc_out is None and want_crc:
            crc_out = torch.empty(n, dtype=torch.int32, device=self.device)
        if valid_out is None and want_valid:
            valid_out = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._check("pairs", pairs, (torch.int64,), 2 * n)
        self._check("data", data, (torch.uint8,), 0)
        self._check_outputs(n, crc_out, valid_out)
        check(lib().ufc_crc_batch_pairs(self._ctx, self._bytes_ptr(data), data.numel(), _ptr(pairs), n, _ptr(crc_out),
                                        _ptr(valid_out), self._stream(stream)), "ufc_crc_batch_pairs")
        return crc_out, valid_out

    # ---- measurement context (not the CRC path) ----
    def hbm_read_probe(self, buf, sink, stream=None):
        """ufc_hbm_read_probe: read buf (uint8, device) as one plain stream, XOR into sink (int32[1]);
        returns the bytes read (whole KiB).  The bench's read-only streaming ceiling."""
        self._check("buf", buf, (torch.uint8,), 0)
        self._check("sink", sink, (torch.int32, torch.uint32), 1)
        nread = ctypes.c_size_t()
        check(lib().ufc_hbm_read_probe(self._ctx, _ptr(buf), buf.numel(), _ptr(sink), ctypes.byref(nread),
                                       self._stream(stream)), "ufc_hbm_read_probe")
        return nread.value

    # ---- the stage calls' argument helpers ----
    def _rec(self, name, t, dtype, count=None):
        """A record argument: uint8 rows of dtype.itemsize bytes each (what rows() makes), at least `count` of them,
        checked like _check before the C ABI sees the pointer.  Returns the number of records t holds (0 for None)."""
        if t is None:
            return 0
        w = dtype.itemsize
        self._check(name, t, (torch.uint8,), w * (count or 0))
        if t.numel() % w or (t.dim() == 2 and t.shape[1] != w):
            raise ValueError(f"{name} must hold rows of {w} bytes, got shape {tuple(t.shape)}")
        return t.numel() // w

    @contextlib.contextmanager
    def _outputs(self, stream):
        """Makes the stream a call is queued on torch's current one and yields z(given, count, kind): `given` when
        the caller supplied it, else `count` zeroed entries, filled on that stream.  kind: a record dtype (uint8 rows
        of its itemsize) or a torch dtype (1-D)."""
        def z(given, count, kind=torch.uint8):
            if given is not None:
                return given
            shape = (count, kind.itemsize) if isinstance(kind, np.dtype) else count
            return torch.zeros(shape, dtype=torch.uint8 if isinstance(kind, np.dtype) else kind, device=self.device)

        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            yield z

    # ---- Frame::read past the gate, on the device (uflow_frame_codec.h) ----
    def parse_varlen(self, data, offsets, valid, items_cap=None, stream=None):
        """Batched Frame::read of a CSR batch after the CRC gate (`valid`, from crc_varlen).
        Returns (infos rows[n], items rows[items_cap], items_used int64[1]) device tensors; the byte rows are
        ufc_frame_info / ufc_item records (records(infos, FRAME_INFO_DTYPE) reads them on the host).  items_cap
        defaults to a bound no batch can exceed."""
        n = offsets.numel() - 1
        self._check("offsets", offsets, (torch.int64,), 1)
        self._check("data", data, (torch.uint8,), 0)
        self._check("valid", valid, (torch.uint8,), n)
        if items_cap is None:  # a datagram takes >= 6 bytes, an ack group 9
            items_cap = max(1, data.numel() // 6)
        infos = torch.empty((max(n, 0), FRAME_INFO_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        items = torch.empty((items_cap, ITEM_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        used = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(lib().ufc_parse_batch_varlen(self._ctx, self._bytes_ptr(data), _ptr(offsets), n, _ptr(valid), _ptr(infos),
                                           _ptr(items), items_cap, _ptr(used), self._stream(stream)),
              "ufc_parse_batch_varlen")
        return infos, items, used

    # ---- Frame::write of a batch, on the device (uflow_frame_codec.h) ----
    def build_sizes_varlen(self, infos, items, payload_len, src_base=None, n_items=None, stream=None):
        """ufc_build_sizes_varlen: (out_offsets int64[n + 1], status uint8[n]) of the frames the records
        describe (infos rows[n] of ufc_frame_info, items rows of ufc_item: what parse_varlen returns)."""
        n = infos.shape[0]
        n_items = items.shape[0] if n_items is None else int(n_items)
        self._rec("infos", infos, FRAME_INFO_DTYPE, n)
        self._rec("items", items, ITEM_DTYPE, n_items)
        self._check("src_base", src_base, (torch.int64,), n)
        # (no fill kernel on torch's current stream: the call writes all n + 1 offsets on `stream`)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device) if n else \
            torch.zeros(1, dtype=torch.int64, device=self.device)
        status = torch.empty(n, dtype=torch.uint8, device=self.device)
        check(lib().ufc_build_sizes_varlen(self._ctx, _ptr(infos), _pn(items, n_items), n_items, _ptr(src_base),
                                           int(payload_len), n, _ptr(offsets), _ptr(status), self._stream(stream)),
              "ufc_build_sizes_varlen")
        return offsets, status

    def build_varlen(self, infos, items, payload, src_base=None, seal=True, out=None, stream=None, n_items=None,
                     crc_out=None):
        """Batched Frame::write: the frames that `infos` / `items` describe (the tensors parse_varlen
        returns; n_items = how many item rows are in use, default all) as a CSR batch, datagram payloads
        gathered from `payload` (uint8) at src_base[i] + data_offset (src_base int64[n], default zeros;
        a parsed batch's own offsets and bytes re-emit it).  Returns (out_bytes, out_offsets int64[n + 1],
        status uint8[n]); frames whose status is not UFC_BUILD_OK have length 0.  seal: write the CRC
        trailers (else 4 zero bytes each); crc_out (int32[n]) receives the CRC words then.  `out`: a
        uint8 tensor to write into (at least out_offsets[n] bytes), else one is allocated.  Reads
        out_offsets[n] on the host between the sizes and the write call (one synchronisation)."""
        n = infos.shape[0]
        n_items = items.shape[0] if n_items is None else int(n_items)
        self._check("payload", payload, (torch.uint8,), 0)
        self._check_outputs(n, crc_out)
        offsets, status = self.build_sizes_varlen(infos, items, payload.numel(), src_base, n_items, stream)
        if n == 0:
            return (out if out is not None else torch.empty(0, dtype=torch.uint8, device=self.device)), offsets, status
        if stream is not None:
            stream.synchronize()
        total = int(offsets[n].item())
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=self.device)
        self._check("out", out, (torch.uint8,), total)
        check(lib().ufc_build_batch_varlen(self._ctx, _ptr(infos), _pn(items, n_items), n_items, _ptr(src_base),
                                           _pn(payload, payload.numel()), payload.numel(), n, _ptr(offsets),
                                           _pn(out, out.numel()), out.numel(), 1 if seal else 0, _ptr(crc_out),
                                           self._stream(stream)), "ufc_build_batch_varlen")
        return out, offsets, status

    # ---- the emitters' push / finalize of many flushes, on the device (uflow_frame_codec.h) ----
    def pack_flushes(self, items, flush_first, flushes, frames_cap=None, nonce_bits=None, stream=None):
        """ufc_pack_varlen: cut every flush's items into frames as DataFrameEmitter / AckFrameEmitter do
        (src/half_connection/emit.rs:47-125, 170-211).  items rows[n_items] (ufc_item records, what parse_varlen
        returns), flush_first int64[n_flushes + 1] (CSR over the items), flushes rows[n_flushes] (ufc_flush records,
        FLUSH_DTYPE), nonce_bits int32 words (bit g: the nonce of the batch's g-th frame; default 0).  Returns (infos
        rows[frames_cap] of ufc_frame_info, results rows[n_flushes] of ufc_flush_result, frames_used int64[1]) device
        tensors; frames_cap defaults to n_items, which is always enough.  infos is one that build_varlen takes as is:
        the rows from frames_used on are zero, which the build skips (or pass infos[:frames_used])."""
        n_items = items.shape[0]
        n = flushes.shape[0]
        if frames_cap is None:
            frames_cap = n_items
        frames_cap = int(frames_cap)
        self._rec("items", items, ITEM_DTYPE, n_items)
        self._check("flush_first", flush_first, (torch.int64,), n + 1)
        self._rec("flushes", flushes, FLUSH_DTYPE, n)
        self._check("nonce_bits", nonce_bits, (torch.int32, torch.uint32), (frames_cap + 31) // 32)
        with self._outputs(stream) as z:
            infos, results = z(None, frames_cap, FRAME_INFO_DTYPE), z(None, n, FLUSH_RESULT_DTYPE)
            used = z(None, 1, torch.int64)
        check(lib().ufc_pack_varlen(self._ctx, _pn(items, n_items), n_items, _ptr(flush_first), _pn(flushes, n), n,
                                    _ptr(nonce_bits), _pn(infos, frames_cap), frames_cap, _pn(results, n), _ptr(used),
                                    self._stream(stream)), "ufc_pack_varlen")
        return infos, results, used

    # ---- PacketSender::emit_packet and fragmentation of many senders, on the device (uflow_frame_codec.h) ----
    def emit_packets(self, packets, packet_first, senders, items_cap, items=None, senders_out=None,
                     want_packet_results=True, stream=None):
        """ufc_emit_packets_varlen: turn every sender's queued packets into datagram items as
        PacketSender::emit_packet and PendingPacket do (src/half_connection/packet_sender.rs:149-238,
        pending_packet.rs:23-42, 84-103).  packets rows[n_packets] (ufc_packet records, PACKET_DTYPE), packet_first
        int64[n_senders + 1] (CSR over the packets), senders rows[n_senders] (ufc_sender records, SENDER_DTYPE).
        Returns (items rows[items_cap] of ufc_item, flush_first int64[n_senders + 1], packet_results rows[n_packets]
        of ufc_packet_result or None, sender_results rows[n_senders] of ufc_sender_result, senders_out
        rows[n_senders], items_used int64[1]) device tensors: items and flush_first are what pack_flushes takes
        (items[:items_used] when items_cap is larger).  Items at an index >= items_cap are not written (compare
        items_used); each sender's reserve_items slots stay as they were (zero in a tensor allocated here).  `items`:
        a tensor to write into; senders_out: where the state after the consumed packets goes (may be `senders`)."""
        n_packets = packets.shape[0]
        n = senders.shape[0]
        items_cap = int(items_cap)
        self._rec("packets", packets, PACKET_DTYPE, n_packets)
        self._check("packet_first", packet_first, (torch.int64,), n + 1)
        self._rec("senders", senders, SENDER_DTYPE, n)
        self._rec("items", items, ITEM_DTYPE, items_cap)
        self._rec("senders_out", senders_out, SENDER_DTYPE, n)
        with self._outputs(stream) as z:
            items = z(items, items_cap, ITEM_DTYPE)
            flush_first = z(None, n + 1, torch.int64)
            packet_results = z(None, n_packets, PACKET_RESULT_DTYPE) if want_packet_results else None
            sender_results = z(None, n, SENDER_RESULT_DTYPE)
            senders_out = z(senders_out, n, SENDER_DTYPE)
            used = z(None, 1, torch.int64)
        check(lib().ufc_emit_packets_varlen(self._ctx, _pn(packets, n_packets), n_packets, _ptr(packet_first),
                                            _pn(senders, n), n, _pn(items, items_cap), items_cap, _ptr(flush_first),
                                            _pn(packet_results, n_packets), _pn(sender_results, n), _pn(senders_out, n),
                                            _ptr(used), self._stream(stream)), "ufc_emit_packets_varlen")
        return items, flush_first, packet_results, sender_results, senders_out, used

    # ---- PacketReceiver's step for many receivers, on the device (uflow_frame_codec.h) ----
    def receive_packets(self, infos, items, payload, frame_first, receivers, slots, slot_first, carry_in,
                        src_base=None, frame_accept=None, carry_cap=None, out_cap=None, packets_cap=None,
                        carry_out=None, out_bytes=None, packets=None, receivers_out=None, want_item_status=True,
                        stream=None):
        """ufc_receive_packets_varlen: one step of PacketReceiver (handle_datagram, receive, resynchronize;
        src/half_connection/packet_receiver/mod.rs:142-435) for every receiver.  infos rows[n_frames] and items
        rows[n_items] (what parse_varlen returns), payload uint8 (the frames' bytes) with src_base int64[n_frames]
        (the parse's offsets; None: zero), frame_first int64[n_receivers + 1] (CSR over the frames), receivers
        rows[n_receivers] (ufc_receiver records, RECEIVER_DTYPE), slots rows[n_slots] (ufc_rx_slot, updated in
        place), slot_first int64[n_receivers + 1], carry_in uint8 (the carry arena the slots point into),
        frame_accept uint8[n_frames] or None.  Returns a dict of device tensors: packets rows[packets_cap] of
        ufc_rx_packet, packet_first int64[n + 1], packets_used, out_bytes, out_used, carry_out, carry_first
        int64[n + 1], carry_used, item_status uint8[n_items] or None, results rows[n] of ufc_receiver_result,
        receivers_out rows[n] (may be given as `receivers`).  Caps that are not given are what the step needs,
        found by a first pass on a copy of the state with caps of zero, whose counts are read back (this waits for
        the stream; give the caps or the tensors to stay asynchronous: an ACTIVE slot holds its whole fragment
        buffer, so the carry has no small bound from the batch's sizes alone, see the header); tensors given for
        carry_out, out_bytes and packets are written into.
        Pass carry_out[:carry_used] as the next step's carry_in (carry_out must not overlap carry_in)."""
        n_frames, n_items, n, n_slots = infos.shape[0], items.shape[0], receivers.shape[0], slots.shape[0]
        self._rec("infos", infos, FRAME_INFO_DTYPE, n_frames)
        self._rec("items", items, ITEM_DTYPE, n_items)
        self._check("payload", payload, (torch.uint8,), 0)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._rec("receivers", receivers, RECEIVER_DTYPE, n)
        self._rec("slots", slots, RX_SLOT_DTYPE, n_slots)
        self._check("slot_first", slot_first, (torch.int64,), n + 1)
        self._check("carry_in", carry_in, (torch.uint8,), 0)
        self._check("src_base", src_base, (torch.int64,), n_frames)
        self._check("frame_accept", frame_accept, (torch.uint8,), n_frames)
        self._rec("receivers_out", receivers_out, RECEIVER_DTYPE, n)
        self._check("carry_out", carry_out, (torch.uint8,), 0)
        self._check("out_bytes", out_bytes, (torch.uint8,), 0)
        self._rec("packets", packets, RX_PACKET_DTYPE)

        def p(t):
            return _pn(t, t is not None and t.numel())

        def size(t, width=1):
            return 0 if t is None else t.numel() // width

        def call(slots_, carry_out_, out_bytes_, packets_, status_, receivers_out_):
            check(lib().ufc_receive_packets_varlen(
                self._ctx, p(infos), n_frames, p(frame_accept), p(items), n_items, p(src_base), p(payload),
                payload.numel(), _ptr(frame_first), p(receivers), n, p(slots_), _ptr(slot_first), n_slots, p(carry_in),
                carry_in.numel(), p(carry_out_), size(carry_out_), _ptr(carry_first),
                ctypes.c_void_p(used.data_ptr() + 16), p(packets_), size(packets_, RX_PACKET_DTYPE.itemsize),
                _ptr(packet_first), ctypes.c_void_p(used.data_ptr()), p(out_bytes_), size(out_bytes_),
                ctypes.c_void_p(used.data_ptr() + 8), p(status_), p(results), p(receivers_out_), self._stream(stream)),
                "ufc_receive_packets_varlen")

        with self._outputs(stream) as z:
            carry_first, packet_first = z(None, n + 1, torch.int64), z(None, n + 1, torch.int64)
            used = z(None, 3, torch.int64)
            results = z(None, n, RECEIVER_RESULT_DTYPE)
            need = [(carry_out, carry_cap), (out_bytes, out_cap), (packets, packets_cap)]
            if n and any(t is None and cap is None for t, cap in need):
                # The used counts are exact whatever the caps: a first pass on a copy of the state, with none.
                # Reading them back waits for the stream: give the caps (or the tensors) to stay asynchronous.
                call(slots.clone(), None, None, None, None, z(None, n, RECEIVER_DTYPE))
                u = used.cpu().tolist()
                packets_cap = u[0] if packets_cap is None else packets_cap
                out_cap = u[1] if out_cap is None else out_cap
                carry_cap = u[2] if carry_cap is None else carry_cap
            carry_out = z(carry_out, int(carry_cap or 0))
            out_bytes = z(out_bytes, int(out_cap or 0))
            packets = z(packets, int(packets_cap or 0), RX_PACKET_DTYPE)
            receivers_out = z(receivers_out, n, RECEIVER_DTYPE)
            item_status = z(None, n_items) if want_item_status else None
        call(slots, carry_out, out_bytes, packets, item_status, receivers_out)
        return {"packets": packets, "packet_first": packet_first, "packets_used": used[0:1], "out_bytes": out_bytes,
                "out_used": used[1:2], "carry_out": carry_out, "carry_first": carry_first, "carry_used": used[2:3],
                "item_status": item_status, "results": results, "receivers_out": receivers_out}

    # ---- FrameAckQueue's step for many connections, on the device (uflow_frame_codec.h) ----
    def frame_window(self, infos, frame_first, windows, groups_cap=None, frame_accept=None, groups=None,
                     windows_out=None, stream=None):
        """ufc_frame_window_varlen: one step of FrameAckQueue (window_contains, mark_seen, resynchronize;
        src/half_connection/frame_ack_queue.rs as half_connection/mod.rs:132-152 drives it) for every connection.
        infos rows[n_frames] (what parse_varlen returns), frame_first int64[n + 1] (CSR over the frames, the one
        receive_packets takes), windows rows[n] (ufc_frame_window records, FRAME_WINDOW_DTYPE).  Returns a dict of
        device tensors: frame_accept uint8[n_frames] (1 for the data frames inside the window: pass it to
        receive_packets), groups rows[groups_cap] (ack groups as ufc_item records, each connection's carried tail
        first), group_first int64[n + 1] (CSR over the groups: pack_flushes' flush_first), groups_used int64[1],
        results rows[n] of ufc_frame_window_result, windows_out rows[n] (may be given as `windows`).  groups_cap
        defaults to n + n_frames, which is always enough; groups at an index >= groups_cap are not written (compare
        groups_used).  Tensors given for frame_accept, groups and windows_out are written into."""
        n_frames, n = infos.shape[0], windows.shape[0]
        if groups_cap is None:
            groups_cap = groups.shape[0] if groups is not None else n + n_frames
        groups_cap = int(groups_cap)
        self._rec("infos", infos, FRAME_INFO_DTYPE, n_frames)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._rec("windows", windows, FRAME_WINDOW_DTYPE, n)
        self._check("frame_accept", frame_accept, (torch.uint8,), n_frames)
        self._rec("groups", groups, ITEM_DTYPE, groups_cap)
        self._rec("windows_out", windows_out, FRAME_WINDOW_DTYPE, n)
        with self._outputs(stream) as z:
            frame_accept = z(frame_accept, n_frames)
            # (the pointer is required even when there are no frames, and an empty tensor has none)
            accept_arg = frame_accept if n_frames else z(None, 1)
            groups = z(groups, groups_cap, ITEM_DTYPE)
            windows_out = z(windows_out, n, FRAME_WINDOW_DTYPE)
            group_first = z(None, n + 1, torch.int64)
            results = z(None, n, FRAME_WINDOW_RESULT_DTYPE)
            used = z(None, 1, torch.int64)
        check(lib().ufc_frame_window_varlen(self._ctx, _pn(infos, n_frames), n_frames, _ptr(frame_first),
                                            _pn(windows, n), n, _pn(accept_arg, n), _pn(groups, groups_cap), groups_cap,
                                            _ptr(group_first), _ptr(used), _pn(results, n), _pn(windows_out, n),
                                            self._stream(stream)), "ufc_frame_window_varlen")
        return {"frame_accept": frame_accept, "groups": groups, "group_first": group_first, "groups_used": used,
                "results": results, "windows_out": windows_out}

    # ---- the sender's FrameQueue step for many connections, on the device (uflow_frame_codec.h) ----
    def frame_queue(self, infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked=None,
                    queues_out=None, stream=None):
        """ufc_frame_queue_varlen: one step of the sender's FrameQueue (push, acknowledge_group,
        advance_transfer_window, forget_frames, get_feedback; src/half_connection/frame_queue.rs with
        reorder_buffer.rs and loss_rate.rs) for every connection.  infos rows[n_frames] and items rows[n_items] (what
        parse_varlen returns), frame_first int64[n + 1] (CSR over the frames), sent rows[n_sent] (ufc_sent_frame
        records to push) with sent_first int64[n + 1], queues rows[n] (FRAME_QUEUE_DTYPE), steps rows[n]
        (FRAME_QUEUE_STEP_DTYPE), log rows[n_log] (SENT_FRAME_DTYPE: the log arena, updated in place), ref_acked
        uint8[refs_cap] or None (set to 1 for the fragments of newly acked frames, in place).  Returns a dict of
        device tensors: results rows[n] (FRAME_QUEUE_RESULT_DTYPE), queues_out rows[n] (may be given as `queues`),
        log, ref_acked."""
        n_frames, n_items, n_sent, n, n_log = infos.shape[0], items.shape[0], sent.shape[0], queues.shape[0], log.shape[0]
        refs_cap = ref_acked.shape[0] if ref_acked is not None else 0
        self._rec("infos", infos, FRAME_INFO_DTYPE, n_frames)
        self._rec("items", items, ITEM_DTYPE, n_items)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._rec("sent", sent, SENT_FRAME_DTYPE, n_sent)
        self._check("sent_first", sent_first, (torch.int64,), n + 1)
        self._rec("queues", queues, FRAME_QUEUE_DTYPE, n)
        self._rec("steps", steps, FRAME_QUEUE_STEP_DTYPE, n)
        self._rec("log", log, SENT_FRAME_DTYPE, n_log)
        self._check("ref_acked", ref_acked, (torch.uint8,), refs_cap)
        self._rec("queues_out", queues_out, FRAME_QUEUE_DTYPE, n)
        with self._outputs(stream) as z:
            queues_out = z(queues_out, n, FRAME_QUEUE_DTYPE)
            results = z(None, n, FRAME_QUEUE_RESULT_DTYPE)
        check(lib().ufc_frame_queue_varlen(self._ctx, _pn(infos, n_frames), n_frames, _pn(items, n_items), n_items,
                                           _ptr(frame_first), _pn(sent, n_sent), n_sent, _ptr(sent_first),
                                           _pn(queues, n), _pn(steps, n), n, _pn(log, n_log), n_log,
                                           _pn(ref_acked, refs_cap), refs_cap, _pn(results, n), _pn(queues_out, n),
                                           self._stream(stream)), "ufc_frame_queue_varlen")
        return {"results": results, "queues_out": queues_out, "log": log, "ref_acked": ref_acked}

    # ---- the send rate control around the frame queue call, on the device (uflow_frame_codec.h) ----
    def rate_begin(self, states, now_ms, extra_flags=None, steps=None, states_out=None, stream=None):
        """ufc_rate_begin_varlen: opens a tick.  states rows[n] (RATE_STATE_DTYPE records), now_ms int64[n],
        extra_flags int32[n] or None (OR-ed into the steps' flags: FQ_MARK_RATE_LIMITED).  Returns a dict of device
        tensors: steps rows[n] (FRAME_QUEUE_STEP_DTYPE: what frame_queue takes), states_out rows[n] (may be given as
        `states`)."""
        n = states.shape[0]
        self._rec("states", states, RATE_STATE_DTYPE, n)
        self._check("now_ms", now_ms, (torch.int64, torch.uint64), n)
        self._check("extra_flags", extra_flags, (torch.int32, torch.uint32), n)
        self._rec("steps", steps, FRAME_QUEUE_STEP_DTYPE, n)
        self._rec("states_out", states_out, RATE_STATE_DTYPE, n)
        with self._outputs(stream) as z:
            steps, states_out = z(steps, n, FRAME_QUEUE_STEP_DTYPE), z(states_out, n, RATE_STATE_DTYPE)
        check(lib().ufc_rate_begin_varlen(self._ctx, _pn(states, n), _pn(now_ms, n), _pn(extra_flags, n), n,
                                          _pn(steps, n), _pn(states_out, n), self._stream(stream)),
              "ufc_rate_begin_varlen")
        return {"steps": steps, "states_out": states_out}

    def rate_step(self, states, ticks, fq_results, entries, flush_results=None, result_index=None, flushes=None,
                  flush_index=None, results=None, states_out=None, stream=None):
        """ufc_rate_step_varlen: closes a tick behind frame_queue (notify_frame_sent, fill_flush_alloc and
        SendRateComp::step; src/half_connection/send_rate.rs, recv_rate_set.rs, mod.rs:165-215) for every connection.
        states rows[n] (RATE_STATE_DTYPE), ticks rows[n] (RATE_TICK_DTYPE), fq_results rows[n] (frame_queue's
        results), entries rows[n_entries] (RECV_RATE_ENTRY_DTYPE: the receive-rate sets, updated in place);
        flush_results rows[m] (FLUSH_RESULT_DTYPE) with result_index int32[n] (the last data flush of each
        connection, -1 for none) and flushes rows[k] (FLUSH_DTYPE) with flush_index int32[n] (where the new
        flush_alloc goes, in place) are optional.  Returns a dict of device tensors: results rows[n]
        (RATE_RESULT_DTYPE), states_out rows[n] (may be given as `states`), entries, flushes."""
        n, n_entries = states.shape[0], entries.shape[0]
        n_fr = flush_results.shape[0] if flush_results is not None else 0
        n_fl = flushes.shape[0] if flushes is not None else 0
        if (n_fr and result_index is None) or (n_fl and flush_index is None):
            raise ValueError("flush_results needs result_index, flushes needs flush_index")
        self._rec("states", states, RATE_STATE_DTYPE, n)
        self._rec("ticks", ticks, RATE_TICK_DTYPE, n)
        self._rec("fq_results", fq_results, FRAME_QUEUE_RESULT_DTYPE, n)
        self._rec("entries", entries, RECV_RATE_ENTRY_DTYPE, n_entries)
        self._rec("flush_results", flush_results, FLUSH_RESULT_DTYPE, n_fr)
        self._check("result_index", result_index, (torch.int32, torch.uint32), n)
        self._rec("flushes", flushes, FLUSH_DTYPE, n_fl)
        self._check("flush_index", flush_index, (torch.int32, torch.uint32), n)
        self._rec("results", results, RATE_RESULT_DTYPE, n)
        self._rec("states_out", states_out, RATE_STATE_DTYPE, n)
        with self._outputs(stream) as z:
            results, states_out = z(results, n, RATE_RESULT_DTYPE), z(states_out, n, RATE_STATE_DTYPE)
        check(lib().ufc_rate_step_varlen(self._ctx, _pn(states, n), _pn(ticks, n), _pn(fq_results, n), n,
                                         _pn(entries, n_entries), n_entries, _pn(flush_results, n_fr), n_fr,
                                         _pn(result_index, n_fr), _pn(flushes, n_fl), n_fl, _pn(flush_index, n_fl),
                                         _pn(results, n), _pn(states_out, n), self._stream(stream)),
              "ufc_rate_step_varlen")
        return {"results": results, "states_out": states_out, "entries": entries, "flushes": flushes}

    # ---- the resend calls around the emit and the pack, on the device (uflow_frame_codec.h) ----
    def _rs_arenas(self, arenas, *names):
        """(pointer, record count) of the named resend arenas, flat, in the order the C calls take them; the arenas
        are device rows of frame.RESEND_ARENAS' dtypes."""
        out = []
        for name in names:
            t = arenas.get(name)
            count = self._rec(name, t, _RS_ARENA_DTYPE[name])
            out += [_pn(t, count), count]
        return out

    def resend_begin(self, infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags=None,
                     results=None, states_out=None, senders_out=None, stream=None):
        """ufc_resend_begin_varlen: behind rate_step, in front of emit_packets.  Ack propagation from ref_acked,
        PacketSender::acknowledge for the ack frames, the resend loop (the heap and the pack's rule) and the pending
        fragments' staging for every connection.  infos rows[n_frames], frame_first int64[n + 1], queues rows[n] and
        log rows[n_log] as frame_queue left them, rate rows[n] (rate_step's results), flushes rows[n] (the data
        flushes the pack gets), states rows[n] (RESEND_DTYPE), senders rows[n] (SENDER_DTYPE), arenas a dict of
        device rows heap, pkts, frag_acked, tx, ref_acked, stage (frame.RESEND_ARENAS names their records; updated in
        place), flags int32[n] or None.  Returns a dict: results rows[n] (RESEND_RESULT_DTYPE), states_out,
        senders_out (may be given as `states`, `senders`)."""
        n_frames, n, n_log = infos.shape[0], states.shape[0], log.shape[0]
        self._rec("infos", infos, FRAME_INFO_DTYPE, n_frames)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._rec("queues", queues, FRAME_QUEUE_DTYPE, n)
        self._rec("log", log, SENT_FRAME_DTYPE, n_log)
        self._rec("rate", rate, RATE_RESULT_DTYPE, n)
        self._rec("flushes", flushes, FLUSH_DTYPE, n)
        self._rec("states", states, RESEND_DTYPE, n)
        self._rec("senders", senders, SENDER_DTYPE, n)
        self._check("flags", flags, (torch.int32, torch.uint32), n)
        self._rec("results", results, RESEND_RESULT_DTYPE, n)
        self._rec("states_out", states_out, RESEND_DTYPE, n)
        self._rec("senders_out", senders_out, SENDER_DTYPE, n)
        A = self._rs_arenas(arenas, "heap", "pkts", "frag_acked", "tx", "ref_acked", "stage")
        with self._outputs(stream) as z:
            results, states_out = z(results, n, RESEND_RESULT_DTYPE), z(states_out, n, RESEND_DTYPE)
            senders_out = z(senders_out, n, SENDER_DTYPE)
        check(lib().ufc_resend_begin_varlen(
            self._ctx, _pn(infos, n_frames), n_frames, _ptr(frame_first), _pn(queues, n), _pn(log, n_log), n_log,
            _pn(rate, n), _pn(flags, n), _pn(flushes, n), _pn(states, n), _pn(senders, n), n, *A, _pn(results, n),
            _pn(states_out, n), _pn(senders_out, n), self._stream(stream)), "ufc_resend_begin_varlen")
        return {"results": results, "states_out": states_out, "senders_out": senders_out}

    def resend_place(self, states, begin_results, arenas, flush_first, items, stream=None):
        """ufc_resend_place_varlen: behind emit_packets.  Every connection's staged items into items[flush_first[c]
        ..], the slots the emit reserved; items rows[items_cap] of ufc_item is written in place and returned."""
        n = states.shape[0]
        self._rec("states", states, RESEND_DTYPE, n)
        self._rec("begin_results", begin_results, RESEND_RESULT_DTYPE, n)
        self._check("flush_first", flush_first, (torch.int64,), n + 1)
        items_cap = self._rec("items", items, ITEM_DTYPE)
        check(lib().ufc_resend_place_varlen(self._ctx, _pn(states, n), _pn(begin_results, n), n,
                                            *self._rs_arenas(arenas, "stage"), _ptr(flush_first), _pn(items, items_cap),
                                            items_cap, self._stream(stream)), "ufc_resend_place_varlen")
        return items

    def resend_commit(self, flush_results, infos, out_offsets, frames_used, items, flush_first, packets, packet_first,
                      packet_results, sender_results, begin_results, rate, states, senders, arenas, sent=None,
                      next_extra_flags=None, results=None, states_out=None, retake=None, stream=None):
        """ufc_resend_commit_varlen: behind pack_flushes over the data flushes (flush c = connection c) and
        build_sizes.  flush_results rows[n], infos rows[n_infos] (the pack's frames), out_offsets int64[n_infos + 1]
        (the size pass), frames_used int64[1] (the pack's), items rows[n_items], flush_first int64[n + 1], packets
        rows[n_packets], packet_first int64[n + 1], packet_results rows[n_packets] and sender_results rows[n] (the
        first emit's), begin_results rows[n], rate rows[n], states rows[n], senders rows[n] (as resend_begin wrote
        them), arenas as in resend_begin (updated in place), next_extra_flags int32[n] or None (in place).  Returns a
        dict: results rows[n] (RESEND_COMMIT_RESULT_DTYPE), states_out, retake (the second emit's senders), sent
        rows[n_infos] (SENT_FRAME_DTYPE), sent_first int64[n + 1], next_extra_flags."""
        n, n_infos, n_items, n_packets = states.shape[0], infos.shape[0], items.shape[0], packets.shape[0]
        self._rec("flush_results", flush_results, FLUSH_RESULT_DTYPE, n)
        self._rec("infos", infos, FRAME_INFO_DTYPE, n_infos)
        self._check("out_offsets", out_offsets, (torch.int64,), n_infos + 1)
        self._check("frames_used", frames_used, (torch.int64,), 1)
        self._rec("items", items, ITEM_DTYPE, n_items)
        self._check("flush_first", flush_first, (torch.int64,), n + 1)
        self._rec("packets", packets, PACKET_DTYPE, n_packets)
        self._check("packet_first", packet_first, (torch.int64,), n + 1)
        self._rec("packet_results", packet_results, PACKET_RESULT_DTYPE, n_packets)
        self._rec("sender_results", sender_results, SENDER_RESULT_DTYPE, n)
        self._rec("begin_results", begin_results, RESEND_RESULT_DTYPE, n)
        self._rec("rate", rate, RATE_RESULT_DTYPE, n)
        self._rec("states", states, RESEND_DTYPE, n)
        self._rec("senders", senders, SENDER_DTYPE, n)
        sent_cap = self._rec("sent", sent, SENT_FRAME_DTYPE) if sent is not None else n_infos
        self._check("next_extra_flags", next_extra_flags, (torch.int32, torch.uint32), n)
        self._rec("results", results, RESEND_COMMIT_RESULT_DTYPE, n)
        self._rec("states_out", states_out, RESEND_DTYPE, n)
        self._rec("retake", retake, SENDER_DTYPE, n)
        A = self._rs_arenas(arenas, "heap", "pkts", "frag_acked", "tx")
        with self._outputs(stream) as z:
            sent = z(sent, n_infos, SENT_FRAME_DTYPE)
            results, states_out = z(results, n, RESEND_COMMIT_RESULT_DTYPE), z(states_out, n, RESEND_DTYPE)
            retake = z(retake, n, SENDER_DTYPE)
            sent_first = z(None, n + 1, torch.int64)
        check(lib().ufc_resend_commit_varlen(
            self._ctx, _pn(flush_results, n), _pn(infos, n_infos), n_infos, _ptr(out_offsets), _ptr(frames_used),
            _pn(items, n_items), n_items, _ptr(flush_first), _pn(packets, n_packets), n_packets, _ptr(packet_first),
            _pn(packet_results, n_packets), _pn(sender_results, n), _pn(begin_results, n), _pn(rate, n), _pn(states, n),
            _pn(senders, n), n, *A, _pn(sent, sent_cap), sent_cap, _ptr(sent_first), _pn(next_extra_flags, n),
            _pn(results, n), _pn(states_out, n), _pn(retake, n), self._stream(stream)), "ufc_resend_commit_varlen")
        return {"results": results, "states_out": states_out, "retake": retake, "sent": sent, "sent_first": sent_first,
                "next_extra_flags": next_extra_flags}

    # ---- the flush control around the data flush, on the device (uflow_flush_ctl.h) ----
    def flush_acks(self, ctl, windows, groups, group_first, receivers, rate, carry, merged_cap=None, frames_cap=None,
                   flushes=None, flags=None, merged=None, infos=None, windows_out=None, ctl_out=None, stream=None):
        """ufc_flush_acks_varlen: emit_ack_frames with push_dud and the deque carry (half_connection/mod.rs:296-333
        over emit.rs:137-211) for every connection, behind frame_window and rate_step, in front of resend_begin.  ctl
        rows[n] (FLUSH_CTL_DTYPE), windows rows[n], groups rows[n_groups] and group_first int64[n + 1] as frame_window
        left them, receivers rows[n], rate rows[n] (rate_step's results), carry rows[n_carry] (ufc_item: the carry
        arena, updated in place), flushes rows[n] (the data flushes) and flags int32[n] optional, in place.  Returns a
        dict of device tensors: merged rows[merged_cap], merged_first int64[n + 1] (the ack flushes' flush_first),
        merged_used int64[1], infos rows[frames_cap] (the ack frames: build_varlen takes them over merged),
        frames_used int64[1], results rows[n] (FLUSH_RESULT_DTYPE), ack_results rows[n] (FLUSH_ACKS_RESULT_DTYPE),
        windows_out, ctl_out (may be given as `windows`, `ctl`), carry, flushes, flags.  merged_cap defaults to n_carry
        + n_groups and frames_cap to n + merged_cap, which are always enough."""
        n, n_groups = ctl.shape[0], groups.shape[0]
        self._rec("ctl", ctl, FLUSH_CTL_DTYPE, n)
        self._rec("windows", windows, FRAME_WINDOW_DTYPE, n)
        self._rec("groups", groups, ITEM_DTYPE, n_groups)
        self._check("group_first", group_first, (torch.int64,), n + 1)
        self._rec("receivers", receivers, RECEIVER_DTYPE, n)
        self._rec("rate", rate, RATE_RESULT_DTYPE, n)
        n_carry = self._rec("carry", carry, ITEM_DTYPE)
        if merged_cap is None:
            merged_cap = merged.shape[0] if merged is not None else n_carry + n_groups
        merged_cap = int(merged_cap)
        if frames_cap is None:
            frames_cap = infos.shape[0] if infos is not None else n + merged_cap
        frames_cap = int(frames_cap)
        self._rec("merged", merged, ITEM_DTYPE, merged_cap)
        self._rec("infos", infos, FRAME_INFO_DTYPE, frames_cap)
        self._rec("flushes", flushes, FLUSH_DTYPE, n)
        self._check("flags", flags, (torch.int32, torch.uint32), n)
        self._rec("windows_out", windows_out, FRAME_WINDOW_DTYPE, n)
        self._rec("ctl_out", ctl_out, FLUSH_CTL_DTYPE, n)
        with self._outputs(stream) as z:
            merged, infos = z(merged, merged_cap, ITEM_DTYPE), z(infos, frames_cap, FRAME_INFO_DTYPE)
            windows_out, ctl_out = z(windows_out, n, FRAME_WINDOW_DTYPE), z(ctl_out, n, FLUSH_CTL_DTYPE)
            merged_first = z(None, n + 1, torch.int64)
            results, ack_results = z(None, n, FLUSH_RESULT_DTYPE), z(None, n, FLUSH_ACKS_RESULT_DTYPE)
            merged_used, frames_used = z(None, 1, torch.int64), z(None, 1, torch.int64)
        check(lib().ufc_flush_acks_varlen(
            self._ctx, _pn(ctl, n), _pn(windows, n), _pn(groups, n_groups), n_groups, _ptr(group_first),
            _pn(receivers, n), _pn(rate, n), n, _pn(carry, n_carry), n_carry, _pn(merged, merged_cap), merged_cap,
            _ptr(merged_first), _ptr(merged_used), _pn(infos, frames_cap), frames_cap, _ptr(frames_used),
            _pn(results, n), _pn(ack_results, n), _pn(windows_out, n), _pn(ctl_out, n), _pn(flushes, n), _pn(flags, n),
            self._stream(stream)), "ufc_flush_acks_varlen")
        return {"merged": merged, "merged_first": merged_first, "merged_used": merged_used, "infos": infos,
                "frames_used": frames_used, "results": results, "ack_results": ack_results, "windows_out": windows_out,
                "ctl_out": ctl_out, "carry": carry, "flushes": flushes, "flags": flags}

    def flush_sync(self, ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders,
                   syncs_cap=None, ticks_next=None, infos=None, ctl_out=None, stream=None):
        """ufc_flush_sync_varlen: emit_sync_frame and emit_frames' early returns (half_connection/mod.rs:217-294) for
        every connection, behind the data flush's last call.  ctl rows[n] (FLUSH_CTL_DTYPE), rate rows[n] (rate_step's
        results), ack_results rows[n] (flush_acks' results, FLUSH_RESULT_DTYPE), begin_results rows[n], pack_results
        rows[n] (the data pack's), commit_results rows[n], queues rows[n] (after this tick's frame_queue), senders
        rows[n] (as the second emit left them), ticks_next rows[n] (RATE_TICK_DTYPE, optional: alloc_adjust = -14 or 0,
        in place).  Returns a dict of device tensors: infos rows[syncs_cap] (the sync frames in connection order:
        build_varlen takes them), sync_index int32[n] (-1: none), syncs_used int64[1], results rows[n]
        (FLUSH_SYNC_RESULT_DTYPE), ctl_out (may be given as `ctl`), ticks_next.  syncs_cap defaults to n."""
        n = ctl.shape[0]
        self._rec("ctl", ctl, FLUSH_CTL_DTYPE, n)
        self._rec("rate", rate, RATE_RESULT_DTYPE, n)
        self._rec("ack_results", ack_results, FLUSH_RESULT_DTYPE, n)
        self._rec("begin_results", begin_results, RESEND_RESULT_DTYPE, n)
        self._rec("pack_results", pack_results, FLUSH_RESULT_DTYPE, n)
        self._rec("commit_results", commit_results, RESEND_COMMIT_RESULT_DTYPE, n)
        self._rec("queues", queues, FRAME_QUEUE_DTYPE, n)
        self._rec("senders", senders, SENDER_DTYPE, n)
        if syncs_cap is None:
            syncs_cap = infos.shape[0] if infos is not None else n
        syncs_cap = int(syncs_cap)
        self._rec("infos", infos, FRAME_INFO_DTYPE, syncs_cap)
        self._rec("ticks_next", ticks_next, RATE_TICK_DTYPE, n)
        self._rec("ctl_out", ctl_out, FLUSH_CTL_DTYPE, n)
        with self._outputs(stream) as z:
            infos, ctl_out = z(infos, syncs_cap, FRAME_INFO_DTYPE), z(ctl_out, n, FLUSH_CTL_DTYPE)
            sync_index = z(None, n, torch.int32)
            results = z(None, n, FLUSH_SYNC_RESULT_DTYPE)
            used = z(None, 1, torch.int64)
        check(lib().ufc_flush_sync_varlen(
            self._ctx, _pn(ctl, n), _pn(rate, n), _pn(ack_results, n), _pn(begin_results, n), _pn(pack_results, n),
            _pn(commit_results, n), _pn(queues, n), _pn(senders, n), n, _pn(infos, syncs_cap), syncs_cap,
            _pn(sync_index, n), _ptr(used), _pn(results, n), _pn(ctl_out, n), _pn(ticks_next, n),
            self._stream(stream)), "ufc_flush_sync_varlen")
        return {"infos": infos, "sync_index": sync_index, "syncs_used": used, "results": results, "ctl_out": ctl_out,
                "ticks_next": ticks_next}

    # ---- the frame routing in front of the frame window, on the device (uflow_route.h) ----
    def route_frames(self, infos, addrs, offsets, slots, seed, max_probe, conn_active, now_ms, active_timeout_ms,
                     timeout_in, infos_out=None, src_base_out=None, timeout_out=None, stream=None):
        """ufc_route_frames_varlen: the address lookup and dispatch of Server::handle_frames (server/mod.rs:591-602)
        for every frame of a parsed batch, behind parse_varlen, in front of frame_window.  infos rows[n] as the parse
        left them, addrs rows[n] (ADDR_DTYPE), offsets int64[n] or None (read as all zero), slots rows[n_slots]
        (ROUTE_SLOT_DTYPE: uflow_amd.route.new_route_table's, uploaded) with its seed and max_probe, conn_active
        uint8[n_conns], timeout_in int64[n_conns].  Returns a dict of device tensors: route int32[n], cls uint8[n],
        bucket_first int64[n_conns + 3] (its first n_conns + 1 entries are the stages' frame_first), order int32[n],
        infos_out rows[n] and src_base_out int64[n] (the stages' infos and src_base), results rows[n_conns]
        (ROUTE_RESULT_DTYPE), timeout_out (may be given as `timeout_in`), first_unknown_control int32[1]."""
        n = infos.shape[0]
        n_conns = conn_active.numel()
        self._rec("infos", infos, FRAME_INFO_DTYPE, n)
        self._rec("addrs", addrs, ADDR_DTYPE, n)
        self._check("offsets", offsets, (torch.int64,), n)
        n_slots = self._rec("slots", slots, ROUTE_SLOT_DTYPE)
        self._check("conn_active", conn_active, (torch.uint8,), n_conns)
        self._check("timeout_in", timeout_in, (torch.int64,), n_conns)
        self._rec("infos_out", infos_out, FRAME_INFO_DTYPE, n)
        self._check("src_base_out", src_base_out, (torch.int64,), n)
        self._check("timeout_out", timeout_out, (torch.int64,), n_conns)
        with self._outputs(stream) as z:
            infos_out, src_base_out = z(infos_out, n, FRAME_INFO_DTYPE), z(src_base_out, n, torch.int64)
            timeout_out = z(timeout_out, n_conns, torch.int64)
            route, cls, order = z(None, n, torch.int32), z(None, n, torch.uint8), z(None, n, torch.int32)
            bucket_first = z(None, n_conns + 3, torch.int64)
            results = z(None, n_conns, ROUTE_RESULT_DTYPE)
            fuc = z(None, 1, torch.int32)
        check(lib().ufc_route_frames_varlen(
            self._ctx, _pn(infos, n), _pn(addrs, n), _pn(offsets, n), n, _pn(slots, n_slots), n_slots,
            int(seed) & 0xFFFFFFFF, int(max_probe) & 0xFFFFFFFF, n_conns, _pn(conn_active, n_conns),
            int(now_ms) & (2**64 - 1), int(active_timeout_ms) & (2**64 - 1), _pn(timeout_in, n_conns), _pn(route, n),
            _pn(cls, n), _ptr(bucket_first), _pn(order, n), _pn(infos_out, n), _pn(src_base_out, n),
            _pn(results, n_conns), _pn(timeout_out, n_conns), _ptr(fuc), self._stream(stream)),
            "ufc_route_frames_varlen")
        return {"route": route, "cls": cls, "bucket_first": bucket_first, "order": order, "infos_out": infos_out,
                "src_base_out": src_base_out, "results": results, "timeout_out": timeout_out,
                "first_unknown_control": fuc}

    # ---- host buffers (frames received into host memory) ----
    def seal_host_varlen(self, data: np.ndarray, offsets: np.ndarray):
        """Seal every frame of a host CSR batch in place (GPU CRC, host trailer write); returns the CRCs."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        crc = np.empty(max(n, 0), dtype=np.uint32)
        check(lib().ufc_seal_host_varlen(self._ctx, data.ctypes.data, offsets.ctypes.data, n, crc.ctypes.data),
              "ufc_seal_host_varlen")
        return crc

    def seal_host_slots(self, slots: np.ndarray, slot_stride: int, lens: np.ndarray):
        """Seal every datagram of a host slots batch in place (lens[i] >= 4 bytes at the start of slot i;
        GPU CRC, host trailer write); returns the CRCs."""
        if slots.dtype != np.uint8 or not slots.flags.c_contiguous or not slots.flags.writeable:
            raise ValueError("slots must be a writable contiguous uint8 array")
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = lens.size
        if n and slots.size < (n - 1) * slot_stride + int(lens[-1]):
            raise ValueError("slots must hold slot n - 1 and its datagram")
        crc = np.empty(n, dtype=np.uint32)
        check(lib().ufc_seal_host_slots(self._ctx, slots.ctypes.data, slot_stride, lens.ctypes.data, n,
                                        crc.ctypes.data), "ufc_seal_host_slots")
        return crc

    def validate_host_slots(self, slots: np.ndarray, slot_stride: int, lens: np.ndarray):
        """Datagrams received into fixed-size slots (recvmmsg layout) -> (crc uint32[n], valid uint8[n])."""
        slots = np.ascontiguousarray(slots, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = lens.size
        if n and slots.size < (n - 1) * slot_stride + int(lens[-1]):
            raise ValueError("slots must hold slot n - 1 and its datagram")
        crc = np.empty(n, dtype=np.uint32)
        valid = np.empty(n, dtype=np.uint8)
        check(lib().ufc_validate_host_slots(self._ctx, slots.ctypes.data, slot_stride, lens.ctypes.data, n,
                                            crc.ctypes.data, valid.ctypes.data), "ufc_validate_host_slots")
        return crc, valid

    def validate_host_slots_async(self, slots, slot_stride: int, lens, crc_out, valid_out, stream):
        """Queue the slots gate on `stream` (torch.cuda.Stream) and return at once: slots (uint8),
        lens (int32) and the outputs crc_out (int32[n]) / valid_out (uint8[n]) are host
        torch tensors, ideally pinned, that must stay alive and unmodified until the stream is done."""
        n = lens.numel() if isinstance(lens, torch.Tensor) else 0
        need = {"lens": (lens, torch.int32, n), "crc_out": (crc_out, torch.int32, n),
                "valid_out": (valid_out, torch.uint8, n), "slots": (slots, torch.uint8, 0)}
        for name, (t, dt, m) in need.items():
            if not isinstance(t, torch.Tensor) or t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous host tensor")
            if t.dtype != dt or t.numel() < m:
                raise ValueError(f"{name} must be {dt} with at least {m} elements")
        # The copy reads (n - 1) * slot_stride + lens[n - 1] bytes of slots (ufc_api.cpp).
        m = (n - 1) * slot_stride + int(lens[n - 1]) if n else 0
        if slots.numel() < m:
            raise ValueError(f"slots must hold at least {m} bytes (slot n - 1 and its datagram), got {slots.numel()}")
        check(lib().ufc_validate_host_slots_async(self._ctx, slots.data_ptr(), slot_stride, lens.data_ptr(), n,
                                                  crc_out.data_ptr(), valid_out.data_ptr(), stream.cuda_stream),
              "ufc_validate_host_slots_async")

    def validate_host_varlen(self, data: np.ndarray, offsets: np.ndarray):
        """numpy uint8 bytes + uint64/int64 offsets in host memory -> (crc uint32[n], valid uint8[n])."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        crc = np.empty(max(n, 0), dtype=np.uint32)
        valid = np.empty(max(n, 0), dtype=np.uint8)
        check(lib().ufc_validate_host_varlen(self._ctx, data.ctypes.data_as(ctypes.c_void_p),
                                             offsets.ctypes.data_as(ctypes.c_void_p), n,
                                             crc.ctypes.data_as(ctypes.c_void_p),
                                             valid.ctypes.data_as(ctypes.c_void_p)), "ufc_validate_host_varlen")
        return crc, valid
