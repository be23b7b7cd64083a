"""Batched, device-resident frame CRC on MI355X (the hot path).

`FrameCrcEngine` owns one libuflowcrc context per device and wraps the batched C-ABI entry
points on torch tensors (torch provides device memory and the current HIP stream only).
Per frame i:  crc[i] = compute(frame_i[:-4]),  valid[i] = len_i >= 5 and crc[i] == BE32(frame_i[-4:])
-- the CRC gate of Frame::read (src/frame/serial/mod.rs:675-690) -- and seal writes the trailer
(src/frame/serial/mod.rs:463-470, build.rs:151-159).

CRC words are returned as int32 tensors holding the uint32 bit patterns
(`crc.cpu().numpy().view(numpy.uint32)`).
"""
import ctypes

import numpy as np
import torch

from ._native import lib, check


# Items of a flush whose frame chain one wave of the pack resolves in LDS at a time (kPackTile, csrc/frame_pack.hpp).
PACK_TILE = 256
# Packets of a sender that one wave of the packet emit resolves at a time (kEmitTile, csrc/packet_emit.hpp).
EMIT_TILE = 64


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


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

    # ---- Frame::read past the gate, on the device (uflow_frame_codec.h) ----
    def parse_varlen(self, data, offsets, valid, items_cap=None, stream=None):
        """Batched Frame::read of a CSR batch after the CRC gate (`valid`, from crc_varlen).
        Returns (infos uint8[n, 32], items uint8[items_cap, 24], items_used int64[1]) device tensors;
        the byte rows are ufc_frame_info / ufc_item records (numpy views: uflow_amd.frame
        FRAME_INFO_DTYPE / ITEM_DTYPE).  items_cap defaults to a bound no batch can exceed."""
        n = offsets.numel() - 1
        self._check("offsets", offsets, (torch.int64,), 1)
        self._check("data", data, (torch.uint8,), 0)
        self._check("valid", valid, (torch.uint8,), n)
        if items_cap is None:  # a datagram takes >= 6 bytes, an ack group 9
            items_cap = max(1, data.numel() // 6)
        infos = torch.empty((max(n, 0), 32), dtype=torch.uint8, device=self.device)
        items = torch.empty((items_cap, 24), dtype=torch.uint8, device=self.device)
        used = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(lib().ufc_parse_batch_varlen(self._ctx, self._bytes_ptr(data), _ptr(offsets), n, _ptr(valid), _ptr(infos),
                                           _ptr(items), items_cap, _ptr(used), self._stream(stream)),
              "ufc_parse_batch_varlen")
        return infos, items, used

    # ---- Frame::write of a batch, on the device (uflow_frame_codec.h) ----
    def build_sizes_varlen(self, infos, items, payload_len, src_base=None, n_items=None, stream=None):
        """ufc_build_sizes_varlen: (out_offsets int64[n + 1], status uint8[n]) of the frames the records
        describe (infos uint8[n, 32], items uint8[*, 24]: what parse_varlen returns)."""
        n = infos.shape[0]
        n_items = items.shape[0] if n_items is None else int(n_items)
        self._check("infos", infos, (torch.uint8,), 32 * n)
        self._check("items", items, (torch.uint8,), 24 * n_items)
        self._check("src_base", src_base, (torch.int64,), n)
        # (no fill kernel on torch's current stream: the call writes all n + 1 offsets on `stream`)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device) if n else \
            torch.zeros(1, dtype=torch.int64, device=self.device)
        status = torch.empty(n, dtype=torch.uint8, device=self.device)
        check(lib().ufc_build_sizes_varlen(self._ctx, _ptr(infos), _ptr(items) if n_items else None, n_items,
                                           _ptr(src_base), int(payload_len), n, _ptr(offsets), _ptr(status),
                                           self._stream(stream)), "ufc_build_sizes_varlen")
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
        check(lib().ufc_build_batch_varlen(self._ctx, _ptr(infos), _ptr(items) if n_items else None, n_items,
                                           _ptr(src_base), _ptr(payload) if payload.numel() else None, payload.numel(),
                                           n, _ptr(offsets), _ptr(out) if out.numel() else None, out.numel(),
                                           1 if seal else 0, _ptr(crc_out), self._stream(stream)),
              "ufc_build_batch_varlen")
        return out, offsets, status

    # ---- the emitters' push / finalize of many flushes, on the device (uflow_frame_codec.h) ----
    def pack_flushes(self, items, flush_first, flushes, frames_cap=None, nonce_bits=None, stream=None):
        """ufc_pack_varlen: cut every flush's items into frames as DataFrameEmitter / AckFrameEmitter do
        (src/half_connection/emit.rs:47-125, 170-211).  items uint8[n_items, 24] (ufc_item records, what
        parse_varlen returns), flush_first int64[n_flushes + 1] (CSR over the items), flushes uint8[n_flushes, 24]
        (ufc_flush records, uflow_amd.frame.FLUSH_DTYPE), nonce_bits int32 words (bit g: the nonce of the batch's
        g-th frame; default 0).  Returns (infos uint8[frames_cap, 32], results uint8[n_flushes, 24], frames_used
        int64[1]) device tensors; frames_cap defaults to n_items, which is always enough.  infos is one that
        build_varlen takes as is: the rows from frames_used on are zero, which the build skips (or pass
        infos[:frames_used])."""
        n_items = items.shape[0]
        n = flushes.shape[0]
        if frames_cap is None:
            frames_cap = n_items
        frames_cap = int(frames_cap)
        self._check("items", items, (torch.uint8,), 24 * n_items)
        self._check("flush_first", flush_first, (torch.int64,), n + 1)
        self._check("flushes", flushes, (torch.uint8,), 24 * n)
        self._check("nonce_bits", nonce_bits, (torch.int32, torch.uint32), (frames_cap + 31) // 32)
        # (the outputs are zeroed on the stream the pack is queued on)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            infos = torch.zeros((frames_cap, 32), dtype=torch.uint8, device=self.device)
            results = torch.zeros((n, 24), dtype=torch.uint8, device=self.device)
            used = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(lib().ufc_pack_varlen(self._ctx, _ptr(items) if n_items else None, n_items, _ptr(flush_first),
                                    _ptr(flushes) if n else None, n, _ptr(nonce_bits),
                                    _ptr(infos) if frames_cap else None, frames_cap, _ptr(results) if n else None,
                                    _ptr(used), self._stream(stream)), "ufc_pack_varlen")
        return infos, results, used

    # ---- PacketSender::emit_packet and fragmentation of many senders, on the device (uflow_frame_codec.h) ----
    def emit_packets(self, packets, packet_first, senders, items_cap, items=None, senders_out=None,
                     want_packet_results=True, stream=None):
        """ufc_emit_packets_varlen: turn every sender's queued packets into datagram items as
        PacketSender::emit_packet and PendingPacket do (src/half_connection/packet_sender.rs:149-238,
        pending_packet.rs:23-42, 84-103).  packets uint8[n_packets, 16] (ufc_packet records,
        uflow_amd.frame.PACKET_DTYPE), packet_first int64[n_senders + 1] (CSR over the packets), senders
        uint8[n_senders, 304] (ufc_sender records, SENDER_DTYPE).  Returns (items uint8[items_cap, 24], flush_first
        int64[n_senders + 1], packet_results uint8[n_packets, 16] or None, sender_results uint8[n_senders, 32],
        senders_out uint8[n_senders, 304], items_used int64[1]) device tensors: items and flush_first are what
        pack_flushes takes (items[:items_used] when items_cap is larger).  Items at an index >= items_cap are not
        written (compare items_used); each sender's reserve_items slots stay as they were (zero in a tensor
        allocated here).  `items`: a tensor to write into; senders_out: where the state after the consumed
        packets goes (may be `senders`)."""
        n_packets = packets.shape[0]
        n = senders.shape[0]
        items_cap = int(items_cap)
        self._check("packets", packets, (torch.uint8,), 16 * n_packets)
        self._check("packet_first", packet_first, (torch.int64,), n + 1)
        self._check("senders", senders, (torch.uint8,), 304 * n)
        self._check("items", items, (torch.uint8,), 24 * items_cap)
        self._check("senders_out", senders_out, (torch.uint8,), 304 * n)
        # (the outputs are zeroed on the stream the emit is queued on)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if items is None:
                items = torch.zeros((items_cap, 24), dtype=torch.uint8, device=self.device)
            flush_first = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            packet_results = torch.zeros((n_packets, 16), dtype=torch.uint8, device=self.device) \
                if want_packet_results else None
            sender_results = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
            if senders_out is None:
                senders_out = torch.zeros((n, 304), dtype=torch.uint8, device=self.device)
            used = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(lib().ufc_emit_packets_varlen(self._ctx, _ptr(packets) if n_packets else None, n_packets,
                                            _ptr(packet_first), _ptr(senders) if n else None, n,
                                            _ptr(items) if items_cap else None, items_cap, _ptr(flush_first),
                                            _ptr(packet_results) if want_packet_results and n_packets else None,
                                            _ptr(sender_results) if n else None, _ptr(senders_out) if n else None,
                                            _ptr(used), self._stream(stream)), "ufc_emit_packets_varlen")
        return items, flush_first, packet_results, sender_results, senders_out, used

    # ---- PacketReceiver's step for many receivers, on the device (uflow_frame_codec.h) ----
    def receive_packets(self, infos, items, payload, frame_first, receivers, slots, slot_first, carry_in,
                        src_base=None, frame_accept=None, carry_cap=None, out_cap=None, packets_cap=None,
                        carry_out=None, out_bytes=None, packets=None, receivers_out=None, want_item_status=True,
                        stream=None):
        """ufc_receive_packets_varlen: one step of PacketReceiver (handle_datagram, receive, resynchronize;
        src/half_connection/packet_receiver/mod.rs:142-435) for every receiver.  infos uint8[n_frames, 32] and
        items uint8[n_items, 24] (what parse_varlen returns), payload uint8 (the frames' bytes) with src_base
        int64[n_frames] (the parse's offsets; None: zero), frame_first int64[n_receivers + 1] (CSR over the frames),
        receivers uint8[n_receivers, 560] (ufc_receiver records, uflow_amd.frame.RECEIVER_DTYPE), slots
        uint8[n_slots, 32] (ufc_rx_slot, updated in place), slot_first int64[n_receivers + 1], carry_in uint8 (the
        carry arena the slots point into), frame_accept uint8[n_frames] or None.  Returns a dict of device tensors:
        packets uint8[packets_cap, 24], packet_first int64[n + 1], packets_used, out_bytes, out_used, carry_out,
        carry_first int64[n + 1], carry_used, item_status uint8[n_items] or None, results uint8[n, 80],
        receivers_out uint8[n, 560] (may be given as `receivers`).  Caps that are not given are what the step needs,
        found by a first pass on a copy of the state with caps of zero, whose counts are read back (this waits for
        the stream; give the caps or the tensors to stay asynchronous: an ACTIVE slot holds its whole fragment
        buffer, so the carry has no small bound from the batch's sizes alone, see the header); tensors given for
        carry_out, out_bytes and packets are written into.
        Pass carry_out[:carry_used] as the next step's carry_in (carry_out must not overlap carry_in)."""
        n_frames, n_items, n, n_slots = infos.shape[0], items.shape[0], receivers.shape[0], slots.shape[0]
        self._check("infos", infos, (torch.uint8,), 32 * n_frames)
        self._check("items", items, (torch.uint8,), 24 * n_items)
        self._check("payload", payload, (torch.uint8,), 0)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._check("receivers", receivers, (torch.uint8,), 560 * n)
        self._check("slots", slots, (torch.uint8,), 32 * n_slots)
        self._check("slot_first", slot_first, (torch.int64,), n + 1)
        self._check("carry_in", carry_in, (torch.uint8,), 0)
        self._check("src_base", src_base, (torch.int64,), n_frames)
        self._check("frame_accept", frame_accept, (torch.uint8,), n_frames)
        self._check("receivers_out", receivers_out, (torch.uint8,), 560 * n)
        for name, t in (("carry_out", carry_out), ("out_bytes", out_bytes), ("packets", packets)):
            self._check(name, t, (torch.uint8,), 0)
        def p(t):
            return _ptr(t) if t is not None and t.numel() else None

        def size(t, width=1):
            return 0 if t is None else t.numel() // width

        def call(slots_, carry_out_, out_bytes_, packets_, status_, receivers_out_):
            check(lib().ufc_receive_packets_varlen(
                self._ctx, p(infos), n_frames, p(frame_accept), p(items), n_items, p(src_base), p(payload),
                payload.numel(), _ptr(frame_first), p(receivers), n, p(slots_), _ptr(slot_first), n_slots, p(carry_in),
                carry_in.numel(), p(carry_out_), size(carry_out_), _ptr(carry_first),
                ctypes.c_void_p(used.data_ptr() + 16), p(packets_), size(packets_, 24), _ptr(packet_first),
                ctypes.c_void_p(used.data_ptr()), p(out_bytes_), size(out_bytes_), ctypes.c_void_p(used.data_ptr() + 8),
                p(status_), p(results), p(receivers_out_), self._stream(stream)), "ufc_receive_packets_varlen")

        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            def zeros(*shape, dtype=torch.uint8):
                return torch.zeros(shape, dtype=dtype, device=self.device)
            carry_first = zeros(n + 1, dtype=torch.int64)
            packet_first = zeros(n + 1, dtype=torch.int64)
            used = zeros(3, dtype=torch.int64)
            results = zeros(n, 80)
            need = [(carry_out, carry_cap), (out_bytes, out_cap), (packets, packets_cap)]
            if n and any(t is None and cap is None for t, cap in need):
                # The used counts are exact whatever the caps: a first pass on a copy of the state, with none.
                # Reading them back waits for the stream: give the caps (or the tensors) to stay asynchronous.
                call(slots.clone(), None, None, None, None, zeros(n, 560))
                u = used.cpu().tolist()
                packets_cap = u[0] if packets_cap is None else packets_cap
                out_cap = u[1] if out_cap is None else out_cap
                carry_cap = u[2] if carry_cap is None else carry_cap
            if carry_out is None:
                carry_out = zeros(int(carry_cap or 0))
            if out_bytes is None:
                out_bytes = zeros(int(out_cap or 0))
            if packets is None:
                packets = zeros(int(packets_cap or 0), 24)
            if receivers_out is None:
                receivers_out = zeros(n, 560)
            item_status = zeros(n_items) if want_item_status else None
        call(slots, carry_out, out_bytes, packets, item_status, receivers_out)
        return {"packets": packets, "packet_first": packet_first, "packets_used": used[0:1], "out_bytes": out_bytes,
                "out_used": used[1:2], "carry_out": carry_out, "carry_first": carry_first, "carry_used": used[2:3],
                "item_status": item_status, "results": results, "receivers_out": receivers_out}

    # ---- FrameAckQueue's step for many connections, on the device (uflow_frame_codec.h) ----
    def frame_window(self, infos, frame_first, windows, groups_cap=None, frame_accept=None, groups=None,
                     windows_out=None, stream=None):
        """ufc_frame_window_varlen: one step of FrameAckQueue (window_contains, mark_seen, resynchronize;
        src/half_connection/frame_ack_queue.rs as half_connection/mod.rs:132-152 drives it) for every connection.
        infos uint8[n_frames, 32] (what parse_varlen returns), frame_first int64[n + 1] (CSR over the frames, the one
        receive_packets takes), windows uint8[n, 24] (ufc_frame_window records, uflow_amd.frame.FRAME_WINDOW_DTYPE).
        Returns a dict of device tensors: frame_accept uint8[n_frames] (1 for the data frames inside the window:
        pass it to receive_packets), groups uint8[groups_cap, 24] (ack groups as ufc_item records, each
        connection's carried tail first), group_first int64[n + 1] (CSR over the groups: pack_flushes' flush_first),
        groups_used int64[1], results uint8[n, 40], windows_out uint8[n, 24] (may be given as `windows`).  groups_cap
        defaults to n + n_frames, which is always enough; groups at an index >= groups_cap are not written (compare
        groups_used).  Tensors given for frame_accept, groups and windows_out are written into."""
        n_frames, n = infos.shape[0], windows.shape[0]
        if groups_cap is None:
            groups_cap = groups.shape[0] if groups is not None else n + n_frames
        groups_cap = int(groups_cap)
        self._check("infos", infos, (torch.uint8,), 32 * n_frames)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._check("windows", windows, (torch.uint8,), 24 * n)
        self._check("frame_accept", frame_accept, (torch.uint8,), n_frames)
        self._check("groups", groups, (torch.uint8,), 24 * groups_cap)
        self._check("windows_out", windows_out, (torch.uint8,), 24 * n)
        # (the outputs are zeroed on the stream the call is queued on)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if frame_accept is None:
                frame_accept = torch.zeros(n_frames, dtype=torch.uint8, device=self.device)
            # (the pointer is required even when there are no frames, and an empty tensor has none)
            accept_arg = frame_accept if n_frames else torch.zeros(1, dtype=torch.uint8, device=self.device)
            if groups is None:
                groups = torch.zeros((groups_cap, 24), dtype=torch.uint8, device=self.device)
            if windows_out is None:
                windows_out = torch.zeros((n, 24), dtype=torch.uint8, device=self.device)
            group_first = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            results = torch.zeros((n, 40), dtype=torch.uint8, device=self.device)
            used = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(lib().ufc_frame_window_varlen(self._ctx, _ptr(infos) if n_frames else None, n_frames, _ptr(frame_first),
                                            _ptr(windows) if n else None, n,
                                            _ptr(accept_arg) if n else None,
                                            _ptr(groups) if groups_cap else None, groups_cap, _ptr(group_first),
                                            _ptr(used), _ptr(results) if n else None,
                                            _ptr(windows_out) if n else None, self._stream(stream)),
              "ufc_frame_window_varlen")
        return {"frame_accept": frame_accept, "groups": groups, "group_first": group_first, "groups_used": used,
                "results": results, "windows_out": windows_out}

    # ---- the sender's FrameQueue step for many connections, on the device (uflow_frame_codec.h) ----
    def frame_queue(self, infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked=None,
                    queues_out=None, stream=None):
        """ufc_frame_queue_varlen: one step of the sender's FrameQueue (push, acknowledge_group,
        advance_transfer_window, forget_frames, get_feedback; src/half_connection/frame_queue.rs with
        reorder_buffer.rs and loss_rate.rs) for every connection.  infos uint8[n_frames, 32] and items uint8[n_items,
        24] (what parse_varlen returns), frame_first int64[n + 1] (CSR over the frames), sent uint8[n_sent, 24]
        (ufc_sent_frame records to push) with sent_first int64[n + 1], queues uint8[n, 192], steps uint8[n, 40], log
        uint8[n_log, 24] (the log arena, updated in place), ref_acked uint8[refs_cap] or None (set to 1 for the
        fragments of newly acked frames, in place).  Returns a dict of device tensors: results uint8[n, 80],
        queues_out uint8[n, 192] (may be given as `queues`), log, ref_acked.  The record layouts are
        uflow_amd.frame's FRAME_QUEUE_DTYPE, FRAME_QUEUE_STEP_DTYPE, SENT_FRAME_DTYPE and FRAME_QUEUE_RESULT_DTYPE."""
        n_frames, n_items, n_sent, n, n_log = infos.shape[0], items.shape[0], sent.shape[0], queues.shape[0], log.shape[0]
        refs_cap = ref_acked.shape[0] if ref_acked is not None else 0
        self._check("infos", infos, (torch.uint8,), 32 * n_frames)
        self._check("items", items, (torch.uint8,), 24 * n_items)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._check("sent", sent, (torch.uint8,), 24 * n_sent)
        self._check("sent_first", sent_first, (torch.int64,), n + 1)
        self._check("queues", queues, (torch.uint8,), 192 * n)
        self._check("steps", steps, (torch.uint8,), 40 * n)
        self._check("log", log, (torch.uint8,), 24 * n_log)
        self._check("ref_acked", ref_acked, (torch.uint8,), refs_cap)
        self._check("queues_out", queues_out, (torch.uint8,), 192 * n)
        # (the outputs are zeroed on the stream the call is queued on)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if queues_out is None:
                queues_out = torch.zeros((n, 192), dtype=torch.uint8, device=self.device)
            results = torch.zeros((n, 80), dtype=torch.uint8, device=self.device)
        check(lib().ufc_frame_queue_varlen(self._ctx, _ptr(infos) if n_frames else None, n_frames,
                                           _ptr(items) if n_items else None, n_items, _ptr(frame_first),
                                           _ptr(sent) if n_sent else None, n_sent, _ptr(sent_first),
                                           _ptr(queues) if n else None, _ptr(steps) if n else None, n,
                                           _ptr(log) if n_log else None, n_log,
                                           _ptr(ref_acked) if refs_cap else None, refs_cap,
                                           _ptr(results) if n else None, _ptr(queues_out) if n else None,
                                           self._stream(stream)), "ufc_frame_queue_varlen")
        return {"results": results, "queues_out": queues_out, "log": log, "ref_acked": ref_acked}

    # ---- the send rate control around the frame queue call, on the device (uflow_frame_codec.h) ----
    def rate_begin(self, states, now_ms, extra_flags=None, steps=None, states_out=None, stream=None):
        """ufc_rate_begin_varlen: opens a tick.  states uint8[n, 112] (RATE_STATE_DTYPE records), now_ms int64[n],
        extra_flags int32[n] or None (OR-ed into the steps' flags: FQ_MARK_RATE_LIMITED).  Returns a dict of device
        tensors: steps uint8[n, 40] (what frame_queue takes), states_out uint8[n, 112] (may be given as `states`)."""
        n = states.shape[0]
        self._check("states", states, (torch.uint8,), 112 * n)
        self._check("now_ms", now_ms, (torch.int64, torch.uint64), n)
        self._check("extra_flags", extra_flags, (torch.int32, torch.uint32), n)
        self._check("steps", steps, (torch.uint8,), 40 * n)
        self._check("states_out", states_out, (torch.uint8,), 112 * n)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if steps is None:
                steps = torch.zeros((n, 40), dtype=torch.uint8, device=self.device)
            if states_out is None:
                states_out = torch.zeros((n, 112), dtype=torch.uint8, device=self.device)
        check(lib().ufc_rate_begin_varlen(self._ctx, _ptr(states) if n else None, _ptr(now_ms) if n else None,
                                          _ptr(extra_flags) if n else None, n, _ptr(steps) if n else None,
                                          _ptr(states_out) if n else None, self._stream(stream)),
              "ufc_rate_begin_varlen")
        return {"steps": steps, "states_out": states_out}

    def rate_step(self, states, ticks, fq_results, entries, flush_results=None, result_index=None, flushes=None,
                  flush_index=None, results=None, states_out=None, stream=None):
        """ufc_rate_step_varlen: closes a tick behind frame_queue (notify_frame_sent, fill_flush_alloc and
        SendRateComp::step; src/half_connection/send_rate.rs, recv_rate_set.rs, mod.rs:165-215) for every connection.
        states uint8[n, 112], ticks uint8[n, 32], fq_results uint8[n, 80] (frame_queue's results), entries
        uint8[n_entries, 16] (the receive-rate sets, updated in place); flush_results uint8[m, 24] with result_index
        int32[n] (the last data flush of each connection, -1 for none) and flushes uint8[k, 24] with flush_index
        int32[n] (where the new flush_alloc goes, in place) are optional.  Returns a dict of device tensors: results
        uint8[n, 56], states_out uint8[n, 112] (may be given as `states`), entries, flushes.  The record layouts are
        uflow_amd.frame's RATE_STATE_DTYPE, RATE_TICK_DTYPE, RATE_RESULT_DTYPE and RECV_RATE_ENTRY_DTYPE."""
        n, n_entries = states.shape[0], entries.shape[0]
        n_fr = flush_results.shape[0] if flush_results is not None else 0
        n_fl = flushes.shape[0] if flushes is not None else 0
        if (n_fr and result_index is None) or (n_fl and flush_index is None):
            raise ValueError("flush_results needs result_index, flushes needs flush_index")
        self._check("states", states, (torch.uint8,), 112 * n)
        self._check("ticks", ticks, (torch.uint8,), 32 * n)
        self._check("fq_results", fq_results, (torch.uint8,), 80 * n)
        self._check("entries", entries, (torch.uint8,), 16 * n_entries)
        self._check("flush_results", flush_results, (torch.uint8,), 24 * n_fr)
        self._check("result_index", result_index, (torch.int32, torch.uint32), n)
        self._check("flushes", flushes, (torch.uint8,), 24 * n_fl)
        self._check("flush_index", flush_index, (torch.int32, torch.uint32), n)
        self._check("results", results, (torch.uint8,), 56 * n)
        self._check("states_out", states_out, (torch.uint8,), 112 * n)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if results is None:
                results = torch.zeros((n, 56), dtype=torch.uint8, device=self.device)
            if states_out is None:
                states_out = torch.zeros((n, 112), dtype=torch.uint8, device=self.device)
        check(lib().ufc_rate_step_varlen(self._ctx, _ptr(states) if n else None, _ptr(ticks) if n else None,
                                         _ptr(fq_results) if n else None, n, _ptr(entries) if n_entries else None,
                                         n_entries, _ptr(flush_results) if n_fr else None, n_fr,
                                         _ptr(result_index) if n_fr else None, _ptr(flushes) if n_fl else None, n_fl,
                                         _ptr(flush_index) if n_fl else None, _ptr(results) if n else None,
                                         _ptr(states_out) if n else None, self._stream(stream)),
              "ufc_rate_step_varlen")
        return {"results": results, "states_out": states_out, "entries": entries, "flushes": flushes}

    # ---- the resend calls around the emit and the pack, on the device (uflow_frame_codec.h) ----
    _RS_ARENA_WIDTH = (("heap", 16), ("pkts", 24), ("frag_acked", 1), ("tx", 8), ("ref_acked", 1), ("stage", 24))

    def _rs_arenas(self, arenas):
        """(pointer, record count) of every resend arena, uint8 device tensors, in the C calls' order."""
        out = {}
        for name, width in self._RS_ARENA_WIDTH:
            t = arenas.get(name)
            self._check(name, t, (torch.uint8,), 0)
            count = 0 if t is None else t.numel() // width
            out[name] = (_ptr(t) if count else None, count)
        return out

    def resend_begin(self, infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags=None,
                     results=None, states_out=None, senders_out=None, stream=None):
        """ufc_resend_begin_varlen: behind rate_step, in front of emit_packets.  Ack propagation from ref_acked,
        PacketSender::acknowledge for the ack frames, the resend loop (the heap and the pack's rule) and the pending
        fragments' staging for every connection.  infos uint8[n_frames, 32], frame_first int64[n + 1], queues
        uint8[n, 192] and log uint8[n_log, 24] as frame_queue left them, rate uint8[n, 56] (rate_step's results),
        flushes uint8[n, 24] (the data flushes the pack gets), states uint8[n, 104], senders uint8[n, 304], arenas a
        dict of uint8 tensors heap [., 16], pkts [., 24], frag_acked, tx [., 8], ref_acked, stage [., 24] (updated in
        place), flags int32[n] or None.  Returns a dict: results uint8[n, 48], states_out, senders_out (may be given
        as `states`, `senders`).  Layouts: uflow_amd.frame's RESEND_DTYPE and RESEND_RESULT_DTYPE."""
        n_frames, n, n_log = infos.shape[0], states.shape[0], log.shape[0]
        self._check("infos", infos, (torch.uint8,), 32 * n_frames)
        self._check("frame_first", frame_first, (torch.int64,), n + 1)
        self._check("queues", queues, (torch.uint8,), 192 * n)
        self._check("log", log, (torch.uint8,), 24 * n_log)
        self._check("rate", rate, (torch.uint8,), 56 * n)
        self._check("flushes", flushes, (torch.uint8,), 24 * n)
        self._check("states", states, (torch.uint8,), 104 * n)
        self._check("senders", senders, (torch.uint8,), 304 * n)
        self._check("flags", flags, (torch.int32, torch.uint32), n)
        self._check("results", results, (torch.uint8,), 48 * n)
        self._check("states_out", states_out, (torch.uint8,), 104 * n)
        self._check("senders_out", senders_out, (torch.uint8,), 304 * n)
        A = self._rs_arenas(arenas)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if results is None:
                results = torch.zeros((n, 48), dtype=torch.uint8, device=self.device)
            if states_out is None:
                states_out = torch.zeros((n, 104), dtype=torch.uint8, device=self.device)
            if senders_out is None:
                senders_out = torch.zeros((n, 304), dtype=torch.uint8, device=self.device)
        check(lib().ufc_resend_begin_varlen(
            self._ctx, _ptr(infos) if n_frames else None, n_frames, _ptr(frame_first), _ptr(queues) if n else None,
            _ptr(log) if n_log else None, n_log, _ptr(rate) if n else None, _ptr(flags) if n else None,
            _ptr(flushes) if n else None, _ptr(states) if n else None, _ptr(senders) if n else None, n, *A["heap"],
            *A["pkts"], *A["frag_acked"], *A["tx"], *A["ref_acked"], *A["stage"], _ptr(results) if n else None,
            _ptr(states_out) if n else None, _ptr(senders_out) if n else None, self._stream(stream)),
            "ufc_resend_begin_varlen")
        return {"results": results, "states_out": states_out, "senders_out": senders_out}

    def resend_place(self, states, begin_results, arenas, flush_first, items, stream=None):
        """ufc_resend_place_varlen: behind emit_packets.  Every connection's staged items into items[flush_first[c]
        ..], the slots the emit reserved; items uint8[items_cap, 24] is written in place and returned."""
        n = states.shape[0]
        self._check("states", states, (torch.uint8,), 104 * n)
        self._check("begin_results", begin_results, (torch.uint8,), 48 * n)
        self._check("flush_first", flush_first, (torch.int64,), n + 1)
        self._check("items", items, (torch.uint8,), 0)
        A = self._rs_arenas(arenas)
        items_cap = items.numel() // 24
        check(lib().ufc_resend_place_varlen(self._ctx, _ptr(states) if n else None, _ptr(begin_results) if n else None,
                                            n, *A["stage"], _ptr(flush_first), _ptr(items) if items_cap else None,
                                            items_cap, self._stream(stream)), "ufc_resend_place_varlen")
        return items

    def resend_commit(self, flush_results, infos, out_offsets, frames_used, items, flush_first, packets, packet_first,
                      packet_results, sender_results, begin_results, rate, states, senders, arenas, sent=None,
                      next_extra_flags=None, results=None, states_out=None, retake=None, stream=None):
        """ufc_resend_commit_varlen: behind pack_flushes over the data flushes (flush c = connection c) and
        build_sizes.  flush_results uint8[n, 24], infos uint8[n_infos, 32] (the pack's frames), out_offsets
        int64[n_infos + 1] (the size pass), frames_used int64[1] (the pack's), items uint8[n_items, 24], flush_first
        int64[n + 1], packets uint8[n_packets, 16], packet_first int64[n + 1], packet_results uint8[n_packets, 16] and
        sender_results uint8[n, 32] (the first emit's), begin_results uint8[n, 48], rate uint8[n, 56], states
        uint8[n, 104], senders uint8[n, 304] (as resend_begin wrote them), arenas as in resend_begin (updated in
        place), next_extra_flags int32[n] or None (in place).  Returns a dict: results uint8[n, 40], states_out, retake
        (the second emit's senders), sent uint8[n_infos, 24], sent_first int64[n + 1], next_extra_flags."""
        n, n_infos, n_items, n_packets = states.shape[0], infos.shape[0], items.shape[0], packets.shape[0]
        self._check("flush_results", flush_results, (torch.uint8,), 24 * n)
        self._check("infos", infos, (torch.uint8,), 32 * n_infos)
        self._check("out_offsets", out_offsets, (torch.int64,), n_infos + 1)
        self._check("frames_used", frames_used, (torch.int64,), 1)
        self._check("items", items, (torch.uint8,), 24 * n_items)
        self._check("flush_first", flush_first, (torch.int64,), n + 1)
        self._check("packets", packets, (torch.uint8,), 16 * n_packets)
        self._check("packet_first", packet_first, (torch.int64,), n + 1)
        self._check("packet_results", packet_results, (torch.uint8,), 16 * n_packets)
        self._check("sender_results", sender_results, (torch.uint8,), 32 * n)
        self._check("begin_results", begin_results, (torch.uint8,), 48 * n)
        self._check("rate", rate, (torch.uint8,), 56 * n)
        self._check("states", states, (torch.uint8,), 104 * n)
        self._check("senders", senders, (torch.uint8,), 304 * n)
        self._check("sent", sent, (torch.uint8,), 0)
        self._check("next_extra_flags", next_extra_flags, (torch.int32, torch.uint32), n)
        self._check("results", results, (torch.uint8,), 40 * n)
        self._check("states_out", states_out, (torch.uint8,), 104 * n)
        self._check("retake", retake, (torch.uint8,), 304 * n)
        A = self._rs_arenas(arenas)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            if sent is None:
                sent = torch.zeros((n_infos, 24), dtype=torch.uint8, device=self.device)
            if results is None:
                results = torch.zeros((n, 40), dtype=torch.uint8, device=self.device)
            if states_out is None:
                states_out = torch.zeros((n, 104), dtype=torch.uint8, device=self.device)
            if retake is None:
                retake = torch.zeros((n, 304), dtype=torch.uint8, device=self.device)
            sent_first = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        sent_cap = sent.numel() // 24
        check(lib().ufc_resend_commit_varlen(
            self._ctx, _ptr(flush_results) if n else None, _ptr(infos) if n_infos else None, n_infos, _ptr(out_offsets),
            _ptr(frames_used), _ptr(items) if n_items else None, n_items, _ptr(flush_first),
            _ptr(packets) if n_packets else None, n_packets, _ptr(packet_first),
            _ptr(packet_results) if n_packets else None, _ptr(sender_results) if n else None,
            _ptr(begin_results) if n else None, _ptr(rate) if n else None, _ptr(states) if n else None,
            _ptr(senders) if n else None, n, *A["heap"], *A["pkts"], *A["frag_acked"], *A["tx"],
            _ptr(sent) if sent_cap else None, sent_cap, _ptr(sent_first),
            _ptr(next_extra_flags) if next_extra_flags is not None and n else None, _ptr(results) if n else None,
            _ptr(states_out) if n else None, _ptr(retake) if n else None, self._stream(stream)),
            "ufc_resend_commit_varlen")
        return {"results": results, "states_out": states_out, "retake": retake, "sent": sent, "sent_first": sent_first,
                "next_extra_flags": next_extra_flags}

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
