"""A plain Python restatement of uflow's receive side, class for class and in release-build semantics
(debug asserts are not enforced): FragmentBuffer (src/half_connection/packet_receiver/assembly_window/
fragment_buffer.rs:12-57), AssemblyWindow (assembly_window/mod.rs:53-199) and PacketReceiver
(packet_receiver/mod.rs:12-31, 94-435).  One difference, as include/uflow_frame_codec.h states it: a packet refused
by the allocation limit (a dud) is delivered as a packet without bytes where the reference's unwrap panics.

Around it: converters between the classes and the records of ufc_receive_packets_* (header, slots, carry arena),
the expected outputs of one batched step, batch generators, and check(), which compares every record, status,
state field, slot field and delivered byte of a native call with the restatement; and, for calls too large for
that, check_receivers (check() on a sample of the receivers), check_sums and check_same (two native forms of one
call) over batches built in numpy.  Nothing here calls the library.
"""
import numpy as np

from uflow_amd import frame as fr

MASK = 0xFFFFF
FRAG = 1448
CHANNELS = 64
NONE = 0xFFFFFFFF
TILE = 64  # ids that the device form of receive() takes at a time (rx_receive_tiles)

# The launch constants of csrc/packet_receive.hip and csrc/packet_emit.hip that the big-shape tests are sized by,
# mirrored here: tests/test_receive_cpu.py::test_launch_constants_mirror_the_source reads them from the source.
LAUNCH_CONSTANTS = {"kRxFew": 32768, "kRxThreads": 64, "kRxThreadsFew": 8, "kCopyThreads": 256, "kCopyBlocksMax": 16384,
                    "kItemLanes": 16, "kRxChunk": 2048, "kEmitThreads": 256, "kItemBlocksMax": 16384}
RX_FEW, RX_CHUNK = LAUNCH_CONSTANTS["kRxFew"], LAUNCH_CONSTANTS["kRxChunk"]
COPY_WAVES_MAX = LAUNCH_CONSTANTS["kCopyBlocksMax"] * LAUNCH_CONSTANTS["kCopyThreads"] // 64              # 65 536 chunks
COPY_ITEMS_MAX = LAUNCH_CONSTANTS["kCopyBlocksMax"] * LAUNCH_CONSTANTS["kCopyThreads"] // LAUNCH_CONSTANTS["kItemLanes"]
VERDICT_GROUPS_MAX = 1 << 20   # (a literal in receive_batch's verdict launch)
EMIT_SLOTS_MAX = LAUNCH_CONSTANTS["kItemBlocksMax"] * LAUNCH_CONSTANTS["kEmitThreads"]                     # 4 194 304


def sub(a, b):
    return (a - b) & MASK


def add(a, b):
    return (a + b) & MASK


class Datagram:
    def __init__(self, sequence_id, channel_id, window_parent_lead, channel_parent_lead, fragment_id, fragment_id_last,
                 data):
        self.sequence_id = sequence_id
        self.channel_id = channel_id
        self.window_parent_lead = window_parent_lead
        self.channel_parent_lead = channel_parent_lead
        self.fragment_id = fragment_id
        self.fragment_id_last = fragment_id_last
        self.data = bytes(data)


def datagram_is_valid(dg):  # mod.rs:12-31
    if dg.channel_id >= CHANNELS:
        return False
    if dg.channel_parent_lead != 0:
        if dg.window_parent_lead == 0 or dg.channel_parent_lead < dg.window_parent_lead:
            return False
    if dg.fragment_id > dg.fragment_id_last:
        return False
    if dg.fragment_id < dg.fragment_id_last and len(dg.data) != FRAG:
        return False
    if len(dg.data) > FRAG:
        return False
    return True


class FragmentBuffer:  # fragment_buffer.rs
    def __init__(self, num_fragments):
        self.buffer = bytearray(num_fragments * FRAG)
        self.fragment_bitfields = [0] * ((num_fragments + 63) // 64)
        self.num_fragments = num_fragments
        self.fragments_remaining = num_fragments
        self.total_size = 0

    def write(self, idx, data):
        """True when the fragment was new (the reference returns nothing)."""
        bit = 1 << (idx % 64)
        if self.fragment_bitfields[idx // 64] & bit:
            return False
        self.fragment_bitfields[idx // 64] |= bit
        self.buffer[idx * FRAG: idx * FRAG + len(data)] = data
        self.fragments_remaining -= 1
        self.total_size += len(data)
        return True

    def finalize(self):
        return bytes(self.buffer[:self.total_size])

    def is_finished(self):
        return self.fragments_remaining == 0


class ActiveEntry:
    def __init__(self, alloc_size, channel_id, window_parent_lead, channel_parent_lead, last_fragment_id, num_fragments):
        self.alloc_size = alloc_size
        self.channel_id = channel_id
        self.window_parent_lead = window_parent_lead
        self.channel_parent_lead = channel_parent_lead
        self.last_fragment_id = last_fragment_id
        self.asm_buffer = FragmentBuffer(num_fragments)


class Closed:
    def __init__(self, alloc_size):
        self.alloc_size = alloc_size


class Packet:
    def __init__(self, dg, data):
        self.channel_id = dg.channel_id
        self.sequence_id = dg.sequence_id
        self.window_parent_lead = dg.window_parent_lead
        self.channel_parent_lead = dg.channel_parent_lead
        self.data = data  # None: a dud


def packet_alloc_size(dg):  # assembly_window/mod.rs:53-60
    n = dg.fragment_id_last + 1
    return n * FRAG if n > 1 else len(dg.data)


class AssemblyWindow:
    def __init__(self, max_alloc, size=4096):
        self.window = [None] * size  # None: Open
        self.alloc = 0
        self.max_alloc = min((max_alloc + FRAG - 1) // FRAG * FRAG, 2 ** 64 - 1)  # (saturating, as the records')

    def try_add(self, idx, dg):
        """(packet or None, status): the status is what ufc_receive_packets_* report for the datagram."""
        e = self.window[idx]
        if e is None:
            alloc_size = packet_alloc_size(dg)
            if self.alloc + alloc_size > self.max_alloc:
                self.window[idx] = Closed(0)
                return Packet(dg, None), fr.RX_DUD
            self.alloc += alloc_size
            if dg.fragment_id_last == 0:
                self.window[idx] = Closed(alloc_size)
                return Packet(dg, dg.data), fr.RX_COMPLETED
            n = dg.fragment_id_last + 1
            e = ActiveEntry(alloc_size, dg.channel_id, dg.window_parent_lead, dg.channel_parent_lead,
                            dg.fragment_id_last, n)
            e.asm_buffer.write(dg.fragment_id, dg.data)
            self.window[idx] = e
            return None, fr.RX_STORED
        if isinstance(e, Closed):
            return None, fr.RX_DROPPED_CLOSED
        if (dg.channel_id != e.channel_id or dg.window_parent_lead != e.window_parent_lead
                or dg.channel_parent_lead != e.channel_parent_lead or dg.fragment_id_last != e.last_fragment_id):
            return None, fr.RX_DROPPED_MISMATCH
        new = e.asm_buffer.write(dg.fragment_id, dg.data)
        if e.asm_buffer.is_finished():
            # (a duplicate cannot finish a buffer: is_finished was false after the write before it)
            self.window[idx] = Closed(e.alloc_size)
            return Packet(dg, e.asm_buffer.finalize()), fr.RX_COMPLETED
        return None, fr.RX_STORED if new else fr.RX_DROPPED_DUPLICATE

    def clear(self, idx):
        e = self.window[idx]
        if e is not None:
            self.alloc -= e.alloc_size
        self.window[idx] = None


class Channel:
    def __init__(self):
        self.base_id = None
        self.packet_count = 0


class PacketReceiver:
    def __init__(self, window_size, base_id, max_alloc):
        self.base_id = base_id
        self.end_id = base_id
        self.max_alloc_given = max_alloc
        self.assembly_window = AssemblyWindow(max_alloc, window_size)
        self.receive_window_size = window_size
        self.receive_window_mask = window_size - 1
        self.channel_entries = [(0, 0)] * window_size  # (channel_id, channel_parent_lead)
        self.window_entries = [0] * window_size        # window_parent_lead
        self.data_entries = [None] * window_size
        self.entry_flags = [False] * window_size
        self.data_flags = [False] * window_size
        self.dud_entries = [False] * window_size       # data_flags set with data None
        self.channels = [Channel() for _ in range(CHANNELS)]
        self.channel_base_markers = [None] * window_size
        self.channel_ready_flags = 0
        self.window_ready_flag = False
        self.advanced = 0   # ids the window moved (a step's driver resets it)
        self.tags = set()   # branches taken, for the generators' coverage condition
        self.receives = self.receives_over_one_tile = 0   # receive() calls, and those over more than TILE ids

    def handle_datagram(self, dg):
        base_id = self.base_id
        if not datagram_is_valid(dg) or dg.sequence_id > MASK:
            return fr.RX_DROPPED_INVALID
        channel = self.channels[dg.channel_id]
        channel_base_id = channel.base_id if channel.base_id is not None else base_id
        channel_lead = sub(channel_base_id, base_id)
        packet_lead = sub(dg.sequence_id, base_id)
        if packet_lead >= self.receive_window_size:
            return fr.RX_DROPPED_WINDOW
        if packet_lead < channel_lead:
            return fr.RX_DROPPED_CHANNEL
        idx = dg.sequence_id & self.receive_window_mask
        opener = self.assembly_window.window[idx] is None
        packet, status = self.assembly_window.try_add(idx, dg)
        if status == fr.RX_DUD:
            self.refused_in_step = True
        elif opener and getattr(self, "refused_in_step", False) and packet_alloc_size(dg) > 0:
            self.tags.add("alloc_refused_then_fits")
        if packet is not None:
            if self.data_flags[idx]:
                self.tags.add("stale_overwritten")
            self.channel_entries[idx] = (packet.channel_id, packet.channel_parent_lead)
            self.window_entries[idx] = packet.window_parent_lead
            self.data_entries[idx] = packet.data
            self.dud_entries[idx] = packet.data is None
            self.entry_flags[idx] = True
            self.data_flags[idx] = True
            if sub(dg.sequence_id, self.end_id) < self.receive_window_size:
                self.end_id = add(dg.sequence_id, 1)
            channel.packet_count += 1
            if packet.channel_parent_lead == 0 or packet.channel_parent_lead > sub(dg.sequence_id, channel_base_id):
                self.channel_ready_flags |= 1 << dg.channel_id
            if packet.window_parent_lead == 0 or packet.window_parent_lead > sub(dg.sequence_id, base_id):
                self.window_ready_flag = True
            if dg.fragment_id_last > 0 and packet.data is not None:
                self.tags.add("multi_completed")
            if packet.data is not None and len(packet.data) == 0:
                self.tags.add("empty_packet")
        return status

    def set_channel_base_id(self, channel_id, new_id):
        channel = self.channels[channel_id]
        if channel.base_id is not None:
            self.channel_base_markers[channel.base_id & self.receive_window_mask] = None
        self.channel_base_markers[new_id & self.receive_window_mask] = channel_id
        channel.base_id = new_id

    def try_unset_channel_base_id(self, sequence_id):
        idx = sequence_id & self.receive_window_mask
        channel_id = self.channel_base_markers[idx]
        self.channel_base_markers[idx] = None
        if channel_id is not None:
            self.channels[channel_id].base_id = None
            self.tags.add("channel_base_unset")

    def advance_window(self, new_base_id):
        new_base_delta = sub(new_base_id, self.base_id)
        if sub(self.end_id, self.base_id) < new_base_delta:
            self.end_id = new_base_id
        i = self.base_id
        while i != new_base_id:
            idx = i & self.receive_window_mask
            self.entry_flags[idx] = False
            if isinstance(self.assembly_window.window[idx], ActiveEntry):
                self.tags.add("active_cleared")
            if self.data_flags[idx]:
                self.tags.add("window_passed_undelivered")
            self.assembly_window.clear(idx)
            i = add(i, 1)
        i = self.base_id
        while i != new_base_id:
            i = add(i, 1)
            self.try_unset_channel_base_id(i)
        self.advanced += new_base_delta
        self.base_id = new_base_id

    def receive(self, sink):
        """sink(sequence_id, channel_id, data or None) per delivered packet."""
        base_id, end_id = self.base_id, self.end_id
        # (the tags on tiles: where the ids lie in runs of TILE from base_id, the device form's unit of work)
        n_ids = sub(end_id, base_id)
        self.receives += 1
        if n_ids > TILE:
            self.receives_over_one_tile += 1
            self.tags.add("ids_over_one_tile")
        if n_ids > 2 * TILE:
            self.tags.add("ids_over_two_tiles")
        served = set()
        seq = base_id
        while seq != end_id:
            if self.channel_ready_flags == 0:
                break
            idx = seq & self.receive_window_mask
            if self.data_flags[idx]:
                channel_id, channel_parent_lead = self.channel_entries[idx]
                bit = 1 << channel_id
                if self.channel_ready_flags & bit:
                    channel = self.channels[channel_id]
                    channel_base_id = channel.base_id if channel.base_id is not None else base_id
                    if channel_parent_lead == 0 or channel_parent_lead > sub(seq, channel_base_id):
                        if channel_id not in served and sub(seq, base_id) >= TILE:
                            self.tags.add("first_delivery_in_later_tile")
                        served.add(channel_id)
                        sink(seq, channel_id, self.data_entries[idx])  # (a dud: None, where the reference panics)
                        self.data_entries[idx] = None
                        self.dud_entries[idx] = False
                        self.data_flags[idx] = False
                        channel.packet_count = (channel.packet_count - 1) & 0xFFFFFFFF
                        if channel.packet_count == 0:
                            self.channel_ready_flags &= ~bit
                        self.set_channel_base_id(channel_id, add(seq, 1))
                    else:
                        self.channel_ready_flags &= ~bit
                        self.tags.add("channel_stalled")
                        later = (sub(seq, base_id) // TILE + 1) * TILE   # the first lead of the next tile
                        for k in range(later, n_ids):
                            j = add(base_id, k) & self.receive_window_mask
                            if self.data_flags[j] and self.channel_entries[j][0] == channel_id:
                                self.tags.add("stalled_with_data_in_later_tile")
                                break
                else:
                    self.tags.add("channel_not_ready")
            seq = add(seq, 1)
        if self.window_ready_flag:
            self.window_ready_flag = False
            new_base_id = base_id
            seq = base_id
            while seq != end_id:
                idx = seq & self.receive_window_mask
                next_id = add(seq, 1)
                if self.entry_flags[idx]:
                    lead = self.window_entries[idx]
                    if lead == 0 or lead > sub(seq, new_base_id):
                        new_base_id = next_id
                    else:
                        self.tags.add("window_stalled")
                        if sub(seq, base_id) >= TILE:
                            self.tags.add("advance_stopped_in_later_tile")
                        break
                seq = next_id
            if sub(new_base_id, base_id) > TILE:
                self.tags.add("advance_past_a_tile_edge")
            self.advance_window(new_base_id)

    def resynchronize(self, sender_next_id):
        base_id = self.base_id
        if sub(sender_next_id, base_id) > self.receive_window_size:
            self.tags.add("resync_ignored")
            return
        seq = base_id
        while seq != sender_next_id:
            if self.entry_flags[seq & self.receive_window_mask]:
                self.tags.add("resync_stopped_at_entry")
                break
            seq = add(seq, 1)
        if seq == sender_next_id:
            self.tags.add("resync_full")
        self.advance_window(seq)


# ---- records <-> classes ----
def align8(v):
    return (v + 7) & ~7


def to_records(rx, carry_base=0, deliver=1, resync_id=NONE):
    """(header RECEIVER_DTYPE[1], slots RX_SLOT_DTYPE[window_size], carry bytes) of a PacketReceiver, the carry
    laid out as the ABI says: slot-index order, held packet then fragment buffer, 8-byte aligned; data_offset =
    carry_base + the slot's offset."""
    W = rx.receive_window_size
    h = np.zeros(1, dtype=fr.RECEIVER_DTYPE)
    h["base_id"], h["end_id"], h["window_size"] = rx.base_id, rx.end_id, W
    h["window_ready"] = 1 if rx.window_ready_flag else 0
    h["deliver"], h["resync_id"] = deliver, resync_id
    h["alloc"], h["max_alloc"] = rx.assembly_window.alloc, rx.max_alloc_given
    h["channel_ready_flags"] = rx.channel_ready_flags
    for c, chn in enumerate(rx.channels):
        h["channel_base_id"][0, c] = NONE if chn.base_id is None else chn.base_id
        h["channel_packet_count"][0, c] = chn.packet_count
    slots = np.zeros(W, dtype=fr.RX_SLOT_DTYPE)
    carry = bytearray()
    for j in range(W):
        s = slots[j]
        e = rx.assembly_window.window[j]
        s["data_offset"] = carry_base + len(carry)
        s["rx_channel_id"], s["rx_channel_parent_lead"] = rx.channel_entries[j]
        s["rx_window_parent_lead"] = rx.window_entries[j]
        s["rx_flags"] = ((fr.RX_SLOT_ENTRY if rx.entry_flags[j] else 0) | (fr.RX_SLOT_DATA if rx.data_flags[j] else 0)
                         | (fr.RX_SLOT_DUD if rx.data_flags[j] and rx.data_entries[j] is None else 0))
        if rx.data_flags[j] and rx.data_entries[j] is not None:
            d = rx.data_entries[j]
            s["data_len"] = len(d)
            carry += d + bytes(align8(len(d)) - len(d))
        if isinstance(e, Closed):
            s["asm_state"], s["asm_size"] = fr.RX_ASM_CLOSED, e.alloc_size
        elif isinstance(e, ActiveEntry):
            b = e.asm_buffer
            s["asm_state"], s["asm_size"] = fr.RX_ASM_ACTIVE, b.total_size
            s["asm_channel_id"] = e.channel_id
            s["asm_window_parent_lead"], s["asm_channel_parent_lead"] = e.window_parent_lead, e.channel_parent_lead
            s["asm_last_fragment_id"] = e.last_fragment_id
            s["asm_received"] = b.num_fragments - b.fragments_remaining
            carry += bytes(b.buffer) + np.array(b.fragment_bitfields, dtype="<u8").tobytes()
    return h, slots, np.frombuffer(bytes(carry), dtype=np.uint8)


def new_state(rxs):
    """(receivers, slots, slot_first, carry) records of a list of PacketReceivers."""
    hs, ss, cs, sf, base = [], [], [], [0], 0
    for rx in rxs:
        h, s, c = to_records(rx, base)
        hs.append(h)
        ss.append(s)
        cs.append(c)
        base += c.size
        sf.append(sf[-1] + s.size)
    return (np.concatenate(hs), np.concatenate(ss), np.array(sf, dtype=np.uint64),
            np.concatenate(cs) if cs else np.zeros(0, np.uint8))


def item_datagram(it, payload, base):
    lo = base + int(it["data_offset"])
    return Datagram(int(it["id"]), int(it["channel_id"]), int(it["window_parent_lead"]), int(it["channel_parent_lead"]),
                    int(it["fragment_id"]), int(it["fragment_id_last"]), payload[lo: lo + int(it["data_len"])].tobytes())


class Batch:
    """The inputs of one batched step besides the state."""

    def __init__(self, infos, items, payload, frame_first, src_base=None, frame_accept=None, resync=None, deliver=None):
        self.infos = np.ascontiguousarray(infos, dtype=fr.FRAME_INFO_DTYPE)
        self.items = np.ascontiguousarray(items, dtype=fr.ITEM_DTYPE)
        self.payload = np.ascontiguousarray(payload, dtype=np.uint8)
        self.frame_first = np.ascontiguousarray(frame_first, dtype=np.uint64)
        self.src_base = None if src_base is None else np.ascontiguousarray(src_base, dtype=np.uint64)
        self.frame_accept = None if frame_accept is None else np.ascontiguousarray(frame_accept, dtype=np.uint8)
        n = self.frame_first.size - 1
        self.resync = [NONE] * n if resync is None else list(resync)
        self.deliver = [1] * n if deliver is None else list(deliver)

    def apply(self, receivers):
        receivers["resync_id"] = self.resync
        receivers["deliver"] = self.deliver
        return receivers


def frames_of(item_lists, per_frame=8, kind=10):
    """infos, items, frame_first for receivers' item lists (each a list of ITEM_DTYPE scalars or tuples): every
    receiver's items cut into data frames of up to per_frame items."""
    infos, items, ff = [], [], [0]
    for lst in item_lists:
        for k in range(0, len(lst), per_frame):
            chunk = lst[k: k + per_frame]
            info = np.zeros(1, dtype=fr.FRAME_INFO_DTYPE)
            info["kind"], info["ok"], info["item_first"], info["item_count"] = kind, 1, len(items), len(chunk)
            infos.append(info)
            items.extend(chunk)
        ff.append(len(infos))
    infos = np.concatenate(infos) if infos else np.zeros(0, dtype=fr.FRAME_INFO_DTYPE)
    arr = np.zeros(len(items), dtype=fr.ITEM_DTYPE)
    for k, it in enumerate(items):
        arr[k] = it
    return infos, arr, np.array(ff, dtype=np.uint64)


def make_item(seq, ch, wl, cl, f, last, off, ln):
    it = np.zeros(1, dtype=fr.ITEM_DTYPE)[0]
    it["id"], it["channel_id"], it["window_parent_lead"], it["channel_parent_lead"] = seq, ch, wl, cl
    it["fragment_id"], it["fragment_id_last"], it["data_offset"], it["data_len"] = f, last, off, ln
    return it


def state_is_bad(h, slots, ff0, ff1, n_frames, s0, s1, n_slots, infos, n_items, carry_in_len):
    W = int(h["window_size"])
    if W == 0 or W > 4096 or W & (W - 1) or int(h["base_id"]) > MASK or int(h["end_id"]) > MASK:
        return True
    if ff0 > ff1 or ff1 > n_frames or s0 > s1 or s1 > n_slots or s1 - s0 < W:
        return True
    for i in range(ff0, ff1):
        if infos[i]["ok"] and int(infos[i]["item_first"]) + int(infos[i]["item_count"]) > n_items:
            return True
    for s in slots[s0: s0 + W]:
        held = int(s["data_len"]) if (int(s["rx_flags"]) & 6) == 2 else 0
        n = int(s["asm_last_fragment_id"]) + 1 if int(s["asm_state"]) == 2 else 0
        region = align8(held) + (n * FRAG + 8 * ((n + 63) // 64) if n else 0)
        off = int(s["data_offset"])
        if int(s["asm_state"]) > 2 or int(s["asm_channel_id"]) >= 64 or int(s["rx_channel_id"]) >= 64:
            return True
        if region and (off & 7 or off > carry_in_len or region > carry_in_len - off):
            return True
    return False


def expected_step(rxs, batch, bad=None):
    """Run one step of `batch` on the PacketReceivers `rxs` (advanced in place).  Returns a dict: per receiver
    the delivered packets [(seq, channel, data or None)], item_status (uint8 per item; 0xEE where no receiver
    owns the item or its receiver is in `bad`), per receiver status counts, packets_completed, packets_dud,
    advanced.  `bad`: indices of receivers whose state the call must refuse (nothing is done for them)."""
    bad = set(bad or ())
    status = np.full(batch.items.size, 0xEE, dtype=np.uint8)
    out = {"delivered": [], "status": status, "counts": [], "completed": [], "dud": [], "advanced": []}
    for r, rx in enumerate(rxs):
        counts = [0] * 11
        delivered, done = [], [0, 0]
        if r in bad:
            out["delivered"].append(delivered)
            out["counts"].append(counts)
            out["completed"].append(0)
            out["dud"].append(0)
            out["advanced"].append(0)
            continue
        rx.advanced = 0
        rx.refused_in_step = False
        if batch.resync[r] != NONE:
            rx.resynchronize(batch.resync[r] & MASK)
        for i in range(int(batch.frame_first[r]), int(batch.frame_first[r + 1])):
            info = batch.infos[i]
            if not info["ok"]:
                continue
            counted = info["kind"] == 10 and (batch.frame_accept is None or batch.frame_accept[i] != 0)
            sb = 0 if batch.src_base is None else int(batch.src_base[i])
            for g in range(int(info["item_first"]), int(info["item_first"]) + int(info["item_count"])):
                it = batch.items[g]
                if not counted:
                    st = fr.RX_NOT_HANDLED
                else:
                    lo, ln = sb + int(it["data_offset"]), int(it["data_len"])
                    # (validity first, from the fields alone; a datagram whose bytes cannot be taken is judged on
                    # its stated length)
                    probe = Datagram(int(it["id"]), int(it["channel_id"]), int(it["window_parent_lead"]),
                                     int(it["channel_parent_lead"]), int(it["fragment_id"]), int(it["fragment_id_last"]),
                                     b"")
                    probe.data = range(ln)  # len() only
                    if not datagram_is_valid(probe) or probe.sequence_id > MASK:
                        st = fr.RX_DROPPED_INVALID
                    elif lo + ln > batch.payload.size:
                        st = fr.RX_DROPPED_BAD_SRC
                    else:
                        st = rx.handle_datagram(item_datagram(it, batch.payload, sb))
                        if st in (fr.RX_COMPLETED, fr.RX_DUD):
                            done[st == fr.RX_DUD] += 1
                status[g] = st
                counts[st] += 1
        if batch.deliver[r]:
            rx.receive(lambda seq, ch, data: delivered.append((seq, ch, data)))
        if rx.advanced > TILE:
            rx.tags.add("advanced_over_one_tile")
        out["delivered"].append(delivered)
        out["counts"].append(counts)
        out["completed"].append(done[0])
        out["dud"].append(done[1])
        out["advanced"].append(rx.advanced)
    return out


FILL = 0xA5


def carry_bound(batch, carry_in_len, n_slots):
    """The header's carry_cap that is always enough: the carry and the payload, 8 bytes of padding per slot, and a
    whole fragment buffer for every datagram that could open one."""
    last = batch.items["fragment_id_last"].astype(np.int64)
    n = last[last > 0] + 1
    return int(carry_in_len + batch.payload.size + 8 * n_slots + (n * FRAG + 8 * ((n + 63) // 64)).sum())


def run_native(call, batch, receivers, slots, slot_first, carry_in, caps=None, **kw):
    """Call a native form (`call` takes receive_packets_host's arguments and returns its dict) on copies of the
    state, outputs pre-filled with FILL."""
    caps = dict(caps or {})
    n_items, n_slots = batch.items.size, slots.size
    carry_cap = caps.get("carry", carry_bound(batch, carry_in.size, n_slots))
    out_cap = caps.get("out", carry_in.size + batch.payload.size)
    packets_cap = caps.get("packets", n_items + n_slots)
    slots2 = slots.copy()
    o = call(batch.infos, batch.items, batch.payload, batch.frame_first, batch.apply(receivers.copy()), slots2, slot_first,
             carry_in, src_base=batch.src_base, frame_accept=batch.frame_accept,
             carry_out=np.full(carry_cap, FILL, dtype=np.uint8), out_bytes=np.full(out_cap, FILL, dtype=np.uint8),
             packets=np.frombuffer(bytes([FILL]) * (24 * packets_cap), dtype=fr.RX_PACKET_DTYPE).copy(), **kw)
    o["slots"] = slots2
    return o


def check(o, exp, rxs, batch, receivers_in, slots_in, slot_first, bad=None, what=""):
    """Compare a native call's outputs `o` (run_native) with the restatement: `exp` = expected_step's result and
    `rxs` the PacketReceivers after the step."""
    bad = set(bad or ())
    n = len(rxs)
    packets_cap, out_cap, carry_cap = o["packets"].size, o["out_bytes"].size, o["carry_out"].size
    pf, ob, cf = [0], [0], [0]
    slots_exp = slots_in.copy()
    heads, carries = [], []
    for r, rx in enumerate(rxs):
        pf.append(pf[-1] + len(exp["delivered"][r]))
        ob.append(ob[-1] + sum(len(d[2] or b"") for d in exp["delivered"][r]))
        if r in bad:
            heads.append(batch.apply(receivers_in.copy())[r: r + 1])
            carries.append(np.zeros(0, np.uint8))
        else:
            h, s, c = to_records(rx, cf[-1], batch.deliver[r], batch.resync[r])
            heads.append(h)
            carries.append(c)
            s0 = int(slot_first[r])
            slots_exp[s0: s0 + s.size] = s
        cf.append(cf[-1] + carries[-1].size)
    assert o["packets_used"] == pf[-1] and o["out_used"] == ob[-1] and o["carry_used"] == cf[-1], \
        (what, o["packets_used"], pf[-1], o["out_used"], ob[-1], o["carry_used"], cf[-1])
    assert o["packet_first"].tolist() == pf, what
    assert o["carry_first"].tolist() == cf, what
    # records and delivered bytes, those below the caps; nothing beyond
    out_exp = np.full(out_cap, FILL, dtype=np.uint8)
    k = 0
    for r in range(n):
        off = ob[r]
        for seq, ch, data in exp["delivered"][r]:
            ln = len(data or b"")
            if k < packets_cap:
                p = o["packets"][k]
                assert (int(p["out_offset"]), int(p["sequence_id"]), int(p["len"]), int(p["channel_id"]), int(p["flags"]),
                        int(p["reserved"]), int(p["reserved2"])) == (off, seq, ln, ch, 1 if data is None else 0, 0, 0), \
                    (what, r, k, p, (off, seq, ln, ch))
            m = max(0, min(ln, out_cap - off))
            out_exp[off: off + m] = np.frombuffer(data or b"", dtype=np.uint8)[:m]
            off += ln
            k += 1
    assert bytes(o["packets"][min(k, packets_cap):].tobytes()) == bytes([FILL]) * (24 * (packets_cap - min(k, packets_cap))), what
    assert np.array_equal(o["out_bytes"], out_exp), what
    if o["item_status"] is not None:
        got = o["item_status"].copy()
        got[exp["status"] == 0xEE] = 0xEE
        assert np.array_equal(got, exp["status"]), (what, got.tolist(), exp["status"].tolist())
    for r in range(n):
        res = o["results"][r]
        want = (pf[r], len(exp["delivered"][r]), exp["counts"][r], exp["completed"][r], exp["dud"][r], exp["advanced"][r],
                fr.RX_BAD_STATE if r in bad else fr.RX_DONE, 0, ob[r + 1] - ob[r])
        got = (int(res["packet_first"]), int(res["packet_count"]), res["status_count"].tolist(), int(res["packets_completed"]),
               int(res["packets_dud"]), int(res["advanced"]), int(res["stop"]), int(res["reserved"]),
               int(res["bytes_delivered"]))
        assert got == want, (what, r, got, want)
        assert o["receivers_out"][r: r + 1].tobytes() == heads[r].tobytes(), (what, r, o["receivers_out"][r], heads[r][0])
    assert o["slots"].size == slots_exp.size, what
    for j in np.flatnonzero((o["slots"].view(np.uint8).reshape(-1, 32) != slots_exp.view(np.uint8).reshape(-1, 32)).any(axis=1)):
        assert o["slots"][j] == slots_exp[j], (what, j, o["slots"][j], slots_exp[j])
    # the carry: held packets and received fragments only (the rest is unspecified), and the bit words
    for r, rx in enumerate(rxs):
        if r in bad:
            continue
        c, base = carries[r], cf[r]
        s0 = int(slot_first[r])
        for j in range(rx.receive_window_size):
            s = slots_exp[s0 + j]
            off = int(s["data_offset"])
            held = int(s["data_len"]) if (int(s["rx_flags"]) & 6) == 2 else 0
            spans = [(off, held)]
            e = rx.assembly_window.window[j]
            if isinstance(e, ActiveEntry):
                b = e.asm_buffer
                fo = off + align8(held)
                for f in range(b.num_fragments):
                    if b.fragment_bitfields[f // 64] >> (f % 64) & 1:
                        spans.append((fo + f * FRAG, FRAG if f < b.num_fragments - 1 else b.total_size - FRAG * (
                            b.num_fragments - b.fragments_remaining - 1)))
                spans.append((fo + b.num_fragments * FRAG, 8 * len(b.fragment_bitfields)))
            for lo, ln in spans:
                hi = min(lo + ln, carry_cap)
                if lo < hi:
                    assert np.array_equal(o["carry_out"][lo:hi], c[lo - base: hi - base]), (what, r, j, lo, ln)
    assert np.all(o["carry_out"][min(cf[-1], carry_cap):] == FILL), what


# ---- calls too large for the restatement: a sample of receivers, sums in numpy, another native form ----
def exclusive_sum(counts):
    return np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)


def sub_batch(batch, sample):
    """The Batch of the receivers `sample` alone: their frames, over the same items and payload."""
    ff = batch.frame_first.astype(np.int64)
    idx = np.concatenate([np.arange(ff[r], ff[r + 1]) for r in sample] + [np.zeros(0, np.int64)]).astype(np.int64)
    first = exclusive_sum([ff[r + 1] - ff[r] for r in sample])
    return Batch(batch.infos[idx], batch.items, batch.payload, first,
                 None if batch.src_base is None else batch.src_base[idx],
                 None if batch.frame_accept is None else batch.frame_accept[idx],
                 [batch.resync[r] for r in sample], [batch.deliver[r] for r in sample])


def check_receivers(o, exp, rxs, batch, sample, receivers_in, slots_in, slot_first, what=""):
    """check() on the receivers `sample` of a call over many more: receiver r's part is cut out of the outputs `o`
    (run_native's, no cap below its need) and laid out as the outputs of a call over the sample alone: its records
    with out_offset relative to the sample's first byte, its delivered bytes (found from bytes_delivered, the
    exclusive sum over all receivers), its carry and slots with data_offset moved likewise.  `exp`, `rxs`: the
    restatement's expected_step over sub_batch(batch, sample) and the sample's PacketReceivers after it."""
    res = o["results"]
    pf, cf = o["packet_first"].astype(np.int64), o["carry_first"].astype(np.int64)
    of = exclusive_sum(res["bytes_delivered"]).astype(np.int64)
    assert o["packets_used"] <= o["packets"].size and o["out_used"] <= o["out_bytes"].size
    assert o["carry_used"] <= o["carry_out"].size and int(of[-1]) == o["out_used"], what
    sf = slot_first.astype(np.int64)
    packets, outs, carries, slots, slots_before, results = [], [], [], [], [], []
    new_pf, new_of, new_cf, new_sf = [0], [0], [0], [0]
    for r in sample:
        W = int(receivers_in["window_size"][r])
        p = o["packets"][pf[r]: pf[r + 1]].copy()
        assert p.size == int(res["packet_count"][r]), (what, r)
        p["out_offset"] = (p["out_offset"].astype(np.int64) - of[r] + new_of[-1]).astype(np.uint64)
        s = o["slots"][sf[r]: sf[r] + W].copy()
        s["data_offset"] = (s["data_offset"].astype(np.int64) - cf[r] + new_cf[-1]).astype(np.uint64)
        one = res[r: r + 1].copy()
        one["packet_first"] = new_pf[-1]
        packets.append(p)
        outs.append(o["out_bytes"][of[r]: of[r + 1]])
        carries.append(o["carry_out"][cf[r]: cf[r + 1]])
        slots.append(s)
        slots_before.append(slots_in[sf[r]: sf[r] + W])
        results.append(one)
        new_pf.append(new_pf[-1] + p.size)
        new_of.append(new_of[-1] + int(of[r + 1] - of[r]))
        new_cf.append(new_cf[-1] + int(cf[r + 1] - cf[r]))
        new_sf.append(new_sf[-1] + W)
    cut = {"packets": np.concatenate(packets), "packet_first": np.array(new_pf, np.uint64), "packets_used": new_pf[-1],
           "out_bytes": np.concatenate(outs), "out_used": new_of[-1], "carry_out": np.concatenate(carries),
           "carry_first": np.array(new_cf, np.uint64), "carry_used": new_cf[-1], "item_status": o["item_status"],
           "results": np.concatenate(results), "receivers_out": o["receivers_out"][list(sample)],
           "slots": np.concatenate(slots)}
    check(cut, exp, rxs, batch, receivers_in[list(sample)], np.concatenate(slots_before), np.array(new_sf, np.uint64),
          what=what)


def slot_regions(slots):
    """Every slot's carry region, in numpy (rx_slot_region)."""
    held = np.where((slots["rx_flags"] & 6) == 2, slots["data_len"], 0).astype(np.uint64)
    n = np.where(slots["asm_state"] == fr.RX_ASM_ACTIVE, slots["asm_last_fragment_id"].astype(np.uint64) + 1, 0).astype(np.uint64)
    return ((held + 7) & ~np.uint64(7)) + n * FRAG + 8 * ((n + 63) // 64), held


def check_sums(o, slot_first, what=""):
    """The firsts and used counts of a call from its own per-receiver outputs: packet_first the exclusive sum of
    the results' packet_count, carry_first that of the carry sizes recomputed from the output slots (the receivers'
    slot ranges lie one behind the other), out_used the sum of bytes_delivered."""
    res = o["results"]
    assert np.array_equal(o["packet_first"], exclusive_sum(res["packet_count"])), what
    assert np.array_equal(res["packet_first"], o["packet_first"][:-1].astype(np.uint32)), what
    region, _ = slot_regions(o["slots"])
    sf = slot_first.astype(np.int64)
    per = np.add.reduceat(region, sf[:-1]) if sf.size > 1 else np.zeros(0, np.uint64)
    per[sf[:-1] == sf[1:]] = 0
    assert np.array_equal(o["carry_first"], exclusive_sum(per)), what
    assert o["packets_used"] == int(o["packet_first"][-1]) and o["carry_used"] == int(o["carry_first"][-1]), what
    assert o["out_used"] == int(res["bytes_delivered"].sum(dtype=np.uint64)), what


def span_index(offsets, lengths):
    """The indices of the bytes [offsets[k], offsets[k] + lengths[k]) for every k, in numpy."""
    lengths = lengths.astype(np.int64)
    total = int(lengths.sum())
    starts = np.cumsum(lengths) - lengths
    return np.repeat(offsets.astype(np.int64) - starts, lengths) + np.arange(total, dtype=np.int64)


def check_same(o, h, what=""):
    """Two native forms of one call over inputs that leave no ACTIVE slot behind, both from run_native (outputs
    pre-filled with FILL): every record, count, status, state field and slot equal, the delivered bytes equal and
    FILL behind them, the carry equal over the held packets' bytes (the padding between them is unspecified) and
    FILL behind carry_used."""
    for key in ("packets_used", "out_used", "carry_used"):
        assert o[key] == h[key], (what, key, o[key], h[key])
    for key in ("packet_first", "carry_first", "item_status", "out_bytes"):
        assert np.array_equal(o[key], h[key]), (what, key)
    for key in ("results", "receivers_out", "slots", "packets"):
        assert o[key].size == h[key].size, (what, key)
        a, b = o[key].view(np.uint8).reshape(o[key].size, -1), h[key].view(np.uint8).reshape(h[key].size, -1)
        if not np.array_equal(a, b):
            bad = np.flatnonzero((a != b).any(axis=1))
            assert bad.size == 0, (what, key, bad.size, bad[:8].tolist(), o[key][bad[0]], h[key][bad[0]])
    assert np.all(o["out_bytes"][o["out_used"]:] == FILL) and np.all(o["carry_out"][o["carry_used"]:] == FILL), what
    assert np.all(o["packets"][o["packets_used"]:].view(np.uint8) == FILL), what
    assert not np.any(o["slots"]["asm_state"] == fr.RX_ASM_ACTIVE), what
    _, held = slot_regions(o["slots"])
    k = np.flatnonzero(held)
    idx = span_index(o["slots"]["data_offset"][k], held[k])
    assert idx.size == 0 or int(idx.max()) < o["carry_used"], what
    assert np.array_equal(o["carry_out"][idx], h["carry_out"][idx]), what


# ---- generators ----
class GenSender:
    """A plain sender model for the generators: sequence ids, window and channel parents (reliable packets become
    parents), fragments."""

    def __init__(self, next_id):
        self.next_id = next_id
        self.window_parent = None
        self.channel_parent = [None] * CHANNELS

    def packet(self, ch, reliable, data):
        seq = self.next_id
        self.next_id = add(seq, 1)
        wl = 0 if self.window_parent is None else sub(seq, self.window_parent) & 0xFFFF
        cl = 0 if self.channel_parent[ch] is None else sub(seq, self.channel_parent[ch]) & 0xFFFF
        if reliable:
            self.window_parent = self.channel_parent[ch] = seq
        last = max((len(data) + FRAG - 1) // FRAG, 1) - 1
        return [(seq, ch, wl, cl, f, last, data[f * FRAG: (f + 1) * FRAG]) for f in range(last + 1)]


class PayloadArena:
    def __init__(self, rng, lead=3):
        self.buf = bytearray(rng.integers(0, 256, lead, dtype=np.uint8).tobytes())  # odd offsets from the start

    def put(self, data):
        off = len(self.buf)
        self.buf += data
        return off

    def array(self):
        return np.frombuffer(bytes(self.buf), dtype=np.uint8)


def datagram_items(arena, dgs):
    """ITEM_DTYPE scalars of (seq, ch, wl, cl, f, last, data) tuples, their bytes put into the arena."""
    return [make_item(seq, ch, wl, cl, f, last, arena.put(data), len(data)) for seq, ch, wl, cl, f, last, data in dgs]


class Harness:
    """PacketReceivers and their records side by side, stepped together: every step is checked in full."""

    def __init__(self, rxs, call):
        self.rxs = rxs
        self.call = call
        self.receivers, self.slots, self.slot_first, self.carry = new_state(rxs)

    def step(self, batch, caps=None, bad=None, what="", **kw):
        exp = expected_step(self.rxs, batch, bad)
        o = run_native(self.call, batch, self.receivers, self.slots, self.slot_first, self.carry, caps, **kw)
        check(o, exp, self.rxs, batch, self.receivers, self.slots, self.slot_first, bad, what)
        self.receivers, self.slots = o["receivers_out"], o["slots"]
        self.carry = o["carry_out"][:min(o["carry_used"], o["carry_out"].size)].copy()  # the carry swap
        return o, exp


def simple_batch(item_lists_dgs, rng=None, per_frame=8, lead=3, **kw):
    """A Batch from, per receiver, a list of (seq, ch, wl, cl, f, last, data) tuples."""
    arena = PayloadArena(rng or np.random.default_rng(1), lead)
    lists = [datagram_items(arena, dgs) for dgs in item_lists_dgs]
    infos, items, ff = frames_of(lists, per_frame)
    return Batch(infos, items, arena.array(), ff, **kw)


SIZES = (0, 1, 7, 64, 200, FRAG - 1, FRAG, FRAG + 1, 2 * FRAG, 3 * FRAG - 5)


def gen_step(rng, rxs, senders, held, n_packets=10, sizes=SIZES, chaos=True, per_frame=5, lie=0.1, resync=0.12,
             hold=0.15):
    """One random step for every receiver: new packets from its sender model (within the receiver's window),
    then reordering, delays to the next step (`held`, per receiver), duplicates with other bytes, mismatching
    fragments, invalid, out-of-window and out-of-payload datagrams, and frames that do not count.  At the rates
    `lie`, `resync` and `hold`: a sender that denies its parents (leads of zero: the window passes packets that
    were never delivered), a step that resynchronizes (to the sender's next id, or to an id inside the window)
    and a step that does not deliver.  Returns a Batch."""
    arena = PayloadArena(rng)
    lists = []
    for r, (rx, tx) in enumerate(zip(rxs, senders)):
        dgs, held[r] = held[r], []
        W = rx.receive_window_size
        room = W - sub(tx.next_id, rx.base_id) if sub(tx.next_id, rx.base_id) <= W else 0
        for _ in range(min(n_packets, room)):
            size = int(sizes[rng.integers(0, len(sizes))])
            data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            new = tx.packet(int(rng.integers(0, 3)), bool(rng.random() < 0.5), data)
            if chaos and rng.random() < lie:
                if rng.random() < 0.5:   # no parents at all
                    new = [(seq, ch, 0, 0, f, last, d) for seq, ch, wl, cl, f, last, d in new]
                else:                    # on another channel than the one its children will name it on
                    new = [(seq, (ch + 1) % 3, wl, wl, f, last, d) for seq, ch, wl, cl, f, last, d in new]
            dgs += new
        out = []
        for dg in dgs:
            seq, ch, wl, cl, f, last, data = dg
            u = rng.random() if chaos else 1.0
            if u < 0.10:
                held[r].append(dg)
                continue
            out.append(dg)
            if u < 0.22:  # a duplicate that carries other bytes; now or in the next step
                other = (seq, ch, wl, cl, f, last, bytes(b ^ 0x5A for b in data))
                (out if u < 0.16 else held[r]).append(other)
            elif u < 0.26 and last > 0:
                out.append((seq, ch, wl + 1, cl + 1 if cl else 0, f, last, data))  # other leads
            elif u < 0.29:
                out.append((seq, ch, wl, cl, last + 1, last, data))                 # fragment_id > last
            elif u < 0.31:
                out.append((seq | 0x100000, ch, wl, cl, f, last, data))             # id >= 2^20
            elif u < 0.34:
                out.append((add(seq, W), ch, wl, cl, f, last, data))                # beyond the window
        if chaos:
            order = np.argsort(np.arange(len(out)) + rng.integers(0, 6, len(out)), kind="stable")
            out = [out[k] for k in order]
        lists.append(datagram_items(arena, out))
    infos, items, ff = frames_of(lists, per_frame)
    payload = arena.array()
    accept = None
    if chaos and infos.size:
        accept = (rng.random(infos.size) > 0.06).astype(np.uint8)
        for i in np.flatnonzero(rng.random(infos.size) < 0.04):
            infos[i]["kind"] = 12  # an ack frame among them
        for g in np.flatnonzero(rng.random(items.size) < 0.02):
            items[g]["data_offset"] = payload.size - int(items[g]["data_len"]) + 1 + int(rng.integers(0, 50))
    n = len(rxs)
    resyncs, delivers = [NONE] * n, [1] * n
    if chaos:
        for r, (rx, tx) in enumerate(zip(rxs, senders)):
            u = rng.random()
            if u < resync / 2:
                resyncs[r] = tx.next_id
            elif u < resync:
                resyncs[r] = add(rx.base_id, int(rng.integers(0, rx.receive_window_size + 2)))
            delivers[r] = 0 if rng.random() < hold else 1
    return Batch(infos, items, payload, ff, frame_accept=accept, resync=resyncs, deliver=delivers)


# ---- batches for many receivers, built in numpy ----
def pair_batch(rng, bases, size0, size1, copies=4, lead=3):
    """A step in which receiver r (window of two ids or more, base bases[r]) gets two whole packets of size0[r] and
    size1[r] bytes, ids base and base + 1, channels 0 to 2, the first reliable (the second names it as its window
    parent, and as its channel parent where the channels agree).  A packet's fragments arrive last first, every
    datagram `copies` times in a row, the later copies with other bytes: the first arrival wins, the later ones
    find the slot closed or, while a fragment buffer is open, their fragment's bit in the step's duplicate table.
    One frame per datagram (its copies).  Returns a Batch that does not deliver, and the packets' channels."""
    n = bases.size
    size = np.stack([size0, size1], axis=1).reshape(-1).astype(np.int64)          # per packet: 2 r + k
    nf = np.maximum(1, (size + FRAG - 1) // FRAG)
    ch = rng.integers(0, 3, 2 * n)
    pid = (np.repeat(bases.astype(np.int64), 2) + np.tile([0, 1], n)) & MASK
    second = np.tile([0, 1], n)
    cl = second * (ch == np.roll(ch, 1))
    D = int(nf.sum())
    p = np.repeat(np.arange(2 * n), nf)
    f = nf[p] - 1 - (np.arange(D) - np.repeat(np.cumsum(nf) - nf, nf))
    ln = np.where(f < nf[p] - 1, FRAG, size[p] - (nf[p] - 1) * FRAG)
    d = np.repeat(np.arange(D), copies)
    items = np.zeros(D * copies, dtype=fr.ITEM_DTYPE)
    items["id"], items["channel_id"] = pid[p][d], ch[p][d]
    items["window_parent_lead"], items["channel_parent_lead"] = second[p][d], cl[p][d]
    items["fragment_id"], items["fragment_id_last"], items["data_len"] = f[d], (nf[p] - 1)[d], ln[d]
    items["data_offset"] = lead + np.cumsum(ln[d]) - ln[d]
    payload = rng.integers(0, 256, lead + int(ln[d].sum()), dtype=np.uint8)
    infos = np.zeros(D, dtype=fr.FRAME_INFO_DTYPE)
    infos["kind"], infos["ok"], infos["item_count"], infos["item_first"] = 10, 1, copies, np.arange(D) * copies
    per = nf.reshape(-1, 2).sum(axis=1)
    return Batch(infos, items, payload, exclusive_sum(per), deliver=[0] * n), ch.reshape(-1, 2)


def sparse_batch(n, frames, rng=None, lead=3, **kw):
    """A Batch over n receivers of which only a few have frames: frames = {receiver: [(kind, accept, [datagram
    tuples])]}, the others' ranges empty."""
    arena = PayloadArena(rng or np.random.default_rng(1), lead)
    infos, items, accept, count = [], [], [], np.zeros(n, dtype=np.int64)
    for r in sorted(frames):
        for kind, acc, dgs in frames[r]:
            info = np.zeros(1, dtype=fr.FRAME_INFO_DTYPE)
            info["kind"], info["ok"], info["item_first"], info["item_count"] = kind, 1, len(items), len(dgs)
            infos.append(info)
            accept.append(acc)
            items += datagram_items(arena, dgs)
        count[r] = len(frames[r])
    arr = np.zeros(len(items), dtype=fr.ITEM_DTYPE)
    for k, it in enumerate(items):
        arr[k] = it
    infos = np.concatenate(infos) if infos else np.zeros(0, dtype=fr.FRAME_INFO_DTYPE)
    return Batch(infos, arr, arena.array(), exclusive_sum(count), frame_accept=np.array(accept, dtype=np.uint8), **kw)


def sample_of(rng, n, fixed, size=64):
    """`size` receiver indices or more: the `fixed` ones that exist, the rest drawn."""
    s = {int(r) for r in fixed if 0 <= r < n}
    while len(s) < min(size, n):
        s.add(int(rng.integers(0, n)))
    return sorted(s)
