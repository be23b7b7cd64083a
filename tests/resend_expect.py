"""What the batched resend calls (ufc_resend_begin_* / ufc_resend_place_* / ufc_resend_commit_*) must compute, and the
driver and traffic both test modules share (test infrastructure, not a test module).

`HalfTx` restates the sender's half of HalfConnection (src/half_connection/mod.rs): handle_ack_frame (:154-163) and
emit_data_frames (:335-432) as the reference interleaves them, frame by frame and fragment by fragment, over
  - `Heap`, std's BinaryHeap (push / pop / sift_down_to_bottom / sift_up) ordered on resend_time reversed
    (resend_queue.rs),
  - `Dfe`, DataFrameEmitter::push and finalize (emit.rs:47-125),
  - emit_expect.Tx (PacketSender) with emit_expect.packet_items (PendingPacket::datagram),
  - queue_expect.FrameQueue (frame_queue.rs), whose acknowledge_fragment hook is PendingPacket::acknowledge_fragment
    behind Weak::upgrade (a fragment ref is the packet *object*: an id that comes round again is another packet),
  - pack_expect.encoded_size (DataFrameBuilder::encoded_size, from the codec oracle).
Where the reference never returns (mod.rs:405-407, :422-424) the model ends the flush and says so; the two capacity
stops of the batched calls (a full stage, a full heap) are modelled as the header states them.  Nothing of the product
is used except the record dtypes.

`Pipeline` runs the same traffic through the batched calls, one tick at a time: frame_queue -> resend_begin ->
emit_packets -> resend_place -> pack -> build_sizes -> resend_commit -> emit_packets (state only), through a backend
(the host calls here; tests/test_gpu_resend.py plugs the device calls in), and `compare` holds every record, the heap
byte for byte, the packet table, the ack bytes, the tx ring and the sent records against the model.
"""
import ctypes
import random
from collections import deque

import numpy as np

import emit_expect as E
import pack_expect as P
import queue_expect as Q
from uflow_amd import frame as fr
from uflow_amd._native import lib, check as native_check

M64 = (1 << 64) - 1
ID_MASK = E.ID_MASK
DONE, SIZE_LIMITED, WINDOW_LIMITED, REF_HANG, BAD_STATE, STAGE_FULL, HEAP_FULL = range(7)
STOP_NAMES = ("DONE", "SIZE_LIMITED", "WINDOW_LIMITED", "REF_HANG", "BAD_STATE", "STAGE_FULL", "HEAP_FULL")


# ---- std::collections::BinaryHeap<resend_queue::Entry> ----
class HeapEntry:
    __slots__ = ("packet", "fragment_id", "resend_time", "send_count")

    def __init__(self, packet, fragment_id, resend_time, send_count):
        self.packet, self.fragment_id, self.resend_time, self.send_count = packet, fragment_id, resend_time, send_count


def le(a, b):  # Ord for Entry: resend_time compared, reversed
    return a.resend_time >= b.resend_time


class Heap:
    def __init__(self):
        self.d = []

    def __len__(self):
        return len(self.d)

    def peek(self):
        return self.d[0] if self.d else None

    def push(self, x):
        self.d.append(x)
        self.sift_up(0, len(self.d) - 1)

    def sift_up(self, start, pos):
        d = self.d
        elem = d[pos]
        while pos > start:
            parent = (pos - 1) // 2
            if le(elem, d[parent]):
                break
            d[pos] = d[parent]
            pos = parent
        d[pos] = elem

    def pop(self):
        d = self.d
        if not d:
            return None
        item = d.pop()
        if d:
            item, d[0] = d[0], item
            self.sift_down_to_bottom(0)
        return item

    def sift_down_to_bottom(self, pos):
        d = self.d
        end = len(d)
        start = pos
        elem = d[pos]
        child = 2 * pos + 1
        while child + 1 < end:  # child <= end.saturating_sub(2)
            child += 1 if le(d[child], d[child + 1]) else 0
            d[pos] = d[child]
            pos = child
            child = 2 * pos + 1
        if child == end - 1:
            d[pos] = d[child]
            pos = child
        d[pos] = elem
        self.sift_up(start, pos)


# ---- PendingPacket ----
class Packet:
    def __init__(self, rec, seq, wl, cl, resend):
        self.rec = rec                       # the PACKET_DTYPE record (data_offset, data_len, channel_id)
        self.size = int(rec["data_len"])
        self.seq, self.wl, self.cl, self.resend = seq, wl, cl, resend
        self.items = E.packet_items(rec, seq, wl, cl)
        self.last = len(self.items) - 1
        self.acked = [False] * len(self.items)
        self.frag_first = None               # (the batch's ack ring position: layout, not reference state)


# ---- DataFrameEmitter ----
class Dfe:
    def __init__(self, now_ms, frame_queue, flush_alloc, on_frame):
        self.now_ms, self.fq, self.alloc, self.on_frame = now_ms, frame_queue, flush_alloc, on_frame
        self.cur = None  # [frame id, size, [(packet, fragment, resend)]]
        self.marked = False   # mark_rate_limited was called in this flush

    def mark(self):
        self.marked = True
        self.fq.mark_rate_limited()

    def push(self, packet, fragment_id, resend):
        e = P.encoded_size(packet.items[fragment_id])
        if self.cur is not None:
            frame_size = self.cur[1]
            if self.alloc - frame_size < 0:
                self.finalize()
                self.mark()
                return SIZE_LIMITED
            if frame_size + e > P.MAX_FRAME_SIZE or len(self.cur[2]) >= P.MAX_PACKET_COUNT:
                self.finalize()
            else:
                self.cur[1] += e
                self.cur[2].append((packet, fragment_id, resend))
                return DONE
        if self.alloc < 0:
            self.mark()
            return SIZE_LIMITED
        if not self.fq.can_push():
            return WINDOW_LIMITED
        self.cur = [self.fq.next_id(), P.DATA_FRAME_OVERHEAD + e, [(packet, fragment_id, resend)]]
        return DONE

    def finalize(self):
        if self.cur is not None:
            frame_id, size, frags = self.cur
            self.cur = None
            refs = tuple((p, f) for p, f, r in frags if r)
            self.fq.push(size, self.now_ms, refs, False)
            self.alloc -= size
            self.on_frame(frame_id, size, frags)


class FlushLog:
    """What one flush did: for the comparison with the batched calls' results."""

    def __init__(self):
        self.frames = []           # [(frame id, size, [(seq, fragment, resend)])]
        self.loop_stop = DONE      # how the resend loop ended (begin's stop)
        self.n_resent = self.dead = self.acked = 0
        self.pending_staged = 0
        self.pending_packed = 0
        self.entered = 0
        self.pushed = self.dropped = 0
        self.size_limited = False  # mark_rate_limited was called
        self.consumed = 0          # queue entries taken (emitted or dropped stale)
        self.alloc_left = 0


class HalfTx:
    def __init__(self, window_size, base_id, max_alloc, frame_window, frame_tail, frame_base, heap_cap=None,
                 stage_cap=None):
        self.tx = E.Tx(window_size, base_id, max_alloc)
        self.pk = {}                         # the window: seq -> Packet
        self.fq = Q.FrameQueue(frame_window, frame_tail, frame_base)
        self.fq.acknowledge_fragment = self.acknowledge_fragment
        self.pending = deque()               # (Packet, fragment, resend)
        self.heap = Heap()
        self.queue = deque()                 # PACKET_DTYPE records (packet_send_queue)
        self.window_bytes = 0
        self.heap_cap, self.stage_cap = heap_cap, stage_cap
        self.freed = self.bytes_freed = self.ignored = 0   # since the last flush
        self.refs_acked = 0
        self.alive_at_tick = set()

    def alive(self, packet):  # Weak::upgrade
        return self.pk.get(packet.seq) is packet

    def acknowledge_fragment(self, ref):
        packet, f = ref
        if packet in self.alive_at_tick:   # (the batch marks before the tick's acknowledges, and counts there)
            self.refs_acked += 1
        if self.alive(packet):
            packet.acked[f] = True

    def handle_ack_frame(self, frame_window_base_id, packet_window_base_id, groups, rtt_ms):  # mod.rs:154-163
        for base_id, bitfield, nonce in groups:
            self.fq.acknowledge_group(base_id, bitfield, nonce, rtt_ms)
        self.fq.advance_transfer_window(frame_window_base_id, rtt_ms)
        self.acknowledge(packet_window_base_id)

    def acknowledge(self, receiver_base_id):  # packet_sender.rs:242-275
        tx = self.tx
        if receiver_base_id > ID_MASK or E.sub(receiver_base_id, tx.base_id) > E.sub(tx.next_id, tx.base_id):
            self.ignored += 1
            return
        while tx.base_id != receiver_base_id:
            p = self.pk.pop(tx.base_id)
            self.window_bytes -= p.size
            self.bytes_freed += p.size
            self.freed += 1
            a, ch = tx.window.pop(tx.base_id)
            if tx.window_parent_id == tx.base_id:
                tx.window_parent_id = None
            if tx.channel_parent_id[ch] == tx.base_id:
                tx.channel_parent_id[ch] = None
            tx.alloc -= a
            tx.base_id = (tx.base_id + 1) & ID_MASK

    def emit_packet(self, flush_id, log):  # packet_sender.rs:149-238 over the queue
        while self.queue and int(self.queue[0]["mode"]) == E.TIME_SENSITIVE and int(self.queue[0]["flush_id"]) != flush_id:
            self.queue.popleft()
            log.consumed += 1
        if not self.queue:
            return None
        rec = self.queue[0]
        got = self.tx.emit_packet(int(rec["data_len"]), int(rec["channel_id"]), int(rec["mode"]))
        if got in (E.WINDOW_LIMITED, E.ALLOC_LIMITED):
            return None
        self.queue.popleft()
        log.consumed += 1
        seq, wl, cl, resend = got
        p = Packet(rec, seq, wl, cl, resend)
        self.pk[seq] = p
        self.window_bytes += p.size
        log.entered += 1
        return p, resend

    def heap_push(self, entry, log):
        if self.heap_cap is not None and len(self.heap) >= self.heap_cap:
            log.dropped += 1   # (the batch's HEAP_FULL rule)
            return
        self.heap.push(entry)
        log.pushed += 1

    def flush(self, now_ms, rtt_ms, flush_id, flush_alloc, no_flush=False):
        """emit_data_frames (mod.rs:335-432).  Returns a FlushLog."""
        log = FlushLog()
        log.alloc_left = flush_alloc
        if no_flush:
            return log
        dfe = Dfe(now_ms, self.fq, flush_alloc,
                  lambda fid, size, frags: log.frames.append((fid, size, [(p.seq, f, r) for p, f, r in frags])))

        def done(stop=None):
            if stop is not None:
                log.loop_stop = stop
            log.size_limited = dfe.marked
            log.alloc_left = dfe.alloc
            return log

        while True:  # :351-383
            entry = self.heap.peek()
            if entry is None:
                break
            if self.alive(entry.packet):
                if entry.packet.acked[entry.fragment_id]:
                    self.heap.pop()
                    log.acked += 1
                    continue
                if entry.resend_time > now_ms:
                    break
                if self.stage_cap is not None and log.n_resent >= self.stage_cap:  # (the batch's STAGE_FULL rule)
                    dfe.finalize()
                    return done(STAGE_FULL)
                r = dfe.push(entry.packet, entry.fragment_id, True)
                if r == WINDOW_LIMITED:
                    return done(WINDOW_LIMITED)
                if r == SIZE_LIMITED:
                    return done(SIZE_LIMITED)
                log.n_resent += 1
                entry = self.heap.pop()
                new_time = (now_ms + rtt_ms * (1 << (entry.send_count & 63))) & M64
                new_count = min((entry.send_count + 1) & 0xFF, 2)
                self.heap.push(HeapEntry(entry.packet, entry.fragment_id, new_time, new_count))
            else:
                self.heap.pop()
                log.dead += 1
        if self.pending:
            # the front the reference would spin on (:405-407, :422-424), and the batch's stage capacity
            packet, f, _ = self.pending[0]
            if not self.alive(packet) or packet.acked[f]:
                dfe.finalize()
                return done(REF_HANG)
            if self.stage_cap is not None and log.n_resent + len(self.pending) > self.stage_cap:
                dfe.finalize()
                return done(STAGE_FULL)
            log.pending_staged = len(self.pending)
        first_pending = len(self.pending)
        while True:  # :385-427
            if not self.pending:
                got = self.emit_packet(flush_id, log)
                if got is None:
                    break
                packet, resend = got
                for i in range(packet.last + 1):
                    self.pending.append((packet, i, resend))
            stop = None
            while self.pending:
                packet, f, resend = self.pending[0]
                assert self.alive(packet) and not packet.acked[f]   # (else the reference spins: handled above)
                r = dfe.push(packet, f, resend)
                if r != DONE:
                    stop = r
                    break
                self.pending.popleft()
                if first_pending:
                    first_pending -= 1
                    log.pending_packed += 1
                if resend:
                    self.heap_push(HeapEntry(packet, f, (now_ms + rtt_ms) & M64, 1), log)
            if stop is not None:
                return done()
        dfe.finalize()
        return done()


# ---- the batched pipeline ----
def build_sizes_host(infos, items):
    n = infos.size
    out = np.zeros(n + 1, dtype=np.uint64)
    native_check(lib().ufc_build_sizes_host(infos.ctypes.data if n else None, items.ctypes.data if items.size else None,
                                            items.size, None, 1 << 40, n, out.ctypes.data, None, 1), "ufc_build_sizes_host")
    return out


class HostBackend:
    """The calls of a tick on host arrays; every method returns host arrays."""

    def __init__(self, nthreads=1):
        self.nthreads = nthreads

    def frame_queue(self, infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked):
        r = fr.frame_queue_host(infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked=ref_acked,
                                nthreads=self.nthreads, queues_out=queues)
        return r["results"]

    def resend_begin(self, infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags):
        return fr.resend_begin_host(infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags=flags,
                                    nthreads=self.nthreads, states_out=states, senders_out=senders)["results"]

    def emit(self, packets, packet_first, senders, items):
        return fr.emit_packets_host(packets, packet_first, senders, items=items, nthreads=self.nthreads)

    def emit_state(self, packets, packet_first, senders):
        out = fr.emit_packets_host(packets, packet_first, senders, items_cap=0, nthreads=self.nthreads)
        return out[3], out[4]

    def resend_place(self, states, begin_results, arenas, flush_first, items):
        fr.resend_place_host(states, begin_results, arenas, flush_first, items, nthreads=self.nthreads)

    def pack(self, items, flush_first, flushes):
        return fr.pack_host(items, flush_first, flushes, nthreads=self.nthreads)

    def build_sizes(self, infos, items):
        return build_sizes_host(infos, items)

    def resend_commit(self, *args, **kw):
        return fr.resend_commit_host(*args, nthreads=self.nthreads, **kw)


class Config:
    def __init__(self, window_size=16, max_alloc=40000, frame_window=8, frame_tail=8, heap_cap=256, stage_cap=None,
                 pkt_cap=None, frag_cap=None, tx_cap=None, base_id=0, frame_base=0):
        self.__dict__.update(locals())
        del self.__dict__["self"]


def marked_refs_of_lane(state, ref_acked, lane=63):
    """How many of a connection's live refs that begin's ack propagation gives to `lane` (the j-th live ref goes to
    lane j % 64) the frame queue has marked: work that only a pass over all 64 lanes does."""
    live, mask = (int(state["tx_head"]) - int(state["tx_tail"])) & 0xFFFFFFFF, int(state["tx_cap"]) - 1
    first, tail = int(state["tx_first"]), int(state["tx_tail"])
    return sum(1 for j in range(lane, live, 64) if ref_acked[first + ((tail + j) & mask)])


def idle_config():
    """An idle filler: the smallest legal capacities (about 3 KB of arena), no packets and no acks ever."""
    return Config(window_size=1, max_alloc=1448, frame_window=1, frame_tail=0, heap_cap=1, stage_cap=1)


def padding_layout(n, replicas, fillers, tail_replicas=0):
    """The kinds of the padding connections in batch order, True a replica and False an idle filler: `replicas` spread
    evenly over the padding slots among the first 256 connections (so that no wave of 64 there holds idle fillers only,
    and the modelled connections share theirs with replicas), those that do not fit there right behind, the idle
    fillers, and `tail_replicas` more replicas at the highest indices."""
    head = max(min(256 - n, replicas + fillers), 0)
    in_head = min(replicas, head)
    kinds = [(k + 1) * in_head // head != k * in_head // head for k in range(head)]
    kinds += [True] * (replicas - in_head) + [False] * (fillers - (head - in_head)) + [True] * tail_replicas
    assert len(kinds) == replicas + fillers + tail_replicas and sum(kinds) == replicas + tail_replicas
    return kinds


class Pipeline:
    """n connections through the batched calls, with one HalfTx model each.

    Padding: `replicas` + `tail_replicas` + `fillers` more connections behind the n modelled ones, in the same arrays
    and arenas (guards between all regions), laid out by padding_layout; every call of a tick gets the whole batch.
    The k-th replica in batch order has the Config of modelled connection k % n and gets its packets, acks,
    flush_alloc, flags and take every tick; an idle filler has idle_config() and gets nothing.  The models, `compare`
    and tick's return value cover the first n; what the calls did to the padding is for the backend to check (against
    the host calls: tests/test_gpu_resend.py's CheckedBackend), and `pad_totals` sums some of its result fields."""

    def __init__(self, configs, backend=None, replicas=0, fillers=0, tail_replicas=0):
        self.backend = backend or HostBackend()
        self.cfg = configs
        n = self.n = len(configs)
        for c in configs:
            if c.stage_cap is None:
                c.stage_cap = c.heap_cap + 200
        self.models = [HalfTx(c.window_size, c.base_id, c.max_alloc, c.frame_window, c.frame_tail, c.frame_base,
                              heap_cap=c.heap_cap, stage_cap=c.stage_cap) for c in configs]
        kinds = padding_layout(n, replicas, fillers, tail_replicas)
        total = self.total = n + len(kinds)
        # src[c]: the modelled connection whose traffic batch index c gets; -1 an idle filler
        self.src = np.arange(total, dtype=np.int64)
        self.src[n:] = -1
        rep = n + np.flatnonzero(kinds)
        self.src[rep] = np.arange(rep.size) % max(n, 1)
        self.active = np.flatnonzero(self.src >= 0)   # batch indices with traffic, ascending
        # one record of each kind per distinct config, then every connection's copy
        idle = idle_config()
        kind_cfg = list(configs) + [idle]
        t_senders = np.zeros(n + 1, dtype=fr.SENDER_DTYPE)
        t_queues = np.zeros(n + 1, dtype=fr.FRAME_QUEUE_DTYPE)
        t_states = np.zeros(n + 1, dtype=fr.RESEND_DTYPE)
        for k, cf in enumerate(kind_cfg):
            E.Tx(cf.window_size, cf.base_id, cf.max_alloc).to_record(t_senders[k])
            t_queues[k] = fr.new_frame_queues(1, cf.frame_window, cf.frame_tail, cf.frame_base)[0][0]
            t_states[k] = fr.new_resend_states(1, cf.window_size, cf.max_alloc, cf.frame_window, cf.frame_tail, cf.heap_cap,
                                               stage_cap=cf.stage_cap, pkt_cap=cf.pkt_cap, frag_cap=cf.frag_cap,
                                               tx_cap=cf.tx_cap)[0][0]
        kind = np.where(self.src >= 0, self.src, n)
        self.senders, self.queues, self.states = t_senders[kind], t_queues[kind], t_states[kind]
        # (regions need not start at 0 nor lie back to back: three records before every log ring, one before and one
        # behind every other region)
        step = self.queues["log_cap"].astype(np.uint64) + np.uint64(3)
        ends = np.cumsum(step, dtype=np.uint64)
        self.queues["log_first"] = ends - self.queues["log_cap"]
        sizes = {"log": int(ends[-1]) if total else 0}
        self.guard_at = {}
        for name, key in (("heap", "heap"), ("pkt", "pkts"), ("frag", "frag_acked"), ("tx", "tx"), ("stage", "stage")):
            cap = self.states[name + "_cap"].astype(np.uint64)
            ends = np.cumsum(cap + np.uint64(2), dtype=np.uint64)
            first = ends - cap - np.uint64(1)
            self.states[name + "_first"] = first
            sizes[key] = int(ends[-1]) if total else 0
            self.guard_at[key] = np.concatenate([first - np.uint64(1), first + cap]).astype(np.int64)
        self.guard_at["ref_acked"] = self.guard_at["tx"]
        self.layout = self.states.copy()
        self.log = np.zeros(sizes["log"], dtype=fr.SENT_FRAME_DTYPE)
        self.arenas = {"heap": np.zeros(sizes["heap"], fr.RESEND_ENTRY_DTYPE), "pkts": np.zeros(sizes["pkts"], fr.SENT_PACKET_DTYPE),
                       "frag_acked": np.zeros(sizes["frag_acked"], np.uint8), "tx": np.zeros(sizes["tx"], fr.TX_REF_DTYPE),
                       "ref_acked": np.zeros(sizes["tx"], np.uint8), "stage": np.zeros(sizes["stage"], fr.ITEM_DTYPE)}
        self.arenas["frag_acked"][:] = 0x5A   # (an ack byte must be zeroed when its packet enters, not before)
        self.guard = {k: v[self.guard_at[k]].copy() for k, v in self.arenas.items()}
        self.sent = np.zeros(0, dtype=fr.SENT_FRAME_DTYPE)
        self.sent_first = np.zeros(total + 1, dtype=np.uint64)
        self.extra = np.zeros(total, dtype=np.uint32)
        self.backlog = [[] for _ in range(n)]   # PACKET_DTYPE records not yet consumed
        self.flush_id = 0
        self.seen_stops = set()
        self.seen = set()
        self.arena_len = 0
        self.pad_totals = {"packets_freed": 0, "refs_acked": 0, "n_resent": 0, "heap_pushed": 0}
        self.last = {}   # the last tick's begin and commit results and placed items, the whole batch

    def enqueue(self, c, size, channel=0, mode=E.RELIABLE):
        p, _ = E.pkt(size, channel, mode, flush_id=self.flush_id, offset=self.arena_len)
        self.arena_len += size
        self.backlog[c].append(p)
        self.models[c].queue.append(p)

    def spread(self, values, idle, dtype):
        """One value per modelled connection (or one for all) as one per connection of the batch."""
        values = np.broadcast_to(np.asarray(values, dtype=dtype), (self.n,))
        out = np.full(self.total, idle, dtype=dtype)
        out[self.active] = values[self.src[self.active]]
        return out

    def tick(self, now_ms, rtt_ms, flush_alloc, acks, flags=None, take=None):
        """acks[c]: [(frame_window_base_id, packet_window_base_id, [(base_id, bitfield, nonce)])] in arrival order.
        flush_alloc: one value or one per connection.  Returns the frames each connection sent, from the batched
        calls: [[(frame id, [(seq, fragment)])]], after every record was compared with the model's."""
        n, total_n, be, src = self.n, self.total, self.backend, self.src
        self.now_ms = now_ms
        self.flush_id = (self.flush_id + 1) & 0xFFFFFFFF
        flush_alloc = np.broadcast_to(np.asarray(flush_alloc, dtype=np.int64), (n,))
        flags = np.zeros(n, dtype=np.uint32) if flags is None else np.asarray(flags, dtype=np.uint32)
        # the ack frames
        infos, groups = [], []
        frame_count = np.zeros(total_n, dtype=np.uint64)
        for c in self.active:
            for fw, pw, gs in acks[src[c]]:
                info = Q.ack_info(fw, len(groups), len(gs))
                info["f"][1] = pw
                infos.append(info)
                groups.extend(Q.group_item(*g) for g in gs)
            frame_count[c] = len(acks[src[c]])
        infos = np.array(infos, dtype=fr.FRAME_INFO_DTYPE) if infos else np.zeros(0, fr.FRAME_INFO_DTYPE)
        groups = np.array(groups, dtype=fr.ITEM_DTYPE) if groups else np.zeros(0, fr.ITEM_DTYPE)
        frame_first = np.zeros(total_n + 1, dtype=np.uint64)
        frame_first[1:] = np.cumsum(frame_count, dtype=np.uint64)
        thresh = max(now_ms - 4 * rtt_ms, 0)
        steps = np.zeros(total_n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
        steps["flags"] = np.uint32(fr.FQ_FORGET | fr.FQ_HAS_RTT) | self.extra
        steps["rtt_ms"], steps["thresh_ms"], steps["now_ms"] = rtt_ms, thresh, now_ms
        # the model, as the reference interleaves it
        logs = []
        for c, m in enumerate(self.models):
            m.freed = m.bytes_freed = m.ignored = m.refs_acked = 0
            m.alive_at_tick = set(m.pk.values())
            for fw, pw, gs in acks[c]:
                m.handle_ack_frame(fw, pw, gs, rtt_ms)
            m.fq.forget_frames(thresh, rtt_ms)
            logs.append(m.flush(now_ms, rtt_ms, self.flush_id, int(flush_alloc[c]), no_flush=bool(flags[c] & 1)))
        flush_alloc, flags = self.spread(flush_alloc, 0, np.int64), self.spread(flags, 0, np.uint32)
        # the batched calls
        fq_res = be.frame_queue(infos, groups, frame_first, self.sent, self.sent_first, self.queues, steps, self.log,
                                self.arenas["ref_acked"])
        assert (fq_res["stop"] == fr.FQ_DONE).all() and (fq_res["pushes_refused"] == 0).all()
        if any(marked_refs_of_lane(self.states[c], self.arenas["ref_acked"]) for c in range(n)):
            self.seen.add("ref_acked_lane_63")
        rate = np.zeros(total_n, dtype=fr.RATE_RESULT_DTYPE)
        rate["now_ms"], rate["rtt_ms"] = now_ms, rtt_ms
        flushes = np.zeros(total_n, dtype=fr.FLUSH_DTYPE)
        flushes["flush_alloc"], flushes["kind"] = flush_alloc, fr.DATA
        flushes["window_room"], flushes["id0"] = fq_res["window_room"], self.queues["log_next_id"]
        self.senders["flush_id"] = self.flush_id
        self.senders["take"] = self.spread(0xFFFFFFFF if take is None else take, 0xFFFFFFFF, np.uint32)
        self.senders["reserve_items"] = 0
        begin = be.resend_begin(infos, frame_first, self.queues, self.log, rate, flushes, self.states, self.senders,
                                self.arenas, flags)
        packets = [p for c in self.active for p in self.backlog[src[c]]]
        packets = np.array(packets, dtype=fr.PACKET_DTYPE) if packets else np.zeros(0, fr.PACKET_DTYPE)
        packet_count = np.zeros(total_n, dtype=np.uint64)
        packet_count[self.active] = [len(self.backlog[src[c]]) for c in self.active]
        packet_first = np.zeros(total_n + 1, dtype=np.uint64)
        packet_first[1:] = np.cumsum(packet_count, dtype=np.uint64)
        pre = self.senders.copy()
        total = int(self.senders["reserve_items"].sum()) + sum(E.fragments(int(p["data_len"])).__len__() for p in packets)
        items = E.filled_items(total + 4)
        items, flush_first, packet_results, sender_results, _, used = be.emit(packets, packet_first, self.senders, items)
        assert int(used) <= items.size
        be.resend_place(self.states, begin, self.arenas, flush_first, items)
        frames, flush_results, frames_used = be.pack(items[:int(used)], flush_first, flushes)
        frames = frames[:frames_used]
        out_offsets = be.build_sizes(frames, items[:int(used)])
        before = self.states.copy()
        r = be.resend_commit(flush_results, frames, out_offsets, frames_used, items[:int(used)], flush_first, packets,
                             packet_first, packet_results, sender_results, begin, rate, self.states, pre, self.arenas,
                             next_extra_flags=self.extra, states_out=self.states)
        commit, retake, self.sent, self.sent_first = r["results"], r["retake"], r["sent"][:frames_used], r["sent_first"]
        self.extra = r["next_extra_flags"]
        sr2, self.senders = be.emit_state(packets, packet_first, retake)
        # (a replica shares its connection's backlog, so it must have consumed as many; an idle filler does nothing)
        taken = sr2["packets_consumed"].astype(np.int64)
        assert np.array_equal(taken[self.active], taken[src[self.active]]), "a replica consumed another count"
        idle = src < 0
        assert not taken[idle].any() and not begin["n_resent"][idle].any() and not commit["frames"][idle].any()
        for fld, res in (("packets_freed", begin), ("refs_acked", begin), ("n_resent", begin), ("heap_pushed", commit)):
            self.pad_totals[fld] += int(res[fld][n:].sum())
        self.last = {"begin": begin, "commit": commit, "items": items, "flush_first": flush_first,
                     "window_room": fq_res["window_room"] - flush_results["frame_count"]}   # (what is left of it)
        out = []
        for c in range(n):
            consumed = int(sr2[c]["packets_consumed"])
            del self.backlog[c][:consumed]
            out.append(self.compare(c, logs[c], begin[c], commit[c], before[c], flush_results[c], frames, items, out_offsets,
                                    consumed, flags[c]))
        self.check_guards()
        return out

    # ---- the comparison ----
    def region(self, c, name, key):
        s = self.states[c]
        a = int(s[name + "_first"])
        return self.arenas[key][a: a + int(s[name + "_cap"])]

    def compare(self, c, log, b, cm, before, fres, frames, items, out_offsets, consumed, flag):
        m, s, sd = self.models[c], self.states[c], self.senders[c]
        what = f"connection {c}"
        self.seen_stops.add(int(b["stop"]))
        self.seen_stops.add(int(cm["stop"]))
        # begin's result
        assert int(b["stop"]) == log.loop_stop, (what, STOP_NAMES[int(b["stop"])], STOP_NAMES[log.loop_stop])
        for fld, want in (("n_resent", log.n_resent), ("n_pending_staged", log.pending_staged),
                          ("heap_popped_dead", log.dead), ("heap_popped_acked", log.acked), ("packets_freed", m.freed),
                          ("bytes_freed", m.bytes_freed), ("acks_ignored", m.ignored), ("refs_acked", m.refs_acked)):
            assert int(b[fld]) == want, (what, fld, int(b[fld]), want)
        # commit's result
        assert int(cm["stop"]) == (HEAP_FULL if log.dropped else DONE), (what, int(cm["stop"]), log.dropped)
        for fld, want in (("pending_packed", log.pending_packed), ("packets_entered", log.entered),
                          ("heap_pushed", log.pushed), ("heap_dropped", log.dropped), ("frames", len(log.frames)),
                          ("heap_len", len(m.heap)), ("pending_count", len(m.pending))):
            assert int(cm[fld]) == want, (what, fld, int(cm[fld]), want)
        assert consumed == log.consumed, (what, "packets consumed", consumed, log.consumed)
        assert int(fres["alloc_left"]) == log.alloc_left, (what, "alloc_left", int(fres["alloc_left"]), log.alloc_left)
        assert bool(self.extra[c] & fr.FQ_MARK_RATE_LIMITED) == log.size_limited, (what, "rate-limited mark")
        # the sender
        want = np.zeros((), dtype=fr.SENDER_DTYPE)
        m.tx.to_record(want)
        for fld in ("base_id", "next_id", "window_size", "alloc", "max_alloc", "window_parent_id", "channel_parent_id"):
            assert np.array_equal(sd[fld], want[fld]), (what, fld, sd[fld], want[fld])
        assert int(s["window_bytes"]) == m.window_bytes, (what, "window_bytes")
        # the heap, byte for byte
        heap = self.region(c, "heap", "heap")
        assert int(s["heap_len"]) == len(m.heap)
        exp = np.zeros(len(m.heap), dtype=fr.RESEND_ENTRY_DTYPE)
        for i, e in enumerate(m.heap.d):
            exp[i] = (e.resend_time, e.packet.seq, e.fragment_id, e.send_count, 0)
        assert heap[:len(exp)].tobytes() == exp.tobytes(), (what, "heap", heap[:len(exp)], exp)
        # the pending queue
        assert int(s["pending_count"]) == len(m.pending)
        if m.pending:
            p, f, resend = m.pending[0]
            assert (int(s["pending_seq"]), int(s["pending_next"]), int(s["pending_resend"])) == (p.seq, f, int(resend)), what
            assert [x[1] for x in m.pending] == list(range(f, p.last + 1)) and all(x[0] is p for x in m.pending)
        else:
            assert (int(s["pending_seq"]), int(s["pending_next"]), int(s["pending_resend"])) == (0, 0, 0), what
        # the packet table and the ack bytes
        pk, fa = self.region(c, "pkt", "pkts"), self.region(c, "frag", "frag_acked")
        frag_next = int(before["frag_next"])
        assert set(m.pk) == {(int(sd["base_id"]) + k) & ID_MASK for k in range(E.sub(int(sd["next_id"]), int(sd["base_id"])))}
        for seq in sorted(m.pk, key=lambda v: E.sub(v, int(sd["base_id"]))):
            p = m.pk[seq]
            k = pk[seq & (pk.size - 1)]
            if p.frag_first is None:   # entered in this tick: its ack bytes come from frag_next, in order
                p.frag_first = frag_next
                frag_next = (frag_next + p.last + 1) & 0xFFFFFFFF
            got = tuple(int(k[f]) for f in ("data_offset", "data_len", "frag_first", "sequence_id", "window_parent_lead",
                                            "channel_parent_lead", "channel_id", "resend", "reserved"))
            assert got == (int(p.rec["data_offset"]), p.size, p.frag_first, seq, p.wl, p.cl, int(p.rec["channel_id"]),
                           int(p.resend), 0), (what, "packet", seq, got)
            flags_got = [int(fa[(p.frag_first + f) & (fa.size - 1)]) for f in range(p.last + 1)]
            assert flags_got == [int(v) for v in p.acked], (what, "ack bytes", seq, flags_got)
        assert int(s["frag_next"]) == frag_next, (what, "frag_next")
        if frag_next - int(before["frag_next"]) and (frag_next & (fa.size - 1)) < (int(before["frag_next"]) & (fa.size - 1)):
            self.seen.add("frag_wrap")
        # the frames: items, sizes, refs and sent records
        f0, fc = int(fres["frame_first"]), int(fres["frame_count"])
        assert fc == len(log.frames) and int(self.sent_first[c]) == f0
        head, cap, tx_first = int(before["tx_head"]), int(s["tx_cap"]), int(s["tx_first"])
        out = []
        for k, (fid, size, frags) in enumerate(log.frames):
            g = f0 + k
            info, rec = frames[g], self.sent[g]
            assert int(info["f"][0]) == fid and int(info["item_count"]) == len(frags), (what, "frame", k)
            its = items[int(info["item_first"]): int(info["item_first"]) + len(frags)]
            for it, (seq, f, resend) in zip(its, frags):
                assert it == m.pk[seq].items[f], (what, "item record", k, it, m.pk[seq].items[f])
            if (head & (cap - 1)) + len(frags) > cap:
                head += cap - (head & (cap - 1))
                self.seen.add("tx_skip")
            ref_first = tx_first + (head & (cap - 1))
            assert int(out_offsets[g + 1] - out_offsets[g]) == size, (what, "frame size", k)
            assert (int(rec["send_time_ms"]), int(rec["size"]), int(rec["ref_first"]), int(rec["ref_count"]), int(rec["flags"])) \
                    == (self.now_ms, size, ref_first, len(frags), 0), (what, "sent record", k, rec)
            refs = self.arenas["tx"][ref_first: ref_first + len(frags)]
            assert [(int(r["sequence_id"]), int(r["fragment_id"]), int(r["flags"])) for r in refs] == \
                [(seq, f, int(resend)) for seq, f, resend in frags], (what, "refs", k)
            head = (head + len(frags)) & 0xFFFFFFFF
            out.append((fid, [(seq, f) for seq, f, _ in frags]))
        assert int(s["tx_head"]) == head, (what, "tx_head")
        if (head & (cap - 1)) < (int(before["tx_head"]) & (cap - 1)):
            self.seen.add("tx_wrap")
        # the frame queue both sides ran
        q = self.queues[c]
        assert (int(q["log_next_id"]) + fc) & 0xFFFFFFFF == m.fq.next_id(), (what, "frame ids")
        for name, cond in (("dead_pop", log.dead), ("acked_pop", log.acked), ("resent", log.n_resent),
                           ("partial_packet", len(m.pending) and m.pending[0][1] > 0), ("hang", log.loop_stop == REF_HANG),
                           ("pending_packed", log.pending_packed), ("id_wrap", int(sd["next_id"]) < int(sd["base_id"]))):
            if cond:
                self.seen.add(name)
        return out

    def check_guards(self):
        """Nothing outside the connections' regions was written, the padding's regions included: the regions stay
        where they were laid out, and the record before and the record behind each (all there is between them) are as
        they were."""
        for name in ("heap", "pkt", "frag", "tx", "stage"):
            for fld in (name + "_first", name + "_cap"):
                assert np.array_equal(self.states[fld], self.layout[fld]), ("a region moved", fld)
        for k, v in self.arenas.items():
            assert np.array_equal(v[self.guard_at[k]], self.guard[k]), ("wrote outside a region", k)


# ---- a lossy link and its peer ----
class Link:
    """A receiver that acknowledges what it got: every frame in a group of its own (nonce 0), the frame window's base
    behind the highest frame seen, and the packet window's base at the first packet the sender still has to deliver (a
    packet it will never resend counts as skipped, as after a sync frame).  Frames are dropped at random."""

    def __init__(self, rng, pipeline, c, loss):
        self.rng, self.p, self.c, self.loss = rng, pipeline, c, loss
        self.got = {}        # packet object -> set of fragments received
        self.delivered = []  # (seq, channel) of resend packets, in completion order
        self.frame_base = pipeline.cfg[c].frame_base

    def deliver(self, frames):
        """frames: [(frame id, [(seq, fragment)])] just sent.  Returns the ack frames that come back."""
        m = self.p.models[self.c]
        acks = []
        for fid, frags in frames:
            if self.rng.random() < self.loss:
                continue
            for seq, f in frags:
                p = m.pk.get(seq)
                if p is not None:
                    self.got.setdefault(p, set()).add(f)
            if ((fid - self.frame_base) & 0xFFFFFFFF) < (1 << 31):
                self.frame_base = (fid + 1) & 0xFFFFFFFF
            acks.append((fid, 1, 0))
        if not acks:
            return []
        base = m.tx.base_id
        while base != m.tx.next_id:
            p = m.pk[base]
            if p.resend and len(self.got.get(p, ())) != p.last + 1:
                break
            if m.pending and m.pending[0][0] is p:   # (not past a packet that is still being sent: the hang)
                break
            base = (base + 1) & ID_MASK
        return [(self.frame_base, base, [(a[0], a[1], a[2])]) for a in acks[:-1]] + \
               [(self.frame_base, base, [acks[-1]])]


def run_lossy(pipeline, rng, ticks, loss=0.25, rtt_ms=40, tick_ms=25, alloc=(3000, 12000), traffic=None, hostile=0.0,
              hostile_from=0, start_ms=1000):
    """Generated traffic over a lossy link for `ticks` ticks; every tick is compared inside Pipeline.tick."""
    n = pipeline.n
    losses = loss if isinstance(loss, (list, tuple)) else [loss] * n
    crng = [random.Random(rng.getrandbits(64)) for _ in range(n)]   # (one stream per connection)
    links = [Link(crng[c], pipeline, c, losses[c]) for c in range(n)]
    acks = [[] for _ in range(n)]
    now = start_ms
    for t in range(ticks):
        fa = []
        for c in range(n):
            r = crng[c]
            for size, ch, mode in (traffic(r, t, c) if traffic else default_traffic(r, t, c)):
                pipeline.enqueue(c, size, ch, mode)
            if hostile and t >= hostile_from and r.random() < hostile and pipeline.models[c].pending:
                m = pipeline.models[c]
                acks[c].append((m.fq.base_id(), m.tx.next_id, []))   # the ack the reference hangs on
            fa.append(r.choice((-5, 0, r.randrange(*alloc), r.randrange(*alloc), 1 << 30)))
        sent = pipeline.tick(now, rtt_ms, fa, acks)
        acks = [links[c].deliver(sent[c]) for c in range(n)]
        now += tick_ms
    pipeline.next_acks, pipeline.next_ms = acks, now   # (what the next tick would get)
    return links


def default_traffic(rng, t, c):
    out = []
    for _ in range(rng.randrange(0, 4)):
        kind = rng.random()
        size = rng.randrange(0, 200) if kind < 0.5 else rng.randrange(1000, 3100) if kind < 0.9 else rng.randrange(4000, 9000)
        out.append((size, rng.randrange(3), rng.choice((E.TIME_SENSITIVE, E.UNRELIABLE, E.PERSISTENT, E.RELIABLE, E.RELIABLE))))
    return out


# ---- the hand-traced cases of tests/golden/resend_cases.json ----
def run_golden(case, backend=None):
    """Runs one case's ticks through a Pipeline (which compares every tick with the model) and holds what the batched
    calls gave against the case's own expectations, traced by hand from the reference."""
    cfg = Config(**case.get("config", {}))
    p = Pipeline([cfg], backend)
    for k, t in enumerate(case["ticks"]):
        for _ in range(t.get("repeat_enqueue", 1)):
            for size, ch, mode in t.get("enqueue", []):
                p.enqueue(0, size, ch, mode)
        acks = [[(fw, pw, [tuple(g) for g in gs]) for fw, pw, gs in t.get("acks", [])]]
        before_heap = p.region(0, "heap", "heap")[:int(p.states[0]["heap_len"])].copy()
        p_begin = {}
        orig = p.backend.resend_begin

        def spy(*a, **kw):
            r = orig(*a, **kw)
            p_begin["r"] = r.copy()
            return r

        p.backend.resend_begin = spy
        try:
            frames = p.tick(t["now"], t["rtt"], t["alloc"], acks, flags=[t.get("flags", 0)])[0]
        finally:
            p.backend.resend_begin = orig
        e, b, what = t["expect"], p_begin["r"][0], (case["name"], "tick", k)
        assert [[list(x) for x in fr_] for _, fr_ in frames] == e["frames"], (what, frames)
        assert STOP_NAMES[int(b["stop"])] == e.get("stop", "DONE"), (what, STOP_NAMES[int(b["stop"])])
        for fld in ("n_resent", "heap_popped_dead", "heap_popped_acked", "packets_freed", "acks_ignored"):
            if fld in e:
                assert int(b[fld]) == e[fld], (what, fld, int(b[fld]))
        s = p.states[0]
        if "heap_len" in e:   # (after the tick)
            assert int(s["heap_len"]) == e["heap_len"], (what, "heap_len", int(s["heap_len"]))
        heap = p.region(0, "heap", "heap")[:int(s["heap_len"])]
        if "heap" in e:
            got = [[int(h["resend_time_ms"]), int(h["sequence_id"]), int(h["fragment_id"]), int(h["send_count"])] for h in heap]
            assert got == e["heap"], (what, "heap", got)
        if e.get("heap_untouched"):
            assert heap.tobytes() == before_heap.tobytes(), (what, "heap touched")
        if "pending" in e:
            assert [int(s["pending_seq"]), int(s["pending_next"]), int(s["pending_count"])] == e["pending"], what
        if "base_id" in e:
            assert int(p.senders[0]["base_id"]) == e["base_id"], what
        if "backlog" in e:
            assert len(p.backlog[0]) == e["backlog"], (what, "backlog", len(p.backlog[0]))
        if "leads" in e:
            got = []
            for seq in sorted(p.models[0].pk):
                k_ = p.region(0, "pkt", "pkts")[seq & (int(s["pkt_cap"]) - 1)]
                got.append([seq, int(k_["channel_id"]), int(k_["window_parent_lead"]), int(k_["channel_parent_lead"]), int(k_["resend"])])
            assert got == e["leads"], (what, "leads", got)
    return p
