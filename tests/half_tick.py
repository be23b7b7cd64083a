"""A tick driver that replays the reference's own HalfConnection tests (src/half_connection/mod.rs:633-1038, as data in
tests/golden/half_connection_cases.json) through the batched stages (test infrastructure, not a test module).

`HalfTick` runs emit_frames(now_ms, rtt_ms, flush_alloc) for a batch of n connections as the library's calls, in the
reference's order (mod.rs:217-232), the way the test apparatus calls it (mod.rs:565-573): directly, never through
step().  So there is no forget_frames (no FQ_FORGET), no flush-id increment (the flush id is what set_flush_id set,
else 0), no rate step (the rate result record is filled in: now_ms, rtt_ms, rto_ms = 4 * rtt_ms, flush_alloc), and
flush_alloc is set, not accumulated.  FQ_HAS_RTT is off for receive_ack (handle_ack_frame passes
send_rate_comp.rtt_ms(), None in every case) and on, with the step's rtt_ms, for acknowledge_frame_group.

A tick, for every connection at once:
  receive side   frame_window -> receive_packets over the pending receive_ack / receive_sync frames, as frame infos
                 and group items built directly (a sync that carries a packet id sets the receiver's resync id first);
                 acknowledge_packet_base_id(b) is an ack frame {0, b, no groups}, acknowledge_frame_group an ack frame
                 with that one group and both base ids 0 (tests/golden/resend_cases.json maps them the same way);
  sender side    frame_queue | flush_acks -> build_sizes -> build | resend_begin -> emit_packets -> resend_place ->
                 pack -> build_sizes -> resend_commit -> emit_packets (retake) -> build | flush_sync -> build_sizes ->
                 build, wired as INTEGRATION.md says: window_room and id0 into the flush records, the ack flush's
                 flush_alloc and UFC_RS_NO_DATA_FLUSH into the data flush, the ack flush's, begin's, the pack's and
                 commit's results into the sync call, consumed packets leaving the backlog.
What every connection emitted comes back in the reference's sink order (ack frames, data frames, the sync frame) as
wire bytes read by fr.Frame.read, every frame's CRC checked with the oracle.

Every connection has its own scenario, clock and step index.  A connection whose scenario has not begun, or is over
(and a filler, which has none), is ticked with its first or last now_ms, no input and flush_alloc 0, and must emit
nothing: the elapsed time is below every timeout (mod.rs:235-238), nothing is due before the next resend time
(resend_timing) and a repeated call emits nothing more (keepalive_timing, mod.rs:956).

The driver asserts the fixture's expectations and that idle rule, and that no stage stopped on a capacity or a bad
state.  It consults no model: not flush_expect, not resend_expect's HalfTx, nor any other.  From resend_expect it takes
HostBackend, the calls of the resend tick on host arrays; `HostCalls` adds the calls the whole tick needs, and
`DeviceCalls` has the same methods on device tensors, queued with nothing read back (test_gpu_resend.GpuBackend, which
reads back after every call, does not fit a tick that is read back once)."""
import json
import os

import numpy as np

import oracle
from uflow_amd import flush as fl, frame as fr
from uflow_amd._native import check, lib
from resend_expect import HostBackend

U8, U32, U64 = np.uint8, np.uint32, np.uint64
NONE = 0xFFFFFFFF
MODES = {"TimeSensitive": fr.SEND_TIME_SENSITIVE, "Unreliable": fr.SEND_UNRELIABLE, "Persistent": fr.SEND_PERSISTENT,
         "Reliable": fr.SEND_RELIABLE}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "half_connection_cases.json")

# One payload arena for every connection: the index pattern (byte i = i mod 256) from offset 0, then a run of each
# constant byte the cases use.  A packet's data_offset points into its pattern.
INDEX_LEN, CONST_LEN, CONST_BYTES = 4096, 1448, 8
PAYLOAD = np.concatenate([np.arange(INDEX_LEN, dtype=np.uint32).astype(U8)] +
                         [np.full(CONST_LEN, b, dtype=U8) for b in range(CONST_BYTES)])


def fill_offset(fill):
    return 0 if fill == "index_u8" else INDEX_LEN + CONST_LEN * int(fill)


def fill_bytes(fill, offset, length):
    if fill == "index_u8":
        return bytes((offset + i) & 0xFF for i in range(length))
    return bytes([int(fill)]) * length


def load_cases():
    with open(FIXTURE) as f:
        doc = json.load(f)
    return doc, {c["name"]: c for c in doc["cases"]}


class Scenario:
    """A case as ticks: [(the steps in front of an emit_frames step, that step)], loops unrolled (by reference)."""

    def __init__(self, case, repeat_limit=None):
        self.name = case["name"]
        flat = []

        def walk(steps):
            for s in steps:
                if s["op"] == "repeat":
                    for _ in range(min(s["count"], repeat_limit or s["count"])):
                        walk(s["steps"])
                else:
                    flat.append(s)
        walk(case["steps"])
        self.ticks, ops = [], []
        for s in flat:
            if s["op"] == "emit_frames":
                self.ticks.append((ops, s))
                ops = []
            else:
                ops.append(s)
        self.tail_ops = ops   # (steps behind the last emit_frames: they change nothing that is asserted)
        # rooms: what the scenario needs.  The packets a test has outstanding at once are those of its largest loop.
        need = max([s.get("times", 1) for s in flat if s["op"] == "enqueue"] + [1])
        total = sum(s.get("times", 1) for s in case["steps"] if s["op"] == "enqueue")
        self.window = 4096 if max(need, total) > 8 else 16


class Rooms:
    """Capacities of one connection: `window` frames and packets in flight (both windows, the log's tail, the
    receiver), the heap and stage that go with them, the ack carry."""

    def __init__(self, window, idle=False):
        self.window = window
        self.tail = 0 if idle else window
        self.heap_cap = 1 if idle else window + 8
        self.stage_cap = 1 if idle else self.heap_cap + 8
        self.carry_cap = 1 if idle else 4
        self.max_alloc = fr.MAX_FRAGMENT_SIZE * window


IDLE_ROOMS = Rooms(1, idle=True)
ROOMS = {w: Rooms(w) for w in (16, 4096)}


# ---- the calls ----
class HostCalls(HostBackend):
    """resend_expect.HostBackend and the calls of the whole tick it lacks, on host arrays."""

    def up(self, a):
        return np.ascontiguousarray(a).copy()

    def down(self, a, dtype, count=None):
        return a if count is None else a[:count]

    def sync(self):
        pass

    def set_field(self, recs, dtype, name, values):
        recs[name] = values

    def copy_field(self, dst, ddt, dname, src, sdt, sname):
        dst[dname] = src[sname]

    def frame_window(self, infos, frame_first, windows):
        return fr.frame_window_host(infos, frame_first, windows, nthreads=self.nthreads, windows_out=windows)

    def resync(self, window_results, infos, receivers):
        first = window_results["first_packet_sync"]
        has = first != NONE
        receivers["resync_id"] = np.where(has, infos["f"][:, 1][np.where(has, first, 0)], NONE)

    def receive_packets(self, infos, items, frame_first, receivers, slots, slot_first, frame_accept):
        z = np.zeros(0, dtype=U8)
        return fr.receive_packets_host(infos, items, z, frame_first, receivers, slots, slot_first, z,
                                       frame_accept=frame_accept, carry_out=np.zeros(64, dtype=U8),
                                       out_bytes=np.zeros(64, dtype=U8), packets=np.zeros(4, dtype=fr.RX_PACKET_DTYPE),
                                       nthreads=self.nthreads, receivers_out=receivers, want_item_status=False)["results"]

    def flush_acks(self, ctl, windows, groups, group_first, receivers, rate, carry, flushes, flags):
        return fl.flush_acks_host(ctl, windows, groups, group_first, receivers, rate, carry, flushes=flushes, flags=flags,
                                  nthreads=self.nthreads, windows_out=windows, ctl_out=ctl)

    def flush_sync(self, ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders):
        return fl.flush_sync_host(ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders,
                                  nthreads=self.nthreads, ctl_out=ctl)

    def pack(self, items, flush_first, flushes, nonce_bits=None):
        return fr.pack_host(items, flush_first, flushes, nonce_bits=nonce_bits, nthreads=self.nthreads)

    def build(self, infos, items, payload, offsets, out_cap):
        if infos.size == 0:
            return np.zeros(0, dtype=U8)
        out = np.zeros(int(offsets[-1]), dtype=U8)
        assert out.size <= out_cap, ("the driver's bound on the built bytes is too small", out.size, out_cap)
        check(lib().ufc_build_batch_host(infos.ctypes.data, items.ctypes.data if items.size else None, items.size, None,
                                         payload.ctypes.data if payload.size else None, payload.size, infos.size,
                                         offsets.ctypes.data, out.ctypes.data if out.size else None, out.size, 1, None,
                                         self.nthreads), "ufc_build_batch_host")
        return out


class DeviceCalls:
    """HostCalls' methods on device tensors (FrameCrcEngine's), every call queued and nothing read back: down() after
    sync() is the tick's one read back."""

    def __init__(self, engine):
        import torch
        from uflow_amd.batch import records, rows
        self.e, self.torch, self.records, self.rows = engine, torch, records, rows
        self.dev = engine.device

    def up(self, a):
        return self.rows(a, self.dev)

    def down(self, t, dtype, count=None):
        return self.records(t if count is None else t[:count], dtype)

    def sync(self):
        self.torch.cuda.synchronize()

    @staticmethod
    def _col(t, dtype, name):
        dt, off = dtype.fields[name][:2]
        return t[:, off: off + dt.itemsize]

    def set_field(self, recs, dtype, name, values):
        dt = dtype.fields[name][0]
        v = np.array(np.broadcast_to(np.asarray(values).astype(dt), (recs.shape[0],)))   # (a writable copy)
        self._col(recs, dtype, name).copy_(self.torch.from_numpy(v.view(U8).reshape(-1, dt.itemsize)).to(self.dev))

    def copy_field(self, dst, ddt, dname, src, sdt, sname):
        self._col(dst, ddt, dname).copy_(self._col(src, sdt, sname))

    def frame_window(self, infos, frame_first, windows):
        return self.e.frame_window(infos, frame_first, windows, windows_out=windows)

    def resync(self, window_results, infos, receivers):
        torch, i32 = self.torch, (lambda x: x.view(self.torch.int32))
        first = i32(window_results)[:, 6].to(torch.int64)   # first_packet_sync, -1: none
        ids = i32(infos)[first.clamp(min=0), 2]              # its next_packet_id
        i32(receivers)[:, 4] = torch.where(first >= 0, ids, torch.full_like(ids, -1))

    def receive_packets(self, infos, items, frame_first, receivers, slots, slot_first, frame_accept):
        z = lambda k, w=None: self.torch.zeros((k, w) if w else k, dtype=self.torch.uint8, device=self.dev)  # noqa: E731
        return self.e.receive_packets(infos, items, z(0), frame_first, receivers, slots, slot_first, z(0),
                                      frame_accept=frame_accept, carry_out=z(64), out_bytes=z(64),
                                      packets=z(4, fr.RX_PACKET_DTYPE.itemsize), receivers_out=receivers,
                                      want_item_status=False)["results"]

    def frame_queue(self, infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked):
        return self.e.frame_queue(infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked,
                                  queues_out=queues)["results"]

    def flush_acks(self, ctl, windows, groups, group_first, receivers, rate, carry, flushes, flags):
        return self.e.flush_acks(ctl, windows, groups, group_first, receivers, rate, carry, flushes=flushes, flags=flags,
                                 windows_out=windows, ctl_out=ctl)

    def flush_sync(self, ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders):
        return self.e.flush_sync(ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders,
                                 ctl_out=ctl)

    def resend_begin(self, infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags):
        return self.e.resend_begin(infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags=flags,
                                   states_out=states, senders_out=senders)["results"]

    def emit(self, packets, packet_first, senders, items):
        return self.e.emit_packets(packets, packet_first, senders, items.shape[0], items=items)

    def emit_state(self, packets, packet_first, senders):
        out = self.e.emit_packets(packets, packet_first, senders, 0)
        return out[3], out[4]

    def resend_place(self, states, begin_results, arenas, flush_first, items):
        self.e.resend_place(states, begin_results, {"stage": arenas["stage"]}, flush_first, items)

    def pack(self, items, flush_first, flushes, nonce_bits=None):
        return self.e.pack_flushes(items, flush_first, flushes, nonce_bits=nonce_bits)

    def build_sizes(self, infos, items):
        return self.e.build_sizes_varlen(infos, items, 1 << 40)[0]

    def resend_commit(self, *args, **kw):
        return self.e.resend_commit(*args, **kw)

    def build(self, infos, items, payload, offsets, out_cap):
        import ctypes
        out = self.torch.zeros(max(int(out_cap), 1), dtype=self.torch.uint8, device=self.dev)
        n = infos.shape[0]
        if n == 0:
            return out
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
        stream = ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        check(lib().ufc_build_batch_varlen(self.e._ctx, P(infos), P(items), items.shape[0], None, P(payload), payload.numel(),
                                           n, P(offsets), P(out), out.numel(), 1, None, stream), "ufc_build_batch_varlen")
        return out


# ---- the driver ----
class Conn:
    def __init__(self, index, scenario, start):
        self.index, self.sc, self.start = index, scenario, start
        self.step = 0
        self.flush_id = 0
        self.backlog = np.zeros(0, dtype=fr.PACKET_DTYPE)   # enqueued and not yet consumed
        self.emits = {}             # an emit step's id -> the frames of its latest run
        self.datagrams_seen = 0

    def now_idle(self):
        ticks = self.sc.ticks
        return ticks[0][1]["args"][0] if self.step == 0 else ticks[self.step - 1][1]["args"][0]


def _layout(caps):
    caps = np.asarray(caps, dtype=U64)
    ends = np.cumsum(caps, dtype=U64)
    return ends - caps, int(ends[-1]) if caps.size else 0


class HalfTick:
    """assign: one (Scenario or None, first tick) per connection; None is an idle filler.  run() ticks until every
    scenario is over (and `extra` ticks more), asserting every expectation of the fixture and the idle rule."""

    def __init__(self, assign, backend=None, keepalive_ms=5000, seed=1):
        be = self.be = backend or HostCalls()
        n = self.n = len(assign)
        self.conns = [Conn(c, sc, start) for c, (sc, start) in enumerate(assign) if sc is not None]
        self.rng = np.random.default_rng(seed)
        self.t = 0
        rooms = [IDLE_ROOMS] * n
        for k in self.conns:
            rooms[k.index] = ROOMS[k.sc.window]
        # one record of each kind per distinct room, then every connection's copy
        kinds = {}
        for r in set(rooms):
            sender = np.zeros(1, dtype=fr.SENDER_DTYPE)
            sender["window_size"], sender["max_alloc"] = r.window, r.max_alloc
            sender["window_parent_id"], sender["channel_parent_id"] = NONE, NONE
            kinds[r] = (sender[0], fr.new_frame_queues(1, r.window, r.tail, 0)[0][0],
                        fr.new_resend_states(1, r.window, r.max_alloc, r.window, r.tail, r.heap_cap, stage_cap=r.stage_cap)[0][0],
                        fr.new_receivers(1, r.window, 0, r.max_alloc)[0], fl.new_flush_ctl(1, keepalive_ms, r.carry_cap)[0][0])
        senders, queues, states, receivers, ctl = (np.array([kinds[r][k] for r in rooms]) for k in range(5))
        queues["log_first"], log_len = _layout(queues["log_cap"])
        sizes = {}
        for name, key in (("heap", "heap"), ("pkt", "pkts"), ("frag", "frag_acked"), ("tx", "tx"), ("stage", "stage")):
            states[name + "_first"], sizes[key] = _layout(states[name + "_cap"])
        sizes["ref_acked"] = sizes["tx"]
        ctl["carry_first"], carry_len = _layout(ctl["carry_cap"])
        slot_first = np.zeros(n + 1, dtype=U64)
        slot_first[1:] = np.cumsum(receivers["window_size"], dtype=U64)
        self.stage_total = int(states["stage_cap"].sum())
        up = be.up
        self.senders, self.queues, self.states, self.receivers, self.ctl = (up(a) for a in (senders, queues, states, receivers, ctl))
        self.windows = up(fr.new_frame_windows(n, 4096, 0))
        self.log = up(np.zeros(log_len, dtype=fr.SENT_FRAME_DTYPE))
        self.arenas = {k: up(np.zeros(sizes[k], dtype=dt)) for k, dt in fr.RESEND_ARENAS}
        self.carry = up(np.zeros(carry_len, dtype=fr.ITEM_DTYPE))
        self.slots, self.slot_first = up(np.zeros(int(slot_first[-1]), dtype=fr.RX_SLOT_DTYPE)), up(slot_first)
        self.sent, self.sent_first = up(np.zeros(0, dtype=fr.SENT_FRAME_DTYPE)), up(np.zeros(n + 1, dtype=U64))
        self.payload = up(PAYLOAD)
        self.extra = np.zeros(n, dtype=U32)   # FQ_MARK_RATE_LIMITED for the next tick, read back with the tick
        self.frames_total = 0

    # ---- a scenario's steps in front of emit_frames ----
    def value(self, k, v):
        if not isinstance(v, dict):
            return v
        if v["from"] == "datagrams_seen":
            return k.datagrams_seen
        frames = k.emits[v["id"]]
        if "xor_nonce_of_frames" in v:
            x = 0
            for j in v["xor_nonce_of_frames"]:
                x ^= int(frames[j].nonce)
            return x
        return getattr(frames[v["frame"]], v["field"])

    def apply(self, k, s, acks):
        """acks: the connection's frames of this tick, [(kind, a, b, groups, rtt_ms or None)]."""
        op, a = s["op"], s.get("args")
        if op == "enqueue":
            size, channel, mode, fill = a
            p = np.zeros(s.get("times", 1), dtype=fr.PACKET_DTYPE)
            p["data_offset"], p["data_len"], p["channel_id"], p["mode"] = fill_offset(fill), size, channel, MODES[mode]
            k.backlog = np.concatenate([k.backlog, p])   # flush_id 0: the connection's own never moves (mod.rs:125)
        elif op == "set_flush_id":
            k.flush_id = a[0]
        elif op == "receive_ack":
            acks.append((fr.ACK, self.value(k, a[0]), self.value(k, a[1]), [[self.value(k, x) for x in g] for g in a[2]], None))
        elif op == "receive_sync":
            acks.append((fr.SYNC, a[0], a[1], [], None))
        elif op == "acknowledge_packet_base_id":
            acks.append((fr.ACK, 0, a[0], [], None))
        elif op == "acknowledge_frame_group":
            acks.append((fr.ACK, 0, 0, [[a[0], a[1], self.value(k, a[2])]], a[3]))
        else:
            raise AssertionError(op)

    # ---- one tick of the whole batch ----
    def tick(self):
        be, n = self.be, self.n
        now, rtt, alloc = np.zeros(n, dtype=U64), np.full(n, 150, dtype=U64), np.zeros(n, dtype=np.int64)
        flush_id, has_rtt = np.zeros(n, dtype=U32), np.zeros(n, dtype=bool)
        frame_count, packet_count = np.zeros(n, dtype=U64), np.zeros(n, dtype=U64)
        infos, groups, active = [], [], []
        for k in self.conns:
            c = k.index
            flush_id[c] = k.flush_id
            if self.t < k.start or k.step >= len(k.sc.ticks):
                now[c] = k.now_idle()
            else:
                ops, em = k.sc.ticks[k.step]
                frames = []
                for s in ops:
                    self.apply(k, s, frames)
                flush_id[c] = k.flush_id
                now[c], rtt[c], alloc[c] = em["args"]
                for kind, a, b, gs, g_rtt in frames:
                    f = np.zeros((), dtype=fr.FRAME_INFO_DTYPE)
                    f["kind"], f["ok"], f["crc_ok"] = kind, 1, 1
                    if kind == fr.SYNC:
                        f["aux"] = (1 if a is not None else 0) | (2 if b is not None else 0)
                    f["f"][0], f["f"][1] = a or 0, b or 0
                    f["item_first"], f["item_count"] = len(groups), len(gs)
                    for base_id, bitfield, nonce in gs:
                        g = np.zeros((), dtype=fr.ITEM_DTYPE)
                        g["id"], g["data_offset"], g["channel_id"], g["form"] = base_id, bitfield, int(nonce) & 1, 3
                        groups.append(g)
                    if g_rtt is not None:
                        has_rtt[c] = True
                        assert g_rtt == rtt[c], "acknowledge_frame_group's rtt_ms is the tick's in every case"
                    infos.append(f)
                assert not has_rtt[c] or all(x[4] is not None for x in frames), "one FQ_HAS_RTT a connection and tick"
                frame_count[c] = len(frames)
                active.append((k, em))
            packet_count[c] = k.backlog.size
        infos.append(np.zeros((), dtype=fr.FRAME_INFO_DTYPE))   # (one row no range holds: a frame list is never empty)
        infos = np.array(infos, dtype=fr.FRAME_INFO_DTYPE)
        groups = np.array(groups, dtype=fr.ITEM_DTYPE) if groups else np.zeros(0, dtype=fr.ITEM_DTYPE)
        frame_first, packet_first = np.zeros(n + 1, dtype=U64), np.zeros(n + 1, dtype=U64)
        frame_first[1:], packet_first[1:] = np.cumsum(frame_count, dtype=U64), np.cumsum(packet_count, dtype=U64)
        backlogs = [k.backlog for k in self.conns if k.backlog.size]
        packets = np.concatenate(backlogs) if backlogs else np.zeros(0, dtype=fr.PACKET_DTYPE)
        steps = np.zeros(n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
        steps["flags"] = np.where(has_rtt, U32(fr.FQ_HAS_RTT), U32(0)) | self.extra
        steps["rtt_ms"], steps["now_ms"] = rtt, now
        rate = np.zeros(n, dtype=fr.RATE_RESULT_DTYPE)
        rate["now_ms"], rate["rtt_ms"], rate["rto_ms"], rate["flush_alloc"] = now, rtt, 4 * rtt, alloc
        flushes = np.zeros(n, dtype=fr.FLUSH_DTYPE)
        flushes["flush_alloc"], flushes["kind"] = alloc, fr.DATA
        fragments = (packets["data_len"].astype(np.int64) + fr.MAX_FRAGMENT_SIZE - 1) // fr.MAX_FRAGMENT_SIZE
        items_cap = self.stage_total + int(np.maximum(fragments, 1).sum()) + 4
        data_cap = min(items_cap * fr.MAX_FRAME_SIZE, int((np.maximum(alloc, 0) + 2 * fr.MAX_FRAME_SIZE)[alloc >= 0].sum()))
        nonce_bits = self.rng.integers(0, 1 << 32, (items_cap + 31) // 32 + 1, dtype=U64).astype(U32)

        d_infos, d_groups, d_ff, d_pf, d_packets, d_rate, d_flushes = (
            be.up(a) for a in (infos, groups, frame_first, packet_first, packets, rate, flushes))
        d_flags, d_extra = be.up(np.zeros(n, dtype=U32)), be.up(np.zeros(n, dtype=U32))
        # ---- the receive side ----
        fw = be.frame_window(d_infos, d_ff, self.windows)
        be.resync(fw["results"], d_infos, self.receivers)
        rx = be.receive_packets(d_infos, d_groups, d_ff, self.receivers, self.slots, self.slot_first, fw["frame_accept"])
        # ---- the sender's side ----
        fq = be.frame_queue(d_infos, d_groups, d_ff, self.sent, self.sent_first, self.queues, be.up(steps), self.log,
                            self.arenas["ref_acked"])
        be.copy_field(d_flushes, fr.FLUSH_DTYPE, "window_room", fq, fr.FRAME_QUEUE_RESULT_DTYPE, "window_room")
        be.copy_field(d_flushes, fr.FLUSH_DTYPE, "id0", self.queues, fr.FRAME_QUEUE_DTYPE, "log_next_id")
        a = be.flush_acks(self.ctl, self.windows, fw["groups"], fw["group_first"], self.receivers, d_rate, self.carry,
                          d_flushes, d_flags)
        a_off = be.build_sizes(a["infos"], a["merged"])
        a_cap = 32 * len(a["infos"]) + 16 * len(a["merged"])
        a_wire = be.build(a["infos"], a["merged"], self.payload, a_off, a_cap)
        for name, v in (("flush_id", flush_id), ("take", NONE), ("reserve_items", 0)):
            be.set_field(self.senders, fr.SENDER_DTYPE, name, v)
        br = be.resend_begin(d_infos, d_ff, self.queues, self.log, d_rate, d_flushes, self.states, self.senders, self.arenas,
                             d_flags)
        items, flush_first, pres, sres, _, _ = be.emit(d_packets, d_pf, self.senders,
                                                       be.up(np.zeros(items_cap, dtype=fr.ITEM_DTYPE)))
        be.resend_place(self.states, br, self.arenas, flush_first, items)
        d_frames, fres, frames_used = be.pack(items, flush_first, d_flushes, be.up(nonce_bits))
        d_off = be.build_sizes(d_frames, items)
        cm = be.resend_commit(fres, d_frames, d_off, frames_used, items, flush_first, d_packets, d_pf, pres, sres, br, d_rate,
                              self.states, self.senders, self.arenas, next_extra_flags=d_extra, states_out=self.states)
        self.sent, self.sent_first = cm["sent"], cm["sent_first"]
        sr2, self.senders = be.emit_state(d_packets, d_pf, cm["retake"])
        d_wire = be.build(d_frames, items, self.payload, d_off, data_cap)
        s = be.flush_sync(self.ctl, d_rate, a["results"], br, fres, cm["results"], self.queues, self.senders)
        no_items = be.up(np.zeros(0, dtype=fr.ITEM_DTYPE))
        s_off = be.build_sizes(s["infos"], no_items)
        s_wire = be.build(s["infos"], no_items, self.payload, s_off, 16 * n)
        # ---- the tick's one read back ----
        be.sync()
        down = be.down
        self.extra = down(d_extra, U32)
        got = {"fw": down(fw["results"], fr.FRAME_WINDOW_RESULT_DTYPE), "rx": down(rx, fr.RECEIVER_RESULT_DTYPE),
               "fq": down(fq, fr.FRAME_QUEUE_RESULT_DTYPE), "ack": down(a["results"], fr.FLUSH_RESULT_DTYPE),
               "acks": down(a["ack_results"], fl.FLUSH_ACKS_RESULT_DTYPE), "begin": down(br, fr.RESEND_RESULT_DTYPE),
               "pack": down(fres, fr.FLUSH_RESULT_DTYPE), "commit": down(cm["results"], fr.RESEND_COMMIT_RESULT_DTYPE),
               "emit2": down(sr2, fr.SENDER_RESULT_DTYPE), "sync": down(s["results"], fl.FLUSH_SYNC_RESULT_DTYPE),
               "sync_index": down(s["sync_index"], U32)}
        wires = []
        for off, wire in ((a_off, a_wire), (d_off, d_wire), (s_off, s_wire)):
            off = down(off, U64)
            raw = np.ascontiguousarray(down(wire, U8, int(off[-1])))
            if off.size > 1 and raw.size:
                _, valid = oracle.validate_varlen(raw, off)
                lens = np.diff(off.astype(np.int64))
                assert (valid[lens > 0] == 1).all(), "a built frame fails the oracle's CRC gate"
            wires.append((off, raw.tobytes()))
        self.check_stops(got)
        # ---- consumed packets leave the backlog ----
        for k in self.conns:
            if k.backlog.size:
                k.backlog = k.backlog[int(got["emit2"][k.index]["packets_consumed"]):]
        # ---- what every connection emitted, against the fixture and the idle rule ----
        count = got["ack"]["frame_count"].astype(np.int64) + got["pack"]["frame_count"] + (got["sync_index"] != NONE)
        quiet = np.ones(n, dtype=bool)
        quiet[[k.index for k, _ in active]] = False
        assert not count[quiet].any(), ("an idle connection emitted frames", self.t, np.flatnonzero(quiet & (count > 0))[:8])
        for k, em in active:
            self.check_emit(k, em, self.frames_of(k.index, got, wires))
            k.step += 1
        self.frames_total += int(count.sum())
        self.t += 1
        return got

    def check_stops(self, got):
        assert (got["fw"]["stop"] == fr.FW_DONE).all() and (got["rx"]["stop"] == fr.RX_DONE).all()
        assert (got["fq"]["stop"] == fr.FQ_DONE).all() and not got["fq"]["pushes_refused"].any()
        assert not got["fq"]["groups_bad_nonce"].any() and not got["fq"]["groups_unknown"].any()
        assert (got["acks"]["stop"] == fl.FA_DONE).all() and not got["acks"]["dropped"].any()
        assert np.isin(got["begin"]["stop"], (fr.RS_DONE, fr.RS_SIZE_LIMITED, fr.RS_WINDOW_LIMITED)).all(), got["begin"]["stop"]
        assert (got["commit"]["stop"] == fr.RS_DONE).all() and not got["begin"]["acks_ignored"].any()

    def frames_of(self, c, got, wires):
        """Connection c's frames of this tick in sink order, read from the wire."""
        out = []
        ranges = [(int(got["ack"][c]["frame_first"]), int(got["ack"][c]["frame_count"])),
                  (int(got["pack"][c]["frame_first"]), int(got["pack"][c]["frame_count"])),
                  (int(got["sync_index"][c]), 0 if got["sync_index"][c] == NONE else 1)]
        for (first, cnt), (off, raw) in zip(ranges, wires):
            for g in range(first, first + cnt):
                b = raw[int(off[g]): int(off[g + 1])]
                f = fr.Frame.read(b)
                assert f is not None, ("an emitted frame does not read back", c, g)
                f.length = len(b)
                out.append(f)
        return out

    def check_emit(self, k, em, frames):
        e = em["expect"]
        what = (k.sc.name, "connection", k.index, "emit_frames at line", em["line"], "tick", self.t)
        seen = k.datagrams_seen
        k.datagrams_seen += sum(len(f.datagrams) for f in frames if isinstance(f, fr.DataFrame))
        if "id" in em:
            k.emits[em["id"]] = frames
        assert len(frames) == e["count"], (what, "count", len(frames), e["count"], [type(f).__name__ for f in frames[:8]])
        for x in e.get("frames", []):
            f = frames[x["index"]]
            w = what + ("frame", x["index"], "line", x["line"])
            if x["kind"] == "data":
                assert isinstance(f, fr.DataFrame), (w, f)
                if "sequence_id" in x:
                    assert f.sequence_id == x["sequence_id"], (w, "sequence_id", f.sequence_id)
                if "datagrams" in x:
                    want = [fr.Datagram(d["sequence_id"], d["channel_id"], d["window_parent_lead"], d["channel_parent_lead"],
                                        d["fragment_id"], d["fragment_id_last"], fill_bytes(*d["data"])) for d in x["datagrams"]]
                    assert f.datagrams == want, (w, "datagrams", [(d.sequence_id, d.fragment_id, len(d.data)) for d in f.datagrams])
                if "datagram_count" in x:
                    assert len(f.datagrams) == x["datagram_count"], (w, "datagram_count", len(f.datagrams))
                if "datagram_sequence_ids" in x:
                    ids = [d.sequence_id for d in f.datagrams]
                    assert ids == list(range(seen, seen + len(ids))), (w, "datagram ids", ids[:4], seen)
                if "length" in x:
                    assert f.length == x["length"], (w, "length", f.length)
            elif x["kind"] == "sync":
                assert f == fr.SyncFrame(x["next_frame_id"], x["next_packet_id"]), (w, f)
            elif x["kind"] == "ack":
                want = fr.AckFrame(x["frame_window_base_id"], x["packet_window_base_id"],
                                   [fr.AckGroup(g[0], g[1], bool(g[2])) for g in x["frame_acks"]])
                assert f == want, (w, f)
            else:
                raise AssertionError(x["kind"])

    def run(self, extra=0):
        last = max(k.start + len(k.sc.ticks) for k in self.conns) + extra
        while self.t < last:
            self.tick()
        assert all(k.step == len(k.sc.ticks) for k in self.conns)
        return self
