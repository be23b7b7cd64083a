"""Expected results of the batched packet emit (ufc_emit_packets_host / ufc_emit_packets_varlen), and the cases
both test modules share (test infrastructure, not a test module).

`Tx` restates PacketSender (src/half_connection/packet_sender.rs: new :89-119, emit_packet :149-238, acknowledge
:242-275) and `fragments` PendingPacket::new / datagram (pending_packet.rs:23-42, 84-103) in plain Python, one
packet at a time.  An item's header form and validity come from the codec oracle (oracle/codec.py
`datagram_header`, `datagram_is_valid`).  Nothing of the product is used except the record dtypes.
"""
import random

import numpy as np

from oracle import codec as C
from uflow_amd.frame import ITEM_DTYPE, PACKET_DTYPE, PACKET_RESULT_DTYPE, SENDER_DTYPE, SENDER_RESULT_DTYPE

ID_MASK = 0xFFFFF                        # src/packet_id.rs
MAX_FRAGMENT_SIZE = 1448                 # src/lib.rs:297
MAX_PACKET_SIZE = MAX_FRAGMENT_SIZE * 65536  # src/lib.rs:300
MAX_PACKET_WINDOW_SIZE = 4096
CHANNEL_COUNT = 64
TIME_SENSITIVE, UNRELIABLE, PERSISTENT, RELIABLE = 0, 1, 2, 3  # SendMode, src/lib.rs:304-323
NO_PARENT = 0xFFFFFFFF
DONE, WINDOW_LIMITED, ALLOC_LIMITED, BAD_PACKET, BAD_RANGE = 0, 1, 2, 3, 4
NOT_REACHED, EMITTED, DROPPED = 0, 1, 2
FILL = 0xA5  # the pattern reserved and unused item slots are pre-filled with


def alloc_size(packet_size):  # packet_sender.rs:16-22
    if packet_size > MAX_FRAGMENT_SIZE:
        return (packet_size + MAX_FRAGMENT_SIZE - 1) // MAX_FRAGMENT_SIZE * MAX_FRAGMENT_SIZE
    return packet_size


def sub(a, b):  # packet_id::sub
    return (a - b) & ID_MASK


class Tx:
    """PacketSender without its queue: the queue is the caller's list of packets."""

    def __init__(self, window_size=MAX_PACKET_WINDOW_SIZE, base_id=0, max_alloc=10000):
        self.base_id = self.next_id = base_id
        self.window_size = window_size
        self.window = {}  # sequence id -> (alloc_size, channel_id)
        self.window_parent_id = None
        self.channel_parent_id = [None] * CHANNEL_COUNT
        self.max_alloc_given = max_alloc
        self.max_alloc = min((max_alloc + MAX_FRAGMENT_SIZE - 1) // MAX_FRAGMENT_SIZE * MAX_FRAGMENT_SIZE, 2**64 - 1)  # :100
        self.alloc = 0

    @classmethod
    def from_record(cls, r):
        t = cls(int(r["window_size"]), int(r["base_id"]), int(r["max_alloc"]))
        t.next_id, t.alloc = int(r["next_id"]), int(r["alloc"])
        opt = lambda v: None if int(v) == NO_PARENT else int(v)  # noqa: E731
        t.window_parent_id = opt(r["window_parent_id"])
        t.channel_parent_id = [opt(v) for v in r["channel_parent_id"]]
        return t

    def to_record(self, r):
        """Writes the state into a SENDER_DTYPE record (flush_id, take, reserve_items are the caller's)."""
        r["base_id"], r["next_id"], r["window_size"] = self.base_id, self.next_id, self.window_size
        r["alloc"], r["max_alloc"] = self.alloc, self.max_alloc_given
        r["window_parent_id"] = NO_PARENT if self.window_parent_id is None else self.window_parent_id
        r["channel_parent_id"] = [NO_PARENT if v is None else v for v in self.channel_parent_id]

    def emit_packet(self, size, channel_id, mode):
        """emit_packet's second half (:164-234) for the packet at the queue's front, stale ones already dropped:
        WINDOW_LIMITED, ALLOC_LIMITED, or (sequence_id, window_parent_lead, channel_parent_lead, resend)."""
        if sub(self.next_id, self.base_id) >= self.window_size:
            return WINDOW_LIMITED
        a = alloc_size(size)
        if self.alloc + a > self.max_alloc:
            return ALLOC_LIMITED
        seq = self.next_id
        lead = lambda parent: 0 if parent is None else sub(seq, parent) & 0xFFFF  # `as u16`  # noqa: E731
        wl, cl = lead(self.window_parent_id), lead(self.channel_parent_id[channel_id])
        self.window[seq] = (a, channel_id)
        self.next_id = (self.next_id + 1) & ID_MASK
        self.alloc += a
        if mode == RELIABLE:
            self.window_parent_id = self.channel_parent_id[channel_id] = seq
        return seq, wl, cl, mode in (PERSISTENT, RELIABLE)

    def acknowledge(self, receiver_base_id):  # :242-275
        if sub(receiver_base_id, self.base_id) > sub(self.next_id, self.base_id):
            return
        while self.base_id != receiver_base_id:
            a, ch = self.window.pop(self.base_id)
            if self.window_parent_id == self.base_id:
                self.window_parent_id = None
            if self.channel_parent_id[ch] == self.base_id:
                self.channel_parent_id[ch] = None
            self.alloc -= a
            self.base_id = (self.base_id + 1) & ID_MASK


def fragments(size):
    """PendingPacket::new's last_fragment_id and datagram()'s ranges: [(offset in the packet, length)]."""
    num = (size + MAX_FRAGMENT_SIZE - 1) // MAX_FRAGMENT_SIZE + (1 if size == 0 else 0)
    return [(f * MAX_FRAGMENT_SIZE, MAX_FRAGMENT_SIZE if f < num - 1 else size - f * MAX_FRAGMENT_SIZE) for f in range(num)]


def _form_flags(channel_id, seq, wl, cl, f, last, length):
    dg = dict(sequence_id=seq, channel_id=channel_id, window_parent_lead=wl, channel_parent_lead=cl, fragment_id=f,
              fragment_id_last=last, data=bytes(length))
    return {6: 0, 9: 1, 14: 2}[len(C.datagram_header(dg))], 1 if C.datagram_is_valid(dg) else 0


def packet_items(pk, seq, wl, cl):
    """The ITEM_DTYPE records of an emitted packet's fragments."""
    frs = fragments(int(pk["data_len"]))
    last = len(frs) - 1
    out = np.zeros(len(frs), dtype=ITEM_DTYPE)
    out["id"], out["channel_id"], out["window_parent_lead"], out["channel_parent_lead"] = seq, pk["channel_id"], wl, cl
    out["fragment_id"], out["fragment_id_last"] = np.arange(len(frs)), last
    out["data_offset"] = (int(pk["data_offset"]) + np.array([o for o, _ in frs], dtype=np.int64)) & 0xFFFFFFFF
    out["data_len"] = [n for _, n in frs]
    # every fragment but the last has fragment 0's form and validity
    ch = int(pk["channel_id"])
    out["form"], out["flags"] = _form_flags(ch, seq, wl, cl, 0, last, frs[0][1])
    out["form"][last], out["flags"][last] = _form_flags(ch, seq, wl, cl, last, last, frs[last][1])
    return out


class Expected:
    pass


def expect(packets, packet_first, senders, txs=None):
    """What an emit of these senders must give, every item listed (no cap): .items (slots no packet owns hold
    FILL bytes), .flush_first, .packet_results, .sender_results, .senders_out, .items_used.  txs: Tx objects to
    use (and advance) instead of ones made from the sender records."""
    n = len(senders)
    e = Expected()
    e.packet_results = np.zeros(len(packets), dtype=PACKET_RESULT_DTYPE)
    e.sender_results = np.zeros(n, dtype=SENDER_RESULT_DTYPE)
    e.senders_out = senders.copy()
    e.flush_first = np.zeros(n + 1, dtype=np.uint64)
    chunks, total = [], 0

    def reserve(k):
        nonlocal total
        if k:
            chunks.append(np.frombuffer(bytes([FILL]) * (ITEM_DTYPE.itemsize * k), dtype=ITEM_DTYPE))
            total += k

    for s in range(n):
        sd, r = senders[s], e.sender_results[s]
        e.flush_first[s] = r["item_first"] = total
        a, b = int(packet_first[s]), int(packet_first[s + 1])
        if a > b or b > len(packets):
            r["stop"] = BAD_RANGE
            continue
        tx = txs[s] if txs is not None else Tx.from_record(sd)
        reserve(int(sd["reserve_items"]))
        stop, i = DONE, 0
        upto = min(b - a, int(sd["take"]))
        while i < upto:
            pk = packets[a + i]
            size, ch, mode = int(pk["data_len"]), int(pk["channel_id"]), int(pk["mode"])
            if ch >= CHANNEL_COUNT or mode > RELIABLE or size > MAX_PACKET_SIZE:  # enqueue_packet's asserts
                stop = BAD_PACKET
                break
            if mode == TIME_SENSITIVE and int(pk["flush_id"]) != int(sd["flush_id"]):  # :150-162
                e.packet_results[a + i]["status"] = DROPPED
                r["packets_dropped"] += 1
                r["bytes_dropped"] += size
                i += 1
                continue
            got = tx.emit_packet(size, ch, mode)
            if got in (WINDOW_LIMITED, ALLOC_LIMITED):
                stop = got
                break
            seq, wl, cl, resend = got
            its = packet_items(pk, seq, wl, cl)
            pr = e.packet_results[a + i]
            pr["sequence_id"], pr["item_first"], pr["item_count"] = seq, total, len(its)
            pr["status"], pr["resend"] = EMITTED, resend
            chunks.append(its)
            total += len(its)
            r["packets_emitted"] += 1
            i += 1
        r["packets_consumed"], r["stop"] = i, stop
        r["item_count"] = total - int(r["item_first"])
        tx.to_record(e.senders_out[s])
    e.flush_first[n] = e.items_used = total
    e.items = np.concatenate(chunks) if chunks else np.zeros(0, ITEM_DTYPE)
    return e


def check(got, exp, items_cap=None):
    """got = (items, flush_first, packet_results, sender_results, senders_out, items_used) of an emit, host
    arrays, the items pre-filled with FILL bytes: every field of every record against exp = expect(...), the
    items below min(items_used, items_cap), and FILL in every slot behind them."""
    items, flush_first, packet_results, sender_results, senders_out, used = got
    assert int(used) == exp.items_used, (int(used), exp.items_used)
    assert np.array_equal(np.asarray(flush_first).astype(np.uint64), exp.flush_first)

    def same(name, a, dtype, b):
        a = np.asarray(a).view(dtype).reshape(-1)
        assert a.size == b.size, (name, a.size, b.size)
        for fld in dtype.names:
            ne = a[fld] != b[fld]
            bad = np.nonzero(ne.any(axis=1) if ne.ndim > 1 else ne)[0]
            assert bad.size == 0, f"{name}[{bad[0]}].{fld}: {a[fld][bad[0]]} != {b[fld][bad[0]]}"

    same("sender_results", sender_results, SENDER_RESULT_DTYPE, exp.sender_results)
    same("senders_out", senders_out, SENDER_DTYPE, exp.senders_out)
    if packet_results is not None:
        same("packet_results", packet_results, PACKET_RESULT_DTYPE, exp.packet_results)
    m = exp.items_used if items_cap is None else min(exp.items_used, items_cap)
    items = np.asarray(items).view(ITEM_DTYPE).reshape(-1)
    assert items.size >= m
    same("items", items[:m], ITEM_DTYPE, exp.items[:m])
    assert (items[m:].view(np.uint8) == FILL).all(), "wrote an item slot past the total or the cap"


# ---- inputs ----

def pkt(size, channel=0, mode=UNRELIABLE, flush_id=0, offset=None):
    p = np.zeros((), dtype=PACKET_DTYPE)
    p["data_len"], p["channel_id"], p["mode"], p["flush_id"] = size, channel, mode, flush_id
    p["data_offset"] = 0xFFFFFFFF if offset is None else offset  # (None: laid out by Senders.arrays)
    return p, offset is None


class Senders:
    """A batch under construction: add(packets, ...) appends one sender that owns the packets given."""

    def __init__(self):
        self.packets, self.first, self.senders, self.names = [], [0], [], []
        self.arena = 0
        self.facts = {}

    def add(self, packets, name="", tx=None, flush_id=0, take=0xFFFFFFFF, reserve_items=0, facts=None, **state):
        """tx: a Tx to take the state from; else Tx(window_size, base_id, max_alloc) with next_id, alloc,
        window_parent_id, channel_parents={channel: id} set as given.  facts: what check_facts asserts of the
        model's output for this sender."""
        if facts is not None:
            assert name and name not in self.facts, name
            self.facts[name] = facts
        if tx is None:
            tx = Tx(state.pop("window_size", MAX_PACKET_WINDOW_SIZE), state.pop("base_id", 0),
                    state.pop("max_alloc", 1 << 40))
            tx.next_id = state.pop("next_id", tx.base_id)
            tx.alloc = state.pop("alloc", 0)
            tx.window_parent_id = state.pop("window_parent_id", None)
            for ch, v in state.pop("channel_parents", {}).items():
                tx.channel_parent_id[ch] = v
        assert not state, state
        for p, lay in packets:
            p = p.copy()
            if lay:
                p["data_offset"] = self.arena
                if int(p["data_len"]) <= MAX_PACKET_SIZE:  # (a bad packet takes no room)
                    self.arena += int(p["data_len"])
            self.packets.append(p)
        self.first.append(len(self.packets))
        sd = np.zeros((), dtype=SENDER_DTYPE)
        tx.to_record(sd)
        sd["flush_id"], sd["take"], sd["reserve_items"] = flush_id, take, reserve_items
        self.senders.append(sd)
        self.names.append(name)
        return self

    def index(self, name):
        return self.names.index(name)

    def arrays(self):
        packets = np.array(self.packets, dtype=PACKET_DTYPE) if self.packets else np.zeros(0, PACKET_DTYPE)
        return packets, np.array(self.first, dtype=np.uint64), np.array(self.senders, dtype=SENDER_DTYPE)


def reference_cases():
    """packet_sender.rs's own tests `basic` and `parent_leads`: (Senders, [per sender: the (sequence_id,
    channel_id, window_parent_lead, channel_parent_lead, resend) tuples its asserts list])."""
    U, R = UNRELIABLE, RELIABLE
    b = Senders()
    b.add([pkt(4, 0, TIME_SENSITIVE), pkt(4, 0, U), pkt(4, 0, PERSISTENT), pkt(4, 0, R)], "basic", max_alloc=10000)
    b.add([pkt(4, 1, U), pkt(4, 1, R), pkt(4, 1, U), pkt(4, 0, R), pkt(4, 0, U), pkt(4, 0, U), pkt(4, 0, R), pkt(4, 1, R)],
          "parent_leads", max_alloc=10000)
    want = [[(0, 0, 0, 0, False), (1, 0, 0, 0, False), (2, 0, 0, 0, True), (3, 0, 0, 0, True)],
            [(0, 1, 0, 0, False), (1, 1, 0, 0, True), (2, 1, 1, 1, False), (3, 0, 2, 0, True), (4, 0, 1, 1, False),
             (5, 0, 2, 2, False), (6, 0, 3, 3, True), (7, 1, 1, 6, True)]]
    return b, want


ACK_ROUND = [(1, UNRELIABLE), (1, RELIABLE), (1, UNRELIABLE), (0, RELIABLE), (0, UNRELIABLE), (0, RELIABLE), (1, RELIABLE)]
# (channel, window_parent_lead, channel_parent_lead, resend) after sequence id ref_id + k
ACK_ROUND_WANT = [(1, 0, 0, False), (1, 0, 0, True), (1, 1, 1, False), (0, 2, 0, True), (0, 1, 1, False), (0, 2, 2, True),
                  (1, 1, 5, True)]
ALLOC_SIZE_TABLE = [(0, 0), (1, 1), (MAX_FRAGMENT_SIZE - 1, MAX_FRAGMENT_SIZE - 1), (MAX_FRAGMENT_SIZE, MAX_FRAGMENT_SIZE),
                    (MAX_FRAGMENT_SIZE + 1, 2 * MAX_FRAGMENT_SIZE), (2 * MAX_FRAGMENT_SIZE - 1, 2 * MAX_FRAGMENT_SIZE),
                    (2 * MAX_FRAGMENT_SIZE, 2 * MAX_FRAGMENT_SIZE), (2 * MAX_FRAGMENT_SIZE + 1, 3 * MAX_FRAGMENT_SIZE)]
EDGE_LENGTHS = (0, 1, 1447, 1448, 1449, 2896, 2897)


def edge_cases():
    """The single edge cases as one batch (each sender one case, found by name)."""
    U, R, T, P = UNRELIABLE, RELIABLE, TIME_SENSITIVE, PERSISTENT
    F = MAX_FRAGMENT_SIZE
    b = Senders()
    b.add([pkt(n, k % 3, (U, R, P)[k % 3]) for k, n in enumerate(EDGE_LENGTHS)], "lengths")
    b.add([pkt(0), pkt(F), pkt(F + 1)], "fragment_emission")
    b.add([pkt(5), pkt(MAX_PACKET_SIZE + 1, offset=0), pkt(5)], "too_long")
    # ids wrap at 2^20, with parents before the wrap
    b.add([pkt(3, 2, U), pkt(3, 2, R), pkt(3, 2, U), pkt(3, 5, U), pkt(3, 2, U)], "id_wrap", base_id=0xFFFFA,
          next_id=0xFFFFE, window_parent_id=0xFFFFD, channel_parents={2: 0xFFFFB, 5: 0xFFFFD})
    b.add([pkt(1), pkt(1)], "window_size_1", window_size=1, base_id=77, next_id=77)
    b.add([pkt(1)] * 10, "window_size_4096", window_size=4096, base_id=100, next_id=100 + 4090)
    for k in (2, 3, 4):  # room for three more packets
        b.add([pkt(1, mode=R)] * k, f"window_{k}_of_3", window_size=8, base_id=0xFFFFE, next_id=3)
    b.add([pkt(1)], "window_full", window_size=8, base_id=10, next_id=18)
    b.add([pkt(1)], "window_overfull", window_size=8, base_id=10, next_id=30)
    # max_alloc 2 * 1448 (given as 1449, rounded up), 1000 bytes in use: room for exactly 1896 more
    for n in (1895, 1896, 1897):
        b.add([pkt(448), pkt(n - 448), pkt(0)], f"alloc_{n}_of_1896", max_alloc=F + 1, alloc=1000)
    b.add([pkt(F + 1)], "alloc_rounded_fragment_fits", max_alloc=2 * F, alloc=0)       # a = 2 * 1448
    b.add([pkt(F + 1)], "alloc_rounded_fragment_limited", max_alloc=2 * F, alloc=1)
    b.add([pkt(1)], "alloc_over_max", max_alloc=F, alloc=5 * F)
    b.add([pkt(9), pkt(5, mode=T, flush_id=5), pkt(7, mode=T, flush_id=4), pkt(8, mode=T, flush_id=6), pkt(9), pkt(9)],
          "stale_before_window_stop", flush_id=5, window_size=2)
    b.add([pkt(7, mode=T, flush_id=4), pkt(9000), pkt(9)], "stale_before_alloc_stop", flush_id=5, max_alloc=F)
    b.add([pkt(1), pkt(7, channel=64, mode=T, flush_id=4), pkt(1)], "stale_and_bad", flush_id=5)
    b.add([pkt(1), pkt(7, mode=4), pkt(1)], "bad_mode")
    b.add([pkt(7, channel=200)], "bad_first")
    b.add([pkt(c + 1, c, R) for c in range(64)] + [pkt(2, 63 - c, U) for c in range(64)], "all_channels_reliable")
    b.add([pkt(1, 3), pkt(1, 4)], "made_up_parents", next_id=50, window_parent_id=None, channel_parents={3: 40})
    b.add([pkt(1, 3)], "made_up_parents_2", next_id=50, window_parent_id=45, channel_parents={3: 48})
    b.add([pkt(1, 3)], "far_parents", next_id=0x20005, window_parent_id=3, channel_parents={3: 1})  # leads over 2^16
    for take in (0, 2, 4, 9):
        b.add([pkt(10 + k, mode=R) for k in range(4)], f"take_{take}", take=take)
    b.add([pkt(7, mode=T, flush_id=1), pkt(3), pkt(7, mode=T, flush_id=1), pkt(4)], "take_ends_on_stale", take=3)
    b.add([pkt(3000), pkt(2)], "reserve_3", reserve_items=3)
    b.add([], "reserve_only", reserve_items=2)
    b.add([pkt(2)], "reserve_take_0", reserve_items=4, take=0)
    b.add([], "empty")
    b.add([pkt(2, mode=T, flush_id=9)] * 3, "all_stale")
    return b


def tile_cases(tile=64):
    """The smallest shapes where one lane per packet, `tile` packets at a time, can go wrong."""
    U, R, T = UNRELIABLE, RELIABLE, TIME_SENSITIVE
    rng = random.Random(17)
    b = Senders()

    def mixed(n):
        return [pkt(rng.choice((0, 5, 300, 1448, 1449, 4000)), rng.randrange(4), rng.choice((T, U, U, PERSISTENT, R)),
                    flush_id=rng.choice((0, 0, 1))) for _ in range(n)]

    for n in (1, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 200):
        b.add(mixed(n), f"queue_{n}")
    b.add(mixed(200), "window_stop_tile_2", window_size=128, base_id=5, next_id=5 + 128 - (tile + 6))
    small = [pkt(100, k % 5, (U, R)[k % 7 == 0]) for k in range(200)]
    b.add(small, "alloc_stop_tile_3", max_alloc=100 * (2 * tile + 16))
    b.add(small[:2 * tile] + [pkt(1, channel=70)] + small, "bad_tile_3")
    # parents set in the first tile, used two tiles later: window (packet 5) and per channel (3 and 9)
    q = [pkt(1, 1, U) for _ in range(3 * tile + 8)]
    q[5], q[9] = pkt(1, 3, R), pkt(1, 9, R)
    for k in (2 * tile + 3, 2 * tile + 20, 3 * tile + 1):
        q[k] = pkt(1, 3, U)
    q[2 * tile + 7] = pkt(1, 9, U)
    b.add(q, "parents_two_tiles_on", window_parent_id=0xFFFF0, channel_parents={1: 0xFFFF8, 3: 0xFFFF9}, next_id=2)
    q = [pkt(2, 2, R) for _ in range(tile - 34)] + [pkt(3, 2, T, flush_id=1)] * 70 + [pkt(4, 2, U), pkt(4, 0, R), pkt(4, 2, U)]
    b.add(q, "stale_run_across_tiles")
    b.add([pkt(3, 1, T, flush_id=1)] * 199 + [pkt(6, 1, R)], "only_last_live")
    b.add([pkt(3, 1, T, flush_id=1)] * (2 * tile), "all_stale_two_tiles")
    b.add(mixed(3 * tile), "take_mid_tile", take=tile + 9)
    return b


def big_case():
    """A MAX_PACKET_SIZE packet (65 536 items, no payload needed) between two small ones."""
    return Senders().add([pkt(3, 1, RELIABLE, offset=0), pkt(MAX_PACKET_SIZE, 1, PERSISTENT, offset=16), pkt(9, 1, offset=3)],
                         "max_packet", reserve_items=1)


def random_batch(seed, n_senders=300, max_packets=150):
    """Senders with mixed modes, channels, sizes and limits: about a third each unlimited, window-limited and
    allocation-limited, stale and multi-fragment packets, a few bad ones."""
    rng = random.Random(seed)
    b = Senders()
    for _ in range(n_senders):
        n = rng.randrange(max_packets + 1) if rng.random() < 0.7 else rng.randrange(12)
        flush_id = rng.randrange(3)
        q = []
        for _ in range(n):
            t = rng.random()
            size = rng.randrange(64) if t < 0.4 else rng.randrange(1500) if t < 0.8 else rng.randrange(1400, 6000)
            mode = rng.choice((TIME_SENSITIVE, TIME_SENSITIVE, UNRELIABLE, PERSISTENT, RELIABLE))
            ch = rng.randrange(64) if rng.random() < 0.3 else rng.randrange(3)
            if rng.random() < 0.002:
                ch, mode, size = rng.choice(((64, mode, size), (ch, 7, size), (ch, mode, MAX_PACKET_SIZE + 1)))
            q.append(pkt(size, ch, mode, flush_id=flush_id if rng.random() < 0.7 else rng.randrange(3)))
        base = rng.getrandbits(20)
        in_flight = rng.randrange(40)
        nxt = (base + in_flight) & ID_MASK
        kind = rng.randrange(3)
        window_size = 4096 if kind != 1 else 1 << rng.randrange(5, 8)
        alloc = rng.randrange(100000)
        max_alloc = 1 << 40 if kind != 2 else alloc + rng.randrange(1, 60000)
        parents = {ch: (nxt - 1 - rng.randrange(in_flight)) & ID_MASK for ch in range(64) if in_flight and rng.random() < 0.1}
        wparent = max(parents.values(), key=lambda v: sub(v, base)) if parents and rng.random() < 0.8 else None
        if wparent is None:
            parents = {}
        b.add(q, flush_id=flush_id, window_size=window_size, base_id=base, next_id=nxt, alloc=alloc, max_alloc=max_alloc,
              window_parent_id=wparent, channel_parents=parents,
              take=0xFFFFFFFF if rng.random() < 0.8 else rng.randrange(n + 2),
              reserve_items=0 if rng.random() < 0.7 else rng.randrange(1, 6))
    return b


def filled_items(n):
    a = np.zeros(n, dtype=ITEM_DTYPE)
    a.view(np.uint8)[:] = FILL
    return a


def many_max_packets(n_big=66, every=20):
    """n_big senders with one reliable MAX_PACKET_SIZE packet each (65 536 items a sender, no payload needed: the
    offsets are made up), ids and parents in flight so that both leads are non-zero, small senders before, after
    every `every` of them and behind.  Returns (Senders, the big senders' indices)."""
    rng = random.Random(41)
    small = [pkt(3, 1, RELIABLE, offset=0), pkt(MAX_FRAGMENT_SIZE + 1, 2, UNRELIABLE, offset=8), pkt(9, 1, offset=3)]
    b, big = Senders(), []
    for k in range(n_big):
        if k % every == 0:
            b.add(small, f"small_{k}", reserve_items=k % 3, base_id=rng.getrandbits(20))
        base = (ID_MASK - 2 if k == 0 else rng.getrandbits(20))   # (the first one's id is past the wrap)
        ch = (7 * k) % CHANNEL_COUNT
        big.append(len(b.senders))
        b.add([pkt(MAX_PACKET_SIZE, ch, RELIABLE, offset=1000 * k + 16)], f"big_{k}", base_id=base, next_id=(base + 5) & ID_MASK,
              window_parent_id=(base + 3) & ID_MASK, channel_parents={ch: (base + 1 + k % 2) & ID_MASK})
    b.add(small, "small_last")
    return b, big


def check_max_packets(items, flush_first, packets, packet_first, senders, big):
    """The items of senders that own one MAX_PACKET_SIZE packet, in closed form: fragment f of 65 536 at data_offset
    + f * 1448, 1448 bytes each, the sequence id and the leads the restatement's: expect() runs on each sender
    alone, its first and last three items are compared field for field, the rest by the formula."""
    items = np.asarray(items).view(ITEM_DTYPE).reshape(-1)
    n = MAX_PACKET_SIZE // MAX_FRAGMENT_SIZE
    f = np.arange(n, dtype=np.int64)
    for s in big:
        a = int(packet_first[s])
        pk = packets[a]
        assert int(packet_first[s + 1]) - a == 1 and int(pk["data_len"]) == MAX_PACKET_SIZE and int(senders[s]["reserve_items"]) == 0
        e = expect(packets[a: a + 1], np.array([0, 1], dtype=np.uint64), senders[s: s + 1])
        got = items[int(flush_first[s]): int(flush_first[s + 1])]
        assert got.size == n == e.items_used, (s, got.size)
        for k in (0, 1, 2, n - 3, n - 2, n - 1):
            assert got[k] == e.items[k], (s, k, got[k], e.items[k])
        seq, wl, cl = (int(e.items[0][fld]) for fld in ("id", "window_parent_lead", "channel_parent_lead"))
        assert wl != 0 and cl != 0 and seq == int(senders[s]["next_id"])
        for fld, want in (("id", seq), ("channel_id", pk["channel_id"]), ("window_parent_lead", wl),
                          ("channel_parent_lead", cl), ("fragment_id", f), ("fragment_id_last", n - 1),
                          ("data_offset", (int(pk["data_offset"]) + f * MAX_FRAGMENT_SIZE) & 0xFFFFFFFF),
                          ("data_len", MAX_FRAGMENT_SIZE)):
            assert np.array_equal(got[fld], np.broadcast_to(want, n)), (s, fld)
        assert (got["form"][:-1] == got["form"][0]).all() and (got["flags"][:-1] == got["flags"][0]).all(), s


# ---- lane 63 and the tile seam of the sender kernel, the seams of the item kernel, the finish kernel's widths ----

SENDER_FACTS = ("packets_consumed", "stop", "packets_emitted", "packets_dropped", "bytes_dropped", "item_count", "item_first")


def check_facts(b, exp):
    """Every named sender's facts against exp = expect(...), the model's output.  Keys: a sender result's field; a
    field of senders_out (alloc, next_id, window_parent_id); channel_parents {channel: id} of senders_out;
    window_leads, channel_leads, seq, status, slot {packet: value} (slot: the packet's absolute first item);
    first_item {packet: its first item relative to the sender's}; zero_past: the packet results from that packet
    on are zero records."""
    for name, f in b.facts.items():
        s = b.index(name)
        a, z = b.first[s], b.first[s + 1]
        r, out = exp.sender_results[s], exp.senders_out[s]
        pr = exp.packet_results[a:z]
        for key, want in f.items():
            if key in SENDER_FACTS:
                got = int(r[key])
            elif key in ("alloc", "next_id", "window_parent_id"):
                got = int(out[key])
            elif key == "channel_parents":
                got = {ch: int(out["channel_parent_id"][ch]) for ch in want}
            elif key in ("window_leads", "channel_leads"):
                fld = "window_parent_lead" if key == "window_leads" else "channel_parent_lead"
                assert all(pr["status"][k] == EMITTED for k in want), (name, key)
                got = {k: int(exp.items[int(pr["item_first"][k])][fld]) for k in want}
            elif key == "seq":
                got = {k: int(pr["sequence_id"][k]) for k in want}
            elif key == "status":
                got = {k: int(pr["status"][k]) for k in want}
            elif key == "slot":
                got = {k: int(pr["item_first"][k]) for k in want}
            elif key == "first_item":
                got = {k: int(pr["item_first"][k]) - int(r["item_first"]) for k in want}
            elif key == "zero_past":
                assert want < z - a, (name, key)
                got = want if not pr[want:].view(np.uint8).any() else None
            else:
                raise KeyError(key)
            assert got == want, (name, key, got, want)


def lane_cases(tile=64):
    """Senders whose deciding packet sits on lane 63 of a tile of `tile` packets or on lane 0 of the next one,
    for every read of the sender kernel that crosses lanes or tiles; senders laid out so that the item kernel's
    workgroups of 256 slots meet a range start, a packet and reserved slots at their seams.  One batch, the item
    kernel's senders first (their slot numbers are absolute).  The packet count is a multiple of 16 (padded)."""
    U, R, T = UNRELIABLE, RELIABLE, TIME_SENSITIVE
    F = MAX_FRAGMENT_SIZE
    assert tile == 64
    b = Senders()
    stale = lambda n=7, ch=2: pkt(n, ch, T, flush_id=1)  # noqa: E731  (under the senders' flush_id 0)

    # The item kernel.  One seam cannot hold all three events, so they sit on three: a packet of three
    # fragments on slots 254, 255 | 256; reserved slots 510, 511 | 512; a range that starts at slot 768 behind
    # two empty senders whose flush_first is 768 as well; and one that starts at slot 1023.
    b.add([pkt(1)] * 254 + [pkt(3000)] + [pkt(1)] * 253, "items_kernel_seams[straddle]",
          facts={"item_first": 0, "item_count": 510, "slot": {253: 253, 254: 254, 255: 257}})
    b.add([pkt(1, 1, R)] * 255, "items_kernel_seams[reserved]", reserve_items=3,
          facts={"item_first": 510, "item_count": 258, "slot": {0: 513}})
    b.add([], "items_kernel_seams[empty_a]", facts={"item_first": 768, "item_count": 0})
    b.add([], "items_kernel_seams[empty_b]", facts={"item_first": 768, "item_count": 0})
    b.add([pkt(3000, 2, R)] + [pkt(1, 2)] * 252, "items_kernel_seams[starts_at_seam]",
          facts={"item_first": 768, "item_count": 255, "slot": {0: 768, 1: 771}, "channel_leads": {1: 1, 5: 5}})
    # (own) a range that starts on the last slot of a workgroup: the narrowed search's upper end is its sender
    b.add([pkt(1, 4, R)] * 2, "items_kernel_seams[starts_at_last_slot]",
          facts={"item_first": 1023, "item_count": 2, "slot": {0: 1023, 1: 1024}})

    # stop_at[p]: a stop of each kind on lane 63, on lane 0 and lane 1 of tile 2, on lane 63 of tile 2 and on
    # lane 0 of tile 3; over an all-live queue, and over one whose even packets (but p) are stale: rank != lane
    for p in (63, 64, 65, 127, 128):
        for form in ("live", "stale_even"):
            is_live = [form == "live" or k % 2 == 1 or k == p for k in range(p + 10)]
            q = [pkt(F * (1 + (k % 3 == 0)), k % 5, R if k % 7 == 3 else U) if is_live[k] else stale(9, k % 5)
                 for k in range(p + 10)]
            rank = sum(is_live[:p])
            before = sum(alloc_size(int(q[k][0]["data_len"])) for k in range(p) if is_live[k])
            dropped = p - rank
            common = {"packets_consumed": p, "packets_emitted": rank, "packets_dropped": dropped, "bytes_dropped": 9 * dropped,
                      "alloc": 500 * F + before}
            base = 0xFFFC0  # (the ids wrap inside the queue)
            # room for `rank` packets: the window stops the live packet with that rank, packet p
            b.add(q, f"stop_at[{p}][window][{form}]", window_size=256, base_id=base, next_id=(base + 256 - rank) & ID_MASK,
                  alloc=500 * F, facts=dict(common, stop=WINDOW_LIMITED, next_id=(base + 256) & ID_MASK))
            assert before % F == 0
            b.add(q, f"stop_at[{p}][alloc][{form}]", base_id=base, next_id=base, alloc=500 * F, max_alloc=500 * F + before,
                  facts=dict(common, stop=ALLOC_LIMITED, next_id=(base + rank) & ID_MASK))
            bad = list(q)
            bad[p] = pkt(1, channel=70)
            b.add(bad, f"stop_at[{p}][bad][{form}]", base_id=base, next_id=base, alloc=500 * F,
                  facts=dict(common, stop=BAD_PACKET, next_id=(base + rank) & ID_MASK))

    # the window parent: the only reliable packet on lane 63; reliable packets on lanes 62 and 63; the reliable
    # packet on lane 0 of tile 2, read by lane 1.  next_id 100, the carried parent 90.
    def on_channel_1(n, reliable):
        return [pkt(2, 1, R if k in reliable else U) for k in range(n)]

    state = dict(next_id=100, window_parent_id=90, channel_parents={1: 80})
    b.add(on_channel_1(130, (63,)), "window_parent_at_63", **state,
          facts={"window_leads": {0: 10, 62: 72, 63: 73, 64: 1, 129: 66}, "channel_leads": {63: 83, 64: 1, 129: 66},
                 "window_parent_id": 163, "channel_parents": {1: 163}})
    b.add(on_channel_1(130, (62, 63)), "window_parent_at_63[62_and_63]", **state,
          facts={"window_leads": {62: 72, 63: 1, 64: 1, 129: 66}, "window_parent_id": 163})
    b.add(on_channel_1(130, (64,)), "window_parent_at_63[64]", **state,
          facts={"window_leads": {63: 73, 64: 74, 65: 1, 129: 65}, "window_parent_id": 164})

    # the channel parent: through parent[5] two tiles on; and lane 63 as the lane that moves mask[63] into parent[63]
    q = on_channel_1(130, ())
    q[63], q[64], q[128] = pkt(2, 5, R), pkt(2, 5, U), pkt(2, 5, U)
    b.add(q, "channel_parent_at_63", next_id=100, channel_parents={5: 70},
          facts={"channel_leads": {63: 93, 64: 1, 128: 65}, "channel_parents": {5: 163, 63: NO_PARENT}})
    q = on_channel_1(70, ())
    q[0], q[63], q[64] = pkt(2, 63, R), pkt(2, 63, U), pkt(2, 63, U)
    b.add(q, "channel_parent_at_63[channel_63]", next_id=100,
          facts={"channel_leads": {0: 0, 63: 63, 64: 64}, "channel_parents": {63: 100, 5: NO_PARENT}})

    # values that only lane 63 carries into the next tile: the fragment count, the alloc size, the dropped bytes
    b.add([stale()] * 63 + [pkt(3000)] + [pkt(F)] * 10, "only_lane_63[fragments]", next_id=500,
          facts={"first_item": {63: 0, 64: 3, 65: 4}, "item_count": 13, "packets_emitted": 11, "seq": {63: 500, 64: 501},
                 "packets_dropped": 63, "alloc": 3 * F + 10 * F})
    b.add([stale()] * 63 + [pkt(3000)] + [pkt(F)] * 10, "only_lane_63[alloc]", max_alloc=3 * F,
          facts={"stop": ALLOC_LIMITED, "packets_consumed": 64, "packets_emitted": 1, "alloc": 3 * F})
    b.add([stale()] * 63 + [pkt(3000)] + [pkt(F)] * 10, "only_lane_63[alloc][one_more]", max_alloc=4 * F,
          facts={"stop": ALLOC_LIMITED, "packets_consumed": 65, "packets_emitted": 2, "alloc": 4 * F})
    b.add([pkt(5)] * 63 + [stale(777)] + [pkt(5)] * 10, "only_lane_63[dropped]",
          facts={"packets_dropped": 1, "bytes_dropped": 777, "packets_emitted": 73, "status": {63: DROPPED, 64: EMITTED}})

    b.add([pkt(5, 3, R)] * 63 + [stale(11)] + [pkt(1, channel=70)] + [pkt(5)] * 5, "stale_63_then_stop_64",
          facts={"packets_consumed": 64, "stop": BAD_PACKET, "packets_dropped": 1, "bytes_dropped": 11, "packets_emitted": 63,
                 "status": {62: EMITTED, 63: DROPPED, 64: NOT_REACHED}})

    rng = random.Random(63)
    q200 = [pkt(rng.choice((0, 5, 300, F, F + 1, 4000)), rng.randrange(4), rng.choice((T, U, U, PERSISTENT, R)),
                flush_id=rng.choice((0, 0, 1))) for _ in range(200)]
    for t in (63, 64, 65, 128):
        b.add(q200, f"take_at[{t}]", take=t, facts={"packets_consumed": t, "stop": DONE, "zero_past": t})

    # the finish kernel's widths: 8 lanes serve 8 packets in one pass and the 9th in a second one
    b.add([pkt(3000, 1, R)] * 8, "finish_form_switch[8]", reserve_items=1, facts={"packets_consumed": 8})
    b.add([pkt(3000, 1, R)] * 9, "finish_form_switch[9]", reserve_items=1, facts={"packets_consumed": 9})
    b.add([pkt(1)] * (-len(b.packets) % 16), "pad_to_16")
    assert len(b.packets) % 16 == 0 and len(b.packets) // 16 > len(b.senders)
    return b


def with_empty_senders(packets, first, senders, n_senders):
    """The batch with empty senders behind it, n_senders in all."""
    extra = n_senders - senders.size
    assert extra >= 0
    empty = np.array([Senders().add([]).senders[0]] * extra, dtype=SENDER_DTYPE)
    return (packets, np.concatenate([first, np.full(extra, first[-1], dtype=np.uint64)]), np.concatenate([senders, empty]))
