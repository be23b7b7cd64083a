"""A Python model of the batched frame routing (include/uflow_route.h), written from the reference's text.

Server::handle_frames (src/server/mod.rs:591-602) takes (frame, SocketAddr) pairs one after the other: Frame::read
(:598, None drops the frame), then handle_frame (:558-589) dispatches on the frame's kind.  handle_data / handle_ack /
handle_sync (:492-556) look the address up in clients: HashMap<SocketAddr, ..> (:118); a client in State::Active takes
the frame and has its timeout refreshed (:507, :529, :551), any other state drops it (`_ => ()`).  The handshake and
disconnect handlers are the only code that changes a client's state or the map's membership inside the loop, and only
for the frame's own address.  The model walks the pairs in order with a dict keyed by the 32 key bytes and a set of
addresses that have "stopped": from an address' first control frame on, what the map says about it is no longer what
the batch started with, so its session frames are deferred, not judged.  (One flag stands for all unknown addresses:
the header defers every unknown address' session frames behind the first control frame of any unknown address.)

The hash, the insertion and the probe are restated too, so that table bytes and lookups in arbitrary tables can be
compared.  numpy only.
"""
import numpy as np

from uflow_amd.records import ADDR_DTYPE, FRAME_INFO_DTYPE, ROUTE_RESULT_DTYPE, ROUTE_SLOT_DTYPE

NO_PARENT = 0xFFFFFFFF
DROP, CONN, CONTROL, DEFERRED = 0, 1, 2, 3
CONTROL_KINDS = (0, 1, 2, 3, 4, 5)      # handshake syn / syn-ack / ack / error, disconnect, disconnect-ack
SESSION_KINDS = (10, 11, 12)            # data, sync, ack
M32 = 0xFFFFFFFF


def key_bytes(addr):
    """The 32 key bytes of one ADDR_DTYPE record."""
    return np.asarray(addr, dtype=ADDR_DTYPE).reshape(1).tobytes()


def hash_key(seed, key):
    h = seed & M32
    for k in range(8):
        w = int.from_bytes(key[4 * k:4 * k + 4], "little")
        h = ((h ^ w) * 0x9E3779B1) & M32
        h ^= h >> 15
    h = (h * 0x85EBCA77) & M32
    h ^= h >> 13
    return h


def home_slot(seed, key, n_slots):
    return hash_key(seed, key) & (n_slots - 1)


def build_table(addrs, seed, n_slots):
    """Connections 0 .. n - 1 inserted in order by linear probing: (slots, max_probe), or ("dup", index)."""
    slots = np.zeros(n_slots, dtype=ROUTE_SLOT_DTYPE)
    keys = [None] * n_slots
    max_probe = 0
    for c in range(len(addrs)):
        key = key_bytes(addrs[c])
        home = home_slot(seed, key, n_slots)
        p = 0
        while True:
            s = (home + p) & (n_slots - 1)
            if keys[s] is None:
                keys[s] = key
                slots[s]["key"] = addrs[c]
                slots[s]["conn"] = c
                slots[s]["used"] = 1
                break
            if keys[s] == key:
                return "dup", c
            p += 1
        max_probe = max(max_probe, p)
    return slots, max_probe


def lookup(slots, seed, max_probe, n_conns, key):
    """The bounded probe over any bytes: the connection, or NO_PARENT."""
    n_slots = slots.size
    home = home_slot(seed, key, n_slots)
    for p in range(min(max_probe, n_slots - 1) + 1):
        s = slots[(home + p) & (n_slots - 1)]
        if s["used"] == 0:
            return NO_PARENT
        if int(s["conn"]) < n_conns and s.tobytes()[:32] == key:
            return int(s["conn"])
    return NO_PARENT


def kind_class(info):
    if info["ok"] == 0:
        return "none"
    if int(info["kind"]) in CONTROL_KINDS:
        return "control"
    return "session" if int(info["kind"]) in SESSION_KINDS else "none"


def route_frames(infos, addrs, offsets, slots, seed, max_probe, n_conns, conn_active, now_ms, active_timeout_ms,
                 timeout_in, clients=None):
    """The sequential loop.  clients: {key bytes: connection}, the map the table stands for; None takes every lookup
    from the table's bytes (garbage tables, a short max_probe).  Returns the outputs of ufc_route_frames_* as a dict."""
    n = len(infos)
    route = np.full(n, NO_PARENT, dtype=np.uint32)
    cls = np.zeros(n, dtype=np.uint8)
    results = np.zeros(n_conns, dtype=ROUTE_RESULT_DTYPE)
    results["first_control"] = NO_PARENT
    first_unknown_control = NO_PARENT
    stopped = set()              # addresses (connections) whose state the batch may have changed
    unknown_stopped = False
    buckets = [[] for _ in range(n_conns + 2)]
    timeout = np.array(timeout_in, dtype=np.uint64).copy()
    memo = {}
    for i in range(n):
        key = key_bytes(addrs[i])
        if key not in memo:
            memo[key] = (clients.get(key, NO_PARENT) if clients is not None
                         else lookup(slots, seed, max_probe, n_conns, key))
        c = memo[key]
        route[i] = c
        k = kind_class(infos[i])
        if k == "control":
            cls[i] = CONTROL
            if c == NO_PARENT:
                if not unknown_stopped:
                    first_unknown_control = i
                unknown_stopped = True
            else:
                if c not in stopped:
                    results["first_control"][c] = i
                stopped.add(c)
        elif k == "session":
            if c == NO_PARENT:
                cls[i] = DEFERRED if unknown_stopped else DROP        # clients.get(..) gave None
            elif c in stopped:
                cls[i] = DEFERRED
                results["deferred"][c] += 1
            elif conn_active[c]:
                cls[i] = CONN                                          # State::Active: the frame is handled,
                results["frames"][c] += 1                              # and the timeout refreshed
                timeout[c] = (now_ms + active_timeout_ms) & (2**64 - 1)
            else:
                cls[i] = DROP                                          # `_ => ()`
        else:
            cls[i] = DROP                                              # Frame::read gave None
        b = c if cls[i] == CONN else n_conns + (1 if cls[i] == DROP else 0)
        buckets[b].append(i)
    bucket_first = np.zeros(n_conns + 3, dtype=np.uint64)
    bucket_first[1:] = np.cumsum([len(b) for b in buckets], dtype=np.uint64)
    order = np.array([i for b in buckets for i in b], dtype=np.uint32)
    infos = np.asarray(infos, dtype=FRAME_INFO_DTYPE)
    off = np.zeros(n, dtype=np.uint64) if offsets is None else np.asarray(offsets, dtype=np.uint64)
    return {"route": route, "cls": cls, "bucket_first": bucket_first, "order": order, "infos_out": infos[order],
            "src_base_out": off[order], "results": results, "timeout_out": timeout,
            "first_unknown_control": first_unknown_control}


def colliding_addrs(seed, n_slots, home, count, start=0, port=7):
    """`count` V4 addresses whose home slot is `home`, found by search with the model's hash: (ip, port) pairs."""
    out = []
    x = start
    while len(out) < count:
        ip = "10.%d.%d.%d" % ((x >> 16) & 255, (x >> 8) & 255, x & 255)
        a = np.zeros(1, dtype=ADDR_DTYPE)
        a["ip"][0, :4] = [10, (x >> 16) & 255, (x >> 8) & 255, x & 255]
        a["port"], a["family"] = port, 4
        if home_slot(seed, a.tobytes(), n_slots) == home:
            out.append((ip, port))
        x += 1
    return out
