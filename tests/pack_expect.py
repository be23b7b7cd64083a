"""Expected results of the batched pack (ufc_pack_host / ufc_pack_varlen), and the cases both test modules
share (test infrastructure, not a test module).

`expect` restates the emitters' push / finalize loop, src/half_connection/emit.rs:47-125 (data) and :170-211
(ack), in plain Python, one item at a time.  A datagram's encoded size comes from the codec oracle: the length
of oracle/codec.py `frame_write` of a data frame holding that one datagram, less the frame's own 10 bytes.
Nothing of the product is used.
"""
import random

import numpy as np

from oracle import codec as C
from uflow_amd.frame import FLUSH_DTYPE, FLUSH_RESULT_DTYPE, FRAME_INFO_DTYPE, ITEM_DTYPE

# Wire constants (src/lib.rs:281-297, src/packet_id.rs:5, src/frame/serial/mod.rs:25-49).
MAX_FRAME_SIZE = 1472
DATA_FRAME_OVERHEAD = 1 + 5 + 4   # frame id, sequence id + nonce|count, CRC
ACK_FRAME_OVERHEAD = 1 + 10 + 4   # frame id, two base ids + count, CRC
ACK_GROUP_SIZE = 9
MIN_DATAGRAM_OVERHEAD, MAX_DATAGRAM_OVERHEAD = 6, 14
MAX_FRAGMENT_SIZE = MAX_FRAME_SIZE - DATA_FRAME_OVERHEAD - MAX_DATAGRAM_OVERHEAD
MAX_PACKET_COUNT = min(0x100000 // (4096 * 2), 127)  # emit.rs:61-62
DATA, ACK = 10, 12
DONE, SIZE_LIMITED, WINDOW_LIMITED, BAD_RANGE = 0, 1, 2, 3
PACK_GRID = 256  # items per workgroup of the hops kernel (batch-relative) and per tile of the chain (flush-relative)

_size_cache = {}


def item_datagram(it, data=None):
    """The oracle's datagram dict of an item record."""
    return dict(sequence_id=int(it["id"]), channel_id=int(it["channel_id"]),
                window_parent_lead=int(it["window_parent_lead"]), channel_parent_lead=int(it["channel_parent_lead"]),
                fragment_id=int(it["fragment_id"]), fragment_id_last=int(it["fragment_id_last"]),
                data=bytes(int(it["data_len"])) if data is None else data)


def encoded_size(it):
    """DataFrameBuilder::encoded_size of an item record, from the oracle's frame_write."""
    key = (int(it["data_len"]), int(it["window_parent_lead"]), int(it["channel_parent_lead"]), int(it["fragment_id"]),
           int(it["fragment_id_last"]))
    if key not in _size_cache:
        f = {"kind": "data", "sequence_id": 0, "nonce": False, "datagrams": [item_datagram(it)]}
        _size_cache[key] = len(C.frame_write(f)) - DATA_FRAME_OVERHEAD
    return _size_cache[key]


def pack_flush(sizes, kind, flush_alloc, window_room):
    """emit.rs's loop over one flush's encoded sizes -> ([(first item, item count)], stop, pushed, alloc)."""
    ack = kind == ACK
    overhead = ACK_FRAME_OVERHEAD if ack else DATA_FRAME_OVERHEAD
    alloc = flush_alloc
    frames = []
    cur = None  # the frame in progress: [first item, size, count]

    def finalize():
        nonlocal cur, alloc
        if cur is not None:
            frames.append((cur[0], cur[2]))
            alloc -= cur[1]
            cur = None

    for idx, e in enumerate(sizes):
        if cur is not None:
            if alloc - cur[1] < 0:
                finalize()
                return frames, SIZE_LIMITED, idx, alloc
            if cur[1] + e > MAX_FRAME_SIZE or (not ack and cur[2] >= MAX_PACKET_COUNT):
                finalize()
            else:
                cur[1] += e
                cur[2] += 1
                continue
        if alloc < 0:
            return frames, SIZE_LIMITED, idx, alloc
        if not ack and len(frames) >= window_room:  # !frame_queue.can_push()
            return frames, WINDOW_LIMITED, idx, alloc
        cur = [idx, overhead + e, 1]
    finalize()
    return frames, DONE, len(sizes), alloc


def expect(items, flush_first, flushes, nonce_bits=None):
    """(infos, results, frames_used) a pack of these flushes must give, every frame listed (no cap)."""
    infos, results = [], np.zeros(len(flushes), dtype=FLUSH_RESULT_DTYPE)
    for j, fl in enumerate(flushes):
        a, b = int(flush_first[j]), int(flush_first[j + 1])
        r = results[j]
        r["frame_first"] = len(infos)
        r["alloc_left"] = fl["flush_alloc"]
        if a > b or b > len(items):
            r["stop"] = BAD_RANGE
            continue
        ack = int(fl["kind"]) == ACK
        sizes = [ACK_GROUP_SIZE if ack else encoded_size(items[i]) for i in range(a, b)]
        frames, stop, pushed, alloc = pack_flush(sizes, int(fl["kind"]), int(fl["flush_alloc"]), int(fl["window_room"]))
        for k, (s, c) in enumerate(frames):
            info = np.zeros((), dtype=FRAME_INFO_DTYPE)
            g = len(infos)
            info["kind"], info["ok"] = (ACK if ack else DATA), 1
            if ack:
                info["f"][0], info["f"][1] = fl["id0"], fl["id1"]
            else:
                info["f"][0] = (int(fl["id0"]) + k) & 0xFFFFFFFF
                info["aux"] = (int(nonce_bits[g // 32]) >> (g % 32)) & 1 if nonce_bits is not None else 0
            info["item_first"], info["item_count"] = a + s, c
            infos.append(info)
        r["frame_count"], r["items_packed"], r["stop"], r["alloc_left"] = len(frames), pushed, stop, alloc
    infos = np.array(infos, dtype=FRAME_INFO_DTYPE) if infos else np.zeros(0, FRAME_INFO_DTYPE)
    return infos, results, len(infos)


INFO_FIELDS = ("kind", "ok", "aux", "f", "item_count", "item_first")  # all but crc_ok


def check(got, exp, frames_cap=None):
    """got = (infos, results, frames_used) of a pack against exp = expect(...): the first min(frames_used,
    frames_cap) infos field by field, the results and the count."""
    infos, results, used = got
    e_infos, e_results, e_used = exp
    assert int(used) == e_used, (int(used), e_used)
    results = np.asarray(results).view(FLUSH_RESULT_DTYPE).reshape(-1)
    for fld in FLUSH_RESULT_DTYPE.names:
        bad = np.nonzero(results[fld] != e_results[fld])[0]
        assert bad.size == 0, f"results[{bad[0]}].{fld}: {results[fld][bad[0]]} != {e_results[fld][bad[0]]}"
    n = e_used if frames_cap is None else min(e_used, frames_cap)
    infos = np.asarray(infos).view(FRAME_INFO_DTYPE).reshape(-1)
    assert infos.size >= n
    for fld in INFO_FIELDS:
        ne = infos[fld][:n] != e_infos[fld][:n]
        bad = np.nonzero(ne.any(axis=1) if ne.ndim > 1 else ne)[0]
        assert bad.size == 0, f"infos[{bad[0]}].{fld}: {infos[fld][bad[0]]} != {e_infos[fld][bad[0]]}"


# ---- inputs ----

class Flushes:
    """A batch under construction: add(kind, items, ...) appends one flush that owns the items given."""

    def __init__(self):
        self.items, self.first, self.flushes = [], [0], []
        self.names, self.facts = [], {}

    def add(self, kind, items, flush_alloc=1 << 40, window_room=1 << 20, id0=0, id1=0, name="", at=None, facts=None):
        """at: the batch index modulo PACK_GRID the flush has to start at; a filler DATA flush of dgram(800)
        items goes in front of it where it would not.  facts: what check_facts asserts of the model's output."""
        if at is not None:
            pad = (at - len(self.items)) % PACK_GRID
            if pad:
                self.add(DATA, [dgram(800)] * pad)
            assert len(self.items) % PACK_GRID == at
        if name:
            assert name not in self.facts and name not in self.names, name
            self.facts[name] = dict(facts or {})
        self.names.append(name)
        self.items.extend(items)
        self.first.append(len(self.items))
        fl = np.zeros((), dtype=FLUSH_DTYPE)
        fl["kind"], fl["flush_alloc"], fl["window_room"], fl["id0"], fl["id1"] = kind, flush_alloc, window_room, id0, id1
        self.flushes.append(fl)
        return self

    def index(self, name):
        return self.names.index(name)

    def arrays(self):
        items = np.array(self.items, dtype=ITEM_DTYPE) if self.items else np.zeros(0, ITEM_DTYPE)
        return items, np.array(self.first, dtype=np.uint64), np.array(self.flushes, dtype=FLUSH_DTYPE)


def dgram(data_len, wpl=0, cpl=0, frag=0, frag_last=0, seq=0, channel=0):
    it = np.zeros((), dtype=ITEM_DTYPE)
    it["id"], it["channel_id"], it["data_len"] = seq, channel, data_len
    it["window_parent_lead"], it["channel_parent_lead"] = wpl, cpl
    it["fragment_id"], it["fragment_id_last"] = frag, frag_last
    return it


def group(base_id=0, bitfield=0, nonce=0):
    it = np.zeros((), dtype=ITEM_DTYPE)
    it["id"], it["data_offset"], it["channel_id"], it["form"] = base_id, bitfield, nonce, 3
    return it


def rand_dgram(rng, max_len=300):
    """Mixed header forms: micro (6), small (9) and large (14) at random, lengths 0..max_len."""
    t = rng.randrange(3)
    n = rng.randrange(max_len + 1) if rng.random() < 0.8 else rng.randrange(64)
    return dgram(n, wpl=rng.choice((0, 1, 127)) if t == 0 else rng.choice((0, 127, 128, 40000)),
                 cpl=rng.choice((0, 9, 255)) if t == 0 else rng.choice((0, 255, 256, 50000)),
                 frag=rng.randrange(3) if t == 2 else 0, frag_last=2 if t == 2 else 0,
                 seq=rng.getrandbits(20), channel=rng.randrange(64))


def rand_groups(rng, n):
    return [group(rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(1)) for _ in range(n)]


def single_cases():
    """The issue's single cases as one batch of flushes (each flush one case)."""
    b = Flushes()
    full = dgram(MAX_FRAGMENT_SIZE, frag=0, frag_last=1)  # a fragment of a two-fragment packet: a 1472-byte frame
    assert DATA_FRAME_OVERHEAD + encoded_size(full) == MAX_FRAME_SIZE
    b.add(DATA, [full, full], flush_alloc=2 * MAX_FRAME_SIZE)  # data_max_frame_size: two 1472-byte frames
    five = dgram(5)
    assert encoded_size(five) == MIN_DATAGRAM_OVERHEAD + 5
    for kind, item, unit, overhead in ((DATA, five, MIN_DATAGRAM_OVERHEAD + 5, DATA_FRAME_OVERHEAD),
                                       (ACK, group(), ACK_GROUP_SIZE, ACK_FRAME_OVERHEAD)):
        len_a, len_b = overhead + unit, overhead + 2 * unit  # data_size_limited / ack_size_limited
        for alloc in (0, len_a - 1, len_a, len_a + 1, len_b - 1, len_b, len_b + 1):
            for pushes in (1, 2, 3, 4):
                b.add(kind, [item] * pushes, flush_alloc=alloc)
    b.add(DATA, [full] * 6, flush_alloc=6 * MAX_FRAME_SIZE, window_room=5)  # data_window_limited
    max_groups = (MAX_FRAME_SIZE - ACK_FRAME_OVERHEAD) // ACK_GROUP_SIZE  # ack_max_frame_size
    assert max_groups == 161
    rng = random.Random(77)
    b.add(ACK, rand_groups(rng, max_groups), flush_alloc=2 * MAX_FRAME_SIZE, id0=0x01020304, id1=0xA0B0C0D0)
    b.add(ACK, rand_groups(rng, max_groups + 1), flush_alloc=2 * MAX_FRAME_SIZE, id0=7, id1=0xFFFFFFFF)
    b.add(ACK, [])  # no groups: no frame
    for cnt in (127, 128):  # the count limit
        b.add(DATA, [dgram(0, seq=k) for k in range(cnt)])
    # a frame of exactly 1472 bytes, and the same items with one more byte
    exact = [dgram(200, wpl=300), dgram(255, wpl=300), dgram(63), dgram(63)]
    rest = MAX_FRAME_SIZE - DATA_FRAME_OVERHEAD - sum(encoded_size(d) for d in exact) - MAX_DATAGRAM_OVERHEAD
    assert rest > 256
    b.add(DATA, exact + [dgram(rest)])
    b.add(DATA, exact + [dgram(rest + 1)])
    # a datagram larger than a frame: alone, and between small ones
    b.add(DATA, [dgram(3000)])
    b.add(DATA, [dgram(10), dgram(20), dgram(3000), dgram(30), dgram(40)])
    four = [full] * 4
    for room in (0, 1, 4, 5):  # window_room: none, one, the exact frame count, one more
        b.add(DATA, four, window_room=room)
    b.add(DATA, four, id0=0xFFFFFFFE)  # frame ids wrap
    b.add(DATA, [five] * 3, flush_alloc=-1)
    b.add(ACK, [group()] * 3, flush_alloc=-1)
    return b


def sweep_cases():
    """One small data flush (3 frames) and one ack flush of 170 groups (2 frames), each once per flush_alloc
    in -1 .. total + 1."""
    rng = random.Random(5)
    mixed = [dgram(400, wpl=1000), dgram(30), dgram(250, cpl=300), dgram(500, frag=1, frag_last=3), dgram(0),
             dgram(63), dgram(64), dgram(700, wpl=200), dgram(255), dgram(256), dgram(600, frag_last=1), dgram(90)]
    frames, _, _, alloc = pack_flush([encoded_size(d) for d in mixed], DATA, 1 << 40, 1 << 20)
    assert len(frames) == 3
    total = (1 << 40) - alloc
    b = Flushes()
    for fa in range(-1, total + 2):
        b.add(DATA, mixed, flush_alloc=fa, id0=fa & 0xFFFFFFFF)
    groups = rand_groups(rng, 170)
    total = 2 * ACK_FRAME_OVERHEAD + 170 * ACK_GROUP_SIZE
    for fa in range(-1, total + 2):
        b.add(ACK, groups, flush_alloc=fa, id0=1, id1=2)
    return b


def random_batch(seed, n_flushes, max_items):
    """Flushes of 0..max_items items with random limits; about one in five an ack flush."""
    rng = random.Random(seed)
    b = Flushes()
    for _ in range(n_flushes):
        n = rng.randrange(max_items + 1)
        ack = rng.random() < 0.2
        items = rand_groups(rng, n) if ack else [rand_dgram(rng) for _ in range(n)]
        r = rng.random()
        alloc = 1 << 40 if r < 0.4 else rng.randrange(-2, 200 * max(n, 1))
        room = 1 << 20 if rng.random() < 0.6 else rng.randrange(0, 6)
        b.add(ACK if ack else DATA, items, flush_alloc=alloc, window_room=room, id0=rng.getrandbits(32),
              id1=rng.getrandbits(32))
    return b


def nonce_words(seed, frames):
    rng = random.Random(seed)
    return np.array([rng.getrandbits(32) for _ in range((frames + 31) // 32 + 1)], dtype=np.uint32)


# ---- lane 63, the slot seams and the tile seams of the chain kernel; the hop window's seams ----

def check_facts(b, exp):
    """Every named flush's facts against exp = expect(...), the model's output: `starts` and `counts` (the
    frames' first items relative to the flush, and their item counts), `stop`, `items_packed`, `frame_count`."""
    infos, results, _ = exp
    for name, f in b.facts.items():
        j = b.index(name)
        r = results[j]
        fr = infos[int(r["frame_first"]): int(r["frame_first"]) + int(r["frame_count"])]
        got = {"starts": [int(x) - b.first[j] for x in fr["item_first"]], "counts": [int(x) for x in fr["item_count"]],
               "stop": int(r["stop"]), "items_packed": int(r["items_packed"]), "frame_count": int(r["frame_count"])}
        for key, want in f.items():
            assert got[key] == want, (name, key, got[key], want)


def _size_stops(b, prefix, kind, items, unit, overhead, starts, stops, at):
    """Per i of stops two flushes of `items`: flush_alloc = F(i) - 1 stops at i, flush_alloc = F(i) at i + 1, with
    F(i) = overhead * (starts before i) + unit * i over the unlimited chain's starts."""
    for i in stops:
        before = sum(1 for s in starts if s < i)
        upto = sum(1 for s in starts if s <= i)
        F = overhead * before + unit * i
        for alloc, tag, packed, n in ((F - 1, "", i, before), (F, "+1", i + 1, upto)):
            b.add(kind, items, flush_alloc=alloc, id0=i, id1=n, name=f"{prefix}[{i}]{tag}@{at}", at=at,
                  facts={"stop": SIZE_LIMITED, "items_packed": packed, "frame_count": n, "starts": starts[:n],
                         "counts": [q - p for p, q in zip(starts, starts[1:n] + [packed])]})


def lane_cases():
    """Flushes whose deciding item sits on lane 63, on lane 0 of the next slot of 64 or on item 0 of the next
    tile of PACK_GRID items, for the reads of the chain kernel that cross lanes; and flushes placed in the batch
    so that the hops kernel's window of prefix sums ends where they need it.  Every named flush carries the
    facts check_facts asserts of the model's output.  One batch: `short_beside_long` first (its four flushes are
    one workgroup's), the hop window's flushes last (one of them has to end the batch)."""
    T = PACK_GRID
    big, five = dgram(800), dgram(5)
    assert [encoded_size(d) for d in (big, five, dgram(16), dgram(67), dgram(0))] == [814, 11, 22, 76, 6]
    sixty_four = ([dgram(16)] * 63 + [dgram(67)]) * 9  # every frame 1472 bytes and 64 items
    assert DATA_FRAME_OVERHEAD + 63 * 22 + 76 == MAX_FRAME_SIZE
    b = Flushes()

    # four flushes of one workgroup: a wave's LDS rows and loop count beside its neighbours'
    b.add(DATA, [five] * 3, id0=1, name="short_beside_long[0]", facts={"starts": [0], "counts": [3], "stop": DONE})
    b.add(DATA, [big] * 513, id0=2, name="short_beside_long[1]",
          facts={"starts": list(range(513)), "counts": [1] * 513, "stop": DONE})
    b.add(DATA, [], id0=3, name="short_beside_long[2]", facts={"starts": [], "frame_count": 0, "stop": DONE})
    b.add(DATA, sixty_four[:257], id0=4, name="short_beside_long[3]",
          facts={"starts": [0, 64, 128, 192, 256], "counts": [64] * 4 + [1], "stop": DONE})
    assert [b.index(f"short_beside_long[{k}]") for k in range(4)] == [0, 1, 2, 3]

    small = [five] * 600
    frames, _, _, _ = pack_flush([encoded_size(d) for d in small], DATA, 1 << 40, 1 << 20)
    data_starts = [s for s, _ in frames]
    assert data_starts == [0, 127, 254, 381, 508]
    groups = rand_groups(random.Random(63), 600)
    frames, _, _, _ = pack_flush([ACK_GROUP_SIZE] * 600, ACK, 1 << 40, 1 << 20)
    ack_starts = [s for s, _ in frames]
    assert ack_starts == [0, 161, 322, 483]

    for at in (0, 7):
        for n in (64, 128, 255, 256, 257, 512, 513):  # the doubling's last round, lane 63's rank in every slot
            b.add(DATA, [big] * n, id0=n, name=f"every_item_a_start[{n}]@{at}", at=at,
                  facts={"starts": list(range(n)), "counts": [1] * n, "stop": DONE, "items_packed": n})
        for r in (63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 511, 512):
            b.add(DATA, [big] * 600, window_room=r, id0=r, name=f"window_stop_at[{r}]@{at}", at=at,
                  facts={"stop": WINDOW_LIMITED, "items_packed": r, "frame_count": r, "starts": list(range(r))})
        _size_stops(b, "size_stop_at", DATA, small, 11, DATA_FRAME_OVERHEAD, data_starts,
                    (63, 64, 127, 128, 191, 192, 254, 255, 256, 257, 381, 511, 512), at)
        for n, name in ((576, "frames_of_64_exact"), (256, "frames_of_64_exact[256]"), (257, "frames_of_64_exact[257]")):
            starts = list(range(0, n, 64))
            b.add(DATA, sixty_four[:n], id0=n, name=f"{name}@{at}", at=at,
                  facts={"starts": starts, "counts": [min(64, n - s) for s in starts], "stop": DONE})
        # a frame that starts on the tile's last item and goes on in the next tile; a frame that starts before
        # the tile's end and covers the whole part-tile behind it
        # (a datagram of 700 bytes does not fit behind one of 800, and takes the small ones behind it)
        b.add(DATA, [big] * 255 + [dgram(700)] + [five] * 39 + [big] * 5, name=f"start_at_255_straddles@{at}", at=at,
              facts={"starts": list(range(256)) + list(range(295, 300)), "counts": [1] * 255 + [40] + [1] * 5, "stop": DONE})
        b.add(DATA, [big] * 230 + [dgram(700)] + [five] * 65, name=f"start_at_255_straddles[covers]@{at}", at=at,
              facts={"starts": list(range(231)), "counts": [1] * 230 + [66], "stop": DONE, "items_packed": T + 40})
        _size_stops(b, "ack_stops", ACK, groups, ACK_GROUP_SIZE, ACK_FRAME_OVERHEAD, ack_starts,
                    (63, 64, 161, 255, 256, 322), at)
        b.add(ACK, groups[:322], id0=5, id1=6, name=f"ack_stops[2x161]@{at}", at=at,
              facts={"starts": [0, 161], "counts": [161, 161], "stop": DONE})

    # the hops kernel's window: zero-length datagrams, hop 127 by count
    zeros = [dgram(0, seq=k) for k in range(300)]
    assert DATA_FRAME_OVERHEAD + 127 * 6 < MAX_FRAME_SIZE
    for at in (129, 255):  # the items at batch index 129 and 255 (mod 256) read P up to base + 256 and base + 382
        b.add(DATA, zeros, name=f"hop_window_seams[at{at}]", at=at,
              facts={"starts": [0, 127, 254], "counts": [127, 127, 46], "stop": DONE})
    # hops near the flush's end are computed across the flush boundary (100 zero-length datagrams and one of 800
    # bytes fit a frame): the emit pass cuts them at the flush's end
    assert DATA_FRAME_OVERHEAD + 100 * 6 + 814 <= MAX_FRAME_SIZE
    b.add(DATA, zeros[:100], name="hop_window_seams[followed]", at=156,
          facts={"starts": [0], "counts": [100], "stop": DONE})
    b.add(DATA, [big] * 5, name="hop_window_seams[follower]", facts={"starts": [0, 1, 2, 3, 4], "counts": [1] * 5})
    assert b.first[b.index("hop_window_seams[follower]")] % T == 0
    # the last hops workgroup holds one item, and the last 126 hops are cut by n_items
    b.add(DATA, zeros[:130], name="hop_window_seams[last]", at=127,
          facts={"starts": [0, 127], "counts": [127, 3], "stop": DONE})
    assert len(b.items) % T == 1 and b.names[-1] == "hop_window_seams[last]"
    return b


def batch_end_case():
    """(own) A batch that ends on two 800-byte datagrams, the first on the last thread of a hops workgroup: its
    hop is 1 only by P[n_items], the one prefix sum the staged window's cap at n_items reaches."""
    b = Flushes().add(DATA, [dgram(800)] * 2, name="batch_ends_on_size", at=PACK_GRID - 1,
                      facts={"starts": [0, 1], "counts": [1, 1], "stop": DONE})
    assert len(b.items) == PACK_GRID + 1
    return b
