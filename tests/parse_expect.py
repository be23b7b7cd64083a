"""Expected outputs of the batched parse (ufc_parse_batch_varlen / ufc_parse_batch_host) built from the
codec oracle alone (test infrastructure, not a test module).

`oracle_records(frames)` decodes each frame with oracle/codec.py `frame_read` (serial/mod.rs:675-706;
datagram_is_valid of packet_receiver/mod.rs:12-30) and lays the result out as the C ABI's records
(include/uflow_frame_codec.h: ufc_frame_info, ufc_item).  `tile_records` expands the records of a few
distinct frames to a batch that repeats them, so a million-frame GPU parse is compared with the oracle
without decoding a million frames in Python (the full-size parse pinned to the oracle,
not to the product's own host parse).
"""
import numpy as np

import oracle
from oracle import codec as C
from uflow_amd.frame import FRAME_INFO_DTYPE, ITEM_DTYPE

ITEM_VALID = 1   # UFC_ITEM_VALID
FORM_ACK = 3     # ufc_item.form of an ack group


def _info_of(fb, ref, crc_ok):
    info = np.zeros(1, dtype=FRAME_INFO_DTYPE)[0]
    info["kind"] = fb[0] if len(fb) >= 1 else 0xFF
    info["crc_ok"] = 1 if crc_ok else 0
    items = []
    if ref is None:
        return info, items
    info["ok"] = 1
    k, f = ref["kind"], [0] * 5
    if k == "handshake_syn":
        info["aux"] = ref["version"]
        f[:4] = [ref["nonce"], ref["max_receive_rate"], ref["max_packet_size"], ref["max_receive_alloc"]]
    elif k == "handshake_syn_ack":
        f = [ref["nonce_ack"], ref["nonce"], ref["max_receive_rate"], ref["max_packet_size"], ref["max_receive_alloc"]]
    elif k == "handshake_ack":
        f[0] = ref["nonce_ack"]
    elif k == "handshake_error":
        f[0] = ref["nonce_ack"]
        info["aux"] = C.ERRORS.index(ref["error"])
    elif k == "data":
        f[0] = ref["sequence_id"]
        info["aux"] = 1 if ref["nonce"] else 0
        for dg in ref["datagrams"]:
            it = np.zeros(1, dtype=ITEM_DTYPE)[0]
            it["id"], it["channel_id"], it["form"] = dg["sequence_id"], dg["channel_id"], dg["header"]
            it["window_parent_lead"], it["channel_parent_lead"] = dg["window_parent_lead"], dg["channel_parent_lead"]
            it["fragment_id"], it["fragment_id_last"] = dg["fragment_id"], dg["fragment_id_last"]
            it["flags"] = ITEM_VALID if C.datagram_is_valid(dg) else 0
            it["data_offset"], it["data_len"] = dg["data_offset"], dg["data_len"]
            items.append(it)
    elif k == "sync":
        info["aux"] = (1 if ref["next_frame_id"] is not None else 0) | (2 if ref["next_packet_id"] is not None else 0)
        f[0] = ref["next_frame_id"] or 0
        f[1] = ref["next_packet_id"] or 0
    elif k == "ack":
        f[:2] = [ref["frame_window_base_id"], ref["packet_window_base_id"]]
        for g in ref["frame_acks"]:
            it = np.zeros(1, dtype=ITEM_DTYPE)[0]
            it["id"], it["channel_id"], it["form"], it["data_offset"] = g["base_id"], 1 if g["nonce"] else 0, FORM_ACK, \
                g["bitfield"]
            items.append(it)
    info["f"] = f
    info["item_count"] = len(items)
    return info, items


def oracle_records(frames):
    """(infos, items) of a batch of frames (bytes each) as the C ABI lays them out, from the oracle."""
    infos = np.zeros(len(frames), dtype=FRAME_INFO_DTYPE)
    items = []
    first = 0
    for i, fb in enumerate(frames):
        fb = bytes(fb)
        info, its = _info_of(fb, C.frame_read(fb), oracle.frame_validate(fb)[0] and len(fb) >= 5)
        info["item_first"] = first
        infos[i] = info
        items.extend(its)
        first += len(its)
    return infos, (np.array(items, dtype=ITEM_DTYPE) if items else np.zeros(0, ITEM_DTYPE))


def tile_records(base_infos, base_items, tile, dead):
    """Records of a batch whose frame i is base frame tile[i], except frames with dead[i] set (a bit
    flipped: the CRC gate fails, Frame::read returns None, no items)."""
    cnt = base_infos["item_count"].astype(np.int64)
    bfirst = base_infos["item_first"].astype(np.int64)
    infos = base_infos[tile].copy()
    if dead.any():
        d = infos[dead]
        d["ok"] = 0
        d["crc_ok"] = 0
        d["aux"] = 0
        d["f"] = 0
        d["item_count"] = 0
        infos[dead] = d
    n_items = np.where(dead, 0, cnt[tile])
    first = np.zeros(tile.size, dtype=np.int64)
    first[1:] = np.cumsum(n_items)[:-1]
    infos["item_first"] = first.astype(np.uint32)
    total = int(n_items.sum())
    # item j of frame i comes from base item bfirst[tile[i]] + j
    src = np.repeat(bfirst[tile] - first, n_items) + np.arange(total, dtype=np.int64)
    return infos, base_items[src]


def compare(got_infos, got_items, exp_infos, exp_items):
    """Every field of every frame Frame::read accepts, kind / ok / crc_ok / item_count / item_first of
    the others (their other fields are unspecified, include/uflow_frame_codec.h), and every item."""
    n = exp_infos.size
    assert got_infos.size == n
    ok = exp_infos["ok"] == 1
    raw_g = got_infos.view(np.uint8).reshape(n, -1)
    raw_e = exp_infos.view(np.uint8).reshape(n, -1)
    bad = np.nonzero(ok & (raw_g != raw_e).any(1))[0]
    assert bad.size == 0, f"{bad.size} accepted frames' infos differ from the oracle, first {bad[:8]}"
    for fld in ("kind", "ok", "crc_ok", "item_count", "item_first"):
        bad = np.nonzero(got_infos[fld] != exp_infos[fld])[0]
        assert bad.size == 0, f"{fld}: {bad.size} frames differ from the oracle, first {bad[:8]}"
    bad = np.nonzero(~ok & (got_infos["ok"] == 1))[0]
    assert bad.size == 0
    k = exp_items.size
    assert got_items.size >= k
    bad = np.nonzero((got_items[:k].view(np.uint8).reshape(k, -1) != exp_items.view(np.uint8).reshape(k, -1)).any(1))[0]
    assert bad.size == 0, f"{bad.size} items differ from the oracle, first {bad[:8]}"


# ---- named cases at workgroup seams and table limits ----
#
# The device parse runs workgroups of 256 frames, one thread per frame (frame_parse.hip).  Every case below
# places a named group of frames on a chosen thread of its workgroup and says, in `facts`, what the group is
# there for; check_facts asserts the facts on the oracle's records, so a generator that drifts fails before any
# product code runs.

WG = 256            # frames per workgroup (kParseThreads)
INLINE_SLOTS = 16   # header slots a frame holds of its own (kInlineSlots)
POS_SLOTS = 64      # header slots a frame may hold at all (kPosSlots)
POOL_SLOTS = 2048   # the workgroup's pool (kPoolSlots)
NONE, SLOT, ACKS, WALK = "none", "slot", "ack", "walk"


def micro(k=0, dl=0):
    """A datagram that takes the 6-byte header, dl payload bytes."""
    return dict(sequence_id=(k * 2654435761) & C.PACKET_ID_MASK, channel_id=k % 64, window_parent_lead=k % 128,
                channel_parent_lead=(k * 7) % 256, fragment_id=0, fragment_id_last=0,
                data=bytes((k + j) & 0xFF for j in range(dl)))


def small(k, dl):
    return dict(micro(k), window_parent_lead=300 + k % 100, channel_parent_lead=400 + k % 100,
                data=bytes((k + j) & 0xFF for j in range(dl)))


def large(k, dl):
    return dict(micro(k), fragment_id=k % 5, fragment_id_last=5 + k % 3, data=bytes((k + j) & 0xFF for j in range(dl)))


def data_frame(dgs, k=0):
    return C.frame_write({"kind": "data", "sequence_id": (k * 40503) & 0xFFFFFFFF, "nonce": bool(k & 1), "datagrams": dgs})


def micros(n, k=0, dl=0):
    return data_frame([micro(k + j, dl) for j in range(n)], k)


def ack_frame(groups, k=0):
    return C.frame_write({"kind": "ack", "frame_window_base_id": k, "packet_window_base_id": k + 1, "frame_acks": [
        {"base_id": (k + j) * 97, "bitfield": ((k + j) * 2654435761) & 0xFFFFFFFF, "nonce": bool((k + j) & 1)}
        for j in range(groups)]})


def _rejected(k):
    fb = bytearray(micros(3, k, 2))
    fb[7] ^= 0x10  # fails the gate
    return bytes(fb)


def filler(k):
    """A frame without items: a sync, a frame the gate rejects, a data frame of 0 datagrams, an ack of 0 groups."""
    r = k % 4
    if r == 0:
        return C.frame_write({"kind": "sync", "next_frame_id": k, "next_packet_id": None})
    if r == 1:
        return _rejected(k)
    if r == 2:
        return micros(0, k)
    return ack_frame(0, k)


def mode_of(info, length):
    """How the emit reaches a frame's items, pool aside: NONE, SLOT (u16 header slots), ACKS (fixed offsets) or
    WALK (walked again: more than POS_SLOTS datagrams, or a frame over 65535 bytes)."""
    if not info["ok"] or info["item_count"] == 0:
        return NONE
    if info["kind"] == C.ACK:
        return ACKS
    return SLOT if info["item_count"] <= POS_SLOTS and length <= 0xFFFF else WALK


class Frames:
    """A batch under construction: add(name, frames, at=, item_at=, facts=) appends a named group."""

    def __init__(self, title):
        self.title, self.frames, self.groups, self.facts = title, [], {}, {}
        self._items = 0  # items of the frames so far (the generators' own count; check_facts pins it to the oracle)

    def _push(self, fb, items):
        self.frames.append(fb)
        self._items += items

    def pad(self, at=None, item_at=None):
        """Fillers until the next frame is frame `at` of its workgroup; before them, where asked, one ack frame whose
        groups move the next item to index `item_at` modulo WG."""
        if item_at is not None and (item_at - self._items) % WG:
            self._push(ack_frame((item_at - self._items) % WG, len(self.frames)), (item_at - self._items) % WG)
        if at is not None:
            while len(self.frames) % WG != at:
                self._push(filler(len(self.frames)), 0)

    def add(self, name, frames, at=None, item_at=None, facts=None):
        """frames: (bytes, item count) pairs.  The group's first frame lands on thread `at`, its first item on item
        index `item_at` modulo WG."""
        self.pad(at, item_at)
        assert name not in self.groups, name
        self.groups[name] = (len(self.frames), len(frames))
        f = dict(facts or {})
        if at is not None:
            f.setdefault("frame_mod", at)
        if item_at is not None:
            f.setdefault("item_first_mod", item_at)
        f.setdefault("counts", [c for _, c in frames])
        self.facts[name] = f
        for fb, c in frames:
            self._push(fb, c)
        return self

    def arrays(self):
        offsets = np.zeros(len(self.frames) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(f) for f in self.frames])
        return np.frombuffer(b"".join(self.frames), dtype=np.uint8).copy(), offsets

    def records(self):
        if not hasattr(self, "_records"):
            self._records = oracle_records(self.frames)
        return self._records


def pool_demand(infos, lens, wg):
    """Pool entries the frames of workgroup `wg` ask for when none gives up: the headers past a frame's own
    INLINE_SLOTS, of the POS_SLOTS the walk records at most."""
    lo, hi = wg * WG, min((wg + 1) * WG, infos.size)
    return sum(max(0, min(int(infos[i]["item_count"]), POS_SLOTS) - INLINE_SLOTS) for i in range(lo, hi)
               if infos[i]["ok"] and infos[i]["kind"] == C.DATA)


def check_facts(batch, infos=None):
    """Asserts every group's facts on the oracle's records of the batch (never on the product's output)."""
    if infos is None:
        infos = batch.records()[0]
    lens = [len(f) for f in batch.frames]
    n = len(batch.frames)
    for name, (at, cnt) in batch.groups.items():
        f = batch.facts[name]
        rows = infos[at:at + cnt]
        got_counts = [int(r["item_count"]) for r in rows]
        wg = at // WG
        lo, hi = wg * WG, min((wg + 1) * WG, n)
        for key, want in f.items():
            if key == "frame_mod":
                got = at % WG
            elif key == "counts":
                got = got_counts
            elif key == "item_first_mod":
                got = int(rows[0]["item_first"]) % WG
            elif key == "item_first":
                got = int(rows[0]["item_first"])
            elif key == "modes":
                got = [mode_of(r, lens[at + j]) for j, r in enumerate(rows)]
            elif key == "wg_items":        # items of the group's workgroup
                got = int(infos["item_count"][lo:hi].sum())
            elif key == "wg_owners":       # which threads of it own items
                got = [i - lo for i in range(lo, hi) if infos[i]["item_count"]]
            elif key == "wg_frames":
                got = hi - lo
            elif key == "pool_demand":
                got = pool_demand(infos, lens, wg)
            elif key == "frame_bytes":
                got = [lens[at + j] for j in range(cnt)]
            elif key == "last_header_offset":  # frame offset of the group's first frame's last datagram header
                last = batch.records()[1][int(rows[0]["item_first"]) + got_counts[0] - 1]
                got = int(last["data_offset"]) - {0: 6, 1: 9, 2: 14}[int(last["form"])]
            elif key == "ends_batch":
                got = at + cnt == n
            elif key == "n_mod":
                got = n % WG
            else:
                raise AssertionError(f"unknown fact {key}")
            assert got == want, f"{batch.title}: {name}: {key} is {got}, the case wants {want}"


def _mix_fillers(k0, count):
    return [(filler(k0 + j), 0) for j in range(count)]


def lane_cases():
    """The batches of named groups, each under 3,000 frames (the Python decode is the larger part of a test's
    time).  Cases that need a batch's end -- an empty last workgroup, an empty last frame, a lone last frame --
    end a batch each, so there is more than one batch."""
    out = []

    # -- owners: the only frame with items on thread 0, on thread 255, on both; a workgroup without items between two
    # that have some; header slots at the inline/pool boundary (16/17) and the kPosSlots boundary (64/65) on threads
    # 0, 100 and 255; the batch ends on a lone frame with items (n = 1 mod 256)
    b = Frames("owners")
    b.add("only_frame_0", [(micros(5, 1, 1), 5)] + _mix_fillers(1, 255), at=0,
          facts={"wg_owners": [0], "wg_items": 5, "modes": [SLOT] + [NONE] * 255})
    b.add("only_frame_255", _mix_fillers(0, 255) + [(ack_frame(3, 9), 3)], at=0,
          facts={"wg_owners": [255], "wg_items": 3, "modes": [NONE] * 255 + [ACKS]})
    b.add("frames_0_and_255", [(micros(2, 3), 2)] + _mix_fillers(1, 254) + [(micros(4, 5, 3), 4)], at=0,
          facts={"wg_owners": [0, 255], "wg_items": 6})
    b.add("empty_workgroup_between[before]", [(micros(1 + k % 3, k), 1 + k % 3) for k in range(WG)], at=0,
          facts={"wg_items": 511})
    b.add("empty_workgroup_between", _mix_fillers(0, WG), at=0, facts={"wg_items": 0, "wg_owners": []})
    b.add("empty_workgroup_between[after]", [(ack_frame(2, k), 2) if k % 2 else (micros(1, k), 1) for k in range(WG)], at=0,
          facts={"wg_items": 384})
    for k in (16, 17, 64, 65):
        for at in (0, 100, 255):
            b.add(f"slots[{k}]@{at}", [(micros(k, at, at % 3), k)], at=at, item_at=255 if at == 100 else None,
                  facts={"modes": [SLOT if k <= POS_SLOTS else WALK],
                         "pool_demand": 3 * (min(k, POS_SLOTS) - INLINE_SLOTS) if at == 255 else None})
            if b.facts[f"slots[{k}]@{at}"]["pool_demand"] is None:
                del b.facts[f"slots[{k}]@{at}"]["pool_demand"]
    b.add("last_frame_alone", [(micros(7, 2, 1), 7)], at=0,
          facts={"ends_batch": True, "n_mod": 1, "wg_frames": 1, "wg_items": 7})
    out.append(b)

    # -- rounds of the emit's item loop: 255, 256, 257 and 513 items in one workgroup, from many small frames and from
    # one ack frame (513: one frame owning three rounds); the u16 slot limit; the batch ends on a frame without items
    b = Frames("rounds")
    for want in (255, 256, 257, 513):
        least = 2 if want > 300 else 1
        group, have = [], 0
        while have < want:
            c = want - have if want - have < least + 2 else least + len(group) % 3
            group.append((micros(c, have, 1), c))
            have += c
        assert len(group) < WG
        b.add(f"items_in_workgroup[{want}][small]", group, at=0, facts={"wg_items": want})
        b.pad(at=0)
        b.add(f"items_in_workgroup[{want}][ack]", [(ack_frame(want, want), want)], at=100,
              facts={"wg_items": want, "wg_owners": [100], "modes": [ACKS]})
        b.pad(at=0)
    for length in (65535, 65536):
        # one large datagram and a trailing micro datagram with no payload: 6 + 14 + dl + 6 + 4 bytes
        fb = data_frame([large(3, length - 30), micro(4)], length)
        b.add(f"len_{length}", [(fb, 2)], at=7, facts={"frame_bytes": [length], "last_header_offset": length - 10,
                                                        "modes": [SLOT if length <= 0xFFFF else WALK]})
    b.add("last_frame_empty[before]", [(micros(1 + k % 2, k), 1 + k % 2) for k in range(40)])
    b.add("last_frame_empty", [(micros(0, 5), 0)], facts={"ends_batch": True, "modes": [NONE]})
    out.append(b)

    # -- the pool: exactly 2048 entries wanted, one more, six times as many; the last workgroup has no items
    b = Frames("pool")
    b.add("pool_exact", [(micros(32, k), 32) if k % 2 else (micros(k % 17, k), k % 17) for k in range(WG)], at=0,
          facts={"pool_demand": POOL_SLOTS})
    b.add("pool_plus_one", [(micros(32, k), 32) if k % 2 else (micros(17 if k == 100 else k % 17, k), 17 if k == 100 else k % 17)
                            for k in range(WG)], at=0, facts={"pool_demand": POOL_SLOTS + 1})
    b.add("pool_all_want_48", [(micros(64, k), 64) for k in range(WG)], at=0,
          facts={"pool_demand": WG * 48, "modes": [SLOT] * WG})
    b.add("last_workgroup_empty", _mix_fillers(0, 100), at=0,
          facts={"ends_batch": True, "wg_items": 0, "wg_frames": 100})
    out.append(b)

    # -- one ack frame of 65535 groups: a single frame owning 256 rounds
    b = Frames("ack_groups_65535")
    b.add("before", [(filler(0), 0)])
    b.add("ack_groups_65535", [(ack_frame(65535, 1), 65535)], facts={"frame_bytes": [15 + 9 * 65535], "modes": [ACKS]})
    b.add("after", [(micros(1, 2), 1)], facts={"item_first": 65535})
    out.append(b)

    out.append(mode_mix())
    return out


def mode_mix():
    """Slot, ack, re-walked and empty frames on adjacent threads; a re-walked frame on thread 255 of workgroup 0 and
    on thread 0 of workgroup 1.  caps: the item caps the capped runs use."""
    b = Frames("mode_mix")
    group, modes = [], []
    for k in range(255):
        r = k % 4
        if r == 0:
            group.append((micros(3, k, 1), 3)), modes.append(SLOT)
        elif r == 1:
            group.append((ack_frame(2, k), 2)), modes.append(ACKS)
        elif r == 2:
            group.append((micros(70, k), 70)), modes.append(WALK)
        else:
            group.append((filler(k), 0)), modes.append(NONE)
    group.append((micros(66, 255), 66)), modes.append(WALK)
    wg0 = 64 * 3 + 64 * 2 + 64 * 70 + 66
    b.add("mode_mix[wg0]", group, at=0, facts={"modes": modes, "wg_items": wg0})
    tail = [(micros(65, 256), 65)] + [(micros(20, k, 2), 20) if k % 2 else (ack_frame(5, k), 5) for k in range(40)]
    b.add("mode_mix[wg1]", tail, at=0, facts={"modes": [WALK] + [SLOT if k % 2 else ACKS for k in range(40)],
                                              "item_first": wg0, "wg_items": 65 + 20 * 20 + 20 * 5})
    total = wg0 + 65 + 20 * 20 + 20 * 5
    # 0; 1; inside a slot frame (frame 0: items 0..2); inside a re-walked frame (frame 2: items 5..74); workgroup 1's
    # first item (a re-walked frame's first); inside that frame; inside a slot frame of workgroup 1 (frame 258: items
    # wg0 + 70 ..); exactly the total
    b.caps = [0, 1, 2, 40, wg0, wg0 + 30, wg0 + 72, total]
    b.total = total
    return b


def backward_offsets_case():
    """fallback_backward_offsets: workgroup 0's bytes lie behind workgroup 1's, so offsets[256] < offsets[0]: frame
    255 gets length 0, workgroup 0's span test fails and its 255 frames' items come through the byte loads.  Micro,
    small and large headers, ack groups, re-walked frames; the frame that ends the buffer's used bytes (frame 254)
    ends with a micro datagram with no payload.  Returns (batch, data, offsets, valid): valid is the oracle's (the
    gate is not under test with such offsets)."""
    b = Frames("fallback_backward_offsets")
    group = []
    for k in range(254):
        r = k % 5
        if r == 0:
            group.append((data_frame([micro(k, 3), small(k, 70), large(k, 300)], k), 3))
        elif r == 1:
            group.append((ack_frame(1 + k % 4, k), 1 + k % 4))
        elif r == 2:
            group.append((data_frame([large(k, 0), small(k, 0), micro(k)], k), 3))
        elif r == 3:
            group.append((micros(70, k), 70))
        else:
            group.append((filler(k), 0))
    group.append((data_frame([small(254, 5), micro(254)], 254), 2))
    group.append((b"", 0))  # frame 255: length 0 by the offsets
    b.add("fallback_backward_offsets", group, at=0, facts={"wg_frames": WG, "frame_bytes": [len(f) for f, _ in group]})
    b.add("workgroup_1", [(micros(2, k, 1), 2) if k % 2 else (ack_frame(2, k), 2) for k in range(60)], at=0)
    n = len(b.frames)
    offsets = np.zeros(n + 1, dtype=np.int64)
    parts, at = [], 0
    for i in list(range(WG, n)) + list(range(255)):
        offsets[i] = at
        parts.append(b.frames[i])
        at += len(b.frames[i])
        if i == n - 1:
            offsets[n] = at
    offsets[255] = at
    assert offsets[256] == 0 and offsets[256] < offsets[0] and offsets[255] - offsets[254] == len(b.frames[254])
    data = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    assert data.size == at and bytes(data[-10:-4])[0] & 0x80 == 0  # the buffer ends: a micro header, no payload, a trailer
    valid = np.array([1 if len(f) >= 5 and oracle.frame_validate(f)[0] else 0 for f in b.frames], dtype=np.uint8)
    return b, data, offsets, valid


def span_4gib_case(total_bytes, guard=16):
    """fallback_span_4gib: a hundred frames at the start of a buffer of total_bytes (over 4 GiB), one "frame" that
    the gate rejected from there to the last hundred frames, which end `guard` bytes before the buffer does.  Returns
    (batch, front bytes, back bytes, back offset, offsets, valid); the front bytes hold the first 16 bytes of the gap
    (the walk reads a rejected frame's first 8)."""
    b = Frames("fallback_span_4gib")
    front = [(ack_frame(1 + k % 3, k), 1 + k % 3) if k % 3 == 0 else
             (data_frame([micro(k), large(k, 20), micro(k + 1)], k), 3) if k % 3 == 1 else (micros(66, k), 66) for k in range(100)]
    back = [(data_frame([small(k, 9), micro(k)], k), 2) if k % 2 else (ack_frame(2, k), 2) for k in range(100)]
    b.add("front", front, at=0)
    b.add("gap", [(bytes([0x5A] * 16), 0)], facts={"modes": [NONE]})
    b.add("back", back, facts={"ends_batch": True, "wg_frames": 201})
    front_bytes = b"".join(f for f, _ in front) + bytes([0x5A] * 16)
    back_bytes = b"".join(f for f, _ in back)
    back_at = total_bytes - guard - len(back_bytes)
    assert back_at - len(front_bytes) > 0 and back_at + len(back_bytes) - 0 >= 2 ** 32
    offsets = np.zeros(202, dtype=np.int64)
    offsets[1:101] = np.cumsum([len(f) for f, _ in front])
    offsets[101] = back_at
    offsets[102:] = back_at + np.cumsum([len(f) for f, _ in back])
    valid = np.array([1] * 100 + [0] + [1] * 100, dtype=np.uint8)
    assert all(oracle.frame_validate(f)[0] for f, _ in front + back)
    return b, front_bytes, back_bytes, back_at, offsets, valid
