"""Inputs and expected outputs of the batched build (ufc_build_*_host / ufc_build_*_varlen), from the codec
oracle alone (test infrastructure, not a test module).

A `Batch` holds the records a build takes (infos, items, payload, src_base) and what the oracle says it
must give: per frame the bytes of oracle/codec.py `frame_write` (serial/mod.rs:437-657, build.rs) and the
status.  Records come from tests/parse_expect.oracle_records over oracle-written frames; cases that a
parse cannot produce (bad fields, a fragment_id under fragment_id_last == 0) alter those records by hand,
and their expected bytes are still `frame_write` of the frame they describe.
"""
import random

import numpy as np

import oracle
from oracle import codec as C
from parse_expect import oracle_records
from uflow_amd.frame import FRAME_INFO_DTYPE, ITEM_DTYPE

OK, SKIPPED, BAD_FIELD, BAD_SRC = 0, 1, 2, 3


class Batch:
    def __init__(self):
        self.infos, self.items, self.src, self.exp, self.status = [], [], [], [], []
        self.payload = bytearray()
        self.n_items = 0

    def add_sources(self, frames):
        """Source frames (bytes): records from the oracle's Frame::read, payload = the frames themselves,
        expected = frame_write(canonical(frame_read(fb))), SKIPPED where frame_read gives None."""
        infos, items = oracle_records(frames)
        infos = infos.copy()
        infos["item_first"] += self.n_items
        for i, fb in enumerate(frames):
            ref = C.frame_read(fb)
            self.infos.append(infos[i])
            self.src.append(len(self.payload))
            self.payload += fb
            self.exp.append(C.frame_write(C.canonical(ref)) if ref is not None else b"")
            self.status.append(OK if ref is not None else SKIPPED)
        self.items.extend(items)
        self.n_items += len(items)
        return self

    def add(self, f, status=OK, mutate=None, exp=None, payload=True, src=None):
        """A constructed frame dict: records of frame_write(f) read back; mutate(info, items) -> (info,
        items) alters them; expected = exp, else frame_write(f) (nothing unless status is OK).
        payload False: the frame's bytes are not appended, its source base is the previous frame's (the
        same frame again, or one that is rejected anyway); src: an explicit source base."""
        fb = C.frame_write(f)
        infos, items = oracle_records([fb])
        info, items = infos[0].copy(), items.copy()
        assert info["ok"] == 1
        if mutate is not None:
            info, items = mutate(info, items)
        info["item_first"] = self.n_items
        self.infos.append(info)
        self.items.extend(items)
        self.n_items += len(items)
        self.src.append(src if src is not None else len(self.payload) if payload else self.src[-1])
        if payload:
            self.payload += fb
        self.exp.append((exp if exp is not None else fb) if status == OK else b"")
        self.status.append(status)
        return self

    def arrays(self):
        infos = np.array(self.infos, dtype=FRAME_INFO_DTYPE) if self.infos else np.zeros(0, FRAME_INFO_DTYPE)
        items = np.array(self.items, dtype=ITEM_DTYPE) if self.items else np.zeros(0, ITEM_DTYPE)
        return (infos, items, np.frombuffer(bytes(self.payload), dtype=np.uint8).copy(),
                np.array(self.src, dtype=np.uint64))

    def expected(self, seal):
        """(bytes, offsets uint64[n + 1], status uint8[n]); seal False: trailers zeroed."""
        exp = [e if seal or not e else e[:-4] + bytes(4) for e in self.exp]
        offsets = np.zeros(len(exp) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(e) for e in exp], dtype=np.uint64)
        return np.frombuffer(b"".join(exp), dtype=np.uint8), offsets, np.array(self.status, dtype=np.uint8)

    def crcs(self):
        """oracle.compute of each written frame's body."""
        return [oracle.compute(e[:-4]) if e else None for e in self.exp]


def check_output(batch, seal, out, offsets, status):
    exp_bytes, exp_off, exp_status = batch.expected(seal)
    assert np.array_equal(np.asarray(status), exp_status), np.nonzero(np.asarray(status) != exp_status)[0][:8]
    assert np.array_equal(np.asarray(offsets).astype(np.uint64), exp_off), "offsets differ from the oracle's sizes"
    out = np.asarray(out)[:int(exp_off[-1])]
    if not np.array_equal(out, exp_bytes):
        pos = int(np.nonzero(out != exp_bytes)[0][0])
        f = int(np.searchsorted(exp_off, pos, side="right")) - 1
        raise AssertionError(f"byte {pos} (frame {f}, byte {pos - int(exp_off[f])} of {len(batch.exp[f])}) differs "
                             f"from the oracle: {out[pos]:#x} != {exp_bytes[pos]:#x}")


def rand_bytes(rng, n):
    return rng.randbytes(n)


def datagram(rng, t, data, **kw):
    """t: 0 micro-able leads, 1 wide leads, 2 fragment ids."""
    a, b = sorted((rng.getrandbits(16), rng.getrandbits(16)))
    d = dict(sequence_id=rng.getrandbits(20), channel_id=rng.randrange(64),
             window_parent_lead=rng.randrange(128) if t == 0 else rng.getrandbits(16),
             channel_parent_lead=rng.randrange(256) if t == 0 else rng.getrandbits(16),
             fragment_id=a if t == 2 else 0, fragment_id_last=max(b, 1) if t == 2 else 0, data=data)
    d.update(kw)
    return d


def data_frame(rng, dgs):
    return {"kind": "data", "sequence_id": rng.getrandbits(32), "nonce": bool(rng.getrandbits(1)), "datagrams": dgs}


def codec_frames(seed, n):
    """Seeded source frames of every kind, with damaged, unsealed and resealed ones among them (the parse
    test's mix, plus receive_side_data_frame and every fixed kind)."""
    rng = random.Random(seed)
    refs = [f for _, f in C.reference_test_frames()]
    frames = []
    for i in range(n):
        r = i % 8
        if r == 0:
            fb = C.frame_write(C.random_data_frame(rng, 24))
        elif r == 1:
            fb = C.frame_write(C.random_ack_frame(rng, 30))
        elif r == 2:
            fb = C.frame_write(C.random_sync_frame(rng))
        elif r == 3:  # a flipped bit: fails the gate
            fb = bytearray(C.frame_write(C.random_data_frame(rng, 8)))
            fb[rng.randrange(len(fb))] ^= 1 << rng.randrange(8)
        elif r == 4:  # damaged header, resealed: Frame::read may still accept it (non-canonical encodings)
            fb = bytearray(C.frame_write(C.random_data_frame(rng, 6)))
            fb[rng.randrange(min(len(fb) - 4, 30))] = rng.getrandbits(8)
            fb[-4:] = oracle.compute(bytes(fb[:-4])).to_bytes(4, "big")
        elif r == 5:
            fb = C.frame_write(refs[(i // 8) % len(refs)])
        elif r == 6:
            fb = C.frame_write(C.receive_side_data_frame(rng))
        else:  # unsealed (zero trailer) or truncated
            fb = bytearray(C.frame_write(C.random_data_frame(rng, 4)))
            fb = fb[:-4] + bytes(4) if i % 16 == 7 else fb[:rng.randrange(len(fb))]
        frames.append(bytes(fb))
    return frames


def _set_fragment_id(v):
    def m(info, items):
        items["fragment_id"] = v
        return info, items
    return m


def boundary_batch():
    """Header-form boundaries (build.rs:81-122) and count limits, one frame each, good frames between."""
    rng = random.Random(1234)
    b = Batch()
    sync = {"kind": "sync", "next_frame_id": 5, "next_packet_id": None}
    for dl in (0, 63, 64, 255, 256, 65535):
        for t in (0, 1):
            b.add(data_frame(rng, [datagram(rng, t, rand_bytes(rng, dl))]))
    for w in (127, 128):
        b.add(data_frame(rng, [datagram(rng, 0, rand_bytes(rng, 10), window_parent_lead=w)]))
    for h in (255, 256):
        b.add(data_frame(rng, [datagram(rng, 0, rand_bytes(rng, 10), channel_parent_lead=h)]))
    for last in (0, 1):
        b.add(data_frame(rng, [datagram(rng, 0, rand_bytes(rng, 10), fragment_id=0, fragment_id_last=last)]))
    # fragment_id != 0 under fragment_id_last == 0: dropped by the micro and small forms, kept by the large
    for dl in (10, 100, 300):
        d = datagram(rng, 0, rand_bytes(rng, dl))
        f = data_frame(rng, [d])
        g = dict(f, datagrams=[dict(d, fragment_id=7)])
        b.add(f, mutate=_set_fragment_id(7), exp=C.frame_write(g))
    b.add(sync)
    for cnt in (0, 127):
        b.add(data_frame(rng, [datagram(rng, k % 3, rand_bytes(rng, k % 5)) for k in range(cnt)]))

    def one_more(info, items):  # 128 datagrams
        info["item_count"] = 128
        return info, np.concatenate([items, items[:1]])
    b.add(data_frame(rng, [datagram(rng, 0, b"") for _ in range(127)]), status=BAD_FIELD, mutate=one_more)
    b.add(sync)
    for cnt in (0, 1, 162, 65535):
        b.add({"kind": "ack", "frame_window_base_id": 0x01020304 + cnt, "packet_window_base_id": 0xA0B0C0D0,
               "frame_acks": [{"base_id": (k * 2654435761) & 0xFFFFFFFF, "bitfield": k ^ 0xF0F0F0F0, "nonce": bool(k & 1)}
                              for k in range(cnt)]})

    def ack_one_more(info, items):  # 65536 groups
        info["item_count"] = 65536
        return info, np.concatenate([items, items[:1]])
    b.add({"kind": "ack", "frame_window_base_id": 1, "packet_window_base_id": 2,
           "frame_acks": [{"base_id": k, "bitfield": k, "nonce": False} for k in range(65535)]},
          status=BAD_FIELD, mutate=ack_one_more)
    b.add(sync)
    return b


def bad_input_batch():
    """Every UFC_BUILD_BAD_FIELD rule and UFC_BUILD_BAD_SRC, each between frames that must still come out
    right.  The last frames' payload ranges end at the payload's end (fine) and one byte past it."""
    rng = random.Random(4321)
    b = Batch()

    def good():
        b.add(data_frame(rng, [datagram(rng, k % 3, rand_bytes(rng, 3 + 40 * k)) for k in range(3)]))

    def info_set(**kw):
        def m(info, items):
            for k, v in kw.items():
                info[k] = v
            return info, items
        return m

    def item_set(**kw):
        def m(info, items):
            for k, v in kw.items():
                items[k][1] = v
            return info, items
        return m

    three = lambda: data_frame(rng, [datagram(rng, k, rand_bytes(rng, 20)) for k in range(3)])  # noqa: E731
    good()
    b.add(three(), status=SKIPPED, mutate=info_set(ok=0))
    good()
    for kind in (6, 9, 13, 255):  # unknown kinds
        b.add(three(), status=BAD_FIELD, mutate=info_set(kind=kind))
    good()
    b.add(three(), status=BAD_FIELD, mutate=info_set(aux=2))                 # data: nonce is 0/1
    b.add(three(), status=BAD_FIELD, mutate=item_set(channel_id=64))         # build.rs:74
    b.add(three(), status=BAD_FIELD, mutate=item_set(id=1 << 20))            # build.rs:75
    good()
    b.add(three(), status=BAD_FIELD, mutate=item_set(data_len=65536))        # build.rs:76
    b.add({"kind": "sync", "next_frame_id": 1, "next_packet_id": 2}, status=BAD_FIELD, mutate=info_set(aux=4))
    b.add({"kind": "handshake_error", "nonce_ack": 9, "error": "Config"}, status=BAD_FIELD, mutate=info_set(aux=3))
    good()
    b.add({"kind": "handshake_error", "nonce_ack": 9, "error": "ServerFull"})
    b.add({"kind": "sync", "next_frame_id": 1, "next_packet_id": 2})
    good()
    # payload ranges against the payload's end: x's bytes are the payload's last, its datagram's 50 bytes end
    # 4 bytes (the trailer) before it
    x = data_frame(rng, [datagram(rng, 1, rand_bytes(rng, 50))])
    xb = C.frame_write(x)
    b.add(x)
    stretched = dict(x, datagrams=[dict(x["datagrams"][0], data=xb[-54:])])
    b.add(x, payload=False, mutate=item_set_all(data_len=54), exp=C.frame_write(stretched))  # ends at payload_len
    b.add(x, payload=False, mutate=item_set_all(data_len=55), status=BAD_SRC)              # one byte past it
    b.add(x, payload=False)
    b.add(x, src=len(b.payload) + 5, payload=False, status=BAD_SRC)                         # base past the end
    b.add(x, src=len(b.payload) - len(xb), payload=False)
    # item_first + item_count > n_items: the batch's last items, one more than there are
    b.add(three(), payload=False, status=BAD_FIELD, mutate=info_set(item_count=4))
    return b


def item_set_all(**kw):
    def m(info, items):
        for k, v in kw.items():
            items[k] = v
        return info, items
    return m


# ---- table limits and caller-made layouts of the GPU write ----
#
# The write kernel's workgroup covers SPAN bytes of the output, cut by address; it stages the offsets, flags and
# infos of the frames that touch the span in LDS when there are at most TAB_FRAMES of them, and the destinations
# of their items when the window from the lowest first item to the highest last one is at most TAB_ITEMS.

SPAN = 16384       # kSpanBytes
TAB_FRAMES = 512   # kTabFrames
TAB_ITEMS = 1024   # kTabItems
GUARD = 0xA5


def _poison(n):
    """Item records no frame may name: every field out of range for an encoder."""
    p = np.zeros(n, dtype=ITEM_DTYPE)
    p["id"], p["channel_id"], p["form"], p["flags"] = 0xFFFFFFFF, 255, 9, 0xFFFF
    p["data_offset"], p["data_len"] = 0xFFFFFF00, 60000
    return p


class Placed:
    """Records with item placement of the caller's: add(frame dict, item_first) puts the frame's item records at
    item_first of an item array that is poison wherever no frame put anything.  Expected bytes: frame_write with a
    zero trailer (the raw write call, seal = 0)."""

    def __init__(self, name, n_items, lead=0, first_off=0):
        self.name, self.lead, self.first_off = name, lead, first_off
        self.items = _poison(n_items)
        self.named = np.zeros(n_items, dtype=bool)
        self.infos, self.src, self.exp = [], [], []
        self.payload = bytearray()
        self.facts = {}
        self.offsets = None  # the caller's offsets, where they are not the sizes' running sum

    def add(self, f, item_first, src=None):
        fb = C.frame_write(f)
        infos, items = oracle_records([fb])
        info = infos[0].copy()
        assert info["ok"] == 1
        k = len(items)
        if self.named[item_first:item_first + k].any():  # a frame that names records another frame put there
            assert self.named[item_first:item_first + k].all()
            assert self.items[item_first:item_first + k].tobytes() == items.tobytes()
        self.items[item_first:item_first + k] = items
        self.named[item_first:item_first + k] = True
        info["item_first"] = item_first
        self.infos.append(info)
        if src is None:
            src = len(self.payload)
            self.payload += fb
        self.src.append(src)
        self.exp.append(fb[:-4] + bytes(4))
        return len(self.infos) - 1

    def arrays(self):
        return (np.array(self.infos, dtype=FRAME_INFO_DTYPE), self.items,
                np.frombuffer(bytes(self.payload), dtype=np.uint8).copy(), np.array(self.src, dtype=np.uint64))

    def sizes(self):
        off = np.zeros(len(self.exp) + 1, dtype=np.int64)
        off[0] = self.first_off
        off[1:] = self.first_off + np.cumsum([len(e) for e in self.exp])
        return off

    def given_offsets(self):
        return self.sizes() if self.offsets is None else self.offsets


def span_frames(off, lead, blk):
    """(f_a, f_b) of workgroup span `blk` as the write kernel takes them from the check kernel's span owners, for an
    output at an address that is `lead` modulo 16 and in-order offsets `off`: the frame that holds the span's first
    byte, and the frame that holds the next span's first byte (the last frame where the batch ends before it)."""
    n = len(off) - 1
    a0 = (lead + int(off[0])) & ~15
    hi = lead + int(off[n])

    def owner(s):
        pos = max(a0 + s * SPAN, lead + int(off[0])) - lead
        return min(int(np.searchsorted(off, pos, side="right")) - 1, n - 1)
    assert a0 + blk * SPAN < hi
    return owner(blk), (owner(blk + 1) if a0 + (blk + 1) * SPAN < hi else n - 1)


def item_window(case, blk):
    off = case.sizes()
    f_a, f_b = span_frames(off, case.lead, blk)
    rows = [r for r in case.infos[f_a:f_b + 1] if r["kind"] == C.DATA and r["item_count"]]
    return max(int(r["item_first"]) + int(r["item_count"]) for r in rows) - min(int(r["item_first"]) for r in rows)


def check_table_facts(case):
    """The case's facts, from its own records and the oracle's frame sizes (never from a build's output)."""
    off = case.sizes()
    for key, want in case.facts.items():
        if key == "nf":          # {span: frames the kernel counts for it}
            got = {blk: span_frames(off, case.lead, blk)[1] - span_frames(off, case.lead, blk)[0] + 1 for blk in want}
        elif key == "touched":   # {span: frames with a byte in it}
            got = {}
            for blk in want:
                a0 = ((case.lead + int(off[0])) & ~15) - case.lead
                lo, hi = a0 + blk * SPAN, a0 + (blk + 1) * SPAN
                got[blk] = sum(1 for i in range(len(case.exp)) if off[i] < hi and off[i + 1] > lo)
        elif key == "item_window":
            got = {blk: item_window(case, blk) for blk in want}
        elif key == "frame_bytes":
            got = sorted({len(e) for e in case.exp})
        elif key == "same_items":  # groups of frames that name the same records
            got = [[(int(case.infos[i]["item_first"]), int(case.infos[i]["item_count"])) for i in g] for g in want]
            assert all(len(set(g)) == 1 and g[0][1] > 0 for g in got), got
            got = want
        elif key == "span_of":   # {frame: span that holds its first byte}
            got = {i: ((case.lead + int(off[i])) - ((case.lead + int(off[0])) & ~15)) // SPAN for i in want}
        elif key == "items_descend":
            firsts = [int(r["item_first"]) for r in case.infos]
            got = all(a >= b + int(r["item_count"]) for a, b, r in zip(firsts, firsts[1:], case.infos[1:]))
        elif key == "unnamed_items":
            got = int((~case.named).sum())
        elif key == "first_off":
            got = int(case.given_offsets()[0])
        elif key == "backward_steps":
            got = int((np.diff(case.given_offsets()) < 0).sum())
        else:
            raise AssertionError(f"unknown fact {key}")
        assert got == want, f"{case.name}: {key} is {got}, the case wants {want}"


def expected_region(case, length):
    """The output buffer's first `length` bytes after the write (in-order offsets): guard bytes, and each frame's
    bytes at its offset."""
    off = case.given_offsets()
    out = np.full(length, GUARD, dtype=np.uint8)
    for i, e in enumerate(case.exp):
        out[int(off[i]):int(off[i]) + len(e)] = np.frombuffer(e, dtype=np.uint8)
    return out


def check_backward_output(case, got):
    """offsets_backwards: nothing outside [offsets[0], offsets[n]) is touched; every byte inside is still the
    guard or the oracle's byte of a frame whose span holds it; frames whose spans lie wholly before the disorder
    are complete."""
    off = case.given_offsets()
    n = len(case.exp)
    lo, hi = int(off[0]), int(off[n])
    assert (got[:lo] == GUARD).all() and (got[hi:] == GUARD).all()
    allowed = got == GUARD
    for i, e in enumerate(case.exp):
        a, b = int(off[i]), int(off[i + 1])
        if b - a == len(e):
            allowed[a:b] |= got[a:b] == np.frombuffer(e, dtype=np.uint8)
    assert allowed.all(), f"{case.name}: bytes {np.nonzero(~allowed)[0][:8]} are neither guard nor a span's frame's"
    step = int(np.nonzero(np.diff(off) < 0)[0][0])  # offsets[step + 1] < offsets[step]
    floor = int(off[step + 1:].min())
    done = [i for i in range(step) if int(off[i + 1]) <= floor]
    assert len(done) >= 5
    for i in done:
        assert got[int(off[i]):int(off[i + 1])].tobytes() == case.exp[i], i
    return done


def table_cases():
    rng = random.Random(515)
    out = []
    # frames of 32 bytes: one micro datagram of 16 bytes.  The kernel's count for a span runs from the frame that
    # holds the span's first byte to the frame that holds the next span's first byte: with the output one byte past
    # a 16-byte boundary span 1 starts in frame 511's last byte (nf = 512 for span 0: staged), with an aligned
    # output it starts with frame 512 (nf = 513: the tables stay in global memory) though 512 frames touch span 0.
    for want, lead in ((512, 1), (513, 0)):
        c = Placed(f"frames_per_span[{want}]", 1100, lead=lead)
        for i in range(1100):
            c.add(data_frame(rng, [datagram(rng, 0, rand_bytes(rng, 16))]), i)
        c.facts = {"frame_bytes": [32], "nf": {0: want, 1: 513}, "touched": {0: 512}}
        out.append(c)
    # two data frames in one span whose items lie 1024 and 1025 records apart, poison between them
    for window in (1024, 1025):
        c = Placed(f"item_window[{window}]", window)
        c.add(data_frame(rng, [datagram(rng, k, rand_bytes(rng, 40 + k)) for k in range(3)]), 0)
        c.add(data_frame(rng, [datagram(rng, k, rand_bytes(rng, 30 + k)) for k in range(3)]), window - 3)
        c.facts = {"item_window": {0: window}, "nf": {0: 2}, "unnamed_items": window - 6}
        out.append(c)
    # a resent frame: two frames that name the same records, side by side and a span apart
    c = Placed("shared_items", 400)
    dgs = [datagram(rng, k % 3, rand_bytes(rng, 50 + 11 * k)) for k in range(5)]
    first = data_frame(rng, dgs)
    a = c.add(first, 7)
    b = c.add(dict(first, sequence_id=first["sequence_id"] ^ 0x55, nonce=not first["nonce"]), 7, src=c.src[a])
    at = 20
    for k in range(50):
        c.add(data_frame(rng, [datagram(rng, j % 3, rand_bytes(rng, 90 + j)) for j in range(4)]), at)
        at += 4
    d = c.add(dict(first, sequence_id=9), 7, src=c.src[a])
    c.facts = {"same_items": [[a, b, d]], "span_of": {a: 0, b: 0, d: 1}}
    out.append(c)
    # frame i's items lie behind frame i + 1's
    c = Placed("items_reversed", 200)
    at = 200
    for k in range(60):
        cnt = 1 + k % 4
        at -= cnt
        if k % 7 == 3:
            c.add({"kind": "ack", "frame_window_base_id": k, "packet_window_base_id": 2 * k, "frame_acks": [
                {"base_id": k + j, "bitfield": rng.getrandbits(32), "nonce": bool(j & 1)} for j in range(cnt)]}, at)
        else:
            c.add(data_frame(rng, [datagram(rng, j % 3, rand_bytes(rng, 100 + 30 * j + k)) for j in range(cnt)]), at)
    c.facts = {"items_descend": True, "span_of": {59: 1}}
    out.append(c)
    # the batch starts 37 bytes into the buffer (out_offsets[0] = 37), at output alignments 0..3
    for lead in range(4):
        c = Placed(f"lo_nonzero@{lead}", 240, lead=lead, first_off=37)
        for k in range(60):
            c.add(data_frame(rng, [datagram(rng, j % 3, rand_bytes(rng, 60 + 9 * j + k)) for j in range(4)]), 4 * k)
        c.facts = {"first_off": 37, "span_of": {59: 1}}
        out.append(c)
    # one backward step in the middle of 40 frames: frame 20 starts 500 bytes before frame 19 does
    c = Placed("offsets_backwards", 160)
    for k in range(40):
        c.add(data_frame(rng, [datagram(rng, j % 3, rand_bytes(rng, 30 + 7 * j + k)) for j in range(4)]), 4 * k)
    off = c.sizes()
    back = int(off[20] - off[19]) + 500
    off[20:] -= back
    c.offsets = off
    c.facts = {"backward_steps": 1}
    out.append(c)
    return out
