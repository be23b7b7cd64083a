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
