"""GPU: the batched build (ufc_build_sizes_varlen + ufc_build_batch_varlen, FrameCrcEngine.build_varlen)
against the codec oracle.  Expected bytes are always oracle/codec.py frame_write (tests/build_expect.py),
never the product's own host build and never the source bytes: Frame::read accepts non-canonical
encodings that re-encode differently."""
import ctypes
import random

import numpy as np
import pytest
import torch

import oracle
from oracle import codec as C
from parse_expect import compare, oracle_records
from uflow_amd import _native
from uflow_amd.batch import records, rows
from uflow_amd.frame import FRAME_INFO_DTYPE, ITEM_DTYPE, build_batch_host

import build_expect as BE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(batch):
    infos, items, payload, src = batch.arrays()
    return (rows(infos, DEV), rows(items, DEV), rows(payload, DEV),
            rows(src.astype(np.int64), DEV))


def _build_and_check(engine, batch, seal=True, **kw):
    infos, items, payload, src = _dev(batch)
    out, off, status = engine.build_varlen(infos, items, payload, src_base=src, seal=seal, **kw)
    torch.cuda.synchronize()
    BE.check_output(batch, seal, out.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy())
    return out, off, status


def test_codec_batch_roundtrip(engine):
    """Gate -> parse -> build with the parsed batch itself as the payload source (no copy in between):
    bytes, offsets and status against the oracle; then the built batch through the gate and the parse
    again: every written frame passes, and its records are the oracle's for the canonical frames and
    carry the first parse's field values."""
    frames = BE.codec_frames(9, 3000)
    offsets = np.zeros(len(frames) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(f) for f in frames])
    d = torch.from_numpy(np.frombuffer(b"".join(frames), dtype=np.uint8).copy()).to(DEV)
    o = torch.from_numpy(offsets).to(DEV)
    _, valid = engine.crc_varlen(d, o)
    infos, items, used = engine.parse_varlen(d, o, valid)
    n_items = int(used.cpu()[0])
    out, off, status = engine.build_varlen(infos, items, d, src_base=o, n_items=n_items)
    torch.cuda.synchronize()
    batch = BE.Batch().add_sources(frames)
    BE.check_output(batch, True, out.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy())
    written = np.array([len(e) > 0 for e in batch.exp])
    assert 2000 < written.sum() < len(frames)
    _, valid2 = engine.crc_varlen(out, off)
    infos2, items2, used2 = engine.parse_varlen(out, off, valid2)
    torch.cuda.synchronize()
    assert np.array_equal(valid2.cpu().numpy() != 0, written)
    assert int(used2.cpu()[0]) == n_items
    i1 = records(infos, FRAME_INFO_DTYPE)
    i2 = records(infos2, FRAME_INFO_DTYPE)
    t1 = records(items, ITEM_DTYPE)[:n_items]
    t2 = records(items2, ITEM_DTYPE)[:n_items]
    exp_infos, exp_items = oracle_records(batch.exp)
    compare(i2, t2, exp_infos, exp_items)
    # against the first parse: the infos whole (item_first too: the same frames are accepted); of the items
    # what a re-encode keeps (form, data_offset and a fragment_id under fragment_id_last == 0 may change)
    assert np.array_equal(i2[written], i1[written])
    for fld in ("id", "channel_id", "window_parent_lead", "channel_parent_lead", "fragment_id_last", "data_len"):
        assert np.array_equal(t2[fld], t1[fld]), fld


def _edge_frames(seed):
    """The parse edge mix: data frames with 65..127 micro datagrams, frames of 3 x 20-30 KB datagrams
    between tiny frames, acks with 0..161 groups, syncs and handshake_syn, rejected frames first, last
    and in runs."""
    rng = random.Random(seed)
    syn = {"kind": "handshake_syn", "version": 3, "nonce": 1, "max_receive_rate": 2, "max_packet_size": 3,
           "max_receive_alloc": 0xFFFFFFFF}
    frames = []
    for i in range(420):
        r = i % 7
        if r == 0:
            f = BE.data_frame(rng, [BE.datagram(rng, 0, BE.rand_bytes(rng, rng.randrange(3)))
                                    for _ in range(rng.randrange(65, 128))])
        elif r == 1 and i % 35 == 1:
            f = BE.data_frame(rng, [BE.datagram(rng, 2, BE.rand_bytes(rng, rng.randrange(20000, 30000))) for _ in range(3)])
        elif r == 1:
            f = {"kind": "disconnect"}
        elif r == 2:
            f = C.random_ack_frame(rng, 162)
        elif r == 3:
            f = C.random_data_frame(rng, 64)
        elif r == 4:
            f = C.random_sync_frame(rng)
        elif r == 5:
            f = syn if i % 14 == 5 else {"kind": "handshake_ack", "nonce_ack": rng.getrandbits(32)}
        else:
            f = C.random_data_frame(rng, 128, 70)
        fb = bytearray(C.frame_write(f))
        if i in (0, 419) or i % 11 == 5 or 200 <= i < 212:  # rejected: first, last, singles, a run
            fb[rng.randrange(len(fb))] ^= 1 << rng.randrange(8)
        frames.append(bytes(fb))
    return frames


def test_every_kernel_path(engine):
    frames = _edge_frames(31)
    batch = BE.Batch().add_sources(frames)
    assert batch.status[0] == batch.status[-1] == BE.SKIPPED and all(s == BE.SKIPPED for s in batch.status[200:212])
    assert max(len(e) for e in batch.exp) > 60000  # frames longer than a workgroup's span
    _build_and_check(engine, batch, seal=True)
    _build_and_check(engine, batch, seal=False)
    # more frames (tiny ones, and length-0 rejected ones) and more items (micro datagrams) in a workgroup's
    # 16-KiB span than its LDS tables hold (512 frames, 1024 items): the tables stay in global memory
    rng = random.Random(32)
    tiny = []
    for i in range(9000):
        f = ({"kind": "disconnect"}, {"kind": "disconnect_ack"}, {"kind": "handshake_ack", "nonce_ack": i},
             C.random_sync_frame(rng))[i % 4]
        fb = bytearray(C.frame_write(f))
        if i % 5 == 2:
            fb[0] ^= 0x40
        tiny.append(bytes(fb))
    dense = [C.frame_write(BE.data_frame(rng, [BE.datagram(rng, 0, BE.rand_bytes(rng, k % 2)) for k in range(127)]))
             for _ in range(60)]
    crowded = BE.Batch().add_sources(tiny + dense + tiny[:700])
    assert sum(len(e) for e in crowded.exp[:9000]) / 16384 * 512 < 9000  # over 512 frames per span on average
    _build_and_check(engine, crowded, seal=True)
    # a batch in which every frame is rejected: nothing to write, the output is empty
    dead = BE.Batch().add_sources([bytes(f[:-1]) + bytes([f[-1] ^ 1]) for f in frames[:50]])
    out, off, status = _build_and_check(engine, dead, seal=True)
    assert out.numel() == 0 and int(off[-1]) == 0 and (status.cpu().numpy() == BE.SKIPPED).all()


def test_alignment_sweep(engine):
    """The payload at pool[s:], s = 0..15, the output at big[64 + 3 + t:], t = 0..3; datagrams of 0..40
    bytes put a piece boundary at every byte position of headers and payloads.  64 guard bytes on either
    side of the output stay as they were."""
    rng = random.Random(77)
    batch = BE.Batch()
    lens = list(range(41))
    for i in range(24):
        rng.shuffle(lens)
        batch.add(BE.data_frame(rng, [BE.datagram(rng, k % 3, BE.rand_bytes(rng, dl)) for k, dl in enumerate(lens[:9 + i % 5])]))
        if i % 5 == 0:
            batch.add(C.random_ack_frame(rng, 7))
    infos, items, payload, src = _dev(batch)
    exp_bytes, exp_off, _ = batch.expected(True)
    total = int(exp_off[-1])
    pool = torch.zeros(payload.numel() + 16, dtype=torch.uint8, device=DEV)
    big = torch.empty(64 + 3 + 3 + total + 64, dtype=torch.uint8, device=DEV)
    for s in range(16):
        pool[s:s + payload.numel()] = payload
        for t in range(4):
            big.fill_(0xA5)
            a = 64 + 3 + t
            out, off, status = engine.build_varlen(infos, items, pool[s:s + payload.numel()], src_base=src,
                                                   out=big[a:a + total])
            torch.cuda.synchronize()
            got = big.cpu().numpy()
            assert np.array_equal(got[a:a + total], exp_bytes), (s, t)
            assert (got[:a] == 0xA5).all() and (got[a + total:] == 0xA5).all(), (s, t)


def _raw_write(engine, infos, items, n_items, src, payload, off, out, out_len, seal, crc=None):
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    return _native.lib().ufc_build_batch_varlen(engine._ctx, p(infos), p(items), n_items, p(src), p(payload),
                                                payload.numel(), infos.shape[0], p(off), p(out), out_len, seal, p(crc),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_skip_rule(engine):
    """The write call alone, with offsets of the caller's: a span whose length disagrees with the frame's
    size is left untouched (a guard pattern shows it), the frames on both sides are written, and a frame
    that would end past out_len is not written; nothing beyond out_len is touched."""
    rng = random.Random(5)
    batch = BE.Batch()
    for k in range(40):
        batch.add(BE.data_frame(rng, [BE.datagram(rng, j % 3, BE.rand_bytes(rng, 30 + 7 * j + k)) for j in range(4)]))
    infos, items, payload, src = _dev(batch)
    exp, eoff, _ = batch.expected(False)
    off = eoff.astype(np.int64)
    victims = (0, 17, 18, 30)
    for v in victims:
        off[v + 1:] += 1 if v != 18 else 3
    d_off = torch.from_numpy(off).to(DEV)
    total = int(off[-1])
    big = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    assert _raw_write(engine, infos, items, items.shape[0], src, payload, d_off, big, total, 0) == 0
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    for i in range(40):
        span = got[off[i]:off[i + 1]]
        if i in victims:
            assert (span == 0xA5).all(), i
        else:
            assert np.array_equal(span, exp[int(eoff[i]):int(eoff[i + 1])]), i
    assert (got[total:] == 0xA5).all()
    # out_len inside the last frame: every frame but that one
    big.fill_(0xA5)
    cut = int(off[-1]) - 2
    assert _raw_write(engine, infos, items, items.shape[0], src, payload, d_off, big, cut, 0) == 0
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert (got[off[39]:] == 0xA5).all()
    assert np.array_equal(got[off[38]:off[39]], exp[int(eoff[38]):int(eoff[39])])


@pytest.mark.parametrize("case", BE.table_cases(), ids=lambda c: c.name)
def test_table_cases(engine, case):
    """The write call alone on build_expect.table_cases: 512 and 513 frames counted for a span
    (the LDS tables' switch), item windows of 1024 and 1025 records with poison between the frames' items, frames
    that name the same records, items in reverse frame order, a batch that starts 37 bytes into the buffer at
    output alignments 0..3, and offsets with one backward step.  Expected bytes are frame_write's; 64 guard bytes
    before the output and everything behind the batch stay as they were.  The output pointer sits `lead` bytes past
    a 16-byte boundary."""
    BE.check_table_facts(case)
    infos, items, payload, src = case.arrays()
    off = case.given_offsets()
    total = int(off.max())
    d_infos, d_items, d_payload = rows(infos, DEV), rows(items, DEV), rows(payload, DEV)
    d_src, d_off = rows(src.astype(np.int64), DEV), torch.from_numpy(off.astype(np.int64)).to(DEV)
    big = torch.full((64 + case.lead + total + 64,), BE.GUARD, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    out = big[64 + case.lead:]
    assert _raw_write(engine, d_infos, d_items, items.size, d_src, d_payload, d_off, out, total, 0) == 0
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert (got[:64 + case.lead] == BE.GUARD).all()
    got = got[64 + case.lead:]
    if case.name == "offsets_backwards":
        BE.check_backward_output(case, got)
        # the host write, for the record: both keep the documented bounds; where spans overlap the host writes every
        # frame whose span matches, the device only the bytes whose frame its search finds
        h = np.full(got.size, BE.GUARD, dtype=np.uint8)
        o64 = off.astype(np.uint64)
        assert _native.lib().ufc_build_batch_host(infos.ctypes.data, items.ctypes.data, items.size, src.ctypes.data,
                                                  payload.ctypes.data, payload.size, infos.size, o64.ctypes.data,
                                                  h.ctypes.data, total, 0, None, 1) == 0
        BE.check_backward_output(case, h)
        print(f"offsets_backwards: device and host writes {'agree' if np.array_equal(h, got) else 'differ'}; "
              f"{int((h != got).sum())} bytes differ, {int((got == BE.GUARD).sum())} device bytes left as guard")
    else:
        assert np.array_equal(got, BE.expected_region(case, got.size))


def test_seal_and_status(engine):
    """seal=False leaves zero trailers; seal=True with crc_out gives oracle.compute of each body; the
    statuses of the bad-input records equal the host build's (and the oracle's expectations)."""
    batch = BE.bad_input_batch()
    infos, items, payload, src = _dev(batch)
    n = infos.shape[0]
    crc = torch.zeros(n, dtype=torch.int32, device=DEV)
    out, off, status = engine.build_varlen(infos, items, payload, src_base=src, seal=True, crc_out=crc)
    torch.cuda.synchronize()
    BE.check_output(batch, True, out.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy())
    words = crc.cpu().numpy().view(np.uint32)
    for i, c in enumerate(batch.crcs()):
        if c is not None:
            assert int(words[i]) == c, i
    _build_and_check(engine, batch, seal=False)
    h = batch.arrays()
    _, h_off, h_status, _ = build_batch_host(h[0], h[1], h[2], h[3])
    assert np.array_equal(status.cpu().numpy(), h_status)
    assert np.array_equal(off.cpu().numpy().astype(np.uint64), h_off)


def test_source_base_beyond_4gib(engine):
    """The payload buffer is 2^32 + 4096 bytes of which only the last 4096 are filled; src_base points
    into them (64-bit source offsets)."""
    rng = random.Random(11)
    batch = BE.Batch()
    for k in range(6):
        batch.add(BE.data_frame(rng, [BE.datagram(rng, j % 3, BE.rand_bytes(rng, 17 * j + k)) for j in range(5)]))
    infos, items, payload, src = _dev(batch)
    assert payload.numel() <= 4096
    big = torch.empty(2 ** 32 + 4096, dtype=torch.uint8, device=DEV)
    at = big.numel() - payload.numel()
    big[at:] = payload
    out, off, status = engine.build_varlen(infos, items, big, src_base=src + at)
    torch.cuda.synchronize()
    BE.check_output(batch, True, out.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy())
    del big


def test_two_streams_release_and_empty(engine):
    """Two streams build different batches at once (the scratch is per stream), then release_stream;
    n == 0 returns UFC_OK whatever the pointers."""
    batches = [BE.Batch().add_sources(BE.codec_frames(21 + k, 800 + 300 * k)) for k in range(2)]
    dev = [_dev(b) for b in batches]
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    outs = [None, None]
    for rep in range(3):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                infos, items, payload, src = dev[k]
                outs[k] = engine.build_varlen(infos, items, payload, src_base=src, stream=streams[k])
    for s in streams:
        s.synchronize()
    for k in range(2):
        out, off, status = outs[k]
        BE.check_output(batches[k], True, out.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy())
    for s in streams:
        engine.release_stream(s)
    lib = _native.lib()
    cur = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ufc_build_sizes_varlen(engine._ctx, None, None, 0, None, 0, 0, None, None, cur) == 0
    assert lib.ufc_build_batch_varlen(engine._ctx, None, None, 0, None, None, 0, 0, None, None, 0, 1, None, cur) == 0
    none = torch.empty((0, FRAME_INFO_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    out, off, status = engine.build_varlen(none, torch.empty((0, ITEM_DTYPE.itemsize), dtype=torch.uint8, device=DEV),
                                           torch.empty(0, dtype=torch.uint8, device=DEV))
    assert out.numel() == 0 and off.cpu().tolist() == [0] and status.numel() == 0
    assert lib.ufc_build_sizes_varlen(engine._ctx, None, None, 0, None, 0, 5, None, None, cur) == _native.UFC_ERR_INVALID_ARG


def test_boundaries_on_device(engine):
    """The CPU test's header-form and count boundaries through the device path."""
    b = BE.boundary_batch()
    _build_and_check(engine, b, seal=True)
    _build_and_check(engine, b, seal=False)
