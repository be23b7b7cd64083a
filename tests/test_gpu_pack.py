"""GPU: the batched pack (ufc_pack_varlen, FrameCrcEngine.pack_flushes) against tests/pack_expect.py, the
emitters' push / finalize loop of src/half_connection/emit.rs restated item by item over the codec oracle's
encoded sizes; and end to end through the build, the gate and the parse."""
import ctypes
import random

import numpy as np
import pytest
import torch

from oracle import codec as C
from uflow_amd import _native
from uflow_amd.batch import PACK_TILE, records, rows
from uflow_amd.frame import FLUSH_DTYPE, FLUSH_RESULT_DTYPE, FRAME_INFO_DTYPE, ITEM_DTYPE

import pack_expect as PE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(items, first, flushes, nonce_bits=None):
    return (rows(items, DEV), rows(first.astype(np.int64), DEV), rows(flushes, DEV),
            rows(nonce_bits.view(np.int32), DEV) if nonce_bits is not None else None)


def _pack(engine, items, first, flushes, nonce_bits=None, **kw):
    d_items, d_first, d_flushes, d_nb = _dev(items, first, flushes, nonce_bits)
    infos, res, used = engine.pack_flushes(d_items, d_first, d_flushes, nonce_bits=d_nb, **kw)
    torch.cuda.synchronize()
    return infos.cpu().numpy(), res.cpu().numpy(), int(used.cpu()[0])


def _run(engine, batch, nonce_bits=None, **kw):
    items, first, flushes = batch.arrays()
    got = _pack(engine, items, first, flushes, nonce_bits, **kw)
    exp = PE.expect(items, first, flushes, nonce_bits)
    PE.check(got, exp, kw.get("frames_cap"))
    return got, exp, (items, first, flushes)


def test_single_cases(engine):
    b = PE.single_cases()
    got, exp, (items, _, _) = _run(engine, b)
    assert {PE.DONE, PE.SIZE_LIMITED, PE.WINDOW_LIMITED} == set(exp[1]["stop"])
    assert (got[0].view(FRAME_INFO_DTYPE).reshape(-1)[exp[2]:].view(np.uint8) == 0).all()  # unused rows stay zero
    _run(engine, b, nonce_bits=PE.nonce_words(3, items.size))


def test_flush_alloc_sweeps(engine):
    got, exp, (_, _, flushes) = _run(engine, PE.sweep_cases())
    assert set(exp[1]["frame_count"][flushes["kind"] == PE.DATA]) == {0, 1, 2, 3}
    assert set(exp[1]["frame_count"][flushes["kind"] == PE.ACK]) == {0, 1, 2}


def test_many_short_flushes(engine):
    """5000 flushes of 0..40 items: several flushes per workgroup, flush boundaries anywhere in a tile."""
    b = PE.random_batch(22, 5000, 40)
    items, _, _ = b.arrays()
    got, exp, _ = _run(engine, b, nonce_bits=PE.nonce_words(7, items.size))
    assert {PE.DONE, PE.SIZE_LIMITED, PE.WINDOW_LIMITED} == set(exp[1]["stop"])


def _long_batch():
    rng = random.Random(42)  # (a seed with which no frame of the mixed flush starts at a tile boundary)
    T = PACK_TILE
    n = 3 * T + T // 2  # three tiles and a half
    mixed = [PE.rand_dgram(rng) for _ in range(n)]
    sizes = [PE.encoded_size(d) for d in mixed]
    frames, _, _, _ = PE.pack_flush(sizes, PE.DATA, 1 << 40, 1 << 20)
    b = PE.Flushes()
    b.add(PE.DATA, [PE.rand_dgram(rng) for _ in range(7)])  # the long flushes start at no round index
    b.add(PE.DATA, mixed, id0=100)
    # cut by flush_alloc in the second tile, by the window in the last
    b.add(PE.DATA, mixed, flush_alloc=sum(sizes[:T + T // 3]), id0=200)
    b.add(PE.DATA, mixed, window_room=len(frames) - 2, id0=300)
    assert frames[len(frames) - 2][0] >= 3 * T
    b.add(PE.DATA, [PE.dgram(0, seq=k) for k in range(4 * T - 1)], id0=400)  # hops of 127
    b.add(PE.ACK, PE.rand_groups(rng, 3 * T + 5), id0=1, id1=2)               # hops of 161
    b.add(PE.ACK, PE.rand_groups(rng, 3 * T + 5), flush_alloc=15 * 2 + 9 * (T + 40), id0=3, id1=4)
    b.add(PE.DATA, [PE.dgram(3000 if k % 50 == 7 else 100, frag_last=1) for k in range(2 * T + 9)], id0=500)
    for m in (T - 1, T, T + 1, 2 * T, 2 * T + 1):  # flushes that end at, before and after a tile's end
        b.add(PE.DATA, [PE.rand_dgram(rng) for _ in range(m)], id0=600 + m)
    return b, frames


def test_flushes_longer_than_a_tile(engine):
    b, frames = _long_batch()
    T = PACK_TILE
    for m in (1, 2, 3):  # a frame straddles every tile boundary of the mixed flush
        assert any(s < m * T < s + c for s, c in frames), m
    got, exp, (_, first, _) = _run(engine, b)
    res = exp[1]
    assert res["stop"][2] == PE.SIZE_LIMITED and T < res["items_packed"][2] < 2 * T
    assert res["stop"][3] == PE.WINDOW_LIMITED and res["items_packed"][3] >= 3 * T
    assert res["stop"][6] == PE.SIZE_LIMITED and T < res["items_packed"][6] < 2 * T


def test_lane_63_slot_and_tile_seams(engine):
    """pack_expect.lane_cases on the device, without and with nonce bits: against the model, and record for
    record against what ufc_pack_host gave for the same batch."""
    from uflow_amd.frame import pack_host
    b = PE.lane_cases()
    items, first, flushes = b.arrays()
    for nb in (None, PE.nonce_words(63, items.size)):
        exp = PE.expect(items, first, flushes, nb)
        PE.check_facts(b, exp)
        got = _pack(engine, items, first, flushes, nb)
        PE.check(got, exp)
        h_infos, h_res, h_used = pack_host(items, first, flushes, nonce_bits=nb)
        assert got[2] == h_used == exp[2]
        assert got[1].view(FLUSH_RESULT_DTYPE).reshape(-1).tobytes() == h_res.tobytes()
        g_infos = got[0].view(FRAME_INFO_DTYPE).reshape(-1)[:h_used]
        for fld in FRAME_INFO_DTYPE.names:
            assert np.array_equal(g_infos[fld], h_infos[fld][:h_used]), fld
    b = PE.batch_end_case()  # the last prefix sum decides the hop of the hops workgroup's last thread
    _, exp, _ = _run(engine, b)
    PE.check_facts(b, exp)


def test_empty_ends_one_item_and_no_flushes(engine):
    rng = random.Random(8)
    b = PE.Flushes()
    for n in (0, 0, 5, 0, 0, 0, 40, 1, 0):  # first and last empty, and runs
        b.add(PE.DATA, [PE.rand_dgram(rng) for _ in range(n)], flush_alloc=-1 if n == 0 else 1 << 40)
    _run(engine, b)
    _run(engine, PE.Flushes().add(PE.DATA, [PE.dgram(17)]))
    _run(engine, PE.Flushes().add(PE.ACK, []))  # no items at all
    # n_flushes == 0: UFC_OK whatever the pointers
    assert _native.lib().ufc_pack_varlen(engine._ctx, None, 0, None, None, 0, None, None, 0, None, None, None) == 0
    infos, res, used = _pack(engine, np.zeros(0, ITEM_DTYPE), np.zeros(1, np.uint64), np.zeros(0, FLUSH_DTYPE))
    assert used == 0 and res.size == 0 and infos.size == 0


def test_argument_checks(engine):
    items, first, flushes = PE.Flushes().add(PE.DATA, [PE.dgram(1)]).arrays()
    d_items, d_first, d_flushes, _ = _dev(items, first, flushes)
    infos = torch.zeros((1, FRAME_INFO_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    res = torch.zeros((1, FLUSH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    used = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = [engine._ctx, p(d_items), 1, p(d_first), p(d_flushes), 1, None, p(infos), 1, p(res), p(used), None]
    assert _native.lib().ufc_pack_varlen(*good) == 0
    torch.cuda.synchronize()
    assert int(used.cpu()[0]) == 1
    for k in (0, 1, 3, 4, 7, 9, 10):  # ctx, items, flush_first, flushes, infos, results, frames_used
        bad = list(good)
        bad[k] = None
        assert _native.lib().ufc_pack_varlen(*bad) == _native.UFC_ERR_INVALID_ARG, k
    for k in (2, 5):  # n_items, n_flushes at 2^31 - 1
        bad = list(good)
        bad[k] = (1 << 31) - 1
        assert _native.lib().ufc_pack_varlen(*bad) == _native.UFC_ERR_INVALID_ARG, k


def test_bad_ranges_leave_neighbours_alone(engine):
    rng = random.Random(9)
    items = np.array([PE.rand_dgram(rng) for _ in range(60)], dtype=ITEM_DTYPE)
    # [0, 20), [20, 10) reversed, [10, 30), [30, 61) past n_items, [61, 61) past, [61, 2^40) past, [2^40, 40)
    # reversed, [40, 60)
    first = np.array([0, 20, 10, 30, 61, 61, 1 << 40, 40, 60], dtype=np.uint64)
    flushes = np.zeros(8, dtype=FLUSH_DTYPE)
    flushes["kind"], flushes["flush_alloc"], flushes["window_room"] = PE.DATA, 5000, 100
    flushes["id0"] = np.arange(8) * 1000
    got = _pack(engine, items, first, flushes)
    exp = PE.expect(items, first, flushes)
    PE.check(got, exp)
    assert list(exp[1]["stop"] == PE.BAD_RANGE) == [False, True, False, True, True, True, True, False]
    assert (exp[1]["frame_count"][[0, 2, 7]] > 0).all()


def test_frames_cap_and_guard(engine):
    """frames_cap below the need: the records below the cap are written, nothing behind it, the count is whole."""
    b = PE.random_batch(23, 300, 40)
    items, first, flushes = b.arrays()
    exp = PE.expect(items, first, flushes)
    cap = exp[2] // 2
    d_items, d_first, d_flushes, _ = _dev(items, first, flushes)
    infos = torch.full((cap + 64, FRAME_INFO_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=DEV)
    res = torch.zeros((flushes.size, FLUSH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    used = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = _native.lib().ufc_pack_varlen(engine._ctx, p(d_items), items.size, p(d_first), p(d_flushes), flushes.size, None,
                                       p(infos), cap, p(res), p(used), None)
    torch.cuda.synchronize()
    assert rc == 0
    h = infos.cpu().numpy()
    PE.check((h, res.cpu().numpy(), int(used.cpu()[0])), exp, frames_cap=cap)
    assert (h[cap:] == 0xA5).all(), "wrote past frames_cap"
    # through the wrapper, whose infos hold frames_cap rows
    got = _pack(engine, items, first, flushes, frames_cap=cap)
    assert got[0].shape[0] == cap
    PE.check(got, exp, frames_cap=cap)


def test_streams_and_scratch_growth(engine):
    """A non-default stream; a small batch, then a larger one on the same stream (its scratch grows), then the
    small one again."""
    small, large = PE.random_batch(24, 50, 20), PE.random_batch(25, 1500, 40)
    s = torch.cuda.Stream(device=DEV)
    outs = []
    for b in (small, large, small):
        items, first, flushes = b.arrays()
        d = _dev(items, first, flushes)
        s.wait_stream(torch.cuda.current_stream())
        outs.append((b, d, engine.pack_flushes(d[0], d[1], d[2], stream=s)))
    s.synchronize()
    for b, _, (infos, res, used) in outs:
        items, first, flushes = b.arrays()
        PE.check((infos.cpu().numpy(), res.cpu().numpy(), int(used.cpu()[0])), PE.expect(items, first, flushes))
    engine.release_stream(s)


def _frame_dict(info, items, payload):
    its = items[int(info["item_first"]):int(info["item_first"]) + int(info["item_count"])]
    if info["kind"] == PE.ACK:
        return {"kind": "ack", "frame_window_base_id": int(info["f"][0]), "packet_window_base_id": int(info["f"][1]),
                "frame_acks": [{"base_id": int(g["id"]), "bitfield": int(g["data_offset"]), "nonce": bool(g["channel_id"])}
                               for g in its]}
    return {"kind": "data", "sequence_id": int(info["f"][0]), "nonce": bool(info["aux"]),
            "datagrams": [PE.item_datagram(d, bytes(payload[int(d["data_offset"]):int(d["data_offset"]) + int(d["data_len"])]))
                          for d in its]}


def test_pack_build_seal_gate_parse(engine):
    """pack_flushes -> build_varlen(seal) -> crc_varlen -> parse_varlen: every frame valid, the datagrams the
    flushes' items in order up to items_packed, no frame over 1472 bytes but a lone oversize datagram's, and
    the bytes those of the oracle's frame_write of the frames pack_expect gives."""
    rng = random.Random(51)
    b = PE.random_batch(26, 400, 40)
    b.add(PE.DATA, [PE.rand_dgram(rng), PE.dgram(3000, frag_last=1), PE.rand_dgram(rng)], id0=9)
    b.add(PE.DATA, [PE.rand_dgram(rng) for _ in range(2 * PACK_TILE + 3)], id0=0xFFFFFFF0)
    items, first, flushes = b.arrays()
    is_ack = np.repeat(flushes["kind"] == PE.ACK, np.diff(first.astype(np.int64)))
    # payloads: one buffer, each datagram's bytes at its data_offset
    lens = np.where(is_ack, 0, items["data_len"]).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    payload = np.frombuffer(rng.randbytes(int(offs[-1])), dtype=np.uint8).copy()
    items["data_offset"] = np.where(is_ack, items["data_offset"], offs[:-1]).astype(np.uint32)
    nonce_bits = PE.nonce_words(9, items.size)
    e_infos, e_res, e_used = exp = PE.expect(items, first, flushes, nonce_bits)

    d_items, d_first, d_flushes, d_nb = _dev(items, first, flushes, nonce_bits)
    infos, res, used = engine.pack_flushes(d_items, d_first, d_flushes, nonce_bits=d_nb)
    d_payload = rows(payload, DEV)
    out, off, status = engine.build_varlen(infos, d_items, d_payload, seal=True)  # the infos as they are
    torch.cuda.synchronize()
    PE.check((infos.cpu().numpy(), res.cpu().numpy(), int(used.cpu()[0])), exp)
    n = e_used
    status, off_h = status.cpu().numpy(), off.cpu().numpy()
    assert (status[:n] == _native.UFC_BUILD_OK).all() and (status[n:] == _native.UFC_BUILD_SKIPPED).all()
    assert (np.diff(off_h)[n:] == 0).all()
    exp_frames = [C.frame_write(_frame_dict(e_infos[g], items, payload)) for g in range(n)]
    exp_off = np.concatenate([[0], np.cumsum([len(f) for f in exp_frames])])
    assert np.array_equal(off_h[:n + 1], exp_off)
    assert np.array_equal(out.cpu().numpy(), np.frombuffer(b"".join(exp_frames), dtype=np.uint8))
    flen = np.diff(exp_off)
    over = np.nonzero(flen > PE.MAX_FRAME_SIZE)[0]
    assert over.size == 1 and e_infos["item_count"][over[0]] == 1
    # the receive side
    d_off = off[:n + 1].contiguous()
    _, valid = engine.crc_varlen(out, d_off)
    infos2, items2, used2 = engine.parse_varlen(out, d_off, valid)
    torch.cuda.synchronize()
    assert (valid.cpu().numpy() == 1).all()
    i2 = records(infos2, FRAME_INFO_DTYPE)
    assert (i2["ok"] == 1).all() and np.array_equal(i2["item_count"], e_infos["item_count"])
    assert np.array_equal(i2["f"][:, 0], e_infos["f"][:, 0]) and np.array_equal(i2["aux"], e_infos["aux"])
    packed = np.concatenate([np.arange(int(first[j]), int(first[j]) + int(e_res["items_packed"][j]))
                             for j in range(flushes.size)])
    assert int(used2.cpu()[0]) == packed.size
    t2 = records(items2, ITEM_DTYPE)[:packed.size]
    src = items[packed]
    ack = is_ack[packed]
    for fld in ("id", "channel_id"):
        assert np.array_equal(t2[fld], src[fld]), fld
    assert np.array_equal(t2["data_offset"][ack], src["data_offset"][ack])  # bitfields
    for fld in ("window_parent_lead", "channel_parent_lead", "fragment_id", "fragment_id_last", "data_len"):
        assert np.array_equal(t2[fld][~ack], src[fld][~ack]), fld
