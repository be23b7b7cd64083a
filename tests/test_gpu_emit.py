"""GPU: the batched packet emit (ufc_emit_packets_varlen, FrameCrcEngine.emit_packets) against
tests/emit_expect.py, PacketSender::emit_packet and PendingPacket of src/half_connection restated packet by
packet; and the whole send path on the device, emit -> pack -> build -> seal -> gate -> parse."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import codec as C
from uflow_amd import _native
from uflow_amd.batch import EMIT_TILE, records, rows
from uflow_amd.frame import FLUSH_DTYPE, FRAME_INFO_DTYPE, ITEM_DTYPE, PACKET_DTYPE, SENDER_DTYPE

import emit_expect as EE
import pack_expect as PE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(packets, first, senders):
    return (rows(packets, DEV), rows(first.astype(np.int64), DEV),
            rows(senders, DEV))


def _host(out):
    items, ff, pres, sres, sout, used = out
    return (items.cpu().numpy(), ff.cpu().numpy(), pres.cpu().numpy() if pres is not None else None, sres.cpu().numpy(),
            sout.cpu().numpy(), int(used.cpu()[0]))


def _emit(engine, packets, first, senders, exp=None, items_cap=None, slack=16, stream=None, **kw):
    """The device emit into items pre-filled with EE.FILL, checked against the expectation."""
    exp = EE.expect(packets, first, senders) if exp is None else exp
    cap = exp.items_used + slack if items_cap is None else items_cap
    d = _dev(packets, first, senders)
    items = torch.full((max(cap, exp.items_used) + slack, ITEM_DTYPE.itemsize), EE.FILL, dtype=torch.uint8, device=DEV)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    out = engine.emit_packets(*d, items_cap=cap, items=items, stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = _host(out)
    EE.check(got, exp, items_cap=cap)
    return got, exp


def test_tile_constant():
    assert EMIT_TILE == 64  # emit_expect.tile_cases is laid out for it


def test_reference_and_edge_cases(engine):
    b, want = EE.reference_cases()
    _emit(engine, *b.arrays())
    b = EE.edge_cases()
    (items, ff, pres, sres, sout, used), exp = _emit(engine, *b.arrays())
    assert {EE.DONE, EE.WINDOW_LIMITED, EE.ALLOC_LIMITED, EE.BAD_PACKET} == set(exp.sender_results["stop"])
    _emit(engine, *b.arrays(), exp=exp, want_packet_results=False)


def test_parent_leads_acknowledgement(engine):
    """Acknowledge + emit rounds with the ids wrapping on the way, the state carried in place on the device
    (senders_out == senders) between the helper's acknowledgements."""
    start = (1 << 20) - 7 * 20 - 3
    tx = EE.Tx(EE.MAX_PACKET_WINDOW_SIZE, start, 10000)
    q = [EE.pkt(4, ch, mode) for ch, mode in EE.ACK_ROUND]
    for i in range(40):
        tx.acknowledge((start + 7 * i) & EE.ID_MASK)
        packets, first, senders = EE.Senders().add(q, tx=tx, flush_id=i).arrays()
        exp = EE.expect(packets, first, senders, txs=[tx])
        d_packets, d_first, d_senders = _dev(packets, first, senders)
        out = engine.emit_packets(d_packets, d_first, d_senders, items_cap=7, senders_out=d_senders)
        torch.cuda.synchronize()
        assert out[4] is d_senders
        EE.check(_host(out), exp)
        assert [int(x) for x in exp.items["id"]] == [(start + 7 * i + k) & EE.ID_MASK for k in range(7)]


def test_tile_cases(engine):
    b = EE.tile_cases(EMIT_TILE)
    packets, first, senders = b.arrays()
    (_, _, _, sres, _, _), exp = _emit(engine, packets, first, senders)
    assert sres.view(EE.SENDER_RESULT_DTYPE)["packets_consumed"][b.index("alloc_stop_tile_3")] == 2 * EMIT_TILE + 16
    # in place, and with fewer item slots than items
    d = _dev(packets, first, senders)
    for cap in (0, exp.items_used // 2):
        state = d[2].clone()
        items = torch.full((exp.items_used + 8, ITEM_DTYPE.itemsize), EE.FILL, dtype=torch.uint8, device=DEV)
        out = engine.emit_packets(d[0], d[1], state, items_cap=cap, items=items, senders_out=state)
        torch.cuda.synchronize()
        EE.check(_host(out), exp, items_cap=cap)


def test_lane_63_and_tile_seam(engine):
    """emit_expect.lane_cases on the device into items pre-filled with EE.FILL (reserved slots stay untouched):
    as it is, in place (senders_out == senders), and without packet results."""
    b = EE.lane_cases(EMIT_TILE)
    packets, first, senders = b.arrays()
    (_, _, _, sres, _, _), exp = _emit(engine, packets, first, senders)
    EE.check_facts(b, exp)
    d = _dev(packets, first, senders)
    state = d[2].clone()
    items = torch.full((exp.items_used + 8, ITEM_DTYPE.itemsize), EE.FILL, dtype=torch.uint8, device=DEV)
    out = engine.emit_packets(d[0], d[1], state, items_cap=exp.items_used, items=items, senders_out=state)
    torch.cuda.synchronize()
    assert out[4] is state
    EE.check(_host(out), exp)
    _emit(engine, packets, first, senders, exp=exp, want_packet_results=False)


def test_finish_form_switch(engine):
    """The lane cases padded with empty senders until n_packets == 16 * n_senders (emit_finish_kernel<8>), and
    with one empty sender fewer (<64>): both the model's, every EMITTED record's absolute item_first included."""
    b = EE.lane_cases(EMIT_TILE)
    packets, first, senders = b.arrays()
    m = packets.size
    assert m % 16 == 0 and m // 16 - 1 >= senders.size
    exp = EE.expect(packets, first, senders)
    consumed = exp.sender_results["packets_consumed"]
    assert (consumed > 64).any() and (consumed == 8).any() and (consumed == 9).any()
    assert (exp.packet_results["status"] == EE.EMITTED).sum() > 1000 and exp.packet_results["item_first"].max() > 4000
    for n in (m // 16, m // 16 - 1):
        p2, f2, s2 = EE.with_empty_senders(packets, first, senders, n)
        assert (p2.size <= 16 * s2.size) == (n == m // 16)  # the switch's condition (packet_emit.hip, emit_batch)
        _emit(engine, p2, f2, s2)
        _emit(engine, p2, f2, s2, want_packet_results=False)


def test_max_packet(engine):
    """A MAX_PACKET_SIZE packet: 65 536 items of one packet, written by many workgroups."""
    b = EE.big_case()
    (items, *_), exp = _emit(engine, *b.arrays())
    assert exp.items_used == 1 + 1 + 65536 + 1


def test_random_batch(engine):
    _emit(engine, *EE.random_batch(31).arrays())


def test_many_short_senders(engine):
    """3000 senders of 0..11 packets: several senders per workgroup, the item kernel's sender search over
    many short and empty ranges."""
    _emit(engine, *EE.random_batch(32, 3000, 0).arrays())


def test_bad_ranges_empty_and_no_senders(engine):
    packets, _, senders = EE.random_batch(3, 8, 30).arrays()
    n = packets.size
    c1, c2, c3 = n // 5, n // 3, n // 2
    first = np.array([1 << 40, 0, c1, n + 1, 1 << 40, c1, c2, c2, c3], dtype=np.uint64)
    senders = senders[:8].copy()
    senders["reserve_items"] = 2
    (_, _, pres, sres, _, _), exp = _emit(engine, packets, first, senders)
    assert list(exp.sender_results["stop"] == EE.BAD_RANGE) == [True, False, True, True, True, False, False, False]
    # n_senders == 0: UFC_OK whatever the pointers
    lib = _native.lib()
    assert lib.ufc_emit_packets_varlen(engine._ctx, None, 0, None, None, 0, None, 0, None, None, None, None, None, None) == 0
    out = engine.emit_packets(*_dev(np.zeros(0, PACKET_DTYPE), np.zeros(1, np.uint64), np.zeros(0, SENDER_DTYPE)), items_cap=0)
    torch.cuda.synchronize()
    assert int(out[5].cpu()[0]) == 0
    # senders without packets at all
    _emit(engine, *EE.Senders().add([], reserve_items=3).add([]).arrays())


def test_argument_checks(engine):
    packets, first, senders = EE.Senders().add([EE.pkt(1)]).arrays()
    d = _dev(packets, first, senders)
    items = torch.zeros((1, ITEM_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    ff = torch.zeros(2, dtype=torch.int64, device=DEV)
    sres = torch.zeros((1, EE.SENDER_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    used = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = [engine._ctx, p(d[0]), 1, p(d[1]), p(d[2]), 1, p(items), 1, p(ff), None, p(sres), None, p(used), None]
    lib = _native.lib()
    assert lib.ufc_emit_packets_varlen(*good) == 0
    torch.cuda.synchronize()
    assert int(used.cpu()[0]) == 1
    for k in (0, 1, 3, 4, 6, 8, 10, 12):  # ctx, packets, packet_first, senders, items, flush_first, results, used
        bad = list(good)
        bad[k] = None
        assert lib.ufc_emit_packets_varlen(*bad) == _native.UFC_ERR_INVALID_ARG, k
    for k in (2, 5):  # n_packets, n_senders at 2^31 - 1
        bad = list(good)
        bad[k] = (1 << 31) - 1
        assert lib.ufc_emit_packets_varlen(*bad) == _native.UFC_ERR_INVALID_ARG, k


def test_streams_and_scratch_reuse(engine):
    """A non-default stream; a large batch, then a smaller one back to back on the same stream (the scratch of
    the first is reused), checked after both."""
    large, small = EE.random_batch(33, 400, 100), EE.random_batch(34, 20, 30)
    s = torch.cuda.Stream(device=DEV)
    outs = []
    s.wait_stream(torch.cuda.current_stream())
    for b in (large, small):
        packets, first, senders = b.arrays()
        exp = EE.expect(packets, first, senders)
        d = _dev(packets, first, senders)
        items = torch.full((exp.items_used, ITEM_DTYPE.itemsize), EE.FILL, dtype=torch.uint8, device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        outs.append((exp, d, engine.emit_packets(*d, items_cap=exp.items_used, items=items, stream=s)))
    s.synchronize()
    for exp, _, out in outs:
        EE.check(_host(out), exp)
    engine.release_stream(s)


def test_emit_pack_build_seal_gate_parse(engine):
    """emit_packets -> pack_flushes -> build_varlen(seal) -> crc_varlen -> parse_varlen, a few dozen senders with
    random payload bytes: every frame the oracle's frame_write of the expected datagrams, every frame through the
    gate, the parsed items the emitted ones in every field but data_offset, and each packet's fragments'
    payloads, concatenated, the packet's bytes."""
    b = EE.random_batch(35, 48, 40)
    packets, first, senders = b.arrays()
    senders["reserve_items"] = 0  # (reserved slots hold the caller's items; there are none here)
    rng = np.random.default_rng(35)
    payload = np.frombuffer(rng.bytes(max(b.arena, 1)), dtype=np.uint8).copy()
    exp = EE.expect(packets, first, senders)
    n = senders.size
    flushes = np.zeros(n, dtype=FLUSH_DTYPE)
    flushes["kind"], flushes["flush_alloc"], flushes["window_room"] = PE.DATA, 1 << 40, 1 << 20
    flushes["id0"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    e_infos, e_res, e_frames = PE.expect(exp.items, exp.flush_first, flushes)
    assert e_frames > n and (exp.packet_results["item_count"] > 1).any()

    d_packets, d_first, d_senders = _dev(packets, first, senders)
    items, ff, pres, sres, sout, used = engine.emit_packets(d_packets, d_first, d_senders, items_cap=exp.items_used)
    infos, res, frames_used = engine.pack_flushes(items, ff, rows(flushes, DEV))
    d_payload = rows(payload, DEV)
    out, off, status = engine.build_varlen(infos, items, d_payload, seal=True)
    torch.cuda.synchronize()
    EE.check(_host((items, ff, pres, sres, sout, used)), exp)
    PE.check((infos.cpu().numpy(), res.cpu().numpy(), int(frames_used.cpu()[0])), (e_infos, e_res, e_frames))
    want = []
    for info in e_infos:
        its = exp.items[int(info["item_first"]):int(info["item_first"]) + int(info["item_count"])]
        dgs = [PE.item_datagram(d, bytes(payload[int(d["data_offset"]):int(d["data_offset"]) + int(d["data_len"])]))
               for d in its]
        want.append(C.frame_write({"kind": "data", "sequence_id": int(info["f"][0]), "nonce": False, "datagrams": dgs}))
    want_off = np.concatenate([[0], np.cumsum([len(f) for f in want])])
    assert np.array_equal(off.cpu().numpy()[:e_frames + 1], want_off)
    assert np.array_equal(out.cpu().numpy(), np.frombuffer(b"".join(want), dtype=np.uint8))
    assert (status.cpu().numpy()[:e_frames] == _native.UFC_BUILD_OK).all()
    # the receive side
    d_off = off[:e_frames + 1].contiguous()
    _, valid = engine.crc_varlen(out, d_off)
    infos2, items2, used2 = engine.parse_varlen(out, d_off, valid)
    torch.cuda.synchronize()
    assert (valid.cpu().numpy() == 1).all()
    i2 = records(infos2, FRAME_INFO_DTYPE)
    assert (i2["ok"] == 1).all()
    assert int(used2.cpu()[0]) == exp.items_used
    t2 = records(items2, ITEM_DTYPE)[:exp.items_used]
    for fld in ITEM_DTYPE.names:
        if fld != "data_offset":
            assert np.array_equal(t2[fld], exp.items[fld]), fld
    # each packet's bytes back from the frames
    wire = out.cpu().numpy()
    frame_of = np.repeat(np.arange(e_frames), i2["item_count"].astype(np.int64))
    for k in np.nonzero(exp.packet_results["status"] == EE.EMITTED)[0]:
        pr, pk = exp.packet_results[k], packets[k]
        parts = []
        for g in range(int(pr["item_first"]), int(pr["item_first"]) + int(pr["item_count"])):
            a = int(want_off[frame_of[g]]) + int(t2["data_offset"][g])
            parts.append(wire[a:a + int(t2["data_len"][g])])
        got = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        assert np.array_equal(got, payload[int(pk["data_offset"]):int(pk["data_offset"]) + int(pk["data_len"])]), k


def test_more_items_than_the_item_grid(engine):
    """66 senders of one MAX_PACKET_SIZE packet each among small ones: 4 325 376 items and more, beyond the item
    kernel's grid of kItemBlocksMax workgroups (its stride loop).  Every output against the host call's, field for
    field, and the big packets' items in closed form (emit_expect.check_max_packets); the slack behind items_used
    stays as it was."""
    import receive_expect as E
    from uflow_amd import frame as fr
    b, big = EE.many_max_packets()
    packets, first, senders = b.arrays()
    ref = fr.emit_packets_host(packets, first, senders, nthreads=8)
    used, slack = ref[5], 1000
    assert used > E.EMIT_SLOTS_MAX and len(big) * 65536 > E.EMIT_SLOTS_MAX   # the threshold, from the inputs
    items = torch.full((used + slack, ITEM_DTYPE.itemsize), EE.FILL, dtype=torch.uint8, device=DEV)
    got = _host(engine.emit_packets(*_dev(packets, first, senders), items_cap=used + slack, items=items))
    torch.cuda.synchronize()
    assert got[5] == used and np.array_equal(got[1].astype(np.uint64), ref[1])
    g_items = got[0].view(ITEM_DTYPE).reshape(-1)
    # (the reserved slots in front of a sender's items stay as they were on both sides: FILL here, zero there)
    reserved = np.zeros(used, dtype=bool)
    for s in np.flatnonzero(senders["reserve_items"]):
        reserved[int(ref[1][s]): int(ref[1][s]) + int(senders["reserve_items"][s])] = True
    same = (g_items[:used].view(np.uint8).reshape(used, -1) == ref[0].view(np.uint8).reshape(used, -1)).all(axis=1)
    assert same[~reserved].all(), np.flatnonzero(~same & ~reserved)[:8]
    assert (g_items[:used][reserved].view(np.uint8) == EE.FILL).all() and (g_items[used:].view(np.uint8) == EE.FILL).all()
    for k, dt in ((2, EE.PACKET_RESULT_DTYPE), (3, EE.SENDER_RESULT_DTYPE), (4, SENDER_DTYPE)):
        assert got[k].tobytes() == ref[k].tobytes(), dt.names
    EE.check_max_packets(g_items, got[1], packets, first, senders, big)
