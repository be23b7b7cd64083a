"""GPU: the batched packet receive (ufc_receive_packets_varlen, FrameCrcEngine.receive_packets) against
tests/receive_expect.py, PacketReceiver / AssemblyWindow / FragmentBuffer restated class for class: the same
scenarios and generators as tests/test_receive_cpu.py at the smallest shapes that can go wrong, every output
pre-filled; and the whole path on the device, emit -> pack -> build -> seal -> gate -> parse -> receive."""
import copy

import numpy as np
import pytest
import torch

from uflow_amd import frame as fr
from uflow_amd.batch import records, rows
from uflow_amd.frame import FLUSH_DTYPE, PACKET_DTYPE, SENDER_DTYPE

import receive_expect as E
import test_receive_cpu as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRAG = E.FRAG
U8 = np.uint8


def _dev_args(infos, items, payload, frame_first, receivers, slots, slot_first, carry_in, src_base, frame_accept):
    return dict(infos=rows(infos, DEV), items=rows(items, DEV), payload=rows(payload, DEV), frame_first=rows(frame_first, DEV),
                receivers=rows(receivers, DEV), slots=rows(slots, DEV), slot_first=rows(slot_first, DEV), carry_in=rows(carry_in, DEV),
                src_base=None if src_base is None else rows(src_base, DEV),
                frame_accept=None if frame_accept is None else rows(frame_accept, DEV))


def _host_out(d, d_slots):
    o = {}
    for k, v in d.items():
        o[k] = None if v is None else v.cpu().numpy()
    o["packets"] = o["packets"].view(fr.RX_PACKET_DTYPE).reshape(-1)
    o["results"] = o["results"].view(fr.RECEIVER_RESULT_DTYPE).reshape(-1)
    o["receivers_out"] = o["receivers_out"].view(fr.RECEIVER_DTYPE).reshape(-1)
    for k in ("packet_first", "carry_first"):
        o[k] = o[k].astype(np.uint64)
    for k in ("packets_used", "out_used", "carry_used"):
        o[k] = int(o[k][0])
    o["slots"] = records(d_slots, fr.RX_SLOT_DTYPE)
    return o


def gpu_call(engine, stream=None):
    """receive_packets_host's calling convention on the device form (what receive_expect.run_native calls)."""
    def call(infos, items, payload, frame_first, receivers, slots, slot_first, carry_in, src_base=None, frame_accept=None,
             carry_out=None, out_bytes=None, packets=None, **_):
        a = _dev_args(infos, items, payload, frame_first, receivers, slots, slot_first, carry_in, src_base, frame_accept)
        opt = lambda x: None if x is None else rows(x, DEV)  # noqa: E731  (None: the wrapper's default caps)
        d = engine.receive_packets(**a, carry_out=opt(carry_out), out_bytes=opt(out_bytes), packets=opt(packets),
                                   stream=stream)
        torch.cuda.synchronize()
        o = _host_out(d, a["slots"])
        slots[:] = o["slots"]
        return o
    return call


@pytest.mark.parametrize("case", T.GOLDEN, ids=[c["name"] for c in T.GOLDEN])
def test_golden_cases(engine, case):
    T.run_golden(case, gpu_call(engine))


@pytest.mark.parametrize("scenario", [
    T.test_reordered_duplicated_and_mismatching_fragments, T.test_out_of_window_and_behind_the_channel_base,
    T.test_stalled_channel_released_two_steps_later, T.test_ready_flag_clear_on_entry,
    T.test_allocation_limit_duds_and_empty_packet, T.test_resynchronize_and_deliver_zero,
    T.test_lying_sender_leaves_a_stale_entry_behind, T.test_bad_state_and_bad_src,
    T.test_first_fragment_alone_with_default_caps, *T.TILE_SCENARIOS, *T.COPY_SCENARIOS], ids=lambda f: f.__name__[5:])
def test_scenarios(engine, monkeypatch, scenario):
    """The host test's scenarios with the device call in the host call's place."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    scenario()


def test_caps_below_need(engine, monkeypatch):
    monkeypatch.setattr(T, "host", gpu_call(engine))
    monkeypatch.setattr(T, "lib_call_null_payload", lambda *a: (_ for _ in ()).throw(
        T.NativeError(T.UFC_ERR_INVALID_ARG)))   # (the host ABI's NULL rule is the host test's)
    T.test_caps_below_need_and_argument_rules()


def test_argument_checks(engine):
    n = fr.new_receivers(1, 4)
    a = _dev_args(np.zeros(0, fr.FRAME_INFO_DTYPE), np.zeros(0, fr.ITEM_DTYPE), np.zeros(0, U8), np.zeros(2, np.uint64), n,
                  np.zeros(4, fr.RX_SLOT_DTYPE), np.array([0, 4], np.uint64), np.zeros(0, U8), None, None)
    o = engine.receive_packets(**a)
    torch.cuda.synchronize()
    res = records(o["results"], fr.RECEIVER_RESULT_DTYPE)
    assert int(o["packets_used"][0]) == 0 and int(res["stop"][0]) == 0
    with pytest.raises(ValueError):
        engine.receive_packets(**{**a, "slot_first": a["slot_first"][:1]})
    with pytest.raises(T.NativeError):   # an unaligned carry arena
        engine.receive_packets(**{**a, "carry_in": torch.zeros(9, dtype=torch.uint8, device=DEV)[1:]})
    # the C ABI's NULL rules: a NULL payload with payload_len != 0, a NULL d_results
    import ctypes
    V = ctypes.c_void_p
    st = V(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    ok = [a["infos"].data_ptr() or None, 0, None, None, 0, None, V(buf.data_ptr()), 8, V(a["frame_first"].data_ptr()),
          V(a["receivers"].data_ptr()), 1, V(a["slots"].data_ptr()), V(a["slot_first"].data_ptr()), 4, None, 0, None, 0,
          V(buf.data_ptr() + 64), V(buf.data_ptr() + 128), None, 0, V(buf.data_ptr() + 256), V(buf.data_ptr() + 136), None, 0,
          V(buf.data_ptr() + 144), None, V(buf.data_ptr() + 512), V(buf.data_ptr() + 1024), st]
    lib = fr.lib()
    assert lib.ufc_receive_packets_varlen(engine._ctx, *ok) == 0
    for k in (6, 28, 29, 8):   # payload, results, receivers_out, frame_first
        bad = list(ok)
        bad[k] = None
        assert lib.ufc_receive_packets_varlen(engine._ctx, *bad) == T.UFC_ERR_INVALID_ARG, k
    torch.cuda.synchronize()
    a0 = {**a, "receivers": a["receivers"][:0], "frame_first": a["frame_first"][:1], "slot_first": a["slot_first"][:1]}
    engine.receive_packets(**a0)   # no receivers: UFC_OK


def test_slot_count_limit_of_the_device_entry(engine):
    """The device entry alone scans 2 n_slots + 1 chunk counts with a 32-bit count, so it takes n_slots below
    (2^31 - 1) // 2 where the host entry takes them below 2^31 - 1: that many slots are refused before any launch,
    with every pointer set; the same arguments with the receiver's own 4 slots are accepted."""
    import ctypes
    V = ctypes.c_void_p
    r = fr.new_receivers(1, 4)
    d = {"receivers": rows(r, DEV), "slots": rows(np.zeros(4, fr.RX_SLOT_DTYPE), DEV),
         "frame_first": rows(np.zeros(2, np.uint64), DEV), "slot_first": rows(np.array([0, 4], np.uint64), DEV)}
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    at = lambda off: V(buf.data_ptr() + off)   # noqa: E731
    st = V(torch.cuda.current_stream().cuda_stream)

    def call(n_slots):
        return fr.lib().ufc_receive_packets_varlen(
            engine._ctx, None, 0, None, None, 0, None, None, 0, V(d["frame_first"].data_ptr()),
            V(d["receivers"].data_ptr()), 1, V(d["slots"].data_ptr()), V(d["slot_first"].data_ptr()), n_slots, None, 0,
            None, 0, at(64), at(128), None, 0, at(256), at(136), None, 0, at(144), None, at(512), at(1024), st)

    assert call(((1 << 31) - 1) // 2) == T.UFC_ERR_INVALID_ARG
    assert call(4) == 0
    torch.cuda.synchronize()
    res = buf[512:592].cpu().numpy().view(fr.RECEIVER_RESULT_DTYPE)
    assert int(res["stop"][0]) == 0


def big_fragment_steps(rng):
    """Two steps for three receivers: window 4096 with the ring wrapped and packets of 2, 64, 65 and 130 fragments
    (bitfield word edges) whose fragments arrive reversed, some withheld until the second step, beside more small
    packets than a tile holds; a receiver with no items; a window of one slot."""
    rxs = [E.PacketReceiver(4096, 0xFFFF0 - 4096 * 3 + 17, 1 << 30), E.PacketReceiver(64, 9, 1 << 30),
           E.PacketReceiver(1, 0xFFFFF, 1 << 30)]
    tx = E.GenSender(rxs[0].base_id)
    first, second = [], []
    for nfrag in (2, 64, 65, 130):
        dgs = tx.packet(1, True, rng.integers(0, 256, nfrag * FRAG - 7, dtype=U8).tobytes())[::-1]
        keep = [k for k in range(nfrag) if k in (0, nfrag - 1) or (nfrag - 1 - k) in (63, 64)]
        first += [d for k, d in enumerate(dgs) if k not in keep]
        second += [dgs[k] for k in keep] + [dgs[1]]   # and a duplicate of one that arrived before
    for _ in range(70):
        first += tx.packet(int(rng.integers(0, 3)), False, rng.integers(0, 256, int(rng.integers(0, 90)), dtype=U8).tobytes())
    one = E.GenSender(0xFFFFF)
    a, b = one.packet(0, True, b"last id"), one.packet(0, True, b"first id")
    return rxs, [E.simple_batch([first, [], a + b], rng), E.simple_batch([second, [], b], rng)]


def test_big_fragments_tiles_and_windows(engine):
    rng = np.random.default_rng(11)
    rxs, batches = big_fragment_steps(rng)
    h = E.Harness(rxs, gpu_call(engine))
    o, exp = h.step(batches[0], what="first")
    assert o["carry_used"] > 250 * FRAG and len(exp["delivered"][0]) < 70   # the held ones wait behind the big ones
    o, exp = h.step(batches[1], what="second")
    assert [len(p[2]) for p in exp["delivered"][0][:4]] == [n * FRAG - 7 for n in (2, 64, 65, 130)]
    assert o["carry_used"] == 0 and rxs[2].base_id == 1


def test_host_and_device_read_each_others_carry(engine):
    rng = np.random.default_rng(12)
    rxs, batches = big_fragment_steps(rng)
    h = E.Harness(rxs, fr.receive_packets_host)
    h.step(batches[0], what="host first")
    h.call = gpu_call(engine)
    h.step(batches[1], what="device second")
    rxs, batches = big_fragment_steps(rng)
    h = E.Harness(rxs, gpu_call(engine))
    h.step(batches[0], what="device first")
    h.call = fr.receive_packets_host
    h.step(batches[1], what="host second")


@pytest.mark.parametrize("n_receivers", [1, 3, 300])
def test_random_runs(engine, n_receivers):
    total, tags = T.random_run(gpu_call(engine), 20 + n_receivers, n_receivers, windows=(1, 8, 64))
    # (resynchronize, steps without delivery and lying senders on carried state.  The branch condition hangs on
    # this one seed: should it ever miss a tag, look at the generator, receive_expect.gen_step, not at the kernels:
    # the tags come from the restatement, and the host test asserts the same over four seeds.)
    if n_receivers == 300:
        assert np.all(total > 0), total
        for tag in T.BRANCHES:
            assert tag in tags, tag


@pytest.mark.parametrize("n_receivers", [12, 96])
def test_random_tile_runs(engine, n_receivers):
    """The random runs over several tiles of ids (tests/test_receive_cpu.py, TILE_GEN): the 12 receivers and four
    steps of the host test, and 96 receivers over two steps.  The condition is the restatement's, as above."""
    rxs = []
    _, tags = T.random_run(gpu_call(engine), T.TILE_SEEDS[0] if n_receivers == 12 else 60, n_receivers,
                           steps=4 if n_receivers == 12 else 2, windows=T.TILE_WINDOWS, gen=T.TILE_GEN, rxs_out=rxs)
    T.assert_tile_condition(tags, rxs)


@pytest.mark.parametrize("family", ["one_tile", "tiles"])
def test_four_steps_one_stream_no_synchronise(engine, family):
    """Four carried steps queued back to back on one stream, state and carry staying on the device (the later
    calls need less scratch than the first: it is reused); everything is checked afterwards.  `tiles`: windows of
    256 ids and the generator options of the runs over several tiles."""
    rng = np.random.default_rng(15 if family == "tiles" else 13)   # (15: the tile condition below holds)
    if family == "tiles":
        rxs = [E.PacketReceiver(256, 0xFFFFF - 5 * r, 4000 if r % 4 == 1 else 1 << 30) for r in range(12)]
        gens = [T.TILE_GEN] * 4
    else:
        rxs = [E.PacketReceiver((1, 8, 64)[r % 3], 0xFFFFF - 5 * r, 4000 if r % 4 == 1 else 1 << 30) for r in range(40)]
        gens = [dict(n_packets=12 if k == 0 else 4) for k in range(4)]
    txs = [E.GenSender(rx.base_id) for rx in rxs]
    held = [[] for _ in rxs]
    receivers, slots, slot_first, carry = E.new_state(rxs)
    plan = []
    for k in range(4):
        b = E.gen_step(rng, rxs, txs, held, **gens[k])
        exp = E.expected_step(rxs, b)
        a = _dev_args(b.infos, b.items, b.payload, b.frame_first, receivers, slots, slot_first, carry, b.src_base,
                      b.frame_accept)
        # the step's inputs in the header: deliver (byte 13) and resync_id (bytes 16..19)
        a["deliver"] = rows(np.array(b.deliver, dtype=U8), DEV)
        a["resync"] = rows(np.array(b.resync, dtype="<u4").view(U8).reshape(-1, 4), DEV)
        plan.append((b, exp, copy.deepcopy(rxs), a))
    d_recv, d_slots, d_sf, d_carry = rows(receivers, DEV), rows(slots, DEV), rows(slot_first, DEV), rows(carry, DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    outs = []
    with torch.cuda.stream(s):
        for b, exp, _, a in plan:
            def fill(*shape):
                return torch.full(shape, E.FILL, dtype=torch.uint8, device=DEV)
            d_recv = d_recv.clone()   # (the step before is checked on its own output)
            d_recv[:, 13] = a["deliver"]
            d_recv[:, 16:20] = a["resync"]
            before = (d_recv, d_slots.clone())
            d = engine.receive_packets(a["infos"], a["items"], a["payload"], a["frame_first"], d_recv, d_slots, d_sf,
                                       d_carry, src_base=a["src_base"], frame_accept=a["frame_accept"],
                                       carry_out=fill(E.carry_bound(b, d_carry.numel(), slots.size)),
                                       out_bytes=fill(d_carry.numel() + b.payload.size),
                                       packets=fill(b.items.size + slots.size, fr.RX_PACKET_DTYPE.itemsize), stream=s)
            outs.append((d, d_slots.clone(), before))
            d_recv, d_carry = d["receivers_out"], d["carry_out"]   # the swap: the arena as it is, not cut to carry_used
    s.synchronize()
    for (b, exp, rxs_k, _), (d, slots_after, (recv_before, slots_before)) in zip(plan, outs):
        E.check(_host_out(d, slots_after), exp, rxs_k, b, records(recv_before, fr.RECEIVER_DTYPE),
                records(slots_before, fr.RX_SLOT_DTYPE), slot_first, what="queued step")
    engine.release_stream(s)
    if family == "tiles":
        T.assert_tile_condition(set().union(*[rx.tags for rx in rxs]), rxs)


def test_scratch_reuse_after_a_larger_call(engine):
    call = gpu_call(engine)
    T.random_run(call, 31, 120, steps=2, windows=(64,))
    T.random_run(call, 32, 2, steps=2, windows=(8,))


def test_emit_to_receive_on_the_device(engine):
    """emit_packets -> pack_flushes -> build_varlen(seal) -> crc_varlen -> parse_varlen -> receive_packets: the
    delivered packets are the queued ones, per receiver in order."""
    rng = np.random.default_rng(14)
    n, per = 24, 12
    packets = np.zeros(n * per, dtype=PACKET_DTYPE)
    sizes = rng.choice([0, 3, 60, 700, FRAG, FRAG + 1, 2 * FRAG + 9], size=packets.size)
    packets["data_len"] = sizes
    packets["data_offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packets["channel_id"] = rng.integers(0, 3, packets.size)
    packets["mode"] = fr.SEND_RELIABLE
    payload = rng.integers(0, 256, int(sizes.sum()), dtype=U8)
    senders = np.zeros(n, dtype=SENDER_DTYPE)
    senders["base_id"] = senders["next_id"] = rng.integers(0, 1 << 20, n)
    senders["window_size"], senders["max_alloc"], senders["take"] = 64, 1 << 30, per
    senders["window_parent_id"] = fr.NO_PARENT
    senders["channel_parent_id"] = fr.NO_PARENT
    items, ff, _, sres, _, used = engine.emit_packets(rows(packets, DEV), rows(np.arange(n + 1) * per, DEV), rows(senders, DEV),
                                                      items_cap=int(np.maximum(1, (sizes + FRAG - 1) // FRAG).sum()))
    flushes = np.zeros(n, dtype=FLUSH_DTYPE)
    flushes["kind"], flushes["flush_alloc"], flushes["window_room"] = 10, 1 << 40, 1 << 20
    infos, res, frames_used = engine.pack_flushes(items, ff, rows(flushes, DEV))
    wire, off, status = engine.build_varlen(infos, items, rows(payload, DEV), seal=True)
    torch.cuda.synchronize()
    n_frames = int(frames_used.cpu()[0])
    d_off = off[:n_frames + 1].contiguous()
    _, valid = engine.crc_varlen(wire, d_off)
    infos2, items2, used2 = engine.parse_varlen(wire, d_off, valid)
    fres = records(res, fr.FLUSH_RESULT_DTYPE)
    frame_first = np.concatenate([fres["frame_first"], [n_frames]]).astype(np.int64)
    receivers = fr.new_receivers(n, 64, senders["base_id"])
    slots = torch.zeros((n * 64, fr.RX_SLOT_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    o = engine.receive_packets(infos2[:n_frames].contiguous(), items2, wire, rows(frame_first, DEV), rows(receivers, DEV), slots,
                               rows(np.arange(n + 1) * 64, DEV), torch.zeros(0, dtype=torch.uint8, device=DEV),
                               src_base=d_off[:n_frames].contiguous(), frame_accept=valid)
    torch.cuda.synchronize()
    h = _host_out(o, slots)
    assert h["packets_used"] == packets.size and h["carry_used"] == 0 and h["out_used"] == payload.size
    assert (h["results"]["stop"] == 0).all() and (h["results"]["packet_count"] == per).all()
    for s in range(n):
        recs = h["packets"][int(h["packet_first"][s]): int(h["packet_first"][s + 1])]
        for c in range(3):
            got = [h["out_bytes"][int(p["out_offset"]): int(p["out_offset"]) + int(p["len"])].tobytes()
                   for p in recs if p["channel_id"] == c]
            want = [payload[int(p["data_offset"]): int(p["data_offset"]) + int(p["data_len"])].tobytes()
                    for p in packets[s * per: (s + 1) * per] if p["channel_id"] == c]
            assert got == want, (s, c)
    assert np.array_equal(h["receivers_out"]["base_id"], (senders["base_id"] + per) & 0xFFFFF)


# ---- launch shapes beyond one grid: many receivers, the copy kernels' second pass ----
def big_step(engine, batch, state, sample, rxs, what):
    """One step of a call too large for the restatement, on the device: every output against the host call's
    (which tests/test_receive_cpu.py pins to the restatement), the firsts and used counts against sums over the
    call's own per-receiver outputs, and the receivers `sample` against the restatement (`rxs`, advanced).
    Returns the next state."""
    receivers, slots, slot_first, carry = state
    dev = E.run_native(gpu_call(engine), batch, receivers, slots, slot_first, carry)
    ref = E.run_native(fr.receive_packets_host, batch, receivers, slots, slot_first, carry, nthreads=8)
    E.check_same(dev, ref, what)
    E.check_sums(dev, slot_first, what)
    sub = E.sub_batch(batch, sample)
    E.check_receivers(dev, E.expected_step(rxs, sub), rxs, sub, sample, batch.apply(receivers.copy()), slots, slot_first,
                      what)
    return dev, (dev["receivers_out"], dev["slots"], slot_first, dev["carry_out"][:dev["carry_used"]].copy())


def pair_receivers(rng, n, big=()):
    """n receivers with a window of two ids, bases over the whole id space and at the wrap; two packets each of
    1 to 40 bytes, every sixteenth with a second packet of two fragments; `big`: sizes of first packets that 40
    receivers spread over the index range get instead."""
    bases = rng.integers(0, 1 << 20, n)
    bases[::97] = 0xFFFFF
    size0, size1 = rng.integers(1, 41, n), rng.integers(1, 41, n)
    size1[5::16] += FRAG
    where = (np.arange(40) * (n - 1) // 39) if len(big) else np.zeros(0, np.int64)
    size0[where] = np.resize(big, where.size)
    fixed = [0, 7, 8, 63, 64, E.RX_FEW - 2, E.RX_FEW - 1, E.RX_FEW, n - 1, 5, 21, 97] + where.tolist()
    sample = E.sample_of(rng, n, fixed, 64 + where.size)
    rxs = [E.PacketReceiver(2, int(bases[r]), 1 << 40) for r in sample]
    state = (fr.new_receivers(n, 2, bases), np.zeros(2 * n, dtype=fr.RX_SLOT_DTYPE), np.arange(n + 1, dtype=np.uint64) * 2,
             np.zeros(0, U8))
    return bases, size0, size1, sample, rxs, state


def held_then_delivered(engine, n, big=()):
    rng = np.random.default_rng(15)
    bases, size0, size1, sample, rxs, state = pair_receivers(rng, n, big)
    held, _ = E.pair_batch(rng, bases, size0, size1)
    o, state = big_step(engine, held, state, sample, rxs, "held")
    assert o["packets_used"] == 0 and int((o["slots"]["rx_flags"] & fr.RX_SLOT_DATA != 0).sum()) == 2 * n
    assert fr.RX_DROPPED_DUPLICATE in o["item_status"] and fr.RX_DROPPED_CLOSED in o["item_status"]
    extra = {r: [(10, 1, [(int(bases[r]), 0, 0, 0, 0, 0, b"again"), (E.add(int(bases[r]), 2), 0, 0, 0, 0, 0, b"beyond")])]
             for r in sample[::2]}
    chunks = int(((np.concatenate([size0, size1]) + E.RX_CHUNK - 1) // E.RX_CHUNK).sum())
    o, state = big_step(engine, E.sparse_batch(n, extra), state, sample, rxs, "delivered")
    assert o["packets_used"] == 2 * n and o["carry_used"] == 0 and o["out_used"] == int(size0.sum() + size1.sum())
    return held, chunks


def test_many_receivers_held_then_delivered(engine):
    """35 000 receivers (the 64-lane form of begin, items and finish), every slot held for a step and delivered in
    the next: 280 000 datagrams, each arriving four times (the item copy's second grid pass), then 140 000 slot
    segments of which 70 000 hold a chunk (the slot copy's grid clipped, and more chunks than its waves)."""
    n = 35000
    held, chunks = held_then_delivered(engine, n)
    assert n + 1 >= E.RX_FEW and held.items.size > E.COPY_ITEMS_MAX   # the thresholds, from the inputs
    assert (2 * 2 * n + 3) // 4 > E.LAUNCH_CONSTANTS["kCopyBlocksMax"] and chunks > E.COPY_WAVES_MAX


def test_multi_chunk_segments_among_many(engine):
    """33 000 receivers as above, 40 of them over the index range holding a packet of 2047 to 4339 bytes: the
    binary search in the chunk prefix over mixed counts, some of those chunks in the second grid pass."""
    n = 33000
    big = (E.RX_CHUNK - 1, E.RX_CHUNK, E.RX_CHUNK + 1, 2 * E.RX_CHUNK + 3, 3 * FRAG - 5)
    held, chunks = held_then_delivered(engine, n, big)
    assert n + 1 >= E.RX_FEW and chunks > E.COPY_WAVES_MAX + 2 * len(big)


def test_more_receivers_than_verdict_workgroups(engine):
    """2^20 + 70 receivers with a window of one id, frames for about 200 of them (valid, invalid, out-of-window
    datagrams, frames that do not count), the others' ranges empty: the verdict kernel's stride over receivers."""
    rng = np.random.default_rng(16)
    top = E.VERDICT_GROUPS_MAX
    n = top + 70
    bases = (np.arange(n, dtype=np.int64) * 7 + 0xFFFF0) & E.MASK
    active = sorted(set(range(top - 1, n)) | {0, 7, 8, 63, 64, E.RX_FEW - 2, E.RX_FEW - 1, E.RX_FEW}
                    | set(rng.integers(0, top, 122).tolist()))
    frames = {}
    for k, r in enumerate(active):
        b = int(bases[r])
        good = (b, k % 3, 0, 0, 0, 0, bytes(rng.integers(0, 256, 1 + k % 40, dtype=U8)))
        bad = [(b, 0, 0, 0, 2, 1, b"fragment 2 of 2"), (E.add(b, 1), 0, 0, 0, 0, 0, b"beyond"), (b, 64, 0, 0, 0, 0, b"channel")]
        frames[r] = [(10, 1, [bad[k % 3], good, good]), (12, 1, [good]), (10, k % 5 != 0, [good, bad[(k + 1) % 3]])]
    batch = E.sparse_batch(n, frames, rng)
    sample = E.sample_of(rng, n, active, len(active) + 8)
    rxs = [E.PacketReceiver(1, int(bases[r]), 1 << 40) for r in sample]
    state = (fr.new_receivers(n, 1, bases), np.zeros(n, dtype=fr.RX_SLOT_DTYPE), np.arange(n + 1, dtype=np.uint64),
             np.zeros(0, U8))
    assert n > E.VERDICT_GROUPS_MAX and {top - 1, top, top + 1, n - 1} <= set(sample)
    o, _ = big_step(engine, batch, state, sample, rxs, "verdict stride")
    assert o["packets_used"] == len(active) and (o["results"]["packet_count"][active] == 1).all()
