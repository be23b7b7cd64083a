"""ufc_receive_packets_host against the plain Python restatement of PacketReceiver / AssemblyWindow /
FragmentBuffer (tests/receive_expect.py): every record, status, state field, slot field and delivered byte, all
exact.  The golden cases are the reference's own unit tests (tests/golden/packet_receiver_cases.json)."""
import json
import os

import numpy as np
import pytest

import receive_expect as E
from uflow_amd import frame as fr
from uflow_amd._native import NativeError, UFC_ERR_INVALID_ARG

HERE = os.path.dirname(os.path.abspath(__file__))
FRAG = E.FRAG
with open(os.path.join(HERE, "golden", "packet_receiver_cases.json")) as f:
    GOLDEN = json.load(f)["cases"]


def host(*a, **kw):
    return fr.receive_packets_host(*a, **kw)


def iota(start, n):
    return bytes((start + i) % 256 for i in range(n))


def golden_datagrams(specs):
    """(datagram tuples, what try_add is expected to return per datagram or None)"""
    dgs, expect = [], []
    for d in specs:
        if isinstance(d, list):
            seq, ch, wl, cl = d
            dgs.append((seq, ch, wl, cl, 0, 0, seq.to_bytes(4, "big")))
            expect.append(None)
        elif "range" in d:
            for seq in range(*d["range"]):
                lead = seq if d["leads"] == "id" else 0
                dgs.append((seq, d["channel"], lead, lead, 0, 0, seq.to_bytes(4, "big")))
                expect.append(None)
        else:
            dgs.append((d["seq"], d.get("ch", 0), d.get("wl", 0), d.get("cl", 0), d["f"], d["last"], iota(*d["iota"])))
            expect.append(d["expect"])
    return dgs, expect


def golden_popped(point):
    ids = []
    for p in point["popped"]:
        ids += list(range(*p["range"])) if isinstance(p, dict) else [p]
    return ids


def run_golden(case, call):
    rx = E.PacketReceiver(case["window_size"], case["base_id"], case["max_alloc"])
    h = E.Harness([rx], call)
    for k, point in enumerate(case["points"]):
        dgs, expect = golden_datagrams(point["datagrams"])
        o, exp = h.step(E.simple_batch([dgs], per_frame=100), what=f"{case['name']} point {k}")
        for g, want in enumerate(expect):
            if want is not None:
                got = {fr.RX_COMPLETED: "packet", fr.RX_DUD: "dud"}.get(int(o["item_status"][g]), "none")
                assert got == want, (case["name"], k, g, got, want)
        ids = golden_popped(point)
        recs = o["packets"][:o["packets_used"]]
        assert recs["sequence_id"].tolist() == ids, (case["name"], k)
        data = point.get("popped_iota")
        for j, rec in enumerate(recs):
            got = o["out_bytes"][int(rec["out_offset"]): int(rec["out_offset"]) + int(rec["len"])].tobytes()
            if data is None:
                assert got == int(rec["sequence_id"]).to_bytes(4, "big") and rec["flags"] == 0
            elif data[j] is None:
                assert rec["flags"] == fr.RX_PACKET_DUD and rec["len"] == 0
            else:
                assert got == iota(*data[j]) and rec["flags"] == 0
        out = o["receivers_out"][0]
        for key in ("base_id", "end_id"):
            if key in point:
                assert int(out[key]) == point[key] == getattr(rx, key), (case["name"], k, key)
        for c, want in point.get("channels", {}).items():
            assert int(out["channel_base_id"][int(c)]) == (E.NONE if want is None else want)
            assert rx.channels[int(c)].base_id == want


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_cases(case):
    run_golden(case, host)


def frags(seq, ch, wl, cl, data):
    last = max((len(data) + FRAG - 1) // FRAG, 1) - 1
    return [(seq, ch, wl, cl, f, last, data[f * FRAG: (f + 1) * FRAG]) for f in range(last + 1)]


def rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def test_reordered_duplicated_and_mismatching_fragments():
    rng = np.random.default_rng(2)
    rx = E.PacketReceiver(8, 0xFFFFD, 1 << 20)  # the ids wrap, and the ring does not start at slot 0
    assert rx.base_id & 7
    h = E.Harness([rx], host)
    a = frags(0xFFFFE, 1, 0, 0, rnd(rng, 3 * FRAG + 9))
    b = frags(0x00001, 2, 0, 0, rnd(rng, 2 * FRAG))
    other = (a[1][0], 1, 0, 0, 1, 3, bytes(FRAG))            # fragment 1 again, with other bytes
    bad_last = (a[2][0], 1, 0, 0, 2, 4, a[2][6])             # another fragment count
    bad_lead = (a[2][0], 1, 3, 0, 2, 3, a[2][6])             # another window lead
    o, exp = h.step(E.simple_batch([[a[3], a[1], other, bad_last, b[1], bad_lead]]), what="first half")
    assert exp["status"].tolist() == [fr.RX_STORED, fr.RX_STORED, fr.RX_DROPPED_DUPLICATE, fr.RX_DROPPED_MISMATCH,
                                      fr.RX_STORED, fr.RX_DROPPED_MISMATCH]
    assert o["packets_used"] == 0 and o["carry_used"] == 4 * FRAG + 8 + 2 * FRAG + 8
    # the duplicate of a fragment received in an earlier step (its bit is in the carry), then the rest
    o, exp = h.step(E.simple_batch([[other, a[0], b[0], a[2], a[0]]]), what="second half")
    assert exp["status"].tolist() == [fr.RX_DROPPED_DUPLICATE, fr.RX_STORED, fr.RX_COMPLETED, fr.RX_COMPLETED,
                                      fr.RX_DROPPED_CLOSED]
    assert o["packets"][:2]["sequence_id"].tolist() == [0xFFFFE, 1] and o["carry_used"] == 0
    assert int(o["receivers_out"][0]["base_id"]) == 2


def test_out_of_window_and_behind_the_channel_base():
    rx = E.PacketReceiver(4, 10, 1 << 20)
    h = E.Harness([rx], host)
    # id 12 on channel 0 is delivered past the missing reliable id 10 of channel 1: channel 0's base moves to 13
    _, exp = h.step(E.simple_batch([[(12, 0, 2, 0, 0, 0, b"twelve"), (14, 0, 0, 0, 0, 0, b"far"), (9, 0, 0, 0, 0, 0, b"old")]]))
    assert exp["status"].tolist() == [fr.RX_COMPLETED, fr.RX_DROPPED_WINDOW, fr.RX_DROPPED_WINDOW]
    assert rx.channels[0].base_id == 13 and rx.base_id == 10
    _, exp = h.step(E.simple_batch([[(11, 0, 1, 0, 0, 0, b"late"), (11, 2, 1, 0, 0, 0, b"other channel")]]))
    assert exp["status"].tolist() == [fr.RX_DROPPED_CHANNEL, fr.RX_COMPLETED]


def test_stalled_channel_released_two_steps_later():
    rx = E.PacketReceiver(16, 0, 1 << 20)
    h = E.Harness([rx], host)
    o, _ = h.step(E.simple_batch([[(1, 3, 1, 1, 0, 0, b"one"), (2, 3, 3, 3, 0, 0, b"two")]]))
    assert o["packets_used"] == 0 and "channel_stalled" in rx.tags
    o, _ = h.step(E.simple_batch([[(3, 5, 3, 0, 0, 0, b"elsewhere")]]))
    assert o["packets"][:o["packets_used"]]["sequence_id"].tolist() == [3]
    o, _ = h.step(E.simple_batch([[(0, 3, 0, 0, 0, 0, b"zero")]]))
    assert o["packets"][:o["packets_used"]]["sequence_id"].tolist() == [0, 1, 2]
    assert o["out_bytes"][:o["out_used"]].tobytes() == b"zeroonetwo" and rx.base_id == 4


def test_ready_flag_clear_on_entry():
    rx = E.PacketReceiver(8, 0, 1 << 20)
    h = E.Harness([rx], host)
    h.step(E.simple_batch([[(0, 1, 0, 0, 0, 0, b"a"), (1, 2, 0, 0, 0, 0, b"b")]], deliver=[0]))
    assert rx.channel_ready_flags == 0b110
    rx.channel_ready_flags = 0b100          # channel 1 not ready, whatever waits behind it
    h.receivers["channel_ready_flags"] = 0b100
    o, _ = h.step(E.simple_batch([[]]))
    assert o["packets"][:o["packets_used"]]["sequence_id"].tolist() == [1] and "channel_not_ready" in rx.tags
    assert rx.base_id == 2 and "window_passed_undelivered" in rx.tags


def test_allocation_limit_duds_and_empty_packet():
    rng = np.random.default_rng(3)
    rx = E.PacketReceiver(8, 0, 3000)  # rounds up to 4344
    h = E.Harness([rx], host)
    big = frags(0, 0, 0, 0, rnd(rng, 3 * FRAG + 1))    # 4 fragments: refused
    mid = frags(1, 0, 0, 0, rnd(rng, 2 * FRAG))        # 2896: fits
    small = frags(2, 0, 0, 0, rnd(rng, 1448))          # 1448: fits exactly
    one = frags(3, 0, 0, 0, b"x")                      # refused
    empty = frags(4, 0, 0, 0, b"")                     # an empty packet needs nothing
    o, exp = h.step(E.simple_batch([[big[0], mid[0], big[1], small[0], one[0], empty[0], mid[1]]]))
    assert exp["status"].tolist() == [fr.RX_DUD, fr.RX_STORED, fr.RX_DROPPED_CLOSED, fr.RX_COMPLETED, fr.RX_DUD,
                                      fr.RX_COMPLETED, fr.RX_COMPLETED]
    recs = o["packets"][:o["packets_used"]]
    assert recs["flags"].tolist() == [1, 0, 0, 1, 0] and recs["len"].tolist() == [0, 2 * FRAG, FRAG, 0, 0]
    assert int(o["results"][0]["packets_dud"]) == 2 and int(o["receivers_out"][0]["alloc"]) == 0
    assert "empty_packet" in rx.tags


def test_resynchronize_and_deliver_zero():
    rx = E.PacketReceiver(8, 0, 1 << 20)
    h = E.Harness([rx], host)
    # a batch split at a sync frame: the datagrams in front of it without delivery ...
    o, _ = h.step(E.simple_batch([[(3, 0, 3, 0, 0, 0, b"three"), (1, 1, 1, 1, 0, 0, b"one")]], deliver=[0]))
    assert o["packets_used"] == 0 and rx.base_id == 0 and o["carry_used"] == 16
    # ... then the resynchronize (it stops at the waiting entry of id 1) and the rest
    o, _ = h.step(E.simple_batch([[(5, 0, 2, 0, 0, 0, b"five")]], resync=[5]))
    assert "resync_stopped_at_entry" in rx.tags and int(o["results"][0]["advanced"]) >= 1
    # (id 1's channel was not ready when it arrived and nothing has made it so: receive() passes it by)
    assert o["packets"][:o["packets_used"]]["sequence_id"].tolist() == [3, 5]
    # nothing waits: the window moves to the sender's next id
    rx = E.PacketReceiver(8, 0xFFFFE, 1 << 20)
    h = E.Harness([rx], host)
    o, _ = h.step(E.simple_batch([[]], resync=[3]))
    assert rx.base_id == 3 and rx.end_id == 3 and "resync_full" in rx.tags and int(o["results"][0]["advanced"]) == 5
    h.step(E.simple_batch([[]], resync=[3 + 9]))           # further than a window: ignored
    assert rx.base_id == 3 and "resync_ignored" in rx.tags


def test_lying_sender_leaves_a_stale_entry_behind():
    rng = np.random.default_rng(4)
    rx = E.PacketReceiver(4, 0, 1 << 20)
    h = E.Harness([rx], host)
    h.step(E.simple_batch([[(1, 0, 1, 1, 0, 0, b"waits for id 0 on channel 0")]]))
    assert rx.channel_ready_flags == 0 and rx.data_flags[1]
    # id 0 arrives on another channel: the window passes id 1, which was never delivered
    o, _ = h.step(E.simple_batch([[(0, 1, 0, 0, 0, 0, b"zero")]]))
    assert rx.base_id == 2 and "window_passed_undelivered" in rx.tags and o["carry_used"] == 32
    # the same slot is opened again (id 5) while the stale packet still lies in it: both in the carry
    five = frags(5, 2, 0, 0, rnd(rng, FRAG + 5))
    o, _ = h.step(E.simple_batch([[five[1], (2, 0, 0, 0, 0, 0, b"two")]]))
    assert o["carry_used"] == 32 + 2 * FRAG + 8
    o, _ = h.step(E.simple_batch([[five[0]]]))
    assert "stale_overwritten" in rx.tags
    # a sender that abandons a half-sent packet: the window passes an ACTIVE slot
    rx2 = E.PacketReceiver(4, 0, 1 << 20)
    h2 = E.Harness([rx2], host)
    half = frags(0, 0, 0, 0, rnd(rng, 2 * FRAG))
    h2.step(E.simple_batch([[half[0]]]))
    o, _ = h2.step(E.simple_batch([[(1, 0, 0, 0, 0, 0, b"next")]]))
    assert "active_cleared" in rx2.tags and o["carry_used"] == 0 and int(o["receivers_out"][0]["alloc"]) == 0


def test_bad_state_and_bad_src():
    rxs = [E.PacketReceiver(4, 0, 1 << 20) for _ in range(6)]
    h = E.Harness(rxs, host)
    b = E.simple_batch([[(0, 0, 0, 0, 0, 0, b"r%d" % r)] for r in range(6)])
    h.receivers["window_size"][1] = 3
    h.receivers["base_id"][2] = 1 << 20
    h.slots["rx_channel_id"][int(h.slot_first[3])] = 64
    h.slots[int(h.slot_first[4]) + 1]["asm_state"] = fr.RX_ASM_ACTIVE   # a fragment buffer outside the carry
    h.slots[int(h.slot_first[4]) + 1]["asm_last_fragment_id"] = 1
    o, _ = h.step(b, bad={1, 2, 3, 4})
    assert o["results"]["stop"].tolist() == [0, 1, 1, 1, 1, 0] and o["packets_used"] == 2
    # frame and slot ranges
    rxs = [E.PacketReceiver(4, 0, 1 << 20) for _ in range(3)]
    h = E.Harness(rxs, host)
    b = E.simple_batch([[(0, 0, 0, 0, 0, 0, b"x")] for _ in range(3)])
    b.frame_first = np.array([0, 2, 1, 3], dtype=np.uint64)        # receiver 1's range is reversed
    h.slot_first = np.array([0, 4, 8, 11], dtype=np.uint64)         # receiver 2 has three slots
    o, _ = h.step(b, bad={1, 2})
    assert o["results"]["stop"].tolist() == [0, 1, 1]
    # payload ranges
    rx = E.PacketReceiver(4, 0, 1 << 20)
    h = E.Harness([rx], host)
    b = E.simple_batch([[(0, 0, 0, 0, 0, 0, b"abcd"), (1, 0, 0, 0, 0, 0, b"efgh"), (2, 0, 0, 0, 0, 0, b"")]], lead=0)
    b.items["data_offset"][1] = 5          # one byte too far
    b.items["data_offset"][2] = 9          # an empty range past the end
    b.src_base = np.array([0], dtype=np.uint64)
    _, exp = h.step(b)
    assert exp["status"].tolist() == [fr.RX_COMPLETED, fr.RX_DROPPED_BAD_SRC, fr.RX_DROPPED_BAD_SRC]
    b.src_base = np.array([1 << 40], dtype=np.uint64)
    _, exp = h.step(b)
    assert exp["status"].tolist() == [fr.RX_DROPPED_BAD_SRC] * 3


def test_caps_below_need_and_argument_rules():
    rng = np.random.default_rng(6)
    for caps in ({"packets": 1}, {"out": 1000}, {"carry": 2000}, {"packets": 0, "out": 0, "carry": 0}):
        rxs = [E.PacketReceiver(8, 0, 1 << 20) for _ in range(2)]
        h = E.Harness(rxs, host)
        lists = []
        for r in range(2):
            held = frags(2, 0, 2, 0, rnd(rng, 700))             # waits behind nothing on its channel: delivered
            part = frags(3, 1, 0, 0, rnd(rng, 2 * FRAG + 3))    # stays in the carry
            stall = frags(1, 1, 1, 1, rnd(rng, 900))            # held: its channel parent is missing
            lists.append(held + part[:2] + stall + frags(4, 0, 0, 0, rnd(rng, FRAG)))
        o, _ = h.step(E.simple_batch(lists), caps=caps, what=str(caps))
        assert o["packets_used"] == 4 and o["out_used"] == 2 * (700 + FRAG) and o["carry_used"] == 2 * (904 + 3 * FRAG + 8)
    z = np.zeros(2, dtype=np.uint64)
    r = fr.new_receivers(1, 4)
    s = np.zeros(4, dtype=fr.RX_SLOT_DTYPE)
    with pytest.raises(NativeError) as err:   # a NULL payload with payload_len != 0 is refused
        lib_call_null_payload(r, s, z)
    assert err.value.code == UFC_ERR_INVALID_ARG
    a = [None, 0, None, None, 0, None, None, 8, None, None, 0, None, None, 0, None, 0, None, 0, None, None, None, 0,
         None, None, None, 0, None, None, None, None, 1]
    assert fr.lib().ufc_receive_packets_host(*a) == 0   # no receivers: UFC_OK whatever the pointers


def lib_call_null_payload(r, s, z):
    import ctypes
    res = np.zeros(1, dtype=fr.RECEIVER_RESULT_DTYPE)
    u = [ctypes.c_uint64(0) for _ in range(3)]
    rc = fr.lib().ufc_receive_packets_host(None, 0, None, None, 0, None, None, 8, z.ctypes.data, r.ctypes.data, 1,
                                           s.ctypes.data, np.array([0, 4], dtype=np.uint64).ctypes.data, 4, None, 0,
                                           None, 0, z.ctypes.data, ctypes.addressof(u[0]), None, 0, z.ctypes.data,
                                           ctypes.addressof(u[1]), None, 0, ctypes.addressof(u[2]), None,
                                           res.ctypes.data, r.ctypes.data, 1)
    fr.check(rc, "ufc_receive_packets_host")


# Branches the random batches must reach (receive_expect.PacketReceiver.tags), beside every item status.
BRANCHES = ("multi_completed", "empty_packet", "channel_stalled", "channel_not_ready", "window_stalled",
            "channel_base_unset", "alloc_refused_then_fits", "resync_full", "resync_stopped_at_entry", "resync_ignored",
            "window_passed_undelivered", "stale_overwritten", "active_cleared")


def random_run(call, seed, n_receivers, steps=4, windows=(1, 8, 64), **kw):
    """`steps` random steps with the carry swapped each time; returns the status totals and the tags seen."""
    rng = np.random.default_rng(seed)
    rxs = [E.PacketReceiver(windows[r % len(windows)], int(rng.integers(0, 1 << 20)) | 3 if r % 2 else 0xFFFFF - r,
                            4000 if r % 5 == 1 else 1 << 30) for r in range(n_receivers)]
    txs = [E.GenSender(rx.base_id) for rx in rxs]
    held = [[] for _ in rxs]
    h = E.Harness(rxs, call)
    total = np.zeros(11, dtype=np.int64)
    for k in range(steps):
        _, exp = h.step(E.gen_step(rng, rxs, txs, held), what=f"seed {seed} step {k}", **kw)
        total += np.sum(exp["counts"], axis=0)
    return total, set().union(*[rx.tags for rx in rxs])


@pytest.mark.parametrize("nthreads", [1, 4])
def test_random_multi_step_runs(nthreads):
    total, tags = np.zeros(11, dtype=np.int64), set()
    for seed in range(4):
        t, g = random_run(host, seed, 12, nthreads=nthreads)
        total += t
        tags |= g
    # the generator's condition: every item status and every branch below occurs
    assert np.all(total > 0), total
    for tag in BRANCHES:
        assert tag in tags, tag
    assert total[fr.RX_DUD] > 0


def test_first_fragment_alone_with_default_caps():
    """One first fragment of a 64-fragment packet: the slot holds the whole buffer, 92 680 bytes for 1448 of
    payload, and the wrapper's default caps take it; the rest arrives a step later."""
    rng = np.random.default_rng(9)
    data = rnd(rng, 64 * FRAG - 3)
    fr64 = frags(0, 0, 0, 0, data)
    rx = E.PacketReceiver(4, 0, 1 << 30)
    receivers, slots, slot_first, carry = E.new_state([rx])
    b = E.simple_batch([[fr64[0]]])
    o = host(b.infos, b.items, b.payload, b.frame_first, receivers, slots, slot_first, carry)
    assert o["carry_used"] == 64 * FRAG + 8 == o["carry_out"].size and o["packets_used"] == 0
    b = E.simple_batch([fr64[1:]], per_frame=20)
    o = host(b.infos, b.items, b.payload, b.frame_first, o["receivers_out"], slots, slot_first, o["carry_out"])
    assert o["packets_used"] == 1 and o["out_bytes"][:o["out_used"]].tobytes() == data and o["carry_used"] == 0
    # the header's bound, from the batch alone
    assert E.carry_bound(E.simple_batch([[fr64[0]]]), 0, 4) >= 64 * FRAG + 8


def test_unaligned_carry_is_refused():
    rx = E.PacketReceiver(4, 0, 1 << 30)
    receivers, slots, slot_first, _ = E.new_state([rx])
    b = E.simple_batch([[(0, 0, 0, 0, 0, 0, b"x")]])
    with pytest.raises(NativeError) as err:   # the bit words are read as 8-byte words
        host(b.infos, b.items, b.payload, b.frame_first, receivers, slots, slot_first, np.zeros(9, np.uint8)[1:])
    assert err.value.code == UFC_ERR_INVALID_ARG


def test_emit_to_receive_end_to_end():
    rng = np.random.default_rng(8)
    n_senders, per = 3, 20
    packets = np.zeros(n_senders * per, dtype=fr.PACKET_DTYPE)
    sizes = rng.choice([0, 5, 300, FRAG, FRAG + 1, 3 * FRAG + 7], size=packets.size)
    packets["data_len"] = sizes
    packets["data_offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packets["channel_id"] = rng.integers(0, 4, packets.size)
    packets["mode"] = fr.SEND_RELIABLE
    payload = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    senders = np.zeros(n_senders, dtype=fr.SENDER_DTYPE)
    senders["base_id"] = senders["next_id"] = [0, 0xFFFF0, 77]
    senders["window_size"], senders["max_alloc"], senders["take"] = 64, 1 << 30, per
    senders["window_parent_id"] = fr.NO_PARENT
    senders["channel_parent_id"] = fr.NO_PARENT
    items, flush_first, _, sres, _, used = fr.emit_packets_host(packets, np.arange(n_senders + 1) * per, senders)
    assert np.all(sres["packets_emitted"] == per)
    # each sender's items shuffled and some duplicated, one frame of items per 6
    infos, order, ff = [], [], [0]
    for s in range(n_senders):
        idx = np.arange(int(flush_first[s]), int(flush_first[s + 1]))
        idx = rng.permutation(np.concatenate([idx, rng.choice(idx, 7)]))
        for k in range(0, idx.size, 6):
            info = np.zeros(1, dtype=fr.FRAME_INFO_DTYPE)
            info["kind"], info["ok"], info["item_first"], info["item_count"] = 10, 1, len(order), len(idx[k: k + 6])
            infos.append(info)
            order += idx[k: k + 6].tolist()
        ff.append(len(infos))
    batch = E.Batch(np.concatenate(infos), items[order], payload, ff)
    rxs = [E.PacketReceiver(64, int(b), 1 << 30) for b in senders["base_id"]]
    o, _ = E.Harness(rxs, host).step(batch, what="emit to receive")
    assert o["packets_used"] == packets.size
    for s in range(n_senders):
        recs = o["packets"][int(o["packet_first"][s]): int(o["packet_first"][s + 1])]
        for c in range(4):
            got = [o["out_bytes"][int(p["out_offset"]): int(p["out_offset"]) + int(p["len"])].tobytes()
                   for p in recs if p["channel_id"] == c]
            want = [payload[int(p["data_offset"]): int(p["data_offset"]) + int(p["data_len"])].tobytes()
                    for p in packets[s * per: (s + 1) * per] if p["channel_id"] == c]
            assert got == want, (s, c)


def test_receive_core_under_sanitizers():
    """tests/c/receive_host_check.hip: the receive core (the walk, the finish, the duplicate table) and the copy
    as the GPU form makes it (chunks found by binary search) as host code under AddressSanitizer and UBSan, over
    exact-size buffers, against the senders' own record; a stand-alone program (nothing is loaded into Python
    under a sanitizer)."""
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(HERE, "c", "receive_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "receive_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
