"""ufc_receive_packets_host against the plain Python restatement of PacketReceiver / AssemblyWindow /
FragmentBuffer (tests/receive_expect.py): every record, status, state field, slot field and delivered byte, all
exact.  The golden cases are the reference's own unit tests (tests/golden/packet_receiver_cases.json)."""
import copy
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


def test_argument_table():
    """Every pointer and every limited count of ufc_receive_packets_host, over one new receiver with a frame that
    did not parse and an item no frame holds: a required pointer that is NULL, an array that is NULL beside its
    non-zero count, and a count of 2^31 - 1 are UFC_ERR_INVALID_ARG; the three nullable arguments may be NULL."""
    import ctypes
    infos, items = np.zeros(1, dtype=fr.FRAME_INFO_DTYPE), np.zeros(1, dtype=fr.ITEM_DTYPE)
    r, ro, slots = fr.new_receivers(1, 4), fr.new_receivers(1, 4), np.zeros(4, dtype=fr.RX_SLOT_DTYPE)
    accept, base, status = np.ones(1, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint8)
    payload, out = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    carry_in, carry_out = np.zeros(1, np.uint64), np.zeros(1, np.uint64)   # (8-byte aligned, as the call demands)
    ff, sf = np.array([0, 1], np.uint64), np.array([0, 4], np.uint64)
    cf, pf = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    packets, res = np.zeros(1, dtype=fr.RX_PACKET_DTYPE), np.zeros(1, dtype=fr.RECEIVER_RESULT_DTYPE)
    u = [ctypes.c_uint64(0) for _ in range(3)]
    p = lambda a: a.ctypes.data   # noqa: E731
    ok = [p(infos), 1, p(accept), p(items), 1, p(base), p(payload), 8, p(ff), p(r), 1, p(slots), p(sf), 4, p(carry_in), 8,
          p(carry_out), 8, p(cf), ctypes.addressof(u[0]), p(packets), 1, p(pf), ctypes.addressof(u[1]), p(out), 8,
          ctypes.addressof(u[2]), p(status), p(res), p(ro), 1]
    call = fr.lib().ufc_receive_packets_host
    assert call(*ok) == 0
    counts = (1, 4, 10, 13)                                   # n_frames, n_items, n_receivers, n_slots
    for k in (8, 9, 12, 18, 19, 22, 23, 26, 28, 29) + (0, 3, 6, 11, 14, 16, 20, 24) + counts:
        bad = list(ok)
        bad[k] = (1 << 31) - 1 if k in counts else None
        assert call(*bad) == UFC_ERR_INVALID_ARG, k
    for k in (2, 5, 27):                                      # frame_accept, src_base, item_status
        fine = list(ok)
        fine[k] = None
        assert call(*fine) == 0, k


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


def random_receivers(rng, n_receivers, windows):
    return [E.PacketReceiver(windows[r % len(windows)], int(rng.integers(0, 1 << 20)) | 3 if r % 2 else 0xFFFFF - r,
                             4000 if r % 5 == 1 else 1 << 30) for r in range(n_receivers)]


def random_run(call, seed, n_receivers, steps=4, windows=(1, 8, 64), gen=None, rxs_out=None, **kw):
    """`steps` random steps with the carry swapped each time; returns the status totals and the tags seen.  gen:
    options of receive_expect.gen_step; the other keywords go to the native call.  rxs_out: a list that receives
    the PacketReceivers."""
    rng = np.random.default_rng(seed)
    rxs = random_receivers(rng, n_receivers, windows)
    txs = [E.GenSender(rx.base_id) for rx in rxs]
    held = [[] for _ in rxs]
    h = E.Harness(rxs, call)
    total = np.zeros(11, dtype=np.int64)
    for k in range(steps):
        _, exp = h.step(E.gen_step(rng, rxs, txs, held, **(gen or {})), what=f"seed {seed} step {k}", **kw)
        total += np.sum(exp["counts"], axis=0)
    if rxs_out is not None:
        rxs_out += rxs
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


# The second family of random runs: receive() over several tiles of ids (the device form takes E.TILE at a time
# and carries the channels' base, count and ready flag, the window's new base and the running sums from tile to
# tile in LDS).  Windows of 128 to 1024 ids, as many new packets a step as the window has room for, three
# channels, small packets (a few of two fragments) so that the restatement stays cheap, and every kind of chaos.
TILE_WINDOWS = (128, 256, 1024)
TILE_GEN = dict(n_packets=300, sizes=(0, 1, 7, 8, 33, 64, 100, 200) * 5 + (FRAG + 9, 2 * FRAG))
# What these runs must reach (receive_expect.PacketReceiver.tags): the inputs' condition, not the kernels'.
TILE_SEEDS = (44, 45)   # (each reaches every one of TILE_BRANCHES on its own)
TILE_BRANCHES = ("ids_over_one_tile", "ids_over_two_tiles", "stalled_with_data_in_later_tile",
                 "first_delivery_in_later_tile", "advance_stopped_in_later_tile", "advance_past_a_tile_edge",
                 "advanced_over_one_tile")


def assert_tile_condition(tags, rxs):
    for tag in TILE_BRANCHES:
        assert tag in tags, tag
    receives = sum(rx.receives for rx in rxs)
    over = sum(rx.receives_over_one_tile for rx in rxs)
    assert 2 * over > receives, (over, receives)   # most receive() calls see more than a tile of ids


@pytest.mark.parametrize("nthreads", [1, 4])
def test_random_multi_tile_runs(nthreads):
    tags, rxs = set(), []
    for seed in TILE_SEEDS:
        _, g = random_run(host, seed, 12, windows=TILE_WINDOWS, gen=TILE_GEN, rxs_out=rxs, nthreads=nthreads)
        tags |= g
    assert_tile_condition(tags, rxs)


def test_launch_constants_mirror_the_source():
    """receive_expect.LAUNCH_CONSTANTS, by which the big-shape GPU tests are sized, are the source's."""
    import re
    csrc = os.path.join(HERE, "..", "uflow_amd", "csrc")
    text = ""
    for name in ("packet_receive.hip", "packet_receive.hpp", "packet_emit.hip", "packet_emit.hpp", "frame_codec_core.hpp"):
        with open(os.path.join(csrc, name)) as f:
            text += f.read()
    for name, value in E.LAUNCH_CONSTANTS.items():
        m = re.search(r"constexpr\s+uint(?:32|64)_t\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"std::min<uint64_t>\(a\.n_receivers,\s*1u << 20\)", text) and E.VERDICT_GROUPS_MAX == 1 << 20
    assert "n1 < kRxFew ? kRxThreadsFew : kRxThreads" in text
    assert E.TILE == 64 and "for (uint32_t t0 = 0; t0 < n; t0 += 64)" in text   # rx_receive_tiles


# ---- receive() over more than one tile of ids: directed scenarios (run on the device by tests/test_gpu_receive.py) ----
def chain(first, n, ch=0, size=lambda k: (7 * k) % 23):
    """n packets of consecutive ids on one channel, each the reliable parent of the next (leads of one), the
    first without a parent: every lead clears once the packet before is delivered."""
    return [(E.add(first, k), ch, 1 if k else 0, 1 if k else 0, 0, 0, iota(k, size(k))) for k in range(n)]


def delivered_ids(o):
    return o["packets"][:o["packets_used"]]["sequence_id"].tolist()


@pytest.mark.parametrize("base", [5, 0xFFFFF - 70, 256 - 20], ids=["plain", "ids_wrap_in_tile_1", "ring_wraps_in_tile_0"])
def test_tile_edge_counts(base):
    """63 to 129 ids between base and end and a full window of 128, one channel, every lead clearing: all
    delivered in id order, out_offset a running sum over the tile edge.  From 0xFFFFF - 70 the ids wrap at lead 71
    (tile 1), and so does the ring index (both are multiples of the window size apart from the base, so they wrap
    together); from 236 the ring of 256 slots wraps at lead 20, inside tile 0."""
    counts = (63, 64, 65, 127, 128, 129, 128)
    windows = (128, 128, 128, 128, 128, 256, 128)   # (the last: n == W)
    rxs = [E.PacketReceiver(W, base, 1 << 30) for W in windows]
    h = E.Harness(rxs, host)
    o, exp = h.step(E.simple_batch([chain(base, n) for n in counts], per_frame=50), what=f"edge counts from {base}")
    for r, n in enumerate(counts):
        recs = o["packets"][int(o["packet_first"][r]): int(o["packet_first"][r + 1])]
        assert recs["sequence_id"].tolist() == [E.add(base, k) for k in range(n)], (r, n)
        assert recs["len"].tolist() == [(7 * k) % 23 for k in range(n)]
        assert np.array_equal(np.diff(recs["out_offset"].astype(np.int64)), recs["len"][:-1]), (r, n)
        assert rxs[r].base_id == E.add(base, n) and int(o["results"][r]["advanced"]) == n
    assert o["carry_used"] == 0 and "advance_past_a_tile_edge" in rxs[2].tags


def test_stall_in_tile_0_holds_the_later_tiles():
    """Channel 1 (the even leads) stalls at lead 10: its reliable parent, lead 8, is withheld.  Everything it has in
    tiles 1 and 2 would clear on its own leads (the first of each tile names no parent, the others the packet
    before) and none of it may go; channel 2 (the odd leads) is delivered throughout.  A step later the parent
    arrives and the rest goes in order."""
    base, n = 0xFFFFF - 100, 192
    rx = E.PacketReceiver(256, base, 1 << 30)
    h = E.Harness([rx], host)
    dgs = []
    for k in range(n):
        seq, data = E.add(base, k), iota(k, k % 19)
        if k % 2:       # channel 2, unreliable; from lead 9 on the packet before it is the window's parent
            dgs.append((seq, 2, 1 if k > 8 else 0, 0, 0, 0, data))
        elif k < 8:
            dgs.append((seq, 1, 0, 0, 0, 0, data))
        elif k == 8:    # channel 1 is reliable from here on: each names the one before as both parents
            parent = (seq, 1, 0, 0, 0, 0, data)
        else:
            dgs.append((seq, 1, 2, 0 if k % 64 < 2 else 2, 0, 0, data))
    o, exp = h.step(E.simple_batch([dgs], per_frame=64), what="stalled")
    got = exp["delivered"][0]
    assert [d[0] for d in got if d[1] == 1] == [E.add(base, k) for k in (0, 2, 4, 6)]
    assert [d[0] for d in got if d[1] == 2] == [E.add(base, k) for k in range(1, n, 2)]
    assert "stalled_with_data_in_later_tile" in rx.tags and rx.base_id == E.add(base, 8)
    o, exp = h.step(E.simple_batch([[parent]]), what="released")
    assert delivered_ids(o) == [E.add(base, k) for k in range(8, n, 2)]
    assert o["carry_used"] == 0 and rx.base_id == E.add(base, n)


@pytest.mark.parametrize("variant", ["all", "part", "count_runs_out"])
def test_channel_count_across_the_tile_edge(variant):
    """70 packets of one channel held over a step without delivery, across the tile edge: receive() starts with
    channel_packet_count = 70 and the ready flag set, and the count that is left and the ready flag are the
    restatement's.  `part`: lead 65 is withheld and lead 66 names it, so 65 packets go and 5 stay.
    `count_runs_out`: the header says 66 where 70 wait (state no run produces; the restatement delivers 66 and
    clears the ready flag with the last of them, in tile 1)."""
    base = 0xFFFFF - 30
    rx = E.PacketReceiver(128, base, 1 << 30)
    h = E.Harness([rx], host)
    if variant == "part":
        dgs = [(E.add(base, k), 4, int(k == 66), int(k == 66), 0, 0, iota(k, 1 + k % 9)) for k in range(71) if k != 65]
    else:
        dgs = [(E.add(base, k), 4, 0, 0, 0, 0, iota(k, 1 + k % 9)) for k in range(70)]
    o, _ = h.step(E.simple_batch([dgs], per_frame=32, deliver=[0]), what="held")
    assert o["packets_used"] == 0 and rx.channels[4].packet_count == 70 and rx.channel_ready_flags == 1 << 4
    if variant == "count_runs_out":
        rx.channels[4].packet_count = 66
        h.receivers["channel_packet_count"][0, 4] = 66
    o, _ = h.step(E.simple_batch([[]]), what=variant)
    want, left = {"all": (70, 0), "part": (65, 5), "count_runs_out": (66, 0)}[variant]
    assert delivered_ids(o) == [E.add(base, k) for k in range(want)]
    assert int(o["receivers_out"][0]["channel_packet_count"][4]) == left == rx.channels[4].packet_count
    assert int(o["receivers_out"][0]["channel_ready_flags"]) == 0 and "ids_over_one_tile" in rx.tags


@pytest.mark.parametrize("stop", [False, True], ids=["runs_through", "stops_at_the_edge"])
def test_window_advance_over_the_tile_edge(stop):
    """ENTRY slots at leads 62, 63 (tile 0) and 64, 65 (tile 1), each naming the packet before as its window
    parent: the advance runs through, on the new base carried over the edge.  With lead 64 withheld, lead 65
    fails (an entry next to a cleared one cannot: its lead is measured from the new base) and the advance stops
    at base + 64, whatever clears in tile 2: channel bases are unset only in (base, base + 64], the allocation is
    given back by the cleared slots only (a CLOSED entry at 62 and 63, an ACTIVE buffer at lead 10; the ACTIVE
    buffer at lead 70 and the entries beyond stay)."""
    rng = np.random.default_rng(21)
    base = 0xFFFFF - 63   # the ids wrap at the tile edge
    rx = E.PacketReceiver(256, base, 1 << 30)
    h = E.Harness([rx], host)
    at = lambda k: E.add(base, k)  # noqa: E731
    dgs = [frags(at(10), 3, 0, 0, rnd(rng, FRAG + 40))[1], frags(at(70), 3, 0, 0, rnd(rng, 2 * FRAG))[0]]
    dgs += [(at(62), 0, 0, 0, 0, 0, b"sixty-two"), (at(63), 0, 1, 0, 0, 0, b"sixty-three")]
    if not stop:
        dgs.append((at(64), 0, 1, 0, 0, 0, b"sixty-four"))
    dgs += [(at(65), 1, 1, 0, 0, 0, b"sixty-five"), (at(130), 5, 0, 0, 0, 0, b"tile two"), (at(131), 5, 0, 0, 0, 0, b"too")]
    o, _ = h.step(E.simple_batch([dgs]), what="advance")
    out = o["receivers_out"][0]
    if stop:
        assert rx.base_id == at(64) and "window_stalled" in rx.tags and "advance_stopped_in_later_tile" in rx.tags
        assert int(out["channel_base_id"][0]) == E.NONE and int(out["channel_base_id"][1]) == at(66)
        assert int(out["alloc"]) == 2 * FRAG + len(b"sixty-five") + len(b"tile two") + len(b"too")
    else:
        assert rx.base_id == at(132) and "advance_past_a_tile_edge" in rx.tags
        assert int(out["channel_base_id"][5]) == E.NONE and int(out["alloc"]) == 0
    assert int(out["base_id"]) == rx.base_id and "active_cleared" in rx.tags
    assert delivered_ids(o) == [at(k) for k in (62, 63, 64, 65, 130, 131) if not (stop and k == 64)]


def test_window_not_ready_with_deliveries_in_tile_2():
    """window_ready is 0 (no arrival's window lead cleared) while channels deliver in tile 2: the channels' state
    and the ready flags are written, the window does not move, end_id stays."""
    base = 0xFFFFF - 140
    rx = E.PacketReceiver(256, base, 1 << 30)
    h = E.Harness([rx], host)
    at = lambda k: E.add(base, k)  # noqa: E731
    dgs = [(at(130 + k), 0, 5, 0, 0, 0, b"zero %d" % k) for k in range(4)]
    dgs += [(at(135), 1, 5, 0, 0, 0, b"one"), (at(145), 1, 5, 6, 0, 0, b"waits for 139"), (at(150), 2, 9, 0, 0, 0, b"two")]
    o, _ = h.step(E.simple_batch([dgs]), what="window not ready")
    out = o["receivers_out"][0]
    assert delivered_ids(o) == [at(k) for k in (130, 131, 132, 133, 135, 150)]
    assert (int(out["base_id"]), int(out["end_id"]), int(out["window_ready"])) == (base, at(151), 0)
    assert int(out["channel_ready_flags"]) == 0 and int(out["channel_packet_count"][1]) == 1
    assert int(o["results"][0]["advanced"]) == 0 and "first_delivery_in_later_tile" in rx.tags


# The cross-lane reads of the tiled receive on lane 63 (a full tile: window 64) and on lane 0 of the second tile
# (window 128); the same cases, with the same numbers, run in tests/c/receive_host_check.hip under
# three lane orders.  The event's lead is 63 or 64; the lane before it, in its channel or among the entries, is lead
# 60.  Every case asserts on the model's side that the event decides what it was meant to decide.
LANE_BASE = 0xFFFFF - 20    # (the ids wrap at lead 21)
LANE_EVENTS = [(64, 63), (128, 64)]


def lane_step(window, dgs, what):
    rx = E.PacketReceiver(window, LANE_BASE, 1 << 30)
    h = E.Harness([rx], host)
    o, exp = h.step(E.simple_batch([[(E.add(LANE_BASE, k), ch, wl, cl, 0, 0, iota(k, n)) for k, ch, wl, cl, n in dgs]],
                                   per_frame=64), what=what)
    return rx, o, [E.sub(d[0], LANE_BASE) for d in exp["delivered"][0]]


@pytest.mark.parametrize("window,ev", LANE_EVENTS)
def test_channel_base_from_the_lane_before(window, ev):
    """The event's packet names lead 60 as its channel parent: it clears only against the channel base that lead 60
    leaves (61); measured from the carried base (none: the window's) it would fail.  Its window parent, the id before
    it, never came: the window stops in front of it."""
    gap = ev - 60
    rx, o, leads = lane_step(window, [(60, 4, 0, 0, 5), (ev, 4, 1, gap, 6)], "channel base")
    assert leads == [60, ev] and not gap > ev and gap > ev - 61   # (lead_clears: lead == 0 or lead > distance)
    out = o["receivers_out"][0]
    assert (int(out["channel_packet_count"][4]), int(out["channel_ready_flags"]), int(out["base_id"])) == (0, 0, E.add(LANE_BASE, 61))


@pytest.mark.parametrize("window,ev", LANE_EVENTS)
def test_entry_prefix_from_the_lane_before(window, ev):
    """The same for the window advance: the event's entry names lead 60 as its window parent and passes only
    against the new base that lead 60 leaves."""
    gap = ev - 60
    rx, o, leads = lane_step(window, [(60, 4, 0, 0, 5), (ev, 5, gap, 0, 6)], "entry prefix")
    assert leads == [60, ev] and not gap > ev and gap > ev - 61 and "window_stalled" not in rx.tags
    out = o["receivers_out"][0]
    assert (int(out["base_id"]), int(o["results"][0]["advanced"]), int(out["alloc"])) == (E.add(LANE_BASE, ev + 1), ev + 1, 0)


@pytest.mark.parametrize("window,ev", LANE_EVENTS)
def test_only_failing_lane_of_its_channel(window, ev):
    """The event's lane is the only failing lane of its channel (its parent, two before it, never came): not
    delivered, the ready flag cleared, one packet left; the window stops in front of it too."""
    rx, o, leads = lane_step(window, [(10, 4, 0, 0, 5), (20, 4, 0, 0, 7), (ev, 4, 2, 2, 6), (5, 9, 0, 0, 1)], "failing lane")
    assert leads == [5, 10, 20] and "channel_stalled" in rx.tags and "window_stalled" in rx.tags
    out = o["receivers_out"][0]
    assert (int(out["channel_packet_count"][4]), int(out["channel_ready_flags"]), int(out["base_id"])) == (1, 0, E.add(LANE_BASE, 21))
    assert int(out["channel_base_id"][4]) == E.NONE


def test_lengths_at_lane_63_and_at_lane_0_of_tile_2():
    """128 ids delivered, lengths 1 but 200 at lead 63 and 77 at lead 64: tile 2's offsets and the used bytes carry
    lane 63's length."""
    size = lambda k: 200 if k == 63 else 77 if k == 64 else 1  # noqa: E731
    rx, o, leads = lane_step(128, [(k, 4, int(k > 0), int(k > 0), size(k)) for k in range(128)], "lengths")
    assert leads == list(range(128)) and o["out_used"] == 126 + 277
    recs = o["packets"][:128]
    assert recs["len"].tolist() == [size(k) for k in range(128)]
    assert recs["out_offset"].tolist() == [sum(size(j) for j in range(k)) for k in range(128)]
    assert rx.base_id == E.add(LANE_BASE, 128)


TILE_SCENARIOS = [test_stall_in_tile_0_holds_the_later_tiles, test_window_not_ready_with_deliveries_in_tile_2,
                  test_lengths_at_lane_63_and_at_lane_0_of_tile_2]
for _w, _ev in LANE_EVENTS:
    TILE_SCENARIOS += [pytest.param(lambda f=f, w=_w, ev=_ev: f(w, ev), id=f"{f.__name__[5:]}_{_ev}")
                       for f in (test_channel_base_from_the_lane_before, test_entry_prefix_from_the_lane_before,
                                 test_only_failing_lane_of_its_channel)]
TILE_SCENARIOS += [pytest.param(lambda b=b: test_tile_edge_counts(b), id=f"tile_edge_counts_{b}") for b in (5, 0xFFFFF - 70, 236)]
TILE_SCENARIOS += [pytest.param(lambda v=v: test_channel_count_across_the_tile_edge(v), id=f"channel_count_{v}")
                   for v in ("all", "part", "count_runs_out")]
TILE_SCENARIOS += [pytest.param(lambda s=s: test_window_advance_over_the_tile_edge(s), id=f"window_advance_stop_{s}")
                   for s in (False, True)]


# ---- the copies: the cap inside a chunk, and every alignment ----
def held_state(call):
    """One receiver after two steps without delivery: a 3-byte packet (so that the next one's delivered bytes
    start at an odd offset), a 5000-byte packet of four fragments, and an ACTIVE buffer with two of its three
    fragments.  Returns (harness, the three steps' batches): the harness has run the first `steps`."""
    rng = np.random.default_rng(22)
    rx = E.PacketReceiver(8, 0xFFFF8, 1 << 30)   # (the carry is laid out in slot order: these are slots 0, 1, 2)
    big, part = frags(0xFFFF9, 0, 0, 0, rnd(rng, 5000)), frags(0xFFFFA, 1, 0, 0, rnd(rng, 2 * FRAG + 77))
    first = E.simple_batch([[(0xFFFF8, 0, 0, 0, 0, 0, b"odd")] + big[::-1] + [part[2], part[0]]], deliver=[0])
    return E.Harness([rx], call), [first, E.simple_batch([[]], deliver=[0]), E.simple_batch([[]])]


# The cap in turn inside the head bytes of a copy (delivered bytes only: a carry destination is 8-byte aligned),
# inside the word body, inside the tail of chunk 0, at the chunk's edge, inside chunk 1 and inside the next segment.
CARRY_CAPS = (8 + 1001, 8 + E.RX_CHUNK - 1, 8 + E.RX_CHUNK, 8 + 3000, 5008 + 100, 5008 + FRAG + 5)
OUT_CAPS = (2, 5, 3 + 5 + 994, 3 + E.RX_CHUNK - 2, 3 + E.RX_CHUNK, 3 + 3000)


@pytest.mark.parametrize("step", [0, 1, 2], ids=["datagrams_to_carry", "carry_to_carry", "carry_to_out"])
def test_cap_inside_a_chunk(step):
    """carry_cap (the datagrams' copy into the carry, then the slot copy from carry to carry) and out_cap (the
    slot copy of the delivering step) below the need, falling inside a copy: the bytes below the cap are right,
    nothing at or beyond it is written (check() compares the whole pre-filled arrays), the used counts exact."""
    for cap in (OUT_CAPS if step == 2 else CARRY_CAPS):
        h, batches = held_state(host)
        for k in range(step):
            h.step(batches[k], what=f"before, step {k}")
        o, _ = h.step(batches[step], caps={"out" if step == 2 else "carry": cap}, what=f"step {step} cap {cap}")
        assert o["carry_used"] == 8 + 5000 + 3 * FRAG + 8 - (5008 if step == 2 else 0)
        assert o["out_used"] == (5003 if step == 2 else 0)


ALIGN_LENGTHS = tuple(range(18)) + (23, 24, 25)


def aligned_packets(lengths_and_alignments, base=0xFFFFF - 9):
    """One receiver's batch of single-fragment packets of consecutive ids on one channel without parents, given as
    (length, delivered offset mod 8, payload offset mod 8): a filler packet in front of each moves the running sum
    of the delivered lengths, padding in the payload arena the source.  Returns (Batch, [(length, dst & 7, src & 7)]
    as the inputs have them: the delivered offset from the lengths in id order, the source from the items)."""
    rng = np.random.default_rng(23)
    arena = E.PayloadArena(rng)
    items, got, seq = [], [], base
    for ln, d, s in lengths_and_alignments:
        for size, src in (((d - sum(int(it["data_len"]) for it in items)) % 8, None), (ln, s)):
            if src is not None:
                arena.put(bytes((src - len(arena.buf)) % 8))
            data = rnd(rng, size)
            last = max((size + FRAG - 1) // FRAG, 1) - 1
            first = len(items)
            items += [E.make_item(seq, 0, 0, 0, f, last, arena.put(data[f * FRAG: (f + 1) * FRAG]),
                                  len(data[f * FRAG: (f + 1) * FRAG])) for f in range(last + 1)]
            if src is not None:
                before = sum(int(it["data_len"]) for it in items[:first])
                got.append((sum(int(it["data_len"]) for it in items[first:]), before & 7, int(items[first]["data_offset"]) & 7))
            seq = E.add(seq, 1)
    infos, arr, ff = E.frames_of([items], per_frame=100)
    return E.Batch(infos, arr, arena.array(), ff), got


def test_item_copy_alignments():
    """The copy of a datagram's bytes (16 lanes, head / 8-byte words / tail): lengths 0..17 and 23..25, delivered
    in the step they arrive in; destination and source together take all 64 (dst & 7, src & 7) pairs in each length
    class (below 8, 8 to 15, 16 and more)."""
    classes = ([n for n in ALIGN_LENGTHS if 0 < n < 8], [n for n in ALIGN_LENGTHS if 8 <= n < 16],
               [n for n in ALIGN_LENGTHS if n >= 16])
    want = [(c[(p + p // 8) % len(c)], p & 7, p >> 3) for c in classes for p in range(64)] + [(0, d, 7 - d) for d in range(8)]
    batch, got = aligned_packets(want)
    assert got == want
    assert {(min(ln // 8, 2), d, s) for ln, d, s in got if ln} == {(c, d, s) for c in range(3) for d in range(8) for s in range(8)}
    assert {ln for ln, _, _ in got} == set(ALIGN_LENGTHS)
    rx = E.PacketReceiver(1024, 0xFFFFF - 9, 1 << 30)
    o, _ = E.Harness([rx], host).step(batch, what="item copy alignments")
    assert o["packets_used"] == 2 * len(want) and o["carry_used"] == 0


def test_slot_copy_alignments():
    """The copy of a held packet (a wave per 2048-byte chunk): the same lengths and 2047, 2048, 2049, held for a
    step and delivered in the next at every destination alignment; in the carry the neighbours' sizes put them at
    every multiple of 8."""
    want = [(ln, d, (ln + d) % 8) for ln in ALIGN_LENGTHS + (E.RX_CHUNK - 1, E.RX_CHUNK, E.RX_CHUNK + 1) for d in range(8)]
    batch, got = aligned_packets(want)
    assert got == want
    batch.deliver = [0]
    rx = E.PacketReceiver(1024, 0xFFFFF - 9, 1 << 30)
    h = E.Harness([rx], host)
    o, _ = h.step(batch, what="held")
    assert o["packets_used"] == 0 and o["carry_used"] > 8 * 3 * E.RX_CHUNK
    o, _ = h.step(E.simple_batch([[]]), what="slot copy alignments")
    assert o["packets_used"] == 2 * len(want) and o["carry_used"] == 0
    assert [(int(p["len"]), int(p["out_offset"]) & 7) for p in o["packets"][1:2 * len(want):2]] == [w[:2] for w in want]


COPY_SCENARIOS = [pytest.param(lambda k=k: test_cap_inside_a_chunk(k), id=f"cap_inside_a_chunk_{k}") for k in range(3)]
COPY_SCENARIOS += [test_item_copy_alignments, test_slot_copy_alignments]


def test_many_receivers_helpers_on_the_host():
    """The big-shape GPU tests' batch builders and checks at a size the restatement affords, on the host call alone:
    pair_batch and sparse_batch against the restatement over every receiver (Harness), then check_receivers on a
    sample, check_sums and check_same (one thread against four) on the same outputs."""
    rng = np.random.default_rng(24)
    n = 150
    bases = rng.integers(0, 1 << 20, n)
    bases[::7] = 0xFFFFF
    size0, size1 = rng.integers(1, 41, n), rng.integers(1, 41, n)
    size1[5::16] += FRAG
    size0[3::50] = (2047, 2048, 4096 + 3)
    rxs = [E.PacketReceiver(2, int(b), 1 << 40) for b in bases]
    h = E.Harness(rxs, host)
    sample = E.sample_of(rng, n, (0, 7, 8, 63, 64, n - 1, 5, 21, 3, 53), 20)
    held, _ = E.pair_batch(rng, bases, size0, size1)
    extra = {r: [(10, 1, [(int(bases[r]), 0, 0, 0, 0, 0, b"again"), (E.add(int(bases[r]), 2), 0, 0, 0, 0, 0, b"beyond")])]
             for r in sample[::2]}
    for k, batch in enumerate((held, E.sparse_batch(n, extra))):
        before = (h.receivers.copy(), h.slots.copy(), h.carry.copy(), [copy.deepcopy(rxs[r]) for r in sample])
        o, exp = h.step(batch, what=f"pairs step {k}")
        if k == 0:   # the later copies: the duplicate table while a buffer is open, a closed slot otherwise
            assert fr.RX_DROPPED_DUPLICATE in exp["status"] and fr.RX_DROPPED_CLOSED in exp["status"]
        assert (o["packets_used"], int((h.slots["rx_flags"] & 2 != 0).sum())) == ((0, 2 * n) if k == 0 else (2 * n, 0))
        o4 = E.run_native(host, batch, before[0], before[1], h.slot_first, before[2], nthreads=4)
        E.check_same(o4, o, what=f"threads step {k}")
        E.check_sums(o4, h.slot_first, what=f"sums step {k}")
        sub = E.sub_batch(batch, sample)
        E.check_receivers(o4, E.expected_step(before[3], sub), before[3], sub, sample, batch.apply(before[0].copy()),
                          before[1], h.slot_first, what=f"sample step {k}")


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
