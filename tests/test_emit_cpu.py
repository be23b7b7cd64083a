"""CPU: the batched host packet emit (ufc_emit_packets_host, uflow_amd.frame.emit_packets_host) against
tests/emit_expect.py, PacketSender::emit_packet and PendingPacket of src/half_connection restated packet by
packet; and emit -> pack -> emit again against the interleaved new-packet loop of emit_data_frames."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import codec as C
from uflow_amd import _native
from uflow_amd._build import HIPCC, REPO_DIR
from uflow_amd.frame import (FLUSH_DTYPE, ITEM_DTYPE, PACKET_DTYPE, SENDER_DTYPE, SENDER_RESULT_DTYPE, build_batch_host,
                             emit_packets_host, pack_host)

import emit_expect as EE
import pack_expect as PE


def _emit(packets, first, senders, nthreads=1, items_cap=None, slack=16, **kw):
    """The host emit into items pre-filled with EE.FILL (slack rows more than the expected total, or items_cap)."""
    exp = EE.expect(packets, first, senders)
    cap = exp.items_used + slack if items_cap is None else items_cap
    items = EE.filled_items(max(cap, exp.items_used) + slack)
    got = emit_packets_host(packets, first, senders, items_cap=cap, items=items, nthreads=nthreads, **kw)
    EE.check(got, exp, items_cap=cap)
    return got, exp


def _run(batch, **kw):
    return _emit(*batch.arrays(), **kw)


def _tuples(exp, packets, a, b):
    """(sequence_id, channel_id, window_parent_lead, channel_parent_lead, resend) of the emitted packets a..b."""
    out = []
    for i in range(a, b):
        pr = exp.packet_results[i]
        if pr["status"] == EE.EMITTED:
            it = exp.items[int(pr["item_first"])]
            out.append((int(pr["sequence_id"]), int(packets[i]["channel_id"]), int(it["window_parent_lead"]),
                        int(it["channel_parent_lead"]), bool(pr["resend"])))
    return out


def test_reference_cases():
    """packet_sender.rs's tests `basic` and `parent_leads`, by the tuples their asserts list."""
    b, want = EE.reference_cases()
    (items, ff, pres, sres, sout, used), exp = _run(b)
    packets, first, _ = b.arrays()
    for s, w in enumerate(want):
        assert _tuples(exp, packets, int(first[s]), int(first[s + 1])) == w
        assert sres["stop"][s] == EE.DONE and sres["packets_emitted"][s] == len(w)
    assert sout["next_id"][1] == 8 and sout["window_parent_id"][1] == 7
    assert list(sout["channel_parent_id"][1][:3]) == [6, 7, EE.NO_PARENT]


def test_alloc_size_table_and_fragment_emission():
    for size, want in EE.ALLOC_SIZE_TABLE:
        assert EE.alloc_size(size) == want
        (_, _, _, _, sout, _), _ = _run(EE.Senders().add([EE.pkt(size)]))
        assert sout["alloc"][0] == want, size
    b = EE.edge_cases()
    (items, ff, pres, *_), exp = _run(b)
    a = int(ff[b.index("fragment_emission")])
    got = [(int(i["fragment_id"]), int(i["fragment_id_last"]), int(i["data_len"])) for i in items[a:a + 4]]
    assert got == [(0, 0, 0), (0, 0, EE.MAX_FRAGMENT_SIZE), (0, 1, EE.MAX_FRAGMENT_SIZE), (1, 1, 1)]


def test_parent_leads_acknowledgement():
    """The reference's test of that name over 300 rounds of acknowledge + emit, the ids wrapping on the way; the
    state goes from call to call through senders_out, and is acknowledged in the helper's restatement."""
    start = (1 << 20) - 7 * 150 - 3
    tx = EE.Tx(EE.MAX_PACKET_WINDOW_SIZE, start, 10000)
    q = [EE.pkt(4, ch, mode) for ch, mode in EE.ACK_ROUND]
    carried = None
    wrapped = False
    for i in range(300):
        ref_id = (start + 7 * i) & EE.ID_MASK
        tx.acknowledge(ref_id)
        b = EE.Senders().add(q, tx=tx, flush_id=i & EE.ID_MASK)
        packets, first, senders = b.arrays()
        if carried is not None:  # the library's own state, acknowledged: base_id, alloc and the parents change
            for fld in ("next_id", "window_size", "max_alloc"):
                assert carried[fld] == senders[fld][0]
        exp = EE.expect(packets, first, senders, txs=[tx])
        got = emit_packets_host(packets, first, senders)
        EE.check((got[0],) + got[1:], exp, items_cap=exp.items_used)
        want = [((ref_id + k) & EE.ID_MASK,) + w for k, w in enumerate(EE.ACK_ROUND_WANT)]
        assert _tuples(exp, packets, 0, 7) == want, i
        wrapped = wrapped or int(got[4]["next_id"][0]) < ref_id
        carried = got[4][0]
    assert wrapped


@pytest.mark.parametrize("nthreads", [1, 4])
def test_edge_cases(nthreads):
    b = EE.edge_cases()
    (items, ff, pres, sres, sout, used), exp = _run(b, nthreads=nthreads)
    r = lambda name: sres[b.index(name)]  # noqa: E731
    # the cases are what they claim to be
    assert r("lengths")["stop"] == EE.DONE and r("lengths")["item_count"] == 1 + 1 + 1 + 1 + 2 + 2 + 3
    assert r("too_long")["stop"] == EE.BAD_PACKET and r("too_long")["packets_consumed"] == 1
    assert sout["next_id"][b.index("id_wrap")] == 3
    a = int(ff[b.index("id_wrap")])
    assert [int(x) for x in items["id"][a:a + 5]] == [0xFFFFE, 0xFFFFF, 0, 1, 2]
    assert [int(x) for x in items["channel_parent_lead"][a:a + 5]] == [3, 4, 1, 4, 3]
    assert r("window_size_1")["stop"] == EE.WINDOW_LIMITED and r("window_size_1")["packets_emitted"] == 1
    assert r("window_size_4096")["packets_emitted"] == 6
    assert [int(r(f"window_{k}_of_3")["stop"]) for k in (2, 3, 4)] == [EE.DONE, EE.DONE, EE.WINDOW_LIMITED]
    assert r("window_4_of_3")["packets_emitted"] == 3
    assert r("window_full")["stop"] == r("window_overfull")["stop"] == EE.WINDOW_LIMITED
    assert [int(r(f"alloc_{n}_of_1896")["stop"]) for n in (1895, 1896, 1897)] == [EE.DONE, EE.DONE, EE.ALLOC_LIMITED]
    assert sout["alloc"][b.index("alloc_1896_of_1896")] == 2 * EE.MAX_FRAGMENT_SIZE
    assert r("alloc_rounded_fragment_fits")["stop"] == EE.DONE
    assert r("alloc_rounded_fragment_limited")["stop"] == r("alloc_over_max")["stop"] == EE.ALLOC_LIMITED
    x = r("stale_before_window_stop")
    assert (x["stop"], x["packets_consumed"], x["packets_dropped"], x["bytes_dropped"]) == (EE.WINDOW_LIMITED, 4, 2, 15)
    x = r("stale_before_alloc_stop")
    assert (x["stop"], x["packets_consumed"], x["packets_dropped"]) == (EE.ALLOC_LIMITED, 1, 1)
    assert r("stale_and_bad")["stop"] == EE.BAD_PACKET and r("stale_and_bad")["packets_dropped"] == 0
    assert r("bad_mode")["packets_consumed"] == 1 and r("bad_first")["packets_consumed"] == 0
    a = int(ff[b.index("all_channels_reliable")])
    assert [int(x) for x in items["channel_parent_lead"][a + 64:a + 128]] == list(range(1, 128, 2))
    for name in ("made_up_parents", "made_up_parents_2"):
        assert items["flags"][int(ff[b.index(name)])] == 0, name
    assert items["flags"][int(ff[b.index("made_up_parents")]) + 1] == 1
    assert [int(r(f"take_{t}")["packets_consumed"]) for t in (0, 2, 4, 9)] == [0, 2, 4, 4]
    assert r("take_ends_on_stale")["packets_dropped"] == 2 and r("take_ends_on_stale")["packets_emitted"] == 1
    assert r("reserve_3")["item_count"] == 3 + 3 + 1 and r("reserve_only")["item_count"] == 2
    assert r("empty")["item_count"] == 0 and r("all_stale")["bytes_dropped"] == 6


@pytest.mark.parametrize("nthreads", [1, 4])
def test_tile_cases(nthreads):
    b = EE.tile_cases()
    (items, ff, pres, sres, sout, used), exp = _run(b, nthreads=nthreads)
    r = lambda name: sres[b.index(name)]  # noqa: E731
    assert r("window_stop_tile_2")["stop"] == EE.WINDOW_LIMITED and 64 < r("window_stop_tile_2")["packets_consumed"] < 128
    assert r("alloc_stop_tile_3")["stop"] == EE.ALLOC_LIMITED and r("alloc_stop_tile_3")["packets_consumed"] == 144
    assert r("bad_tile_3")["stop"] == EE.BAD_PACKET and r("bad_tile_3")["packets_consumed"] == 128
    a = int(ff[b.index("parents_two_tiles_on")])
    assert int(items["channel_parent_lead"][a + 131]) == 131 - 5 and int(items["window_parent_lead"][a + 131]) == 131 - 9
    assert int(items["channel_parent_lead"][a + 135]) == 135 - 9
    x = r("stale_run_across_tiles")
    assert x["packets_dropped"] == 70 and x["packets_emitted"] == 33
    assert r("only_last_live")["packets_emitted"] == 1 and r("only_last_live")["packets_dropped"] == 199
    assert r("take_mid_tile")["packets_consumed"] == 73


def _finish_forms(packets, first, senders):
    """emit_expect.lane_cases padded with empty senders to the two sides of the finish kernel's width switch:
    n_packets == 16 * n_senders (8 lanes per sender), and one sender fewer (64)."""
    m = packets.size
    assert m % 16 == 0 and m // 16 - 1 >= senders.size
    return [EE.with_empty_senders(packets, first, senders, n) for n in (m // 16, m // 16 - 1)]


@pytest.mark.parametrize("nthreads", [1, 4])
def test_lane_cases(nthreads):
    """emit_expect.lane_cases: stops, parents and carried sums on lane 63 and on lane 0 of the next tile of the
    sender kernel, the item kernel's seams, the finish kernel's two widths.  The host call runs the serial
    walk; the facts hold the generator to what it claims (asserted on the model's output)."""
    b = EE.lane_cases()
    packets, first, senders = b.arrays()
    (items, ff, pres, sres, sout, used), exp = _emit(packets, first, senders, nthreads=nthreads)
    EE.check_facts(b, exp)
    for name in ("stop_at[64][window][stale_even]", "stop_at[128][alloc][live]", "stop_at[63][bad][live]", "window_parent_at_63",
                 "channel_parent_at_63", "only_lane_63[fragments]", "only_lane_63[alloc]", "only_lane_63[dropped]",
                 "stale_63_then_stop_64", "take_at[64]", "items_kernel_seams[straddle]", "finish_form_switch[9]"):
        assert b.facts[name], name  # the named cases exist and carry facts
    consumed = exp.sender_results["packets_consumed"]
    assert (consumed > 64).any() and (consumed == 8).any() and (consumed == 9).any()
    assert (exp.packet_results["status"] == EE.EMITTED).sum() > 1000 and exp.packet_results["item_first"].max() > 4000
    for p2, f2, s2 in _finish_forms(packets, first, senders):
        assert (p2.size <= 16 * s2.size) == (s2.size == packets.size // 16)
        _emit(p2, f2, s2, nthreads=nthreads)
    _emit(packets, first, senders, nthreads=nthreads, want_packet_results=False)
    state = senders.copy()  # senders_out == senders
    got = emit_packets_host(packets, first, state, items=EE.filled_items(exp.items_used), senders_out=state)
    EE.check(got, exp)


def test_max_packet():
    b = EE.big_case()
    (items, ff, pres, sres, *_), exp = _run(b)
    assert sres["item_count"][0] == 1 + 1 + 65536 + 1 and pres["item_count"][1] == 65536
    assert items["data_len"][2 + 65535] == EE.MAX_FRAGMENT_SIZE and items["fragment_id"][2 + 65535] == 65535


@pytest.mark.parametrize("nthreads", [1, 4])
def test_many_max_packets(nthreads):
    """66 senders of one MAX_PACKET_SIZE packet each among small ones (the GPU test's batch beyond the item
    kernel's grid): the host call, which is that test's reference, against the closed form and the restatement
    (emit_expect.check_max_packets), and the small senders against the restatement in full."""
    b, big = EE.many_max_packets()
    packets, first, senders = b.arrays()
    items, ff, pres, sres, sout, used = emit_packets_host(packets, first, senders, nthreads=nthreads)
    assert used == len(big) * 65536 + 23 and int(ff[-1]) == used
    EE.check_max_packets(items, ff, packets, first, senders, big)
    for s in sorted(set(range(senders.size)) - set(big)):
        a, z = int(first[s]), int(first[s + 1])
        e = EE.expect(packets[a:z], np.array([0, z - a], dtype=np.uint64), senders[s: s + 1])
        r = int(senders[s]["reserve_items"])
        assert int(sres[s]["item_first"]) == int(ff[s]) and int(sres[s]["item_count"]) == e.items_used == int(ff[s + 1] - ff[s])
        assert (items[int(ff[s]) + r: int(ff[s + 1])] == e.items[r:]).all(), s
        assert sout[s: s + 1].tobytes() == e.senders_out.tobytes(), s
    assert (sres["stop"] == EE.DONE).all() and (pres["status"] == EE.EMITTED).all()


def test_items_cap_in_place_and_no_packet_results():
    b = EE.tile_cases()
    packets, first, senders = b.arrays()
    exp = EE.expect(packets, first, senders)
    for cap in (0, 1, exp.items_used // 2, exp.items_used - 1):
        _emit(packets, first, senders, items_cap=cap, nthreads=2)
    _emit(packets, first, senders, want_packet_results=False)
    state = senders.copy()  # senders_out == senders
    got = emit_packets_host(packets, first, state, items=EE.filled_items(exp.items_used), senders_out=state)
    assert got[4] is state
    EE.check(got, exp)


def test_bad_ranges_empty_and_no_senders():
    b = EE.random_batch(3, 8, 30)
    packets, _, senders = b.arrays()
    n = packets.size
    cut = [0, n // 5, n // 3, n // 2]
    # [2^40, 0) reversed, [0, c1), [c1, n + 1) past the array, [n + 1, 2^40) past, [2^40, c1) reversed, [c1, c2),
    # [c2, c2) empty, [c2, c3)
    first = np.array([1 << 40, 0, cut[1], n + 1, 1 << 40, cut[1], cut[2], cut[2], cut[3]], dtype=np.uint64)
    senders = senders[:8].copy()
    senders["reserve_items"] = 2
    for nthreads in (1, 3):
        (items, ff, pres, sres, sout, used), exp = _emit(packets, first, senders, nthreads=nthreads)
        assert list(sres["stop"] == EE.BAD_RANGE) == [True, False, True, True, True, False, False, False]
        assert (sres["item_count"][[0, 2, 3, 4]] == 0).all() and sres["item_count"][6] == 2
        assert (pres["status"][cut[3]:] == 0).all()
    lib = _native.lib()
    assert lib.ufc_emit_packets_host(None, 0, None, None, 0, None, 0, None, None, None, None, None, 1) == 0
    got = emit_packets_host(np.zeros(0, PACKET_DTYPE), np.zeros(1, np.uint64), np.zeros(0, SENDER_DTYPE))
    assert got[5] == 0 and got[0].size == 0 and got[3].size == 0


def test_argument_checks():
    packets, first, senders = EE.Senders().add([EE.pkt(1)]).arrays()
    items, ff = np.zeros(1, ITEM_DTYPE), np.zeros(2, np.uint64)
    sres, used = np.zeros(1, SENDER_RESULT_DTYPE), ctypes.c_uint64(0)
    good = [packets.ctypes.data, 1, first.ctypes.data, senders.ctypes.data, 1, items.ctypes.data, 1, ff.ctypes.data, None,
            sres.ctypes.data, None, ctypes.byref(used), 1]
    lib = _native.lib()
    assert lib.ufc_emit_packets_host(*good) == 0 and used.value == 1
    for k in (0, 2, 3, 5, 7, 9, 11):  # packets, packet_first, senders, items, flush_first, sender_results, items_used
        bad = list(good)
        bad[k] = None
        assert lib.ufc_emit_packets_host(*bad) == _native.UFC_ERR_INVALID_ARG, k
    for k in (1, 4):  # n_packets, n_senders at 2^31 - 1
        bad = list(good)
        bad[k] = (1 << 31) - 1
        assert lib.ufc_emit_packets_host(*bad) == _native.UFC_ERR_INVALID_ARG, k


RANDOM_SEED = 31


def test_random_batch_exercises_the_call():
    """A condition on the inputs, from the expectation alone: every stop is common, packets are dropped and
    fragmented."""
    packets, first, senders = EE.random_batch(RANDOM_SEED).arrays()
    exp = EE.expect(packets, first, senders)
    stops = exp.sender_results["stop"]
    for why in (EE.DONE, EE.WINDOW_LIMITED, EE.ALLOC_LIMITED):
        assert (stops == why).sum() >= 0.1 * senders.size, why
    assert (stops == EE.BAD_PACKET).any()
    assert exp.sender_results["packets_dropped"].sum() > 100
    assert (exp.packet_results["item_count"] > 1).sum() > 100
    assert (exp.senders_out["window_parent_id"] != senders["window_parent_id"]).any()
    assert senders["reserve_items"].any() and (senders["take"] < 1000).any()


@pytest.mark.parametrize("nthreads", [1, 4])
def test_random_batch(nthreads):
    _run(EE.random_batch(RANDOM_SEED), nthreads=nthreads)


# ---- emit -> pack -> emit again against the reference's interleaved loop ----

def _interleaved(tx, queue, flush_id, flush_alloc, window_room):
    """The new-packet loop of emit_data_frames (half_connection/mod.rs:385-427) with empty resend and pending
    queues: emit_packet when the pending queue is empty, then push its fragments one by one into the data frame
    emitter (pack_expect.pack_flush over the encoded sizes pushed so far plus this one).  Returns (frames as
    [(first item, count)], the items pushed, the fragments left pending, packets taken off the queue)."""
    sizes, pushed, pending, i = [], [], [], 0
    while True:
        if not pending:
            while i < len(queue) and int(queue[i]["mode"]) == EE.TIME_SENSITIVE and int(queue[i]["flush_id"]) != flush_id:
                i += 1  # emit_packet's drop loop, packet_sender.rs:150-162
            if i == len(queue):
                break
            pk = queue[i]
            got = tx.emit_packet(int(pk["data_len"]), int(pk["channel_id"]), int(pk["mode"]))
            if got in (EE.WINDOW_LIMITED, EE.ALLOC_LIMITED):
                break
            i += 1
            pending = list(EE.packet_items(pk, *got[:3]))
        while pending:
            trial = sizes + [PE.encoded_size(pending[0])]
            frames, stop, _, _ = PE.pack_flush(trial, PE.DATA, flush_alloc, window_room)
            if stop != PE.DONE:  # dfe.push failed: both errors return from emit_data_frames
                return frames, pushed, pending, i
            sizes = trial
            pushed.append(pending.pop(0))
    return PE.pack_flush(sizes, PE.DATA, flush_alloc, window_room)[0], pushed, pending, i


def _frame_bytes(frames, items, payload, id0):
    out = []
    for k, (a, c) in enumerate(frames):
        dgs = [PE.item_datagram(d, bytes(payload[int(d["data_offset"]):int(d["data_offset"]) + int(d["data_len"])]))
               for d in items[a:a + c]]
        out.append(C.frame_write({"kind": "data", "sequence_id": (id0 + k) & 0xFFFFFFFF, "nonce": False, "datagrams": dgs}))
    return out


def test_emit_pack_emit_equals_the_interleaved_loop():
    """For flushes whose flush_alloc or window_room bites inside a packet, at a packet boundary and not at all:
    emit everything, pack, and when the pack stopped early emit again with take = p + 1 (p the packet that owns
    the first unpacked item) for the state to commit.  State, frames and leftover fragments are the
    reference's."""
    U, R, P, T = EE.UNRELIABLE, EE.RELIABLE, EE.PERSISTENT, EE.TIME_SENSITIVE
    b = EE.Senders().add([EE.pkt(100, 1, R), EE.pkt(5000, 1, P), EE.pkt(50, 2, T, flush_id=1), EE.pkt(200, 2, U),
                          EE.pkt(3000, 1, R), EE.pkt(9, 0, T, flush_id=1), EE.pkt(10, 2, U), EE.pkt(2000, 3, R)],
                         flush_id=2, base_id=0xFFFF0, next_id=0xFFFFD, window_parent_id=0xFFFFB,
                         channel_parents={1: 0xFFFF9, 2: 0xFFFFB}, max_alloc=9 * 1448, alloc=1448)
    packets, first, senders = b.arrays()
    payload = np.frombuffer(np.random.default_rng(5).bytes(b.arena), dtype=np.uint8)
    full = emit_packets_host(packets, first, senders)
    items, ff, pres, sres, sout, used = full
    assert sres["stop"][0] == EE.ALLOC_LIMITED and sres["packets_consumed"][0] == 7  # the last packet never fits
    sizes = [PE.encoded_size(d) for d in items]
    total = sum(sizes) + 10 * len(sizes)
    seen = set()
    limits = [(fa, 1 << 20) for fa in range(0, total, 29)] + [(1 << 40, room) for room in range(0, 12)]
    for flush_alloc, room in limits:
        tx = EE.Tx.from_record(senders[0])
        frames, pushed, pending, taken = _interleaved(tx, list(packets), 2, flush_alloc, room)
        flushes = np.zeros(1, dtype=FLUSH_DTYPE)
        flushes["kind"], flushes["flush_alloc"], flushes["window_room"], flushes["id0"] = PE.DATA, flush_alloc, room, 0xFFFFFFFE
        infos, res, frames_used = pack_host(items, ff, flushes)
        packed = int(res["items_packed"][0])
        want_state = senders.copy()
        if res["stop"][0] == PE.DONE:
            committed, left = sout, items[:0]
            seen.add("none")
        else:
            owner = np.nonzero((pres["status"] == EE.EMITTED) & (pres["item_first"] <= packed) &
                               (packed < pres["item_first"] + pres["item_count"]))[0]
            assert owner.size == 1
            p = int(owner[0])
            seen.add("boundary" if pres["item_first"][p] == packed else "inside")
            again = senders.copy()
            again["take"] = want_state["take"] = p + 1
            _, _, _, sres2, committed, _ = emit_packets_host(packets, first, again, items_cap=0)
            assert sres2["packets_consumed"][0] == p + 1 == taken
            left = items[packed:int(pres["item_first"][p] + pres["item_count"][p])]  # the next flush's reserved slots
        tx.to_record(want_state[0])
        assert committed.tobytes() == want_state.tobytes(), (flush_alloc, room)
        assert frames_used == len(frames) and packed == len(pushed)
        assert [(int(i["item_first"]), int(i["item_count"])) for i in infos[:frames_used]] == frames
        assert items[:packed].tobytes() == np.array(pushed, dtype=ITEM_DTYPE).tobytes() if pushed else packed == 0
        assert left.tobytes() == (np.array(pending, dtype=ITEM_DTYPE).tobytes() if pending else b"")
        out, off, status, _ = build_batch_host(infos[:frames_used], items, payload)
        want = _frame_bytes(frames, items, payload, 0xFFFFFFFE)
        assert bytes(out) == b"".join(want) and list(np.diff(off)) == [len(f) for f in want]
    assert seen == {"none", "boundary", "inside"}


def test_emit_core_under_sanitizers():
    """tests/c/emit_host_check.hip: the emit core and the GPU emit's tile form (ballots as 64-bit masks, the
    per-channel masks, the carries, the stop search, the item search) as host code under AddressSanitizer and
    UBSan against the serial walk, over exact-size buffers, seeded senders and emit_expect.lane_cases' numbers
    with literals; a stand-alone program (nothing is loaded into Python under a sanitizer)."""
    src = os.path.join(REPO_DIR, "tests", "c", "emit_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "emit_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
