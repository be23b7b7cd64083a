"""CPU: the batched resend calls (ufc_resend_begin_host / ufc_resend_place_host / ufc_resend_commit_host) against
the hand-traced cases of tests/golden/resend_cases.json and, tick by tick over generated lossy traffic, against
tests/resend_expect.py's restatement of HalfConnection's sender half: every result field, the sender, the heap byte
for byte, the pending queue, the packet table, the ack bytes, the tx ring and the sent records.
"""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

import emit_expect as E
import resend_expect as R
from uflow_amd import _build, frame as fr
from uflow_amd._native import lib, UFC_OK, UFC_ERR_INVALID_ARG

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "resend_cases.json")) as f:
    GOLDEN = json.load(f)


def test_golden_note_says_hand_traced():
    assert "by hand" in GOLDEN["note"] and len(GOLDEN["cases"]) >= 11


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_golden(case):
    R.run_golden(case)


def test_heap_check_value_of_the_model():
    """The tie-order check value on the model's heap alone: six entries of time 100 pushed 0..5."""
    def heap():
        h = R.Heap()
        for k in range(6):
            h.push(R.HeapEntry(k, 0, 100, 1))
        return h
    h, order = heap(), []
    while h.peek().resend_time <= 100:
        e = h.pop()
        order.append(e.packet)
        h.push(R.HeapEntry(e.packet, 0, 300, 2))
    assert order == [0, 2, 5, 1, 4, 3]
    h = heap()
    assert [h.pop().packet for _ in range(6)] == [0, 2, 5, 4, 1, 3]


def lossy_configs():
    """Small capacities, so that every ring wraps within a run: a 4-packet window with pkt_cap 4 and ids through 2^20,
    a heap that fills, a stage that fills, a frame window that limits."""
    return [
        R.Config(window_size=4, max_alloc=20000, frame_window=4, frame_tail=2, heap_cap=32, base_id=0xFFFF0, frame_base=0xFFFFFFF0),
        R.Config(window_size=16, max_alloc=40000, frame_window=8, frame_tail=8, heap_cap=128, base_id=5),
        R.Config(window_size=8, max_alloc=30000, frame_window=8, frame_tail=1, heap_cap=6, base_id=0xFFFFC),   # HEAP_FULL
        R.Config(window_size=8, max_alloc=30000, frame_window=16, frame_tail=4, heap_cap=64, stage_cap=3),     # STAGE_FULL
        R.Config(window_size=32, max_alloc=60000, frame_window=16, frame_tail=16, heap_cap=256),
        R.Config(window_size=8, max_alloc=30000, frame_window=2, frame_tail=1, heap_cap=64),                   # WINDOW_LIMITED
    ]


def run(nthreads, seed, ticks, **kw):
    rng = random.Random(seed)
    p = R.Pipeline(lossy_configs(), R.HostBackend(nthreads))
    R.run_lossy(p, rng, ticks, **kw)
    return p


@pytest.fixture(scope="module")
def long_run():
    # (a connection that hangs stays hung, so the hostile acks come late)
    return run(1, 5, 150, hostile=0.3, hostile_from=125, loss=[0.25, 0.25, 0.25, 0.25, 0.1, 0.6])


def test_lossy_traffic_every_tick(long_run):
    p = long_run
    assert {R.DONE, R.SIZE_LIMITED, R.WINDOW_LIMITED, R.REF_HANG, R.STAGE_FULL, R.HEAP_FULL} <= p.seen_stops, \
        [R.STOP_NAMES[s] for s in p.seen_stops]
    assert R.BAD_STATE not in p.seen_stops
    want = {"dead_pop", "acked_pop", "resent", "partial_packet", "pending_packed", "frag_wrap", "id_wrap", "hang"}
    assert want <= p.seen, want - p.seen
    # the ack ring and the packet ring went round (the heap region was full: HEAP_FULL above)
    assert any(int(s["frag_next"]) > int(s["frag_cap"]) for s in p.states)
    assert any(R.E.sub(int(d["next_id"]), c.base_id) > 2 * c.window_size for d, c in zip(p.senders, p.cfg))


def test_tx_ring_wraps_and_skips():
    """A frame window of one frame (tx_cap 256) and ten small packets a tick: the ring goes round several times, and a
    frame whose refs would straddle its end starts at its beginning."""
    p = R.Pipeline([R.Config(window_size=64, max_alloc=1 << 20, frame_window=1, frame_tail=0, heap_cap=64)])
    assert int(p.states[0]["tx_cap"]) == 256
    rng = random.Random(3)
    R.run_lossy(p, rng, 70, loss=0.0, alloc=(1 << 20, 1 << 21),
                traffic=lambda r, t, c: [(r.randrange(20), 0, E.RELIABLE) for _ in range(r.randrange(7, 12))])
    assert {"tx_wrap", "tx_skip"} <= p.seen and int(p.states[0]["tx_head"]) > 2 * 256


def test_lossy_traffic_rtt_zero():
    p = run(1, 5, 25, rtt_ms=0, loss=0.3)
    assert {R.SIZE_LIMITED, R.WINDOW_LIMITED} & p.seen_stops


def test_threads_agree():
    a, b = run(1, 23, 30), run(4, 23, 30)
    assert a.states.tobytes() == b.states.tobytes() and a.senders.tobytes() == b.senders.tobytes()
    for k in a.arenas:
        assert a.arenas[k].tobytes() == b.arenas[k].tobytes(), k


def test_padding_changes_nothing():
    """The padding of resend_expect.Pipeline (what puts the GPU tests' launches into the lane form): the six
    connections with six replicas and sixty idle fillers in the same arrays and arenas send the same frames, tick by
    tick, and see the same events as the six alone."""
    def frames(**kw):
        p = R.Pipeline(lossy_configs(), R.HostBackend(2), **kw)
        out, tick = [], p.tick
        p.tick = lambda *a, **k: (out.append(tick(*a, **k)), out[-1])[1]
        R.run_lossy(p, random.Random(5), 40, loss=0.3)
        return p, out

    plain, want = frames()
    padded, got = frames(replicas=6, fillers=60)
    assert padded.total == 72 and plain.total == plain.n == 6
    assert list(padded.src[:6]) == list(range(6)) and sorted(padded.src[6:])[60:] == list(range(6))
    assert got == want and len(got) == 40 and any(f for t in got for f in t)
    assert padded.seen == plain.seen and padded.seen_stops == plain.seen_stops
    # the replicas did the same work as their connections, the idle fillers none
    assert padded.pad_totals["heap_pushed"] > 0 and padded.pad_totals["n_resent"] > 0 and plain.pad_totals["n_resent"] == 0
    for c in np.flatnonzero(padded.src[6:] >= 0) + 6:
        s, m = padded.states[c], padded.states[padded.src[c]]
        assert (int(s["heap_len"]), int(s["tx_head"]), int(s["frag_next"])) == (int(m["heap_len"]), int(m["tx_head"]), int(m["frag_next"]))
    assert plain.states.tobytes() == padded.states[:6].tobytes()   # (the first regions lie where they lay)


# ---- the wave form's cross-lane reads on lane 63 and on lane 0 of the next tile.  The same cases,
# with the same numbers, run in tests/c/resend_host_check.hip under three lane orders; tests/test_gpu_resend.py runs
# these pipelines on the device.  Every case asserts on the model's side that its event sits where it was meant to. ----
LANE_BASE = 0xFFFF0   # (the ids pass 2^20 inside every case)


def lane_id(k):
    return (LANE_BASE + k) & E.ID_MASK


def lane_pipeline(backend, frame_window=64, frame_tail=16):
    return R.Pipeline([R.Config(window_size=128, max_alloc=1 << 20, frame_window=frame_window, frame_tail=frame_tail, heap_cap=256,
                                base_id=LANE_BASE)], backend)


def parents_pipeline(backend, at):
    """begin, the freed ids' parents: the window's parent and channel 63's are the id at lane 63 of a tile of freed ids
    (at = 63: 64 freed), or at lane 0 of the next (at = 64: 65 freed); that id's packet is the only long one, so the
    sums over the freed ids have their weight on the same lane."""
    p = lane_pipeline(backend)
    for k in range(70):
        if k == at:
            p.enqueue(0, 1000, 63, E.RELIABLE)
        else:
            p.enqueue(0, 1 + k % 5, k % 3, E.UNRELIABLE)
    p.tick(0, 1000, 1 << 30, [[]])
    m = p.models[0]
    assert m.tx.window_parent_id == lane_id(at) and m.tx.channel_parent_id[63] == lane_id(at) and m.tx.next_id == lane_id(70)
    p.tick(10, 1000, 1 << 30, [[(int(p.queues[0]["window_base_id"]), lane_id(at + 1), [])]])
    assert m.tx.window_parent_id is None and m.tx.channel_parent_id[63] is None
    assert (m.freed, m.tx.base_id, m.bytes_freed) == (at + 1, lane_id(at + 1), 1000 + sum(1 + k % 5 for k in range(at)))
    assert int(p.last["begin"][0]["packets_freed"]) == at + 1
    return p


def ack_frames_pipeline(backend):
    """begin, the ack frames' ballot: the ack that frees sits at frame 63, and the one behind it is stale only if it
    ran; then at frame 64 (lane 0 of the second tile), with a last one at 129 (lane 1 of the third)."""
    p = lane_pipeline(backend)
    for k in range(20):
        p.enqueue(0, 2 + k, k % 3, E.UNRELIABLE)
    p.tick(0, 1000, 1 << 30, [[]])
    m, fw = p.models[0], int(p.queues[0]["window_base_id"])
    p.tick(10, 1000, 1 << 30, [[(fw, lane_id(5) if i == 63 else lane_id(3) if i == 64 else LANE_BASE, []) for i in range(70)]])
    assert (m.freed, m.ignored, m.tx.base_id) == (5, 6, lane_id(5))
    assert (int(p.last["begin"][0]["packets_freed"]), int(p.last["begin"][0]["acks_ignored"])) == (5, 6)
    acks = [(fw, lane_id(9) if i == 64 else lane_id(7) if i == 65 else lane_id(11) if i == 129 else lane_id(5) if i < 64 else LANE_BASE, [])
            for i in range(130)]
    p.tick(20, 1000, 1 << 30, [acks])
    assert (m.freed, m.ignored, m.tx.base_id) == (6, 64, lane_id(11))
    assert (int(p.last["begin"][0]["packets_freed"]), int(p.last["begin"][0]["acks_ignored"])) == (6, 64)
    return p


def stop_packet_pipeline(backend, at):
    """commit, the stopping packet: a frame window of one frame; the packets in front of `at` fit it, packet `at` (1400
    bytes) does not and is the first whose items lie past the packed ones: lane 63 of the first tile of packets
    (at = 63), or lane 0 of the second (at = 64).  The frame is then acknowledged and the rest goes on."""
    p = lane_pipeline(backend, frame_window=1, frame_tail=0)
    for k in range(70):
        p.enqueue(0, 1400 if k == at else 1, k % 3, E.PERSISTENT)
    sent = p.tick(0, 1000, 1 << 30, [[]])[0]
    m = p.models[0]
    assert len(sent) == 1 and [seq for seq, _ in sent[0][1]] == [lane_id(k) for k in range(at)]
    assert len(m.pending) == 1 and m.pending[0][0].seq == lane_id(at) and m.tx.next_id == lane_id(at + 1)
    cm = p.last["commit"][0]
    assert (int(cm["take"]), int(cm["packets_entered"]), int(cm["pending_count"]), int(cm["heap_pushed"])) == (at + 1, at + 1, 1, at)
    assert int(p.states[0]["window_bytes"]) == at + 1400 == m.window_bytes
    fid = sent[0][0]
    sent = p.tick(10, 1000, 1 << 30, [[(fid + 1, LANE_BASE, [(fid, 1, 0)])]])[0]
    assert len(sent) == 1 and sent[0][1][0] == (lane_id(at), 0) and int(p.last["commit"][0]["pending_packed"]) == 1
    return p


LANE_PIPELINES = [pytest.param(lambda be, f=f, at=at: f(be, at), id=f"{f.__name__[:-9]}_{at}")
                  for f in (parents_pipeline, stop_packet_pipeline) for at in (63, 64)]
LANE_PIPELINES.append(pytest.param(ack_frames_pipeline, id="ack_frames_63_64_129"))


@pytest.mark.parametrize("pipeline", LANE_PIPELINES)
def test_lane_63_and_tile_seam(pipeline):
    pipeline(R.HostBackend())


def one_connection(**kw):
    p = R.Pipeline([R.Config(**kw)])
    for _ in range(3):
        p.enqueue(0, 2000, 0, E.RELIABLE)
    p.tick(1000, 50, 1 << 30, [[]])
    return p


def begin_args(p, n=None):
    n = p.n if n is None else n
    rate = np.zeros(p.n, dtype=fr.RATE_RESULT_DTYPE)
    rate["now_ms"], rate["rtt_ms"] = 2000, 50
    flushes = np.zeros(p.n, dtype=fr.FLUSH_DTYPE)
    flushes["flush_alloc"], flushes["kind"], flushes["window_room"] = 1 << 30, fr.DATA, 64
    return rate, flushes


def test_begin_out_of_place_equals_in_place():
    p = one_connection()
    rate, flushes = begin_args(p)
    ff = np.zeros(2, dtype=np.uint64)
    none = np.zeros(0, dtype=fr.FRAME_INFO_DTYPE)
    a2 = {k: v.copy() for k, v in p.arenas.items()}
    out = fr.resend_begin_host(none, ff, p.queues, p.log, rate, flushes, p.states, p.senders, a2)
    s2, d2 = p.states.copy(), p.senders.copy()
    inp = fr.resend_begin_host(none, ff, p.queues, p.log, rate, flushes, s2, d2, p.arenas, states_out=s2, senders_out=d2)
    assert out["states_out"].tobytes() == s2.tobytes() and out["senders_out"].tobytes() == d2.tobytes()
    assert out["results"].tobytes() == inp["results"].tobytes() and int(out["results"]["n_resent"][0]) == 6
    for k in a2:
        assert a2[k].tobytes() == p.arenas[k].tobytes(), k


def test_pack_agrees_with_begins_rule():
    """ufc_pack_host over begin's staged items packs every one (DONE), and with the refused entry appended stops as
    begin did."""
    for alloc, room, want in ((1 << 30, 2, R.WINDOW_LIMITED), (2000, 64, R.SIZE_LIMITED), (1 << 30, 64, R.DONE)):
        p = R.Pipeline([R.Config(frame_window=64, frame_tail=8, heap_cap=64, window_size=64, max_alloc=1 << 20)])
        for _ in range(5):
            p.enqueue(0, 1448, 0, E.PERSISTENT)
        p.tick(0, 100, 1 << 30, [[]])
        rate, flushes = begin_args(p)
        rate["now_ms"], rate["rtt_ms"] = 100, 100
        flushes["flush_alloc"], flushes["window_room"] = alloc, room
        heap0 = p.region(0, "heap", "heap").copy()
        r = fr.resend_begin_host(np.zeros(0, fr.FRAME_INFO_DTYPE), np.zeros(2, np.uint64), p.queues, p.log, rate, flushes,
                                 p.states.copy(), p.senders.copy(), p.arenas)
        res = r["results"][0]
        assert int(res["stop"]) == want
        n = int(res["n_resent"])
        a = int(p.states[0]["stage_first"])
        staged = p.arenas["stage"][a: a + n].copy()
        first = np.array([0, n], dtype=np.uint64)
        _, fres, _ = fr.pack_host(staged, first, flushes)
        assert (int(fres[0]["stop"]), int(fres[0]["items_packed"])) == (fr.PACK_DONE, n)
        if want != R.DONE:
            top = r["states_out"][0]
            refused = p.region(0, "heap", "heap")[0]   # the entry the loop stopped at stays on top
            assert int(refused["send_count"]) == 1 and int(top["heap_len"]) == 5
            more = np.concatenate([staged, p.models[0].pk[int(refused["sequence_id"])].items[:1]])
            _, fres, _ = fr.pack_host(more, np.array([0, n + 1], dtype=np.uint64), flushes)
            assert (int(fres[0]["stop"]), int(fres[0]["items_packed"])) == \
                ({R.WINDOW_LIMITED: fr.PACK_WINDOW_LIMITED, R.SIZE_LIMITED: fr.PACK_SIZE_LIMITED}[want], n)
        del heap0


def test_acknowledge_after_all_frame_queue_work_equals_interleaved():
    """Two ack frames in one tick: the first frees packet 0, the second acknowledges the frame that carried it.  The
    model handles them interleaved, as handle_ack_frame does; the batched calls run the frame queue first."""
    p = R.Pipeline([R.Config(frame_window=16, frame_tail=8, heap_cap=32)])
    for _ in range(3):
        p.enqueue(0, 1448, 0, E.RELIABLE)
    sent = p.tick(0, 100, 1 << 30, [[]])[0]
    assert len(sent) == 3
    p.tick(50, 100, 1 << 30, [[(0, 1, []), (3, 1, [(0, 0b111, 0)])]])
    p.tick(100, 100, 1 << 30, [[]])
    assert int(p.states[0]["heap_len"]) == 0 and "acked_pop" in p.seen


def test_bad_state_copies_through():
    p = one_connection()
    rate, flushes = begin_args(p)
    ff = np.zeros(2, dtype=np.uint64)
    none = np.zeros(0, dtype=fr.FRAME_INFO_DTYPE)
    for fld, val in (("pkt_cap", 3), ("frag_cap", 8), ("tx_cap", 128), ("heap_len", 10**6), ("heap_first", 10**9),
                     ("stage_first", 10**9), ("tx_head", 10**6)):
        s = p.states.copy()
        s[fld] = val
        arenas = {k: v.copy() for k, v in p.arenas.items()}
        r = fr.resend_begin_host(none, ff, p.queues, p.log, rate, flushes, s, p.senders, arenas)
        assert int(r["results"]["stop"][0]) == R.BAD_STATE, fld
        assert r["states_out"].tobytes() == s.tobytes(), fld
        want = p.senders.copy()
        want["take"] = 0
        assert r["senders_out"].tobytes() == want.tobytes(), fld
        for k in arenas:
            assert arenas[k].tobytes() == p.arenas[k].tobytes(), (fld, k)
    r = fr.resend_begin_host(none, np.array([1, 0], dtype=np.uint64), p.queues, p.log, rate, flushes, p.states, p.senders,
                             {k: v.copy() for k, v in p.arenas.items()})
    assert int(r["results"]["stop"][0]) == R.BAD_STATE


def test_null_and_zero_count_rules():
    L = lib()
    assert L.ufc_resend_begin_host(*([None, 0, None, None, None, 0, None, None, None, None, None, 0] + [None, 0] * 6 +
                                     [None, None, None, 1])) == UFC_OK
    assert L.ufc_resend_place_host(None, None, 0, None, 0, None, None, 0, 1) == UFC_OK
    assert L.ufc_resend_commit_host(*([None, None, 0, None, None, None, 0, None, None, 0] + [None] * 7 + [0] +
                                      [None, 0] * 5 + [None] * 5 + [1])) == UFC_OK
    p = one_connection()
    rate, flushes = begin_args(p)
    ff = np.zeros(2, dtype=np.uint64)
    res = np.zeros(1, dtype=fr.RESEND_RESULT_DTYPE)
    A = p.arenas

    def begin(**null):
        def g(name, v):
            return None if name in null else v.ctypes.data
        return L.ufc_resend_begin_host(None, 0, g("frame_first", ff), g("queues", p.queues), p.log.ctypes.data, p.log.size,
                                       g("rate", rate), None, g("flushes", flushes), g("states", p.states),
                                       g("senders", p.senders), 1, g("heap", A["heap"]), A["heap"].size,
                                       A["pkts"].ctypes.data, A["pkts"].size, A["frag_acked"].ctypes.data,
                                       A["frag_acked"].size, A["tx"].ctypes.data, A["tx"].size, None, 0,
                                       A["stage"].ctypes.data, A["stage"].size, g("results", res),
                                       g("states_out", p.states), g("senders_out", p.senders), 1)

    for name in ("frame_first", "queues", "rate", "flushes", "states", "senders", "heap", "results", "states_out", "senders_out"):
        assert begin(**{name: 1}) == UFC_ERR_INVALID_ARG, name
    assert begin() == UFC_OK   # flags and ref_acked are nullable
    assert L.ufc_resend_place_host(p.states.ctypes.data, None, 1, None, 0, ff.ctypes.data, None, 0, 1) == UFC_ERR_INVALID_ARG


def check_argument_table(call, ok, required, counted, counts, nullable):
    """`ok` is accepted; NULL in place of a required pointer, NULL for an array whose count is not zero and a count of
    2^31 - 1 are UFC_ERR_INVALID_ARG; NULL for a nullable argument is accepted."""
    assert call(*ok) == UFC_OK
    for k in required + counted + counts:
        bad = list(ok)
        bad[k] = (1 << 31) - 1 if k in counts else None
        assert call(*bad) == UFC_ERR_INVALID_ARG, k
    for k in nullable:
        fine = list(ok)
        fine[k] = None
        assert call(*fine) == UFC_OK, k


def test_place_and_commit_argument_rules():
    """Every pointer and every limited count of ufc_resend_place_host and ufc_resend_commit_host, over one connection
    that begin refused (UFC_RS_BAD_STATE: place leaves it alone, commit copies it through), so that one record per
    array is enough."""
    def rec(dtype, n=1):
        return np.zeros(n, dtype=dtype)
    states, begin = rec(fr.RESEND_DTYPE), rec(fr.RESEND_RESULT_DTYPE)
    begin["stop"] = fr.RS_BAD_STATE
    stage, items, first = rec(fr.ITEM_DTYPE), rec(fr.ITEM_DTYPE), rec(np.uint64, 2)
    p = lambda a: a.ctypes.data   # noqa: E731
    check_argument_table(lib().ufc_resend_place_host,
                         [p(states), p(begin), 1, p(stage), 1, p(first), p(items), 1, 1],
                         required=(0, 1, 5), counted=(3, 6), counts=(2,), nullable=())
    keep = [rec(d) for d in (fr.FLUSH_RESULT_DTYPE, fr.FRAME_INFO_DTYPE, fr.PACKET_DTYPE, fr.PACKET_RESULT_DTYPE,
                             fr.SENDER_RESULT_DTYPE, fr.RATE_RESULT_DTYPE, fr.SENDER_DTYPE, fr.RESEND_ENTRY_DTYPE,
                             fr.SENT_PACKET_DTYPE, np.uint8, fr.TX_REF_DTYPE, fr.SENT_FRAME_DTYPE, np.uint32,
                             fr.RESEND_COMMIT_RESULT_DTYPE, fr.RESEND_DTYPE, fr.SENDER_DTYPE)]
    (flush_results, infos, packets, packet_results, sender_results, rate, senders, heap, pkts, frag, tx, sent, extra,
     results, states_out, retake) = keep
    offsets, used, sent_first = rec(np.uint64, 2), rec(np.uint64), rec(np.uint64, 2)
    ok = [p(flush_results), p(infos), 1, p(offsets), p(used), p(items), 1, p(first), p(packets), 1, p(first),
          p(packet_results), p(sender_results), p(begin), p(rate), p(states), p(senders), 1, p(heap), 1, p(pkts), 1,
          p(frag), 1, p(tx), 1, p(sent), 1, p(sent_first), p(extra), p(results), p(states_out), p(retake), 1]
    check_argument_table(lib().ufc_resend_commit_host, ok,
                         required=(0, 3, 4, 7, 10, 12, 13, 14, 15, 16, 28, 30, 31, 32),
                         counted=(1, 5, 8, 11, 18, 20, 22, 24, 26), counts=(2, 6, 9, 17), nullable=(29,))


def test_core_under_sanitizers():
    """tests/c/resend_host_check.hip: the wave-policy core (rs_begin, rs_place, rs_commit) as host code under
    AddressSanitizer and UBSan, the lanes of a phase forwards, backwards and shuffled, over exact-size buffers, with the heap
    held against a plain sorted-order oracle; a stand-alone program (nothing is loaded into Python under a
    sanitizer)."""
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(HERE, "c", "resend_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "resend_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
