"""GPU: the batched sender frame queue (ufc_frame_queue_varlen, FrameCrcEngine.frame_queue) against
tests/queue_expect.py and against the host call, byte for byte on results (loss_rate as its 64 bits), states, the
log and ref_acked: the goldens, scenarios and generators of tests/test_queue_cpu.py with the device call in the host
call's place, at the smallest shapes that can go wrong; two streams; queues_out = queues; the C ABI's NULL rules;
and the whole path on the device, emit -> pack -> push -> build -> (frames lost) -> gate -> parse -> the peer's
frame_window -> pack and build of its ack frames -> gate -> parse -> frame_queue -> the next pack."""
import ctypes

import numpy as np
import pytest
import torch

from uflow_amd import frame as fr
from uflow_amd.batch import records, rows
from uflow_amd.frame import FLUSH_DTYPE, PACKET_DTYPE, SENDER_DTYPE

import queue_expect as E
import test_queue_cpu as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8 = np.uint8
KEYS = ("results", "queues_out", "log", "ref_acked")


def _args(call, queues, log, ref_acked):
    return (rows(call["infos"], DEV), rows(call["items"], DEV), rows(call["frame_first"], DEV), rows(call["sent"], DEV), rows(call["sent_first"], DEV),
            rows(queues, DEV), rows(call["steps"], DEV), rows(log, DEV), rows(ref_acked, DEV) if ref_acked is not None else None)


def _host_out(d):
    return {"results": records(d["results"], fr.FRAME_QUEUE_RESULT_DTYPE),
            "queues_out": records(d["queues_out"], fr.FRAME_QUEUE_DTYPE),
            "log": records(d["log"], fr.SENT_FRAME_DTYPE),
            "ref_acked": d["ref_acked"].cpu().numpy() if d["ref_acked"] is not None else None}


def gpu_call(engine, stream=None):
    """test_queue_cpu.host's calling convention on the device form."""
    def call(infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked, nthreads, in_place):
        a = _args({"infos": infos, "items": items, "frame_first": frame_first, "sent": sent, "sent_first": sent_first,
                   "steps": steps}, queues, log, ref_acked)
        d = engine.frame_queue(*a, queues_out=a[5] if in_place else None, stream=stream)
        (stream.synchronize if stream is not None else torch.cuda.synchronize)()
        return _host_out(d)
    return call


@pytest.mark.parametrize("case", T.QUEUE_CASES, ids=[c["name"].split(" (")[0].split(":")[0] for c in T.QUEUE_CASES])
def test_golden_queue_cases(engine, monkeypatch, case):
    """Among them max_loss: a nack run of 8,189 ids across 128 tiles."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    T.run_queue_case(case)


def test_golden_reorder_cases(engine, monkeypatch):
    monkeypatch.setattr(T, "host", gpu_call(engine))
    for case in T.GOLDEN["reorder_cases"]:
        T.run_reorder_case(case)


@pytest.mark.parametrize("n", [1, 3])
def test_generated_traffic(engine, monkeypatch, n):
    """window 4 / tail 4 / log_cap 8 with ids through 2^32 (the ring wraps within a tile), and window 4096."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    t = T.chain(n, 4, 4, 0xFFFFFFFA, seed=3 + n, rounds=8, log_cap=8, sends=6)
    assert t["log_culled"] > 8 and t["frames_acked"] > 0   # (culled past log_cap: the ring has wrapped)
    t = T.chain(n, 4096, 4096, 0xFFFFF000, seed=5 + n, rounds=3, sends=150, loss=0.3)
    assert t["li_nacks"] > 20


def test_in_place_non_monotone_and_hostile(engine, monkeypatch):
    """queues_out = queues; send times all over (the nack tiles entry by entry); every kind of hostile group."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    t = T.chain(4, 256, 256, 100, seed=5, rounds=5, monotone=False, loss=0.4, in_place=True)
    assert t["li_nacks"] > 100
    T.check_generator(T.chain(40, 64, 64, 0xFFFFFFF0, seed=9, rounds=3, hostile=0.5))


def test_frames_of_0_and_161_groups(engine, monkeypatch):
    """An ack frame with no groups (it still advances the window) and one with 161, the most a frame holds: more
    than a tile of groups, each acknowledging one frame out of order."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    q, log = fr.new_frame_queues(1, 256, 256, 0xFFFFFF80)
    base = 0xFFFFFF80
    got, _ = T.run(T.one_call(q[0], [E.sent_frame(100 + k, 10 * k, k & 1, k, 1) for k in range(200)]), q, log)
    q, log = got["queues_out"][:1].copy(), got["log"]
    order = np.random.default_rng(4).permutation(161)
    groups = [[(base + int(k)) & E.M32, 1, int(k) & 1] for k in order]
    refs = np.zeros(200, dtype=U8)
    got, _ = T.run(T.one_call(q[0], acks=[((base + 3) & E.M32, []), ((base + 161) & E.M32, groups)], flags=fr.FQ_FEEDBACK,
                              rtt_ms=20, now_ms=5000), q, log, refs)
    r = got["results"][0]
    assert int(r["ack_frames"]) == 2 and int(r["groups"]) == 161 and int(r["frames_acked"]) == 161
    assert int(r["window_advanced"]) == 161 and int(r["has_feedback"]) == 1
    assert got["ref_acked"][:161].all() and not got["ref_acked"][161:].any()


@pytest.mark.parametrize("scenario", T.LANE_SCENARIOS, ids=lambda f: f.__name__[9:])
def test_lane_scenarios(engine, monkeypatch, scenario):
    """The step's ballots with their deciding lane on lane 0, on lane 63 and across a tile seam."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    scenario()


@pytest.mark.parametrize("rule", ["ring outside the arena", "held frames out of order", "ack frame's items outside",
                                  "reset with no interval", "log starts more than tail behind the window"])
def test_state_check(engine, monkeypatch, rule):
    monkeypatch.setattr(T, "host", gpu_call(engine))
    T.test_state_check(rule)


def test_float_edges_and_random_states(engine, monkeypatch):
    monkeypatch.setattr(T, "host", gpu_call(engine))
    T.test_receive_rate_edges()
    T.test_loss_rate_edges()
    for p, length in ((0.0, E.M32), (-1.0, 0), (float("nan"), 0), (1e-12, E.M32), (0.4, 3)):
        T.test_reset_loss_rate_edges(p, length)
    T.scenario_random_states(range(60))


def many_connections(n=70000):
    """More connections than the launch grid: two frames pushed each, then one ack frame each."""
    rng = np.random.default_rng(51)
    q, log = fr.new_frame_queues(n, 2, 2, 0)
    base = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for k in ("log_base_id", "log_next_id", "window_base_id", "rb_base_id"):
        q[k] = base
    sent = np.zeros(2 * n, dtype=fr.SENT_FRAME_DTYPE)
    sent["send_time_ms"] = np.arange(2 * n) // 2
    sent["size"], sent["ref_first"], sent["ref_count"] = 100, np.arange(2 * n), 1
    sent["flags"] = rng.integers(0, 2, 2 * n)
    steps = np.zeros(n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
    none = np.zeros(n + 1, dtype=np.uint64)
    push = {"infos": np.zeros(0, fr.FRAME_INFO_DTYPE), "items": np.zeros(0, fr.ITEM_DTYPE), "frame_first": none, "sent": sent,
            "sent_first": np.arange(0, 2 * n + 1, 2, dtype=np.uint64), "steps": steps}
    which = rng.integers(0, 3, n)     # the group acks the first frame, the second, or both
    items = np.zeros(n, dtype=fr.ITEM_DTYPE)
    items["form"] = 3
    items["id"] = base + (which == 1)
    items["data_offset"] = np.where(which == 2, 3, 1)
    n0, n1 = sent["flags"][0::2] & 1, sent["flags"][1::2] & 1
    items["channel_id"] = np.where(which == 0, n0, np.where(which == 1, n1, n0 ^ n1))
    infos = np.zeros(n, dtype=fr.FRAME_INFO_DTYPE)
    infos["kind"], infos["ok"], infos["item_count"], infos["item_first"] = fr.ACK, 1, 1, np.arange(n)
    infos["f"][:, 0] = base + 2
    steps2 = steps.copy()
    steps2["flags"], steps2["now_ms"] = fr.FQ_FEEDBACK, 2 * n
    ack = {"infos": infos, "items": items, "frame_first": np.arange(n + 1, dtype=np.uint64), "sent": sent[:0], "sent_first": none,
           "steps": steps2}
    return q, log, push, ack, which


def test_70000_connections_equal_the_host_call(engine):
    """Device == host on every byte, past the launch grid of 65,536."""
    q, log, push, ack, which = many_connections()
    refs = np.zeros(len(push["sent"]), dtype=U8)
    for call in (push, ack):
        h = fr.frame_queue_host(call["infos"], call["items"], call["frame_first"], call["sent"], call["sent_first"], q,
                                call["steps"], log.copy(), ref_acked=refs.copy(), nthreads=8)
        d = engine.frame_queue(*_args(call, q, log, refs))
        torch.cuda.synchronize()
        o = _host_out(d)
        for k in KEYS:
            assert o[k].tobytes() == h[k].tobytes(), k
        q, log, refs = o["queues_out"], o["log"], o["ref_acked"]
    assert np.array_equal(refs[0::2], (which != 1).astype(U8)) and np.array_equal(refs[1::2], (which != 0).astype(U8))
    assert (o["results"]["has_feedback"] == 1).all() and (o["results"]["window_room"] == 2).all()


def test_equals_the_host_call(engine):
    """Chained generated calls through ufc_frame_queue_host and the device call: every output byte for byte."""
    rng = np.random.default_rng(61)
    q, log, calls = E.make_batch(rng, 30, 128, 128, 0xFFFFFF00, rounds=4, hostile=0.3, loss=0.2)
    refs = np.zeros(calls[-1]["refs"] + 5, dtype=U8)
    acked = 0
    for call in calls:
        h = fr.frame_queue_host(call["infos"], call["items"], call["frame_first"], call["sent"], call["sent_first"], q,
                                call["steps"], log.copy(), ref_acked=refs.copy(), nthreads=4)
        d = engine.frame_queue(*_args(call, q, log, refs))
        torch.cuda.synchronize()
        o = _host_out(d)
        for k in KEYS:
            assert o[k].tobytes() == h[k].tobytes(), k
        acked += int(o["results"]["frames_acked"].sum())
        q, log, refs = o["queues_out"], o["log"], o["ref_acked"]
    assert acked > 500


def test_two_streams_two_batches(engine):
    """Two different batches in flight on two streams, three times over: the call keeps nothing between calls."""
    rng = np.random.default_rng(71)
    batches = []
    for n, w in ((40, 64), (7, 512)):
        q, log, calls = E.make_batch(rng, n, w, w, 9, rounds=2, hostile=0.2)
        out = E.expect_batch(calls[0]["infos"], calls[0]["items"], calls[0]["frame_first"], calls[0]["sent"],
                             calls[0]["sent_first"], q, calls[0]["steps"], log)
        refs = np.zeros(calls[1]["refs"] + 1, dtype=U8)
        c = calls[1]
        want = E.expect_batch(c["infos"], c["items"], c["frame_first"], c["sent"], c["sent_first"], out["queues_out"],
                              c["steps"], out["log"], refs)
        batches.append((c, out["queues_out"], out["log"], refs, want))
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    args = [[_args(c, q, log, refs) for (c, q, log, refs, _) in batches] for _ in range(3)]   # (the log is marked in place)
    torch.cuda.synchronize()   # (the uploads are on the default stream, the calls are not)
    outs = []
    for k in range(3):
        for a, s in zip(args[k], (s1, s2)):
            outs.append(engine.frame_queue(*a, stream=s))
    s1.synchronize()
    s2.synchronize()
    for k, d in enumerate(outs):
        want = batches[k % 2][4]
        o = _host_out(d)
        for key in KEYS:
            assert o[key].tobytes() == want[key].tobytes(), (k, key)
    engine.release_stream(s1)
    engine.release_stream(s2)


def test_argument_checks(engine):
    q, log = fr.new_frame_queues(1, 8, 8, 0)
    c = T.one_call(q[0], [E.sent_frame(9, 1, 1, 0, 1)], [(None, [[0, 1, 1]])])
    a = _args(c, q, log, np.zeros(4, U8))
    with pytest.raises(ValueError):
        engine.frame_queue(a[0], a[1], a[2][:1], *a[3:])
    with pytest.raises(ValueError):
        engine.frame_queue(*a[:5], a[5][:, :100].contiguous(), *a[6:])
    with pytest.raises(ValueError):
        engine.frame_queue(*a, queues_out=torch.zeros(10, dtype=torch.uint8, device=DEV))
    V = ctypes.c_void_p
    st = V(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    ok = [V(a[0].data_ptr()), 1, V(a[1].data_ptr()), 1, V(a[2].data_ptr()), V(a[3].data_ptr()), 1, V(a[4].data_ptr()),
          V(a[5].data_ptr()), V(a[6].data_ptr()), 1, V(a[7].data_ptr()), len(log), V(a[8].data_ptr()), 4, V(p), V(p + 256), st]
    call = fr.lib().ufc_frame_queue_varlen
    assert call(engine._ctx, *ok) == 0
    for k in (0, 2, 4, 5, 7, 8, 9, 11, 15, 16):
        bad = list(ok)
        bad[k] = None
        assert call(engine._ctx, *bad) == T.UFC_ERR_INVALID_ARG, k
    for k in (1, 3, 6, 10):
        bad = list(ok)
        bad[k] = (1 << 31) - 1
        assert call(engine._ctx, *bad) == T.UFC_ERR_INVALID_ARG, k
    assert call(None, *ok) == T.UFC_ERR_INVALID_ARG
    assert call(engine._ctx, None, 0, None, 0, None, None, 0, None, None, None, 0, None, 0, None, 0, None, None, st) == 0
    torch.cuda.synchronize()
    res = buf[:80].cpu().numpy().view(fr.FRAME_QUEUE_RESULT_DTYPE)[0]
    assert int(res["stop"]) == fr.FQ_DONE and int(res["frames_acked"]) == 1 and int(res["pushes_taken"]) == 1
    assert a[8].cpu().numpy().tolist() == [1, 0, 0, 0]
    d = engine.frame_queue(a[0][:0], a[1][:0], rows(np.zeros(1, np.uint64), DEV), a[3][:0], rows(np.zeros(1, np.uint64), DEV), a[5][:0],
                           a[6][:0], a[7])   # no connections: UFC_OK
    assert d["results"].shape[0] == 0


def test_whole_path_on_the_device(engine):
    """emit -> pack (window_room and id0 from the frame queues) -> build -> seal -> push into the queues; frames 3, 8
    and 13 of each connection's 16 are lost (the first two are nacked once three later frames are acked, the third
    stays open behind the two held ones); the peer's gate -> parse -> frame_window gives groups, packed and built into ack frames; back
    here gate -> parse -> frame_queue: ref_acked marks exactly the items of the frames that arrived, and the window
    room that comes out goes into the next pack.  Every stage is compared with its host call."""
    rng = np.random.default_rng(83)
    n, per, FRAG = 3, 60, fr.MAX_FRAME_SIZE - 24
    same = lambda dev, host, dt, what: T.same(dev.cpu().numpy().view(dt).reshape(-1)[:len(host)], host, what)
    packets = np.zeros(n * per, dtype=PACKET_DTYPE)
    sizes = rng.choice([0, 3, 60, 700, FRAG, FRAG + 1], size=packets.size)
    packets["data_len"] = sizes
    packets["data_offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packets["channel_id"] = rng.integers(0, 3, packets.size)
    packets["mode"] = fr.SEND_UNRELIABLE
    payload = rng.integers(0, 256, int(sizes.sum()), dtype=U8)
    senders = np.zeros(n, dtype=SENDER_DTYPE)
    senders["base_id"] = senders["next_id"] = rng.integers(0, 1 << 20, n)
    senders["window_size"], senders["max_alloc"], senders["take"] = 64, 1 << 30, per
    senders["window_parent_id"] = fr.NO_PARENT
    senders["channel_parent_id"] = fr.NO_PARENT
    pf = np.arange(n + 1) * per
    # 1. emit
    cap = int(np.maximum(1, (sizes + FRAG - 1) // FRAG).sum())
    items, iff, _, _, _, _ = engine.emit_packets(rows(packets, DEV), rows(pf, DEV), rows(senders, DEV), items_cap=cap)
    h_items, h_iff, _, _, _, h_used = fr.emit_packets_host(packets, pf.astype(np.uint64), senders)
    same(items, h_items[:h_used], fr.ITEM_DTYPE, "emit: items")
    # 2. pack, with the room and the first id the frame queues give
    first_ids = np.array([0xFFFFFFF8, 5, 0x12345678], dtype=np.uint64)   # (the first connection's ids wrap)
    queues, log = fr.new_frame_queues(n, 16, 16, first_ids.astype(np.uint32))
    flushes = np.zeros(n, dtype=FLUSH_DTYPE)
    flushes["kind"], flushes["flush_alloc"] = fr.DATA, 1 << 40
    flushes["window_room"], flushes["id0"] = queues["window_size"], queues["log_next_id"]
    nonce_words = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    infos, res, frames_used = engine.pack_flushes(items, iff, rows(flushes, DEV), nonce_bits=rows(nonce_words.view(np.int32), DEV))
    h_infos, h_res, nfr = fr.pack_host(h_items[:h_used], h_iff, flushes, nonce_bits=nonce_words)
    same(infos, h_infos[:nfr], fr.FRAME_INFO_DTYPE, "pack: infos")
    same(res, h_res, fr.FLUSH_RESULT_DTYPE, "pack: results")
    assert (h_res["frame_count"] == 16).all() and (h_res["stop"] == fr.PACK_WINDOW_LIMITED).all()
    # 3. build and seal; push the packed frames into the queues
    wire, off, _ = engine.build_varlen(infos, items, rows(payload, DEV), seal=True)
    h_wire, h_off, _, _ = fr.build_batch_host(h_infos[:nfr], h_items[:h_used], payload)
    torch.cuda.synchronize()
    wire_h, off_h = wire.cpu().numpy(), off.cpu().numpy()[:nfr + 1].astype(np.int64)
    assert np.array_equal(off_h, h_off.astype(np.int64)) and wire_h[:off_h[-1]].tobytes() == h_wire.tobytes()
    sent = np.zeros(nfr, dtype=fr.SENT_FRAME_DTYPE)
    sent["send_time_ms"] = 100 + np.arange(nfr)
    sent["size"] = off_h[1:] - off_h[:-1]
    sent["ref_first"], sent["ref_count"] = h_infos["item_first"][:nfr], h_infos["item_count"][:nfr]
    sent["flags"] = [(int(nonce_words[g // 32]) >> (g % 32)) & 1 for g in range(nfr)]
    sf = np.concatenate([h_res["frame_first"], [nfr]]).astype(np.uint64)
    steps = np.zeros(n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
    push = {"infos": np.zeros(0, fr.FRAME_INFO_DTYPE), "items": np.zeros(0, fr.ITEM_DTYPE),
            "frame_first": np.zeros(n + 1, np.uint64), "sent": sent, "sent_first": sf, "steps": steps}
    refs = np.zeros(h_used, dtype=U8)
    d_log, d_refs = rows(log, DEV), rows(refs, DEV)
    a = _args(push, queues, log, None)
    fq1 = engine.frame_queue(*a[:7], d_log, d_refs)
    h1 = fr.frame_queue_host(push["infos"], push["items"], push["frame_first"], sent, sf, queues, steps, log, ref_acked=refs)
    torch.cuda.synchronize()
    o1 = _host_out(fq1)
    for k in KEYS:
        assert o1[k].tobytes() == h1[k].tobytes(), k
    assert (o1["results"]["pushes_taken"] == 16).all() and (o1["results"]["window_room"] == 0).all()
    # 4. the wire loses every fifth frame; the peer's gate, parse and frame window
    arrive = [g for g in range(nfr) if (g - int(sf[np.searchsorted(sf, g, side="right") - 1])) % 5 != 3]
    owner = [int(np.searchsorted(sf, g, side="right") - 1) for g in arrive]
    off2 = np.concatenate([[0], np.cumsum([off_h[g + 1] - off_h[g] for g in arrive])]).astype(np.int64)
    wire2 = np.concatenate([wire_h[off_h[g]:off_h[g + 1]] for g in arrive])
    frame_first = np.searchsorted(np.array(owner), np.arange(n + 1)).astype(np.int64)
    d_wire, d_off = rows(wire2, DEV), rows(off2, DEV)
    _, valid = engine.crc_varlen(d_wire, d_off)
    infos2, items2, _ = engine.parse_varlen(d_wire, d_off, valid)
    hp_infos, hp_items = fr.parse_batch_host(wire2, off2.astype(np.uint64))
    same(infos2, hp_infos, fr.FRAME_INFO_DTYPE, "parse: infos")
    windows = fr.new_frame_windows(n, 4096, first_ids.astype(np.uint32))
    fw = engine.frame_window(infos2, rows(frame_first, DEV), rows(windows, DEV))
    hw = fr.frame_window_host(hp_infos, frame_first.astype(np.uint64), windows)
    torch.cuda.synchronize()
    used = int(fw["groups_used"].cpu()[0])
    assert used == hw["groups_used"]
    same(fw["groups"], hw["groups"][:used], fr.ITEM_DTYPE, "frame_window: groups")
    same(fw["windows_out"], hw["windows_out"], fr.FRAME_WINDOW_DTYPE, "frame_window: state")
    # 5. its ack frames, packed, built and sealed
    ack = np.zeros(n, dtype=FLUSH_DTYPE)
    ack["kind"], ack["flush_alloc"] = fr.ACK, 1 << 40
    ack["id0"], ack["id1"] = hw["windows_out"]["base_id"], 77
    groups = fw["groups"][:used].contiguous()
    a_infos, a_res, a_used = engine.pack_flushes(groups, fw["group_first"], rows(ack, DEV))
    ha_infos, ha_res, na = fr.pack_host(hw["groups"][:used], hw["group_first"], ack)
    same(a_infos, ha_infos[:na], fr.FRAME_INFO_DTYPE, "ack pack: infos")
    assert na == n
    a_wire, a_off, _ = engine.build_varlen(a_infos, groups, torch.zeros(0, dtype=torch.uint8, device=DEV), seal=True)
    ha_wire, ha_off, _, _ = fr.build_batch_host(ha_infos[:na], hw["groups"][:used], np.zeros(0, U8))
    torch.cuda.synchronize()
    a_off = a_off[:na + 1].contiguous()
    assert a_wire.cpu().numpy()[:int(ha_off[-1])].tobytes() == ha_wire.tobytes()
    # 6. back at the sender: gate and parse
    _, a_valid = engine.crc_varlen(a_wire, a_off)
    p_infos, p_items, p_used = engine.parse_varlen(a_wire, a_off, a_valid)
    hq_infos, hq_items = fr.parse_batch_host(ha_wire, ha_off)
    same(p_infos, hq_infos, fr.FRAME_INFO_DTYPE, "ack parse: infos")
    same(p_items, hq_items, fr.ITEM_DTYPE, "ack parse: items")
    assert a_valid.cpu().numpy().all() and (hq_infos["kind"] == fr.ACK).all()
    # 7. the frame queue: acked fragments, the window, feedback
    steps2 = steps.copy()
    steps2["flags"], steps2["rtt_ms"], steps2["now_ms"] = fr.FQ_FEEDBACK | fr.FQ_HAS_RTT, 30, 500
    af = np.arange(n + 1, dtype=np.uint64)
    none = np.zeros(n + 1, dtype=np.uint64)
    fq2 = engine.frame_queue(p_infos, p_items[:len(hq_items)].contiguous(), rows(af, DEV), rows(sent[:0], DEV), rows(none, DEV), fq1["queues_out"],
                             rows(steps2, DEV), d_log, d_refs, queues_out=fq1["queues_out"])
    h2 = fr.frame_queue_host(hq_infos, hq_items, af, sent[:0], none, h1["queues_out"], steps2, h1["log"],
                             ref_acked=h1["ref_acked"])
    torch.cuda.synchronize()
    o2 = _host_out(fq2)
    for k in KEYS:
        assert o2[k].tobytes() == h2[k].tobytes(), k
    want = np.zeros(h_used, dtype=U8)
    for g in arrive:
        want[int(h_infos["item_first"][g]):int(h_infos["item_first"][g]) + int(h_infos["item_count"][g])] = 1
    assert np.array_equal(o2["ref_acked"], want) and want.any()
    lost = [g for g in range(nfr) if g not in arrive]
    assert len(lost) == 3 * n and all(h_infos["item_count"][g] > 0 and not want[int(h_infos["item_first"][g])] for g in lost)
    r = o2["results"]
    assert (r["has_feedback"] == 1).all() and (r["frames_acked"] == 13).all() and (r["li_nacks"] == 2).all()
    assert (r["window_advanced"] == 16).all() and (r["window_room"] == 16).all()
    assert (r["loss_rate"] > 0).all() and (r["groups_bad_nonce"] == 0).all() and (r["groups_unknown"] == 0).all()
    # the room and the next id go back into the next pack
    flushes["window_room"], flushes["id0"] = r["window_room"], o2["queues_out"]["log_next_id"]
    infos3, res3, used3 = engine.pack_flushes(items, iff, rows(flushes, DEV))
    h_infos3, h_res3, nfr3 = fr.pack_host(h_items[:h_used], h_iff, flushes)
    same(infos3, h_infos3[:nfr3], fr.FRAME_INFO_DTYPE, "next pack: infos")
    assert (h_res3["frame_count"] == 16).all()
    assert [int(h_infos3["f"][int(h_res3["frame_first"][s]), 0]) for s in range(n)] == \
        [(int(first_ids[s]) + 16) & E.M32 for s in range(n)]
