"""GPU: the batched resend calls (ufc_resend_begin_varlen / ufc_resend_place_varlen / ufc_resend_commit_varlen,
FrameCrcEngine.resend_begin / resend_place / resend_commit) with the device calls in the host calls' place: the
hand-traced goldens and the generated lossy traffic of tests/test_resend_cpu.py, every tick compared with
tests/resend_expect.py's model byte for byte (results, states, the heap, the packet table, the ack bytes, the tx ring,
staged and placed items, sent records), at the smallest shapes that can go wrong; two streams; a BAD_STATE
connection between good ones against the host call.  Every other call of the tick (frame_queue, emit_packets,
pack_flushes, build_sizes) is the device form too."""
import json
import os
import random

import numpy as np
import pytest
import torch

from uflow_amd import frame as fr

import emit_expect as E
import resend_expect as R
import test_resend_cpu as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8 = np.uint8
WIDTH = {"heap": 16, "pkts": 24, "frag_acked": None, "tx": 8, "ref_acked": None, "stage": 24}


def _t(a, width=None):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint64, np.uint32):
        a = a.view(np.int64 if a.dtype == np.uint64 else np.int32)
    return torch.from_numpy(a.view(U8).reshape(-1, width) if width else a.copy()).to(DEV)


def _back(t, arr):
    """The device tensor's bytes into the host array it was made from."""
    arr.view(U8).reshape(-1)[:] = t.cpu().numpy().view(U8).reshape(-1)


def _np(t, dtype):
    return t.cpu().numpy().view(U8).reshape(-1).view(dtype).copy()


class GpuBackend:
    """resend_expect.HostBackend's methods on the device forms: arrays go up, the call is queued, arrays come back."""

    def __init__(self, engine, stream=None):
        self.e, self.stream = engine, stream

    def sync(self):
        (self.stream.synchronize if self.stream is not None else torch.cuda.synchronize)()

    def ctx(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else torch.cuda.stream(torch.cuda.current_stream())

    def up_arenas(self, arenas):
        return {k: _t(v, WIDTH[k]) for k, v in arenas.items()}

    def down_arenas(self, d, arenas):
        for k in arenas:
            _back(d[k], arenas[k])

    def frame_queue(self, infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked):
        with self.ctx():
            q, lg, ra = _t(queues, 192), _t(log, 24), _t(ref_acked)
            d = self.e.frame_queue(_t(infos, 32), _t(items, 24), _t(frame_first), _t(sent, 24), _t(sent_first), q,
                                   _t(steps, 40), lg, ra, queues_out=q, stream=self.stream)
            self.sync()
        _back(q, queues), _back(lg, log), _back(ra, ref_acked)
        return _np(d["results"], fr.FRAME_QUEUE_RESULT_DTYPE)

    def resend_begin(self, infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags):
        with self.ctx():
            A, s, sd = self.up_arenas(arenas), _t(states, 104), _t(senders, 304)
            d = self.e.resend_begin(_t(infos, 32), _t(frame_first), _t(queues, 192), _t(log, 24), _t(rate, 56),
                                    _t(flushes, 24), s, sd, A, flags=_t(flags), states_out=s, senders_out=sd,
                                    stream=self.stream)
            self.sync()
        self.down_arenas(A, arenas)
        _back(s, states), _back(sd, senders)
        return _np(d["results"], fr.RESEND_RESULT_DTYPE)

    def emit(self, packets, packet_first, senders, items):
        with self.ctx():
            it = _t(items, 24)
            out = self.e.emit_packets(_t(packets, 16), _t(packet_first), _t(senders, 304), items.size, items=it,
                                      stream=self.stream)
            self.sync()
        _back(it, items)
        return (items, _np(out[1], np.uint64), _np(out[2], fr.PACKET_RESULT_DTYPE), _np(out[3], fr.SENDER_RESULT_DTYPE),
                _np(out[4], fr.SENDER_DTYPE), int(out[5].item()))

    def emit_state(self, packets, packet_first, senders):
        with self.ctx():
            out = self.e.emit_packets(_t(packets, 16), _t(packet_first), _t(senders, 304), 0, stream=self.stream)
            self.sync()
        return _np(out[3], fr.SENDER_RESULT_DTYPE), _np(out[4], fr.SENDER_DTYPE)

    def resend_place(self, states, begin_results, arenas, flush_first, items):
        with self.ctx():
            it = _t(items, 24)
            self.e.resend_place(_t(states, 104), _t(begin_results, 48), {"stage": _t(arenas["stage"], 24)}, _t(flush_first),
                                it, stream=self.stream)
            self.sync()
        _back(it, items)

    def pack(self, items, flush_first, flushes):
        with self.ctx():
            infos, results, used = self.e.pack_flushes(_t(items, 24), _t(flush_first), _t(flushes, 24), stream=self.stream)
            self.sync()
        return _np(infos, fr.FRAME_INFO_DTYPE), _np(results, fr.FLUSH_RESULT_DTYPE), int(used.item())

    def build_sizes(self, infos, items):
        if infos.size == 0:
            return np.zeros(1, dtype=np.uint64)
        with self.ctx():
            offsets, _ = self.e.build_sizes_varlen(_t(infos, 32), _t(items, 24), 1 << 40, stream=self.stream)
            self.sync()
        return _np(offsets, np.uint64)

    def resend_commit(self, flush_results, infos, out_offsets, frames_used, items, flush_first, packets, packet_first,
                      packet_results, sender_results, begin_results, rate, states, senders, arenas, next_extra_flags=None,
                      states_out=None):
        with self.ctx():
            A = self.up_arenas({k: v for k, v in arenas.items() if k not in ("ref_acked", "stage")})
            s, extra = _t(states, 104), _t(next_extra_flags)
            d = self.e.resend_commit(_t(flush_results, 24), _t(infos, 32), _t(out_offsets),
                                     torch.tensor([frames_used], dtype=torch.int64, device=DEV), _t(items, 24),
                                     _t(flush_first), _t(packets, 16), _t(packet_first), _t(packet_results, 16),
                                     _t(sender_results, 32), _t(begin_results, 48), _t(rate, 56), s, _t(senders, 304), A,
                                     next_extra_flags=extra, states_out=s, stream=self.stream)
            self.sync()
        for k in A:
            _back(A[k], arenas[k])
        _back(s, states)
        return {"results": _np(d["results"], fr.RESEND_COMMIT_RESULT_DTYPE), "retake": _np(d["retake"], fr.SENDER_DTYPE),
                "sent": _np(d["sent"], fr.SENT_FRAME_DTYPE), "sent_first": _np(d["sent_first"], np.uint64),
                "next_extra_flags": _np(extra, np.uint32)}


@pytest.mark.parametrize("case", T.GOLDEN["cases"], ids=[c["name"] for c in T.GOLDEN["cases"]])
def test_golden(engine, case):
    R.run_golden(case, GpuBackend(engine))


def test_lossy_traffic_small_rings(engine):
    """The CPU file's six connections (a 4-packet window with pkt_cap 4 and ids through 2^20, a heap and a stage that
    fill, a frame window of 2), every tick compared; every stop code but BAD_STATE."""
    p = R.Pipeline(T.lossy_configs(), GpuBackend(engine))
    R.run_lossy(p, random.Random(5), 150, hostile=0.3, hostile_from=125, loss=[0.25, 0.25, 0.25, 0.25, 0.1, 0.6])
    assert {R.DONE, R.SIZE_LIMITED, R.WINDOW_LIMITED, R.REF_HANG, R.STAGE_FULL, R.HEAP_FULL} <= p.seen_stops
    assert {"dead_pop", "acked_pop", "resent", "partial_packet", "frag_wrap", "id_wrap", "hang"} <= p.seen


@pytest.mark.parametrize("n", [1, 3, 65])
def test_connections(engine, n):
    """65 connections: past one launch's first 64 blocks; mixed capacities side by side."""
    base = T.lossy_configs()
    cfgs = [R.Config(**{**base[c % len(base)].__dict__, "base_id": (0xFFFF0 + 37 * c) & E.ID_MASK}) for c in range(n)]
    p = R.Pipeline(cfgs, GpuBackend(engine))
    R.run_lossy(p, random.Random(100 + n), 12 if n == 65 else 40, loss=0.3)
    assert "resent" in p.seen and (n == 1 or "acked_pop" in p.seen)


def test_tx_ring_wraps_within_a_call(engine):
    p = R.Pipeline([R.Config(window_size=64, max_alloc=1 << 20, frame_window=1, frame_tail=0, heap_cap=64)], GpuBackend(engine))
    R.run_lossy(p, random.Random(3), 70, loss=0.0, alloc=(1 << 20, 1 << 21),
                traffic=lambda r, t, c: [(r.randrange(20), 0, E.RELIABLE) for _ in range(r.randrange(7, 12))])
    assert {"tx_wrap", "tx_skip"} <= p.seen


@pytest.mark.parametrize("k", [1, 63, 64, 65, 1000])
def test_heap_sizes(engine, k):
    """k Persistent packets sent at once and all due one RTT later: k pops and pushes through a heap of k entries (63
    fills six levels, 64 and 65 open the seventh), then the acks empty it."""
    p = R.Pipeline([R.Config(window_size=1024, max_alloc=1 << 20, frame_window=64, frame_tail=16, heap_cap=1024)],
                   GpuBackend(engine))
    for _ in range(k):
        p.enqueue(0, 10, 0, E.PERSISTENT)
    sent = p.tick(0, 100, 1 << 30, [[]])[0]
    assert int(p.states[0]["heap_len"]) == k
    again = p.tick(100, 100, 1 << 30, [[]])[0]
    assert sum(len(f) for _, f in again) == k and "resent" in p.seen
    base = int(p.senders[0]["base_id"])
    acks = [(fid + 1, base, [(fid, 1, 0)]) for fid, _ in sent + again]
    p.tick(150, 100, 1 << 30, [acks])
    p.tick(300, 100, 1 << 30, [[]])
    assert int(p.states[0]["heap_len"]) == 0 and "acked_pop" in p.seen


def test_130_fragment_packet_cut_by_the_flush_allocation(engine):
    """One fragment goes, 129 stay pending: staged in three lane passes, then packed, pushed and acknowledged."""
    p = R.Pipeline([R.Config(window_size=8, max_alloc=200000, frame_window=256, frame_tail=16, heap_cap=256, stage_cap=512)],
                   GpuBackend(engine))
    p.enqueue(0, 130 * 1448, 2, E.PERSISTENT)
    p.tick(0, 100, 1000, [[]])
    assert int(p.states[0]["pending_count"]) == 129
    sent = p.tick(10, 100, 1 << 30, [[]])[0]
    assert len(sent) == 129 and int(p.states[0]["heap_len"]) == 130 and int(p.states[0]["pending_count"]) == 0
    p.tick(110, 100, 1 << 30, [[]])
    assert "pending_packed" in p.seen and "resent" in p.seen


def test_acknowledge_frees_0_1_64_65_packets(engine):
    p = R.Pipeline([R.Config(window_size=256, max_alloc=1 << 20, frame_window=64, frame_tail=16, heap_cap=256)],
                   GpuBackend(engine))
    rng = random.Random(9)
    for _ in range(140):
        p.enqueue(0, rng.randrange(30), rng.randrange(5), rng.choice((E.RELIABLE, E.UNRELIABLE, E.PERSISTENT)))
    p.tick(0, 1000, 1 << 30, [[]])
    base = int(p.senders[0]["base_id"])
    now = 10
    for step in (0, 1, 64, 65):
        base = (base + step) & E.ID_MASK
        p.tick(now, 1000, 1 << 30, [[(0, base, [])]])
        assert int(p.senders[0]["base_id"]) == base
        now += 10
    assert E.sub(int(p.senders[0]["next_id"]), base) == 10


def test_two_streams(engine):
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    try:
        a = R.Pipeline(T.lossy_configs()[:3], GpuBackend(engine, s1))
        b = R.Pipeline(T.lossy_configs()[2:5], GpuBackend(engine, s2))
        ra, rb = random.Random(1), random.Random(2)
        for k in range(6):
            R.run_lossy(a, ra, 3, loss=0.3, start_ms=1000 + 75 * k)
            R.run_lossy(b, rb, 3, loss=0.3, start_ms=1000 + 75 * k)
    finally:
        engine.release_stream(s1)
        engine.release_stream(s2)


def test_bad_state_between_good_ones_equals_host(engine):
    """Three connections after some traffic, the middle one's state broken: begin on the device and on the host give
    the same bytes everywhere, the middle one BAD_STATE and untouched."""
    p = R.Pipeline(T.lossy_configs()[:3], GpuBackend(engine))
    R.run_lossy(p, random.Random(4), 20, loss=0.3)
    states = p.states.copy()
    states[1]["pkt_cap"] = 3
    rate = np.zeros(3, dtype=fr.RATE_RESULT_DTYPE)
    rate["now_ms"], rate["rtt_ms"] = 5000, 40
    flushes = np.zeros(3, dtype=fr.FLUSH_DTYPE)
    flushes["flush_alloc"], flushes["kind"], flushes["window_room"] = 1 << 30, fr.DATA, 4
    ff = np.zeros(4, dtype=np.uint64)
    none = np.zeros(0, dtype=fr.FRAME_INFO_DTYPE)
    host_arenas = {k: v.copy() for k, v in p.arenas.items()}
    h = fr.resend_begin_host(none, ff, p.queues, p.log, rate, flushes, states, p.senders, host_arenas)
    dev_arenas = {k: v.copy() for k, v in p.arenas.items()}
    s, sd = states.copy(), p.senders.copy()
    res = GpuBackend(engine).resend_begin(none, ff, p.queues, p.log, rate, flushes, s, sd, dev_arenas, np.zeros(3, np.uint32))
    assert list(res["stop"]) == list(h["results"]["stop"]) and int(res["stop"][1]) == R.BAD_STATE
    assert int(res["n_resent"][0]) + int(res["n_resent"][2]) > 0
    assert res.tobytes() == h["results"].tobytes()
    assert s.tobytes() == h["states_out"].tobytes() and sd.tobytes() == h["senders_out"].tobytes()
    assert s[1].tobytes() == states[1].tobytes()
    for k in host_arenas:
        if k == "stage":   # (slots behind the staged items are not part of the contract)
            for c in (0, 2):
                a, m = int(s[c]["stage_first"]), int(res["n_resent"][c]) + int(res["n_pending_staged"][c])
                assert dev_arenas[k][a: a + m].tobytes() == host_arenas[k][a: a + m].tobytes()
        else:
            assert dev_arenas[k].tobytes() == host_arenas[k].tobytes(), k


def test_end_to_end_on_the_device(engine):
    """Senders and their receiving peers for 90 ticks over a link that drops a fifth of the data frames and a tenth of
    the ack frames, every call of both sides queued on device tensors and nothing read back until the last tick is
    queued: rate_begin -> frame_queue -> rate_step -> resend_begin -> emit -> resend_place -> pack -> sizes ->
    resend_commit -> emit (state) -> build and seal | gate -> parse -> frame_window -> receive_packets -> the ack
    flush's pack -> build and seal | gate -> parse -> (the next tick's frame_queue and resend_begin).  What lies
    between the calls is byte moves on the device (the flushes' window_room and ids, the dropped frames' valid flags,
    the consumed packets marked stale).  flush_alloc is a fixed 4,000 bytes a tick in place of the rate step's value,
    so that the test does not hang on TFRC's ramp; the rate calls run and give now_ms and rtt_ms.  Every Persistent
    and Reliable packet comes out of receive_packets once, per channel in order, with its bytes; the heaps and the
    pending queues end empty."""
    import ctypes
    from uflow_amd._native import lib, check
    rng = np.random.default_rng(77)
    n, per, W, TICKS, QUIET = 3, 14, 16, 90, 25
    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    sizes = rng.choice([0, 5, 200, 1448, 1449, 3000, 6000], size=n * per)
    sizes[per - 1::per] = 3000
    packets = np.zeros(n * per, dtype=fr.PACKET_DTYPE)
    packets["data_len"], packets["data_offset"] = sizes, np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packets["channel_id"] = rng.integers(0, 3, n * per)
    # Reliable packets, and a Persistent one at the end of every queue: the receiver may skip a Persistent packet
    # that is missing once a later packet has arrived (src/lib.rs:314-319, packet_receiver/mod.rs:365-400), so only
    # one with nothing behind it is sure to be delivered.
    packets["mode"] = fr.SEND_RELIABLE
    packets["mode"][per - 1::per] = fr.SEND_PERSISTENT
    payload = rng.integers(0, 256, int(sizes.sum()), dtype=U8)
    base = np.array([0xFFFF9, 7, 0x4321], dtype=np.uint32)
    fbase = np.array([0xFFFFFFFA, 3, 0x777], dtype=np.uint32)
    senders = np.zeros(n, dtype=fr.SENDER_DTYPE)
    senders["base_id"] = senders["next_id"] = base
    senders["window_size"], senders["max_alloc"] = W, 64 * 1448
    senders["window_parent_id"], senders["channel_parent_id"] = fr.NO_PARENT, fr.NO_PARENT
    queues, log = fr.new_frame_queues(n, 16, 16, fbase)
    states, arenas = fr.new_resend_states(n, W, 64 * 1448, 16, 16, heap_cap=256, stage_cap=320)
    rstates, entries = fr.new_rate_states(n, 0xFFFFFFFF, 32)
    windows = fr.new_frame_windows(n, 4096, fbase)
    receivers = fr.new_receivers(n, W, base, 64 * 1448)
    frags = int(np.maximum(1, (sizes + 1447) // 1448).sum())
    IC = frags + n * 320       # item slots: every fragment new, and a full stage per connection
    FC = IC                    # frames
    d = {k: _t(v, w) for k, v, w in (("packets", packets, 16), ("senders", senders, 304), ("queues", queues, 192),
                                     ("log", log, 24), ("states", states, 104), ("rstates", rstates, 112),
                                     ("entries", entries, 16), ("windows", windows, 24), ("receivers", receivers, 560))}
    A = {k: _t(v, WIDTH[k]) for k, v in arenas.items()}
    pf = _t(np.arange(n + 1, dtype=np.uint64) * per)
    owner = torch.arange(n * per, device=DEV) // per
    local = torch.arange(n * per, device=DEV) % per
    d_payload = _t(payload)
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
    flushes = _t(np.zeros(n, dtype=fr.FLUSH_DTYPE), 24)
    ack_fl = np.zeros(n, dtype=fr.FLUSH_DTYPE)
    ack_fl["kind"], ack_fl["flush_alloc"] = fr.ACK, 1 << 40
    ack_flushes = _t(ack_fl, 24)
    data_fl = np.zeros(n, dtype=fr.FLUSH_DTYPE)
    data_fl["kind"], data_fl["flush_alloc"] = fr.DATA, 4000
    flushes.copy_(_t(data_fl, 24))
    budget = flushes[:, 0:8].clone()
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    extra = z(n, dtype=torch.int32)
    slots, slot_first = z(n * W, 32), _t(np.arange(n + 1, dtype=np.uint64) * W)
    carry = [z(1 << 21), z(1 << 21)]
    GC = n + FC                # ack groups, and so ack frames
    ack_infos, ack_items, ack_ff = z(GC, 32), z(GC, 24), z(n + 1, dtype=torch.int64)
    sent, sent_first, fres = z(FC, 24), z(n + 1, dtype=torch.int64), z(n, 24)
    nonce = torch.from_numpy(rng.integers(0, 1 << 31, (FC + 31) // 32 + 1).astype(np.int32)).to(DEV)
    keep_data = torch.from_numpy((rng.random((TICKS, FC)) >= 0.2).astype(U8)).to(DEV)
    keep_ack = torch.from_numpy((rng.random((TICKS, GC)) >= 0.1).astype(U8)).to(DEV)
    keep_data[TICKS - QUIET:], keep_ack[TICKS - QUIET:] = 1, 1        # (the link is clean at the end: the queues drain)
    ticks_np = np.zeros((TICKS, n), dtype=fr.RATE_TICK_DTYPE)
    ticks_np["now_ms"], ticks_np["delta_time_s"] = (1000 + 20 * np.arange(TICKS))[:, None], 0.02
    d_ticks = _t(ticks_np.reshape(-1), 32).reshape(TICKS, n, 32)
    d_now = torch.from_numpy(ticks_np["now_ms"].astype(np.int64)).to(DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def build(infos, items, pay, offsets, rows):
        out = z(rows * 1472)
        check(lib().ufc_build_batch_varlen(engine._ctx, P(infos), P(items), items.shape[0], None, P(pay) if pay.numel() else None,
                                           pay.numel(), rows, P(offsets), P(out), out.numel(), 1, None, st), "build")
        return out

    delivered, trace = [], []
    for t in range(TICKS):
        # ---- the sender ----
        steps = engine.rate_begin(d["rstates"], d_now[t].contiguous(), extra, states_out=d["rstates"])["steps"]
        fq = engine.frame_queue(ack_infos, ack_items, ack_ff, sent, sent_first, d["queues"], steps, d["log"], A["ref_acked"],
                                queues_out=d["queues"])["results"]
        rate = engine.rate_step(d["rstates"], d_ticks[t].contiguous(), fq, d["entries"], flush_results=fres, result_index=idx,
                                flushes=flushes, flush_index=idx, states_out=d["rstates"])["results"]
        flushes[:, 0:8] = budget
        flushes[:, 12:16] = fq[:, 52:56]              # window_room
        flushes[:, 16:20] = d["queues"][:, 4:8]       # id0 = log_next_id
        i32(d["senders"])[:, 3] = t + 1               # flush_id
        i32(d["senders"])[:, 9] = -1                  # take
        i32(d["senders"])[:, 10] = 0                  # reserve_items
        br = engine.resend_begin(ack_infos, ack_ff, d["queues"], d["log"], rate, flushes, d["states"], d["senders"], A,
                                 states_out=d["states"], senders_out=d["senders"])["results"]
        items, flush_first, pres, sres, _, _ = engine.emit_packets(d["packets"], pf, d["senders"], IC)
        engine.resend_place(d["states"], br, A, flush_first, items)
        infos, fres, frames_used = engine.pack_flushes(items, flush_first, flushes, frames_cap=FC, nonce_bits=nonce)
        offsets, _ = engine.build_sizes_varlen(infos, items, d_payload.numel())
        cm = engine.resend_commit(fres, infos, offsets, frames_used, items, flush_first, d["packets"], pf, pres, sres, br, rate,
                                  d["states"], d["senders"], A, next_extra_flags=extra, states_out=d["states"])
        sent, sent_first = cm["sent"], cm["sent_first"]
        out2 = engine.emit_packets(d["packets"], pf, cm["retake"], 0, senders_out=d["senders"])
        consumed = i32(out2[3])[:, 2].to(torch.int64)[owner]
        stale = local < consumed                       # the consumed packets: stale TimeSensitive ones from now on
        d["packets"][:, 13] = torch.where(stale, torch.zeros_like(d["packets"][:, 13]), d["packets"][:, 13])
        d["packets"][:, 8:12] = torch.where(stale[:, None], torch.full_like(d["packets"][:, 8:12], 255), d["packets"][:, 8:12])
        wire = build(infos, items, d_payload, offsets, FC)
        # ---- the link, and the receiving peer ----
        _, valid = engine.crc_varlen(wire, offsets)
        valid &= keep_data[t]
        infos2, items2, _ = engine.parse_varlen(wire, offsets, valid, items_cap=IC)
        fw = engine.frame_window(infos2, sent_first, d["windows"], groups_cap=GC, windows_out=d["windows"])
        rx = engine.receive_packets(infos2, items2, wire, sent_first, d["receivers"], slots, slot_first, carry[t % 2],
                                    src_base=offsets[:FC].contiguous(), frame_accept=fw["frame_accept"],
                                    carry_out=carry[1 - t % 2], out_bytes=z(1 << 18), packets=z(n * per + 8, 24),
                                    receivers_out=d["receivers"], want_item_status=False)
        delivered.append((rx["packets"], rx["packet_first"], rx["out_bytes"], rx["results"]))
        trace.append((br, cm["results"], fres, fq, d["senders"][:, 0:8].clone(), d["receivers"][:, 0:8].clone()))
        ack_flushes[:, 16:20] = d["windows"][:, 0:4]    # frame_window_base_id
        ack_flushes[:, 20:24] = d["receivers"][:, 0:4]  # packet_window_base_id
        a_infos, a_res, a_used = engine.pack_flushes(fw["groups"], fw["group_first"], ack_flushes, frames_cap=GC)
        d["windows"][:, 17] = 0                         # every group was flushed: has_tail
        a_off, _ = engine.build_sizes_varlen(a_infos, fw["groups"], 0)
        a_wire = build(a_infos, fw["groups"], z(0), a_off, GC)
        # ---- the link back: the next tick's ack frames ----
        _, a_valid = engine.crc_varlen(a_wire, a_off)
        a_valid &= keep_ack[t]
        ack_infos, ack_items, _ = engine.parse_varlen(a_wire, a_off, a_valid, items_cap=GC)
        ack_ff = torch.cat([i32(a_res)[:, 0].to(torch.int64), a_used])
    torch.cuda.synchronize()
    # ---- read back, once ----
    def timeline(c):
        """One line per tick of connection c, for a failure's message."""
        out = []
        for t, ((b, m, f, q, sd, rv), (pk, pfirst, _, res)) in enumerate(zip(trace, delivered)):
            b, m = _np(b, fr.RESEND_RESULT_DTYPE)[c], _np(m, fr.RESEND_COMMIT_RESULT_DTYPE)[c]
            f, q = _np(f, fr.FLUSH_RESULT_DTYPE)[c], _np(q, fr.FRAME_QUEUE_RESULT_DTYPE)[c]
            sd, rv = sd.cpu().numpy().view(np.uint32)[c], rv.cpu().numpy().view(np.uint32)[c]
            res = _np(res, fr.RECEIVER_RESULT_DTYPE)[c]
            seqs = _np(pk, fr.RX_PACKET_DTYPE)["sequence_id"][int(pfirst[c]): int(pfirst[c + 1])]
            out.append(f"t{t} begin stop {int(b['stop'])} resent {int(b['n_resent'])} pend {int(b['n_pending_staged'])} freed "
                       f"{int(b['packets_freed'])} dead {int(b['heap_popped_dead'])} acked {int(b['heap_popped_acked'])} | pack frames "
                       f"{int(f['frame_count'])} items {int(f['items_packed'])} stop {int(f['stop'])} | commit stop {int(m['stop'])} take "
                       f"{int(m['take'])} entered {int(m['packets_entered'])} heap {int(m['heap_len'])} pending {int(m['pending_count'])} | "
                       f"fq acked {int(q['frames_acked'])} room {int(q['window_room'])} | tx {sd[0]:x}..{sd[1]:x} rx {rv[0]:x}..{rv[1]:x} "
                       f"status {[int(v) for v in res['status_count']]} completed {int(res['packets_completed'])} dud {int(res['packets_dud'])} "
                       f"advanced {int(res['advanced'])} delivered "
                       f"{[hex(int(v)) for v in seqs]}")
        return "\n".join(out)

    got = {}
    order = {}
    for pk, pfirst, ob, res in delivered:
        res = _np(res, fr.RECEIVER_RESULT_DTYPE)
        assert (res["stop"] == 0).all()
        pk, pfirst, ob = _np(pk, fr.RX_PACKET_DTYPE), pfirst.cpu().numpy(), ob.cpu().numpy()
        for c in range(n):
            for r in pk[int(pfirst[c]): int(pfirst[c + 1])]:
                key = (c, int(r["sequence_id"]))
                assert key not in got and not int(r["flags"]), ("delivered twice, or a dud", key)
                got[key] = ob[int(r["out_offset"]): int(r["out_offset"]) + int(r["len"])].tobytes()
                order.setdefault((c, int(r["channel_id"])), []).append(E.sub(int(r["sequence_id"]), int(base[c])))
    for c in range(n):
        for k in range(per):
            p = packets[c * per + k]
            want = payload[int(p["data_offset"]): int(p["data_offset"]) + int(p["data_len"])].tobytes()
            assert got.get((c, (int(base[c]) + k) & E.ID_MASK)) == want, f"packet {k} of connection {c} {p}\n" + timeline(c)
    assert len(got) == n * per and all(v == sorted(v) for v in order.values())
    s = _np(d["states"], fr.RESEND_DTYPE)
    sd = _np(d["senders"], fr.SENDER_DTYPE)
    assert (s["heap_len"] == 0).all() and (s["pending_count"] == 0).all(), (s["heap_len"], s["pending_count"])
    assert (sd["base_id"] == sd["next_id"]).all() and (sd["alloc"] == 0).all()
    assert int(s["tx_head"].min()) > 20   # (frames went out, and fragments were resent: more refs than fragments)
    assert int(s["tx_head"].sum()) > frags


def test_lane_form_equals_host(engine):
    """16,500 connections: from 16,384 on the launch gives every connection a lane in place of a wave.  Three
    connections' states after some lossy traffic, tiled; begin and commit on the device against the host calls, every
    output and every arena byte."""
    p = R.Pipeline(T.lossy_configs()[:3], R.HostBackend(4))
    R.run_lossy(p, random.Random(8), 20, loss=0.3)
    reps, n0 = 5500, p.n
    n = reps * n0
    k = np.repeat(np.arange(reps, dtype=np.uint64), n0)
    states, senders, queues = np.tile(p.states, reps), np.tile(p.senders, reps), np.tile(p.queues, reps)
    for name, key in (("heap", "heap"), ("pkt", "pkts"), ("frag", "frag_acked"), ("tx", "tx"), ("stage", "stage")):
        states[name + "_first"] += k * np.uint64(p.arenas[key].size)
    queues["log_first"] += k * np.uint64(p.log.size)
    log = np.tile(p.log, reps)
    arenas = {key: np.tile(v, reps) for key, v in p.arenas.items()}
    rate = np.zeros(n, dtype=fr.RATE_RESULT_DTYPE)
    rate["now_ms"], rate["rtt_ms"] = 5000, 40
    flushes = np.zeros(n, dtype=fr.FLUSH_DTYPE)
    flushes["flush_alloc"], flushes["kind"], flushes["window_room"] = 20000, fr.DATA, 6
    flushes["id0"] = queues["log_next_id"]
    senders["take"], senders["reserve_items"] = 0xFFFFFFFF, 0
    ff = np.zeros(n + 1, dtype=np.uint64)
    none = np.zeros(0, dtype=fr.FRAME_INFO_DTYPE)
    be = GpuBackend(engine)
    copy = lambda a: {key: v.copy() for key, v in a.items()}  # noqa: E731
    # begin
    h_ar = copy(arenas)
    h = fr.resend_begin_host(none, ff, queues, log, rate, flushes, states, senders, h_ar, nthreads=8)
    d_ar, d_s, d_sd = copy(arenas), states.copy(), senders.copy()
    d_res = be.resend_begin(none, ff, queues, log, rate, flushes, d_s, d_sd, d_ar, np.zeros(n, np.uint32))
    assert d_res.tobytes() == h["results"].tobytes() and int(d_res["n_resent"].sum()) > reps
    assert d_s.tobytes() == h["states_out"].tobytes() and d_sd.tobytes() == h["senders_out"].tobytes()
    for key in h_ar:
        assert d_ar[key].tobytes() == h_ar[key].tobytes(), key
    # the emit, the place, the pack and the sizes on the host; then commit
    packets = np.zeros(2 * n, dtype=fr.PACKET_DTYPE)
    packets["data_len"], packets["mode"] = np.tile([300, 2000], n), fr.SEND_RELIABLE
    packets["data_offset"] = np.arange(2 * n) * 2000 % (1 << 30)
    pfirst = np.arange(n + 1, dtype=np.uint64) * 2
    items, flush_first, pres, sres, _, used = fr.emit_packets_host(packets, pfirst, h["senders_out"], nthreads=8)
    fr.resend_place_host(h["states_out"], h["results"], h_ar, flush_first, items, nthreads=8)
    frames, fres, frames_used = fr.pack_host(items, flush_first, flushes, nthreads=8)
    frames = frames[:frames_used]
    offs = R.build_sizes_host(frames, items)
    hc = fr.resend_commit_host(fres, frames, offs, frames_used, items, flush_first, packets, pfirst, pres, sres, h["results"],
                               rate, h["states_out"], h["senders_out"], h_ar, next_extra_flags=np.zeros(n, np.uint32), nthreads=8)
    dc = be.resend_commit(fres, frames, offs, frames_used, items, flush_first, packets, pfirst, pres, sres, d_res, rate, d_s, d_sd,
                          d_ar, next_extra_flags=np.zeros(n, np.uint32))
    assert (hc["results"]["stop"] != R.BAD_STATE).all(), np.unique(hc["results"]["stop"])
    assert int(hc["results"]["heap_pushed"].sum()) > reps and int(hc["results"]["packets_entered"].sum()) > reps
    for key in ("results", "retake", "sent", "sent_first", "next_extra_flags"):
        assert dc[key].tobytes() == np.ascontiguousarray(hc[key]).tobytes(), key
    assert d_s.tobytes() == hc["states_out"].tobytes()
    for key in ("heap", "pkts", "frag_acked", "tx"):
        assert d_ar[key].tobytes() == h_ar[key].tobytes(), key
