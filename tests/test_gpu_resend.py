"""GPU: the batched resend calls (ufc_resend_begin_varlen / ufc_resend_place_varlen / ufc_resend_commit_varlen,
FrameCrcEngine.resend_begin / resend_place / resend_commit) with the device calls in the host calls' place: the
hand-traced goldens and the generated lossy traffic of tests/test_resend_cpu.py, every tick compared with
tests/resend_expect.py's model byte for byte (results, states, the heap, the packet table, the ack bytes, the tx ring,
staged and placed items, sent records), at the smallest shapes that can go wrong; two streams; a BAD_STATE
connection between good ones against the host call.  Every other call of the tick (frame_queue, emit_packets,
pack_flushes, build_sizes) is the device form too.

All of that runs a wave per connection.  From 16,384 connections on the launch gives a connection a lane (the form
the product's batches always take), and the tests at the end run it: the same edges in batches padded to 16,400 and
more connections, the switch between the two forms, and 66,000 connections past the launch grid; there every resend
call has the host call over the same inputs as a second reference (CheckedBackend)."""
import json
import os
import random

import numpy as np
import pytest
import torch

from uflow_amd import frame as fr
from uflow_amd.batch import records, rows

import emit_expect as E
import resend_expect as R
import test_resend_cpu as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8 = np.uint8


def _back(t, arr):
    """The device tensor's bytes into the host array it was made from."""
    arr[...] = records(t, arr.dtype).reshape(arr.shape)


class GpuBackend:
    """resend_expect.HostBackend's methods on the device forms: arrays go up, the call is queued, arrays come back."""

    def __init__(self, engine, stream=None):
        self.e, self.stream = engine, stream

    def sync(self):
        (self.stream.synchronize if self.stream is not None else torch.cuda.synchronize)()

    def ctx(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else torch.cuda.stream(torch.cuda.current_stream())

    def up_arenas(self, arenas):
        return {k: rows(v, DEV) for k, v in arenas.items()}

    def down_arenas(self, d, arenas):
        for k in arenas:
            _back(d[k], arenas[k])

    def frame_queue(self, infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked):
        with self.ctx():
            q, lg, ra = rows(queues, DEV), rows(log, DEV), rows(ref_acked, DEV)
            d = self.e.frame_queue(rows(infos, DEV), rows(items, DEV), rows(frame_first, DEV), rows(sent, DEV), rows(sent_first, DEV), q,
                                   rows(steps, DEV), lg, ra, queues_out=q, stream=self.stream)
            self.sync()
        _back(q, queues), _back(lg, log), _back(ra, ref_acked)
        return records(d["results"], fr.FRAME_QUEUE_RESULT_DTYPE)

    def resend_begin(self, infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags):
        with self.ctx():
            A, s, sd = self.up_arenas(arenas), rows(states, DEV), rows(senders, DEV)
            d = self.e.resend_begin(rows(infos, DEV), rows(frame_first, DEV), rows(queues, DEV), rows(log, DEV), rows(rate, DEV),
                                    rows(flushes, DEV), s, sd, A, flags=rows(flags, DEV), states_out=s, senders_out=sd,
                                    stream=self.stream)
            self.sync()
        self.down_arenas(A, arenas)
        _back(s, states), _back(sd, senders)
        return records(d["results"], fr.RESEND_RESULT_DTYPE)

    def emit(self, packets, packet_first, senders, items):
        with self.ctx():
            it = rows(items, DEV)
            out = self.e.emit_packets(rows(packets, DEV), rows(packet_first, DEV), rows(senders, DEV), items.size, items=it,
                                      stream=self.stream)
            self.sync()
        _back(it, items)
        return (items, records(out[1], np.uint64), records(out[2], fr.PACKET_RESULT_DTYPE), records(out[3], fr.SENDER_RESULT_DTYPE),
                records(out[4], fr.SENDER_DTYPE), int(out[5].item()))

    def emit_state(self, packets, packet_first, senders):
        with self.ctx():
            out = self.e.emit_packets(rows(packets, DEV), rows(packet_first, DEV), rows(senders, DEV), 0, stream=self.stream)
            self.sync()
        return records(out[3], fr.SENDER_RESULT_DTYPE), records(out[4], fr.SENDER_DTYPE)

    def resend_place(self, states, begin_results, arenas, flush_first, items):
        with self.ctx():
            it = rows(items, DEV)
            self.e.resend_place(rows(states, DEV), rows(begin_results, DEV), {"stage": rows(arenas["stage"], DEV)}, rows(flush_first, DEV),
                                it, stream=self.stream)
            self.sync()
        _back(it, items)

    def pack(self, items, flush_first, flushes):
        with self.ctx():
            infos, results, used = self.e.pack_flushes(rows(items, DEV), rows(flush_first, DEV), rows(flushes, DEV), stream=self.stream)
            self.sync()
        return records(infos, fr.FRAME_INFO_DTYPE), records(results, fr.FLUSH_RESULT_DTYPE), int(used.item())

    def build_sizes(self, infos, items):
        if infos.size == 0:
            return np.zeros(1, dtype=np.uint64)
        with self.ctx():
            offsets, _ = self.e.build_sizes_varlen(rows(infos, DEV), rows(items, DEV), 1 << 40, stream=self.stream)
            self.sync()
        return records(offsets, np.uint64)

    def resend_commit(self, flush_results, infos, out_offsets, frames_used, items, flush_first, packets, packet_first,
                      packet_results, sender_results, begin_results, rate, states, senders, arenas, next_extra_flags=None,
                      states_out=None):
        with self.ctx():
            A = self.up_arenas({k: v for k, v in arenas.items() if k not in ("ref_acked", "stage")})
            s, extra = rows(states, DEV), rows(next_extra_flags, DEV)
            d = self.e.resend_commit(rows(flush_results, DEV), rows(infos, DEV), rows(out_offsets, DEV),
                                     torch.tensor([frames_used], dtype=torch.int64, device=DEV), rows(items, DEV),
                                     rows(flush_first, DEV), rows(packets, DEV), rows(packet_first, DEV), rows(packet_results, DEV),
                                     rows(sender_results, DEV), rows(begin_results, DEV), rows(rate, DEV), s, rows(senders, DEV), A,
                                     next_extra_flags=extra, states_out=s, stream=self.stream)
            self.sync()
        for k in A:
            _back(A[k], arenas[k])
        _back(s, states)
        return {"results": records(d["results"], fr.RESEND_COMMIT_RESULT_DTYPE), "retake": records(d["retake"], fr.SENDER_DTYPE),
                "sent": records(d["sent"], fr.SENT_FRAME_DTYPE), "sent_first": records(d["sent_first"], np.uint64),
                "next_extra_flags": records(extra, np.uint32)}


def _same(dev, host, what):
    """Byte equality of what the device call and the host call left, with the first differing record named."""
    dev, host = np.ascontiguousarray(dev).reshape(-1), np.ascontiguousarray(host).reshape(-1)
    assert dev.dtype == host.dtype and dev.size == host.size, (what, dev.dtype, dev.size, host.dtype, host.size)
    x, y = dev.view(U8), host.view(U8)
    if not np.array_equal(x, y):
        at = int(np.flatnonzero(x != y)[0]) // dev.dtype.itemsize
        raise AssertionError((what, "device and host differ, first at record", at, dev[at], host[at]))


def _staged(states, begin):
    """The stage slots that are part of the contract: the first n_resent + n_pending_staged of every region."""
    m = begin["n_resent"].astype(np.int64) + begin["n_pending_staged"].astype(np.int64)
    m[begin["stop"] == R.BAD_STATE] = 0
    return np.repeat(states["stage_first"].astype(np.int64) - (np.cumsum(m) - m), m) + np.arange(int(m.sum()))


def _copy(arenas):
    return {k: v.view(U8).copy().view(v.dtype) for k, v in arenas.items()}   # (as bytes: a record copy goes field by field)


class CheckedBackend:
    """The device calls with the host calls as their reference: resend_begin, resend_place and resend_commit run on
    the host and on the device over copies of the same inputs, every output, every state record and every arena must
    be equal byte for byte (of the stage, the slots begin staged: what lies behind them is outside the contract), and
    the device's arrays go back to the caller.  The other calls of a tick run on the device alone.  Under a
    resend_expect.Pipeline this gives the modelled connections two references and its padding one."""

    def __init__(self, dev, host=None):
        self.dev, self.host = dev, host or R.HostBackend(8)
        self.checked = {"begin": 0, "place": 0, "commit": 0}
        self.room = {}

    def __getattr__(self, name):   # frame_queue, emit, emit_state, pack, build_sizes
        return getattr(self.dev, name)

    def copies(self, arenas):
        """The host call's copies of the arenas, in buffers that are kept from call to call."""
        for k, v in arenas.items():
            if k not in self.room or self.room[k].size != v.size:
                self.room[k] = np.empty_like(v)
            np.copyto(self.room[k].view(U8), v.view(U8))   # (as bytes: a record copy goes field by field)
        return {k: self.room[k] for k in arenas}

    def resend_begin(self, infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags):
        h_s, h_sd, h_ar = states.copy(), senders.copy(), self.copies(arenas)
        h = self.host.resend_begin(infos, frame_first, queues, log, rate, flushes, h_s, h_sd, h_ar, flags)
        d = self.dev.resend_begin(infos, frame_first, queues, log, rate, flushes, states, senders, arenas, flags)
        _same(d, h, "begin: results")
        _same(states, h_s, "begin: states")
        _same(senders, h_sd, "begin: senders")
        at = _staged(states, d)
        for k in arenas:
            if k == "stage":
                _same(arenas[k][at], h_ar[k][at], "begin: the staged items")
            else:
                _same(arenas[k], h_ar[k], "begin: arena " + k)
        self.checked["begin"] += 1
        return d

    def resend_place(self, states, begin_results, arenas, flush_first, items):
        h_items = items.copy()
        self.host.resend_place(states, begin_results, arenas, flush_first, h_items)
        self.dev.resend_place(states, begin_results, arenas, flush_first, items)
        _same(items, h_items, "place: items")
        self.checked["place"] += 1

    def resend_commit(self, flush_results, infos, out_offsets, frames_used, items, flush_first, packets, packet_first,
                      packet_results, sender_results, begin_results, rate, states, senders, arenas, next_extra_flags=None,
                      states_out=None):
        """In place: `states`, the arenas and (as the device form does) nothing else of the caller's."""
        args = (flush_results, infos, out_offsets, frames_used, items, flush_first, packets, packet_first, packet_results,
                sender_results, begin_results, rate)
        h_s, h_ar = states.copy(), self.copies(arenas)
        h = self.host.resend_commit(*args, h_s, senders, h_ar, next_extra_flags=next_extra_flags.copy(), states_out=h_s)
        d = self.dev.resend_commit(*args, states, senders, arenas, next_extra_flags=next_extra_flags, states_out=states)
        for k in ("results", "retake", "sent", "sent_first", "next_extra_flags"):
            _same(d[k], h[k], "commit: " + k)
        _same(states, h_s, "commit: states")
        for k in ("heap", "pkts", "frag_acked", "tx"):
            _same(arenas[k], h_ar[k], "commit: arena " + k)
        self.checked["commit"] += 1
        return d


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


def tx_ring_pipeline(backend, ticks=70, **padding):
    p = R.Pipeline([R.Config(window_size=64, max_alloc=1 << 20, frame_window=1, frame_tail=0, heap_cap=64)], backend, **padding)
    R.run_lossy(p, random.Random(3), ticks, loss=0.0, alloc=(1 << 20, 1 << 21),
                traffic=lambda r, t, c: [(r.randrange(20), 0, E.RELIABLE) for _ in range(r.randrange(7, 12))])
    assert {"tx_wrap", "tx_skip"} <= p.seen
    return p


def test_tx_ring_wraps_within_a_call(engine):
    tx_ring_pipeline(GpuBackend(engine))


def heap_pipeline(backend, k, **padding):
    p = R.Pipeline([R.Config(window_size=1024, max_alloc=1 << 20, frame_window=64, frame_tail=16, heap_cap=1024)],
                   backend, **padding)
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
    return p


@pytest.mark.parametrize("k", [1, 63, 64, 65, 1000])
def test_heap_sizes(engine, k):
    """k Persistent packets sent at once and all due one RTT later: k pops and pushes through a heap of k entries (63
    fills six levels, 64 and 65 open the seventh), then the acks empty it."""
    heap_pipeline(GpuBackend(engine), k)


def fragments_pipeline(backend, **padding):
    p = R.Pipeline([R.Config(window_size=8, max_alloc=200000, frame_window=256, frame_tail=16, heap_cap=256, stage_cap=512)],
                   backend, **padding)
    p.enqueue(0, 130 * 1448, 2, E.PERSISTENT)
    p.tick(0, 100, 1000, [[]])
    assert int(p.states[0]["pending_count"]) == 129
    sent = p.tick(10, 100, 1 << 30, [[]])[0]
    assert len(sent) == 129 and int(p.states[0]["heap_len"]) == 130 and int(p.states[0]["pending_count"]) == 0
    p.tick(110, 100, 1 << 30, [[]])
    assert "pending_packed" in p.seen and "resent" in p.seen
    return p


def test_130_fragment_packet_cut_by_the_flush_allocation(engine):
    """One fragment goes, 129 stay pending: staged in three lane passes, then packed, pushed and acknowledged."""
    fragments_pipeline(GpuBackend(engine))


def acknowledge_pipeline(backend, **padding):
    p = R.Pipeline([R.Config(window_size=256, max_alloc=1 << 20, frame_window=64, frame_tail=16, heap_cap=256)],
                   backend, **padding)
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
    return p


def test_acknowledge_frees_0_1_64_65_packets(engine):
    acknowledge_pipeline(GpuBackend(engine))


@pytest.mark.parametrize("pipeline", T.LANE_PIPELINES)
def test_lane_63_and_tile_seam(engine, pipeline):
    """The wave form's cross-lane reads on lane 63 and on lane 0 of the next tile: the freed ids' window and channel
    parents, the ack frames' ballot, the stopping packet of commit (one connection each: the wave form)."""
    pipeline(GpuBackend(engine))


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
    d = {k: rows(v, DEV) for k, v in (("packets", packets), ("senders", senders), ("queues", queues), ("log", log),
                                      ("states", states), ("rstates", rstates), ("entries", entries),
                                      ("windows", windows), ("receivers", receivers))}
    A = {k: rows(v, DEV) for k, v in arenas.items()}
    pf = rows(np.arange(n + 1, dtype=np.uint64) * per, DEV)
    owner = torch.arange(n * per, device=DEV) // per
    local = torch.arange(n * per, device=DEV) % per
    d_payload = rows(payload, DEV)
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
    zrec = lambda count, dt: z(count, dt.itemsize)  # noqa: E731
    flushes = rows(np.zeros(n, dtype=fr.FLUSH_DTYPE), DEV)
    ack_fl = np.zeros(n, dtype=fr.FLUSH_DTYPE)
    ack_fl["kind"], ack_fl["flush_alloc"] = fr.ACK, 1 << 40
    ack_flushes = rows(ack_fl, DEV)
    data_fl = np.zeros(n, dtype=fr.FLUSH_DTYPE)
    data_fl["kind"], data_fl["flush_alloc"] = fr.DATA, 4000
    flushes.copy_(rows(data_fl, DEV))
    budget = flushes[:, 0:8].clone()
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    extra = z(n, dtype=torch.int32)
    slots, slot_first = zrec(n * W, fr.RX_SLOT_DTYPE), rows(np.arange(n + 1, dtype=np.uint64) * W, DEV)
    carry = [z(1 << 21), z(1 << 21)]
    GC = n + FC                # ack groups, and so ack frames
    ack_infos, ack_items, ack_ff = zrec(GC, fr.FRAME_INFO_DTYPE), zrec(GC, fr.ITEM_DTYPE), z(n + 1, dtype=torch.int64)
    sent, sent_first, fres = zrec(FC, fr.SENT_FRAME_DTYPE), z(n + 1, dtype=torch.int64), zrec(n, fr.FLUSH_RESULT_DTYPE)
    nonce = torch.from_numpy(rng.integers(0, 1 << 31, (FC + 31) // 32 + 1).astype(np.int32)).to(DEV)
    keep_data = torch.from_numpy((rng.random((TICKS, FC)) >= 0.2).astype(U8)).to(DEV)
    keep_ack = torch.from_numpy((rng.random((TICKS, GC)) >= 0.1).astype(U8)).to(DEV)
    keep_data[TICKS - QUIET:], keep_ack[TICKS - QUIET:] = 1, 1        # (the link is clean at the end: the queues drain)
    ticks_np = np.zeros((TICKS, n), dtype=fr.RATE_TICK_DTYPE)
    ticks_np["now_ms"], ticks_np["delta_time_s"] = (1000 + 20 * np.arange(TICKS))[:, None], 0.02
    d_ticks = rows(ticks_np.reshape(-1), DEV).reshape(TICKS, n, -1)
    d_now = torch.from_numpy(ticks_np["now_ms"].astype(np.int64)).to(DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def build(infos, items, pay, offsets, count):
        out = z(count * 1472)
        check(lib().ufc_build_batch_varlen(engine._ctx, P(infos), P(items), items.shape[0], None, P(pay) if pay.numel() else None,
                                           pay.numel(), count, P(offsets), P(out), out.numel(), 1, None, st), "build")
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
                                    carry_out=carry[1 - t % 2], out_bytes=z(1 << 18), packets=zrec(n * per + 8, fr.RX_PACKET_DTYPE),
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
            b, m = records(b, fr.RESEND_RESULT_DTYPE)[c], records(m, fr.RESEND_COMMIT_RESULT_DTYPE)[c]
            f, q = records(f, fr.FLUSH_RESULT_DTYPE)[c], records(q, fr.FRAME_QUEUE_RESULT_DTYPE)[c]
            sd, rv = sd.cpu().numpy().view(np.uint32)[c], rv.cpu().numpy().view(np.uint32)[c]
            res = records(res, fr.RECEIVER_RESULT_DTYPE)[c]
            seqs = records(pk, fr.RX_PACKET_DTYPE)["sequence_id"][int(pfirst[c]): int(pfirst[c + 1])]
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
        res = records(res, fr.RECEIVER_RESULT_DTYPE)
        assert (res["stop"] == 0).all()
        pk, pfirst, ob = records(pk, fr.RX_PACKET_DTYPE), pfirst.cpu().numpy(), ob.cpu().numpy()
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
    s = records(d["states"], fr.RESEND_DTYPE)
    sd = records(d["senders"], fr.SENDER_DTYPE)
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


# ---- the lane form (a lane per connection, from 16,384 connections on) and the launches past one grid ----
# Every test below runs through CheckedBackend, over a batch that resend_expect.Pipeline pads with replicas of its
# modelled connections and idle fillers until the launch takes the lane form.
LOSSY_LOSS = [0.25, 0.25, 0.25, 0.25, 0.1, 0.6]
LOSSY_SEED, LOSSY_TICKS, LOSSY_HOSTILE_FROM = 18, 12, 10   # the shortest host-only run found that sees every event below
LANE_TOTAL = 16406   # 16,384 + 22: the last lane block is part full


def checked(engine):
    return CheckedBackend(GpuBackend(engine))


def padded(n, total, replicas):
    return {"replicas": replicas, "fillers": total - n - replicas}


def busy_traffic(rng, t, c):
    """resend_expect.default_traffic and up to nine small packets more a tick: with them a connection comes to have
    more than 64 live refs, and begin's ack propagation (a lane per live ref) has marked refs for its last lane too
    ("ref_acked_lane_63"), which the default traffic does not reach within 40 ticks."""
    return R.default_traffic(rng, t, c) + [(rng.randrange(1, 100), rng.randrange(3), E.RELIABLE) for _ in range(rng.randrange(0, 10))]


def lossy_batch(backend):
    """The six lossy connections, 250 replicas in the first 256 slots and idle fillers behind, LOSSY_TICKS ticks."""
    p = R.Pipeline(T.lossy_configs(), backend, **padded(6, LANE_TOTAL, 250))
    R.run_lossy(p, random.Random(LOSSY_SEED), LOSSY_TICKS, hostile=0.3, hostile_from=LOSSY_HOSTILE_FROM, loss=LOSSY_LOSS,
                traffic=busy_traffic)
    return p


@pytest.fixture(scope="module")
def lane_lossy(engine):
    try:
        return lossy_batch(checked(engine))
    except AssertionError as e:   # (raised again by ran() in every test that uses the run: they fail, each by name)
        return e


def ran(batch):
    if isinstance(batch, AssertionError):
        raise batch
    return batch


def clone(p):
    """A Pipeline of its own with the same backend (the shared one stays as it was)."""
    import copy
    return copy.deepcopy(p, {id(p.backend): p.backend})


def test_lane_lossy_traffic(lane_lossy):
    """16,406 connections, so rs_begin_lane_kernel and rs_commit_lane_kernel (SerialWave) with a part-full last block:
    the lossy traffic of test_lossy_traffic_small_rings with ack frames every tick, in every wave of the first 256
    connections; the padding's acknowledge, ack propagation and heap pushes had work to do."""
    p = ran(lane_lossy)
    assert p.total == LANE_TOTAL >= 16384 and p.total % 64 and p.backend.checked == {k: LOSSY_TICKS for k in ("begin", "place", "commit")}
    assert {R.DONE, R.SIZE_LIMITED, R.WINDOW_LIMITED, R.REF_HANG, R.STAGE_FULL, R.HEAP_FULL} <= p.seen_stops
    assert R.BAD_STATE not in p.seen_stops
    assert {"dead_pop", "acked_pop", "resent", "partial_packet", "frag_wrap", "id_wrap", "hang"} <= p.seen
    assert "ref_acked_lane_63" in p.seen   # (SerialWave::sum's 64th turn had a ref to propagate)
    assert p.pad_totals["packets_freed"] > 0 and p.pad_totals["refs_acked"] > 0 and p.pad_totals["heap_pushed"] > 0, p.pad_totals


@pytest.mark.parametrize("k,replicas", [(64, 0), (65, 64), (1000, 0)])
def test_lane_heap_sizes(engine, k, replicas):
    """16,400 connections (lane form): test_heap_sizes' k pops and pushes through a heap of k entries inside one lane
    of SerialWave, beside idle fillers (k = 65: and 64 replicas)."""
    p = heap_pipeline(checked(engine), k, **padded(1, 16400, replicas))
    assert p.total == 16400 and p.total % 64 and (not replicas or p.pad_totals["n_resent"] == replicas * k)


def test_lane_130_fragment_packet(engine):
    """16,401 connections (lane form): the 129 pending fragments are staged by the three passes of SerialWave::lanes'
    own loop, in the modelled connection and in 64 replicas."""
    p = fragments_pipeline(checked(engine), **padded(1, 16401, 64))
    assert p.total == 16401 and p.total % 64 and p.pad_totals["heap_pushed"] == 64 * 130


def test_lane_acknowledge_frees_0_1_64_65_packets(engine):
    """16,402 connections (lane form): SerialWave::ballot and ::sum over acknowledge deltas of 0, 1, 64 and 65 packets,
    in the modelled connection and in 64 replicas."""
    p = acknowledge_pipeline(checked(engine), **padded(1, 16402, 64))
    assert p.total == 16402 and p.total % 64 and p.pad_totals["packets_freed"] == 64 * 130


TX_RING_TICKS = 31   # the first count at which the host-only run has seen tx_wrap and tx_skip


def test_lane_tx_ring_wraps_within_a_call(engine):
    """16,403 connections (lane form): rs_commit's walk over the frames inside a lane, the tx ring wrapping and
    skipping within a call, in the modelled connection and in 64 replicas."""
    p = tx_ring_pipeline(checked(engine), TX_RING_TICKS, **padded(1, 16403, 64))
    assert p.total == 16403 and p.total % 64


def one_round(be, B, m, now_ms, rtt_ms=40, flush_alloc=20000, infos=None, frame_first=None, flags=None):
    """begin, place and commit once through `be` over the first m connections of the batch B (states, senders, queues,
    log, arenas, window_room: copies are made), the emit, the pack and the sizes on the host in between; two packets
    wait at every connection.  Returns everything the calls left."""
    host = R.HostBackend(8)
    states, senders, queues, arenas = B["states"][:m].copy(), B["senders"][:m].copy(), B["queues"][:m], _copy(B["arenas"])
    infos = np.zeros(0, dtype=fr.FRAME_INFO_DTYPE) if infos is None else infos
    frame_first = np.zeros(m + 1, dtype=np.uint64) if frame_first is None else np.ascontiguousarray(frame_first[:m + 1])
    flags = np.zeros(m, dtype=np.uint32) if flags is None else flags
    rate = np.zeros(m, dtype=fr.RATE_RESULT_DTYPE)
    rate["now_ms"], rate["rtt_ms"] = now_ms, rtt_ms
    flushes = np.zeros(m, dtype=fr.FLUSH_DTYPE)
    flushes["flush_alloc"], flushes["kind"], flushes["window_room"] = flush_alloc, fr.DATA, B["window_room"][:m]
    flushes["id0"] = queues["log_next_id"]
    senders["take"], senders["reserve_items"] = 0xFFFFFFFF, 0
    senders["flush_id"] += 1
    begin = be.resend_begin(infos, frame_first, queues, B["log"], rate, flushes, states, senders, arenas, flags)
    after_begin = states.copy()
    packets = np.zeros(2 * m, dtype=fr.PACKET_DTYPE)
    packets["data_len"], packets["mode"], packets["flush_id"] = np.tile([300, 2000], m), fr.SEND_RELIABLE, np.repeat(senders["flush_id"], 2)
    packets["data_offset"] = np.arange(2 * m) * 2000 % (1 << 30)
    pfirst = np.arange(m + 1, dtype=np.uint64) * 2
    pre = senders.copy()
    items = E.filled_items(int(senders["reserve_items"].sum()) + 3 * m + 4)
    items, flush_first, pres, sres, _, used = host.emit(packets, pfirst, senders, items)
    be.resend_place(states, begin, arenas, flush_first, items)
    frames, fres, frames_used = host.pack(items[:int(used)], flush_first, flushes)
    frames = frames[:frames_used]
    offs = host.build_sizes(frames, items[:int(used)])
    commit = be.resend_commit(fres, frames, offs, frames_used, items[:int(used)], flush_first, packets, pfirst, pres, sres,
                              begin, rate, states, pre, arenas, next_extra_flags=B["extra"][:m].copy(), states_out=states)
    return {"begin": begin, "after_begin": after_begin, "senders": pre, "items": items[:int(used)], "flush_first": flush_first,
            "commit": commit, "states": states, "arenas": arenas}


def batch_of(p):
    """A Pipeline's arrays as one_round takes them; the frame window's room is what the last tick's frames left."""
    return {"states": p.states, "senders": p.senders, "queues": p.queues, "log": p.log, "arenas": p.arenas, "extra": p.extra,
            "window_room": p.last["window_room"]}


def region_bytes(states, arenas, c):
    s = states[c]
    return [arenas[key][int(s[name + "_first"]): int(s[name + "_first"]) + int(s[name + "_cap"])].tobytes()
            for name, key in (("heap", "heap"), ("pkt", "pkts"), ("frag", "frag_acked"), ("tx", "tx"), ("tx", "ref_acked"),
                              ("stage", "stage"))]


def test_lane_bad_state_among_good_ones(lane_lossy):
    """16,406 connections (lane form): a BAD_STATE lane of SerialWave returns early while its 63 neighbours go on.
    The connections at batch indices 0, 31, 63, 64, the last one and the modelled connection 4 are broken after the
    lossy ticks; they stop BAD_STATE in begin and in commit with their state and arena bytes untouched, and every
    other connection equals the host, with resends among the broken ones' wave neighbours."""
    p = ran(lane_lossy)
    B = dict(batch_of(p))
    broken = [0, 31, 63, 64, p.total - 1, 4]
    B["states"] = p.states.copy()
    B["states"]["pkt_cap"][broken] = 3
    r = one_round(p.backend, B, p.total, p.next_ms + 1000)
    ok = np.ones(p.total, dtype=bool)
    ok[broken] = False
    assert (r["begin"]["stop"][broken] == R.BAD_STATE).all() and (r["commit"]["results"]["stop"][broken] == R.BAD_STATE).all()
    assert (r["begin"]["stop"][ok] != R.BAD_STATE).all() and (r["commit"]["results"]["stop"][ok] != R.BAD_STATE).all()
    for c in broken:
        assert r["after_begin"][c].tobytes() == B["states"][c].tobytes() == r["states"][c].tobytes(), c
        assert region_bytes(B["states"], r["arenas"], c) == region_bytes(B["states"], p.arenas, c), c
    assert int(r["begin"]["n_resent"][:128].sum()) > 0 and int(r["commit"]["results"]["heap_pushed"][:128].sum()) > 0


def test_lane_no_data_flush(lane_lossy):
    """16,406 connections (lane form): NO_DATA_FLUSH on every third connection for one tick; those lanes skip the
    resend loop and the staging while their neighbours flush."""
    p = clone(ran(lane_lossy))
    for c in range(p.n):
        p.enqueue(c, 500, 1, E.RELIABLE)
    off = np.array([0, 1, 0, 0, 1, 0], dtype=np.uint32)   # (connection 4 has acks waiting, 2 and 3 resends due)
    p.tick(p.next_ms + 200, 40, 20000, p.next_acks, flags=off)
    flagged = off[p.src[p.active]] == 1
    begin, commit = p.last["begin"][p.active], p.last["commit"][p.active]
    assert flagged[6:].sum() > 80 and not begin["n_resent"][flagged].any() and not commit["frames"][flagged].any()
    assert int(begin["n_resent"][~flagged].sum()) > 0 and int(commit["frames"][~flagged].sum()) > 0
    assert int(begin["packets_freed"][flagged].sum()) + int(begin["refs_acked"][flagged].sum()) > 0   # (acks are still taken)


def tiled(p, reps):
    """The Pipeline's connections reps times over, every copy with arenas and a log of its own, and the ack frames
    the next tick would bring (p.next_acks) already through the host's frame_queue call."""
    n0, n = p.n, p.n * reps
    k = np.repeat(np.arange(reps, dtype=np.uint64), n0)
    states, senders, queues = np.tile(p.states, reps), np.tile(p.senders, reps), np.tile(p.queues, reps)
    for name, key in (("heap", "heap"), ("pkt", "pkts"), ("frag", "frag_acked"), ("tx", "tx"), ("stage", "stage")):
        states[name + "_first"] += k * np.uint64(p.arenas[key].size)
    queues["log_first"] += k * np.uint64(p.log.size)
    arenas = {key: np.tile(v, reps) for key, v in p.arenas.items()}
    tx_size = p.arenas["tx"].size
    log, sent = np.tile(p.log, reps), np.tile(p.sent, reps)   # (their refs lie in the copy's own tx ring)
    log["ref_first"] += np.repeat(np.arange(reps, dtype=np.uint32) * np.uint32(tx_size), p.log.size)
    sent["ref_first"] += np.repeat(np.arange(reps, dtype=np.uint32) * np.uint32(tx_size), p.sent.size)
    sent_first = np.append((p.sent_first[:-1][None, :] + np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(p.sent.size)).reshape(-1),
                           np.uint64(reps * p.sent.size))
    infos, groups, first = [], [], [0]
    for c in range(n0):
        for fw, pw, gs in p.next_acks[c]:
            info = R.Q.ack_info(fw, len(groups), len(gs))
            info["f"][1] = pw
            infos.append(info)
            groups.extend(R.Q.group_item(*g) for g in gs)
        first.append(len(infos))
    assert infos and groups
    infos, groups = np.array(infos, dtype=fr.FRAME_INFO_DTYPE), np.array(groups, dtype=fr.ITEM_DTYPE)
    all_infos = np.tile(infos, reps)
    all_infos["item_first"] += np.repeat(np.arange(reps, dtype=np.uint32) * np.uint32(groups.size), infos.size)
    frame_first = np.append((np.array(first[:-1], dtype=np.uint64)[None, :] +
                             np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(infos.size)).reshape(-1), np.uint64(reps * infos.size))
    now, rtt = p.next_ms, 40
    steps = np.zeros(n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
    steps["flags"] = np.uint32(fr.FQ_FORGET | fr.FQ_HAS_RTT) | np.tile(p.extra, reps)
    steps["rtt_ms"], steps["thresh_ms"], steps["now_ms"] = rtt, max(now - 4 * rtt, 0), now
    res = fr.frame_queue_host(all_infos, np.tile(groups, reps), frame_first, sent, sent_first, queues, steps, log,
                              ref_acked=arenas["ref_acked"], nthreads=8, queues_out=queues)["results"]
    assert (res["stop"] == fr.FQ_DONE).all() and (res["pushes_refused"] == 0).all() and int(res["frames_acked"].sum()) > reps
    return {"states": states, "senders": senders, "queues": queues, "log": log, "arenas": arenas, "extra": np.tile(p.extra, reps),
            "window_room": res["window_room"], "infos": all_infos, "frame_first": frame_first, "now": now}


@pytest.fixture(scope="module")
def switch_batch():
    # (the seed: the first whose state has a marked ref for the last lane of begin's ack propagation, so that a pass
    # over fewer than 64 lanes shows)
    p = R.Pipeline(T.lossy_configs(), R.HostBackend(4))
    R.run_lossy(p, random.Random(6), 20, loss=0.3, traffic=busy_traffic)
    B = tiled(p, 2742)   # 16,452 connections
    assert sum(R.marked_refs_of_lane(B["states"][c], B["arenas"]["ref_acked"]) for c in range(p.n)) > 0
    return B


def switch_pass(be, B, m):
    r = one_round(be, B, m, B["now"], infos=B["infos"], frame_first=B["frame_first"])
    begin, commit = r["begin"], r["commit"]["results"]
    assert int(begin["packets_freed"].sum()) > m // 6 and int(begin["refs_acked"].sum()) > m // 6
    assert int(begin["n_resent"].sum()) > m // 6 and int(commit["heap_pushed"].sum()) > m // 6
    assert (commit["stop"] != R.BAD_STATE).all()
    return r


def test_form_switch_16383_against_16384(engine, switch_batch):
    """The same connections at 16,383 (the last wave-form count: rs_begin_kernel, rs_commit_kernel, DevWave) and at
    16,384 (the first lane-form count: the _lane_ kernels, SerialWave, every block full), with a tick's ack frames so
    that acknowledge runs: each pass equals the host, and the first 16,383 connections come out the same from both."""
    be, B = checked(engine), switch_batch
    a, b = switch_pass(be, B, 16383), switch_pass(be, B, 16384)
    m, last = 16383, B["states"][16383]
    for k in ("begin", "after_begin", "senders", "states"):
        _same(a[k], b[k][:m], "the forms: " + k)
    for k in ("results", "retake", "next_extra_flags"):
        _same(a["commit"][k], b["commit"][k][:m], "the forms: commit " + k)
    _same(a["flush_first"][:m + 1], b["flush_first"][:m + 1], "the forms: flush_first")
    _same(a["commit"]["sent_first"][:m], b["commit"]["sent_first"][:m], "the forms: sent_first")
    _same(a["items"][:int(a["flush_first"][m])], b["items"][:int(a["flush_first"][m])], "the forms: placed items")
    n_sent = int(b["commit"]["sent_first"][m])
    _same(a["commit"]["sent"][:n_sent], b["commit"]["sent"][:n_sent], "the forms: sent")
    for name, key in (("heap", "heap"), ("pkt", "pkts"), ("frag", "frag_acked"), ("tx", "tx"), ("tx", "ref_acked"), ("stage", "stage")):
        x, y = a["arenas"][key], b["arenas"][key]
        if key == "stage":   # (the staged slots alone are in the contract)
            at = _staged(a["states"], a["begin"])
            x, y = x[at], y[at]
        else:
            lo, hi = int(last[name + "_first"]), int(last[name + "_first"]) + int(last[name + "_cap"])
            y[lo:hi] = x[lo:hi]   # (the one connection more that the second pass ran)
        _same(x, y, "the forms: arena " + key)


def test_lane_form_full_last_block(engine, switch_batch):
    """64 x 257 = 16,448 connections: the lane form with its last block full, against the host."""
    switch_pass(checked(engine), switch_batch, 16448)


def test_place_and_the_tick_past_the_launch_grid(engine):
    """66,000 connections, more than the 65,536 blocks a launch gets: rs_place_kernel's blocks stride over the
    connections, and begin and commit run 1,032 lane blocks.  The highest 64 connections are replicas that send a
    Persistent packet in tick 1 and, with no ack and an rtt shorter than two ticks, resend it in tick 3, so that the
    blocks that have strided place items."""
    p = R.Pipeline(T.lossy_configs(), checked(engine), replicas=186, tail_replicas=64, fillers=66000 - 6 - 250)
    assert p.total == 66000 > 65536 + 64 and (p.src[-64:] >= 0).all() and (p.src[256:-64] < 0).all()
    for c in range(p.n):
        p.enqueue(c, 700, 1, E.PERSISTENT)
    sent = p.tick(1000, 40, 1 << 20, [[] for _ in range(p.n)])
    assert all(len(s) == 1 for s in sent) and int(p.last["commit"]["heap_pushed"][-64:].sum()) == 64
    p.tick(1025, 40, 1 << 20, [[] for _ in range(p.n)])
    assert not p.last["begin"]["n_resent"].any()
    sent = p.tick(1050, 40, 1 << 20, [[] for _ in range(p.n)])
    assert all(len(s) == 1 for s in sent)
    begin, first, items = p.last["begin"], p.last["flush_first"], p.last["items"]
    assert (begin["n_resent"][-64:] == 1).all()
    for c in range(p.total - 64, p.total):
        it = items[int(first[c])]
        assert int(first[c + 1]) - int(first[c]) == 1 and int(it["data_len"]) == 700 and int(it["id"]) == p.cfg[p.src[c]].base_id, (c, it)
