"""GPU: the batched flush control (ufc_flush_acks_varlen / ufc_flush_sync_varlen, FrameCrcEngine.flush_acks /
flush_sync) against tests/flush_expect.py and against the host calls, byte for byte on every output: the scenarios
of tests/test_flush_cpu.py with the device calls in the host calls' place; n = 1, 63, 64, 65 and 130 connections;
connections with 63, 64, 65 and 130 merged groups (the copy's lane seam); a carry whose last group sits at lane 63
and at lane 0 of the next tile; the compaction's patterns; separate and in-place outputs; caps one short; 270,000
connections (past the lane kernels' launch grid, and past the 65,536 waves of the writing kernel); the ack frames
through the device build; the wrappers' checks."""
import numpy as np
import pytest
import torch

from uflow_amd import flush as fl, frame as fr
from uflow_amd.batch import records, rows

import flush_expect as E
import pack_expect as P
import test_flush_cpu as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACK_DT = {"merged": fr.ITEM_DTYPE, "infos": fr.FRAME_INFO_DTYPE, "results": fr.FLUSH_RESULT_DTYPE,
          "ack_results": fl.FLUSH_ACKS_RESULT_DTYPE, "windows_out": fr.FRAME_WINDOW_DTYPE, "ctl_out": fl.FLUSH_CTL_DTYPE,
          "carry": fr.ITEM_DTYPE, "flushes": fr.FLUSH_DTYPE, "flags": np.uint32, "merged_first": np.uint64}
SYNC_DT = {"infos": fr.FRAME_INFO_DTYPE, "sync_index": np.uint32, "results": fl.FLUSH_SYNC_RESULT_DTYPE,
           "ctl_out": fl.FLUSH_CTL_DTYPE, "ticks_next": fr.RATE_TICK_DTYPE}


def _up(a):
    return None if a is None else rows(a, DEV)


def _down(d, dts, used):
    out = {k: (None if d[k] is None else records(d[k], dt)) for k, dt in dts.items()}
    for k in used:
        out[k] = int(d[k].cpu()[0])
    return out


def gpu_acks(engine):
    def call(ctl, windows, groups, group_first, receivers, rate, carry, merged_cap, frames_cap, flushes, flags, merged,
             infos, windows_out, ctl_out):
        d_ctl, d_w = _up(ctl), _up(windows)
        d = engine.flush_acks(d_ctl, d_w, _up(groups), _up(group_first), _up(receivers), _up(rate), _up(carry),
                              merged_cap=merged_cap, frames_cap=frames_cap, flushes=_up(flushes), flags=_up(flags),
                              merged=_up(merged), infos=_up(infos), windows_out=d_w if windows_out is windows else None,
                              ctl_out=d_ctl if ctl_out is ctl else None)
        torch.cuda.synchronize()
        o = _down(d, ACK_DT, ("merged_used", "frames_used"))
        if ctl_out is ctl:   # in place: the inputs' tensors took the outputs
            assert d["ctl_out"] is d_ctl and d["windows_out"] is d_w
            ctl[:], windows[:] = o["ctl_out"], o["windows_out"]
        else:
            assert records(d_ctl, fl.FLUSH_CTL_DTYPE).tobytes() == ctl.tobytes()
            assert records(d_w, fr.FRAME_WINDOW_DTYPE).tobytes() == windows.tobytes()
        return o
    return call


def gpu_sync(engine):
    def call(ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders, syncs_cap, ticks_next,
             infos, ctl_out):
        d_ctl = _up(ctl)
        d = engine.flush_sync(d_ctl, _up(rate), _up(ack_results), _up(begin_results), _up(pack_results),
                              _up(commit_results), _up(queues), _up(senders), syncs_cap=syncs_cap,
                              ticks_next=_up(ticks_next), infos=_up(infos), ctl_out=d_ctl if ctl_out is ctl else None)
        torch.cuda.synchronize()
        o = _down(d, SYNC_DT, ("syncs_used",))
        if ctl_out is ctl:
            ctl[:] = o["ctl_out"]
        else:
            assert records(d_ctl, fl.FLUSH_CTL_DTYPE).tobytes() == ctl.tobytes()
        return o
    return call


@pytest.fixture
def on_gpu(engine, monkeypatch):
    monkeypatch.setattr(T, "acks_call", gpu_acks(engine))
    monkeypatch.setattr(T, "sync_call", gpu_sync(engine))


@pytest.mark.parametrize("scenario", [s for s in T.ACK_SCENARIOS if s is not T.scenario_many_connections],
                         ids=lambda f: f.__name__[9:])
def test_ack_scenarios(on_gpu, scenario):
    """The host test's scenarios on the device: the pack equivalence, the carry over three ticks (separate and in-place
    outputs in turn), at its cap and one over, both BAD_STATE cases and the structural ones, seeded connections, caps
    one short and caps of zero."""
    scenario()


@pytest.mark.parametrize("sync_reply", [0, 1])
def test_alloc_and_count_grid(on_gpu, sync_reply):
    T.test_alloc_and_count_grid(sync_reply)


def test_carry_over_two_ticks(on_gpu):
    T.test_carry_over_two_ticks()


@pytest.mark.parametrize("scenario", T.SYNC_SCENARIOS, ids=lambda f: f.__name__[9:])
def test_sync_scenarios(on_gpu, scenario):
    """Every rule at its edge, 1,000 seeded connections, and the compaction: frames from lane 63 alone, from lane 0
    of the second tile alone, from all and from none, at n = 1, 63, 64, 65 and 130; in-place and separate ctl_out;
    syncs_cap one short and zero."""
    scenario()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ack_batches_around_a_tile(on_gpu, n):
    """n seeded connections (the count kernel's tile of 64 lanes), in place and apart."""
    rng = np.random.default_rng(40 + n)
    inp = E.ack_inputs([E.rand_ack_conn(rng) for _ in range(n)])
    T.run_acks(inp, in_place=False)
    T.run_acks(inp, in_place=True)


@pytest.mark.parametrize("merged", [63, 64, 65, 130])
def test_merged_lists_around_the_copy_tile(on_gpu, merged):
    """A connection whose merged list has 63, 64, 65 and 130 groups, 60 of them from the carry, between two small
    ones; sent whole, and with nothing sent, so that the new carry's last group is merged group `merged` - 1: lane 63
    of the first tile at 64, lane 0 of the second at 65.  Then the same into a room one short."""
    all_g = E.seq_groups(merged, start=11)
    carry = all_g[:59] + [(all_g[59][0], 1, all_g[59][2] ^ 1)]
    small = dict(groups=E.seq_groups(2, start=7), alloc=100)
    for alloc, cap in ((1 << 20, 140), (-5, 140), (-5, merged - 1)):
        got, want = T.run_acks(E.ack_inputs([small, dict(carry=carry, groups=all_g[59:], alloc=alloc, carry_cap=cap), small]),
                               in_place=alloc < 0)
        ar = got["ack_results"][1]
        assert ar["merged_count"] == merged and got["results"][1]["items_packed"] == (merged if alloc > 0 else 0)
        if alloc < 0:
            assert ar["carried"] == min(cap, merged) and ar["dropped"] == merged - min(cap, merged)
            c0 = int(got["ctl_out"][1]["carry_first"])
            kept = int(ar["carried"])
            assert [int(g["id"]) for g in got["carry"][c0: c0 + kept]] == [g[0] for g in all_g[merged - kept:]]
            assert int(got["carry"][c0 + kept - 1]["data_offset"]) == all_g[-1][1]   # the tail as the window wrote it


def test_many_connections_equal_the_host_calls(engine):
    """270,000 connections: past the 262,144 lanes of the counting and deciding kernels' launch grids and past the
    65,536 waves of the writing kernel, so that all of them go round again.  Against the host calls."""
    rng = np.random.default_rng(9)
    base = E.ack_inputs([E.rand_ack_conn(rng, max_groups=3) for _ in range(1000)], guard=0, carry_cap=4)
    inp = E.tile_acks(base, 270)
    n = len(inp["ctl"])
    flushes, flags = np.zeros(n, dtype=fr.FLUSH_DTYPE), np.arange(n, dtype=np.uint32)
    h = fl.flush_acks_host(inp["ctl"], inp["windows"], inp["groups"], inp["group_first"], inp["receivers"], inp["rate"],
                           inp["carry"].copy(), flushes=flushes.copy(), flags=flags.copy(), nthreads=8)
    d_ctl = _up(inp["ctl"])
    d = engine.flush_acks(d_ctl, _up(inp["windows"]), _up(inp["groups"]), _up(inp["group_first"]), _up(inp["receivers"]),
                          _up(inp["rate"]), _up(inp["carry"]), flushes=_up(flushes), flags=_up(flags), ctl_out=d_ctl)
    torch.cuda.synchronize()
    o = _down(d, ACK_DT, ("merged_used", "frames_used"))
    assert o["merged_used"] == h["merged_used"] > n // 2 and o["frames_used"] == h["frames_used"] > n // 4
    for k in ACK_DT:
        assert o[k].tobytes() == np.asarray(h[k]).tobytes(), k
    assert (h["ack_results"]["carried"] > 0).sum() > 1000 and (h["results"]["stop"] == P.SIZE_LIMITED).sum() > 1000
    del d, o, h
    s = E.sync_inputs([E.rand_sync_conn(rng) for _ in range(1000)])
    s = {k: np.tile(v, 270) for k, v in s.items()}
    h = fl.flush_sync_host(s["ctl"], s["rate"], s["ack_results"], s["begin_results"], s["pack_results"],
                           s["commit_results"], s["queues"], s["senders"], ticks_next=s["ticks_next"].copy(), nthreads=8)
    d = engine.flush_sync(_up(s["ctl"]), _up(s["rate"]), _up(s["ack_results"]), _up(s["begin_results"]),
                          _up(s["pack_results"]), _up(s["commit_results"]), _up(s["queues"]), _up(s["senders"]),
                          ticks_next=_up(s["ticks_next"]))
    torch.cuda.synchronize()
    o = _down(d, SYNC_DT, ("syncs_used",))
    assert o["syncs_used"] == h["syncs_used"] > n // 20
    for k in SYNC_DT:
        assert o[k].tobytes() == np.asarray(h[k]).tobytes(), k


def test_ack_and_sync_frames_through_the_device_build(engine):
    """The stage's records are what ufc_build_* takes with no step in between: the ack frames over `merged` and the
    sync frames, built and sealed on the device, parse back (on the host) as the frames the model describes."""
    conns = [dict(groups=E.seq_groups(3, start=50), alloc=1 << 20, sync_reply=1, base_id=900, rx_base_id=41),
             dict(groups=[], alloc=20, sync_reply=1, base_id=7, rx_base_id=8),
             dict(groups=E.seq_groups(170, start=9), alloc=1 << 20, base_id=0xFFFFFFFF, rx_base_id=0xFFFFF)]
    inp = E.ack_inputs(conns)
    d = engine.flush_acks(*[_up(inp[k]) for k in ("ctl", "windows", "groups", "group_first", "receivers", "rate", "carry")])
    out, offsets, status = engine.build_varlen(d["infos"], d["merged"], torch.zeros(0, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert int(d["frames_used"].cpu()[0]) == 4
    off, raw = offsets.cpu().numpy(), out.cpu().numpy().tobytes()
    frames = [fr.Frame.read(raw[int(off[k]): int(off[k + 1])]) for k in range(4)]
    assert [(f.frame_window_base_id, f.packet_window_base_id, len(f.frame_acks)) for f in frames] == \
        [(900, 41, 3), (7, 8, 0), (0xFFFFFFFF, 0xFFFFF, 161), (0xFFFFFFFF, 0xFFFFF, 9)]
    assert [(a.base_id, a.bitfield, int(a.nonce)) for a in frames[0].frame_acks] == E.seq_groups(3, start=50)
    assert (off[5:] == off[4]).all() and (status.cpu().numpy()[:4] == 0).all()
    s = E.sync_inputs([dict(next_id=31, window_base_id=499), dict(), dict(keepalive_ms=5)])
    e = engine.flush_sync(*[_up(s[k]) for k in ("ctl", "rate", "ack_results", "begin_results", "pack_results",
                                                 "commit_results", "queues", "senders")])
    out, offsets, status = engine.build_varlen(e["infos"], torch.zeros((0, 24), dtype=torch.uint8, device=DEV),
                                               torch.zeros(0, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    off, raw = offsets.cpu().numpy(), out.cpu().numpy().tobytes()
    assert int(e["syncs_used"].cpu()[0]) == 2 and off.tolist() == [0, 14, 28, 28]
    a, b = fr.Frame.read(raw[:14]), fr.Frame.read(raw[14:28])
    assert (a.next_frame_id, a.next_packet_id, b.next_frame_id, b.next_packet_id) == (500, 31, None, None)
    assert e["sync_index"].cpu().tolist() == [0, -1, 1]


def test_two_streams(engine):
    """Calls on two non-default streams, each with its own scratch."""
    rng = np.random.default_rng(77)
    batches = [E.ack_inputs([E.rand_ack_conn(rng) for _ in range(k)]) for k in (200, 70)]
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    keys = ("ctl", "windows", "groups", "group_first", "receivers", "rate", "carry")
    args = [[_up(b[k]) for k in keys] for b in batches]
    torch.cuda.synchronize()
    outs = [engine.flush_acks(*a, stream=s) for a, s in zip(args, streams)]
    for s in streams:
        s.synchronize()
    for b, d in zip(batches, outs):
        want = E.expect_acks(**b)
        got = _down(d, ACK_DT, ("merged_used", "frames_used"))
        assert got["merged_used"] == want["merged_used"] and got["frames_used"] == want["frames_used"] > 0
        for k in ("merged", "infos", "results", "ack_results", "windows_out", "ctl_out", "carry", "merged_first"):
            assert got[k].tobytes() == want[k].tobytes(), k
    for s in streams:
        engine.release_stream(s)


def test_wrappers_refuse_bad_tensors(engine, monkeypatch):
    """Device, row width and size of every record tensor are checked before the C entry point is reached and before
    any output is allocated."""
    from uflow_amd import _native

    def reached(*a):
        raise AssertionError("the C entry point was reached")
    for sym in ("ufc_flush_acks_varlen", "ufc_flush_sync_varlen"):
        monkeypatch.setattr(_native.lib(), sym, reached)
    inp = E.ack_inputs([dict(groups=E.seq_groups(2), alloc=5)] * 3)
    keys = ("ctl", "windows", "groups", "group_first", "receivers", "rate", "carry")
    s = E.sync_inputs([dict()] * 3)
    skeys = ("ctl", "rate", "ack_results", "begin_results", "pack_results", "commit_results", "queues", "senders", "ticks_next")
    for method, kw in (("flush_acks", {k: _up(inp[k]) for k in keys}), ("flush_sync", {k: _up(s[k]) for k in skeys})):
        torch.cuda.synchronize()
        for k, v in kw.items():
            bads = [v.cpu()] + ([v[:, :-1].contiguous()] if v.dim() == 2 else []) + ([v[:-1]] if k not in ("ctl", "carry", "groups") else [])
            for bad in bads:
                before = torch.cuda.memory_allocated()
                with pytest.raises(ValueError):
                    getattr(engine, method)(**dict(kw, **{k: bad}))
                assert torch.cuda.memory_allocated() == before, (method, k)


# ---- a loop queued on device tensors: window -> ack flush -> sync decision, tick after tick, read back once ----
def loop_traffic(rng, n, ticks, starve):
    """Per tick: the frames every connection receives (data frames in order with gaps, none at all for stretches, a
    sync frame now and then), the rate results (250 ms a tick; flush_alloc generous, or near zero when `starve`) and
    the data flush's upstream results for the sync decision."""
    nxt = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    windows = fr.new_frame_windows(n, 256, 0)
    windows["base_id"] = nxt
    out = []
    for t in range(ticks):
        infos, ff = [], [0]
        for c in range(n):
            quiet = (t // 8 + c) % 3 == 0   # nothing arrives for eight ticks in every 24
            for _ in range(0 if quiet else int(rng.integers(0, 4))):
                nxt[c] += np.uint32(1 + (40 if rng.integers(0, 5) == 0 else 0))
                infos.append(E.W.data_info(int(nxt[c]), int(rng.integers(0, 2))))
            if rng.integers(0, 12) == 0:
                infos.append(E.W.sync_info(int(nxt[c]) + 1 if rng.integers(0, 2) else None, None))
            ff.append(len(infos))
        s = E.sync_inputs([dict(now_ms=1000 + 250 * t, rto_ms=600, log_next_id=500 + c, window_base_id=500 + c - (c & 1),
                                base_id=30, next_id=30 + ((c >> 1) & 1), heap_len=int(c % 16 == 6),
                                frame_count=int(rng.integers(0, 10) == 0), alloc_left=int(rng.integers(-1, 3)) * 50)
                           for c in range(n)])
        s["rate"]["flush_alloc"] = rng.integers(-10, 40, n) if starve else rng.integers(0, 4000, n)
        out.append({"infos": np.array(infos, dtype=fr.FRAME_INFO_DTYPE) if infos else np.zeros(0, fr.FRAME_INFO_DTYPE),
                    "frame_first": np.array(ff, dtype=np.uint64), **{k: s[k] for k in
                    ("rate", "begin_results", "pack_results", "commit_results", "queues", "senders", "ticks_next")}})
    return windows, out


def run_loop(engine, starve, n=130, ticks=40, carry_cap=6):
    rng = np.random.default_rng(5 + starve)
    windows, traffic = loop_traffic(rng, n, ticks, starve)
    ctl, carry = fl.new_flush_ctl(n, 5000, carry_cap)
    receivers = fr.new_receivers(n, 8, base_id=3)
    cap = n + max(tr["infos"].size for tr in traffic) + carry.size
    # the model, tick for tick
    m_w, m_ctl, m_carry = windows.copy(), ctl.copy(), carry.copy()
    want, facts = [], dict(dud=0, carried=0, dropped=0, size_limited=0, frames=0, modes=[0] * 4, sync_idle=0)
    for tr in traffic:
        w = E.W.expect_batch(tr["infos"], tr["frame_first"], m_w, groups_cap=cap)
        a = E.expect_acks(m_ctl, w["windows_out"], w["groups"], w["group_first"], receivers, tr["rate"], m_carry,
                          merged_cap=cap, frames_cap=cap)
        s = E.expect_sync(a["ctl_out"], tr["rate"], a["results"], tr["begin_results"], tr["pack_results"],
                          tr["commit_results"], tr["queues"], tr["senders"], ticks_next=tr["ticks_next"])
        m_w, m_ctl, m_carry = a["windows_out"], s["ctl_out"], a["carry"]
        assert a["facts"]["bad_state"] == 0
        want.append((w, a, s))
        for k in ("dud", "carried", "dropped", "size_limited", "frames"):
            facts[k] += a["facts"][k]
        facts["modes"] = [x + y for x, y in zip(facts["modes"], s["facts"]["modes"])]
        facts["sync_idle"] += s["facts"]["reasons"][E.FS_IDLE]
    assert facts["dud"] > 20 and facts["frames"] > 500 and all(facts["modes"]) and facts["sync_idle"] > 100, facts
    if starve:
        assert facts["carried"] > 1000 and facts["dropped"] > 10 and facts["size_limited"] > 1000, facts
    # the device: everything uploaded first, three calls a tick queued, one synchronize, one read back
    up = [{k: rows(v, DEV) for k, v in tr.items()} for tr in traffic]
    d_w, d_ctl, d_carry, d_rx = rows(windows, DEV), rows(ctl, DEV), rows(carry, DEV), rows(receivers, DEV)
    keep = []
    torch.cuda.synchronize()
    for u in up:
        w = engine.frame_window(u["infos"], u["frame_first"], d_w, groups_cap=cap, windows_out=d_w)
        a = engine.flush_acks(d_ctl, d_w, w["groups"], w["group_first"], d_rx, u["rate"], d_carry, merged_cap=cap,
                              frames_cap=cap, windows_out=d_w, ctl_out=d_ctl)
        s = engine.flush_sync(d_ctl, u["rate"], a["results"], u["begin_results"], u["pack_results"], u["commit_results"],
                              u["queues"], u["senders"], ticks_next=u["ticks_next"], ctl_out=d_ctl)
        keep.append((a, s))
    torch.cuda.synchronize()
    for t, ((a, s), (_, wa, ws)) in enumerate(zip(keep, want)):
        for k in ("merged", "infos", "results", "ack_results", "merged_first"):
            assert records(a[k], ACK_DT[k]).tobytes() == wa[k].tobytes(), (t, k)
        for k in ("infos", "sync_index", "results", "ticks_next"):
            assert records(s[k], SYNC_DT[k]).tobytes() == ws[k].tobytes(), (t, k)
    assert records(d_w, fr.FRAME_WINDOW_DTYPE).tobytes() == m_w.tobytes()
    assert records(d_ctl, fl.FLUSH_CTL_DTYPE).tobytes() == m_ctl.tobytes()
    assert records(d_carry, fr.ITEM_DTYPE).tobytes() == m_carry.tobytes()


def test_loop_on_the_device(engine):
    """130 connections, 40 ticks of frame_window -> flush_acks -> flush_sync on device tensors only, the windows, the
    control records and the carry rooms updated in place, nothing read back before the end: every tick's ack frames,
    merged groups, results, sync frames and alloc_adjust, and the final states, equal the model run tick for tick.
    On the model's side: sync frames answered with dud acks, sync frames of all four modes (the keepalive among
    them), idle stretches.  (The receive side and the sync decision of a connection; the data flush's results are
    given.  A loop of two whole peers through every stage of the tick is not part of this test.)"""
    run_loop(engine, starve=0)


def test_loop_on_the_device_starved(engine):
    """The same loop with flush_alloc held between -10 and 39: most ticks send one group or none, groups are carried
    from tick to tick in rooms of 2, and some outgrow them."""
    run_loop(engine, starve=1, carry_cap=2)


# ---- two whole peers, every call of the full-duplex tick queued on device tensors, read back once ----
class Peer:
    """One end of a connection with every stage's state on the device: the sender's side (rate, frame queue, resend,
    packet emit, pack, build), the receiver's side (gate, parse, frame window, packet receive) and the flush control
    between them.  tick(t, incoming) queues the whole tick and returns what goes on the wire: three batches (ack
    frames, data frames, the sync frame) with their CSR offsets.  Nothing is read back; what the flush control's two
    calls and the window call took and gave is kept (clones, on the device) for the comparison with the model."""
    W, GC, FC, IC = 16, 40, 40, 80   # packet window; caps of ack groups / frames, data frames, items

    def __init__(self, engine, rng, sizes, modes, base, fbase, peer_base, peer_fbase, ticks, budget, keepalive_ms, carry_cap):
        import ctypes
        self.e, self.ct = engine, ctypes
        n, per = 1, len(sizes)
        self.per = per
        packets = np.zeros(per, dtype=fr.PACKET_DTYPE)
        packets["data_len"], packets["data_offset"] = sizes, np.concatenate([[0], np.cumsum(sizes)[:-1]])
        packets["mode"] = modes
        self.payload = rows(rng.integers(0, 256, max(int(np.sum(sizes)), 1), dtype=np.uint8), DEV)
        senders = np.zeros(n, dtype=fr.SENDER_DTYPE)
        senders["base_id"] = senders["next_id"] = base
        senders["window_size"], senders["max_alloc"] = self.W, 64 * 1448
        senders["window_parent_id"], senders["channel_parent_id"] = fr.NO_PARENT, fr.NO_PARENT
        queues, log = fr.new_frame_queues(n, 16, 16, fbase)
        states, arenas = fr.new_resend_states(n, self.W, 64 * 1448, 16, 16, heap_cap=64, stage_cap=self.IC)
        rstates, entries = fr.new_rate_states(n, 0xFFFFFFFF, 32)
        ctl, carry = fl.new_flush_ctl(n, keepalive_ms, carry_cap)
        self.host = {"base": base, "fbase": fbase}
        self.d = {k: rows(v, DEV) for k, v in (
            ("packets", packets), ("senders", senders), ("queues", queues), ("log", log), ("states", states),
            ("rstates", rstates), ("entries", entries), ("windows", fr.new_frame_windows(n, 4096, peer_fbase)),
            ("receivers", fr.new_receivers(n, self.W, peer_base, 64 * 1448)), ("ctl", ctl), ("carry", carry))}
        self.A = {k: rows(v, DEV) for k, v in arenas.items()}
        z = self.z
        self.pf = rows(np.array([0, per], dtype=np.uint64), DEV)
        self.local = torch.arange(per, device=DEV)
        self.flushes = rows(np.zeros(n, dtype=fr.FLUSH_DTYPE), DEV)
        self.flushes[:, 8:12] = rows(np.array([fr.DATA], dtype=np.uint32), DEV).view(torch.uint8)
        self.budget = torch.from_numpy(np.asarray(budget, dtype=np.int64)).to(DEV).view(torch.uint8).reshape(ticks, 1, 8)
        self.flags, self.extra = z(n, dtype=torch.int32), z(n, dtype=torch.int32)
        self.idx = torch.arange(n, dtype=torch.int32, device=DEV)
        self.slots, self.slot_first = self.zrec(n * self.W, fr.RX_SLOT_DTYPE), rows(np.array([0, self.W], dtype=np.uint64), DEV)
        self.rx_carry = [z(1 << 16), z(1 << 16)]
        self.sent, self.sent_first = self.zrec(self.FC, fr.SENT_FRAME_DTYPE), z(n + 1, dtype=torch.int64)
        self.fres = self.zrec(n, fr.FLUSH_RESULT_DTYPE)
        self.nonce = torch.from_numpy(rng.integers(0, 1 << 31, self.FC // 32 + 2).astype(np.int32)).to(DEV)
        tk = np.zeros((ticks + 1, n), dtype=fr.RATE_TICK_DTYPE)
        tk["now_ms"], tk["delta_time_s"] = (1000 + 250 * np.arange(ticks + 1))[:, None], 0.25
        self.ticks = rows(tk.reshape(-1), DEV).reshape(ticks + 1, n, -1)
        self.now = torch.from_numpy(tk["now_ms"].astype(np.int64)).to(DEV)
        self.NF = self.GC + self.FC + 1
        self.ff = rows(np.array([0, self.NF], dtype=np.uint64), DEV)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.kept = []

    @staticmethod
    def z(*shape, dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype, device=DEV)

    def zrec(self, count, dt):
        return self.z(count, dt.itemsize)

    def build(self, infos, items, pay, offsets, count):
        from uflow_amd._native import lib, check
        P = lambda t: self.ct.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
        out = self.z(count * 1472)
        check(lib().ufc_build_batch_varlen(self.e._ctx, P(infos), P(items), items.shape[0], None, P(pay), pay.numel(), count,
                                           P(offsets), P(out), out.numel(), 1, None, self.st), "build")
        return out

    def silence(self):
        """What arrives when the peer has sent nothing yet."""
        return [(self.z(256), self.z(c + 1, dtype=torch.int64), self.z(c)) for c in (self.GC, self.FC, 1)]

    def tick(self, t, incoming):
        e, d, A, i32 = self.e, self.d, self.A, (lambda x: x.view(torch.int32))
        GC, FC, IC, NF = self.GC, self.FC, self.IC, self.NF
        # ---- what arrived: three batches gated and parsed, then one frame range (byte moves: the item indices of the
        # second batch, the frames' places in the joined bytes) ----
        parsed, at_item, at_byte, src = [], 0, 0, []
        for (wire, off, keep), cap, icap in zip(incoming, (GC, FC, 1), (GC, IC, 1)):
            _, valid = e.crc_varlen(wire, off)
            valid &= keep
            infos, items, _ = e.parse_varlen(wire, off, valid, items_cap=icap)
            i32(infos)[:, 7] += at_item
            parsed.append((infos, items))
            src.append(off[:cap] + at_byte)
            at_item, at_byte = at_item + icap, at_byte + wire.numel()
        infos = torch.cat([p[0] for p in parsed]).contiguous()
        items = torch.cat([p[1] for p in parsed]).contiguous()
        wire = torch.cat([w for w, _, _ in incoming]).contiguous()
        src = torch.cat(src).contiguous()
        # ---- the receiver's side ----
        w_before = d["windows"].clone()
        fw = e.frame_window(infos, self.ff, d["windows"], groups_cap=GC, windows_out=d["windows"])
        first_sync = i32(fw["results"])[:, 6].to(torch.int64)          # first_packet_sync, -1: none
        f1 = i32(infos)[first_sync.clamp(min=0), 2]                     # its next_packet_id
        i32(d["receivers"])[:, 4] = torch.where(first_sync >= 0, f1, torch.full_like(f1, -1))   # resync_id
        rx_before = d["receivers"][:, 0:4].clone()
        rx = e.receive_packets(infos, items, wire, self.ff, d["receivers"], self.slots, self.slot_first, self.rx_carry[t % 2],
                               src_base=src, frame_accept=fw["frame_accept"], carry_out=self.rx_carry[1 - t % 2],
                               out_bytes=self.z(1 << 16), packets=self.zrec(16, fr.RX_PACKET_DTYPE),
                               receivers_out=d["receivers"], want_item_status=False)
        # ---- the sender's side: the tick opens ----
        steps = e.rate_begin(d["rstates"], self.now[t].contiguous(), self.extra, states_out=d["rstates"])["steps"]
        fq = e.frame_queue(infos, items, self.ff, self.sent, self.sent_first, d["queues"], steps, d["log"], A["ref_acked"],
                           queues_out=d["queues"])["results"]
        tick_in = self.ticks[t].clone()
        rate = e.rate_step(d["rstates"], self.ticks[t], fq, d["entries"], flush_results=self.fres, result_index=self.idx,
                           flushes=self.flushes, flush_index=self.idx, states_out=d["rstates"])["results"]
        rate_alloc = rate[:, 32:40].clone()
        rate[:, 32:40] = self.budget[t]                   # a fixed allocation in place of TFRC's ramp
        self.flushes[:, 12:16] = fq[:, 52:56]             # window_room
        self.flushes[:, 16:20] = d["queues"][:, 4:8]      # id0 = log_next_id
        # ---- the ack flush ----
        a_in = {k: v.clone() for k, v in (("ctl", d["ctl"]), ("windows", d["windows"]), ("groups", fw["groups"]),
                                         ("group_first", fw["group_first"]), ("receivers", d["receivers"]), ("rate", rate),
                                         ("carry", d["carry"]), ("flushes", self.flushes), ("flags", self.flags))}
        a = e.flush_acks(d["ctl"], d["windows"], fw["groups"], fw["group_first"], d["receivers"], rate, d["carry"],
                         merged_cap=GC, frames_cap=GC, flushes=self.flushes, flags=self.flags, windows_out=d["windows"],
                         ctl_out=d["ctl"])
        a_out = {k: a[k].clone() for k in ("merged", "merged_first", "infos", "results", "ack_results", "windows_out",
                                           "ctl_out", "carry", "flushes", "flags")}
        a_off, _ = e.build_sizes_varlen(a["infos"], a["merged"], 0)
        a_wire = self.build(a["infos"], a["merged"], self.z(0), a_off, GC)
        # ---- the data flush (the eleven-call tick's calls 4 to 11) ----
        i32(d["senders"])[:, 3] = t + 1
        i32(d["senders"])[:, 9] = -1
        i32(d["senders"])[:, 10] = 0
        br = e.resend_begin(infos, self.ff, d["queues"], d["log"], rate, self.flushes, d["states"], d["senders"], A,
                            flags=self.flags, states_out=d["states"], senders_out=d["senders"])["results"]
        its, flush_first, pres, sres, _, _ = e.emit_packets(d["packets"], self.pf, d["senders"], IC)
        e.resend_place(d["states"], br, A, flush_first, its)
        dinfos, self.fres, frames_used = e.pack_flushes(its, flush_first, self.flushes, frames_cap=FC, nonce_bits=self.nonce)
        d_off, _ = e.build_sizes_varlen(dinfos, its, self.payload.numel())
        cm = e.resend_commit(self.fres, dinfos, d_off, frames_used, its, flush_first, d["packets"], self.pf, pres, sres, br,
                             rate, d["states"], d["senders"], A, next_extra_flags=self.extra, states_out=d["states"])
        self.sent, self.sent_first = cm["sent"], cm["sent_first"]
        out2 = e.emit_packets(d["packets"], self.pf, cm["retake"], 0, senders_out=d["senders"])
        stale = self.local < i32(out2[3])[:, 2].to(torch.int64)[0]       # the consumed packets are not sent again
        d["packets"][:, 13] = torch.where(stale, torch.zeros_like(d["packets"][:, 13]), d["packets"][:, 13])
        d["packets"][:, 8:12] = torch.where(stale[:, None], torch.full_like(d["packets"][:, 8:12], 255), d["packets"][:, 8:12])
        d_wire = self.build(dinfos, its, self.payload, d_off, FC)
        # ---- the sync frame; its 14 bytes go into the next tick's rate step ----
        s_in = {k: v.clone() for k, v in (("ctl", d["ctl"]), ("rate", rate), ("ack_results", a["results"]), ("begin_results", br),
                                         ("pack_results", self.fres), ("commit_results", cm["results"]),
                                         ("queues", d["queues"]), ("senders", d["senders"]), ("ticks_next", self.ticks[t + 1]))}
        s = e.flush_sync(d["ctl"], rate, a["results"], br, self.fres, cm["results"], d["queues"], d["senders"], syncs_cap=1,
                         ticks_next=self.ticks[t + 1], ctl_out=d["ctl"])
        s_out = {k: s[k].clone() for k in ("infos", "sync_index", "results", "ctl_out", "ticks_next")}
        s_off, _ = e.build_sizes_varlen(s["infos"], self.zrec(0, fr.ITEM_DTYPE), 0)
        s_wire = self.build(s["infos"], self.zrec(0, fr.ITEM_DTYPE), self.z(0), s_off, 1)
        self.kept.append({"a_in": a_in, "a_out": a_out, "a_used": (a["merged_used"], a["frames_used"]), "s_in": s_in,
                          "s_out": s_out, "s_used": s["syncs_used"], "w_before": w_before, "w_infos": infos,
                          "w_out": {k: fw[k].clone() for k in ("groups", "group_first", "results", "frame_accept")},
                          "w_after": a_in["windows"], "rx_before": rx_before, "rx_after": d["receivers"][:, 0:4].clone(),
                          "rx_results": rx["results"], "tick_in": tick_in, "rate_alloc": rate_alloc,
                          "senders": d["senders"][:, 0:8].clone(), "begin": br, "fq": fq})
        return [(a_wire, a_off, None), (d_wire, d_off, None), (s_wire, s_off, None)]


def _link(out, keep):
    return [(w, o, k) for (w, o, _), k in zip(out, keep)]


def run_two_peers(engine, starve, ticks=44):
    """A and B for `ticks` ticks of 250 ms.  Returns per peer and tick what the flush control's calls and the window call
    took and gave (host arrays), after every one was compared with the model."""
    rng = np.random.default_rng(3 + starve)
    ones = lambda k: torch.ones(k, dtype=torch.uint8, device=DEV)   # noqa: E731
    n_a = 12 if starve else 3
    b_budget = [4000] + [-1] * 15 + [4000] * (ticks - 16) if starve else [4000] * ticks
    A = Peer(engine, rng, [1448] * n_a, [fr.SEND_UNRELIABLE] * n_a, 0xFFFFE, 0xFFFFFFFE, 7, 3, ticks, [4000] * ticks, 3000, 4)
    B = Peer(engine, rng, [5], [fr.SEND_UNRELIABLE], 7, 3, 0xFFFFE, 0xFFFFFFFE, ticks, b_budget, 3000, 2 if starve else 4)
    GC, FC = Peer.GC, Peer.FC
    from_b = B.silence()
    torch.cuda.synchronize()
    for t in range(ticks):
        out_a = A.tick(t, from_b)
        # the link A -> B loses A's third data frame of the first tick (B's window and receiver fall behind)
        keep_d = ones(FC)
        if t == 0:
            keep_d[2] = 0
        out_b = B.tick(t, _link(out_a, (ones(GC), keep_d, ones(1))))
        # the link B -> A loses every ack frame of the first eight ticks
        from_b = _link(out_b, (ones(GC) * (0 if t < 8 else 1), ones(FC), ones(1)))
    torch.cuda.synchronize()
    # ---- read back, once; the model, tick for tick, on what each call took ----
    traces = []
    for P in (A, B):
        trace = []
        for t, k in enumerate(P.kept):
            a_in = {n_: records(v, dt) for (n_, v), dt in zip(k["a_in"].items(), (
                fl.FLUSH_CTL_DTYPE, fr.FRAME_WINDOW_DTYPE, fr.ITEM_DTYPE, np.uint64, fr.RECEIVER_DTYPE, fr.RATE_RESULT_DTYPE,
                fr.ITEM_DTYPE, fr.FLUSH_DTYPE, np.uint32))}
            want = E.expect_acks(**a_in, merged_cap=GC, frames_cap=GC)
            got = _down(k["a_out"], ACK_DT, ())
            assert int(k["a_used"][0].cpu()[0]) == want["merged_used"] and int(k["a_used"][1].cpu()[0]) == want["frames_used"], t
            for key in ACK_DT:
                assert got[key].tobytes() == want[key].tobytes(), (t, key)
            s_dt = (fl.FLUSH_CTL_DTYPE, fr.RATE_RESULT_DTYPE, fr.FLUSH_RESULT_DTYPE, fr.RESEND_RESULT_DTYPE, fr.FLUSH_RESULT_DTYPE,
                    fr.RESEND_COMMIT_RESULT_DTYPE, fr.FRAME_QUEUE_DTYPE, fr.SENDER_DTYPE, fr.RATE_TICK_DTYPE)
            s_in = {n_: records(v, dt) for (n_, v), dt in zip(k["s_in"].items(), s_dt)}
            swant = E.expect_sync(**s_in, syncs_cap=1)
            sgot = _down(k["s_out"], SYNC_DT, ())
            assert int(k["s_used"].cpu()[0]) == swant["syncs_used"], t
            for key in SYNC_DT:
                assert sgot[key].tobytes() == swant[key].tobytes(), (t, key)
            winfos = records(k["w_infos"], fr.FRAME_INFO_DTYPE)
            wwant = E.W.expect_batch(winfos, np.array([0, winfos.size], dtype=np.uint64),
                                     records(k["w_before"], fr.FRAME_WINDOW_DTYPE), groups_cap=GC)
            assert records(k["w_out"]["groups"], fr.ITEM_DTYPE).tobytes() == wwant["groups"].tobytes(), t
            assert records(k["w_after"], fr.FRAME_WINDOW_DTYPE).tobytes() == wwant["windows_out"].tobytes(), t
            # the calls feed each other: the ack flush's flush_alloc is the data flush's, its flag is begin's, and the
            # sync frame's bytes are in the next rate step's accounting
            tick_in = records(k["tick_in"], fr.RATE_TICK_DTYPE)
            if t:
                assert int(tick_in["alloc_adjust"][0]) == (-14 if trace[-1]["sync"]["results"]["sent"][0] else 0), t
            begin = records(k["begin"], fr.RESEND_RESULT_DTYPE)
            trace.append({"acks": want, "sync": swant, "window": wwant, "rx_before": records(k["rx_before"], np.uint32),
                          "rx_after": records(k["rx_after"], np.uint32), "senders": records(k["senders"], np.uint32),
                          "begin": begin, "fq": records(k["fq"], fr.FRAME_QUEUE_RESULT_DTYPE),
                          "rate_alloc": records(k["rate_alloc"], np.int64), "tick_in": tick_in,
                          "rx_results": records(k["rx_results"], fr.RECEIVER_RESULT_DTYPE),
                          "rto_ms": int(s_in["rate"]["rto_ms"][0])})
        traces.append(trace)
    return traces


def test_two_peers_on_the_device(engine):
    """Two whole peers, 44 ticks, every call of both full-duplex ticks queued on device tensors and read back once:
    gate -> parse -> frame_window -> receive_packets | rate_begin -> frame_queue -> rate_step -> flush_acks -> build |
    resend_begin -> emit -> place -> pack -> sizes -> commit -> emit -> build | flush_sync -> build, each peer's three
    batches of frames the other's input.  A sends three unreliable packets in three frames and goes idle; the third
    frame is lost; B's acks are lost for eight ticks.  The flush control's two calls and the window call equal their
    models tick for tick on what the pipeline handed them, and on the models' side: A's sync frame carries both ids;
    B's window moves on it and B's receiver resynchronizes to A's next_id; B answers with a dud ack in the same tick;
    that ack empties A's windows; A's keepalive sync goes out once 3000 ms and the timeout have passed, and B duds again.  (flush_alloc is a
    fixed 4,000 bytes a tick in the rate step's result, as in test_gpu_resend.py's end-to-end loop, so that the test
    does not wait on TFRC's ramp; the rate step runs and takes the sync frames' alloc_adjust.)"""
    ta, tb = run_two_peers(engine, starve=0)
    modes = [int(x["sync"]["results"]["mode"][0]) if x["sync"]["results"]["sent"][0] else None for x in ta]
    both = modes.index(3)
    assert both == 8 and all(m is None for m in modes[:both])           # 2000 ms after the data frames of tick 0
    assert ta[0]["acks"]["facts"]["frames"] == 0 and tb[0]["acks"]["facts"]["frames"] == 1
    # B, the same tick: the window moves to A's next frame id, the receiver to A's next packet id, a dud ack answers
    assert tb[both]["window"]["facts"]["sync_moved"] == 1 and tb[both]["window"]["results"]["packet_syncs"][0] == 1
    assert int(tb[both]["rx_before"][0]) != int(tb[both]["rx_after"][0]) == (0xFFFFE + 3) & 0xFFFFF
    f = tb[both]["acks"]["facts"]
    assert f["dud"] == 1 and f["dud_empty"] == 1 and tb[both]["acks"]["merged_used"] == 0
    assert tb[both]["acks"]["windows_out"]["sync_reply"][0] == 0
    # A, the next tick: the dud ack frees the packets and empties the frame window; nothing is outstanding
    assert int(ta[both]["senders"][0]) != int(ta[both]["senders"][1])
    assert int(ta[both + 1]["senders"][0]) == int(ta[both + 1]["senders"][1]) == (0xFFFFE + 3) & 0xFFFFF
    assert ta[both + 1]["begin"]["packets_freed"][0] == 3
    # the sync frame's 14 bytes reach the next rate step
    assert int(ta[both + 1]["tick_in"]["alloc_adjust"][0]) == -14 and int(ta[both]["tick_in"]["alloc_adjust"][0]) == 0
    # A's keepalive: no ids; the first tick at which both the keepalive interval of 3000 ms and the sync timeout
    # max(rto_ms, 2000) have passed since the sync frame (the acks that took eight ticks have stretched rto_ms), and
    # B answers with a dud again
    later = modes.index(0, both + 1)
    due = [t for t in range(both + 1, len(ta)) if 250 * (t - both) >= max(ta[t]["rto_ms"], 3000)]
    assert later == due[0] >= both + 12 and tb[later]["acks"]["facts"]["dud_empty"] == 1
    assert all(m is None for m in modes[both + 1: later])


def test_two_peers_on_the_device_starved(engine):
    """The same loop with twelve packets from A and B's flush_alloc held at -1 for fifteen ticks: B's ack flushes stop
    SIZE_LIMITED, its groups are carried from tick to tick, UFC_RS_NO_DATA_FLUSH reaches B's resend_begin (which stages
    nothing), and when the allocation returns the carried groups go out."""
    ta, tb = run_two_peers(engine, starve=1)
    lim = [t for t, x in enumerate(tb) if x["acks"]["facts"]["size_limited"]]
    assert lim == list(range(1, 16))
    assert sum(x["acks"]["facts"]["carried"] for x in tb) >= 5 and tb[15]["acks"]["ctl_out"]["carry_count"][0] >= 1
    assert all(int(tb[t]["acks"]["flags"][0]) & 1 for t in lim) and not int(tb[16]["acks"]["flags"][0]) & 1
    assert tb[16]["acks"]["facts"]["frames"] >= 1 and tb[16]["acks"]["ctl_out"]["carry_count"][0] == 0
    assert sum(x["acks"]["facts"]["frames"] for x in tb[1:16]) == 0
