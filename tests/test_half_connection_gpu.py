"""GPU: the reference's own HalfConnection tests (tests/golden/half_connection_cases.json) replayed through the device
calls by tests/half_tick.py, every call of a tick queued on device tensors and read back once a tick: the mixed batch
of 130 connections of tests/test_half_connection_cpu.py (a wave a connection), the same cases inside a batch of 16,390
connections (past kRsLaneFrom = 16,384: the resend calls give a connection a lane), the first 40 iterations of
packet_unambiguity, and sync_frame_window_only's 4,096 frames in one flush between two small connections.  What is
expected comes from the reference's assert lines and the idle rule alone; nothing here reads the reference."""
import time

import pytest

import half_tick as H
import test_half_connection_cpu as T

pytestmark = pytest.mark.gpu

LANE_FROM = 16384   # kRsLaneFrom (uflow_amd/csrc/resend.hip)


def counted(scenario):
    """The frames a scenario's `expect` blocks count."""
    return sum(em["expect"]["count"] for _, em in scenario.ticks)


def run(engine, assign, what):
    t0 = time.perf_counter()
    d = H.HalfTick(assign, H.DeviceCalls(engine)).run()
    print(f"{what}: {d.n} connections, {d.t} ticks, {d.frames_total} frames, {time.perf_counter() - t0:.2f} s")
    return d


@pytest.mark.parametrize("rotate", [0, 9])
def test_mixed_batch_of_130(engine, rotate):
    """The batch the host test runs, on the device: 130 connections, connection c running case (c + rotate) % 11, the
    groups of 11 staggered by 0, 1 and 2 ticks, so that one launch of every stage holds connections at different step
    indices and with different clocks.  resend_timing's 23 ticks and the stagger.  Indices 63 and 64 hold
    sync_response and resend_timing, and rotated by 9 sync_frame_window_only (4,096 frames in one flush) and
    sync_packet_window_only; the host test runs all eleven rotations."""
    assign = T.mixed_assignment(rotate=rotate)
    assert [assign[c][0].name for c in (63, 64)] == (["sync_response", "resend_timing"] if rotate == 0 else
                                                     ["sync_frame_window_only", "sync_packet_window_only"])
    d = run(engine, assign, f"mixed batch, rotated by {rotate}")
    assert d.t == 23 + 2 and d.frames_total == sum(counted(k.sc) for k in d.conns)


def test_cases_inside_16390_connections(engine):
    """16,390 connections, so that the resend calls take their lane form: one replica of each of the 11 cases at
    indices 0-10, one at 53-63, one at 64-74 (63 and 64 are each a live case) and one at the last 11 indices, staggered;
    every other connection is an idle filler with the smallest rooms.  Fillers emit nothing; replicas meet their
    `expect`."""
    n = LANE_FROM + 6
    assign = [(None, 0)] * n
    for base, start in ((0, 0), (53, 1), (64, 2), (n - 11, 1)):
        for j, name in enumerate(T.MIXED):
            assign[base + j] = (H.Scenario(T.CASES[name]), start)
    assert assign[63][0].name == T.MIXED[10] and assign[64][0].name == T.MIXED[0] and assign[n - 1][0] is not None
    d = run(engine, assign, "lane form")
    assert d.n >= LANE_FROM and len(d.conns) == 44 and d.frames_total == sum(counted(k.sc) for k in d.conns)


def test_packet_unambiguity_first_40_iterations(engine):
    """The loop's first 40 iterations, alone: one frame of 127 datagrams with consecutive ids every iteration, the ack
    built from the emitted frame's sequence id and the running datagram count.  (All 8192 iterations: the host test.)"""
    d = run(engine, [(H.Scenario(T.CASES["packet_unambiguity"], repeat_limit=40), 0)], "packet_unambiguity")
    assert d.conns[0].datagrams_seen == 40 * 127 and d.frames_total == 40


def test_sync_frame_window_only_between_two_small(engine):
    """The one case with 4,096 frames from one connection in one flush, between two small connections."""
    assign = [(H.Scenario(T.CASES[name]), 0) for name in ("no_resend_after_ack", "sync_frame_window_only", "keepalive_timing")]
    d = run(engine, assign, "sync_frame_window_only")
    assert d.frames_total == sum(counted(k.sc) for k in d.conns) > 4096
