"""The reference's twelve deterministic HalfConnection tests (src/half_connection/mod.rs:633-1038), transcribed as data
in tests/golden/half_connection_cases.json, replayed through the batched host calls by tests/half_tick.py: every case
alone, and the mixed batch of 130 connections that tests/test_half_connection_gpu.py runs on the device.  What is
expected comes from the reference's own assert lines and from no model of this repository.  No GPU here."""
import os
import re
import time

import pytest

import half_tick as H

DOC, CASES = H.load_cases()
NAMES = [c["name"] for c in DOC["cases"]]
MIXED = [n for n in NAMES if n != "packet_unambiguity"]


def reference_source():
    """Where the reference's mod.rs is when its sources are at hand: under $UFLOW_REFERENCE, else under the
    reference_path that BASELINE.json records."""
    import json
    root = os.environ.get("UFLOW_REFERENCE")
    if not root:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "BASELINE.json")) as f:
            root = json.load(f).get("reference_path", "")
    return os.path.join(root, *DOC["source"].split("/"))


def test_fixture_is_the_twelve_tests_as_data():
    """Twelve cases with a line range each, the apparatus config, and only the step kinds the note names; every
    emit_frames step has a count with its line; resend_timing is unrolled (2 + 7 * 3 emits); packet_unambiguity's loop
    is a repeat count of 8192; the two values taken from earlier outputs are references, not numbers."""
    assert len(NAMES) == 12 == len(set(NAMES)) and "transcription" in DOC["note"]
    cfg = DOC["config"]
    assert (cfg["tx_frame_window_size"], cfg["rx_frame_window_size"], cfg["tx_packet_window_size"],
            cfg["rx_packet_window_size"], cfg["keepalive_interval_ms"]) == (4096, 4096, 4096, 4096, 5000)
    assert cfg["tx_alloc_limit"] == cfg["rx_alloc_limit"] == 1448 * 4096
    assert all(cfg[k] == 0 for k in ("tx_frame_base_id", "rx_frame_base_id", "tx_packet_base_id", "rx_packet_base_id"))
    kinds = {"enqueue", "set_flush_id", "receive_ack", "receive_sync", "acknowledge_packet_base_id",
             "acknowledge_frame_group", "emit_frames", "repeat"}

    def walk(steps):
        for s in steps:
            assert s["op"] in kinds and isinstance(s["line"], int)
            if s["op"] == "repeat":
                walk(s["steps"])
            if s["op"] == "emit_frames":
                assert isinstance(s["expect"]["count"], int) and isinstance(s["expect"]["count_line"], int)
    for c in DOC["cases"]:
        assert len(c["lines"]) == 2 and c["lines"][0] < c["lines"][1]
        walk(c["steps"])
    assert [s["op"] for s in CASES["resend_timing"]["steps"]].count("emit_frames") == 2 + 7 * 3
    rep = CASES["packet_unambiguity"]["steps"][0]
    assert rep["op"] == "repeat" and rep["count"] == 8192
    assert 8192 * 127 < DOC["constants"]["PACKET_ID_SPAN"]
    assert isinstance(rep["steps"][2]["args"][0], dict) and isinstance(rep["steps"][2]["args"][1], dict)
    assert isinstance(CASES["no_resend_after_ack"]["steps"][6]["args"][2], dict)


def test_cited_lines_name_the_tests():
    """With the reference at hand: every case's first cited line holds `fn <name>`, and its last the closing brace of
    that function (names and line numbers are compared; nothing is copied)."""
    path = reference_source()
    if not os.path.exists(path):
        pytest.skip("the reference's sources are not on this machine")
    with open(path) as f:
        lines = f.read().split("\n")
    for c in DOC["cases"]:
        first, last = c["lines"]
        m = re.search(r"\bfn\s+(\w+)\s*\(", lines[first - 1])
        assert m and m.group(1) == c["name"], (c["name"], first)
        assert lines[last - 1].strip() == "}", (c["name"], last)
        assert not any(re.search(r"\bfn\s+\w+", x) for x in lines[first: last]), (c["name"], "another fn inside")


@pytest.mark.parametrize("name", NAMES)
def test_case_alone(name):
    """One connection, the host calls, every `expect` of the case met; an extra idle tick behind it emits nothing.
    packet_unambiguity runs all of its 8192 iterations: 8192 * 127 packet ids below packet_id::SPAN."""
    t0 = time.perf_counter()
    d = H.HalfTick([(H.Scenario(CASES[name]), 0)]).run(extra=1)
    print(f"{name}: {d.t} ticks, {d.frames_total} frames, {time.perf_counter() - t0:.2f} s")
    if name == "packet_unambiguity":
        assert d.conns[0].datagrams_seen == 8192 * 127 and d.frames_total == 8192


def mixed_assignment(n=130, rotate=0):
    """Connection c runs case (c + rotate) % 11 (all but packet_unambiguity); the groups of 11 start 0, 1 and 2 ticks
    late in turn."""
    return [(H.Scenario(CASES[MIXED[(c + rotate) % 11]]), (c // 11) % 3) for c in range(n)]


def test_mixed_assignment_covers_the_seams():
    """Every case sits at an index <= 62 and at one >= 65 under different staggers, and indices 63 and 64 are live."""
    a = mixed_assignment()
    for name in MIXED:
        at = [c for c, (sc, _) in enumerate(a) if sc.name == name]
        assert min(at) <= 62 and max(at) >= 65 and len({a[c][1] for c in at}) == 3, name
    assert a[63][0].name != a[64][0].name and a[63][1] == a[64][1] == 2


@pytest.mark.parametrize("rotate", range(11))
def test_mixed_batch_of_130(rotate):
    """130 connections at different step indices and with different now_ms in one call of every stage: every
    connection meets its case's `expect`, and emits nothing before its scenario begins and after it is over.
    rotate = 0 is the batch the device runs.  No one batch can hold eleven cases at index 63, so the assignment is
    rotated: over the eleven batches every case sits at index 63 and at index 64 (and, in each, at <= 62 and >= 65)."""
    t0 = time.perf_counter()
    assign = mixed_assignment(rotate=rotate)
    assert assign[63][0].name == MIXED[(63 + rotate) % 11] and assign[64][0].name == MIXED[(64 + rotate) % 11]
    d = H.HalfTick(assign, H.HostCalls(nthreads=4)).run()
    print(f"mixed batch, rotated by {rotate}: {d.t} ticks, {d.frames_total} frames, {time.perf_counter() - t0:.2f} s")
    assert d.t == 23 + 2 and d.frames_total == sum(em["expect"]["count"] for k in d.conns for _, em in k.sc.ticks)
