"""CPU: the batched flush control (ufc_flush_acks_host, ufc_flush_sync_host) against tests/flush_expect.py, byte
for byte on every output record; the ack flush against ufc_pack_host over its own merged array; the directed cases
of the allocation, the frame seam, the carry, BAD_STATE, the sync frame's timeout, ids, keepalive, allocation and
upstream stops; the argument contract; the binding (records, signatures, wrappers) against
include/uflow_flush_ctl.h.  tests/test_flush_gpu.py runs the same scenarios with the device calls in
the host calls' place (it replaces `acks_call` and `sync_call`)."""

import numpy as np
import pytest

from uflow_amd import flush as fl, frame as fr
from uflow_amd._native import lib, UFC_ERR_INVALID_ARG, UFC_OK

import flush_expect as E
import pack_expect as P

ACK_OUT = ("merged", "merged_first", "infos", "results", "ack_results", "windows_out", "ctl_out", "carry", "flushes",
           "flags")
SYNC_OUT = ("infos", "sync_index", "results", "ctl_out", "ticks_next")


def acks_call(ctl, windows, groups, group_first, receivers, rate, carry, merged_cap, frames_cap, flushes, flags, merged,
              infos, windows_out, ctl_out):
    return fl.flush_acks_host(ctl, windows, groups, group_first, receivers, rate, carry, merged_cap=merged_cap,
                              frames_cap=frames_cap, flushes=flushes, flags=flags, nthreads=3, merged=merged, infos=infos,
                              windows_out=windows_out, ctl_out=ctl_out)


def sync_call(ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders, syncs_cap,
              ticks_next, infos, ctl_out):
    return fl.flush_sync_host(ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders,
                              syncs_cap=syncs_cap, ticks_next=ticks_next, nthreads=3, infos=infos, ctl_out=ctl_out)


def _same(got, want, keys, what=""):
    for k in keys:
        if want[k] is None:
            assert got[k] is None, k
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(min(g.size, w.size)) if g.reshape(-1)[i].tobytes() != w.reshape(-1)[i].tobytes()]
            raise AssertionError(f"{what}{k}[{bad[:1]}]: {g.reshape(-1)[bad[0]] if bad else g.size} != "
                                 f"{w.reshape(-1)[bad[0]] if bad else w.size}")


def run_acks(inp, with_flushes=True, in_place=False, merged_cap=None, frames_cap=None):
    """One call against the model; the capped outputs start from a pattern, so that what must not be written shows.
    Returns (got, want)."""
    n = len(inp["ctl"])
    flushes = flags = None
    if with_flushes:
        flushes = np.zeros(n, dtype=fr.FLUSH_DTYPE)
        flushes["kind"], flushes["window_room"], flushes["id0"], flushes["id1"] = fr.DATA, 7, np.arange(n) + 3, 0xEEEE
        flushes["flush_alloc"] = -12345
        flags = (np.arange(n, dtype=np.uint32) * np.uint32(0x9E3779B1)) | np.uint32(2)   # bit 0 either way
    mc = merged_cap if merged_cap is not None else inp["carry"].size + inp["groups"].size
    fc = frames_cap if frames_cap is not None else n + mc
    merged = np.frombuffer(bytes([0xC3]) * (24 * mc), dtype=fr.ITEM_DTYPE).copy()
    infos = np.frombuffer(bytes([0x3C]) * (32 * fc), dtype=fr.FRAME_INFO_DTYPE).copy()
    want = E.expect_acks(**inp, flushes=flushes, flags=flags, merged_cap=mc, frames_cap=fc,
                         prefill={"merged": merged, "infos": infos})
    a = {k: v.copy() for k, v in inp.items()}
    got = acks_call(a["ctl"], a["windows"], a["groups"], a["group_first"], a["receivers"], a["rate"], a["carry"], mc, fc,
                    None if flushes is None else flushes.copy(), None if flags is None else flags.copy(), merged.copy(),
                    infos.copy(), a["windows"] if in_place else None, a["ctl"] if in_place else None)
    assert got["merged_used"] == want["merged_used"] and got["frames_used"] == want["frames_used"]
    _same(got, want, ACK_OUT)
    for k in ("groups", "group_first", "receivers", "rate"):   # the inputs stay
        assert a[k].tobytes() == inp[k].tobytes(), k
    if not in_place:
        assert a["ctl"].tobytes() == inp["ctl"].tobytes() and a["windows"].tobytes() == inp["windows"].tobytes()
    return got, want


def run_sync(inp, in_place=False, syncs_cap=None, with_ticks=True):
    n = len(inp["ctl"])
    sc = n if syncs_cap is None else syncs_cap
    infos = np.frombuffer(bytes([0x3C]) * (32 * sc), dtype=fr.FRAME_INFO_DTYPE).copy()
    inp = dict(inp)
    if not with_ticks:
        inp["ticks_next"] = None
    want = E.expect_sync(**inp, syncs_cap=sc, prefill={"infos": infos})
    a = {k: (None if v is None else v.copy()) for k, v in inp.items()}
    got = sync_call(a["ctl"], a["rate"], a["ack_results"], a["begin_results"], a["pack_results"], a["commit_results"],
                    a["queues"], a["senders"], sc, a["ticks_next"], infos.copy(), a["ctl"] if in_place else None)
    assert got["syncs_used"] == want["syncs_used"]
    _same(got, want, SYNC_OUT)
    for k in ("rate", "ack_results", "begin_results", "pack_results", "commit_results", "queues", "senders"):
        assert a[k].tobytes() == inp[k].tobytes(), k
    return got, want


# ---- the ack flush ----

ALLOCS = (-1, 0, 14, 15, 23, 24, 1463, 1464, 1465)
COUNTS = (0, 1, 161, 162, 163, 323)


def scenario_pack_equivalence():
    """Without sync_reply the frames and results are ufc_pack_host's over the merged array with an ack flush."""
    conns = [dict(groups=E.seq_groups(k, start=9 * k), alloc=a) for k in COUNTS for a in ALLOCS + (1 << 40, 2929, 2930)]
    conns += [dict(carry=E.seq_groups(3), groups=E.seq_groups(4, start=5 + 80), alloc=a) for a in (0, 40, 1 << 30)]
    inp = E.ack_inputs(conns)
    got, want = run_acks(inp)
    n = len(conns)
    flushes = np.zeros(n, dtype=fr.FLUSH_DTYPE)
    flushes["kind"], flushes["flush_alloc"] = fr.ACK, inp["rate"]["flush_alloc"]
    flushes["id0"], flushes["id1"] = inp["windows"]["base_id"], inp["receivers"]["base_id"]
    used = got["merged_used"]
    infos, results, frames_used = fr.pack_host(got["merged"][:used], got["merged_first"], flushes)
    assert frames_used == got["frames_used"] > n
    assert results.tobytes() == got["results"].tobytes()
    assert infos[:frames_used].tobytes() == got["infos"][:frames_used].tobytes()
    assert want["facts"]["full_frames"] > 10 and want["facts"]["size_limited"] > 10


@pytest.mark.parametrize("sync_reply", [0, 1, 0x80])
def test_alloc_and_count_grid(sync_reply):
    """Every alloc of the issue's list against every group count, with and without sync_reply; 161 groups fill a
    frame at 1464 bytes, the 162nd would make 1473."""
    conns = [dict(groups=E.seq_groups(k, start=3 + k), alloc=a, sync_reply=sync_reply) for k in COUNTS for a in ALLOCS]
    got, want = run_acks(E.ack_inputs(conns))
    f = want["facts"]
    assert f["dud"] == (len(COUNTS) * (len(ALLOCS) - 1) if sync_reply else 0)
    assert f["dud_empty"] == (len(COUNTS) * 2 + len(ALLOCS) - 3 if sync_reply else 0)   # alloc 0 and 14; no groups
    r = got["results"].reshape(len(COUNTS), len(ALLOCS))
    k161, k162 = COUNTS.index(161), COUNTS.index(162)
    a1463, a1464 = ALLOCS.index(1463), ALLOCS.index(1464)
    # 161 groups: the push of the last one needs alloc >= 15 + 160 * 9 = 1455; one frame of 1464 bytes either way
    assert r[k161][a1463]["frame_count"] == 1 and r[k161][a1463]["items_packed"] == 161 and r[k161][a1463]["stop"] == P.DONE
    assert r[k161][a1463]["alloc_left"] == 1463 - 1464
    # 162 groups: the 162nd finds the frame full; the next frame starts only with alloc - 1464 >= 0
    assert r[k162][a1463]["stop"] == P.SIZE_LIMITED and r[k162][a1463]["items_packed"] == 161
    assert r[k162][a1464]["stop"] == P.DONE and r[k162][a1464]["frame_count"] == 2
    a0, a15 = ALLOCS.index(0), ALLOCS.index(15)
    k1 = COUNTS.index(1)
    if sync_reply:   # the dud frame is finalized empty at the first push; with 15 bytes it takes the group
        assert r[k1][a0]["frame_count"] == 1 and r[k1][a0]["items_packed"] == 0 and r[k1][a0]["alloc_left"] == -15
        assert r[k1][a15]["items_packed"] == 1 and r[k1][a15]["stop"] == P.DONE
        assert (got["windows_out"]["sync_reply"].reshape(len(COUNTS), -1)[:, 1:] == 0).all()
        assert (got["windows_out"]["sync_reply"].reshape(len(COUNTS), -1)[:, 0] == sync_reply).all()   # alloc -1
    else:            # without a dud the same alloc packs one group first
        assert r[k1][a0]["frame_count"] == 1 and r[k1][a0]["items_packed"] == 1 and r[k1][a0]["alloc_left"] == -24


def scenario_carry_over_ticks(ticks=3, cap=8, alloc=20):
    """A connection whose allocation sends one group a tick (15 <= alloc < 24: a frame starts, the second push ends it): what stays is carried, the window re-emits the
    tail, and the groups go out in order, each once, over `ticks` ticks; then an allocation that empties the queue."""
    pending = E.seq_groups(6, start=100)
    inp = E.ack_inputs([dict(groups=pending, alloc=alloc, carry_cap=cap), dict(groups=E.seq_groups(2), alloc=1 << 20)])
    sent = []
    for t in range(ticks + 1):
        if t == ticks:
            inp["rate"]["flush_alloc"][0] = 1 << 20
        got, want = run_acks(inp, in_place=bool(t & 1))
        r = got["results"][0]
        m0 = int(got["merged_first"][0])
        sent += [int(g["id"]) for g in got["merged"][m0: m0 + int(r["items_packed"])]]
        kept = int(got["ctl_out"][0]["carry_count"])
        assert kept == int(got["ack_results"][0]["carried"]) == int(got["ack_results"][0]["merged_count"]) - int(r["items_packed"])
        if t < ticks:
            assert r["stop"] == P.SIZE_LIMITED and kept > 0 and got["windows_out"][0]["has_tail"] == 1
            assert int(got["flags"][0]) & 1 and int(got["flags"][1]) & 1 == 0
        else:
            assert r["stop"] == P.DONE and kept == 0 and got["windows_out"][0]["has_tail"] == 0
        # the next tick: the window writes the tail again, updated (one more bit), and nothing new
        c0 = int(got["ctl_out"][0]["carry_first"])
        tail = got["carry"][c0 + kept - 1] if kept else None
        inp = E.ack_inputs([dict(carry=[(int(g["id"]), int(g["data_offset"]), int(g["channel_id"]))
                                        for g in got["carry"][c0: c0 + kept]],
                                 groups=[(int(tail["id"]), int(tail["data_offset"]) | (1 << (t + 1)), int(tail["channel_id"]) ^ 1)]
                                 if kept else [], alloc=alloc, carry_cap=cap),
                            dict(groups=[], alloc=1 << 20)])
    assert sent == [g[0] for g in pending] and ticks >= 2


def scenario_carry_at_and_over_cap():
    """Unpacked groups that fill carry_cap exactly, and one more: the oldest is dropped, the tail survives."""
    gs = E.seq_groups(10, start=77)
    # alloc 20: one group is packed, nine stay
    got, want = run_acks(E.ack_inputs([dict(groups=gs, alloc=20, carry_cap=9), dict(groups=gs, alloc=20, carry_cap=8),
                                       dict(groups=gs, alloc=-1, carry_cap=1), dict(groups=gs, alloc=-1, carry_cap=0)]))
    ar = got["ack_results"]
    assert ar["stop"].tolist() == [E.FA_DONE, E.FA_CARRY_FULL, E.FA_CARRY_FULL, E.FA_CARRY_FULL]
    assert ar["carried"].tolist() == [9, 8, 1, 0] and ar["dropped"].tolist() == [0, 1, 9, 10]
    for c, kept in ((0, 9), (1, 8), (2, 1)):
        c0 = int(got["ctl_out"][c]["carry_first"])
        assert [int(g["id"]) for g in got["carry"][c0: c0 + kept]] == [g[0] for g in gs[10 - kept:]]
    assert want["facts"]["dropped"] == 20


def scenario_bad_state():
    gs = E.seq_groups(3, start=50)
    conns = [dict(carry=gs[:2], groups=[], alloc=1000, sync_reply=1),                     # a carry and no window group
             dict(carry=gs[:2], groups=[(gs[1][0] + 1, 1, 0)], alloc=1000, sync_reply=1),   # the ids differ
             dict(carry=gs[:2], groups=gs[1:], alloc=1000, sync_reply=1)]                  # sound
    inp = E.ack_inputs(conns)
    got, want = run_acks(inp, in_place=True)
    assert got["ack_results"]["stop"].tolist() == [E.FA_BAD_STATE, E.FA_BAD_STATE, E.FA_DONE]
    assert got["results"]["frame_count"].tolist() == [0, 0, 1] and want["facts"]["bad_state"] == 2
    assert got["ctl_out"][:2].tobytes() == inp["ctl"][:2].tobytes() and got["windows_out"][:2].tobytes() == inp["windows"][:2].tobytes()
    # the structural ones: carry_count over carry_cap, a room outside the arena, a reversed and an outlying range
    for breaker in ("count", "room", "reversed", "outlying"):
        inp = E.ack_inputs([dict(groups=gs, alloc=1000), dict(groups=gs, alloc=1000)])
        if breaker == "count":
            inp["ctl"]["carry_count"][0] = 9
        elif breaker == "room":
            inp["ctl"]["carry_first"][0] = inp["carry"].size - 7
        elif breaker == "reversed":
            inp["group_first"][:] = [3, 0, 6]
        else:
            inp["group_first"][1:] = [3, 7]
        got, want = run_acks(inp)
        assert want["facts"]["bad_state"] >= 1 and got["ack_results"]["stop"][0 if breaker != "outlying" else 1] == E.FA_BAD_STATE


def scenario_generated_acks(seed=5, n=300):
    rng = np.random.default_rng(seed)
    inp = E.ack_inputs([E.rand_ack_conn(rng) for _ in range(n)])
    _, want = run_acks(inp, in_place=bool(seed & 1))
    f = want["facts"]
    assert f["dud"] and f["dud_empty"] and f["size_limited"] and f["carried"] and f["dropped"] and f["bad_state"] == 0


def scenario_caps_one_short():
    conns = [dict(groups=E.seq_groups(k), alloc=1 << 30, sync_reply=int(k in (3, 0, 1))) for k in (3, 0, 170, 1)]
    inp = E.ack_inputs(conns)
    full, _ = run_acks(inp)
    got, _ = run_acks(inp, merged_cap=full["merged_used"] - 1, frames_cap=full["frames_used"] - 1)
    assert got["merged_used"] == full["merged_used"] == 174 and got["frames_used"] == full["frames_used"] == 5
    run_acks(inp, merged_cap=0, frames_cap=0, with_flushes=False)


def scenario_many_connections(n=65536 + 130):
    """More connections than the launch grid holds in one pass (the device's waves stride)."""
    rng = np.random.default_rng(12)
    kinds = [E.rand_ack_conn(rng, max_groups=3) for _ in range(50)]
    inp = E.ack_inputs([kinds[(c * 7) % 50] for c in range(n)], guard=0)
    run_acks(inp, in_place=True)


ACK_SCENARIOS = [scenario_pack_equivalence, scenario_carry_over_ticks, scenario_carry_at_and_over_cap, scenario_bad_state,
                 scenario_generated_acks, scenario_caps_one_short, scenario_many_connections]


@pytest.mark.parametrize("scenario", ACK_SCENARIOS, ids=lambda f: f.__name__[9:])
def test_ack_scenarios(scenario):
    scenario()


def test_carry_over_two_ticks():
    scenario_carry_over_ticks(ticks=2, alloc=15)


# ---- the sync frame ----

def scenario_sync_directed():
    """Every rule at its edge; each case names the reason and the mode the model must give."""
    S = E
    big = (1 << 64) - 1
    cases = [
        # elapsed at timeout - 1 and at timeout, rto below and above 2000
        (dict(now_ms=10000, base_ms=8001, rto_ms=600, next_id=31), S.FS_NOT_DUE, 0),
        (dict(now_ms=10000, base_ms=8000, rto_ms=600, next_id=31), S.FS_SENT, 2),
        (dict(now_ms=10000, base_ms=7001, rto_ms=3000, next_id=31), S.FS_NOT_DUE, 0),
        (dict(now_ms=10000, base_ms=7000, rto_ms=3000, next_id=31), S.FS_SENT, 2),
        # the ids: neither, the frame id, the packet id, both
        (dict(), S.FS_IDLE, 0),
        (dict(window_base_id=499), S.FS_SENT, 1),
        (dict(next_id=31), S.FS_SENT, 2),
        (dict(window_base_id=499, next_id=31), S.FS_SENT, 3),
        # the packet id needs an empty heap and no pending fragment
        (dict(next_id=31, heap_len=1), S.FS_IDLE, 0),
        (dict(next_id=31, pending_count=1), S.FS_IDLE, 0),
        (dict(next_id=31, pending_count=1, window_base_id=3), S.FS_SENT, 1),
        # keepalive: none, elapsed one below the interval, elapsed equal to it
        (dict(now_ms=50000, base_ms=10000), S.FS_IDLE, 0),
        (dict(now_ms=50000, base_ms=10000, keepalive_ms=40001), S.FS_IDLE, 0),
        (dict(now_ms=50000, base_ms=10000, keepalive_ms=40000), S.FS_SENT, 0),
        (dict(now_ms=50000, base_ms=10000, keepalive_ms=40000, has_keepalive=0x40), S.FS_SENT, 0),
        (dict(now_ms=50000, base_ms=10000, stale_interval=5), S.FS_IDLE, 0),
        # the allocation
        (dict(next_id=31, alloc_left=-1), S.FS_NO_ALLOC, 0),
        (dict(next_id=31, alloc_left=0), S.FS_SENT, 2),
        (dict(next_id=31, alloc_left=13), S.FS_SENT, 2),
        # the upstream stops
        (dict(next_id=31, ack_stop=P.SIZE_LIMITED, frame_count=1), S.FS_ACK_LIMITED, 0),
        (dict(next_id=31, ack_stop=P.BAD_RANGE), S.FS_SENT, 2),
        (dict(next_id=31, begin_stop=S.RS_SIZE_LIMITED, frame_count=1), S.FS_DATA_LIMITED, 0),
        (dict(next_id=31, pack_stop=P.SIZE_LIMITED), S.FS_DATA_LIMITED, 0),
        (dict(next_id=31, begin_stop=S.RS_WINDOW_LIMITED), S.FS_SENT, 2),
        (dict(next_id=31, pack_stop=P.WINDOW_LIMITED), S.FS_SENT, 2),
        (dict(next_id=31, begin_stop=S.RS_STAGE_FULL), S.FS_SENT, 2),
        (dict(next_id=31, begin_stop=S.RS_REF_HANG), S.FS_UPSTREAM, 0),
        (dict(next_id=31, begin_stop=S.RS_BAD_STATE), S.FS_UPSTREAM, 0),
        (dict(next_id=31, commit_stop=S.RS_BAD_STATE), S.FS_UPSTREAM, 0),
        (dict(next_id=31, commit_stop=S.RS_HEAP_FULL, frame_count=3), S.FS_UPSTREAM, 0),
        # a data frame went out: the timeout starts again
        (dict(next_id=31, frame_count=1), S.FS_NOT_DUE, 0),
        # now_ms below the base: the difference wraps and is huge
        (dict(now_ms=5, base_ms=6, next_id=31), S.FS_SENT, 2),
        (dict(now_ms=0, base_ms=big, next_id=31), S.FS_NOT_DUE, 0),
        (dict(now_ms=1999, base_ms=big, next_id=31, keepalive_ms=big), S.FS_SENT, 2),
    ]
    inp = E.sync_inputs([c[0] for c in cases])
    for in_place in (False, True):
        got, want = run_sync(inp, in_place=in_place)
        for k, (d, reason, mode) in enumerate(cases):
            assert int(want["results"][k]["reason"]) == reason and int(want["results"][k]["mode"]) == mode, (k, d)
        assert want["facts"]["wrapped"] == 3 and all(want["facts"]["reasons"]) and all(want["facts"]["modes"])
    sent = [k for k, c in enumerate(cases) if c[1] == E.FS_SENT]
    assert got["sync_index"][sent].tolist() == list(range(len(sent))) and got["syncs_used"] == len(sent)
    assert (got["ticks_next"]["alloc_adjust"][sent] == -14).all() and got["ticks_next"]["alloc_adjust"].sum() == -14 * len(sent)
    # the base moved exactly where a data frame or the sync frame went out
    moved = got["ctl_out"]["sync_timeout_base_ms"] != inp["ctl"]["sync_timeout_base_ms"]
    assert moved.tolist() == [bool((c[1] == E.FS_SENT or (c[0].get("frame_count", 0) and c[1] != E.FS_ACK_LIMITED)) and
                                   c[0].get("now_ms", 100000) != c[0].get("base_ms", 1000)) for c in cases]
    run_sync(inp, with_ticks=False, syncs_cap=len(sent) - 1)
    run_sync(inp, syncs_cap=0)


def scenario_generated_sync(seed=3, n=1000):
    rng = np.random.default_rng(seed)
    _, want = run_sync(E.sync_inputs([E.rand_sync_conn(rng) for _ in range(n)]), in_place=bool(seed & 1))
    assert all(want["facts"]["reasons"]) and all(want["facts"]["modes"])


def sync_pattern(n, senders):
    """n connections of which exactly `senders` (a set of indices) send a frame."""
    return E.sync_inputs([dict(next_id=31, log_next_id=c) if c in senders else dict(log_next_id=c) for c in range(n)])


def scenario_sync_compaction():
    """Frames only from lane 63, only from lane 0 of the second tile, from all and from none; sizes around a tile."""
    for n in (1, 63, 64, 65, 130):
        for senders in ({63}, {64}, set(range(n)), set(), {0, 63, 64, 129}, set(range(0, n, 3))):
            senders = {c for c in senders if c < n}
            got, _ = run_sync(sync_pattern(n, senders))
            assert got["syncs_used"] == len(senders)
            assert [c for c in range(n) if got["sync_index"][c] != fr.NO_PARENT] == sorted(senders)


SYNC_SCENARIOS = [scenario_sync_directed, scenario_generated_sync, scenario_sync_compaction]


@pytest.mark.parametrize("scenario", SYNC_SCENARIOS, ids=lambda f: f.__name__[9:])
def test_sync_scenarios(scenario):
    scenario()


# ---- the argument contract ----

def test_argument_contract():
    l = lib()
    inp = E.ack_inputs([dict(groups=E.seq_groups(2), alloc=100)])
    n = 1
    out = {"merged": np.zeros(8, fr.ITEM_DTYPE), "merged_first": np.zeros(2, np.uint64), "merged_used": np.zeros(1, np.uint64),
           "infos": np.zeros(8, fr.FRAME_INFO_DTYPE), "frames_used": np.zeros(1, np.uint64),
           "results": np.zeros(1, fr.FLUSH_RESULT_DTYPE), "ack_results": np.zeros(1, fl.FLUSH_ACKS_RESULT_DTYPE),
           "windows_out": np.zeros(1, fr.FRAME_WINDOW_DTYPE), "ctl_out": np.zeros(1, fl.FLUSH_CTL_DTYPE)}

    def acks(n=n, **null):
        p = lambda k, a: None if k in null else a.ctypes.data   # noqa: E731
        return l.ufc_flush_acks_host(p("ctl", inp["ctl"]), p("windows", inp["windows"]), p("groups", inp["groups"]),
                                     inp["groups"].size, p("group_first", inp["group_first"]),
                                     p("receivers", inp["receivers"]), p("rate", inp["rate"]), n, p("carry", inp["carry"]),
                                     inp["carry"].size, p("merged", out["merged"]), 0 if "merged" in null and null["merged"] else 8,
                                     p("merged_first", out["merged_first"]), p("merged_used", out["merged_used"]),
                                     p("infos", out["infos"]), 0 if "infos" in null and null["infos"] else 8,
                                     p("frames_used", out["frames_used"]), p("results", out["results"]),
                                     p("ack_results", out["ack_results"]), p("windows_out", out["windows_out"]),
                                     p("ctl_out", out["ctl_out"]), None, None, 1)

    assert acks() == UFC_OK and out["frames_used"][0] == 1
    for k in ("ctl", "windows", "groups", "group_first", "receivers", "rate", "carry", "merged_first", "merged_used",
              "frames_used", "results", "ack_results", "windows_out", "ctl_out"):
        assert acks(**{k: 0}) == UFC_ERR_INVALID_ARG, k
    assert acks(merged=0) == UFC_ERR_INVALID_ARG and acks(infos=0) == UFC_ERR_INVALID_ARG   # NULL with a nonzero cap
    assert acks(merged=1, infos=1) == UFC_OK and out["merged_used"][0] == 2                  # NULL with a zero cap
    for at in (3, 9):   # n_groups and n_carry of 2^31 - 1: the merged counts are 32-bit
        args = [None] * 3 + [0] + [None] * 3 + [1, None, 0, None, 0] + [None] * 3 + [0] + [None] * 7 + [1]
        args[at] = (1 << 31) - 1
        assert l.ufc_flush_acks_host(*args) == UFC_ERR_INVALID_ARG, at
    assert l.ufc_flush_acks_host(*([None] * 3), 0, *([None] * 3), 0, None, 0, None, 0, *([None] * 3), 0,
                                 *([None] * 7), 1) == UFC_OK   # n == 0
    assert l.ufc_flush_acks_host(*([None] * 3), 0, *([None] * 3), (1 << 31) - 1, None, 0, None, 0, *([None] * 3), 0,
                                 *([None] * 7), 1) == UFC_ERR_INVALID_ARG

    s = E.sync_inputs([dict(next_id=31)])
    so = {"infos": np.zeros(1, fr.FRAME_INFO_DTYPE), "sync_index": np.zeros(1, np.uint32), "syncs_used": np.zeros(1, np.uint64),
          "results": np.zeros(1, fl.FLUSH_SYNC_RESULT_DTYPE), "ctl_out": np.zeros(1, fl.FLUSH_CTL_DTYPE)}
    names = ("ctl", "rate", "ack_results", "begin_results", "pack_results", "commit_results", "queues", "senders")

    def sync(cap=1, **null):
        p = lambda k, a: None if k in null else a.ctypes.data   # noqa: E731
        return l.ufc_flush_sync_host(*[p(k, s[k]) for k in names], 1, p("infos", so["infos"]), cap,
                                     p("sync_index", so["sync_index"]), p("syncs_used", so["syncs_used"]),
                                     p("results", so["results"]), p("ctl_out", so["ctl_out"]), None, 1)

    assert sync() == UFC_OK and so["syncs_used"][0] == 1 and so["infos"][0]["kind"] == fr.SYNC
    for k in names + ("infos", "sync_index", "syncs_used", "results", "ctl_out"):
        assert sync(**{k: 0}) == UFC_ERR_INVALID_ARG, k
    assert sync(cap=0, infos=0) == UFC_OK
    assert l.ufc_flush_sync_host(*([None] * 8), 0, None, 0, *([None] * 5), 1) == UFC_OK
    assert l.ufc_flush_sync_host(*([None] * 8), (1 << 31) - 1, None, 0, *([None] * 5), 1) == UFC_ERR_INVALID_ARG


def test_wrappers_allocate_and_new_flush_ctl():
    ctl, carry = fl.new_flush_ctl(3, 30000, 4)
    assert ctl["carry_first"].tolist() == [0, 4, 8] and carry.size == 12 and (ctl["has_keepalive"] == 1).all()
    ctl2, _ = fl.new_flush_ctl(2, None, 1)
    assert (ctl2["has_keepalive"] == 0).all() and (ctl2["keepalive_interval_ms"] == 0).all()
    inp = E.ack_inputs([dict(groups=E.seq_groups(2), alloc=1 << 20, sync_reply=1)] * 3, guard=0, carry_cap=4)
    got = fl.flush_acks_host(ctl, inp["windows"], inp["groups"], inp["group_first"], inp["receivers"], inp["rate"], carry)
    assert got["frames_used"] == 3 and got["merged"].size == 12 + 6 and got["infos"].size == 3 + 18
    assert (got["windows_out"]["sync_reply"] == 0).all() and (got["windows_out"]["has_tail"] == 0).all()
    s = E.sync_inputs([dict(next_id=31)] * 3)
    d = fl.flush_sync_host(ctl, s["rate"], got["results"], s["begin_results"], s["pack_results"], s["commit_results"],
                           s["queues"], s["senders"])
    assert d["syncs_used"] == 3 and d["ticks_next"] is None and (d["ctl_out"]["sync_timeout_base_ms"] == 100000).all()
    empty = fl.flush_acks_host(ctl[:0], inp["windows"][:0], inp["groups"][:0], np.zeros(1, np.uint64), inp["receivers"][:0],
                               inp["rate"][:0], carry[:0])
    assert empty["frames_used"] == 0 and empty["merged_used"] == 0


def test_flush_core_under_sanitizers():
    """tests/c/flush_host_check.hip: the wave-policy core of the flush control (fa_plan / fa_write, fs_decide_tile /
    fs_write_tile, the lanes of a phase run one after the other: forwards, backwards, shuffled, and on a carried
    shared block) as host code under AddressSanitizer and UBSan, against a serial restatement and literals, over
    exact-size buffers; a stand-alone program (nothing is loaded into Python under a sanitizer)."""
    import os
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "flush_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "flush_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


# ---- the binding of include/uflow_flush_ctl.h: what tests/test_records_cpu.py, tests/test_native_cpu.py and
# tests/test_host_args_cpu.py check for the other headers, for this one ----

def test_flush_records_match_the_header(tmp_path):
    """FLUSH_RECORDS of uflow_amd/records.py against sizeof / offsetof compiled from the header (C99, -pedantic, through
    uflow_frame_codec.h, which brings the header along); uflow_amd.flush exports the dtypes; no struct of the header
    is left out of the table."""
    import os
    import re
    from test_records_cpu import INCLUDE, _header_layout
    from uflow_amd.records import FLUSH_RECORDS, RECORDS
    assert len(FLUSH_RECORDS) == 3 and not set(FLUSH_RECORDS) & set(RECORDS)
    for struct, dt in FLUSH_RECORDS.items():
        assert getattr(fl, struct[len("ufc_"):].upper() + "_DTYPE") is dt
    got = _header_layout(tmp_path, {s: dt.names for s, dt in FLUSH_RECORDS.items()})
    want = {}
    for struct, dt in FLUSH_RECORDS.items():
        want["S", struct] = (dt.itemsize,)
        for f in dt.names:
            want["F", f"{struct}.{f}"] = (dt.fields[f][1], dt.fields[f][0].itemsize)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    with open(os.path.join(INCLUDE, "uflow_flush_ctl.h")) as f:
        text = f.read()
    assert set(re.findall(r"^\} (ufc_\w+);", text, flags=re.M)) == set(FLUSH_RECORDS)
    consts = dict(re.findall(r"#define\s+(UFC_F[AS]_\w+)\s+(\d+)", text))
    assert len(consts) == 10
    for name, value in consts.items():   # the stop codes and reasons, each written once in _native
        assert getattr(fl, name[len("UFC_"):]) == int(value), name


def test_flush_signatures_match_the_header():
    """Every prototype of the header against _native._FLUSH_SIGNATURES (parameter count, pointer-ness by position),
    and the library exports each."""
    import ctypes
    import os
    import re
    from test_records_cpu import INCLUDE
    from uflow_amd import _native
    with open(os.path.join(INCLUDE, "uflow_flush_ctl.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = {name: [p.strip() for p in params.split(",")]
              for name, params in re.findall(r"\b(ufc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert set(protos) == set(_native._FLUSH_SIGNATURES) == set(_native.FLUSH_SYMBOLS) and len(protos) == 4
    assert not set(protos) & set(_native.SYMBOLS)
    pointer_types = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, (_, argtypes) in _native._FLUSH_SIGNATURES.items():
        assert hasattr(raw, name) and getattr(lib(), name).argtypes == argtypes, name
        assert len(protos[name]) == len(argtypes), (name, len(protos[name]), len(argtypes))
        for k, (p, t) in enumerate(zip(protos[name], argtypes)):
            assert ("*" in p) == issubclass(t, pointer_types), (name, k, p, t)


def _wrapper_table(n):
    """As tests/test_host_args_cpu.py's table: (function, keyword arguments of a passing call, {written argument:
    entries it must hold}, inputs that are one entry short when their last entry is cut)."""
    Z = lambda k, dt: np.zeros(k, dtype=dt)   # noqa: E731
    ctl, carry = fl.new_flush_ctl(n, 1000, 2)
    queues, _ = fr.new_frame_queues(n, 8, 4)
    yield (fl.flush_acks_host,
           dict(ctl=ctl, windows=fr.new_frame_windows(n, 8), groups=Z(0, fr.ITEM_DTYPE), group_first=Z(n + 1, np.uint64),
                receivers=fr.new_receivers(n, 8), rate=Z(n, fr.RATE_RESULT_DTYPE), carry=carry, merged_cap=2 * n,
                frames_cap=n, flushes=Z(n, fr.FLUSH_DTYPE), flags=Z(n, np.uint32), merged=Z(2 * n, fr.ITEM_DTYPE),
                infos=Z(n, fr.FRAME_INFO_DTYPE), windows_out=Z(n, fr.FRAME_WINDOW_DTYPE), ctl_out=Z(n, fl.FLUSH_CTL_DTYPE)),
           {"carry": 0, "merged": 2 * n, "infos": n, "flushes": n, "flags": n, "windows_out": n, "ctl_out": n},
           ["windows", "group_first", "receivers", "rate"])
    yield (fl.flush_sync_host,
           dict(ctl=ctl, rate=Z(n, fr.RATE_RESULT_DTYPE), ack_results=Z(n, fr.FLUSH_RESULT_DTYPE),
                begin_results=Z(n, fr.RESEND_RESULT_DTYPE), pack_results=Z(n, fr.FLUSH_RESULT_DTYPE),
                commit_results=Z(n, fr.RESEND_COMMIT_RESULT_DTYPE), queues=queues, senders=Z(n, fr.SENDER_DTYPE),
                syncs_cap=n, ticks_next=Z(n, fr.RATE_TICK_DTYPE), infos=Z(n, fr.FRAME_INFO_DTYPE),
                ctl_out=Z(n, fl.FLUSH_CTL_DTYPE)),
           {"infos": n, "ticks_next": n, "ctl_out": n},
           ["rate", "ack_results", "begin_results", "pack_results", "commit_results", "queues", "senders"])


@pytest.mark.parametrize("n", [1, 3])
def test_host_wrappers_refuse_bad_arguments(n):
    """Every array the C side writes into, given with the wrong dtype, one entry short, non-contiguous and read-only,
    raises a ValueError that names the argument before the C call sees it; so do the per-record inputs one entry
    short.  The module has no other *_host wrapper."""
    assert {k for k in vars(fl) if k.endswith("_host")} == {"flush_acks_host", "flush_sync_host"}
    for f, kw, written, short in _wrapper_table(n):
        f(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()})   # the table's call passes
        for arg, need in written.items():
            good = kw[arg]
            ro = good.copy()
            ro.flags.writeable = False
            bad = {"wrong dtype": np.zeros(good.size, dtype="<i2"),
                   "non-contiguous": np.zeros(2 * max(good.size, 2), dtype=good.dtype)[::2], "read-only": ro}
            if need:
                bad["one entry short"] = good[:need - 1].copy()
            for what, value in bad.items():
                with pytest.raises(ValueError) as e:
                    f(**dict(kw, **{arg: value}))
                assert arg in str(e.value), (f.__name__, arg, what, str(e.value))
        for arg in short:
            with pytest.raises(ValueError):
                f(**dict(kw, **{arg: kw[arg][:-1].copy()}))
