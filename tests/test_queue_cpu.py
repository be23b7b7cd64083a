"""CPU: the batched sender frame queue on the host (ufc_frame_queue_host, uflow_amd.frame.frame_queue_host) against
tests/queue_expect.py, FrameQueue, FrameLog, FeedbackGen, ReorderBuffer and LossIntervalQueue restated class for class
from the reference, and the hand-traced cases of tests/golden/frame_queue_cases.json.  Results (loss_rate as its 64
bits), states, every log byte and ref_acked are compared.  tests/test_gpu_queue.py runs the same scenarios with the
device call in `host`'s place."""
import ctypes
import json
import os

import numpy as np
import pytest

from uflow_amd import frame as fr
from uflow_amd._native import UFC_ERR_INVALID_ARG, lib

import queue_expect as E

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "frame_queue_cases.json")) as _f:
    GOLDEN = json.load(_f)
M32 = E.M32


def host(infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked, nthreads, in_place):
    """The call under test (the GPU tests put the device call here).  log and ref_acked are updated in place."""
    return fr.frame_queue_host(infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked=ref_acked,
                               nthreads=nthreads, queues_out=queues if in_place else None)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = [k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} records differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


def run(call, queues, log, ref_acked=None, nthreads=1, in_place=False):
    """One call, compared byte for byte with the restatement.  Returns (outputs, expected); the inputs are left as
    they are."""
    want = E.expect_batch(call["infos"], call["items"], call["frame_first"], call["sent"], call["sent_first"], queues,
                          call["steps"], log, ref_acked)
    q_in, log_io = queues.copy(), log.copy()
    refs_io = ref_acked.copy() if ref_acked is not None else None
    got = host(call["infos"], call["items"], call["frame_first"], call["sent"], call["sent_first"], q_in, call["steps"],
               log_io, refs_io, nthreads, in_place)
    n = len(queues)
    same(got["results"][:n], want["results"], "results")
    same(got["queues_out"][:n], want["queues_out"], "queues_out")
    same(got["log"], want["log"], "log")
    if ref_acked is not None:
        same(got["ref_acked"], want["ref_acked"], "ref_acked")
    if not in_place:
        same(q_in, queues, "queues (input)")
    return got, want


def one_call(queue, sent=(), acks=(), flags=0, rtt_ms=None, thresh_ms=0, now_ms=0, reset=0.0):
    """A call for one connection: acks = [(frame_window_base_id or None, [[base_id, bitfield, nonce], ...]), ...]."""
    infos, items = [], []
    for base, groups in acks:
        infos.append(E.ack_info(int(queue["window_base_id"]) if base is None else base, len(items), len(groups)))
        items += [E.group_item(*g) for g in groups]
    arr = lambda xs, dt: np.array(xs, dtype=dt) if len(xs) else np.zeros(0, dtype=dt)
    if rtt_ms is not None:
        flags |= fr.FQ_HAS_RTT
    return {"infos": arr(infos, fr.FRAME_INFO_DTYPE), "items": arr(items, fr.ITEM_DTYPE),
            "frame_first": np.array([0, len(infos)], dtype=np.uint64), "sent": arr(list(sent), fr.SENT_FRAME_DTYPE),
            "sent_first": np.array([0, len(sent)], dtype=np.uint64),
            "steps": np.array([E.make_step(flags, rtt_ms or 0, thresh_ms, now_ms, reset)], dtype=fr.FRAME_QUEUE_STEP_DTYPE)}


# ---- the goldens ----
def run_queue_case(case):
    size, tail, base = case["new"]
    q, log = fr.new_frame_queues(1, size, tail, base)
    refs = np.zeros(16, dtype=np.uint8)
    for k, c in enumerate(case["calls"]):
        sent = [E.sent_frame(s, t, n, ref_first=j % 16, ref_count=1, mark=bool(m)) for j, (s, t, n, m) in enumerate(c.get("push", []))]
        if "fill" in c:
            f = c["fill"]
            sent += [E.sent_frame(f["size"], f["time"], (int(q[0]["log_next_id"]) + j) & 1) for j in range(f["count"])]
        flags = (fr.FQ_FORGET if c.get("forget") is not None else 0) | (fr.FQ_FEEDBACK if c.get("feedback") is not None else 0)
        call = one_call(q[0], sent, [(a["base"], a["groups"]) for a in c.get("acks", [])], flags, c.get("rtt"),
                        c.get("forget") or 0, c.get("feedback") or 0)
        got, _ = run(call, q, log, refs)
        res, out = got["results"][0], got["queues_out"][0]
        assert int(res["stop"]) == fr.FQ_DONE, k
        x = c["expect"]
        if "feedback" in x:
            if x["feedback"] is None:
                assert int(res["has_feedback"]) == 0, k
            else:
                assert int(res["has_feedback"]) == 1, k
                assert float(res["loss_rate"]) == x["feedback"]["loss_rate"], (k, float(res["loss_rate"]))
                for key in ("receive_rate", "rate_limited", "rtt_ms"):
                    assert int(res[key]) == x["feedback"][key], (k, key)
        for key, v in x.get("result", {}).items():
            assert int(res[key]) == v, (k, key, int(res[key]))
        for key, v in x.get("queue", {}).items():
            assert int(out[key]) == v, (k, key, int(out[key]))
        if "li_length" in x:
            assert out["li_length"][:int(out["li_count"])].tolist() == x["li_length"], k
        q, log, refs = got["queues_out"][:1].copy(), got["log"], got["ref_acked"]


QUEUE_CASES = GOLDEN["queue_cases"] + GOLDEN["loss_cases"]


@pytest.mark.parametrize("case", QUEUE_CASES, ids=[c["name"].split(" (")[0].split(":")[0] for c in QUEUE_CASES])
def test_golden_queue_cases(case):
    run_queue_case(case)


def frame_time(frame_id):
    return 1000 * frame_id + 7


def run_reorder_case(case):
    """A reorder_buffer.rs row through the batch call: put(x) is an ack group for frame x alone, advance(x) a forget
    with the threshold at frame x's send time.  Frame id is sent at frame_time(id) and rtt is 0, so every nack opens
    a loss interval that ends at its frame's time, and every ack counts into the front one: the intervals spell
    out the callbacks."""
    q, log = fr.new_frame_queues(1, 64, 36, 0)
    assert int(q[0]["rb_max_span"]) == 100
    got, _ = run(one_call(q[0], [E.sent_frame(10, frame_time(k), 0) for k in range(10)]), q, log)
    q, log = got["queues_out"][:1].copy(), got["log"]
    ends, lengths = [], []
    for op, arg, callbacks in case["ops"]:
        if op == "put":
            call = one_call(q[0], acks=[(None, [[arg, 1, 0]])], rtt_ms=0)
        else:
            call = one_call(q[0], flags=fr.FQ_FORGET, rtt_ms=0, thresh_ms=frame_time(arg))
        got, _ = run(call, q, log)
        res = got["results"][0]
        assert int(res["li_acks"]) == sum(1 for _, seen in callbacks if seen), (op, arg)
        assert int(res["li_nacks"]) == sum(1 for _, seen in callbacks if not seen), (op, arg)
        for frame_id, seen in callbacks:
            if not seen:
                ends.insert(0, frame_time(frame_id))
                lengths.insert(0, 1)
            elif lengths:
                lengths[0] += 1
        q, log = got["queues_out"][:1].copy(), got["log"]
        assert q[0]["li_end_time_ms"][:int(q[0]["li_count"])].tolist() == ends, (op, arg)
        assert q[0]["li_length"][:int(q[0]["li_count"])].tolist() == lengths, (op, arg)
    assert int(q[0]["rb_count"]) == case["frame_count"]


@pytest.mark.parametrize("case", GOLDEN["reorder_cases"], ids=[c["name"] for c in GOLDEN["reorder_cases"]])
def test_golden_reorder_cases(case):
    rb = E.ReorderBuffer(0, 100)                 # the restated class alone, callback for callback
    for op, arg, callbacks in case["ops"]:
        seen = []
        (rb.put if op == "put" else rb.advance)(arg, lambda frame_id, was_seen: seen.append([frame_id, was_seen]))
        assert seen == callbacks, (op, arg)
    assert rb.frame_count == case["frame_count"]
    run_reorder_case(case)                       # and through the batch call


def test_golden_span_case():
    c = GOLDEN["span_case"]
    rb = E.ReorderBuffer(c["base_id"], c["max_span"])
    assert [[x, rb.can_put(x)] for x, _ in c["can_put"]] == c["can_put"]
    assert [[x, rb.can_advance(x)] for x, _ in c["can_advance"]] == c["can_advance"]


# ---- generated traffic ----
def chain(n, window, tail, base, nthreads=1, seed=1, rounds=4, in_place=False, **kw):
    """`rounds` chained calls of generated traffic; returns the summed result counters."""
    rng = np.random.default_rng(seed)
    q, log, calls = E.make_batch(rng, n, window, tail, base, rounds=rounds, **kw)
    refs = np.zeros(calls[-1]["refs"] + 3, dtype=np.uint8)
    total = {}
    for call in calls:
        got, want = run(call, q, log, refs, nthreads=nthreads, in_place=in_place)
        for key in want["results"].dtype.names:
            if want["results"].dtype[key].kind == "u":
                total[key] = total.get(key, 0) + int(want["results"][key].astype(np.uint64).sum())
        q, log, refs = got["queues_out"][:n].copy(), got["log"], got["ref_acked"]
    total["refs_marked"] = int(refs.sum())
    return total


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("base", [0, 0xFFFFFFF0])
@pytest.mark.parametrize("window", [1, 4, 4096])
@pytest.mark.parametrize("n", [1, 3])
def test_generated_traffic(n, window, base, nthreads):
    t = chain(n, window, window, base, nthreads, seed=window + n, rounds=6 if window < 4096 else 4)
    assert t["pushes_taken"] > 0 and t["ack_frames"] > 0


def check_generator(t):
    """What the generated traffic must exercise, judged on the expectation's side."""
    for key in ("pushes_taken", "pushes_refused", "groups_dud", "groups_unknown", "groups_bad_nonce", "frames_acked", "li_acks",
                "li_nacks", "window_advanced", "log_culled", "has_feedback", "refs_marked"):
        assert t[key] > 0, (key, t)


@pytest.mark.parametrize("nthreads", [1, 4])
def test_generated_traffic_1000_connections(nthreads):
    check_generator(chain(1000, 64, 64, 0xFFFFFFF0, nthreads, seed=9, rounds=3))


def test_in_place_and_a_ring_that_wraps():
    """queues_out = queues, and window 4 / tail 4 / log_cap 8: the ring wraps every other call."""
    t = chain(5, 4, 4, 0xFFFFFFFA, 2, seed=3, rounds=12, in_place=True, log_cap=8, sends=6)
    assert t["log_culled"] > 16 and t["frames_acked"] > 16


def test_non_monotone_log():
    """Send times all over: the nack tiles must give push_nack's answer entry by entry."""
    t = chain(4, 256, 256, 100, 1, seed=5, rounds=5, monotone=False, loss=0.4)
    assert t["li_nacks"] > 100


def split_call(call, c, at):
    """`call` in two: connection c's frames up to `at` (with the pushes and the reset), then the rest (with the
    forget and the feedback); the other connections whole in the first."""
    ff = call["frame_first"].astype(np.int64)
    a, b = dict(call), dict(call)
    fa = ff.copy()
    fa[c + 1:] -= ff[c + 1] - at
    a["infos"] = np.concatenate([call["infos"][:at], call["infos"][ff[c + 1]:]])
    a["frame_first"] = fa.astype(np.uint64)
    a["steps"] = call["steps"].copy()
    a["steps"]["flags"][c] &= M32 ^ (fr.FQ_FORGET | fr.FQ_FEEDBACK)
    n = len(ff) - 1
    fb = np.zeros(n + 1, dtype=np.uint64)
    fb[c + 1:] = ff[c + 1] - at
    b["infos"] = call["infos"][at:ff[c + 1]]
    b["frame_first"] = fb
    b["sent"], b["sent_first"] = call["sent"][:0], np.zeros(n + 1, dtype=np.uint64)
    b["steps"] = call["steps"].copy()
    b["steps"]["flags"] &= fr.FQ_HAS_RTT
    b["steps"]["flags"][c] |= call["steps"]["flags"][c] & (fr.FQ_FORGET | fr.FQ_FEEDBACK)
    return a, b


def test_split_batch_equals_one_call():
    rng = np.random.default_rng(17)
    q, log, calls = E.make_batch(rng, 3, 64, 64, 0xFFFFFFC0, rounds=3, hostile=0.1)
    refs = np.zeros(calls[-1]["refs"] + 1, dtype=np.uint8)
    for call in calls[:2]:
        got, _ = run(call, q, log, refs)
        q, log, refs = got["queues_out"][:3].copy(), got["log"], got["ref_acked"]
    call = calls[2]
    whole, _ = run(call, q, log, refs)
    ff = call["frame_first"].astype(np.int64)
    c = int(np.argmax(ff[1:] - ff[:-1]))
    assert ff[c + 1] - ff[c] >= 2
    for at in range(int(ff[c]), int(ff[c + 1]) + 1):
        a, b = split_call(call, c, at)
        first, _ = run(a, q, log, refs)
        second, _ = run(b, first["queues_out"][:3].copy(), first["log"], first["ref_acked"])
        same(second["queues_out"][:3], whole["queues_out"][:3], f"state, split at {at}")
        same(second["log"], whole["log"], "log")
        same(second["ref_acked"], whole["ref_acked"], "ref_acked")
        r2, rw = second["results"][c], whole["results"][c]
        for key in ("has_feedback", "rate_limited", "receive_rate", "rtt_ms", "loss_rate", "window_room"):
            assert r2[key].tobytes() == rw[key].tobytes(), (at, key)


# ---- the state check ----
def busy_state(seed=23):
    """A connection in mid traffic: a state with held reorder-buffer frames, loss intervals and pending ack data,
    and a call for it."""
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        q, log, calls = E.make_batch(rng, 1, 64, 64, 1000, rounds=4, hostile=0.0, loss=0.3, sends=40)
        for call in calls[:3]:
            call["steps"]["flags"] &= M32 ^ (fr.FQ_FEEDBACK | fr.FQ_RESET_LOSS)
            out = E.expect_batch(call["infos"], call["items"], call["frame_first"], call["sent"], call["sent_first"], q,
                                 call["steps"], log)
            q, log = out["queues_out"], out["log"]
        if int(q[0]["rb_count"]) == 2 and int(q[0]["li_count"]) >= 2 and q[0]["has_ack_data"]:
            return q, log, calls[3]
    raise AssertionError("no busy state found")


BAD_STATES = {
    "log_cap not a power of two": lambda q, c: q.__setitem__("log_cap", 96),
    "log_cap zero": lambda q, c: q.__setitem__("log_cap", 0),
    "log_cap below window + tail": lambda q, c: q.__setitem__("tail_size", 65),
    "ring outside the arena": lambda q, c: q.__setitem__("log_first", 1),
    "log longer than the ring": lambda q, c: (q.__setitem__("log_base_id", int(q["log_next_id"][0]) - 129),
                                              q.__setitem__("rb_base_id", int(q["log_next_id"][0]) - 129)),
    "window behind by more than its size": lambda q, c: q.__setitem__("window_base_id", int(q["log_next_id"][0]) - 65),
    "log starts more than tail behind the window": lambda q, c: q.__setitem__("tail_size", 1),
    "max_span below window + tail": lambda q, c: q.__setitem__("rb_max_span", 127),
    "max_span beyond 2^31": lambda q, c: q.__setitem__("rb_max_span", (1 << 31) + 1),
    "reorder base outside the log": lambda q, c: q.__setitem__("rb_base_id", int(q["log_next_id"][0]) + 1),
    "reorder base behind the log": lambda q, c: q.__setitem__("rb_base_id", int(q["log_base_id"][0]) - 1),
    "rb_count 3": lambda q, c: q.__setitem__("rb_count", 3),
    "held frame at the base": lambda q, c: q["rb_frames"].__setitem__((0, 0), int(q["rb_base_id"][0])),
    "held frame outside the log": lambda q, c: q["rb_frames"].__setitem__((0, 1), int(q["log_next_id"][0])),
    "held frames out of order": lambda q, c: q["rb_frames"].__setitem__((0, slice(None)), q["rb_frames"][0, ::-1].copy()),
    "li_count 10": lambda q, c: q.__setitem__("li_count", 10),
    "reset with no interval": lambda q, c: (q.__setitem__("li_count", 0), c["steps"].__setitem__("flags", fr.FQ_RESET_LOSS)),
    "frame range reversed": lambda q, c: (c["frame_first"].__setitem__(0, 1), c["frame_first"].__setitem__(1, 0)),
    "frame range outside": lambda q, c: c["frame_first"].__setitem__(1, len(c["infos"]) + 1),
    "sent range reversed": lambda q, c: (c["sent_first"].__setitem__(0, 1), c["sent_first"].__setitem__(1, 0)),
    "sent range outside": lambda q, c: c["sent_first"].__setitem__(1, len(c["sent"]) + 1),
    "ack frame's items outside": lambda q, c: c["infos"]["item_count"].__setitem__(
        int(np.flatnonzero((c["infos"]["kind"] == fr.ACK) & (c["infos"]["ok"] != 0))[-1]), len(c["items"]) + 1),
}


@pytest.mark.parametrize("rule", list(BAD_STATES))
def test_state_check(rule):
    q, log, call = busy_state()
    call = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in call.items()}
    refs = np.zeros(call["refs"] + 1, dtype=np.uint8)
    good, _ = run(call, q, log, refs)
    assert int(good["results"][0]["stop"]) == fr.FQ_DONE and int(good["results"][0]["frames_acked"]) > 0
    q = q.copy()
    BAD_STATES[rule](q, call)
    got, _ = run(call, q, log, refs)
    res = got["results"][0]
    assert int(res["stop"]) == fr.FQ_BAD_STATE
    zero = np.zeros((), dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    zero["stop"] = fr.FQ_BAD_STATE
    assert res.tobytes() == zero.tobytes()
    same(got["queues_out"][:1], q, "state copied through")
    same(got["log"], log, "log untouched")
    assert not got["ref_acked"].any()


def test_bad_state_beside_good_ones():
    rng = np.random.default_rng(29)
    q, log, calls = E.make_batch(rng, 5, 16, 16, 7, rounds=2)
    got, _ = run(calls[0], q, log)
    q, log = got["queues_out"][:5].copy(), got["log"]
    q["rb_count"][2] = 9
    got, _ = run(calls[1], q, log, nthreads=3)
    assert [int(x) for x in got["results"]["stop"][:5]] == [0, 0, 1, 0, 0]


# ---- float edge cases ----
def feedback_of(total_size, last_feedback, now, li=()):
    q, log = fr.new_frame_queues(1, 8, 8, 0)
    got, _ = run(one_call(q[0], [E.sent_frame(total_size & M32, 5, 0)]), q, log)
    q, log = got["queues_out"][:1].copy(), got["log"]
    if last_feedback is not None:
        q["has_last_feedback"], q["last_feedback_ms"] = 1, last_feedback
    q["li_count"] = len(li)
    for k, (end, length) in enumerate(li):
        q["li_end_time_ms"][0, k], q["li_length"][0, k] = end, length
    got, _ = run(one_call(q[0], acks=[(None, [[0, 1, 0]])], flags=fr.FQ_FEEDBACK, now_ms=now), q, log)
    assert int(got["results"][0]["has_feedback"]) == 1
    return got["results"][0]


def test_receive_rate_edges():
    assert int(feedback_of(48, None, 1000)["receive_rate"]) == 0           # no earlier feedback
    assert int(feedback_of(48, 0, 1000)["receive_rate"]) == 48
    assert int(feedback_of(48, 1000, 1000)["receive_rate"]) == M32         # a difference of 0: x / 0 = inf
    assert int(feedback_of(0, 1000, 1000)["receive_rate"]) == 0            # 0 / 0 = NaN
    assert int(feedback_of(1000, 999, 1000)["receive_rate"]) == 1000000    # 1000 / 0.001
    assert int(feedback_of(M32, 999, 1000)["receive_rate"]) == M32         # clamped
    assert int(feedback_of(7, 2000, 1000)["receive_rate"]) == 0            # the difference wraps: 7 / 1.8e16 s
    r = feedback_of(7, 0, 3)
    assert int(r["rtt_ms"]) == (3 - 5) & E.M64                             # now - last_send_time wraps


def test_loss_rate_edges():
    bits = lambda r: np.array([r["loss_rate"]]).view(np.uint64)[0]
    assert float(feedback_of(1, None, 10)["loss_rate"]) == 0.0
    assert float(feedback_of(1, None, 10, [(10**9, 4)])["loss_rate"]) == 1.0 / 5.0      # (the ack counts in)
    assert float(feedback_of(1, None, 10, [(10**9, M32)])["loss_rate"]) == 1.0 / 4294967295.0   # saturated
    li = [(10**9, 3), (9, 7), (8, 100), (7, 5), (6, 11), (5, 13), (4, 17), (3, 19), (2, 23)]
    r = feedback_of(1, None, 10, li)
    lens = [4] + [x[1] for x in li[1:]]
    w = E.LossIntervalQueue.WEIGHTS
    i0 = i1 = wt = 0.0
    for i in range(8):
        i0 += float(lens[i]) * w[i]
        wt += w[i]
    for i in range(1, 9):
        i1 += float(lens[i]) * w[i - 1]
    assert bits(r) == np.array([wt / max(i0, i1)]).view(np.uint64)[0]


@pytest.mark.parametrize("p,length", [(0.0, M32), (-0.0, 0), (-1.0, 0), (float("nan"), 0), (1e-12, M32), (0.4, 3), (2.0 / 3.0, 2),
                                      (1.0 / 2.5, 3), (0.25, 4), (3.0, 0), (float("inf"), 0), (2.0, 1)])
def test_reset_loss_rate_edges(p, length):
    """(1.0 / p).clamp(0, u32::MAX).round() as u32: 1 / 0.4 = 2.5 rounds away from zero to 3, 1 / 2 = 0.5 to 1."""
    q, log = fr.new_frame_queues(1, 8, 8, 0)
    q["li_count"] = 3
    q["li_end_time_ms"][0, :3], q["li_length"][0, :3] = [30, 20, 10], [5, 6, 7]
    got, _ = run(one_call(q[0], flags=fr.FQ_RESET_LOSS, reset=p), q, log)
    out = got["queues_out"][0]
    assert int(out["li_count"]) == 1 and int(out["li_length"][0]) == length and int(out["li_end_time_ms"][0]) == 30
    assert not out["li_length"][1:].any() and not out["li_end_time_ms"][1:].any()


# ---- records, arguments ----
def test_record_layouts_and_new_queues():
    assert fr.SENT_FRAME_DTYPE.itemsize == 24 and fr.FRAME_QUEUE_DTYPE.itemsize == 192
    assert fr.FRAME_QUEUE_STEP_DTYPE.itemsize == 40 and fr.FRAME_QUEUE_RESULT_DTYPE.itemsize == 80
    q, log = fr.new_frame_queues(3, 5, 3, 7)
    assert q["log_cap"].tolist() == [8] * 3 and q["log_first"].tolist() == [0, 8, 16] and len(log) == 24
    assert q["rb_max_span"].tolist() == [8] * 3 and q["rb_base_id"].tolist() == [7] * 3
    q, log = fr.new_frame_queues(2, 4096, 4096, 0, log_cap=16384)
    assert len(log) == 32768 and q["log_first"].tolist() == [0, 16384]
    with pytest.raises(ValueError):
        fr.new_frame_queues(1, 5, 3, 0, log_cap=12)
    with pytest.raises(ValueError):
        fr.new_frame_queues(1, 5, 4, 0, log_cap=8)


def test_argument_rules():
    q, log = fr.new_frame_queues(1, 8, 8, 0)
    c = one_call(q[0], [E.sent_frame(9, 1, 1)], [(None, [[0, 1, 1]])])
    res, out = np.zeros(1, fr.FRAME_QUEUE_RESULT_DTYPE), np.zeros(1, fr.FRAME_QUEUE_DTYPE)
    refs = np.zeros(4, np.uint8)
    ok = [c["infos"].ctypes.data, 1, c["items"].ctypes.data, 1, c["frame_first"].ctypes.data, c["sent"].ctypes.data, 1,
          c["sent_first"].ctypes.data, q.ctypes.data, c["steps"].ctypes.data, 1, log.ctypes.data, len(log), refs.ctypes.data, 4,
          res.ctypes.data, out.ctypes.data, 1]
    call = lib().ufc_frame_queue_host
    assert call(*ok) == 0 and int(res[0]["frames_acked"]) == 1 and int(out[0]["log_next_id"]) == 1
    log[:] = 0
    for k in (0, 2, 4, 5, 7, 8, 9, 11, 15, 16):   # every required pointer: NULL is an error (four of them: with their counts)
        bad = list(ok)
        bad[k] = None
        assert call(*bad) == UFC_ERR_INVALID_ARG, k
    for k in (1, 3, 6, 10):                        # counts of 2^31 - 1 and beyond
        bad = list(ok)
        bad[k] = (1 << 31) - 1
        assert call(*bad) == UFC_ERR_INVALID_ARG, k
    assert call(*([None, 0, None, 0, None, None, 0, None, None, None, 0, None, 0, None, 0, None, None, 1])) == 0
    nothing = list(ok)                             # no frames, items, records to push, arena or marks: fine
    zeros = np.zeros(2, np.uint64)
    for k, v in ((0, None), (1, 0), (2, None), (3, 0), (4, zeros.ctypes.data), (5, None), (6, 0), (7, zeros.ctypes.data),
                 (13, None), (14, 0)):
        nothing[k] = v
    assert call(*nothing) == 0 and int(res[0]["stop"]) == fr.FQ_DONE
    nothing[11], nothing[12] = None, 0             # (and then the ring is outside the arena)
    assert call(*nothing) == 0 and int(res[0]["stop"]) == fr.FQ_BAD_STATE
    with pytest.raises(ValueError):
        fr.frame_queue_host(c["infos"], c["items"], c["frame_first"][:1], c["sent"], c["sent_first"], q, c["steps"], log)
    with pytest.raises(ValueError):
        fr.frame_queue_host(c["infos"], c["items"], c["frame_first"], c["sent"], c["sent_first"], q, c["steps"],
                            np.zeros(16, np.uint8))
    d = fr.frame_queue_host(c["infos"], c["items"], c["frame_first"], c["sent"], c["sent_first"], q, c["steps"], log)
    assert d["ref_acked"] is None and int(d["results"][0]["frames_acked"]) == 1


# ---- a property run: states that pass the check never make the reference panic ----
def random_state(rng, n_log_extra=0):
    cap = 1 << int(rng.integers(0, 8))
    size = int(rng.integers(0, cap + 1))
    tail = int(rng.integers(0, cap - size + 1))
    ahead = int(rng.integers(0, size + 1))
    length = int(rng.integers(0, ahead + tail + 1))
    q = np.zeros(1, dtype=fr.FRAME_QUEUE_DTYPE)
    nxt = int(rng.integers(0, 1 << 32)) if rng.random() < 0.5 else (M32 - int(rng.integers(0, 100)))
    q["log_next_id"], q["log_base_id"], q["window_base_id"] = nxt, (nxt - length) & M32, (nxt - ahead) & M32
    q["window_size"], q["tail_size"], q["log_cap"] = size, tail, cap
    q["rb_max_span"] = int(rng.choice([size + tail, size + tail + 1, 1 << 31, max(size + tail, cap)]))
    rb = int(rng.integers(0, length + 1))
    q["rb_base_id"] = (int(q["log_base_id"][0]) + rb) & M32
    room = length - rb - 1
    count = min(int(rng.integers(0, 3)), max(room, 0))
    if count:
        d = sorted(rng.choice(np.arange(1, room + 1), size=count, replace=False).tolist())
        for k, x in enumerate(d):
            q["rb_frames"][0, k] = (int(q["rb_base_id"][0]) + x) & M32
    q["rb_count"] = count
    q["rate_limited"], q["has_ack_data"], q["ack_rate_limited"], q["has_last_feedback"] = rng.integers(0, 2, 4)
    q["ack_last_send_time_ms"], q["ack_total_size"], q["last_feedback_ms"] = rng.integers(0, 5000, 3)
    q["li_count"] = int(rng.integers(0, 10))
    q["li_end_time_ms"][0, :int(q["li_count"][0])] = rng.integers(0, 3000, int(q["li_count"][0]))
    q["li_length"][0, :int(q["li_count"][0])] = rng.choice([1, 2, 50, M32 - 1, M32], int(q["li_count"][0]))
    q["log_first"] = int(rng.integers(0, 3))
    log = np.zeros(cap + 2, dtype=fr.SENT_FRAME_DTYPE)
    log["send_time_ms"] = rng.integers(0, 3000, len(log))
    log["size"] = rng.integers(0, 1 << 32, len(log))
    log["ref_first"], log["ref_count"] = rng.integers(0, 40, len(log)), rng.integers(0, 30, len(log))
    log["flags"] = rng.integers(0, 8, len(log))
    return q, log


def random_call(rng, q):
    nxt, base = int(q["log_next_id"][0]), int(q["log_base_id"][0])
    acks = []
    for _ in range(int(rng.integers(0, 4))):
        groups = []
        for _ in range(int(rng.integers(0, 4))):
            gid = (base + int(rng.integers(-3, ((nxt - base) & M32) + 3))) & M32
            bits = int(rng.integers(0, 1 << 32)) >> int(rng.integers(0, 32))
            groups.append([gid, bits, int(rng.integers(0, 2))])
        acks.append(((nxt - int(rng.integers(0, 2 * int(q["window_size"][0]) + 2))) & M32 if rng.random() < 0.8 else None, groups))
    sent = [E.sent_frame(int(rng.integers(0, 1 << 32)), int(rng.integers(0, 3000)), int(rng.integers(0, 2)),
                         int(rng.integers(0, 40)), int(rng.integers(0, 30)), rng.random() < 0.3)
            for _ in range(int(rng.integers(0, 6)))]
    flags = int(rng.integers(0, 32))
    if int(q["li_count"][0]) == 0:
        flags &= ~fr.FQ_RESET_LOSS
    return one_call(q[0], sent, acks, flags, None, int(rng.integers(0, 3000)), int(rng.integers(0, 3000)),
                    float(rng.choice([0.0, 0.3, 1e-12, -1.0])))


def scenario_random_states(seeds=range(400)):
    done = nacks = groups = 0
    for seed in seeds:
        rng = np.random.default_rng(1000 + seed)
        q, log = random_state(rng)
        refs = np.zeros(48, dtype=np.uint8)
        for _ in range(3):
            call = random_call(rng, q)
            assert E.state_ok(q[0], call["steps"][0], len(log), 0, len(call["infos"]), len(call["infos"]), 0, len(call["sent"]),
                              len(call["sent"])), seed
            got, want = run(call, q, log, refs)     # (a ReferencePanic of the restatement would surface here)
            r = want["results"][0]
            assert int(r["stop"]) == fr.FQ_DONE, seed
            done, nacks, groups = done + 1, nacks + int(r["li_nacks"]), groups + int(r["frames_acked"])
            q, log, refs = got["queues_out"][:1].copy(), got["log"], got["ref_acked"]
            if not E.state_ok(q[0], call["steps"][0], len(log), 0, 0, 0, 0, 0, 0):
                break                               # (a held frame acked twice: the header says so)
    assert done > len(seeds)
    return nacks, groups


def test_random_states_never_panic():
    nacks, acked = scenario_random_states()
    assert nacks > 200 and acked > 200, (nacks, acked)


# ---- the step's ballots with their deciding lane on lane 0, on lane 63 and across a tile seam.  The
# same cases, with the same numbers, run in tests/c/queue_host_check.hip under three lane orders.  One connection,
# window 256 / tail 256 at ids through 2^32; a first call pushes 200 frames, the second is the case.  Every case
# asserts on the model's side that its event sits where it was meant to. ----
LANE_BASE = 0xFFFFFFC0


def pushed(times):
    q, log = fr.new_frame_queues(1, 256, 256, LANE_BASE)
    refs = np.zeros(len(times), dtype=np.uint8)
    got, want = run(one_call(q[0], [E.sent_frame(100 + k, t, k & 1, k, 1) for k, t in enumerate(times)]), q, log, refs)
    assert int(want["results"][0]["pushes_taken"]) == len(times)
    return got["queues_out"][:1].copy(), got["log"], got["ref_acked"]


def ack_frames_at_63_64_129(bad_at=None):
    """130 frames of which the ok ack frames sit at 63, 64 and 129, three ids each; the others are not acks or not
    ok, with item ranges that must never be looked at.  bad_at: that ack frame's item range runs past the items."""
    q, log, refs = pushed([10 * k for k in range(200)])
    infos = np.zeros(130, dtype=fr.FRAME_INFO_DTYPE)
    items = []
    for i in range(130):
        if i in (63, 64, 129):
            g = (63, 64, 129).index(i)
            infos[i] = E.ack_info(LANE_BASE + 9 if i == 129 else LANE_BASE, g, 4 - g if i == bad_at else 1)
            items.append(E.group_item(LANE_BASE + 3 * g, 7, 0 if g == 1 else 1))   # (nonces k & 1: 0 1 0 | 1 0 1 | 0 1 0)
        else:
            infos[i]["kind"], infos[i]["ok"] = (fr.DATA, 1) if i % 2 else (fr.ACK, 0)
            infos[i]["item_first"], infos[i]["item_count"] = 0xFFFFFFF0, 100
    call = one_call(q[0])
    call["infos"], call["items"] = infos, np.array(items, dtype=fr.ITEM_DTYPE)
    call["frame_first"] = np.array([0, 130], dtype=np.uint64)
    assert np.flatnonzero((infos["kind"] == fr.ACK) & (infos["ok"] != 0)).tolist() == [63, 64, 129]
    got, want = run(call, q, log, refs)
    r = want["results"][0]
    if bad_at is not None:
        assert int(r["stop"]) == fr.FQ_BAD_STATE and not want["ref_acked"].any()
        return
    assert (int(r["stop"]), int(r["ack_frames"]), int(r["groups"]), int(r["frames_acked"]), int(r["li_acks"]),
            int(r["window_advanced"])) == (fr.FQ_DONE, 3, 3, 9, 9, 9)
    assert want["ref_acked"].tolist() == [1] * 9 + [0] * 191


def scenario_ack_frames_at_63_64_129():
    ack_frames_at_63_64_129()


def scenario_bad_item_range_at_63():
    ack_frames_at_63_64_129(63)


def scenario_bad_item_range_at_64_and_129():
    ack_frames_at_63_64_129(64)
    ack_frames_at_63_64_129(129)


def nack_run_times(lead):
    times = [500 + k for k in range(lead)]
    for k in range(140):
        wobble = (k * 7) % 50
        times.append(1000 if k == 0 else 1049 - wobble if k < 63 else 1050 if k == 63 else 1100 if k == 64 else
                     1149 - wobble if k < 128 else 1150 if k == 128 else 1199 - wobble)
    return times + [3000] * (200 - len(times))


def nack_run(lead):
    """A nack run of 140 ids over a log whose send times go up and down: a forget whose first kept entry is lead +
    140, the first `lead` ids acknowledged in the same call so that the run starts there.  rtt 50: the run's entry 0
    opens an interval (none is open), entries 1..62 fall under it, entry 63 (number 63 of the first nack tile) is
    the first at or after its end and opens the next, entry 64 (number 0 of the next tile) the next, entry 128 the
    last."""
    times = nack_run_times(lead)
    run_times = times[lead:lead + 140]
    assert any(a > b for a, b in zip(run_times, run_times[1:])) and any(a < b for a, b in zip(run_times, run_times[1:]))
    q, log, refs = pushed(times)
    call = one_call(q[0], acks=[(None, [[LANE_BASE + k, 1, k & 1] for k in range(lead)])], flags=fr.FQ_FORGET, rtt_ms=50,
                    thresh_ms=2000)
    # on the model's side: which entries of the run open an interval
    li = E.LossIntervalQueue()
    openers = []
    for k, t in enumerate(run_times):
        before = len(li.entries)
        li.push_nack(t, 50)
        if len(li.entries) != before:
            openers.append(k)
    assert openers == [0, 63, 64, 128]
    got, want = run(call, q, log, refs)
    r, out = want["results"][0], want["queues_out"][0]
    assert (int(r["li_nacks"]), int(r["li_acks"]), int(r["log_culled"]), int(out["li_count"])) == (140, lead, lead + 140, 4)
    assert out["li_length"][:4].tolist() == [12, 64, 1, 63] and out["li_end_time_ms"][:4].tolist() == [1200, 1150, 1100, 1050]


def scenario_nack_run_opens_at_63_and_at_0_of_the_next_tile():
    nack_run(0)


def scenario_nack_run_behind_five_acked_ids():
    nack_run(5)


def forget_kept_at(kept):
    q, log, refs = pushed([10 * k for k in range(200)])
    assert E.load_queue(q[0], log).frame_log.find_expiration_cutoff(10 * kept) == (LANE_BASE + kept) & M32
    _, want = run(one_call(q[0], flags=fr.FQ_FORGET, thresh_ms=10 * kept), q, log, refs)
    r = want["results"][0]
    assert (int(r["log_culled"]), int(r["li_nacks"]), int(want["queues_out"][0]["log_base_id"])) == (kept, kept, (LANE_BASE + kept) & M32)


def scenario_forget_first_kept_at_63_then_64():
    """The expiry cutoff at the last lane of the first tile of 64 entries, at the first of the next, and at 128."""
    for kept in (63, 64, 128):
        forget_kept_at(kept)


LANE_SCENARIOS = [scenario_ack_frames_at_63_64_129, scenario_bad_item_range_at_63, scenario_bad_item_range_at_64_and_129,
                  scenario_nack_run_opens_at_63_and_at_0_of_the_next_tile, scenario_nack_run_behind_five_acked_ids,
                  scenario_forget_first_kept_at_63_then_64]


@pytest.mark.parametrize("scenario", LANE_SCENARIOS, ids=lambda f: f.__name__[9:])
def test_lane_scenarios(scenario):
    scenario()


def test_queue_core_under_sanitizers():
    """tests/c/queue_host_check.hip: the wave-policy core of the frame queue (fq_step, the lanes of a phase run one
    after the other: forwards, backwards, shuffled, and on a carried shared block) as host code under AddressSanitizer and UBSan, against a scalar loop that follows the
    reference entry by entry, on generated traffic and random states over exact-size buffers; a stand-alone program
    (nothing is loaded into Python under a sanitizer)."""
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(HERE, "c", "queue_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "queue_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
