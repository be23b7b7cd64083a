"""CPU: the batched send rate control on the host (ufc_rate_begin_host, ufc_rate_step_host; uflow_amd.frame's
rate_begin_host and rate_step_host) against tests/rate_expect.py, SendRateComp and RecvRateSet restated from the
reference, the hand-traced cases of tests/golden/send_rate_cases.json, and rate_expect.set_cases(), the sets longer
than the four entries a step holds in registers.  Results, states (every double as its 64
bits), every entry of the arena and the gathered flushes are compared as bytes.  tests/test_gpu_rate.py runs the
same comparisons with the device calls in the host calls' place."""
import json
import os

import numpy as np
import pytest

from uflow_amd import frame as fr
from uflow_amd._native import UFC_ERR_INVALID_ARG, UFC_OK, lib

import queue_expect as Q
import rate_expect as E

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "send_rate_cases.json")) as _f:
    GOLDEN = json.load(_f)
M64 = E.M64


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = [k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} records differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


def check_step(b, nthreads=1, in_place=False, gather_in=True, gather_out=True, step=fr.rate_step_host):
    """One ufc_rate_step call on the batch `b` (rate_expect.random_batch's dict), compared byte for byte with the
    restatement.  Returns the outputs."""
    fres, ri = (b["flush_results"], b["result_index"]) if gather_in else (None, None)
    fl, fi = (b["flushes"], b["flush_index"]) if gather_out else (None, None)
    want = E.expect_step(b["states"], b["ticks"], b["fq"], b["entries"], fres, ri, fl, fi)
    states, entries = b["states"].copy(), b["entries"].copy()
    flushes = fl.copy() if fl is not None else None
    got = step(states, b["ticks"], b["fq"], entries, flush_results=fres, result_index=ri, flushes=flushes,
               flush_index=fi, nthreads=nthreads, states_out=states if in_place else None)
    same(got["results"], want["results"], "results")
    same(got["states_out"], want["states_out"], "states_out")
    same(got["entries"], want["entries"], "entries")
    if fl is not None:
        same(got["flushes"], want["flushes"], "flushes")
    if not in_place:
        same(states, b["states"], "states (input)")
    return got


# ---- the goldens ----
def golden_state(case):
    states, entries = fr.new_rate_states(1, case["new"][0], case["new"][1])
    for k, v in case.get("state", {}).items():
        states[0][k] = v
    for k, e in enumerate(case.get("entries", [])):
        entries[k] = (e[0], e[1], e[2], (0, 0, 0))
    states[0]["recv_count"] = len(case.get("entries", []))
    return states, entries


def golden_inputs(step):
    tick = E.make_tick(*step["tick"])
    fq = E.make_feedback(*step["fq"]) if step["fq"] is not None else np.zeros((), dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    return np.array([tick]), np.array([fq])


def check_golden_step(k, step, res, out, entries):
    assert int(res["stop"]) == step["stop"], k
    for key, v in step["result"].items():
        assert int(res[key]) == v, (k, key, int(res[key]))
    for key, v in step["state"].items():
        assert out[key] == v, (k, key, out[key])
    have = [[int(e["timestamp_ms"]), int(e["value"]), int(e["is_initial"])] for e in entries[:int(out["recv_count"])]]
    assert have == step["entries"], (k, have)


CASE_IDS = [c["name"].split(":")[0].split(";")[0] for c in GOLDEN["cases"]]


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=CASE_IDS)
def test_golden_cases_host(case):
    states, entries = golden_state(case)
    for k, step in enumerate(case["steps"]):
        ticks, fq = golden_inputs(step)
        got = fr.rate_step_host(states, ticks, fq, entries)
        check_golden_step(k, step, got["results"][0], got["states_out"][0], got["entries"])
        states = got["states_out"]


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=CASE_IDS)
def test_golden_cases_restatement(case):
    """The same cases through the restated classes, with the reference's own behaviour: where the golden says the
    reference panics or hangs, SendRateComp (without the stall rule) raises exactly that."""
    states, entries = golden_state(case)
    for k, step in enumerate(case["steps"]):
        ticks, fq = golden_inputs(step)
        comp = E.load_comp(states[0], entries, stall_rule=False)
        if int(ticks[0]["flags"]) & fr.RATE_FRAME_SENT:
            comp.notify_frame_sent(int(states[0]["now_ms"]))
        fb = E.FeedbackData(*step["fq"][:3], bool(step["fq"][3])) if step["fq"] is not None else None
        how = "ok"
        try:
            comp.step(int(ticks[0]["now_ms"]), fb, lambda p: None)
        except E.ReferencePanic:
            how = "panic"
        except E.ReferenceHang:
            how = "hang"
        assert how == step["reference"], k
        want = E.expect_step(states, ticks, fq, entries)
        check_golden_step(k, step, want["results"][0], want["states_out"][0], want["entries"])
        assert bool(int(want["results"][0]["flags"]) & fr.RATE_INV_STALLED) == (how == "hang"), k
        states, entries = want["states_out"], want["entries"]


@pytest.mark.parametrize("case", GOLDEN["inverse"], ids=[f"{c['rtt']}-{c['target']}" for c in GOLDEN["inverse"]])
def test_golden_inverse(case):
    p, iterations, stalled = E.eval_tcp_throughput_inv(case["rtt"], case["target"], stall_rule=True)
    assert (p, iterations, stalled) == (case["p"], case["iterations"], case["reference"] == "hang")
    if stalled:
        with pytest.raises(E.ReferenceHang):
            E.eval_tcp_throughput_inv(case["rtt"], case["target"])
    else:
        assert E.eval_tcp_throughput_inv(case["rtt"], case["target"])[0] == p


def test_golden_begin():
    cases = GOLDEN["begin"]
    states, _ = fr.new_rate_states(len(cases), 1000, 1)
    for c, case in enumerate(cases):
        for k, v in case["state"].items():
            states[c][k] = v
    now = np.array([c["now_ms"] for c in cases], dtype=np.uint64)
    extra = np.array([c["extra"] for c in cases], dtype=np.uint32)
    want = E.expect_begin(states, now, extra)
    for got in (want, fr.rate_begin_host(states, now, extra)):
        for c, case in enumerate(cases):
            s = got["steps"][c]
            assert (int(s["flags"]), int(s["rtt_ms"]), int(s["thresh_ms"]), int(s["now_ms"]), float(s["reset_loss_rate"]),
                    int(s["reserved"])) == (case["flags"], case["rtt_ms"], case["thresh_ms"], case["now_ms"],
                                            case["reset_loss_rate"], 0), c
            assert int(got["states_out"][c]["has_reset"]) == 0 and float(got["states_out"][c]["reset_loss_rate"]) == 0.0
    got = fr.rate_begin_host(states, now, extra)
    same(got["steps"], want["steps"], "steps")
    same(got["states_out"], want["states_out"], "states_out")
    none = fr.rate_begin_host(states, now)
    assert (none["steps"]["flags"] == (want["steps"]["flags"] & ~np.uint32(4))).all()


# ---- properties ----
@pytest.mark.parametrize("seed", range(6))
def test_random_states_against_the_restatement(seed):
    """Random passing states and random inputs, every output compared as bits: rtt 0, u64 times near the wrap, NaN,
    infinite and denormal loss rates, receive rates 0 and u32::MAX are all among them."""
    rng = np.random.default_rng(100 + seed)
    b = E.random_batch(rng, 400, recv_cap=1 + seed % 4, spoil=0.0)
    got = check_step(b)
    stops = got["results"]["stop"]
    assert (stops != fr.RATE_BAD_STATE).all() and (stops == fr.RATE_DONE).sum() > 200


def test_random_batches_cover_every_outcome():
    rng = np.random.default_rng(7)
    stops, flags = np.zeros(4, dtype=int), 0
    for k in range(4):
        got = check_step(E.random_batch(rng, 300, recv_cap=1 + k, spoil=0.1), gather_in=k != 1, gather_out=k != 2)
        stops += np.bincount(got["results"]["stop"], minlength=4)
        flags |= int(np.bitwise_or.reduce(got["results"]["flags"]))
    assert (stops > 0).all() and flags == 31, (stops, flags)


# ---- sets past the entries a step holds in registers ----
def test_set_cases():
    """rate_expect.set_cases(): sets of more than kRateHeld = 4 entries, every case between two connections of one
    entry whose rooms adjoin its own.  The facts are asserted on the restatement's output first; then the host calls
    against it, bit for bit, serial and threaded, separate and in place."""
    b = E.set_cases_between_neighbours()
    assert len(b["index"]) == 17 and all(len(v) == 1 for v in b["index"].values())
    for (c,) in b["index"].values():   # a neighbour's room on either side, but at the arena's ends
        lo, cap = int(b["states"][c]["recv_first"]), int(b["states"][c]["recv_cap"])
        beside = [k for k in (c - 1, c + 1) if int(b["states"][k]["recv_first"]) in (lo - 1, lo + cap)]
        assert all(int(b["states"][k]["recv_cap"]) == 1 for k in (c - 1, c + 1)), c
        assert len(beside) == (1 if lo + cap == len(b["entries"]) else 2), c
    want = E.expect_step(b["states"], b["ticks"], b["fq"], b["entries"], None, None, b["flushes"], b["flush_index"])
    E.check_set_facts(b, want)
    seen = E.set_coverage(b, want)
    assert seen["large_done"] == 15 and seen["full_large"] == 2 and seen["moved"] == 2 and seen["largest"] == 23, seen
    one = check_step(b, gather_in=False)
    many = check_step(b, gather_in=False, nthreads=16, in_place=True)
    same(many["entries"], one["entries"], "entries")


@pytest.mark.parametrize("recv_cap", [5, 8, 24])
def test_random_states_large_sets(recv_cap):
    """4 x 400 generated connections in rooms of 5, 8 and 24 entries, a fifth of them full: on the restatement's
    side at least 100 DONE connections that came in with more than 4 entries, a RECV_FULL in such a room, and a
    survivor carried from the part of the set read from memory into a held slot."""
    rng = np.random.default_rng(200 + recv_cap)
    seen = {}
    for k in range(4):
        b = E.random_batch(rng, 400, recv_cap=recv_cap, spoil=0.0, fill=0.2)
        want = E.expect_step(b["states"], b["ticks"], b["fq"], b["entries"], b["flush_results"], b["result_index"],
                             b["flushes"], b["flush_index"])
        for key, v in E.set_coverage(b, want).items():
            seen[key] = max(seen.get(key, 0), v) if key == "largest" else seen.get(key, 0) + v
        check_step(b, in_place=bool(k & 1), nthreads=1 + 15 * (k >> 1))
    assert seen["large_done"] >= 100 and seen["full_large"] >= 1 and seen["moved"] >= 1, seen
    assert seen["largest"] == recv_cap, seen


def test_fill_leaves_the_seeds_alone():
    """fill = 0 draws nothing more: a seed's batch is what it was; and the filled connections are RECV_FULL."""
    a = E.random_batch(np.random.default_rng(5), 50, recv_cap=3)
    b = E.random_batch(np.random.default_rng(5), 50, recv_cap=3, fill=0.0)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    c = E.random_batch(np.random.default_rng(5), 50, recv_cap=3, spoil=0.0, fill=1.0)
    want = E.expect_step(c["states"], c["ticks"], c["fq"], c["entries"])
    assert (want["results"]["stop"] == fr.RATE_RECV_FULL).all()


def bad_state_rules():
    def rule(name, f):
        return pytest.param(f, id=name)
    return [rule("mode", lambda s, n: s.__setitem__("mode", 3)),
            rule("recv_cap_zero", lambda s, n: s.__setitem__("recv_cap", 0)),
            rule("count_over_cap", lambda s, n: s.__setitem__("recv_count", int(s["recv_cap"]) + 1)),
            rule("room_past_arena", lambda s, n: s.__setitem__("recv_first", n - int(s["recv_cap"]) + 1)),
            rule("room_wraps", lambda s, n: s.__setitem__("recv_first", M64)),
            rule("empty_set_in_slow_start", lambda s, n: (s.__setitem__("mode", 1), s.__setitem__("recv_count", 0))),
            rule("empty_set_in_equation", lambda s, n: (s.__setitem__("mode", 2), s.__setitem__("has_rtt_s", 1),
                                                        s.__setitem__("recv_count", 0))),
            rule("equation_without_rtt", lambda s, n: (s.__setitem__("mode", 2), s.__setitem__("has_rtt_s", 0)))]


@pytest.mark.parametrize("spoil", bad_state_rules())
def test_state_check(spoil):
    """Each rule of the header breaks one connection between two good ones: it stops BAD_STATE with its state copied
    through, its entries and its flush untouched and a result that is zero but for `stop`; its neighbours are done."""
    rng = np.random.default_rng(3)
    b = E.random_batch(rng, 3, recv_cap=3, spoil=0.0)
    b["states"]["mode"] = [1, 1, 2]
    b["states"]["has_rtt_s"] = 1
    b["states"]["recv_count"] = 2
    b["fq"]["has_feedback"], b["fq"]["rate_limited"], b["fq"]["rtt_ms"] = 1, 0, 40
    b["flush_index"][:] = [0, 1, 2]
    assert all(E.state_ok(s, len(b["entries"])) for s in b["states"])
    spoil(b["states"][1], len(b["entries"]))
    assert not E.state_ok(b["states"][1], len(b["entries"]))
    got = check_step(b)
    assert got["results"]["stop"].tolist() == [fr.RATE_DONE, fr.RATE_BAD_STATE, fr.RATE_DONE]
    zero = np.zeros((), dtype=fr.RATE_RESULT_DTYPE)
    zero["stop"] = fr.RATE_BAD_STATE
    assert got["results"][1].tobytes() == zero.tobytes()
    assert got["states_out"][1].tobytes() == b["states"][1].tobytes()
    assert int(got["flushes"][1]["flush_alloc"]) == -7


def test_threads_and_aliasing():
    rng = np.random.default_rng(11)
    b = E.random_batch(rng, 1000, recv_cap=3)
    one = check_step(b, nthreads=1)
    many = check_step(b, nthreads=16)
    for k in ("results", "states_out", "entries", "flushes"):
        same(many[k], one[k], k)
    alias = check_step(b, nthreads=16, in_place=True)
    same(alias["states_out"], one["states_out"], "states_out in place")
    now = b["ticks"]["now_ms"].copy()
    want = E.expect_begin(b["states"], now)
    for nthreads in (1, 16):
        got = fr.rate_begin_host(b["states"], now, nthreads=nthreads)
        same(got["steps"], want["steps"], "steps")
        same(got["states_out"], want["states_out"], "states_out")
    states = b["states"].copy()
    got = fr.rate_begin_host(states, now, states_out=states)
    assert got["states_out"] is states
    same(states, want["states_out"], "begin in place")


def test_record_layouts_and_new_states():
    assert fr.RATE_STATE_DTYPE.itemsize == 112 and fr.RATE_TICK_DTYPE.itemsize == 32
    assert fr.RATE_RESULT_DTYPE.itemsize == 56 and fr.RECV_RATE_ENTRY_DTYPE.itemsize == 16
    assert all(fr.RATE_STATE_DTYPE.fields[k][1] % 8 == 0 for k in ("time_last_doubled_ms", "rtt_s", "flush_alloc", "recv_first"))
    states, entries = fr.new_rate_states(3, 12345, 4)
    assert len(entries) == 12 and states["recv_first"].tolist() == [0, 4, 8]
    comp = E.load_comp(states[1], entries)
    fresh = E.SendRateComp(12345)
    for k in ("mode", "send_rate", "max_send_rate", "prev_loss_rate", "nofeedback_exp_ms", "nofeedback_idle", "rtt_s",
              "rtt_ms", "rto_ms", "time_last_doubled_ms"):
        assert getattr(comp, k) == getattr(fresh, k), k
    assert comp.recv_rate_set.entries == [] and int(states[1]["flush_alloc"]) == 0 and not states[1]["has_last_flush"]
    with pytest.raises(ValueError):
        fr.new_rate_states(1, 1, 0)


def test_argument_rules():
    L = lib()
    states, entries = fr.new_rate_states(2, 1000, 2)
    ticks = np.zeros(2, dtype=fr.RATE_TICK_DTYPE)
    fq = np.zeros(2, dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    results = np.zeros(2, dtype=fr.RATE_RESULT_DTYPE)
    out = states.copy()
    steps = np.zeros(2, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
    now = np.zeros(2, dtype=np.uint64)
    idx = np.zeros(2, dtype=np.uint32)
    fres = np.zeros(1, dtype=fr.FLUSH_RESULT_DTYPE)
    fl = np.zeros(1, dtype=fr.FLUSH_DTYPE)
    p = lambda a: a.ctypes.data

    def step(states_p=p(states), ticks_p=p(ticks), fq_p=p(fq), n=2, entries_p=p(entries), n_entries=4, fres_p=None,
             n_fres=0, ri_p=None, fl_p=None, n_fl=0, fi_p=None, results_p=p(results), out_p=p(out)):
        return L.ufc_rate_step_host(states_p, ticks_p, fq_p, n, entries_p, n_entries, fres_p, n_fres, ri_p, fl_p, n_fl,
                                    fi_p, results_p, out_p, 1)

    assert step() == UFC_OK
    assert step(n=0, states_p=None, ticks_p=None, fq_p=None, results_p=None, out_p=None) == UFC_OK
    for null in ("states_p", "ticks_p", "fq_p", "results_p", "out_p", "entries_p"):
        assert step(**{null: None}) == UFC_ERR_INVALID_ARG, null
    assert step(entries_p=None, n_entries=0) == UFC_OK      # (no arena: every state is then a bad one)
    assert results["stop"].tolist() == [fr.RATE_BAD_STATE] * 2
    assert step(fres_p=p(fres), n_fres=1) == UFC_ERR_INVALID_ARG
    assert step(fres_p=p(fres), n_fres=1, ri_p=p(idx)) == UFC_OK
    assert step(fl_p=p(fl), n_fl=1) == UFC_ERR_INVALID_ARG
    idx2 = np.array([0, fr.NO_INDEX], dtype=np.uint32)
    assert step(fl_p=p(fl), n_fl=1, fi_p=p(idx2)) == UFC_OK
    assert step(n=(1 << 31) - 1) == UFC_ERR_INVALID_ARG

    def begin(states_p=p(states), now_p=p(now), extra_p=None, n=2, steps_p=p(steps), out_p=p(out)):
        return L.ufc_rate_begin_host(states_p, now_p, extra_p, n, steps_p, out_p, 1)

    assert begin() == UFC_OK and begin(extra_p=p(idx)) == UFC_OK
    assert begin(n=0, states_p=None, now_p=None, steps_p=None, out_p=None) == UFC_OK
    for null in ("states_p", "now_p", "steps_p", "out_p"):
        assert begin(**{null: None}) == UFC_ERR_INVALID_ARG, null
    assert begin(n=(1 << 31) - 1) == UFC_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        fr.rate_step_host(states, ticks[:1], fq, entries)
    with pytest.raises(ValueError):
        fr.rate_begin_host(states, now[:1])


# ---- order equivalence ----
def run_order_equivalence(n, ticks, seed, begin, step):
    """n connections over `ticks` ticks of queue_expect's traffic, once through HalfConnectionRate (the reference's
    order: acks as they arrive, step() with its immediate reset callback, flush) and once through the batched order
    (begin -> the frame queue's step -> rate step, the reset carried to the next tick).  Every tick the frame queue's
    feedback and the rate control's whole state are compared.  Returns how many feedbacks, resets and expired
    timers were seen."""
    rng = np.random.default_rng(seed)
    window = 16
    refs = [0]
    peers = [Q.Peer(rng, window, 0, 0, refs) for _ in range(n)]
    conns = [E.HalfConnectionRate(window, 0, 200000) for _ in range(n)]
    queues = [Q.FrameQueue(window, window, 0) for _ in range(n)]        # the batched side's frame queues
    states, entries = fr.new_rate_states(n, 200000, 24)
    now = np.zeros(n, dtype=np.uint64)
    pending = [([], False) for _ in range(n)]                           # (frames of the last flush, mark) per connection
    seen = {"feedback": 0, "reset": 0, "nofeedback": 0, "rate_limited": 0}
    for t in range(ticks):
        dt = rng.integers(5, 60, n)
        quiet = rng.random(n) < 0.02
        dt[quiet] += rng.integers(500, 5000, int(quiet.sum()))          # (a pause long enough for the timer)
        now = now + dt.astype(np.uint64)
        acks = [p.acks(loss=0.05 if t % 50 < 40 else 0.4, frames=int(rng.integers(1, 3)), hostile=0.0) if t else []
                for p in peers]
        # the batched order
        extra = np.array([fr.FQ_MARK_RATE_LIMITED if m else 0 for _, m in pending], dtype=np.uint32)
        opened = begin(states, now, extra)
        fq_results = np.zeros(n, dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
        rate_ticks = np.zeros(n, dtype=fr.RATE_TICK_DTYPE)
        for c in range(n):
            s, q = opened["steps"][c], queues[c]
            flags = int(s["flags"])
            rtt = int(s["rtt_ms"]) if flags & fr.FQ_HAS_RTT else None
            if flags & fr.FQ_RESET_LOSS:
                q.reset_loss_rate(float(s["reset_loss_rate"]))
            taken = 0
            for size, nonce in pending[c][0]:
                if q.can_push():
                    q.push(size, int(states[c]["now_ms"]), (), bool(nonce))
                    taken += 1
            if flags & fr.FQ_MARK_RATE_LIMITED:
                q.mark_rate_limited()
            for base, groups in acks[c]:
                for g in groups:
                    q.acknowledge_group(g[0], g[1], bool(g[2]), rtt)
                q.advance_transfer_window(base, rtt)
            q.forget_frames(int(s["thresh_ms"]), rtt)
            fb = q.get_feedback(int(s["now_ms"]))
            if fb is not None:
                fq_results[c] = E.make_feedback(fb.rtt_ms, fb.receive_rate, fb.loss_rate, fb.rate_limited)
            rate_ticks[c] = E.make_tick(int(now[c]), float(dt[c]) / 1000.0, -sum(f[0] for f in pending[c][0][:taken]),
                                        fr.RATE_FRAME_SENT if taken else 0)
        closed = step(opened["states_out"], rate_ticks, fq_results, entries)
        assert (closed["results"]["stop"] == fr.RATE_DONE).all(), t
        states, entries = closed["states_out"], closed["entries"]
        # the reference's order, and the comparison
        for c, h in enumerate(conns):
            for base, groups in acks[c]:
                h.handle_ack_frame(base, groups)
            h.step(int(now[c]), float(dt[c]) / 1000.0)
            fb, r = h.last_feedback, fq_results[c]
            assert (fb is not None) == bool(r["has_feedback"]), (t, c)
            if fb is not None:
                assert (fb.rtt_ms, fb.receive_rate, fb.rate_limited) == (int(r["rtt_ms"]), int(r["receive_rate"]),
                                                                         bool(r["rate_limited"])), (t, c)
                assert np.float64(fb.loss_rate).tobytes() == r["loss_rate"].tobytes(), (t, c)
            want = E.store_comp(h.send_rate_comp, states[c], entries.copy())
            want["now_ms"], want["flush_alloc"], want["has_last_flush"] = h.now_ms, h.flush_alloc, 1
            want["has_reset"], want["reset_loss_rate"] = states[c]["has_reset"], states[c]["reset_loss_rate"]
            assert want.tobytes() == states[c].tobytes(), (t, c, want, states[c])
            first = int(states[c]["recv_first"])
            have = [(int(e["timestamp_ms"]), int(e["value"]), bool(e["is_initial"]))
                    for e in entries[first:first + int(states[c]["recv_count"])]]
            assert have == [(e.timestamp_ms, e.value, e.is_initial) for e in h.send_rate_comp.recv_rate_set.entries], (t, c)
            assert (int(closed["results"][c]["rtt_ms"]), int(closed["results"][c]["rto_ms"])) == (h.rtt_ms, h.rto_ms), (t, c)
            # (the reset the reference applied at once waits in the state: the queues differ by it until the next call)
            if states[c]["has_reset"]:
                seen["reset"] += 1
            flags = int(closed["results"][c]["flags"])
            seen["feedback"] += bool(flags & fr.RATE_FEEDBACK)
            seen["nofeedback"] += bool(flags & fr.RATE_NOFEEDBACK)
            seen["rate_limited"] += bool(fb is not None and fb.rate_limited)
        # the flush: the same frames offered to both sides
        for c, (p, h) in enumerate(zip(peers, conns)):
            count = int(rng.integers(0, 4)) if rng.random() < 0.9 else 0
            p.now = int(now[c])
            before = p.next_id
            frames = [(int(s["size"]), int(s["flags"]) & fr.SENT_NONCE) for s in p.send(count)]
            mark = bool(rng.random() < 0.1)
            sent = h.flush(frames, mark)
            assert sent == ((p.next_id - before) & Q.M32), (t, c)
            pending[c] = (frames, mark)
    return seen


def test_order_equivalence():
    """The batched order (the reset carried as a pending flag into the next frame queue call) against the
    reference's own, on the restatement alone."""
    seen = run_order_equivalence(200, 200, 5, E.expect_begin, E.expect_step)
    assert seen["feedback"] > 2000 and seen["reset"] > 50 and seen["nofeedback"] > 50 and seen["rate_limited"] > 50, seen


def test_order_equivalence_host_calls():
    """The same, shorter, with the host calls in the batched order's place."""
    host_begin = lambda states, now, extra: fr.rate_begin_host(states, now, extra)
    host_step = lambda states, ticks, fq, entries: fr.rate_step_host(states, ticks, fq, entries.copy())
    seen = run_order_equivalence(100, 100, 6, host_begin, host_step)
    assert seen["feedback"] > 500 and seen["reset"] > 10, seen


def test_rate_core_under_sanitizers():
    """tests/c/rate_host_check.hip: the core of the send rate control (rate_step, rate_begin) as host code under
    AddressSanitizer and UBSan, on the goldens' shapes and a random batch over exact-size buffers; a stand-alone
    program (nothing is loaded into Python under a sanitizer)."""
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(HERE, "c", "rate_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rate_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
