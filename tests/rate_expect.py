"""What ufc_rate_begin_* and ufc_rate_step_* must compute: the reference's send rate control restated in Python, class
for class and line for line from the Rust: SendRateComp (src/half_connection/send_rate.rs), RecvRateSet
(recv_rate_set.rs), and the parts of HalfConnection that drive them (half_connection/mod.rs: step :165-193,
fill_flush_alloc :200-215, handle_ack_frame :154-163, the emit callback of emit_data_frames :342-347).  The release
build is restated: integer arithmetic wraps where the reference writes plain operators, and debug_assert!s are gone.

Where the reference panics, ReferencePanic is raised; where it would go round its bisection for ever, ReferenceHang.
expect_begin / expect_step restate the batched calls on top of these classes, with the header's answers for the two.
HalfConnectionRate runs a connection in the reference's own order (acks, step with the immediate reset callback,
flush) on queue_expect's FrameQueue; tests/test_rate_cpu.py holds the batched order against it."""
import math

import numpy as np

from uflow_amd import frame as fr

import queue_expect as Q
from queue_expect import M32, M64, ReferencePanic, as_u32, f64_div, unwrap

MSS = fr.MAX_FRAME_SIZE
INITIAL_TCP_WINDOW = 4380
MINIMUM_RATE = MSS // 64
INITIAL_RTT_ESTIMATE_MS = 150
INITIAL_RTO_ESTIMATE_MS = 4 * INITIAL_RTT_ESTIMATE_MS
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


class ReferenceHang(Exception):
    pass


# ---- Rust's float arithmetic ----
def f64_round(v):          # f64::round: half away from zero, either sign
    if v != v or math.isinf(v):
        return v
    t = float(math.trunc(v))
    d = v - t
    return t + 1.0 if d >= 0.5 else t - 1.0 if d <= -0.5 else t


def f64_max(a, b):         # f64::max: a NaN gives the other operand
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def as_u64(v):             # `as u64`: saturating, NaN is 0
    if v != v or v <= 0.0:
        return 0
    return M64 if v >= 18446744073709551616.0 else int(v)


def as_isize(v):           # `as isize`: saturating, NaN is 0
    if v != v:
        return 0
    if v >= 9223372036854775808.0:
        return I64_MAX
    if v <= -9223372036854775808.0:
        return I64_MIN
    return int(v)


def f64_mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def f64_sqrt(v):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v)))   # (IEEE: correctly rounded; a negative or NaN operand gives NaN)


def saturating_mul2(v):
    return min(v * 2, M32)


# ---- send_rate.rs:16-59 ----
def s_to_ms(v_s):
    return as_u64(f64_round(f64_max(f64_mul(v_s, 1000.0), 0.0)))


def ms_to_s(v_ms):
    return float(v_ms) / 1000.0


def eval_tcp_throughput(rtt, p):
    s = float(MSS)
    f_p = f64_sqrt(f64_mul(p, 2.0) / 3.0) + f64_mul(f64_mul(f64_mul(12.0, f64_sqrt(f64_mul(p, 3.0) / 8.0)), p),
                                                    1.0 + f64_mul(f64_mul(32.0, p), p))
    return as_u32(f64_div(s, f64_mul(rtt, f_p)))


def eval_tcp_throughput_inv(rtt, target_rate_bps, stall_rule=False):
    """Returns (c, iterations, stalled).  The reference's loop has no exit for a midpoint that no longer moves; it is
    ReferenceHang here, or with stall_rule the batched call's answer (that midpoint, stalled = True)."""
    delta = as_u32(target_rate_bps * 0.05)
    a, b = 0.0, 1.0
    iterations = 0
    while True:
        c = (b + a) / 2.0
        rate = eval_tcp_throughput(rtt, c)
        iterations += 1
        if rate > target_rate_bps:
            if rate - target_rate_bps <= delta:
                return c, iterations, False
            moved = c != a and c != b
            a = c
        elif rate < target_rate_bps:
            if target_rate_bps - rate <= delta:
                return c, iterations, False
            moved = c != a and c != b
            b = c
        else:
            return c, iterations, False
        if not moved:      # (a, b) is what it was an iteration ago: every later one repeats this one
            if stall_rule:
                return c, iterations, True
            raise ReferenceHang(f"eval_tcp_throughput_inv({rtt!r}, {target_rate_bps}) stays at {c!r}")


def compute_initial_send_rate(rtt_s):
    return as_u32(f64_div(float(INITIAL_TCP_WINDOW), rtt_s))


def compute_initial_loss_send_rate(rtt_s):
    return as_u32(f64_div(float(MSS // 2), rtt_s))


# ---- recv_rate_set.rs ----
class RecvEntry:
    def __init__(self, value, timestamp_ms, is_initial):
        self.value, self.timestamp_ms, self.is_initial = value, timestamp_ms, is_initial


class RecvRateSet:
    def __init__(self):
        self.entries = []

    def reset_initial(self, now_ms):
        self.entries = [RecvEntry(M32, now_ms, True)]

    def replace_max(self, now_ms, recv_rate):
        self.entries = [e for e in self.entries if not e.is_initial]
        max_rate = recv_rate if not self.entries else max(self.max(), recv_rate)
        self.reset(now_ms, max_rate)
        return max_rate

    def reset(self, now_ms, recv_rate):
        self.entries = [RecvEntry(recv_rate, now_ms, False)]

    def rate_limited_update(self, now_ms, recv_rate, rtt_ms):
        self.entries.append(RecvEntry(recv_rate, now_ms, False))
        self.entries = [e for e in self.entries if ((now_ms - e.timestamp_ms) & M64) < ((2 * rtt_ms) & M64)]
        return self.max()

    def loss_increase_update(self, now_ms, recv_rate):
        for e in self.entries:
            e.value //= 2
        return self.replace_max(now_ms, as_u32(recv_rate * 0.85))

    def data_limited_update(self, now_ms, recv_rate):
        return self.replace_max(now_ms, recv_rate)

    def max(self):
        max_rate = unwrap(self.entries[0] if self.entries else None).value
        for e in self.entries[1:]:
            if e.value > max_rate:
                max_rate = e.value
        return max_rate


# ---- send_rate.rs:61-387 ----
class FeedbackData:
    def __init__(self, rtt_ms, receive_rate, loss_rate, rate_limited):
        self.rtt_ms, self.receive_rate, self.loss_rate, self.rate_limited = rtt_ms, receive_rate, loss_rate, rate_limited


AWAIT_SEND, SLOW_START, THROUGHPUT_EQN = 0, 1, 2


class SendRateComp:
    def __init__(self, max_send_rate, stall_rule=False):
        self.prev_loss_rate = 0.0
        self.nofeedback_exp_ms = None
        self.nofeedback_idle = False
        self.mode = AWAIT_SEND
        self.time_last_doubled_ms = None   # SlowStartState
        self.send_rate_tcp = 0             # ThroughputEqnState
        self.send_rate = MSS
        self.max_send_rate = max_send_rate
        self.recv_rate_set = RecvRateSet()
        self.rtt_s = None
        self.rtt_ms = None
        self.rto_ms = None
        self.stall_rule = stall_rule       # (not in the reference: the batched call's answer to the endless loop)
        self.trace = {}                    # (not in the reference: what the last step() did, for the result's flags)

    def notify_frame_sent(self, now_ms):
        if self.mode == AWAIT_SEND:
            self.nofeedback_exp_ms = (now_ms + 2000) & M64
            self.mode = SLOW_START
            self.time_last_doubled_ms = None
            self.recv_rate_set.reset_initial(now_ms)
        self.nofeedback_idle = False

    def step(self, now_ms, feedback, reset_loss_rate):
        self.trace = {"flags": 0, "iterations": 0}
        if self.mode == AWAIT_SEND:
            return
        if feedback is not None:
            self.handle_feedback(now_ms, feedback, reset_loss_rate)
        elif self.nofeedback_exp_ms is not None:
            if now_ms >= self.nofeedback_exp_ms:
                self.nofeedback_expired(now_ms)

    def handle_feedback(self, now_ms, feedback, reset_loss_rate):
        self.trace["flags"] |= fr.RATE_FEEDBACK
        rtt_sample_s = ms_to_s(feedback.rtt_ms)
        recv_rate = feedback.receive_rate
        loss_rate = feedback.loss_rate
        rate_limited = feedback.rate_limited
        rtt_s, rtt_ms = self.update_rtt(rtt_sample_s)
        rto_s = self.update_rto(rtt_s, self.send_rate)
        loss_increase = loss_rate > self.prev_loss_rate
        if rate_limited:
            max_val = self.recv_rate_set.rate_limited_update(now_ms, recv_rate, rtt_ms)
            recv_limit = saturating_mul2(max_val)
        elif loss_increase:
            recv_limit = self.recv_rate_set.loss_increase_update(now_ms, recv_rate)
        else:
            max_val = self.recv_rate_set.data_limited_update(now_ms, recv_rate)
            recv_limit = saturating_mul2(max_val)
        self.prev_loss_rate = loss_rate
        if self.mode == SLOW_START:
            if loss_increase:
                if self.time_last_doubled_ms is None:
                    send_rate_target = compute_initial_loss_send_rate(rtt_s)
                else:
                    send_rate_target = self.send_rate // 2
                initial_p, iterations, stalled = eval_tcp_throughput_inv(rtt_s, send_rate_target, self.stall_rule)
                self.trace["iterations"] = iterations
                self.trace["flags"] |= fr.RATE_RESET_ISSUED | fr.RATE_ENTERED_EQN | (fr.RATE_INV_STALLED if stalled else 0)
                reset_loss_rate(initial_p)
                self.send_rate = max(min(send_rate_target, recv_limit), MINIMUM_RATE)
                self.mode = THROUGHPUT_EQN
                self.time_last_doubled_ms = None
                self.send_rate_tcp = send_rate_target
            else:
                initial_rate = compute_initial_send_rate(rtt_s)
                if self.time_last_doubled_ms is not None:
                    if ((now_ms - self.time_last_doubled_ms) & M64) >= rtt_ms:
                        self.time_last_doubled_ms = now_ms
                        self.send_rate = max(min((2 * self.send_rate) & M32, recv_limit), initial_rate)
                else:
                    self.time_last_doubled_ms = now_ms
                    self.send_rate = initial_rate
        elif self.mode == THROUGHPUT_EQN:
            self.send_rate_tcp = eval_tcp_throughput(rtt_s, loss_rate)
            self.send_rate = max(min(self.send_rate_tcp, recv_limit), MINIMUM_RATE)
        else:
            raise ReferencePanic("panic!()")
        self.send_rate = min(self.send_rate, self.max_send_rate)
        self.nofeedback_exp_ms = (now_ms + s_to_ms(rto_s)) & M64
        self.nofeedback_idle = True

    def nofeedback_expired(self, now_ms):
        self.trace["flags"] |= fr.RATE_NOFEEDBACK
        if self.mode == SLOW_START:
            if self.rtt_s is not None:
                recover_rate = compute_initial_send_rate(self.rtt_s)
                if self.nofeedback_idle and self.send_rate < ((2 * recover_rate) & M32):
                    pass
                else:
                    self.send_rate = max(self.send_rate // 2, MINIMUM_RATE)
            else:
                self.send_rate = max(self.send_rate // 2, MINIMUM_RATE)
        elif self.mode == THROUGHPUT_EQN:
            rtt_s = unwrap(self.rtt_s)
            recover_rate = compute_initial_send_rate(rtt_s)
            recv_rate = self.recv_rate_set.max()
            if self.nofeedback_idle and recv_rate < recover_rate:
                pass
            else:
                current_limit = min(self.send_rate_tcp, saturating_mul2(recv_rate))
                new_limit = max(current_limit // 2, MINIMUM_RATE)
                self.recv_rate_set.reset(now_ms, new_limit // 2)
                self.send_rate = min(self.send_rate_tcp, new_limit)
        else:
            raise ReferencePanic("panic!()")
        rto_s = self.update_rto(self.rtt_s if self.rtt_s is not None else 0.0, self.send_rate)
        self.nofeedback_exp_ms = (now_ms + s_to_ms(rto_s)) & M64
        self.nofeedback_idle = True

    def update_rtt(self, rtt_sample_s):
        RTT_ALPHA = 0.1
        if self.rtt_s is not None:
            new_rtt_s = f64_mul(1.0 - RTT_ALPHA, self.rtt_s) + f64_mul(RTT_ALPHA, rtt_sample_s)
        else:
            new_rtt_s = rtt_sample_s
        new_rtt_ms = s_to_ms(new_rtt_s)
        self.rtt_s = new_rtt_s
        self.rtt_ms = new_rtt_ms
        return new_rtt_s, new_rtt_ms

    def update_rto(self, rtt_s, send_rate):
        rto_s = f64_max(f64_mul(4.0, rtt_s), f64_div(float(2 * MSS), float(send_rate)))
        self.rto_ms = s_to_ms(rto_s)
        return rto_s


def fill_flush_alloc(flush_alloc, send_rate, rtt_s, delta_time):
    """mod.rs:200-215 behind its `if let Some(time_last_flushed)`."""
    rate = float(send_rate)
    new_bytes = as_isize(f64_round(f64_mul(rate, delta_time)))
    alloc_max = as_isize(f64_round(f64_mul(rate, rtt_s if rtt_s is not None else 0.0)))
    return min(max(min(flush_alloc + new_bytes, I64_MAX), I64_MIN), alloc_max)


# ---- a connection in the reference's own order ----
class HalfConnectionRate:
    """The fields and calls of HalfConnection that touch the frame queue and the rate control, in mod.rs's order."""

    def __init__(self, window_size, base_id, max_send_rate):
        self.frame_queue = Q.FrameQueue(window_size, window_size, base_id)   # (mod.rs:89)
        self.send_rate_comp = SendRateComp(max_send_rate)
        self.now_ms = self.rtt_ms = self.rto_ms = 0
        self.has_last_flush = False
        self.flush_alloc = 0
        self.last_feedback = None          # (not in the reference: what step() handed to the rate control)

    def handle_ack_frame(self, frame_window_base_id, groups):
        rtt_ms = self.send_rate_comp.rtt_ms
        for base_id, bitfield, nonce in groups:
            self.frame_queue.acknowledge_group(base_id, bitfield, bool(nonce), rtt_ms)
        self.frame_queue.advance_transfer_window(frame_window_base_id, rtt_ms)

    def step(self, now_ms, delta_time_s):
        rtt_ms = self.send_rate_comp.rtt_ms if self.send_rate_comp.rtt_ms is not None else INITIAL_RTT_ESTIMATE_MS
        rto_ms = self.send_rate_comp.rto_ms if self.send_rate_comp.rto_ms is not None else INITIAL_RTO_ESTIMATE_MS
        self.now_ms, self.rtt_ms, self.rto_ms = now_ms, rtt_ms, rto_ms
        self.frame_queue.forget_frames(max(now_ms - ((rtt_ms * 4) & M64), 0), self.send_rate_comp.rtt_ms)
        if self.has_last_flush:
            self.flush_alloc = fill_flush_alloc(self.flush_alloc, self.send_rate_comp.send_rate,
                                                self.send_rate_comp.rtt_s, delta_time_s)
        self.has_last_flush = True
        self.last_feedback = self.frame_queue.get_feedback(now_ms)
        self.send_rate_comp.step(now_ms, self.last_feedback, self.frame_queue.reset_loss_rate)

    def flush(self, frames, mark_rate_limited=False):
        """emit_data_frames for `frames` = [(size, nonce), ...]: the emitter pushes while the window takes frames
        (emit.rs); its callback (:342-347) runs per frame.  Returns how many went out."""
        sent = 0
        for size, nonce in frames:
            if not self.frame_queue.can_push():
                break
            self.frame_queue.push(size, self.now_ms, (), bool(nonce))
            self.send_rate_comp.notify_frame_sent(self.now_ms)
            self.flush_alloc -= size
            sent += 1
        if mark_rate_limited:
            self.frame_queue.mark_rate_limited()
        return sent


# ---- records ----
def state_ok(s, n_entries):
    """The batched call's state check, restated from the header."""
    if int(s["mode"]) > 2 or int(s["recv_cap"]) == 0 or int(s["recv_count"]) > int(s["recv_cap"]):
        return False
    if int(s["recv_first"]) + int(s["recv_cap"]) > n_entries:
        return False
    if int(s["mode"]) != AWAIT_SEND and int(s["recv_count"]) == 0:
        return False
    if int(s["mode"]) == THROUGHPUT_EQN and not s["has_rtt_s"]:
        return False
    return True


def load_comp(s, entries, stall_rule=True):
    """The SendRateComp a ufc_rate_state record and its entries stand for."""
    c = SendRateComp(int(s["max_send_rate"]), stall_rule)
    c.mode = int(s["mode"])
    c.send_rate = int(s["send_rate"])
    c.prev_loss_rate = float(s["prev_loss_rate"])
    c.nofeedback_idle = bool(s["nofeedback_idle"])
    if c.mode == SLOW_START and s["has_time_last_doubled"]:
        c.time_last_doubled_ms = int(s["time_last_doubled_ms"])
    if c.mode == THROUGHPUT_EQN:
        c.send_rate_tcp = int(s["send_rate_tcp"])
    if s["has_nofeedback_exp"]:
        c.nofeedback_exp_ms = int(s["nofeedback_exp_ms"])
    if s["has_rtt_s"]:
        c.rtt_s = float(s["rtt_s"])
    if s["has_rtt_ms"]:
        c.rtt_ms = int(s["rtt_ms"])
    if s["has_rto_ms"]:
        c.rto_ms = int(s["rto_ms"])
    first = int(s["recv_first"])
    for e in entries[first:first + int(s["recv_count"])]:
        c.recv_rate_set.entries.append(RecvEntry(int(e["value"]), int(e["timestamp_ms"]), bool(e["is_initial"])))
    return c


def store_comp(c, s_in, entries):
    """The record of a SendRateComp after a step (the HalfConnection fields are the caller's), its entries written."""
    s = s_in.copy()
    s["mode"], s["send_rate"], s["max_send_rate"] = c.mode, c.send_rate, c.max_send_rate
    s["send_rate_tcp"] = c.send_rate_tcp if c.mode == THROUGHPUT_EQN else 0
    tld = c.time_last_doubled_ms if c.mode == SLOW_START else None
    for key, flag, v in (("time_last_doubled_ms", "has_time_last_doubled", tld),
                         ("nofeedback_exp_ms", "has_nofeedback_exp", c.nofeedback_exp_ms),
                         ("rtt_s", "has_rtt_s", c.rtt_s), ("rtt_ms", "has_rtt_ms", c.rtt_ms),
                         ("rto_ms", "has_rto_ms", c.rto_ms)):
        s[flag] = 0 if v is None else 1
        s[key] = 0 if v is None else v
    s["nofeedback_idle"] = 1 if c.nofeedback_idle else 0
    s["prev_loss_rate"] = c.prev_loss_rate
    first = int(s["recv_first"])
    for k, e in enumerate(c.recv_rate_set.entries):
        entries[first + k] = (e.timestamp_ms, e.value, 1 if e.is_initial else 0, (0, 0, 0))
    s["recv_count"] = len(c.recv_rate_set.entries)
    return s


def expect_begin(states, now_ms, extra_flags=None):
    """ufc_rate_begin_*: returns {"steps", "states_out"}."""
    n = len(states)
    steps = np.zeros(n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
    out = states.copy()
    for c in range(n):
        s = states[c]
        has_rtt = bool(s["has_rtt_ms"])
        rtt = int(s["rtt_ms"]) if has_rtt else INITIAL_RTT_ESTIMATE_MS
        now = int(now_ms[c])
        flags = fr.FQ_FORGET | fr.FQ_FEEDBACK | (fr.FQ_HAS_RTT if has_rtt else 0) | \
            (fr.FQ_RESET_LOSS if s["has_reset"] else 0) | (int(extra_flags[c]) if extra_flags is not None else 0)
        steps[c] = Q.make_step(flags, int(s["rtt_ms"]) if has_rtt else 0, max(now - ((rtt * 4) & M64), 0), now,
                               float(s["reset_loss_rate"]) if s["has_reset"] else 0.0)
        out[c]["has_reset"], out[c]["reset_loss_rate"] = 0, 0.0
    return {"steps": steps, "states_out": out}


def expect_connection(s, tick, fq, entries, last_flush=None):
    """One connection of ufc_rate_step_*.  last_flush = (alloc_left, frame_count) of the gathered flush result, or
    None.  entries is updated in place when the connection is not stopped.  Returns (result, state_out)."""
    res = np.zeros((), dtype=fr.RATE_RESULT_DTYPE)
    if not state_ok(s, len(entries)):
        res["stop"] = fr.RATE_BAD_STATE
        return res, s.copy()
    comp = load_comp(s, entries)
    # 1. the last flush's accounting
    alloc = int(s["flush_alloc"])
    sent = bool(int(tick["flags"]) & fr.RATE_FRAME_SENT)
    if last_flush is not None:
        alloc = int(last_flush[0])
        sent = sent or int(last_flush[1]) > 0
    alloc = (alloc + int(tick["alloc_adjust"]) - I64_MIN) % (1 << 64) + I64_MIN
    if sent:
        comp.notify_frame_sent(int(s["now_ms"]))
    # 2. step(): mod.rs:168-175
    now = int(tick["now_ms"])
    rtt_ms = comp.rtt_ms if comp.rtt_ms is not None else INITIAL_RTT_ESTIMATE_MS
    rto_ms = comp.rto_ms if comp.rto_ms is not None else INITIAL_RTO_ESTIMATE_MS
    # 3. fill_flush_alloc
    if s["has_last_flush"]:
        alloc = fill_flush_alloc(alloc, comp.send_rate, comp.rtt_s, float(tick["delta_time_s"]))
    # 4. the rate step
    feedback = None
    if fq["has_feedback"]:
        feedback = FeedbackData(int(fq["rtt_ms"]), int(fq["receive_rate"]), float(fq["loss_rate"]), bool(fq["rate_limited"]))
    reset = []
    try:
        comp.step(now, feedback, reset.append)
    except ReferencePanic:
        res["stop"] = fr.RATE_REF_PANIC
        return res, s.copy()
    if len(comp.recv_rate_set.entries) > int(s["recv_cap"]):
        res["stop"] = fr.RATE_RECV_FULL
        return res, s.copy()
    # 5. outputs
    out = store_comp(comp, s, entries)
    out["now_ms"], out["flush_alloc"], out["has_last_flush"] = now, alloc, 1
    if reset:
        out["has_reset"], out["reset_loss_rate"] = 1, reset[0]
    else:
        out["has_reset"] = 1 if s["has_reset"] else 0
        out["reset_loss_rate"] = float(s["reset_loss_rate"]) if s["has_reset"] else 0.0
    res["mode"], res["now_ms"], res["rtt_ms"], res["rto_ms"], res["flush_alloc"] = comp.mode, now, rtt_ms, rto_ms, alloc
    res["send_rate"], res["flags"], res["inv_iterations"] = comp.send_rate, comp.trace["flags"], comp.trace["iterations"]
    res["recv_count"] = out["recv_count"]
    return res, out


def expect_step(states, ticks, fq_results, entries, flush_results=None, result_index=None, flushes=None, flush_index=None):
    """ufc_rate_step_*: returns {"results", "states_out", "entries", "flushes"}; the inputs are left as they are."""
    n = len(states)
    entries = entries.copy()
    flushes = flushes.copy() if flushes is not None else None
    results = np.zeros(n, dtype=fr.RATE_RESULT_DTYPE)
    out = states.copy()
    for c in range(n):
        last = None
        if flush_results is not None and int(result_index[c]) < len(flush_results):
            r = flush_results[int(result_index[c])]
            last = (int(r["alloc_left"]), int(r["frame_count"]))
        results[c], out[c] = expect_connection(states[c], ticks[c], fq_results[c], entries, last)
        if flushes is not None and int(results[c]["stop"]) == fr.RATE_DONE and int(flush_index[c]) < len(flushes):
            flushes[int(flush_index[c])]["flush_alloc"] = int(results[c]["flush_alloc"])
    return {"results": results, "states_out": out, "entries": entries, "flushes": flushes}


def make_tick(now_ms, delta_time_s=0.0, alloc_adjust=0, flags=0):
    t = np.zeros((), dtype=fr.RATE_TICK_DTYPE)
    t["now_ms"], t["delta_time_s"], t["alloc_adjust"], t["flags"] = now_ms, delta_time_s, alloc_adjust, flags
    return t


def make_feedback(rtt_ms, receive_rate, loss_rate, rate_limited=False):
    f = np.zeros((), dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    f["has_feedback"], f["rtt_ms"], f["receive_rate"], f["loss_rate"], f["rate_limited"] = 1, rtt_ms, receive_rate, \
        loss_rate, 1 if rate_limited else 0
    return f


# ---- generated batches ----
EDGE_U64 = [0, 1, 2, 999, 150, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, M64 - 2000, M64 - 1, M64]
EDGE_F64 = [0.0, -0.0, 1.0, 0.5, 1e-3, 1e-9, 5e-324, 2.2250738585072014e-308, 1e-310, float("inf"), float("-inf"),
            float("nan"), -1.0, 1e300, 2.0 / 3.0, 0.1]
EDGE_U32 = [0, 1, 22, 23, 24, 46, 1472, 4380, (1 << 31) - 1, 1 << 31, M32 - 1, M32]


def _u64(rng, near=None):
    u = rng.random()
    if u < 0.15:
        return EDGE_U64[int(rng.integers(0, len(EDGE_U64)))]
    if near is not None and u < 0.8:
        return (near + int(rng.integers(-3000, 3000))) & M64
    return int(rng.integers(0, 1 << 40))


def _u32(rng):
    u = rng.random()
    if u < 0.2:
        return EDGE_U32[int(rng.integers(0, len(EDGE_U32)))]
    return int(10 ** rng.uniform(0, 9.6)) & M32


def _f64(rng, lo=-6.0, hi=0.0):
    u = rng.random()
    if u < 0.15:
        return EDGE_F64[int(rng.integers(0, len(EDGE_F64)))]
    return float(10 ** rng.uniform(lo, hi))


def random_batch(rng, n, recv_cap=4, spoil=0.05):
    """n random connections for one ufc_rate_step call: states over all three modes that pass the state check (but
    for a fraction `spoil`, broken in one rule each), their sets, ticks, frame queue results with and without
    feedback, timers expired or not, and both gathers.  The inputs include rtt 0 (REF_PANIC with a rate-limited
    feedback), sets at their capacity (RECV_FULL), times near the u64 wrap, NaN, infinite and denormal loss rates,
    receive rates 0 and u32::MAX.  Returns a dict of arrays."""
    states, entries = fr.new_rate_states(n, 0, recv_cap)
    slack = int(rng.integers(0, 5))
    entries = np.zeros(len(entries) + slack, dtype=fr.RECV_RATE_ENTRY_DTYPE)
    ticks = np.zeros(n, dtype=fr.RATE_TICK_DTYPE)
    fq = np.zeros(n, dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    for c in range(n):
        s = states[c]
        base = _u64(rng)
        mode = int(rng.integers(0, 3))
        s["mode"] = mode
        s["send_rate"], s["max_send_rate"] = _u32(rng), _u32(rng) if rng.random() < 0.5 else M32
        s["send_rate_tcp"] = _u32(rng)
        for k in ("has_time_last_doubled", "has_nofeedback_exp", "nofeedback_idle", "has_rtt_s", "has_rtt_ms",
                  "has_rto_ms", "has_last_flush", "has_reset"):
            s[k] = int(rng.choice([0, 1, 1, 1, 2, 255]))
        if mode == THROUGHPUT_EQN and not s["has_rtt_s"]:
            s["has_rtt_s"] = 1
        s["time_last_doubled_ms"] = _u64(rng, base)
        s["prev_loss_rate"] = _f64(rng)
        s["nofeedback_exp_ms"] = _u64(rng, base)
        s["rtt_s"] = _f64(rng, -4.0, 1.0)
        s["rtt_ms"], s["rto_ms"] = _u64(rng, 100), _u64(rng, 400)
        s["now_ms"] = base
        s["flush_alloc"] = [0, -1, 1, I64_MIN, I64_MAX, int(rng.integers(-100000, 100000))][int(rng.integers(0, 6))]
        s["reset_loss_rate"] = _f64(rng)
        count = int(rng.integers(0 if mode == AWAIT_SEND else 1, recv_cap + 1))
        s["recv_count"] = count
        first = int(s["recv_first"])
        for k in range(recv_cap):   # (the room behind the count holds rubbish the call must leave alone)
            entries[first + k] = (_u64(rng, base), _u32(rng), 1 if k == 0 and rng.random() < 0.3 else 0,
                                  (0, 0, 0) if k < count else (7, 7, 7))
        t = ticks[c]
        t["now_ms"] = (base + int(rng.integers(0, 3000))) & M64 if rng.random() < 0.9 else _u64(rng)
        t["delta_time_s"] = _f64(rng, -4.0, 1.0) if rng.random() < 0.8 else float(rng.choice([1e18, -5.0, 1e-320]))
        t["alloc_adjust"] = [0, 0, -1472, -28, I64_MIN, I64_MAX, int(rng.integers(-5000, 1))][int(rng.integers(0, 7))]
        t["flags"] = int(rng.integers(0, 4))
        f = fq[c]
        if rng.random() < 0.6:
            f["has_feedback"] = int(rng.choice([1, 1, 1, 3]))
            f["rtt_ms"] = [0, 0, 1, int(rng.integers(0, 2000)), _u64(rng)][int(rng.integers(0, 5))]
            f["receive_rate"] = _u32(rng)
            f["loss_rate"] = _f64(rng)
            f["rate_limited"] = int(rng.random() < 0.4)
        else:   # (everything but has_feedback must be ignored)
            f["rtt_ms"], f["receive_rate"], f["loss_rate"], f["rate_limited"] = 5, 5, 0.5, 1
        f["stop"], f["window_room"] = int(rng.integers(0, 2)), int(rng.integers(0, 100))
        if rng.random() < spoil:
            rule = int(rng.integers(0, 6))
            if rule == 0:
                s["mode"] = [3, 255, M32][int(rng.integers(0, 3))]
            elif rule == 1:
                s["recv_cap"] = 0
            elif rule == 2:
                s["recv_count"] = recv_cap + 1 + int(rng.integers(0, 3))
            elif rule == 3:
                s["recv_first"] = [len(entries) - recv_cap + 1, len(entries), M64, M64 - recv_cap + 1][int(rng.integers(0, 4))]
            elif rule == 4:
                s["mode"], s["recv_count"] = int(rng.integers(1, 3)), 0
            else:
                s["mode"], s["has_rtt_s"] = THROUGHPUT_EQN, 0
    m = max(1, n // 2 + 1)
    flush_results = np.zeros(m, dtype=fr.FLUSH_RESULT_DTYPE)
    flush_results["alloc_left"] = rng.integers(-3000, 100000, m)
    flush_results["frame_count"] = rng.integers(0, 3, m)
    flush_results["frame_first"], flush_results["items_packed"] = 9, 9
    result_index = rng.integers(0, m + 2, n).astype(np.uint32)
    result_index[rng.random(n) < 0.3] = fr.NO_INDEX
    flushes = np.zeros(n + 3, dtype=fr.FLUSH_DTYPE)
    flushes["flush_alloc"], flushes["kind"], flushes["window_room"], flushes["id0"], flushes["id1"] = -7, 1, 2, 3, 4
    flush_index = rng.permutation(n + 3)[:n].astype(np.uint32)      # (no flush named twice)
    flush_index[rng.random(n) < 0.2] = fr.NO_INDEX
    flush_index[rng.random(n) < 0.05] = n + 3
    return {"states": states, "entries": entries, "ticks": ticks, "fq": fq, "flush_results": flush_results,
            "result_index": result_index, "flushes": flushes, "flush_index": flush_index}
