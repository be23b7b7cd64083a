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
    t = math.copysign(float(math.trunc(v)), v)   # (trunc keeps the sign of a zero)
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


def eval_tcp_throughput_f64(rtt, p):
    """The value eval_tcp_throughput casts (not a function of the reference: tests/test_float_paths.py compares it
    as 64 bits)."""
    s = float(MSS)
    f_p = f64_sqrt(f64_mul(p, 2.0) / 3.0) + f64_mul(f64_mul(f64_mul(12.0, f64_sqrt(f64_mul(p, 3.0) / 8.0)), p),
                                                    1.0 + f64_mul(f64_mul(32.0, p), p))
    return f64_div(s, f64_mul(rtt, f_p))


def eval_tcp_throughput(rtt, p):
    return as_u32(eval_tcp_throughput_f64(rtt, p))


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


# ---- the square root sweep (tests/test_gpu_rate.py, tests/test_float_paths.py) ----
def sweep_values():
    """4096 (rtt_ms, loss_rate) pairs: loss rates over the decades with their neighbours in the last bit, 0, 1,
    denormals, infinity and NaN; RTTs over the decades."""
    rng = np.random.default_rng(42)
    decades = 10.0 ** rng.uniform(-12, 0.5, 1200)
    near = np.concatenate([np.nextafter(decades[:400], 0.0), np.nextafter(decades[:400], 2.0)])
    third = np.array([2.0 / 3.0, 1.5, 8.0 / 3.0, 0.375, 0.25, 1.0, 0.0, -0.0, np.inf, np.nan, -1.0, 5e-324, 1e-310,
                      2.2250738585072014e-308, 2.225073858507201e-308, 1e-300, 4.0, 1e300])
    edges = np.concatenate([third, np.nextafter(third, 0.0), np.nextafter(third, np.inf)])
    squares = (rng.integers(1, 1 << 26, 600).astype(np.float64) ** 2) * 1.5 / 2.0 ** 60   # p*2/3 a perfect square
    loss = np.concatenate([decades, near, edges, squares, np.nextafter(squares, 0.0), np.nextafter(squares, 1.0)])
    loss = np.resize(loss, 4096)
    rtt = np.resize(np.concatenate([[0, 1, 2, 3, 10, 50, 100, 1000, 60000, 1 << 40],
                                    (10.0 ** rng.uniform(0, 4.5, 500)).astype(np.uint64)]), 4096).astype(np.uint64)
    return rtt, rng.permutation(loss)


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


def random_batch(rng, n, recv_cap=4, spoil=0.05, fill=0.0):
    """n random connections for one ufc_rate_step call: states over all three modes that pass the state check (but
    for a fraction `spoil`, broken in one rule each), their sets, ticks, frame queue results with and without
    feedback, timers expired or not, and both gathers.  The inputs include rtt 0 (REF_PANIC with a rate-limited
    feedback), sets at their capacity (RECV_FULL), times near the u64 wrap, NaN, infinite and denormal loss rates,
    receive rates 0 and u32::MAX.  A fraction `fill` of the connections has its set at capacity, every stamp younger
    than two RTTs, and a rate-limited feedback (RECV_FULL whatever recv_cap is); at fill = 0 nothing more is drawn, so
    a seed gives the batch it always gave.  Returns a dict of arrays."""
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
        if fill and rng.random() < fill:   # a full room: rtt_ms stays 50, every entry younger than 100 ms
            s["mode"] = int(rng.integers(1, 3))
            s["has_rtt_s"], s["rtt_s"], s["recv_count"] = 1, 0.05, recv_cap
            t["now_ms"] = (base + 100) & M64
            t["flags"] = 0
            for k in range(recv_cap):
                entries[first + k] = ((base + 1 + int(rng.integers(0, 100))) & M64, _u32(rng), 0, (0, 0, 0))
            f["has_feedback"], f["rtt_ms"], f["rate_limited"] = 1, 50, 1
            f["receive_rate"], f["loss_rate"] = _u32(rng), _f64(rng)
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


# ---- sets longer than the entries a step holds in registers (kRateHeld = 4) ----
HELD = 4
NOW, FRESH, EXPIRED = 10000, 9950, 9000          # with rtt_ms 50: ages 50 (< 100, kept) and 1000 (dropped)
TINY_LOSS = 1e-9                                 # send_rate_tcp about 1.1e9: the receive limit decides send_rate
FED = 50000                                      # the feedback's receive rate, below every value of the sets
RUBBISH = (0x5A5A5A5A5A5A5A5A, 0xA5A5A5A5, 0, (7, 7, 7))


def _val(k):
    return 100000 + 1000 * k


def _set(stamps, values=None):
    return [(t, _val(k) if values is None else values[k], 0) for k, t in enumerate(stamps)]


def set_cases():
    """One connection per case, as dicts: name, cap, entries [(timestamp_ms, value, is_initial)], what differs from
    the common state (THROUGHPUT_EQN, rtt_s 0.05, rtt_ms 50, max_send_rate u32::MAX), tick and feedback (now 10,000,
    rtt 50 ms, receive rate 50,000, loss 1e-9, rate limited), and `facts`, which check_set_facts asserts on the
    restatement's output: `stop`; `entries`, the set afterwards ("new" is the entry the feedback appends);
    `send_rate`; `unchanged` for a stopped connection; `arena_last` for the room that ends the arena."""
    F, X = FRESH, EXPIRED
    new = (NOW, FED, 0)
    cases = []

    def case(name, cap, entries, facts, **kw):
        cases.append(dict(name=name, cap=cap, entries=entries, facts=facts, **kw))

    def kept(entries, idx):
        return [entries[k] for k in idx] + [new]

    e = _set([F] * 5)
    case("five_all_kept", 8, e, {"stop": fr.RATE_DONE, "entries": kept(e, range(5)), "send_rate": 2 * _val(4)})
    e = _set([X] * 4 + [F] * 4)
    case("tail_only_kept", 8, e, {"stop": fr.RATE_DONE, "entries": kept(e, (4, 5, 6, 7)), "send_rate": 2 * _val(7)})
    e = _set([F] * 4 + [X] * 4)
    case("head_only_kept", 8, e, {"stop": fr.RATE_DONE, "entries": kept(e, (0, 1, 2, 3)), "send_rate": 2 * _val(3)})
    e = _set([F, X] * 4)
    case("alternate_kept", 8, e, {"stop": fr.RATE_DONE, "entries": kept(e, (0, 2, 4, 6)), "send_rate": 2 * _val(6)})
    e = _set([X] * 8)
    case("none_kept", 8, e, {"stop": fr.RATE_DONE, "entries": [new], "send_rate": 2 * FED})
    e = _set([F] * 5)
    case("full_by_the_tail", 5, e, {"stop": fr.RATE_RECV_FULL, "unchanged": True})
    e = _set([F] * 4 + [X])
    case("room_by_the_tail", 5, e, {"stop": fr.RATE_DONE, "entries": kept(e, range(4)), "send_rate": 2 * _val(3)})
    e = _set([F] * 23)
    case("cap24_fills", 24, e, {"stop": fr.RATE_DONE, "entries": kept(e, range(23)), "send_rate": 2 * _val(22)})
    e = _set([F] * 24)
    case("cap24_full", 24, e, {"stop": fr.RATE_RECV_FULL, "unchanged": True})
    values = [_val(5), _val(4), _val(3), _val(2), _val(1), 900000]
    e = _set([F] * 6, values)
    case("max_in_tail", 8, e, {"stop": fr.RATE_DONE, "entries": kept(e, range(6)), "send_rate": 2 * 900000})
    e = _set([F] * 5 + [X], values)
    case("max_in_tail_expired", 8, e, {"stop": fr.RATE_DONE, "entries": kept(e, range(5)), "send_rate": 2 * _val(5)})
    # now 40: M64 - 10 and M64 wrap to the ages 51 and 41 (kept); 45 and 1000 lie ahead of now (ages near 2^64)
    e = _set([10, 10, 10, 10, M64 - 10, 45, M64, 1000])
    case("wrapped_ages_in_tail", 8, e, {"stop": fr.RATE_DONE, "send_rate": 2 * _val(6),
                                        "entries": [e[k] for k in (0, 1, 2, 3, 4, 6)] + [(40, FED, 0)]}, now=40)

    values = [_val(k) for k in range(6)] + [900000, _val(7)]
    e = _set([F] * 8, values)
    case("replace_max_tail", 8, e, {"stop": fr.RATE_DONE, "entries": [(NOW, 900000, 0)], "send_rate": 2 * 900000},
         limited=False)
    case("replace_max_tail_loss_increase", 8, e, {"stop": fr.RATE_DONE, "entries": [(NOW, 450000, 0)],
                                                  "send_rate": 450000}, limited=False, prev_loss=0.0)
    e = [(F, M32, 1)] + _set([F] * 5, [_val(1), _val(2), _val(3), _val(4), 900000])
    case("initial_skipped_with_tail", 8, e, {"stop": fr.RATE_DONE, "entries": [(NOW, 900000, 0)],
                                             "send_rate": 2 * 900000}, limited=False)

    values = [_val(k) for k in range(7)] + [900000]
    e = _set([F] * 8, values)
    # current_limit = min(send_rate_tcp, 2 * 900000), new_limit = 900000: the set becomes one entry of new_limit / 2
    case("nofeedback_max_in_tail", 8, e, {"stop": fr.RATE_DONE, "entries": [(NOW, 450000, 0)], "send_rate": 900000},
         feedback=False, state={"nofeedback_exp_ms": NOW, "nofeedback_idle": 0, "send_rate_tcp": 1000000000})

    e = _set([F] * 5)
    case("room_at_arena_end", 6, e, {"stop": fr.RATE_DONE, "entries": kept(e, range(5)), "send_rate": 2 * _val(4),
                                     "arena_last": True}, arena_last=True)
    return cases


def set_neighbour(k=0, count=1):
    """A connection with `count` entries in a room of as many: what stands beside the cases (count 1), and the
    fillers of the device batch (1..3)."""
    e = [(FRESH, 30000 + k % 1000 + j, 0) for j in range(count)]
    return dict(name=None, cap=count, entries=e, facts=None, limited=False)


def set_batch(conns):
    """The connections `conns` (dicts of set_cases or set_neighbour) as one batch in their order.  The rooms lie in
    the arena in the connections' order and adjoin each other, but for the last connection with `arena_last`, whose
    room ends the arena, and the connection behind it, whose room then begins it.  Behind a set's count the room is
    rubbish.  Every connection has a flush of its own; no flush result is gathered.  The dict of random_batch, and
    "index": the connections of each name."""
    n = len(conns)
    last = max((c for c in range(n) if conns[c].get("arena_last")), default=None)
    order = list(range(n))
    if last is not None:
        tail = order[last + 1:]
        order = tail + order[:last] + [last]
    total = sum(c["cap"] for c in conns)
    states, _ = fr.new_rate_states(n, M32, 1)
    entries = np.zeros(total, dtype=fr.RECV_RATE_ENTRY_DTYPE)
    first = 0
    for c in order:
        states[c]["recv_first"], states[c]["recv_cap"] = first, conns[c]["cap"]
        first += conns[c]["cap"]
    ticks = np.zeros(n, dtype=fr.RATE_TICK_DTYPE)
    fq = np.zeros(n, dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    index = {}
    for c, conn in enumerate(conns):
        s = states[c]
        now = conn.get("now", NOW)
        s["mode"], s["send_rate"], s["send_rate_tcp"] = THROUGHPUT_EQN, 100000, 100000
        s["has_rtt_s"], s["rtt_s"], s["has_rtt_ms"], s["rtt_ms"] = 1, 0.05, 1, 50
        s["has_rto_ms"], s["rto_ms"], s["nofeedback_idle"] = 1, 200, 1
        s["has_nofeedback_exp"], s["nofeedback_exp_ms"] = 1, now + 5000
        s["prev_loss_rate"] = conn.get("prev_loss", TINY_LOSS)
        s["now_ms"] = max(now - 10, 0)
        for k, v in conn.get("state", {}).items():
            s[k] = v
        s["recv_count"] = len(conn["entries"])
        r0 = int(s["recv_first"])
        for k in range(conn["cap"]):
            entries[r0 + k] = conn["entries"][k] + ((0, 0, 0),) if k < len(conn["entries"]) else RUBBISH
        ticks[c] = make_tick(now, 0.01)
        if conn.get("feedback", True):
            fq[c] = make_feedback(50, FED, TINY_LOSS, conn.get("limited", True))
        if conn["name"] is not None:
            index.setdefault(conn["name"], []).append(c)
    flushes = np.zeros(n, dtype=fr.FLUSH_DTYPE)
    flushes["flush_alloc"], flushes["kind"] = -7, 1
    return {"states": states, "entries": entries, "ticks": ticks, "fq": fq, "flush_results": None, "result_index": None,
            "flushes": flushes, "flush_index": np.arange(n, dtype=np.uint32), "index": index, "conns": conns}


def set_cases_between_neighbours():
    """Every case between two connections of one entry: neighbour, case, neighbour, case, ..., neighbour."""
    conns = [set_neighbour(0)]
    for k, case in enumerate(set_cases()):
        conns += [case, set_neighbour(k + 1)]
    return set_batch(conns)


def set_cases_at_tile_seams():
    """Case i at the connections 64 i + 63 and 64 i + 64 (lane 63 of one tile of the kernel and lane 0 of the next),
    connections of 1 to 3 entries everywhere else."""
    cases = set_cases()
    conns = [set_neighbour(c, 1 + c % 3) for c in range(64 * len(cases) + 1)]
    for i, case in enumerate(cases):
        conns[64 * i + 63] = case
        conns[64 * i + 64] = case
    return set_batch(conns)


def check_set_facts(b, exp):
    """Every named connection's facts against exp = expect_step(...), the restatement's output; and for every
    connection that the room behind its set is what it was."""
    arena, ends = len(b["entries"]), 0
    for c, conn in enumerate(b["conns"]):
        s, out, res = b["states"][c], exp["states_out"][c], exp["results"][c]
        r0, cap = int(s["recv_first"]), int(s["recv_cap"])
        room_in, room = b["entries"][r0:r0 + cap], exp["entries"][r0:r0 + cap]
        behind = max(int(out["recv_count"]), int(s["recv_count"]))
        assert room[behind:].tobytes() == room_in[behind:].tobytes(), (conn["name"], c)
        f = conn["facts"]
        if f is None:
            assert int(res["stop"]) == fr.RATE_DONE and int(out["recv_count"]) == 1 and cap <= 3, c
            continue
        assert int(res["stop"]) == f["stop"], (conn["name"], int(res["stop"]))
        assert cap > HELD and int(s["recv_count"]) >= HELD + 1, conn["name"]
        if f.get("unchanged"):
            assert out.tobytes() == s.tobytes() and room.tobytes() == room_in.tobytes(), conn["name"]
            assert int(exp["flushes"][c]["flush_alloc"]) == -7, conn["name"]
            continue
        assert int(out["rtt_ms"]) == 50, (conn["name"], int(out["rtt_ms"]))
        count = int(out["recv_count"])
        have = [(int(e["timestamp_ms"]), int(e["value"]), int(e["is_initial"])) for e in room[:count]]
        assert have == list(f["entries"]) and int(res["recv_count"]) == count, (conn["name"], have)
        assert all(bytes(e["reserved"]) == b"\0\0\0" for e in room[:count]), conn["name"]
        assert int(res["send_rate"]) == f["send_rate"] == int(out["send_rate"]), (conn["name"], int(res["send_rate"]))
        assert int(exp["flushes"][c]["flush_alloc"]) == int(res["flush_alloc"]), conn["name"]
        if f.get("arena_last") and r0 + cap == arena:   # (of two copies of the case only one can end the arena)
            assert count == cap and have[-1] == f["entries"][-1], conn["name"]
            assert exp["entries"][arena - 1].tobytes() != b["entries"][arena - 1].tobytes(), conn["name"]
            ends += 1
    assert ends == 1


def set_coverage(b, exp):
    """What a batch does past the held entries, counted on exp = expect_step(...): DONE connections that came in with
    more than HELD entries (`large_done`), RECV_FULL in a room of more than HELD (`full_large`), and rate-limited
    updates that carry a survivor from an index >= HELD to one below (`moved`)."""
    seen = {"large_done": 0, "full_large": 0, "moved": 0, "largest": 0}
    for c in range(len(b["states"])):
        s, out, res, f = b["states"][c], exp["states_out"][c], exp["results"][c], b["fq"][c]
        stop, count = int(res["stop"]), int(s["recv_count"])
        if stop == fr.RATE_RECV_FULL and int(s["recv_cap"]) > HELD:
            seen["full_large"] += 1
        if stop != fr.RATE_DONE or count <= HELD:
            continue
        seen["large_done"] += 1
        seen["largest"] = max(seen["largest"], count)
        if int(s["mode"]) == AWAIT_SEND or not f["has_feedback"] or not f["rate_limited"]:
            continue
        r0, now, two_rtt = int(s["recv_first"]), int(b["ticks"][c]["now_ms"]), (2 * int(out["rtt_ms"])) & M64
        room_in, room = b["entries"][r0:r0 + count], exp["entries"][r0:r0 + count]
        kept = [k for k in range(count) if ((now - int(room_in[k]["timestamp_ms"])) & M64) < two_rtt]
        assert len(kept) + 1 == int(out["recv_count"]), c
        assert all(room[j].tobytes()[:13] == room_in[k].tobytes()[:13] for j, k in enumerate(kept)), c
        seen["moved"] += any(k >= HELD and j < HELD for j, k in enumerate(kept))
    return seen
