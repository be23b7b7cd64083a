"""What the batched sender frame queue (ufc_frame_queue_host / ufc_frame_queue_varlen) must compute, restated class for
class from the reference: FrameLog, FeedbackGen and FrameQueue (src/half_connection/frame_queue.rs), ReorderBuffer
(reorder_buffer.rs) and LossIntervalQueue (loss_rate.rs), with plain deques and `& 0xFFFFFFFF` where the release build
wraps.  The control flow follows the Rust line for line so that it can be read against it; nothing is copied.  Where
the reference would panic (an unwrap of None, an index into an empty deque) ReferencePanic is raised: the batch call's
state check exists so that this never happens, and the tests assert it.

Then: the driver that turns one batch call into those method calls (expect_batch), the state check restated
(state_ok), and a traffic generator (frames sent at rising times; a receiver that loses, duplicates and reorders,
and acknowledges in groups the way FrameAckQueue does, now and then out of order, stale, with a bad nonce or empty).
"""
import math
from collections import deque

import numpy as np

from uflow_amd import frame as fr

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
U32_MAX_F = 4294967295.0


class ReferencePanic(Exception):
    pass


def unwrap(v):
    if v is None:
        raise ReferencePanic("unwrap of None")
    return v


# ---- Rust's float arithmetic ----
def f64_div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def clamp(v, lo, hi):      # f64::clamp: a NaN stays a NaN
    if v != v:
        return v
    return lo if v < lo else hi if v > hi else v


def f64_round(v):          # f64::round: half away from zero (v >= 0 here)
    if v != v or math.isinf(v):
        return v
    t = math.floor(v)
    return float(t + 1) if v - t >= 0.5 else float(t)


def as_u32(v):             # `as u32`: saturating, NaN is 0
    if v != v or v <= 0.0:
        return 0
    return M32 if v >= U32_MAX_F else int(v)


# ---- frame_queue.rs:14-84 ----
class Entry:
    def __init__(self, size, send_time_ms, fragment_refs, nonce, rate_limited, acked):
        self.size, self.send_time_ms, self.fragment_refs = size, send_time_ms, fragment_refs
        self.nonce, self.rate_limited, self.acked = nonce, rate_limited, acked


class FrameLog:
    def __init__(self, base_id):
        self.next_id = base_id
        self.base_id = base_id
        self.frames = deque()
        self.drained = []   # (not in the reference: what drain removed, for the driver's ring)

    def get_frame(self, frame_id):
        k = (frame_id - self.base_id) & M32
        return self.frames[k] if k < len(self.frames) else None

    def len(self):
        return len(self.frames) & M32

    def push(self, entry):
        self.frames.append(entry)
        self.next_id = (self.next_id + 1) & M32

    def find_expiration_cutoff(self, thresh_ms):
        expiry_point = self.base_id
        for frame in self.frames:
            if frame.send_time_ms < thresh_ms:
                expiry_point = (expiry_point + 1) & M32
            else:
                break
        return expiry_point

    def drain(self, frame_id):
        drain_idx = (frame_id - self.base_id) & M32
        if drain_idx > len(self.frames):
            raise ReferencePanic("drain past the end")
        for k in range(drain_idx):
            self.drained.append(((self.base_id + k) & M32, self.frames.popleft()))
        self.base_id = frame_id


# ---- reorder_buffer.rs ----
class ReorderBuffer:
    def __init__(self, base_id, max_span):
        self.frames = [0, 0]
        self.frame_count = 0
        self.base_id = base_id
        self.max_span = max_span

    def can_put(self, new_frame_id):
        return ((new_frame_id - self.base_id) & M32) < self.max_span

    def put(self, new_frame_id, callback):
        if self.frame_count == 0:
            if new_frame_id == self.base_id:
                callback(new_frame_id, True)
                self.base_id = (self.base_id + 1) & M32
            else:
                self.frames[0] = new_frame_id
                self.frame_count = 1
        elif self.frame_count == 1:
            if new_frame_id == self.base_id:
                callback(new_frame_id, True)
                self.base_id = (self.base_id + 1) & M32
                if self.frames[0] == self.base_id:
                    callback(self.frames[0], True)
                    self.base_id = (self.base_id + 1) & M32
                    self.frame_count = 0
            else:
                delta_new = (new_frame_id - self.base_id) & M32
                delta_0 = (self.frames[0] - self.base_id) & M32
                if delta_new < delta_0:
                    self.frames[1] = self.frames[0]
                    self.frames[0] = new_frame_id
                else:
                    self.frames[1] = new_frame_id
                self.frame_count = 2
        elif self.frame_count == 2:
            min_frame_id = new_frame_id
            delta_min = (new_frame_id - self.base_id) & M32
            delta_1 = (self.frames[1] - self.base_id) & M32
            if delta_1 < delta_min:
                self.frames[1], min_frame_id = min_frame_id, self.frames[1]
                delta_min = delta_1
            delta_0 = (self.frames[0] - self.base_id) & M32
            if delta_0 < delta_min:
                self.frames[0], min_frame_id = min_frame_id, self.frames[0]
            while self.base_id != min_frame_id:
                callback(self.base_id, False)
                self.base_id = (self.base_id + 1) & M32
            callback(min_frame_id, True)
            self.base_id = (self.base_id + 1) & M32
            if self.frames[0] == self.base_id:
                callback(self.frames[0], True)
                self.base_id = (self.base_id + 1) & M32
                self.frame_count -= 1
                if self.frames[1] == self.base_id:
                    callback(self.frames[1], True)
                    self.base_id = (self.base_id + 1) & M32
                    self.frame_count -= 1
                else:
                    self.frames[0] = self.frames[1]

    def can_advance(self, new_base_id):
        delta = (new_base_id - self.base_id) & M32
        return 1 <= delta <= self.max_span

    def advance(self, new_base_id, callback):
        while self.frame_count > 0 and ((self.frames[0] - self.base_id) & M32) < ((new_base_id - self.base_id) & M32):
            while self.base_id != self.frames[0]:
                callback(self.base_id, False)
                self.base_id = (self.base_id + 1) & M32
            callback(self.frames[0], True)
            self.base_id = (self.base_id + 1) & M32
            if self.frame_count == 2:
                self.frames[0] = self.frames[1]
            self.frame_count -= 1
        while self.base_id != new_base_id:
            callback(self.base_id, False)
            self.base_id = (self.base_id + 1) & M32
        if self.frame_count == 1:
            if self.frames[0] == self.base_id:
                callback(self.frames[0], True)
                self.base_id = (self.base_id + 1) & M32
                self.frame_count = 0
        elif self.frame_count == 2:
            if self.frames[0] == self.base_id:
                callback(self.frames[0], True)
                self.base_id = (self.base_id + 1) & M32
                self.frame_count -= 1
                if self.frames[1] == self.base_id:
                    callback(self.frames[1], True)
                    self.base_id = (self.base_id + 1) & M32
                    self.frame_count -= 1
                else:
                    self.frames[0] = self.frames[1]


# ---- loss_rate.rs ----
class LossInterval:
    def __init__(self, end_time_ms, length):
        self.end_time_ms, self.length = end_time_ms, length


class LossIntervalQueue:
    WEIGHTS = [1.0, 1.0, 1.0, 1.0, 0.8, 0.6, 0.4, 0.2]

    def __init__(self):
        self.entries = deque()
        self.acks = self.nacks = 0   # (not in the reference: calls counted for the result)

    def truncate(self, n):
        while len(self.entries) > n:
            self.entries.pop()

    def reset(self, initial_p):
        self.truncate(1)
        if not self.entries:
            raise ReferencePanic("entries[0] of an empty queue")
        self.entries[0].length = as_u32(f64_round(clamp(f64_div(self.WEIGHTS[0], initial_p), 0.0, U32_MAX_F)))

    def push_ack(self):
        self.acks += 1
        if self.entries:
            last_interval = self.entries[0]
            last_interval.length = min(last_interval.length + 1, M32)

    def push_nack(self, send_time_ms, rtt_ms):
        self.nacks += 1
        if self.entries:
            last_interval = self.entries[0]
            if send_time_ms >= last_interval.end_time_ms:
                self.entries.appendleft(LossInterval((send_time_ms + rtt_ms) & M64, 1))
                self.truncate(9)
            else:
                last_interval.length = min(last_interval.length + 1, M32)
        else:
            self.entries.appendleft(LossInterval((send_time_ms + rtt_ms) & M64, 1))

    def compute_loss_rate(self):
        n = len(self.entries)
        if n > 0:
            i_total_0 = 0.0
            i_total_1 = 0.0
            w_total = 0.0
            if n > 1:
                for i in range(n - 1):
                    i_total_0 += float(self.entries[i].length) * self.WEIGHTS[i]
                    w_total += self.WEIGHTS[i]
                for i in range(1, n):
                    i_total_1 += float(self.entries[i].length) * self.WEIGHTS[i - 1]
                return f64_div(w_total, max(i_total_0, i_total_1))
            return f64_div(self.WEIGHTS[0], float(self.entries[0].length) * self.WEIGHTS[0])
        return 0.0


# ---- frame_queue.rs:86-195 ----
def ms_to_s(v):
    return f64_div(float(v), 1000.0)


class AckData:
    def __init__(self, last_send_time_ms, total_ack_size, rate_limited):
        self.last_send_time_ms, self.total_ack_size, self.rate_limited = last_send_time_ms, total_ack_size, rate_limited


class FeedbackData:
    def __init__(self, rtt_ms, receive_rate, loss_rate, rate_limited):
        self.rtt_ms, self.receive_rate, self.loss_rate, self.rate_limited = rtt_ms, receive_rate, loss_rate, rate_limited


class FeedbackGen:
    INITIAL_RTT_MS = 100

    def __init__(self, base_id, max_span):
        self.last_feedback_ms = None
        self.ack_data = None
        self.reorder_buffer = ReorderBuffer(base_id, max_span)
        self.loss_intervals = LossIntervalQueue()

    def reset_loss_rate(self, new_loss_rate):
        self.loss_intervals.reset(new_loss_rate)

    def get_feedback(self, now_ms):
        if self.ack_data is not None:
            ack_data, self.ack_data = self.ack_data, None
            rtt_ms = (now_ms - ack_data.last_send_time_ms) & M64
            if self.last_feedback_ms is not None:
                delta_time_s = ms_to_s((now_ms - self.last_feedback_ms) & M64)
                receive_rate = as_u32(clamp(f64_div(float(ack_data.total_ack_size), delta_time_s), 0.0, U32_MAX_F))
            else:
                receive_rate = 0
            self.last_feedback_ms = now_ms
            loss_rate = self.loss_intervals.compute_loss_rate()
            return FeedbackData(rtt_ms, receive_rate, loss_rate, ack_data.rate_limited)
        return None

    def put_ack_data(self, ack_data):
        if self.ack_data is not None:
            fd = self.ack_data
            fd.last_send_time_ms = max(fd.last_send_time_ms, ack_data.last_send_time_ms)
            fd.total_ack_size = (fd.total_ack_size + ack_data.total_ack_size) & M64
            fd.rate_limited |= ack_data.rate_limited
        else:
            self.ack_data = ack_data

    def _callback(self, frame_log, rtt_ms):
        def cb(frame_id, was_seen):
            sent_frame = unwrap(frame_log.get_frame(frame_id))
            if was_seen:
                self.loss_intervals.push_ack()
            else:
                self.loss_intervals.push_nack(sent_frame.send_time_ms, rtt_ms if rtt_ms is not None else self.INITIAL_RTT_MS)
        return cb

    def notify_ack(self, frame_id, frame_log, rtt_ms):
        if self.reorder_buffer.can_put(frame_id):
            self.reorder_buffer.put(frame_id, self._callback(frame_log, rtt_ms))
        else:
            pass  # old frame: nothing

    def notify_advancement(self, new_base_id, frame_log, rtt_ms):
        if self.reorder_buffer.can_advance(new_base_id):
            self.reorder_buffer.advance(new_base_id, self._callback(frame_log, rtt_ms))


# ---- frame_queue.rs:197-388 ----
class TransferWindow:
    def __init__(self, base_id, size, tail_size):
        self.base_id, self.size, self.tail_size = base_id, size, tail_size


class FrameQueue:
    def __init__(self, size, tail_size, base_id):
        self.frame_log = FrameLog(base_id)
        self.feedback_gen = FeedbackGen(base_id, (size + tail_size) & M32)
        self.window = TransferWindow(base_id, size, tail_size)
        self.rate_limited = False
        self.acknowledge_fragment = lambda ref: None   # (PendingPacket::acknowledge_fragment, the caller's)
        self.frames_acked = 0                          # (not in the reference: counted for the result)

    def can_push(self):
        return ((self.next_id() - self.window.base_id) & M32) < self.window.size

    def next_id(self):
        return self.frame_log.next_id

    def base_id(self):
        return self.window.base_id

    def mark_rate_limited(self):
        self.rate_limited = True

    def push(self, size, now_ms, fragment_refs, nonce):
        if self.can_push():
            self.frame_log.push(Entry(size & M32, now_ms, fragment_refs, nonce, self.rate_limited, False))
            self.rate_limited = False
            return True
        return False

    def forget_frames(self, thresh_ms, rtt_ms):
        max_base_id = self.frame_log.find_expiration_cutoff(thresh_ms)
        delta = (max_base_id - self.frame_log.base_id) & M32
        if delta != 0:
            self.cull_log_entries(max_base_id, rtt_ms)

    def get_feedback(self, now_ms):
        return self.feedback_gen.get_feedback(now_ms)

    def reset_loss_rate(self, new_loss_rate):
        self.feedback_gen.reset_loss_rate(new_loss_rate)

    def acknowledge_group(self, base_id, bitfield, nonce, rtt_ms):
        """Returns which way it left ("dud", "unknown", "bad_nonce", "done"): the reference returns nothing."""
        true_nonce = False
        last_send_time_ms = 0
        total_ack_size = 0
        rate_limited = False
        bitfield_size = 0
        for i in reversed(range(32)):
            if bitfield & (1 << i) != 0:
                bitfield_size = i + 1
                break
        if bitfield_size == 0:
            return "dud"
        for i in range(bitfield_size):
            frame_id = (base_id + i) & M32
            sent_frame = self.frame_log.get_frame(frame_id)
            if sent_frame is not None:
                if bitfield & (1 << i) != 0:
                    true_nonce ^= sent_frame.nonce
            else:
                return "unknown"
        if nonce != true_nonce:
            return "bad_nonce"
        for i in range(bitfield_size):
            frame_id = (base_id + i) & M32
            sent_frame = unwrap(self.frame_log.get_frame(frame_id))
            rate_limited |= sent_frame.rate_limited
            if bitfield & (1 << i) != 0:
                if not sent_frame.acked:
                    sent_frame.acked = True
                    self.frames_acked += 1
                    fragment_refs, sent_frame.fragment_refs = sent_frame.fragment_refs, ()
                    for fragment_ref in fragment_refs:
                        self.acknowledge_fragment(fragment_ref)
                    last_send_time_ms = max(last_send_time_ms, sent_frame.send_time_ms)
                    total_ack_size = (total_ack_size + sent_frame.size) & M64
                    self.feedback_gen.notify_ack(frame_id, self.frame_log, rtt_ms)
        self.feedback_gen.put_ack_data(AckData(last_send_time_ms, total_ack_size, rate_limited))
        return "done"

    def can_advance_transfer_window(self, new_base_id):
        next_delta = (self.frame_log.next_id - self.window.base_id) & M32
        delta = (new_base_id - self.window.base_id) & M32
        return delta != 0 and delta <= next_delta

    def advance_transfer_window(self, new_base_id, rtt_ms):
        if self.can_advance_transfer_window(new_base_id):
            self.window.base_id = new_base_id
            max_base_id = (self.window.base_id - self.window.tail_size) & M32
            delta = (max_base_id - self.frame_log.base_id) & M32
            if delta != 0 and delta <= self.frame_log.len():
                self.cull_log_entries(max_base_id, rtt_ms)

    def cull_log_entries(self, new_log_base_id, rtt_ms):
        self.feedback_gen.notify_advancement(new_log_base_id, self.frame_log, rtt_ms)
        self.frame_log.drain(new_log_base_id)


# ---- the batch call's state check, restated from the header ----
def state_ok(q, step, n_log, ff0, ff1, n_frames, sf0, sf1, n_sent):
    span = int(q["window_size"]) + int(q["tail_size"])
    cap = int(q["log_cap"])
    if cap == 0 or cap & (cap - 1) or cap < span:
        return False
    if int(q["log_first"]) + cap > n_log:
        return False
    length = (int(q["log_next_id"]) - int(q["log_base_id"])) & M32
    ahead = (int(q["log_next_id"]) - int(q["window_base_id"])) & M32
    if length > cap or ahead > int(q["window_size"]) or length > ahead + int(q["tail_size"]):
        return False
    if int(q["rb_max_span"]) < span or int(q["rb_max_span"]) > 1 << 31:
        return False
    rb = (int(q["rb_base_id"]) - int(q["log_base_id"])) & M32
    if rb > length or int(q["rb_count"]) > 2:
        return False
    d = [(int(f) - int(q["rb_base_id"])) & M32 for f in q["rb_frames"]]
    for k in range(int(q["rb_count"])):
        if d[k] == 0 or rb + d[k] >= length:
            return False
    if int(q["rb_count"]) == 2 and d[0] >= d[1]:
        return False
    if int(q["li_count"]) > 9 or (int(step["flags"]) & fr.FQ_RESET_LOSS and int(q["li_count"]) == 0):
        return False
    return ff0 <= ff1 <= n_frames and sf0 <= sf1 <= n_sent


def load_queue(q, log):
    """The FrameQueue object a ufc_frame_queue record and its ring stand for."""
    fq = FrameQueue(int(q["window_size"]), int(q["tail_size"]), int(q["log_base_id"]))
    cap, first = int(q["log_cap"]), int(q["log_first"])
    length = (int(q["log_next_id"]) - int(q["log_base_id"])) & M32
    for k in range(length):
        e = log[first + ((int(q["log_base_id"]) + k) & (cap - 1))]
        flags = int(e["flags"])
        acked = bool(flags & fr.SENT_ACKED)
        refs = () if acked else range(int(e["ref_first"]), int(e["ref_first"]) + int(e["ref_count"]))
        entry = Entry(int(e["size"]), int(e["send_time_ms"]), refs, bool(flags & fr.SENT_NONCE),
                      bool(flags & fr.SENT_RATE_LIMITED), acked)
        entry.ref_first, entry.ref_count = int(e["ref_first"]), int(e["ref_count"])
        fq.frame_log.push(entry)
    fq.window.base_id = int(q["window_base_id"])
    rb = fq.feedback_gen.reorder_buffer
    rb.base_id, rb.max_span = int(q["rb_base_id"]), int(q["rb_max_span"])
    rb.frames, rb.frame_count = [int(q["rb_frames"][0]), int(q["rb_frames"][1])], int(q["rb_count"])
    fq.rate_limited = bool(q["rate_limited"])
    if q["has_ack_data"]:
        fq.feedback_gen.ack_data = AckData(int(q["ack_last_send_time_ms"]), int(q["ack_total_size"]),
                                           bool(q["ack_rate_limited"]))
    if q["has_last_feedback"]:
        fq.feedback_gen.last_feedback_ms = int(q["last_feedback_ms"])
    for k in range(int(q["li_count"])):
        fq.feedback_gen.loss_intervals.entries.append(LossInterval(int(q["li_end_time_ms"][k]), int(q["li_length"][k])))
    return fq


def store_queue(fq, q_in, log):
    """The record (and the ring's slots) of a FrameQueue object after a step."""
    q = q_in.copy()
    cap, first = int(q["log_cap"]), int(q["log_first"])

    def put(frame_id, entry):
        e = log[first + (frame_id & (cap - 1))]
        e["send_time_ms"], e["size"] = entry.send_time_ms, entry.size
        e["ref_first"], e["ref_count"] = entry.ref_first, entry.ref_count
        e["flags"] = (fr.SENT_NONCE if entry.nonce else 0) | (fr.SENT_RATE_LIMITED if entry.rate_limited else 0) | \
            (fr.SENT_ACKED if entry.acked else 0)
        e["reserved"] = 0

    for frame_id, entry in fq.frame_log.drained:
        put(frame_id, entry)
    for k, entry in enumerate(fq.frame_log.frames):
        put((fq.frame_log.base_id + k) & M32, entry)
    q["log_base_id"], q["log_next_id"] = fq.frame_log.base_id, fq.frame_log.next_id
    q["window_base_id"] = fq.window.base_id
    rb = fq.feedback_gen.reorder_buffer
    q["rb_base_id"], q["rb_count"] = rb.base_id, rb.frame_count
    q["rb_frames"][0], q["rb_frames"][1] = rb.frames
    q["rate_limited"] = 1 if fq.rate_limited else 0
    ad = fq.feedback_gen.ack_data
    q["has_ack_data"] = 1 if ad else 0
    q["ack_rate_limited"] = 1 if ad and ad.rate_limited else 0
    q["ack_last_send_time_ms"] = ad.last_send_time_ms if ad else 0
    q["ack_total_size"] = ad.total_ack_size if ad else 0
    if fq.feedback_gen.last_feedback_ms is not None:
        q["has_last_feedback"], q["last_feedback_ms"] = 1, fq.feedback_gen.last_feedback_ms
    li = fq.feedback_gen.loss_intervals.entries
    q["li_count"] = len(li)
    q["li_end_time_ms"][:] = 0
    q["li_length"][:] = 0
    for k, iv in enumerate(li):
        q["li_end_time_ms"][k], q["li_length"][k] = iv.end_time_ms, iv.length
    return q


def expect_connection(q, step, infos, items, ff0, ff1, sent, sf0, sf1, log, ref_acked):
    """One connection's step through the restated classes; log and ref_acked are updated in place.  Returns (result,
    queue_out)."""
    res = np.zeros((), dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    ok = state_ok(q, step, len(log), ff0, ff1, len(infos), sf0, sf1, len(sent))
    if ok:
        for i in range(ff0, ff1):
            f = infos[i]
            if f["ok"] and f["kind"] == fr.ACK and int(f["item_first"]) + int(f["item_count"]) > len(items):
                ok = False
    if not ok:
        res["stop"] = fr.FQ_BAD_STATE
        return res, q.copy()
    fq = load_queue(q, log)
    refs_cap = len(ref_acked) if ref_acked is not None else 0

    def acknowledge_fragment(ref):
        ref_acked[ref] = 1
    fq.acknowledge_fragment = acknowledge_fragment
    flags = int(step["flags"])
    rtt = int(step["rtt_ms"]) if flags & fr.FQ_HAS_RTT else None
    base0, wbase0 = fq.frame_log.base_id, fq.window.base_id
    if flags & fr.FQ_RESET_LOSS:
        fq.reset_loss_rate(float(step["reset_loss_rate"]))
    for j in range(sf0, sf1):
        s = sent[j]
        if not fq.can_push():              # (the emitters ask can_push first; a refused record is only counted)
            res["pushes_refused"] += 1
            continue
        if int(s["flags"]) & fr.SENT_MARK:
            fq.mark_rate_limited()
        fq.push(int(s["size"]), int(s["send_time_ms"]), None, bool(int(s["flags"]) & fr.SENT_NONCE))
        entry = fq.frame_log.frames[-1]
        entry.ref_first, entry.ref_count = int(s["ref_first"]), int(s["ref_count"])
        entry.fragment_refs = range(entry.ref_first, entry.ref_first + entry.ref_count)
        res["pushes_taken"] += 1
    if flags & fr.FQ_MARK_RATE_LIMITED:
        fq.mark_rate_limited()
    # (fragments at an index >= refs_cap are not the caller's: the ranges are clipped, not walked)
    for e in fq.frame_log.frames:
        if len(e.fragment_refs):
            e.fragment_refs = range(min(e.fragment_refs.start, refs_cap), min(e.fragment_refs.stop, refs_cap))
    for i in range(ff0, ff1):
        f = infos[i]
        if not (f["ok"] and f["kind"] == fr.ACK):
            continue
        res["ack_frames"] += 1
        for g in items[int(f["item_first"]):int(f["item_first"]) + int(f["item_count"])]:
            res["groups"] += 1
            how = fq.acknowledge_group(int(g["id"]), int(g["data_offset"]), bool(int(g["channel_id"]) & 1), rtt)
            if how != "done":
                res["groups_" + how] += 1
        fq.advance_transfer_window(int(f["f"][0]), rtt)
    if flags & fr.FQ_FORGET:
        fq.forget_frames(int(step["thresh_ms"]), rtt)
    if flags & fr.FQ_FEEDBACK:
        fb = fq.get_feedback(int(step["now_ms"]))
        if fb is not None:
            res["has_feedback"], res["rate_limited"] = 1, 1 if fb.rate_limited else 0
            res["receive_rate"], res["rtt_ms"], res["loss_rate"] = fb.receive_rate, fb.rtt_ms, fb.loss_rate
    res["frames_acked"] = fq.frames_acked
    res["li_acks"], res["li_nacks"] = fq.feedback_gen.loss_intervals.acks, fq.feedback_gen.loss_intervals.nacks
    res["window_advanced"] = (fq.window.base_id - wbase0) & M32
    res["log_culled"] = (fq.frame_log.base_id - base0) & M32
    ahead = (fq.next_id() - fq.window.base_id) & M32
    res["window_room"] = fq.window.size - ahead if ahead < fq.window.size else 0
    return res, store_queue(fq, q, log)


def expect_batch(infos, items, frame_first, sent, sent_first, queues, steps, log, ref_acked=None):
    """The whole call: returns {"results", "queues_out", "log", "ref_acked"}; the inputs are left as they are."""
    log = log.copy()
    ref_acked = ref_acked.copy() if ref_acked is not None else None
    n = len(queues)
    results = np.zeros(n, dtype=fr.FRAME_QUEUE_RESULT_DTYPE)
    out = queues.copy()
    for c in range(n):
        results[c], out[c] = expect_connection(queues[c], steps[c], infos, items, int(frame_first[c]), int(frame_first[c + 1]),
                                               sent, int(sent_first[c]), int(sent_first[c + 1]), log, ref_acked)
    return {"results": results, "queues_out": out, "log": log, "ref_acked": ref_acked}


# ---- records ----
def ack_info(frame_window_base_id, item_first, item_count, ok=1):
    f = np.zeros((), dtype=fr.FRAME_INFO_DTYPE)
    f["kind"], f["ok"], f["crc_ok"] = fr.ACK, ok, 1
    f["f"][0] = frame_window_base_id & M32
    f["item_first"], f["item_count"] = item_first, item_count
    return f


def group_item(base_id, bitfield, nonce):
    g = np.zeros((), dtype=fr.ITEM_DTYPE)
    g["id"], g["data_offset"], g["channel_id"], g["form"] = base_id & M32, bitfield & M32, nonce & 1, 3
    return g


def sent_frame(size, send_time_ms, nonce, ref_first=0, ref_count=0, mark=False):
    s = np.zeros((), dtype=fr.SENT_FRAME_DTYPE)
    s["size"], s["send_time_ms"], s["ref_first"], s["ref_count"] = size, send_time_ms, ref_first, ref_count
    s["flags"] = (fr.SENT_NONCE if nonce else 0) | (fr.SENT_MARK if mark else 0)
    return s


def make_step(flags=0, rtt_ms=0, thresh_ms=0, now_ms=0, reset_loss_rate=0.0):
    s = np.zeros((), dtype=fr.FRAME_QUEUE_STEP_DTYPE)
    s["flags"], s["rtt_ms"], s["thresh_ms"], s["now_ms"], s["reset_loss_rate"] = flags, rtt_ms, thresh_ms, now_ms, \
        reset_loss_rate
    return s


# ---- traffic ----
class Peer:
    """A sender's side of the generator: what it has sent (for the nonces), and the receiver's FrameAckQueue-like
    grouping of what arrived."""

    def __init__(self, rng, window_size, base_id, now_ms, ref_counter):
        self.rng, self.size, self.ref_counter = rng, window_size, ref_counter   # (one fragment table for all peers)
        self.next_id = self.window_base = self.rx_base = base_id
        self.now = now_ms
        self.nonces = {}

    def send(self, count, monotone=True):
        """`count` frames to push, at rising times (or, with monotone False, times all over)."""
        out = []
        for _ in range(count):
            self.now += int(self.rng.integers(0, 40))
            t = self.now if monotone else int(self.rng.integers(0, self.now + 200))
            nonce = int(self.rng.integers(0, 2))
            refs = int(self.rng.choice([0, 1, 1, 2, 3, 5, 20, 70]))
            out.append(sent_frame(int(self.rng.integers(1, 1473)), t, nonce, self.ref_counter[0], refs,
                                  mark=self.rng.random() < 0.05))
            self.ref_counter[0] += refs
            if ((self.next_id - self.window_base) & M32) < self.size:
                self.nonces[self.next_id] = nonce
                self.next_id = (self.next_id + 1) & M32
        return out

    def acks(self, loss=0.1, frames=1, hostile=0.0):
        """The receiver's answer to everything sent and not yet answered: `frames` ack frames' worth of (frame
        record's base id, [groups])."""
        rng = self.rng
        arrived = []
        k = self.rx_base
        while k != self.next_id:
            if rng.random() >= loss:
                arrived.append(k)
                if rng.random() < 0.05:
                    arrived.append(k)          # a duplicate: refused by the receiver's window, never acked
            k = (k + 1) & M32
        groups, cur = [], None
        base = self.rx_base
        for fid in arrived:
            if ((fid - base) & M32) >= self.size:
                continue
            base = (fid + 1) & M32
            if cur is not None and ((fid - cur[0]) & M32) < 32:
                cur[1] |= 1 << ((fid - cur[0]) & M32)
                cur[2] ^= self.nonces[fid]
            else:
                cur = [fid, 1, self.nonces[fid]]
                groups.append(cur)
        self.rx_base = self.next_id
        if rng.random() < 0.3 and len(groups) > 1:   # groups out of order: the reorder buffer holds frames
            j = int(rng.integers(0, len(groups) - 1))
            groups[j], groups[j + 1] = groups[j + 1], groups[j]
        if rng.random() < 0.3 and groups:            # a group split in two: its later half first
            g = groups.pop(int(rng.integers(0, len(groups))))
            ids = [(g[0] + b) & M32 for b in range(32) if g[1] >> b & 1]
            for part in (ids[len(ids) // 2:], ids[:len(ids) // 2]):
                if part:
                    bits, n = 0, 0
                    for fid in part:
                        bits |= 1 << ((fid - part[0]) & M32)
                        n ^= self.nonces[fid]
                    groups.append([part[0], bits, n])
        extra = []
        for g in groups:
            u = rng.random()
            if u < hostile * 0.25:
                extra.append([g[0], g[1], g[2] ^ 1])                      # a bad nonce
            elif u < hostile * 0.5:
                extra.append([g[0], 0, int(rng.integers(0, 2))])          # a dud
            elif u < hostile * 0.75:
                extra.append([(g[0] + int(rng.integers(0, 1 << 32))) & M32, int(rng.integers(1, 1 << 32)), 0])
            elif u < hostile:
                extra.append(list(g))                                     # said twice
        groups += extra
        new_base = base if rng.random() < 0.9 else (base + int(rng.integers(0, 1 << 32))) & M32
        per = max(1, -(-len(groups) // frames))
        out = [(new_base if k + per >= len(groups) else self.window_base, groups[k:k + per])
               for k in range(0, max(len(groups), 1), per)]
        if ((new_base - self.window_base) & M32) <= ((self.next_id - self.window_base) & M32):
            self.window_base = new_base
        return out


def make_batch(rng, n, window_size, tail_size, base_id, rounds=3, log_cap=None, hostile=0.2, loss=0.1, monotone=True,
               sends=None):
    """`rounds` successive calls' inputs for n connections: a list of dicts (infos, items, frame_first, sent,
    sent_first, steps), and the initial (queues, log).  The calls are meant to be chained through queues_out."""
    queues, log = fr.new_frame_queues(n, window_size, tail_size, base_id, log_cap)
    ref_counter = [0]
    peers = [Peer(rng, window_size, base_id, 1000 * c, ref_counter) for c in range(n)]
    calls = []
    for r in range(rounds):
        infos, items, sent = [], [], []
        ff, sf = [0], [0]
        steps = np.zeros(n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)
        for c, p in enumerate(peers):
            for base, groups in (p.acks(loss, frames=int(rng.integers(1, 3)), hostile=hostile) if r else []):
                infos.append(ack_info(base, len(items), len(groups)))
                items += [group_item(*g) for g in groups]
                if rng.random() < 0.2:
                    other = np.zeros((), dtype=fr.FRAME_INFO_DTYPE)   # a frame that is not an ack, or not ok
                    other["kind"], other["ok"] = (fr.DATA, 1) if rng.random() < 0.5 else (fr.ACK, 0)
                    other["item_first"], other["item_count"] = 0xFFFFFFF0, 100
                    infos.append(other)
            count = sends if sends is not None else int(rng.integers(0, max(2, min(window_size + 3, 150))))
            sent += p.send(count, monotone)
            ff.append(len(infos))
            sf.append(len(sent))
            flags = int(rng.integers(0, 32)) & ~(0 if rng.random() < 0.1 else fr.FQ_RESET_LOSS)
            steps[c] = make_step(flags, rtt_ms=int(rng.integers(0, 300)), thresh_ms=max(0, p.now - int(rng.integers(0, 3000))),
                                 now_ms=p.now + int(rng.integers(0, 50)),
                                 reset_loss_rate=float(rng.choice([0.5, 0.01, 1e-12, 3.0])))
        arr = lambda xs, dt: np.array(xs, dtype=dt) if xs else np.zeros(0, dtype=dt)
        calls.append({"infos": arr(infos, fr.FRAME_INFO_DTYPE), "items": arr(items, fr.ITEM_DTYPE),
                      "frame_first": np.array(ff, dtype=np.uint64), "sent": arr(sent, fr.SENT_FRAME_DTYPE),
                      "sent_first": np.array(sf, dtype=np.uint64), "steps": steps,
                      "refs": ref_counter[0]})
    return queues, log, calls
