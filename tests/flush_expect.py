"""The glue of HalfConnection::flush as the reference has it, restated in Python, with generators and directed
scenarios: what ufc_flush_acks_* and ufc_flush_sync_* are tested against (tests/test_flush_cpu.py,
tests/test_flush_gpu.py).

    AckFrameEmitter         <- src/half_connection/emit.rs:137-211 (push_dud :149-166, push :170-203, finalize :205-211)
    Half.emit_ack_frames    <- src/half_connection/mod.rs:296-333, over window_expect.FrameAckQueue's deque
    Half.emit_sync_frame    <- mod.rs:234-294
    Half.flush_tail         <- emit_frames, mod.rs:217-232, behind emit_ack_frames: the early returns and the
                               notify of emit_data_frames (:342-347) that moves sync_timeout_base_ms
    Half.is_send_pending    <- mod.rs:120-122
    expect_acks, expect_sync<- the C ABI's record formats around them (include/uflow_flush_ctl.h)

The deque and its groups are window_expect's; the frame sizes and the emitter's constants are pack_expect's, whose
pack_flush is the no-dud emitter the tests compare this one with.  Nothing here calls the library.
"""
import numpy as np

import pack_expect as P
import window_expect as W
from uflow_amd.flush import FLUSH_ACKS_RESULT_DTYPE, FLUSH_CTL_DTYPE, FLUSH_SYNC_RESULT_DTYPE
from uflow_amd.frame import ACK, SYNC, FLUSH_RESULT_DTYPE, FRAME_INFO_DTYPE, ITEM_DTYPE, NO_PARENT

M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
MIN_SYNC_TIMEOUT_MS = 2000
SYNC_FRAME_SIZE = 1 + 1 + 4 + 4 + 4   # frame id, mode, two ids, CRC (serial/mod.rs write_sync)
GROUPS_PER_FRAME = (P.MAX_FRAME_SIZE - P.ACK_FRAME_OVERHEAD) // P.ACK_GROUP_SIZE
FA_DONE, FA_BAD_STATE, FA_CARRY_FULL = 0, 1, 2
FS_SENT, FS_ACK_LIMITED, FS_DATA_LIMITED, FS_UPSTREAM, FS_NOT_DUE, FS_IDLE, FS_NO_ALLOC = range(7)
RS_SIZE_LIMITED, RS_WINDOW_LIMITED, RS_REF_HANG, RS_BAD_STATE, RS_STAGE_FULL, RS_HEAP_FULL = 1, 2, 3, 4, 5, 6
RS_NO_DATA_FLUSH = 1


class AckFrameEmitter:
    """emit.rs:137-211.  emit_cb(groups of the frame, its size)."""

    def __init__(self, flush_alloc, emit_cb):
        self.in_progress = None   # [groups]
        self.flush_alloc = flush_alloc
        self.emit_cb = emit_cb

    @staticmethod
    def size(groups):
        return P.ACK_FRAME_OVERHEAD + P.ACK_GROUP_SIZE * len(groups)

    def push_dud(self):
        if self.in_progress is not None:
            return True
        if self.flush_alloc < 0:
            return False
        self.in_progress = []
        return True

    def push(self, group):
        if self.in_progress is not None:
            frame_size = self.size(self.in_progress)
            if self.flush_alloc - frame_size < 0:
                self.finalize()
                return False
            elif frame_size + P.ACK_GROUP_SIZE > P.MAX_FRAME_SIZE:
                self.finalize()
            else:
                self.in_progress.append(group)
                return True
        if self.flush_alloc < 0:
            return False
        self.in_progress = [group]
        return True

    def finalize(self):
        if self.in_progress is not None:
            frame, self.in_progress = self.in_progress, None
            self.flush_alloc -= self.size(frame)
            self.emit_cb(frame, self.size(frame))


class Half:
    """The flush-control part of HalfConnection: the ack queue's deque, sync_reply, flush_alloc,
    sync_timeout_base_ms and the keepalive option."""

    def __init__(self, entries=(), sync_reply=False, sync_timeout_base_ms=0, keepalive_ms=None):
        self.frame_ack_queue = W.FrameAckQueue(1, 0)
        self.frame_ack_queue.entries = list(entries)
        self.sync_reply = sync_reply
        self.flush_alloc = 0
        self.sync_timeout_base_ms = sync_timeout_base_ms
        self.sync_keepalive_interval_ms = keepalive_ms

    def emit_ack_frames(self, sink):  # mod.rs:296-333
        def emit_cb(frame, size):
            sink.append(list(frame))
            self.flush_alloc -= size
            self.sync_reply = False

        afe = AckFrameEmitter(self.flush_alloc, emit_cb)
        if self.sync_reply:
            if not afe.push_dud():
                return False
        q = self.frame_ack_queue.entries
        while q:
            if not afe.push(q[0]):
                return False
            q.pop(0)
        afe.finalize()
        return True

    def emit_sync_frame(self, now_ms, rto_ms, next_frame_id, next_packet_id, sink):  # mod.rs:234-294
        """next_frame_id / next_packet_id: what :244-263 computed (None: absent).  Returns (ok, reason)."""
        elapsed_ms = (now_ms - self.sync_timeout_base_ms) & M64
        if elapsed_ms >= max(rto_ms, MIN_SYNC_TIMEOUT_MS):
            if next_frame_id is None and next_packet_id is None:
                if self.sync_keepalive_interval_ms is not None:
                    if elapsed_ms < self.sync_keepalive_interval_ms:
                        return True, FS_IDLE
                else:
                    return True, FS_IDLE
            if self.flush_alloc < 0:
                return False, FS_NO_ALLOC
            sink.append((next_frame_id, next_packet_id))
            self.flush_alloc -= SYNC_FRAME_SIZE
            self.sync_timeout_base_ms = now_ms
            return True, FS_SENT
        return True, FS_NOT_DUE


def group_of(item):
    """The deque entry of an ack group record; it remembers the record (the calls copy records whole)."""
    g = W.AckGroup(int(item["id"]), int(item["data_offset"]), int(item["channel_id"]))
    g.item = item.copy()
    return g


def item_of(g):
    return g.item


def expect_acks(ctl, windows, groups, group_first, receivers, rate, carry, flushes=None, flags=None, merged_cap=None,
                frames_cap=None, prefill=None):
    """What ufc_flush_acks_* must leave in every output, as the wrappers' dict has them (carry, flushes and flags:
    copies as updated), plus "facts".  prefill: arrays the capped outputs start from (merged, infos)."""
    n = len(ctl)
    pre = prefill or {}
    carry = carry.copy()
    flushes = None if flushes is None else flushes.copy()
    flags = None if flags is None else flags.copy()
    merged_all, infos_all = [], []
    merged_first = np.zeros(n + 1, dtype=np.uint64)
    results = np.zeros(n, dtype=FLUSH_RESULT_DTYPE)
    ack_results = np.zeros(n, dtype=FLUSH_ACKS_RESULT_DTYPE)
    windows_out, ctl_out = windows.copy(), ctl.copy()
    facts = dict(bad_state=0, dud=0, dud_empty=0, size_limited=0, carried=0, dropped=0, full_frames=0, frames=0)
    for c in range(n):
        C, Wn = ctl[c], windows[c]
        g0, g1 = int(group_first[c]), int(group_first[c + 1])
        cc, cap, first = int(C["carry_count"]), int(C["carry_cap"]), int(C["carry_first"])
        merged_first[c] = len(merged_all)
        r, ar = results[c], ack_results[c]
        r["frame_first"], ar["merged_first"] = len(infos_all), len(merged_all)
        alloc = int(rate[c]["flush_alloc"])
        ok = g0 <= g1 <= len(groups) and cc <= cap and first <= len(carry) and len(carry) - first >= cap
        if ok and cc:
            ok = g1 > g0 and int(groups[g0]["id"]) == int(carry[first + cc - 1]["id"])
        if not ok:
            r["stop"], r["alloc_left"], ar["stop"] = P.BAD_RANGE, alloc, FA_BAD_STATE
            facts["bad_state"] += 1
            if flushes is not None:
                flushes[c]["flush_alloc"] = alloc
            if flags is not None:
                flags[c] &= ~np.uint32(RS_NO_DATA_FLUSH)
            continue
        # the deque: what earlier flushes left (its last entry is the tail the window has since updated), then the
        # window's groups
        items = [it.copy() for it in carry[first: first + max(cc - 1, 0)]] + [it.copy() for it in groups[g0:g1]]
        h = Half([group_of(it) for it in items], sync_reply=bool(Wn["sync_reply"]))
        h.flush_alloc = alloc
        sink = []
        done = h.emit_ack_frames(sink)
        at = 0
        for fr_groups in sink:
            info = np.zeros((), dtype=FRAME_INFO_DTYPE)
            info["kind"], info["ok"] = ACK, 1
            info["f"][0], info["f"][1] = Wn["base_id"], receivers[c]["base_id"]
            info["item_first"], info["item_count"] = len(merged_all) + at, len(fr_groups)
            at += len(fr_groups)
            infos_all.append(info)
            facts["full_frames"] += len(fr_groups) == GROUPS_PER_FRAME
        left = h.frame_ack_queue.entries
        assert at + len(left) == len(items)
        kept = left[len(left) - min(len(left), cap):] if cap else []
        for k, g in enumerate(kept):
            carry[first + k] = item_of(g)
        merged_all.extend(items)
        dud = bool(Wn["sync_reply"]) and alloc >= 0
        r["frame_count"], r["items_packed"], r["alloc_left"] = len(sink), at, h.flush_alloc
        r["stop"] = P.DONE if done else P.SIZE_LIMITED
        ar["merged_count"], ar["carried"], ar["dropped"], ar["dud"] = len(items), len(kept), len(left) - len(kept), dud
        ar["stop"] = FA_CARRY_FULL if len(left) > len(kept) else FA_DONE
        windows_out[c]["sync_reply"] = 1 if h.sync_reply else 0
        if sink:
            assert not h.sync_reply
        else:
            windows_out[c]["sync_reply"] = Wn["sync_reply"]   # (untouched, not canonicalised)
        if not left:
            windows_out[c]["has_tail"] = 0
        ctl_out[c]["carry_count"] = len(kept)
        if flushes is not None:
            flushes[c]["flush_alloc"] = h.flush_alloc
        if flags is not None:
            flags[c] = (int(flags[c]) & ~RS_NO_DATA_FLUSH) | (0 if done else RS_NO_DATA_FLUSH)
        facts["dud"] += dud
        facts["dud_empty"] += dud and bool(sink) and not sink[0]
        facts["size_limited"] += not done
        facts["carried"] += len(kept)
        facts["dropped"] += len(left) - len(kept)
        facts["frames"] += len(sink)
    merged_first[n] = len(merged_all)
    if merged_cap is None:
        merged_cap = len(carry) + len(groups)
    if frames_cap is None:
        frames_cap = n + merged_cap
    merged = pre["merged"].copy() if "merged" in pre else np.zeros(merged_cap, dtype=ITEM_DTYPE)
    infos = pre["infos"].copy() if "infos" in pre else np.zeros(frames_cap, dtype=FRAME_INFO_DTYPE)
    for k, it in enumerate(merged_all[:merged_cap]):
        merged[k] = it
    for k, it in enumerate(infos_all[:frames_cap]):
        infos[k] = it
    return {"merged": merged, "merged_first": merged_first, "merged_used": len(merged_all), "infos": infos,
            "frames_used": len(infos_all), "results": results, "ack_results": ack_results, "windows_out": windows_out,
            "ctl_out": ctl_out, "carry": carry, "flushes": flushes, "flags": flags, "facts": facts}


def expect_sync(ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders, ticks_next=None,
                syncs_cap=None, prefill=None):
    """What ufc_flush_sync_* must leave in every output, as the wrappers' dict has them, plus "facts"."""
    n = len(ctl)
    pre = prefill or {}
    ctl_out = ctl.copy()
    ticks_next = None if ticks_next is None else ticks_next.copy()
    results = np.zeros(n, dtype=FLUSH_SYNC_RESULT_DTYPE)
    sync_index = np.full(n, NO_PARENT, dtype=np.uint32)
    frames = []
    facts = {"reasons": [0] * 7, "modes": [0] * 4, "wrapped": 0}
    for c in range(n):
        C, R, Pk, Cm, Q, S = ctl[c], rate[c], pack_results[c], commit_results[c], queues[c], senders[c]
        res = results[c]
        heap_len, pending = int(Cm["heap_len"]), int(Cm["pending_count"])
        res["heap_len"], res["pending_count"] = heap_len, pending
        res["is_send_pending"] = 1 if heap_len or pending else 0   # mod.rs:120-122, less the caller's own queue
        now, bstop = int(R["now_ms"]), int(begin_results[c]["stop"])
        h = Half(sync_timeout_base_ms=int(C["sync_timeout_base_ms"]),
                 keepalive_ms=int(C["keepalive_interval_ms"]) if C["has_keepalive"] else None)
        mode = 0
        if int(ack_results[c]["stop"]) == P.SIZE_LIMITED:      # mod.rs:218-221
            reason = FS_ACK_LIMITED
        else:
            if int(Pk["frame_count"]):                          # :342-347
                h.sync_timeout_base_ms = now
            if bstop == RS_SIZE_LIMITED or int(Pk["stop"]) == P.SIZE_LIMITED:   # :223-226
                reason = FS_DATA_LIMITED
            elif bstop in (RS_REF_HANG, RS_BAD_STATE) or int(Cm["stop"]) in (RS_REF_HANG, RS_BAD_STATE, RS_HEAP_FULL):
                reason = FS_UPSTREAM
            else:
                next_id = (int(Q["log_next_id"]) + int(Pk["frame_count"])) & M32
                nfi = next_id if next_id != int(Q["window_base_id"]) else None            # :244-249
                npi = int(S["next_id"]) if (int(S["next_id"]) != int(S["base_id"]) and heap_len == 0 and
                                            pending == 0) else None                         # :257-263
                h.flush_alloc = int(Pk["alloc_left"])
                sink = []
                if now < int(C["sync_timeout_base_ms"]) and not int(Pk["frame_count"]):
                    facts["wrapped"] += 1
                _, reason = h.emit_sync_frame(now, int(R["rto_ms"]), nfi, npi, sink)
                if sink:
                    mode = (1 if nfi is not None else 0) | (2 if npi is not None else 0)
                    info = np.zeros((), dtype=FRAME_INFO_DTYPE)
                    info["kind"], info["ok"], info["aux"] = SYNC, 1, mode
                    info["f"][0], info["f"][1] = nfi or 0, npi or 0
                    sync_index[c] = len(frames)
                    frames.append(info)
                    facts["modes"][mode] += 1
            ctl_out[c]["sync_timeout_base_ms"] = h.sync_timeout_base_ms
        if C["has_keepalive"]:   # the Option is written canonically, whatever the reason
            ctl_out[c]["has_keepalive"] = 1
        else:
            ctl_out[c]["keepalive_interval_ms"] = 0
        res["reason"], res["sent"], res["mode"] = reason, reason == FS_SENT, mode
        facts["reasons"][reason] += 1
        if ticks_next is not None:
            ticks_next[c]["alloc_adjust"] = -SYNC_FRAME_SIZE if reason == FS_SENT else 0
    if syncs_cap is None:
        syncs_cap = n
    infos = pre["infos"].copy() if "infos" in pre else np.zeros(syncs_cap, dtype=FRAME_INFO_DTYPE)
    for k, it in enumerate(frames[:syncs_cap]):
        infos[k] = it
    return {"infos": infos, "sync_index": sync_index, "syncs_used": len(frames), "results": results,
            "ctl_out": ctl_out, "ticks_next": ticks_next, "facts": facts}


# ---- inputs ----

def ack_inputs(conns, carry_cap=8, keepalive_ms=None, guard=1):
    """The arrays of an ack flush from a list of connections, each a dict: carry [(id, bitfield, nonce)] (the last
    one the stale copy of the tail), groups [(id, bitfield, nonce)] (the window's, the tail first), alloc,
    sync_reply, and optionally carry_cap, base_id, rx_base_id.  The carry rooms have `guard` records between them.
    Returns a dict of keyword arguments for flush_acks_host / expect_acks (without flushes and flags)."""
    from uflow_amd.frame import FRAME_WINDOW_DTYPE, RATE_RESULT_DTYPE, RECEIVER_DTYPE
    n = len(conns)
    ctl = np.zeros(n, dtype=FLUSH_CTL_DTYPE)
    windows = np.zeros(n, dtype=FRAME_WINDOW_DTYPE)
    receivers = np.zeros(n, dtype=RECEIVER_DTYPE)
    rate = np.zeros(n, dtype=RATE_RESULT_DTYPE)
    groups, carry = [], []
    group_first = np.zeros(n + 1, dtype=np.uint64)
    for c, d in enumerate(conns):
        cap = d.get("carry_cap", carry_cap)
        cy = d.get("carry", [])
        carry.extend([P.group(0xDEAD0000 + c, 0xFFFFFFFF, 1)] * guard)
        ctl[c]["carry_first"], ctl[c]["carry_cap"], ctl[c]["carry_count"] = len(carry), cap, len(cy)
        if keepalive_ms is not None:
            ctl[c]["has_keepalive"], ctl[c]["keepalive_interval_ms"] = 1, keepalive_ms
        ctl[c]["reserved0"], ctl[c]["reserved1"], ctl[c]["reserved2"] = 0xA5, 0xBEEF, 0xC0FFEE00 + c
        room = [P.group(*g) for g in cy] + [P.group(0xFEED0000 + c, 0x55555555, 1)] * (cap - min(len(cy), cap))
        carry.extend(room)
        gs = d.get("groups", [])
        groups.extend(P.group(*g) for g in gs)
        group_first[c + 1] = len(groups)
        w = windows[c]
        w["base_id"], w["size"] = d.get("base_id", 1000 + c), 64
        w["sync_reply"] = d.get("sync_reply", 0)
        w["reserved"], w["reserved2"] = 0x3C, 0x12345678
        if gs:
            w["has_tail"] = 1
            w["tail_base_id"], w["tail_bitfield"], w["tail_nonce"] = gs[-1]
        receivers[c]["base_id"] = d.get("rx_base_id", 77 + c)
        rate[c]["flush_alloc"] = d.get("alloc", 1 << 40)
    carry.extend([P.group(0xDEADFFFF, 0xFFFFFFFF, 1)] * guard)
    return {"ctl": ctl, "windows": windows,
            "groups": np.array(groups, dtype=ITEM_DTYPE) if groups else np.zeros(0, ITEM_DTYPE),
            "group_first": group_first, "receivers": receivers, "rate": rate,
            "carry": np.array(carry, dtype=ITEM_DTYPE) if carry else np.zeros(0, ITEM_DTYPE)}


def tile_acks(inp, times):
    """`times` copies of a batch in one: the carry rooms and the group ranges of copy k behind those of copy k - 1."""
    n, n_carry, n_groups = len(inp["ctl"]), inp["carry"].size, inp["groups"].size
    out = {k: np.tile(inp[k], times) for k in ("ctl", "windows", "groups", "receivers", "rate", "carry")}
    out["ctl"]["carry_first"] += np.repeat(np.arange(times, dtype=np.uint64) * np.uint64(n_carry), n)
    gf = inp["group_first"][:-1][None, :] + (np.arange(times, dtype=np.uint64) * np.uint64(n_groups))[:, None]
    out["group_first"] = np.append(gf.reshape(-1), np.uint64(times * n_groups)).astype(np.uint64)
    return out


def seq_groups(n, start=5, nonce_seed=0):
    """n distinct ack groups with ids 40 apart (no two within one bitfield)."""
    return [((start + 40 * k) & M32, (1 | (k * 2654435761)) & M32, (k + nonce_seed) & 1) for k in range(n)]


def rand_ack_conn(rng, max_groups=12):
    """A seeded connection: a consistent carry (its last id the window's first), some groups, an alloc around the
    frame sizes, sync_reply now and then."""
    n_carry = int(rng.integers(0, 5)) if rng.integers(0, 3) == 0 else 0
    n_groups = int(rng.integers(0, max_groups + 1))
    if n_carry and not n_groups:
        n_groups = 1
    all_g = seq_groups(n_carry + n_groups - (1 if n_carry else 0), start=int(rng.integers(0, 1 << 32)),
                       nonce_seed=int(rng.integers(0, 2)))
    carry = all_g[:n_carry]
    groups = all_g[n_carry - 1:] if n_carry else all_g
    if n_carry:  # the tail moved on since it was carried
        carry = carry[:-1] + [(carry[-1][0], carry[-1][1] & 0x0F0F0F0F | 1, carry[-1][2] ^ 1)]
    alloc = [1 << 40, -1, 0, 14, 15, 23, 24, int(rng.integers(-5, 200)), int(rng.integers(0, 3000))][int(rng.integers(0, 9))]
    return dict(carry=carry, groups=groups, alloc=alloc, sync_reply=int(rng.integers(0, 4) == 0) * int(rng.integers(1, 256)),
                carry_cap=[0, 1, 2, 8, 8, 8][int(rng.integers(0, 6))] if not n_carry else 8)


def sync_inputs(conns):
    """The arrays of a sync decision from a list of connections, each a dict with any of: base_ms, keepalive_ms,
    now_ms, rto_ms, ack_stop, begin_stop, pack_stop, commit_stop, frame_count, alloc_left, heap_len, pending_count,
    log_next_id, window_base_id, base_id, next_id.  The defaults are a quiet connection long past its timeout with
    nothing outstanding.  Returns a dict of keyword arguments for flush_sync_host / expect_sync."""
    from uflow_amd.frame import (FRAME_QUEUE_DTYPE, RATE_RESULT_DTYPE, RATE_TICK_DTYPE, RESEND_COMMIT_RESULT_DTYPE,
                                 RESEND_RESULT_DTYPE, SENDER_DTYPE)
    n = len(conns)
    ctl = np.zeros(n, dtype=FLUSH_CTL_DTYPE)
    rate = np.zeros(n, dtype=RATE_RESULT_DTYPE)
    ack = np.zeros(n, dtype=FLUSH_RESULT_DTYPE)
    begin = np.zeros(n, dtype=RESEND_RESULT_DTYPE)
    pack = np.zeros(n, dtype=FLUSH_RESULT_DTYPE)
    commit = np.zeros(n, dtype=RESEND_COMMIT_RESULT_DTYPE)
    queues = np.zeros(n, dtype=FRAME_QUEUE_DTYPE)
    senders = np.zeros(n, dtype=SENDER_DTYPE)
    ticks = np.zeros(n, dtype=RATE_TICK_DTYPE)
    for c, d in enumerate(conns):
        ctl[c]["sync_timeout_base_ms"] = d.get("base_ms", 1000)
        ka = d.get("keepalive_ms")
        if ka is not None:
            ctl[c]["has_keepalive"], ctl[c]["keepalive_interval_ms"] = d.get("has_keepalive", 1), ka
        else:
            ctl[c]["keepalive_interval_ms"] = d.get("stale_interval", 0)   # (ignored, written 0)
        ctl[c]["carry_first"], ctl[c]["carry_cap"], ctl[c]["carry_count"] = 8 * c, 8, c % 3
        ctl[c]["reserved0"], ctl[c]["reserved1"], ctl[c]["reserved2"] = 0x5A, 0xF00D, 0xABCD0000 + c
        rate[c]["now_ms"], rate[c]["rto_ms"] = d.get("now_ms", 100000), d.get("rto_ms", 600)
        ack[c]["stop"], begin[c]["stop"] = d.get("ack_stop", 0), d.get("begin_stop", 0)
        pack[c]["stop"], pack[c]["frame_count"] = d.get("pack_stop", 0), d.get("frame_count", 0)
        pack[c]["alloc_left"] = d.get("alloc_left", 5000)
        commit[c]["stop"], commit[c]["heap_len"] = d.get("commit_stop", 0), d.get("heap_len", 0)
        commit[c]["pending_count"] = d.get("pending_count", 0)
        queues[c]["log_next_id"] = d.get("log_next_id", 500)
        queues[c]["window_base_id"] = d.get("window_base_id", d.get("log_next_id", 500))
        senders[c]["base_id"] = d.get("base_id", 30)
        senders[c]["next_id"] = d.get("next_id", d.get("base_id", 30))
        ticks[c]["now_ms"], ticks[c]["delta_time_s"], ticks[c]["alloc_adjust"] = 777 + c, 0.25, 123456
        ticks[c]["flags"], ticks[c]["reserved"] = 1, 0x99
    return {"ctl": ctl, "rate": rate, "ack_results": ack, "begin_results": begin, "pack_results": pack,
            "commit_results": commit, "queues": queues, "senders": senders, "ticks_next": ticks}


def rand_sync_conn(rng):
    now = int(rng.integers(0, 1 << 40))
    rto = [600, 1999, 2000, 2001, 5000][int(rng.integers(0, 5))]
    timeout = max(rto, MIN_SYNC_TIMEOUT_MS)
    elapsed = [timeout - 1, timeout, timeout + int(rng.integers(0, 10000)), int(rng.integers(0, timeout))][int(rng.integers(0, 4))]
    d = dict(now_ms=now, rto_ms=rto, base_ms=(now - elapsed) & M64)
    u = int(rng.integers(0, 16))
    if u == 0:
        d["ack_stop"] = P.SIZE_LIMITED
    elif u == 1:
        d["begin_stop"] = int(rng.integers(1, 6))
    elif u == 2:
        d["pack_stop"] = int(rng.integers(1, 4))
    elif u == 3:
        d["commit_stop"] = [RS_BAD_STATE, RS_HEAP_FULL][int(rng.integers(0, 2))]
    if rng.integers(0, 4) == 0:
        d["frame_count"] = int(rng.integers(1, 4))
    d["log_next_id"] = int(rng.integers(0, 1 << 32))
    if rng.integers(0, 2):
        d["window_base_id"] = (d["log_next_id"] + d.get("frame_count", 0) - int(rng.integers(0, 3))) & M32
    d["base_id"] = int(rng.integers(0, 1 << 20))
    d["next_id"] = (d["base_id"] + int(rng.integers(0, 3))) & 0xFFFFF
    d["heap_len"], d["pending_count"] = int(rng.integers(0, 4) == 0), int(rng.integers(0, 4) == 0)
    if rng.integers(0, 2):
        d["keepalive_ms"] = [elapsed - 1, elapsed, elapsed + 1, 0][int(rng.integers(0, 4))] & M64
    d["alloc_left"] = [-1, 0, 13, 14, 5000][int(rng.integers(0, 5))]
    return d
