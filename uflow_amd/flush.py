"""The batched flush control in host memory (include/uflow_flush_ctl.h), beside uflow_amd.frame's stages:

    new_flush_ctl(n, keepalive_ms, carry_cap)  <- the flush-control fields of HalfConnection::new
    flush_acks_host(ctl, windows, groups, group_first, receivers, rate, carry)
                                               <- emit_ack_frames with push_dud and the deque carry
                                                  (src/half_connection/mod.rs:296-333, emit.rs:137-211)
    flush_sync_host(ctl, rate, ack_results, begin_results, pack_results, commit_results, queues, senders)
                                               <- emit_sync_frame and emit_frames' early returns (mod.rs:217-294)
    (device-resident: uflow_amd.batch.FrameCrcEngine.flush_acks / flush_sync)

The wrappers go through frame.py's one marshalling path (_in, _inout, _p).  The stage has a module of its own
because its C declarations have a header of their own; tests/test_flush_cpu.py holds its records, signatures and
argument checks to that header as tests/test_records_cpu.py and tests/test_host_args_cpu.py hold frame.py's.
"""
from typing import Optional

import numpy as np

from ._native import check, lib
# The stage's constants without their prefix: each value is written once, in _native.
from ._native import (  # noqa: F401
    UFC_FA_DONE as FA_DONE, UFC_FA_BAD_STATE as FA_BAD_STATE, UFC_FA_CARRY_FULL as FA_CARRY_FULL,
    UFC_FS_SENT as FS_SENT, UFC_FS_ACK_LIMITED as FS_ACK_LIMITED, UFC_FS_DATA_LIMITED as FS_DATA_LIMITED,
    UFC_FS_UPSTREAM as FS_UPSTREAM, UFC_FS_NOT_DUE as FS_NOT_DUE, UFC_FS_IDLE as FS_IDLE,
    UFC_FS_NO_ALLOC as FS_NO_ALLOC)
from .frame import _U32, _U64, _in, _inout, _p
from .records import (  # noqa: F401
    FLUSH_ACKS_RESULT_DTYPE, FLUSH_CTL_DTYPE, FLUSH_DTYPE, FLUSH_RESULT_DTYPE, FLUSH_SYNC_RESULT_DTYPE, FRAME_INFO_DTYPE,
    FRAME_QUEUE_DTYPE, FRAME_WINDOW_DTYPE, ITEM_DTYPE, RATE_RESULT_DTYPE, RATE_TICK_DTYPE, RECEIVER_DTYPE,
    RESEND_COMMIT_RESULT_DTYPE, RESEND_RESULT_DTYPE, SENDER_DTYPE)


def new_flush_ctl(n: int, keepalive_ms=None, carry_cap: int = 8):
    """n ufc_flush_ctl records of a new HalfConnection (sync_timeout_base_ms 0, nothing carried) and their carry
    arena: returns (ctl, carry).  keepalive_ms: config.keepalive_interval_ms, None for no keepalive.  Every
    connection's carry has room for carry_cap ack groups; the rooms lie back to back, carry_first = c * carry_cap."""
    c = np.zeros(n, dtype=FLUSH_CTL_DTYPE)
    if keepalive_ms is not None:
        c["has_keepalive"] = 1
        c["keepalive_interval_ms"] = keepalive_ms
    c["carry_cap"] = carry_cap
    c["carry_first"] = np.arange(n, dtype=np.uint64) * np.uint64(carry_cap)
    return c, np.zeros(n * int(carry_cap), dtype=ITEM_DTYPE)


def flush_acks_host(ctl: np.ndarray, windows: np.ndarray, groups: np.ndarray, group_first: np.ndarray,
                    receivers: np.ndarray, rate: np.ndarray, carry: np.ndarray, merged_cap: Optional[int] = None,
                    frames_cap: Optional[int] = None, flushes: Optional[np.ndarray] = None,
                    flags: Optional[np.ndarray] = None, nthreads: int = 1, merged: Optional[np.ndarray] = None,
                    infos: Optional[np.ndarray] = None, windows_out: Optional[np.ndarray] = None,
                    ctl_out: Optional[np.ndarray] = None):
    """ufc_flush_acks_host: emit_ack_frames for every connection, behind frame_window_host and rate_step_host and in
    front of resend_begin_host.  ctl (FLUSH_CTL_DTYPE) with carry (ITEM_DTYPE, the arena new_flush_ctl returns,
    updated in place); windows, groups and group_first as frame_window_host left them; receivers (RECEIVER_DTYPE,
    base_id is read); rate (RATE_RESULT_DTYPE, flush_alloc is read).  flushes (FLUSH_DTYPE, the data flushes) and
    flags (uint32) are optional and updated in place.  Returns a dict: merged (ITEM_DTYPE), merged_first (uint64 CSR:
    the flush_first of the ack flushes), merged_used, infos (the ack frames, as build_batch_host takes them over
    merged), frames_used, results (FLUSH_RESULT_DTYPE), ack_results (FLUSH_ACKS_RESULT_DTYPE), windows_out and
    ctl_out (may be given as `windows` and `ctl`), carry, flushes, flags.  merged_cap defaults to carry.size +
    groups.size and frames_cap to n + merged_cap, which are always enough."""
    ctl = _in("ctl", ctl, FLUSH_CTL_DTYPE)
    n = ctl.size
    windows = _in("windows", windows, FRAME_WINDOW_DTYPE, n)
    groups = _in("groups", groups, ITEM_DTYPE)
    group_first = _in("group_first", group_first, _U64, n + 1)
    receivers = _in("receivers", receivers, RECEIVER_DTYPE, n)
    rate = _in("rate", rate, RATE_RESULT_DTYPE, n)
    carry = _inout("carry", carry, ITEM_DTYPE)
    if merged_cap is None:
        merged_cap = merged.size if merged is not None else carry.size + groups.size
    merged_cap = int(merged_cap)
    if frames_cap is None:
        frames_cap = infos.size if infos is not None else n + merged_cap
    frames_cap = int(frames_cap)
    merged = _inout("merged", merged, ITEM_DTYPE, merged_cap)
    infos = _inout("infos", infos, FRAME_INFO_DTYPE, frames_cap)
    if flushes is not None:
        flushes = _inout("flushes", flushes, FLUSH_DTYPE, n)
    if flags is not None:
        flags = _inout("flags", flags, _U32, n)
    merged_first = np.zeros(n + 1, dtype=np.uint64)
    results = np.zeros(n, dtype=FLUSH_RESULT_DTYPE)
    ack_results = np.zeros(n, dtype=FLUSH_ACKS_RESULT_DTYPE)
    windows_out = _inout("windows_out", windows_out, FRAME_WINDOW_DTYPE, n)
    ctl_out = _inout("ctl_out", ctl_out, FLUSH_CTL_DTYPE, n)
    used = np.zeros(2, dtype=np.uint64)
    check(lib().ufc_flush_acks_host(_p(ctl), _p(windows), _p(groups), groups.size, group_first.ctypes.data,
                                    _p(receivers), _p(rate), n, _p(carry), carry.size,
                                    merged.ctypes.data if merged_cap else None, merged_cap, merged_first.ctypes.data,
                                    used[0:].ctypes.data, infos.ctypes.data if frames_cap else None, frames_cap,
                                    used[1:].ctypes.data, _p(results), _p(ack_results), _p(windows_out), _p(ctl_out),
                                    _p(flushes), _p(flags), nthreads), "ufc_flush_acks_host")
    return {"merged": merged, "merged_first": merged_first, "merged_used": int(used[0]), "infos": infos,
            "frames_used": int(used[1]), "results": results, "ack_results": ack_results, "windows_out": windows_out,
            "ctl_out": ctl_out, "carry": carry, "flushes": flushes, "flags": flags}


def flush_sync_host(ctl: np.ndarray, rate: np.ndarray, ack_results: np.ndarray, begin_results: np.ndarray,
                    pack_results: np.ndarray, commit_results: np.ndarray, queues: np.ndarray, senders: np.ndarray,
                    syncs_cap: Optional[int] = None, ticks_next: Optional[np.ndarray] = None, nthreads: int = 1,
                    infos: Optional[np.ndarray] = None, ctl_out: Optional[np.ndarray] = None):
    """ufc_flush_sync_host: emit_sync_frame and the early returns of emit_frames for every connection, behind the
    data flush's last call.  ctl (FLUSH_CTL_DTYPE); rate (RATE_RESULT_DTYPE: now_ms, rto_ms); ack_results
    (FLUSH_RESULT_DTYPE, flush_acks_host's results); begin_results (RESEND_RESULT_DTYPE); pack_results
    (FLUSH_RESULT_DTYPE, the data pack's); commit_results (RESEND_COMMIT_RESULT_DTYPE); queues (FRAME_QUEUE_DTYPE,
    after this tick's frame_queue_host) and senders (SENDER_DTYPE, as the second emit left them).  ticks_next
    (RATE_TICK_DTYPE, optional) gets alloc_adjust = -14 or 0 in place.  Returns a dict: infos (the sync frames in
    connection order, as build_batch_host takes them), sync_index (uint32 per connection, NO_PARENT for none),
    syncs_used, results (FLUSH_SYNC_RESULT_DTYPE), ctl_out (may be given as `ctl`), ticks_next.  syncs_cap defaults
    to n, which is always enough."""
    ctl = _in("ctl", ctl, FLUSH_CTL_DTYPE)
    n = ctl.size
    rate = _in("rate", rate, RATE_RESULT_DTYPE, n)
    ack_results = _in("ack_results", ack_results, FLUSH_RESULT_DTYPE, n)
    begin_results = _in("begin_results", begin_results, RESEND_RESULT_DTYPE, n)
    pack_results = _in("pack_results", pack_results, FLUSH_RESULT_DTYPE, n)
    commit_results = _in("commit_results", commit_results, RESEND_COMMIT_RESULT_DTYPE, n)
    queues = _in("queues", queues, FRAME_QUEUE_DTYPE, n)
    senders = _in("senders", senders, SENDER_DTYPE, n)
    if syncs_cap is None:
        syncs_cap = infos.size if infos is not None else n
    syncs_cap = int(syncs_cap)
    infos = _inout("infos", infos, FRAME_INFO_DTYPE, syncs_cap)
    if ticks_next is not None:
        ticks_next = _inout("ticks_next", ticks_next, RATE_TICK_DTYPE, n)
    sync_index = np.zeros(n, dtype=np.uint32)
    results = np.zeros(n, dtype=FLUSH_SYNC_RESULT_DTYPE)
    ctl_out = _inout("ctl_out", ctl_out, FLUSH_CTL_DTYPE, n)
    used = np.zeros(1, dtype=np.uint64)
    check(lib().ufc_flush_sync_host(_p(ctl), _p(rate), _p(ack_results), _p(begin_results), _p(pack_results),
                                    _p(commit_results), _p(queues), _p(senders), n,
                                    infos.ctypes.data if syncs_cap else None, syncs_cap, _p(sync_index),
                                    used.ctypes.data, _p(results), _p(ctl_out), _p(ticks_next), nthreads),
          "ufc_flush_sync_host")
    return {"infos": infos, "sync_index": sync_index, "syncs_used": int(used[0]), "results": results,
            "ctl_out": ctl_out, "ticks_next": ticks_next}
