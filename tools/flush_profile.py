"""The workload behind the flush control's kernel times: ufc_flush_acks_varlen and
ufc_flush_sync_varlen at 250,000 and at 2,048 connections, each call `--reps` times, beside a device-to-device copy
of (bytes read + bytes written) / 2 of the call, the yardstick of 5.13 and 5.14.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/flush_profile.py`: the kernels' times are read from the trace
(fa_count_kernel, fa_write_kernel, fs_decide_kernel, fs_write_kernel and the scans between them); the JSON line this
prints holds the event-pair times of the whole calls and of the copies, and the byte counts.

Traffic: per connection 0 to 3 window groups (a third of them none), one in four owing a sync reply, one in three
with a carry of 1 to 4 groups in a room of 4, allocations from generous to negative (tests/flush_expect.py's
rand_ack_conn, 1,000 seeded connections repeated); for the sync decision tests/flush_expect.py's rand_sync_conn.
The carry rooms are restored from a pristine copy in front of every ack call, outside the timed span.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from uflow_amd import flush as fl, frame as fr  # noqa: E402
from uflow_amd.batch import FrameCrcEngine, records, rows  # noqa: E402
import flush_expect as E  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, before=None):
    ms = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def copy_ms(nbytes, reps):
    src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    eng = FrameCrcEngine(0)
    rng = np.random.default_rng(17)
    base = E.ack_inputs([E.rand_ack_conn(rng, max_groups=3) for _ in range(1000)], guard=0, carry_cap=4)
    sbase = E.sync_inputs([E.rand_sync_conn(rng) for _ in range(1000)])
    out = {}
    for n in (250000, 2048):
        times = (n + 999) // 1000
        inp = {k: v[:n] if k not in ("groups", "carry", "group_first") else v for k, v in E.tile_acks(base, times).items()}
        inp["group_first"] = inp["group_first"][:n + 1]
        d = {k: rows(v, DEV) for k, v in inp.items()}
        pristine = d["carry"].clone()
        flushes = torch.zeros((n, fr.FLUSH_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
        flags = torch.zeros(n, dtype=torch.int32, device=DEV)
        o = {}

        def acks():
            o.update(eng.flush_acks(d["ctl"], d["windows"], d["groups"], d["group_first"], d["receivers"], d["rate"],
                                    d["carry"], flushes=flushes, flags=flags, merged=o.get("merged"), infos=o.get("infos"),
                                    windows_out=o.get("windows_out"), ctl_out=o.get("ctl_out")))

        acks()
        torch.cuda.synchronize()
        h = fl.flush_acks_host(inp["ctl"], inp["windows"], inp["groups"], inp["group_first"], inp["receivers"], inp["rate"],
                               inp["carry"].copy(), nthreads=16)
        assert records(o["results"], fr.FLUSH_RESULT_DTYPE).tobytes() == h["results"].tobytes()
        m, f = h["merged_used"], h["frames_used"]
        moved = int(h["ack_results"]["carried"].sum())
        read = n * (40 + 24 + 8 + 4 + 8 + 4) + 24 * m   # ctl, window, group_first, base_id, flush_alloc, flags; the groups
        written = 24 * (m + moved) + 32 * f + n * (8 + 24 + 24 + 24 + 40 + 8 + 4)
        a_ms = timed(acks, args.reps, before=lambda: d["carry"].copy_(pristine))
        s = {k: rows(np.tile(v, times)[:n], DEV) for k, v in sbase.items()}
        so = {}

        def sync():
            so.update(eng.flush_sync(s["ctl"], s["rate"], s["ack_results"], s["begin_results"], s["pack_results"],
                                     s["commit_results"], s["queues"], s["senders"], ticks_next=s["ticks_next"],
                                     infos=so.get("infos"), ctl_out=so.get("ctl_out")))

        sync()
        torch.cuda.synchronize()
        sent = int(so["syncs_used"].cpu()[0])
        s_read = n * (40 + 16 + 4 + 4 + 16 + 12 + 8 + 8)
        s_written = n * (24 + 40 + 8 + 4) + 32 * sent
        s_ms = timed(sync, args.reps)
        out[str(n)] = {"connections": n, "merged_groups": m, "ack_frames": f, "groups_carried": moved,
                       "acks_call_ms": round(a_ms, 4), "acks_bytes_read": read, "acks_bytes_written": written,
                       "acks_copy_ms": round(copy_ms((read + written) // 2, args.reps), 4),
                       "sync_frames": sent, "sync_call_ms": round(s_ms, 4), "sync_bytes_read": s_read,
                       "sync_bytes_written": s_written, "sync_copy_ms": round(copy_ms((s_read + s_written) // 2, args.reps), 4)}
    print(json.dumps({"flush_profile": out, "reps": args.reps}))


if __name__ == "__main__":
    main()
