"""The workload behind the frame routing's kernel times: ufc_route_frames_varlen over the parse_mtu
batch (tools/bench_configs.py: 1M uflow frames <= MAX_FRAME_SIZE, gated and parsed on the device), its frames'
addresses interleaved across 250,000 and across 2,048 connections, round-robin and at random, each call `--reps`
times.  Beside it, in the same process: a device-to-device copy of (bytes read + bytes written) / 2 of the call, the
yardstick of 5.13 and 5.14, and the parse of the same batch.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/route_profile.py --only 250000:random` under a time limit, one
configuration per traced run so that the stats are that configuration's: the kernels' times are read from the trace
(rt_init_kernel, rt_lookup_kernel, rt_classify_kernel, rt_hist_kernel, rt_scatter_kernel, rt_gather_kernel,
rt_finish_kernel and the scans between them); the JSON line this prints holds the event-pair times of the whole calls,
of the copies and of the parse, and the byte counts.

Traffic: every connection active, 1 frame in 1,000 from an unknown address, and about 1 connection in 1,000 sending
one control frame (a disconnect) somewhere in the batch, which defers its later frames, so that all four classes
occur; the outputs are checked against ufc_route_frames_host once.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from uflow_amd import frame as fr, route as rt  # noqa: E402
from uflow_amd.batch import FrameCrcEngine, records, rows  # noqa: E402
from bench_configs import parse_batch, settle  # noqa: E402

DEV = "cuda:0"
CONFIGS = ("250000:rr", "250000:random", "2048:rr", "2048:random")


def timed(fn, reps):
    ms = []
    for _ in range(reps):
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
    ap.add_argument("--only", default=",".join(CONFIGS))
    ap.add_argument("--frames", type=int, default=1_000_000)
    args = ap.parse_args()
    eng = FrameCrcEngine(0)
    n = args.frames
    data, offsets, _ = parse_batch(n, True)
    d, o = torch.from_numpy(data).to(DEV), torch.from_numpy(offsets).to(DEV)
    _, valid = eng.crc_varlen(d, o)
    infos, items, _ = eng.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    cap = items.shape[0]
    parse = lambda: eng.parse_varlen(d, o, valid, items_cap=cap)  # noqa: E731
    settle(parse)
    parse_ms = timed(parse, args.reps)
    h_infos = records(infos, fr.FRAME_INFO_DTYPE)
    src_base = o[:-1]
    out = {}
    for cfg in args.only.split(","):
        nc, how = cfg.split(":")
        nc = int(nc)
        rng = np.random.default_rng(nc)
        conn = np.zeros(nc, dtype=rt.ADDR_DTYPE)
        conn["family"], conn["port"] = 4, 7000
        conn["ip"][:, :4] = (np.arange(nc, dtype=np.uint32) + 0x0A000000).astype(">u4").view(np.uint8).reshape(-1, 4)
        table = rt.new_route_table(conn, int(rng.integers(0, 2**32)))
        who = np.arange(n) % nc if how == "rr" else rng.integers(0, nc, n)
        addrs = conn[who]
        addrs["port"][rng.random(n) < 0.001] = 1
        fi = h_infos.copy()
        fi["kind"][rng.choice(n, max(1, nc // 1000), replace=False)] = 4
        active, tin = np.ones(nc, dtype=np.uint8), np.zeros(nc, dtype=np.uint64)
        t = dict(infos=rows(fi, DEV), addrs=rows(addrs, DEV), slots=rows(table.slots, DEV), active=rows(active, DEV),
                 tin=rows(tin, DEV))
        r = {}

        def call():
            r.update(eng.route_frames(t["infos"], t["addrs"], src_base, t["slots"], table.seed, table.max_probe,
                                      t["active"], 1000, 5000, t["tin"], infos_out=r.get("infos_out"),
                                      src_base_out=r.get("src_base_out"), timeout_out=r.get("timeout_out")))

        call()
        torch.cuda.synchronize()
        h = rt.route_frames_host(fi, addrs, offsets[:-1].astype(np.uint64), table, active, 1000, 5000, tin, nthreads=16)
        for k, dt in (("order", np.uint32), ("cls", np.uint8), ("bucket_first", np.uint64),
                      ("infos_out", fr.FRAME_INFO_DTYPE), ("results", rt.ROUTE_RESULT_DTYPE)):
            assert records(r[k], dt).tobytes() == h[k].tobytes(), k
        # what the caller sees move: infos, addrs, offsets and about one slot per frame in; route, cls, order, infos_out,
        # src_base_out out; per connection the flag and timeout in, bucket_first, results and timeout out
        read = n * (32 + 32 + 8 + 48) + nc * (1 + 8)
        written = n * (4 + 1 + 4 + 32 + 8) + nc * (8 + 16 + 8)
        settle(call, 300)
        ms = timed(call, args.reps)
        cls = h["cls"]
        out[cfg] = {"frames": n, "connections": nc, "addresses": how, "slots": int(table.slots.size),
                    "max_probe": table.max_probe, "passes": 1 + (nc + 1 > 255) + (nc + 1 > 65535),
                    "conn_frames": int((cls == rt.ROUTE_CONN).sum()), "control": int((cls == rt.ROUTE_CONTROL).sum()),
                    "deferred": int((cls == rt.ROUTE_DEFERRED).sum()), "dropped": int((cls == rt.ROUTE_DROP).sum()),
                    "call_ms": round(ms, 4), "bytes_read": read, "bytes_written": written,
                    "copy_ms": round(copy_ms((read + written) // 2, args.reps), 4)}
        del t, r
    print(json.dumps({"route_profile": out, "parse_ms": round(parse_ms, 4), "reps": args.reps}))


if __name__ == "__main__":
    main()
