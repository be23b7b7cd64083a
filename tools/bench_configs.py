"""Secondary measurements for DESIGN.md (BASELINE.json configs 3, 4-per-GPU and 5, the seal and the
parse), one JSON line each.  Not the driver's bench (bench.py is); run on the GPU box:
    python tools/bench_configs.py [--only varlen,shard,seal,seal_varlen,parse,parse_mtu,build,pack,emit,receive,window,queue,rate,resend,gate_tg,host] [--reps 20]

  varlen   config 3: 10M frames, lengths U[64,1500] (splitmix64, seed 0x5EED0002), CSR offsets,
           device-resident; every frame checked against the oracle; CPU baseline of the same loop
           (1 thread and all threads) on a sample.
  shard    config 4, one GPU's shard: frames [37.5M, 50M) of the 100M-frame batch (seed 0x5EED0003),
           18.75 GB device-resident (3 launches of the lean kernel).
  seal     the encode side of config 2: 1M x 1500-B frames sealed in place on the device.
  parse    Frame::read past the gate on the device (ufc_parse_batch_varlen): 1M real uflow frames from
           the reference's test generators (38 % longer than MAX_FRAME_SIZE).
  parse_mtu  the same with frames <= MAX_FRAME_SIZE only (what a uflow receiver gets).
  build    Frame::write on the device (ufc_build_sizes_varlen / ufc_build_batch_varlen): the parse_mtu batch
           gated and parsed, then built again from its records with the batch itself as payload source;
           the sizes call, the write call (seal = 0) and the seal that follows timed separately, and a
           device-to-device copy of the same output bytes as the floor.  Run with --only build.
  pack     the emitters' push / finalize on the device (ufc_pack_varlen): the parse_mtu batch's datagram
           records regrouped into many short and into a few thousand long flushes; the pack, ufc_pack_host
           with 1 and 16 threads on the same records and the build's write call over the packed frames, one
           line per grouping.  Run with --only pack.
  emit     queued packets into datagram items on the device (ufc_emit_packets_varlen): synthetic send queues as
           many short and as a few thousand long ones; the emit, ufc_emit_packets_host with 1 and 16 threads
           on the same records and ufc_pack_varlen over the items produced, one line per grouping.  Run with
           --only emit.
  receive  datagram items into delivered packets on the device (ufc_receive_packets_varlen): the parse_mtu
           batch's datagrams as many small receivers and as 2048 receivers; the receive, ufc_receive_packets_host
           with 1 thread on the same records and a device-to-device copy of the delivered bytes, one line per
           grouping.  Run with --only receive.
  window   parsed frames into accept verdicts and ack groups on the device (ufc_frame_window_varlen): the parse_mtu
           batch's frames as 250,000 connections and as 2,048; the call, ufc_frame_window_host with 1 and 16
           threads on the same records and a plain device read of the records as the floor, one line per
           grouping, also written to profiles/window_configs.jsonl.  Run with --only window.
  queue    parsed ack frames into acked fragments, the transfer window and feedback on the device
           (ufc_frame_queue_varlen): 1M synthesized ack frames over filled logs, as 250,000 connections and as 2,048;
           the call and ufc_frame_queue_host with 1 and 16 threads; one line per grouping, also written to
           profiles/queue_configs.jsonl.  Run with --only queue.
  rate     the send rate control behind the frame queue on the device (ufc_rate_step_varlen): one tick of 250,000
           and of 2,048 connections in a mix of modes, most with feedback; the call, ufc_rate_step_host with 1 and 16
           threads and a device-to-device copy of the bytes the call reads and writes; one line per grouping, also
           written to profiles/rate_configs.jsonl.  Run with --only rate.
  resend   the three resend calls of one tick (begin, place, commit) for 250,000 and 2,048 connections with heaps that
           earlier ticks filled, each timed on the device and on the host, against a copy of the bytes they move;
           written to profiles/resend_configs.jsonl.  Run with --only resend.
  host     config 5's GPU leg: 1M x 1472-B frames (uflow's MAX_FRAME_SIZE) that start and end in
           host memory -> ufc_validate_host_varlen (H2D + CRC + D2H) from pinned and from pageable
           buffers; GiB/s of frame bytes including the copies.
Kernel times: HIP events around groups of 10 back-to-back launches on the current stream (median
over the groups of --reps launches); ceiling_GBs = ufc_hbm_read_probe (a plain read-only stream) over
the same buffer, timed the same way.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402  (the checker and the CPU baseline only)
from uflow_amd import frame as fr, synth  # noqa: E402
from uflow_amd.batch import FrameCrcEngine, records, rows  # noqa: E402

PEAK = 8e12
CHECK = True  # --no-check: skip the oracle comparisons and CPU baselines


def zrows(n, dtype, dev):
    """n zeroed device rows of a record dtype (what the stage calls write their records into)."""
    return torch.zeros((n, dtype.itemsize), dtype=torch.uint8, device=dev)


def timed(fn, reps, group=10):
    """HIP events around groups of `group` back-to-back launches on the current stream (as bench.py:
    an event pair around every launch adds ~6 us); returns (median, mean) ms per launch over the
    ceil(reps / group) groups."""
    s = torch.cuda.current_stream()
    ng = max(1, -(-reps // group))
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ng)]
    for e0, e1 in evs:
        e0.record(s)
        for _ in range(group):
            fn()
        e1.record(s)
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) / group for a, b in evs]
    return float(np.median(t)), float(np.mean(t))


def ceiling(eng, buf, reps):
    """Read-only streaming ceiling over the same bytes (ufc_hbm_read_probe): GB/s."""
    sink = torch.zeros(1, dtype=torch.int32, device=buf.device)
    nbytes = eng.hbm_read_probe(buf, sink)
    settle(lambda: eng.hbm_read_probe(buf, sink), 20)
    med, _ = timed(lambda: eng.hbm_read_probe(buf, sink), reps)
    return round(nbytes / med / 1e-3 / 1e9, 1)


def settle(fn, ms=1000):
    """Launches for `ms` before timing: a GPU out of idle runs at reduced clocks for up to ~1 s."""
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        fn()
        torch.cuda.synchronize()


def threads():
    """The process's effective CPU share (cgroup quota, else the box's declared share, never more
    than the affinity mask): bench.py's cpu_baseline rule."""
    from bench import effective_cpus
    return effective_cpus()[0]


def rates(name, nbytes, algo, med, mean, ceil_gbs=None, **kw):
    r = {"config": name, "kernel_ms": round(med, 4), "kernel_mean_ms": round(mean, 4),
         "GiB_s": round(nbytes / med / 1e-3 / 2**30, 1), "algo_GB_s": round(algo / med / 1e-3 / 1e9, 1),
         "hbm_frac": round(algo / med / 1e-3 / PEAK, 4), "algorithmic_bytes": algo}
    if ceil_gbs:
        r["ceiling_GBs"] = ceil_gbs
        r["frac_of_ceiling"] = round(algo / med / 1e-3 / 1e9 / ceil_gbs, 4)
    r.update(kw)
    return r


def varlen(eng, dev, reps, n=10_000_000):
    data, offsets = synth.varlen_batch(n, 64, 1500, synth.SEED_CONFIG3, device=dev)
    eng.seal_varlen(data, offsets)
    flipped = torch.arange(0, n, 997, device=dev)
    synth.flip_bits(data, offsets[flipped], byte_in_frame=7, mask=0x20)
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    fn = lambda: eng.crc_varlen(data, offsets, crc_out=crc, valid_out=valid)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    total = int(offsets[-1])
    settle(fn)
    med, mean = timed(fn, reps)
    ceil_gbs = ceiling(eng, data, reps)
    algo = total + 8 * (n + 1) + 4 * n + n
    # A/B: the generic kernel on the same batch (the same results, timed beside the product kernel)
    from uflow_amd import _native as N
    other = N.UFC_VARLEN_GENERIC
    saved = eng.get_option(N.UFC_OPT_VARLEN_KERNEL)
    eng.set_option(N.UFC_OPT_VARLEN_KERNEL, other)
    crc2 = torch.empty(n, dtype=torch.int32, device=dev)
    valid2 = torch.empty(n, dtype=torch.uint8, device=dev)
    fn2 = lambda: eng.crc_varlen(data, offsets, crc_out=crc2, valid_out=valid2)  # noqa: E731
    fn2()
    torch.cuda.synchronize()
    same = bool(torch.equal(crc, crc2) and torch.equal(valid, valid2))
    settle(fn2)
    med2, _ = timed(fn2, reps)
    eng.set_option(N.UFC_OPT_VARLEN_KERNEL, saved)
    ab = {"other_kernel": "generic",
          "other_kernel_ms": round(med2, 4),
          "other_equal_results": same}
    if not CHECK:
        return rates("3: varlen 10M x U[64,1500] device-resident (unchecked counter pass)", total, algo, med, mean,
                     ceil_gbs, frames=n, **ab)
    h_data, h_off = data.cpu().numpy(), offsets.cpu().numpy().astype(np.uint64)
    ref_crc, ref_valid = oracle.validate_varlen_mt(h_data, h_off, min(64, threads()))
    exact = bool(np.array_equal(crc.cpu().numpy().view(np.uint32), ref_crc) and
                 np.array_equal(valid.cpu().numpy(), ref_valid))
    # CPU baseline: the oracle's bytewise loop (crc.rs:94-100) on the first frames, 1 thread and all
    k1, kn = 50_000, min(n, 50_000 * threads())

    def cpu(k, t):
        o = h_off[: k + 1]
        t0 = time.perf_counter()
        oracle.validate_varlen_mt(h_data, o, t)
        return (int(o[-1]) - int(o[0])) / (time.perf_counter() - t0) / 2**30

    cpu1, cpun = cpu(k1, 1), cpu(kn, threads())
    return rates("3: varlen 10M x U[64,1500] device-resident", total, algo, med, mean, ceil_gbs, frames=n, bytes=total,
                 bit_exact_all_frames=exact, valid_count_ok=int(ref_valid.sum()) == n - flipped.numel(), **ab,
                 cpu_baseline={"unit": "GiB/s", "single_thread": round(cpu1, 4), "all_threads": round(cpun, 3),
                               "threads": threads(), "nproc": os.cpu_count(),
                               "sample": f"first {k1} frames on 1 thread, first {kn} frames on {threads()} threads"})


def shard(eng, dev, reps, world=8, rank=3, total=100_000_000, L=1500):
    lo, hi = total * rank // world, total * (rank + 1) // world
    n = hi - lo
    frames = synth.fixed_frames(n, L, synth.SEED_CONFIG4, first_frame=lo, device=dev)
    eng.seal_fixed(frames, L, n=n)
    frames[torch.arange(0, n, 1000, device=dev) * L + 3] ^= 1
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    fn = lambda: eng.crc_fixed(frames, L, n=n, crc_out=crc, valid_out=valid)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    ok = int(valid.sum()) == n - len(range(0, n, 1000))
    settle(fn)
    med, mean = timed(fn, reps)
    out = rates(f"4 (one GPU's shard): frames [{lo}, {hi}) of 100M x 1500 B, device-resident", n * L, n * L + 5 * n,
                med, mean, ceiling(eng, frames, reps), frames=n, valid_ok=ok)
    del frames
    torch.cuda.empty_cache()
    return out


def seal(eng, dev, reps, n=1_000_000, L=1500):
    """The encode side on config 2's batch: ufc_seal_batch_fixed writes every frame's BE32 trailer
    in place (reads 1500 B, writes 4 B per frame); checked by validating afterwards."""
    frames = synth.fixed_frames(n, L, synth.SEED_CONFIG2, device=dev)
    fn = lambda: eng.seal_fixed(frames, L, n=n)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    crc, valid = eng.crc_fixed(frames, L, n=n)
    ok = int(valid.sum()) == n
    settle(fn)
    med, mean = timed(fn, reps)
    # the round-3 shape for comparison: two passes (CRC words, then a non-temporal trailer pass)
    from uflow_amd import _native as N
    eng.set_option(N.UFC_OPT_SEAL_KERNEL, N.UFC_SEAL_TWO_PASS)
    try:
        settle(fn)
        med_two, _ = timed(fn, reps)
    finally:
        eng.set_option(N.UFC_OPT_SEAL_KERNEL, N.UFC_SEAL_INLINE)
    return rates("2 (encode side): seal 1M x 1500-B frames in place, device-resident (one kernel: each "
                 "workgroup's trailers after its reads, non-temporal)", n * L, n * L + 4 * n,
                 med, mean, ceiling(eng, frames, reps), frames=n, valid_after_seal=ok,
                 two_pass_seal_ms=round(med_two, 4))


def seal_varlen(eng, dev, reps, n=10_000_000):
    """The encode side on config 3's batch: ufc_seal_batch_varlen writes every frame's BE32
    trailer in place (from the CRC kernel: a separate trailer pass measured 1.961 against
    1.860 ms here, 10M scattered writes); checked by validating every frame afterwards."""
    data, offsets = synth.varlen_batch(n, 64, 1500, synth.SEED_CONFIG3, device=dev)
    fn = lambda: eng.seal_varlen(data, offsets)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    _, valid = eng.crc_varlen(data, offsets)
    ok = int(valid.sum()) == n
    settle(fn)
    med, mean = timed(fn, reps)
    total = int(offsets[-1])
    return rates("3 (encode side): seal 10M x U[64,1500] frames in place, CSR, device-resident",
                 total, total + 8 * (n + 1) + 4 * n, med, mean, ceiling(eng, data, reps), frames=n,
                 valid_after_seal=ok)


def parse_batch(n, mtu):
    """The parse workloads' batch (host arrays): 600 distinct frames from the codec oracle, tiled (see parse)."""
    import random
    from oracle import codec as C
    rng = random.Random(5)

    def fit(fr):  # (data frames: drop datagrams from the end until the frame fits)
        while mtu and fr["kind"] == "data" and fr["datagrams"] and len(C.frame_write(fr)) > C.MAX_FRAME_SIZE:
            fr["datagrams"].pop()
        return C.frame_write(fr)
    base = [fit(C.random_data_frame(rng) if i % 3 == 0 else C.receive_side_data_frame(rng)
                if i % 3 == 1 else C.random_ack_frame(rng, 20)) for i in range(600)]
    assert not mtu or max(len(f) for f in base) <= C.MAX_FRAME_SIZE
    lens = np.array([len(base[i % 600]) for i in range(n)], dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lens)
    blob = np.frombuffer(b"".join(base), dtype=np.uint8)
    data = np.concatenate([blob] * (n // 600 + 1))[: int(offsets[-1])]
    return data, offsets, lens


def gate_tg(eng, dev, reps, n=1_000_000):
    """The variable-length gate alone on the parse workload's test-generator batch (38 % of frames over
    13 lines: the first launch's byte path defers them to frame_crc_long8_kernel), every frame against
    the oracle; the generic kernel timed beside it."""
    data, offsets, lens = parse_batch(n, False)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offsets).to(dev)
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    fn = lambda: eng.crc_varlen(d, o, crc_out=crc, valid_out=valid)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    settle(fn)
    med, mean = timed(fn, reps)
    total = int(offsets[-1])
    from uflow_amd import _native as N
    saved = eng.get_option(N.UFC_OPT_VARLEN_KERNEL)
    eng.set_option(N.UFC_OPT_VARLEN_KERNEL, N.UFC_VARLEN_GENERIC)
    crc2 = torch.empty(n, dtype=torch.int32, device=dev)
    valid2 = torch.empty(n, dtype=torch.uint8, device=dev)
    fn2 = lambda: eng.crc_varlen(d, o, crc_out=crc2, valid_out=valid2)  # noqa: E731
    fn2()
    torch.cuda.synchronize()
    same = bool(torch.equal(crc, crc2) and torch.equal(valid, valid2))
    settle(fn2, 300)
    med2, _ = timed(fn2, reps)
    eng.set_option(N.UFC_OPT_VARLEN_KERNEL, saved)
    extra = {}
    if CHECK:
        ref_crc, ref_valid = oracle.validate_varlen_mt(data, offsets.astype(np.uint64), min(64, threads()))
        extra["bit_exact_all_frames"] = bool(np.array_equal(crc.cpu().numpy().view(np.uint32), ref_crc) and
                                             np.array_equal(valid.cpu().numpy(), ref_valid))
    return rates("gate on the parse test-generator batch (1M uflow frames, 38 % over 1532 B)", total,
                 total + 8 * (n + 1) + 5 * n, med, mean, None, frames=n, over_13_lines=float(np.mean(lens > 1532)),
                 other_kernel="generic", other_kernel_ms=round(med2, 4), other_equal_results=same, **extra)


def parse(eng, dev, reps, n=1_000_000, mtu=False):
    """ufc_parse_batch_varlen over n real uflow frames (data frames with datagrams, acks, syncs):
    600 distinct frames from the codec oracle, tiled.  The generators are the reference's test
    generators (random_data_frame, serial/mod.rs:932-992), which ignore the frame size limit: 38 % of
    these frames are longer than MAX_FRAME_SIZE (1472 B, src/lib.rs:291-294), up to 7.5 KB, and take
    the gate's byte path.  mtu=True keeps only frames a uflow receiver can get (<= MAX_FRAME_SIZE: the
    emitters' limit, half_connection/emit.rs:69, and the receive buffer, server/mod.rs:595): each data
    frame keeps the longest prefix of its datagrams that fits, as the emitter packs a frame until the
    next datagram would not fit (emit.rs:69)."""
    data, offsets, lens = parse_batch(n, mtu)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offsets).to(dev)
    _, valid = eng.crc_varlen(d, o)
    infos, items, used = eng.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    cap = items.shape[0]
    fn = lambda: eng.parse_varlen(d, o, valid, items_cap=cap)  # noqa: E731
    settle(fn)
    med, mean = timed(fn, reps)
    total = int(offsets[-1])
    k = int(used.cpu()[0])
    # (a checksum of the item records and infos: equal across A/B variants)
    digest = int(items[:k].view(torch.int64).sum()) ^ int(infos.view(torch.int64).sum())
    # the gate and the parse back to back (Frame::read end to end: serial/mod.rs:675-706)
    crc = torch.empty(n, dtype=torch.int32, device=dev)

    def both():
        eng.crc_varlen(d, o, crc_out=crc, valid_out=valid)
        eng.parse_varlen(d, o, valid, items_cap=cap)
    settle(both, 300)
    med2, _ = timed(both, reps)
    # algorithmic bytes of the parse: the frame bytes read once, the offsets and
    # gate flags read, the 24-byte items and 32-byte infos written
    algo = total + 8 * (n + 1) + n + 24 * k + 32 * n
    return {"config": ("f3: device parse of 1M uflow frames <= MAX_FRAME_SIZE after the gate" if mtu else
                       "f3: device parse of 1M uflow frames after the gate (test generators, 38 % over MAX_FRAME_SIZE)"),
            "frames": n,
            "frame_bytes": total, "items": k, "items_digest": digest, "ms": round(med, 4), "mean_ms": round(mean, 4),
            "frames_per_s": round(n / med * 1e3), "GB_s_of_frame_bytes": round(total / med / 1e-3 / 1e9, 1),
            "algorithmic_bytes": algo, "frac_of_8TBs": round(algo / (med * 1e-3) / 8e12, 4),
            "gate_plus_parse_ms": round(med2, 4)}


def parse_mtu(eng, dev, reps):
    return parse(eng, dev, reps, mtu=True)


def build(eng, dev, reps, n=1_000_000):
    """The send-side mirror of parse_mtu: gate and parse the parse_mtu batch (1M frames <= MAX_FRAME_SIZE),
    then build it again from the records, datagram payloads gathered from the parsed batch's own bytes.
    Timed separately (events around groups of launches, after a settle): ufc_build_sizes_varlen,
    ufc_build_batch_varlen with seal = 0 (item sizes + scan + frame check + the write kernel),
    ufc_seal_batch_varlen over the built batch, and a device-to-device hipMemcpyAsync of the same byte
    count (the floor: it reads and writes each output byte once)."""
    import ctypes
    from uflow_amd import _native as N
    data, offsets, lens = parse_batch(n, True)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offsets).to(dev)
    _, valid = eng.crc_varlen(d, o)
    infos, items, used = eng.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    k = int(used.cpu()[0])
    out, off, status = eng.build_varlen(infos, items, d, src_base=o, n_items=k)
    torch.cuda.synchronize()
    total = int(off[-1])
    extra = {"all_ok": bool((status == 0).all())}
    if CHECK:  # every frame of this batch is canonical (written by the oracle): the build re-emits it
        extra["equals_source_batch"] = bool(total == d.numel() and torch.equal(out, d) and torch.equal(off, o))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, ctx = N.lib(), eng._ctx
    off2 = torch.empty_like(off)
    status2 = torch.empty_like(status)
    f_sizes = lambda: lib.ufc_build_sizes_varlen(ctx, p(infos), p(items), k, p(o), d.numel(), n, p(off2), p(status2), st)  # noqa: E731
    f_write = lambda: lib.ufc_build_batch_varlen(ctx, p(infos), p(items), k, p(o), p(d), d.numel(), n, p(off), p(out),  # noqa: E731
                                                 total, 0, None, st)
    f_seal = lambda: eng.seal_varlen(out, off)  # noqa: E731
    dst = torch.empty_like(out)
    f_copy = lambda: dst.copy_(out)  # noqa: E731
    res = {}
    for name, fn in (("sizes", f_sizes), ("write", f_write), ("seal", f_seal), ("copy", f_copy)):
        settle(fn, 500)
        res[name] = timed(fn, reps)
    payload_bytes = int(items[:k, 20:24].contiguous().view(torch.int32).sum())  # (every item here is a datagram or an ack group: data_len)
    algo = payload_bytes + total + 24 * k + 32 * n + 8 * (n + 1) + 8 * n
    w = res["write"][0]
    return {"config": "f4: device build of 1M uflow frames <= MAX_FRAME_SIZE from their parsed records",
            "frames": n, "items": k, "out_bytes": total, "payload_bytes": payload_bytes,
            "sizes_ms": round(res["sizes"][0], 4), "write_ms": round(w, 4), "write_mean_ms": round(res["write"][1], 4),
            "seal_ms": round(res["seal"][0], 4), "d2d_copy_ms": round(res["copy"][0], 4),
            "write_over_copy": round(w / res["copy"][0], 3), "algorithmic_bytes": algo,
            "write_algo_GB_s": round(algo / w / 1e-3 / 1e9, 1), "frac_of_8TBs": round(algo / (w * 1e-3) / 8e12, 4),
            "frames_per_s": round(n / w * 1e3), **extra}


def pack(eng, dev, reps, n=1_000_000):
    """The step before the build: the parse_mtu batch gated and parsed, its datagram records (ack groups left
    out) regrouped into flushes with no limit that bites, and packed into frames again (ufc_pack_varlen).
    Two groupings: many short flushes (10 datagrams each) and a few thousand long ones (4096 each).  Per
    grouping one JSON line: the pack's time per batch (events around groups of launches, after a settle),
    ufc_pack_host on the same records with 1 and 16 threads (wall clock, median of 5), every record of the
    GPU pack against the host's, and the existing build's write call (seal = 0) over the frames the pack
    gave, in the same process, for scale.  Run with --only pack."""
    import ctypes
    from uflow_amd import _native as N
    from uflow_amd.frame import FLUSH_DTYPE, FLUSH_RESULT_DTYPE, FRAME_INFO_DTYPE, ITEM_DTYPE, pack_host
    data, offsets, lens = parse_batch(n, True)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offsets).to(dev)
    _, valid = eng.crc_varlen(d, o)
    infos0, items0, used0 = eng.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    k0 = int(used0.cpu()[0])
    h_infos0 = records(infos0, FRAME_INFO_DTYPE)
    h_items = records(items0[:k0], ITEM_DTYPE)
    del infos0, items0
    # payload offsets relative to the whole batch (one source base, 0, for every new frame), then the datagrams alone
    frame_of = np.repeat(np.arange(n), h_infos0["item_count"])
    h_items["data_offset"] = (h_items["data_offset"] + offsets[frame_of]).astype(np.uint32)
    h_items = np.ascontiguousarray(h_items[h_items["form"] != 3])
    k = h_items.size
    d_items = rows(h_items, dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, ctx = N.lib(), eng._ctx
    out = []
    for name, per in (("short", 10), ("long", 4096)):
        first = np.minimum(np.arange(0, k + per, per), k).astype(np.uint64)
        nf = first.size - 1
        flushes = np.zeros(nf, dtype=FLUSH_DTYPE)
        flushes["kind"], flushes["flush_alloc"], flushes["window_room"] = 10, 1 << 50, 0xFFFFFFFF
        flushes["id0"] = np.arange(nf, dtype=np.uint32) * 7
        d_first = torch.from_numpy(first.astype(np.int64)).to(dev)
        d_flushes = rows(flushes, dev)
        infos = zrows(k, fr.FRAME_INFO_DTYPE, dev)
        res = zrows(nf, fr.FLUSH_RESULT_DTYPE, dev)
        used = torch.zeros(1, dtype=torch.int64, device=dev)
        f_pack = lambda: lib.ufc_pack_varlen(ctx, p(d_items), k, p(d_first), p(d_flushes), nf, None, p(infos), k,  # noqa: E731
                                             p(res), p(used), st)
        assert f_pack() == 0
        torch.cuda.synchronize()
        frames = int(used.cpu()[0])
        settle(f_pack, 500)
        med, mean = timed(f_pack, reps)
        host_ms = {}
        h_out = np.zeros(k, dtype=FRAME_INFO_DTYPE)
        for T in (1, 16):
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                h_infos, h_res, h_used = pack_host(h_items, first, flushes, nthreads=T, infos=h_out)
                ts.append(time.perf_counter() - t0)
            host_ms[T] = float(np.median(ts)) * 1e3
        extra = {}
        if CHECK:
            g_infos = records(infos[:frames], FRAME_INFO_DTYPE)
            g_res = records(res, FLUSH_RESULT_DTYPE)
            extra["equals_host_pack"] = bool(frames == h_used and np.array_equal(g_infos, h_infos[:frames]) and
                                             np.array_equal(g_res, h_res))
        # the build's write over these frames
        bi = infos[:frames]
        boff, bstatus = eng.build_sizes_varlen(bi, d_items, d.numel())
        torch.cuda.synchronize()
        total = int(boff[-1])
        bout = torch.empty(total, dtype=torch.uint8, device=dev)
        f_write = lambda: lib.ufc_build_batch_varlen(ctx, p(bi), p(d_items), k, None, p(d), d.numel(), frames, p(boff),  # noqa: E731
                                                     p(bout), total, 0, None, st)
        assert f_write() == 0
        settle(f_write, 500)
        w, _ = timed(f_write, reps)
        out.append({"config": f"f5: device pack of the parse_mtu batch's datagrams, {name} flushes ({per} items each)",
                    "items": k, "flushes": nf, "frames": frames, "pack_ms": round(med, 4), "pack_mean_ms": round(mean, 4),
                    "ns_per_item": round(med * 1e6 / k, 4), "host_pack_1t_ms": round(host_ms[1], 2),
                    "host_pack_16t_ms": round(host_ms[16], 2), "host_1t_over_gpu": round(host_ms[1] / med, 1),
                    "host_16t_over_gpu": round(host_ms[16] / med, 1), "build_write_ms": round(w, 4),
                    "build_all_ok": bool((bstatus == 0).all()), "out_bytes": total,
                    "pack_over_build_write": round(med / w, 3), **extra})
        del infos, res, bout, boff, bstatus
    return out


def emit(eng, dev, reps):
    """The step before the pack: synthetic send queues turned into datagram items (ufc_emit_packets_varlen).
    Two groupings of 8.4M packets of U[0, 3000] bytes, modes and 8 channels at random, half of the time-sensitive
    packets stale, no limit that bites: many short queues (2^20 senders of 8 packets) and a few long ones (2048
    senders of 4096 packets, the whole transfer window).  Per grouping one JSON line: the emit's time per batch
    (events around groups of calls, after a settle), ufc_emit_packets_host on the same records with 1 and 16
    threads (wall clock, median of 5), every output of the GPU emit against the host's, and ufc_pack_varlen over
    the items produced, in the same process, for scale.  Run with --only emit."""
    import ctypes
    from uflow_amd import _native as N
    from uflow_amd.frame import (FLUSH_DTYPE, ITEM_DTYPE, PACKET_DTYPE, PACKET_RESULT_DTYPE, SENDER_DTYPE,
                                 SENDER_RESULT_DTYPE)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, ctx = N.lib(), eng._ctx
    out = []
    for name, ns, per in (("short", 1 << 20, 8), ("long", 2048, 4096)):
        rng = np.random.default_rng(7)
        npk = ns * per
        packets = np.zeros(npk, dtype=PACKET_DTYPE)
        packets["data_len"] = rng.integers(0, 3001, npk)
        packets["data_offset"] = np.cumsum(packets["data_len"], dtype=np.uint64) % (1 << 31)
        packets["mode"] = rng.integers(0, 4, npk)
        packets["channel_id"] = rng.integers(0, 8, npk)
        packets["flush_id"] = np.where(packets["mode"] == 0, rng.integers(0, 2, npk), 1)
        first = np.arange(ns + 1, dtype=np.uint64) * per
        senders = np.zeros(ns, dtype=SENDER_DTYPE)
        senders["base_id"] = senders["next_id"] = rng.integers(0, 1 << 20, ns)
        senders["window_size"], senders["flush_id"], senders["max_alloc"] = 4096, 1, 1 << 40
        senders["window_parent_id"], senders["take"] = N.UFC_NO_PARENT, 0xFFFFFFFF
        senders["channel_parent_id"] = N.UFC_NO_PARENT
        # the host call: the item total, then timed with every output kept
        h_ff = np.zeros(ns + 1, dtype=np.uint64)
        h_pres = np.zeros(npk, dtype=PACKET_RESULT_DTYPE)
        h_sres = np.zeros(ns, dtype=SENDER_RESULT_DTYPE)
        h_sout = np.zeros(ns, dtype=SENDER_DTYPE)
        h_used = ctypes.c_uint64(0)
        h_call = lambda items, cap, T: lib.ufc_emit_packets_host(  # noqa: E731
            packets.ctypes.data, npk, first.ctypes.data, senders.ctypes.data, ns, items, cap, h_ff.ctypes.data,
            h_pres.ctypes.data, h_sres.ctypes.data, h_sout.ctypes.data, ctypes.byref(h_used), T)
        assert h_call(None, 0, 16) == 0
        k = int(h_used.value)
        h_items = np.zeros(k, dtype=ITEM_DTYPE)
        host_ms = {}
        for T in (1, 16):
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                assert h_call(h_items.ctypes.data, k, T) == 0
                ts.append(time.perf_counter() - t0)
            host_ms[T] = float(np.median(ts)) * 1e3
        d_packets = rows(packets, dev)
        d_first = torch.from_numpy(first.astype(np.int64)).to(dev)
        d_senders = rows(senders, dev)
        items = zrows(k, fr.ITEM_DTYPE, dev)
        ff = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
        pres = zrows(npk, fr.PACKET_RESULT_DTYPE, dev)
        sres = zrows(ns, fr.SENDER_RESULT_DTYPE, dev)
        sout = zrows(ns, fr.SENDER_DTYPE, dev)
        used = torch.zeros(1, dtype=torch.int64, device=dev)
        f_emit = lambda: lib.ufc_emit_packets_varlen(ctx, p(d_packets), npk, p(d_first), p(d_senders), ns, p(items), k,  # noqa: E731
                                                     p(ff), p(pres), p(sres), p(sout), p(used), st)
        assert f_emit() == 0
        torch.cuda.synchronize()
        assert int(used.cpu()[0]) == k
        settle(f_emit, 500)
        med, mean = timed(f_emit, reps)
        extra = {}
        if CHECK:
            same = lambda t, h: bool(np.array_equal(t.cpu().numpy().reshape(-1), h.view(np.uint8).reshape(-1)))  # noqa: E731
            extra["equals_host_emit"] = (same(items, h_items) and same(pres, h_pres) and same(sres, h_sres) and
                                         same(sout, h_sout) and bool(np.array_equal(ff.cpu().numpy(), h_ff.astype(np.int64))))
        # the pack over these items
        flushes = np.zeros(ns, dtype=FLUSH_DTYPE)
        flushes["kind"], flushes["flush_alloc"], flushes["window_room"] = 10, 1 << 50, 0xFFFFFFFF
        d_flushes = rows(flushes, dev)
        infos = zrows(k, fr.FRAME_INFO_DTYPE, dev)
        fres = zrows(ns, fr.FLUSH_RESULT_DTYPE, dev)
        fused = torch.zeros(1, dtype=torch.int64, device=dev)
        f_pack = lambda: lib.ufc_pack_varlen(ctx, p(items), k, p(ff), p(d_flushes), ns, None, p(infos), k, p(fres),  # noqa: E731
                                             p(fused), st)
        assert f_pack() == 0
        settle(f_pack, 500)
        w, _ = timed(f_pack, reps)
        algo = 16 * npk + 24 * k + 16 * npk + ns * (2 * 304 + 32 + 8 + 8)
        out.append({"config": f"f6: device packet emit, {name} queues ({ns} senders of {per} packets, U[0, 3000] B)",
                    "packets": npk, "senders": ns, "items": k, "packets_dropped": int(h_sres["packets_dropped"].sum()),
                    "frames": int(fused.cpu()[0]), "emit_ms": round(med, 4), "emit_mean_ms": round(mean, 4),
                    "ns_per_packet": round(med * 1e6 / npk, 4), "algorithmic_bytes": algo,
                    "algo_GB_s": round(algo / med / 1e-3 / 1e9, 1), "host_emit_1t_ms": round(host_ms[1], 2),
                    "host_emit_16t_ms": round(host_ms[16], 2), "host_1t_over_gpu": round(host_ms[1] / med, 1),
                    "host_16t_over_gpu": round(host_ms[16] / med, 1), "pack_ms": round(w, 4),
                    "emit_over_pack": round(med / w, 3), **extra})
        del d_packets, d_senders, items, ff, pres, sres, sout, infos, fres
        torch.cuda.empty_cache()
    return out


def receive(eng, dev, reps, n=1_000_000):
    """The step behind the parse: the parse_mtu batch gated and parsed, its data frames' datagrams given sequence
    ids a receiver takes (consecutive per receiver from a random base, one fragment each, no parents: every packet
    is delivered and the window moves past it) and run through ufc_receive_packets_varlen.  Two groupings: many
    small receivers (4 frames each, window 64) and 2048 receivers (window 4096).  Per grouping one JSON line: the
    receive's time per batch (events around groups of calls, after a settle; a step leaves the slots empty
    again, so every call does the same work), ufc_receive_packets_host on the same records with 1 thread (the baseline) and 16 (wall
    clock, median of 3); a plain device-to-device copy of the delivered bytes: the ceiling of the copy
    kernel; every output of the GPU call against the host's.  Run with --only receive."""
    import ctypes
    from uflow_amd import _native as N
    from uflow_amd.frame import (FRAME_INFO_DTYPE, ITEM_DTYPE, RECEIVER_RESULT_DTYPE, RX_PACKET_DTYPE, RX_SLOT_DTYPE,
                                 new_receivers)
    data, offsets, lens = parse_batch(n, True)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offsets).to(dev)
    _, valid = eng.crc_varlen(d, o)
    infos0, items0, used0 = eng.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    k = int(used0.cpu()[0])
    h_infos = records(infos0, FRAME_INFO_DTYPE)
    h_items0 = records(items0[:k], ITEM_DTYPE)
    h_valid = valid.cpu().numpy().copy()
    del infos0, items0
    counted = (h_infos["ok"] != 0) & (h_infos["kind"] == 10) & (h_valid != 0)
    cnt = np.where(counted, h_infos["item_count"], 0).astype(np.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, ctx = N.lib(), eng._ctx
    src_base = offsets[:n].astype(np.uint64)
    out = []
    for name, nr, W in (("small", n // 4, 64), ("2048", 2048, 4096)):
        rng = np.random.default_rng(9)
        ff = (np.arange(nr + 1, dtype=np.uint64) * n) // nr
        recv = new_receivers(nr, W, rng.integers(0, 1 << 20, nr))
        # sequence ids: consecutive over each receiver's handled datagrams
        items = h_items0.copy()
        cc = cnt[counted]
        fi = np.repeat(np.flatnonzero(counted), cc)                      # the frame of every handled datagram
        pos = np.arange(fi.size)
        idx = np.repeat(h_infos["item_first"][counted].astype(np.int64), cc) + pos - np.repeat(np.cumsum(cc) - cc, cc)
        owner = np.searchsorted(ff, fi, side="right") - 1                # its receiver (ascending)
        within = pos - np.searchsorted(owner, np.arange(nr), side="left")[owner]
        items["id"][idx] = (recv["base_id"][owner] + within) & 0xFFFFF
        items["window_parent_lead"] = items["channel_parent_lead"] = 0
        items["fragment_id"] = items["fragment_id_last"] = 0
        slot_first = np.arange(nr + 1, dtype=np.uint64) * W
        ns = nr * W
        pay = int(d.numel())
        caps = {"carry": 8 * ns + 64, "out": pay, "packets": k}
        # host, one thread
        h_slots = np.zeros(ns, dtype=RX_SLOT_DTYPE)
        h = {"carry_out": np.zeros(caps["carry"], np.uint8), "out": np.zeros(pay, np.uint8),
             "packets": np.zeros(k, dtype=RX_PACKET_DTYPE), "cf": np.zeros(nr + 1, np.uint64), "pf": np.zeros(nr + 1, np.uint64),
             "status": np.zeros(k, np.uint8), "res": np.zeros(nr, dtype=RECEIVER_RESULT_DTYPE), "rout": recv.copy()}
        hu = [ctypes.c_uint64(0) for _ in range(3)]
        c = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        h_call = lambda T: lib.ufc_receive_packets_host(  # noqa: E731
            c(h_infos), n, c(h_valid), c(items), k, c(src_base), c(data), pay, c(ff), c(recv), nr, c(h_slots), c(slot_first), ns,
            None, 0, c(h["carry_out"]), caps["carry"], c(h["cf"]), ctypes.addressof(hu[0]), c(h["packets"]), k, c(h["pf"]),
            ctypes.addressof(hu[1]), c(h["out"]), pay, ctypes.addressof(hu[2]), c(h["status"]), c(h["res"]), c(h["rout"]), T)
        host_ms = {}
        for T in (1, 16):
            ts = []
            for _ in range(3):
                h_slots[:] = 0
                t0 = time.perf_counter()
                assert h_call(T) == 0
                ts.append(time.perf_counter() - t0)
            host_ms[T] = float(np.median(ts)) * 1e3
        delivered, out_used = int(hu[1].value), int(hu[2].value)
        # device
        g = {"infos": rows(h_infos, dev), "accept": rows(h_valid, dev), "items": rows(items, dev), "src": rows(src_base.astype(np.int64), dev),
             "ff": rows(ff.astype(np.int64), dev), "recv": rows(recv, dev), "slots": zrows(ns, fr.RX_SLOT_DTYPE, dev),
             "sf": rows(slot_first.astype(np.int64), dev), "carry_out": torch.zeros(caps["carry"], dtype=torch.uint8, device=dev),
             "cf": torch.zeros(nr + 1, dtype=torch.int64, device=dev), "used": torch.zeros(3, dtype=torch.int64, device=dev),
             "packets": zrows(k, fr.RX_PACKET_DTYPE, dev),
             "pf": torch.zeros(nr + 1, dtype=torch.int64, device=dev), "out": torch.zeros(pay, dtype=torch.uint8, device=dev),
             "status": torch.zeros(k, dtype=torch.uint8, device=dev), "res": zrows(nr, fr.RECEIVER_RESULT_DTYPE, dev),
             "rout": zrows(nr, fr.RECEIVER_DTYPE, dev)}
        u = g["used"].data_ptr()
        f_rx = lambda: lib.ufc_receive_packets_varlen(  # noqa: E731
            ctx, p(g["infos"]), n, p(g["accept"]), p(g["items"]), k, p(g["src"]), p(d), pay, p(g["ff"]), p(g["recv"]), nr,
            p(g["slots"]), p(g["sf"]), ns, None, 0, p(g["carry_out"]), caps["carry"], p(g["cf"]), ctypes.c_void_p(u),
            p(g["packets"]), k, p(g["pf"]), ctypes.c_void_p(u + 8), p(g["out"]), pay, ctypes.c_void_p(u + 16),
            p(g["status"]), p(g["res"]), p(g["rout"]), st)
        assert f_rx() == 0
        torch.cuda.synchronize()
        extra = {}
        if CHECK:
            same = lambda a, b: bool(np.array_equal(a.cpu().numpy().reshape(-1), b.view(np.uint8).reshape(-1)))  # noqa: E731
            extra["equals_host_receive"] = (same(g["packets"], h["packets"]) and same(g["status"], h["status"]) and
                                            same(g["res"], h["res"]) and same(g["rout"], h["rout"]) and
                                            same(g["slots"], h_slots) and
                                            bool(np.array_equal(g["out"][:out_used].cpu().numpy(), h["out"][:out_used])) and
                                            g["used"].cpu().tolist() == [hu[0].value, hu[1].value, hu[2].value])
        settle(f_rx, 500)
        med, mean = timed(f_rx, reps)
        src_t, dst_t = d[:out_used], torch.empty(out_used, dtype=torch.uint8, device=dev)
        f_copy = lambda: dst_t.copy_(src_t)  # noqa: E731
        settle(f_copy, 300)
        cp, _ = timed(f_copy, reps)
        out.append({"config": f"f7: device packet receive of the parse_mtu batch's datagrams, {name} receivers "
                              f"({nr} receivers, window {W})",
                    "frames": n, "items": k, "receivers": nr, "slots": ns, "delivered": delivered, "bytes_delivered": out_used,
                    "status_counts": h["res"]["status_count"].sum(axis=0).tolist(), "receive_ms": round(med, 4),
                    "receive_mean_ms": round(mean, 4), "ns_per_item": round(med * 1e6 / max(k, 1), 4),
                    "host_receive_1t_ms": round(host_ms[1], 2), "host_receive_16t_ms": round(host_ms[16], 2),
                    "host_1t_over_gpu": round(host_ms[1] / med, 1), "host_16t_over_gpu": round(host_ms[16] / med, 1),
                    "d2d_copy_ms": round(cp, 4), "d2d_copy_GB_s": round(2 * out_used / cp / 1e-3 / 1e9, 1),
                    "receive_over_d2d_copy": round(med / cp, 2), **extra})
        del g, dst_t
        torch.cuda.empty_cache()
    return out


WINDOW_OUT = os.path.join(REPO, "profiles", "window_configs.jsonl")


def window(eng, dev, reps, n=1_000_000):
    """The step between the parse and the receive: the parse_mtu batch gated and parsed, its data frames given
    consecutive sequence ids per connection from a random base, about 0.5 % of them repeating the id before
    (duplicates) and 0.5 % skipping one (a frame lost), and run through ufc_frame_window_varlen.  Two groupings:
    250,000 connections of 4 frames and 2,048 connections of about 488 (window 4096 in both).  Per grouping one JSON
    line, also written to profiles/window_configs.jsonl: the call's time per batch (events around groups of calls,
    after a settle; the state is not written back, so every call does the same work), ufc_frame_window_host on the
    same records with 1 and 16 threads (wall clock, median of 3), a plain device read of the same 32 MB of
    records as the floor, and every output of the GPU call against the host's.  Run with --only window."""
    import ctypes
    from uflow_amd import _native as N
    from uflow_amd.frame import FRAME_INFO_DTYPE, FRAME_WINDOW_DTYPE, FRAME_WINDOW_RESULT_DTYPE, ITEM_DTYPE, new_frame_windows
    data, offsets, lens = parse_batch(n, True)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offsets).to(dev)
    _, valid = eng.crc_varlen(d, o)
    infos0, _, _ = eng.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    h_infos0 = records(infos0, FRAME_INFO_DTYPE)
    del infos0, d, o
    torch.cuda.empty_cache()
    is_data = (h_infos0["ok"] != 0) & (h_infos0["kind"] == 10)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    c = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, ctx = N.lib(), eng._ctx
    out = []
    for name, nw in (("250,000", 250_000), ("2,048", 2048)):
        rng = np.random.default_rng(10)
        ff = (np.arange(nw + 1, dtype=np.uint64) * n) // nw
        win = new_frame_windows(nw, 4096, rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32))
        infos = h_infos0.copy()
        di = np.flatnonzero(is_data)
        owner = np.searchsorted(ff, di, side="right") - 1
        u = rng.random(di.size)
        inc = np.where(u < 0.005, 0, np.where(u < 0.010, 2, 1)).astype(np.int64)
        first = np.searchsorted(owner, np.arange(nw), side="left")     # each connection's first data frame
        first = first[first < di.size]
        inc[first] = 1
        run = np.cumsum(inc)
        start = run[first] - 1                                           # the running sum in front of each connection
        seq = run - 1 - start[np.searchsorted(first, np.arange(di.size), side="right") - 1]
        infos["f"][di, 0] = (win["base_id"][owner].astype(np.int64) + seq) & 0xFFFFFFFF
        cap = nw + n
        h = {"accept": np.zeros(n, np.uint8), "groups": np.zeros(cap, dtype=ITEM_DTYPE), "gf": np.zeros(nw + 1, np.uint64),
             "res": np.zeros(nw, dtype=FRAME_WINDOW_RESULT_DTYPE), "wout": np.zeros(nw, dtype=FRAME_WINDOW_DTYPE)}
        hu = ctypes.c_uint64(0)
        h_call = lambda T: lib.ufc_frame_window_host(  # noqa: E731
            c(infos), n, c(ff), c(win), nw, c(h["accept"]), c(h["groups"]), cap, c(h["gf"]), ctypes.addressof(hu),
            c(h["res"]), c(h["wout"]), T)
        host_ms = {}
        for T in (1, 16):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                assert h_call(T) == 0
                ts.append(time.perf_counter() - t0)
            host_ms[T] = float(np.median(ts)) * 1e3
        g = {"infos": rows(infos, dev), "ff": rows(ff.astype(np.int64), dev), "win": rows(win, dev),
             "accept": torch.zeros(n, dtype=torch.uint8, device=dev), "groups": zrows(cap, fr.ITEM_DTYPE, dev),
             "gf": torch.zeros(nw + 1, dtype=torch.int64, device=dev), "used": torch.zeros(1, dtype=torch.int64, device=dev),
             "res": zrows(nw, fr.FRAME_WINDOW_RESULT_DTYPE, dev), "wout": zrows(nw, fr.FRAME_WINDOW_DTYPE, dev)}
        f_fw = lambda: lib.ufc_frame_window_varlen(  # noqa: E731
            ctx, p(g["infos"]), n, p(g["ff"]), p(g["win"]), nw, p(g["accept"]), p(g["groups"]), cap, p(g["gf"]), p(g["used"]),
            p(g["res"]), p(g["wout"]), st)
        assert f_fw() == 0
        torch.cuda.synchronize()
        extra = {}
        if CHECK:
            same = lambda a, b: bool(np.array_equal(a.cpu().numpy().reshape(-1), b.view(np.uint8).reshape(-1)))  # noqa: E731
            extra["equals_host"] = (same(g["accept"], h["accept"]) and same(g["groups"], h["groups"]) and
                                    same(g["res"], h["res"]) and same(g["wout"], h["wout"]) and
                                    bool(np.array_equal(g["gf"].cpu().numpy().astype(np.uint64), h["gf"])) and
                                    int(g["used"].cpu()[0]) == hu.value)
        settle(f_fw, 500)
        med, mean = timed(f_fw, reps)
        read_gbs = ceiling(eng, g["infos"].reshape(-1), reps)
        read_ms = 32 * n / read_gbs / 1e9 * 1e3
        res = h["res"]
        out.append({"config": f"f8: device frame window of the parse_mtu batch's frames, {name} connections (window 4096)",
                    "frames": n, "connections": nw, "data_frames": int(is_data.sum()), "accepted": int(res["accepted"].sum()),
                    "refused": int(res["refused"].sum()), "syncs": int(res["syncs"].sum()), "groups": int(hu.value),
                    "window_ms": round(med, 4), "window_mean_ms": round(mean, 4), "ns_per_frame": round(med * 1e6 / n, 4),
                    "host_1t_ms": round(host_ms[1], 2), "host_16t_ms": round(host_ms[16], 2),
                    "host_1t_over_gpu": round(host_ms[1] / med, 1), "host_16t_over_gpu": round(host_ms[16] / med, 1),
                    "infos_read_GBs": read_gbs, "infos_read_ms": round(read_ms, 4), "window_over_read": round(med / read_ms, 1),
                    **extra})
        del g
        torch.cuda.empty_cache()
    with open(WINDOW_OUT, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return out


QUEUE_OUT = os.path.join(REPO, "profiles", "queue_configs.jsonl")


def queue(eng, dev, reps, n=1_000_000):
    """The sender's step behind the parse: 1M synthesized ack frames over filled logs, run through
    ufc_frame_queue_varlen.  Two groupings: 250,000 connections of 4 frames (window 64, tail 64: each frame
    acknowledges 16 of the 64 logged frames) and 2,048 connections of about 488 (window 4096, tail 4096: each frame
    acknowledges 8 of the 4096).  Every frame carries one group; 2 % of its bits are clear (frames lost, nacked once
    three later ones are acked), its frame window base is the id behind its group, and every step asks for
    feedback.  The call marks the log in place, so the log and ref_acked are restored from a pristine copy before
    every call, outside the timed span: an event pair around each call on the device, wall clock around each call on
    the host (1 and 16 threads, median of 3).  Per grouping one JSON line, also written to
    profiles/queue_configs.jsonl, with every output of the GPU call against the host's.  Run with --only queue."""
    import ctypes
    from uflow_amd import _native as N
    from uflow_amd.frame import (FRAME_INFO_DTYPE, FRAME_QUEUE_DTYPE, FRAME_QUEUE_RESULT_DTYPE, FRAME_QUEUE_STEP_DTYPE,
                                 ITEM_DTYPE, SENT_FRAME_DTYPE, new_frame_queues)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    c = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, ctx = N.lib(), eng._ctx
    out = []
    for name, nq, W, S in (("250,000", 250_000, 64, 16), ("2,048", 2048, 4096, 8)):
        rng = np.random.default_rng(12)
        ff = (np.arange(nq + 1, dtype=np.uint64) * n) // nq
        base = rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
        queues, log = new_frame_queues(nq, W, W, base)
        cap = int(queues["log_cap"][0])
        queues["log_next_id"] = base + np.uint32(W)                      # the window is full: W frames logged
        nonce = rng.integers(0, 2, (nq, W), dtype=np.uint8)
        rel = np.arange(W, dtype=np.int64)
        slot = (queues["log_first"].astype(np.int64)[:, None] + ((base.astype(np.int64)[:, None] + rel) & (cap - 1))).reshape(-1)
        log["send_time_ms"][slot] = np.tile(10 * rel, nq)
        log["size"][slot] = 1000
        log["ref_first"][slot] = np.arange(nq * W)
        log["ref_count"][slot] = 1
        log["flags"][slot] = nonce.reshape(-1)
        own = (np.searchsorted(ff, np.arange(n), side="right") - 1).astype(np.int64)
        j = np.arange(n, dtype=np.int64) - ff[own].astype(np.int64)       # the frame's index in its connection
        bits = (rng.random((n, S)) >= 0.02)
        bits[:, 0] = True
        claimed = nonce[own[:, None], j[:, None] * S + np.arange(S)] & bits
        items = np.zeros(n, dtype=ITEM_DTYPE)
        items["form"] = 3
        items["id"] = (base[own].astype(np.int64) + j * S) & 0xFFFFFFFF
        items["data_offset"] = (bits * (1 << np.arange(S))).sum(axis=1)
        items["channel_id"] = claimed.sum(axis=1) & 1
        infos = np.zeros(n, dtype=FRAME_INFO_DTYPE)
        infos["kind"], infos["ok"], infos["crc_ok"], infos["item_count"], infos["item_first"] = 12, 1, 1, 1, np.arange(n)
        infos["f"][:, 0] = (base[own].astype(np.int64) + j * S + S) & 0xFFFFFFFF
        steps = np.zeros(nq, dtype=FRAME_QUEUE_STEP_DTYPE)
        steps["flags"], steps["rtt_ms"], steps["now_ms"] = N.UFC_FQ_HAS_RTT | N.UFC_FQ_FEEDBACK, 50, 10 * W + 100
        none = np.zeros(nq + 1, dtype=np.uint64)
        sent = np.zeros(0, dtype=SENT_FRAME_DTYPE)
        refs0 = np.zeros(nq * W, dtype=np.uint8)
        h = {"log": log.copy(), "refs": refs0.copy(), "res": np.zeros(nq, dtype=FRAME_QUEUE_RESULT_DTYPE),
             "qout": np.zeros(nq, dtype=FRAME_QUEUE_DTYPE)}
        h_call = lambda T: lib.ufc_frame_queue_host(  # noqa: E731
            c(infos), n, c(items), n, c(ff), c(sent), 0, c(none), c(queues), c(steps), nq, c(h["log"]), h["log"].size,
            c(h["refs"]), h["refs"].size, c(h["res"]), c(h["qout"]), T)
        host_ms = {}
        for T in (1, 16):
            ts = []
            for _ in range(3):
                np.copyto(h["log"], log)
                h["refs"][:] = 0
                t0 = time.perf_counter()
                assert h_call(T) == 0
                ts.append(time.perf_counter() - t0)
            host_ms[T] = float(np.median(ts)) * 1e3
        g = {"infos": rows(infos, dev), "items": rows(items, dev), "ff": rows(ff.astype(np.int64), dev), "none": rows(none.astype(np.int64), dev),
             "queues": rows(queues, dev), "steps": rows(steps, dev), "log0": rows(log, dev), "log": rows(log, dev),
             "refs": torch.zeros(nq * W, dtype=torch.uint8, device=dev),
             "res": zrows(nq, fr.FRAME_QUEUE_RESULT_DTYPE, dev), "qout": zrows(nq, fr.FRAME_QUEUE_DTYPE, dev)}

        def restore():
            g["log"].copy_(g["log0"])
            g["refs"].zero_()

        f_fq = lambda: lib.ufc_frame_queue_varlen(  # noqa: E731
            ctx, p(g["infos"]), n, p(g["items"]), n, p(g["ff"]), None, 0, p(g["none"]), p(g["queues"]), p(g["steps"]), nq,
            p(g["log"]), g["log"].shape[0], p(g["refs"]), g["refs"].numel(), p(g["res"]), p(g["qout"]), st)
        restore()
        assert f_fq() == 0
        torch.cuda.synchronize()
        extra = {}
        if CHECK:
            same = lambda a, b: bool(np.array_equal(a.cpu().numpy().reshape(-1), b.view(np.uint8).reshape(-1)))  # noqa: E731
            extra["equals_host"] = (same(g["res"], h["res"]) and same(g["qout"], h["qout"]) and same(g["log"], h["log"]) and
                                    same(g["refs"], h["refs"]))
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:                             # (out of idle clocks)
            restore()
            f_fq()
            torch.cuda.synchronize()
        s = torch.cuda.current_stream()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in evs:
            restore()
            e0.record(s)
            f_fq()
            e1.record(s)
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in evs]
        med, mean = float(np.median(ms)), float(np.mean(ms))
        res = h["res"]
        out.append({"config": f"f9: device frame queue of 1M synthesized ack frames, {name} connections (window {W}, tail {W})",
                    "frames": n, "connections": nq, "groups": int(res["groups"].sum()), "frames_acked": int(res["frames_acked"].sum()),
                    "li_acks": int(res["li_acks"].sum()), "li_nacks": int(res["li_nacks"].sum()),
                    "feedbacks": int(res["has_feedback"].sum()), "bad_state": int((res["stop"] != 0).sum()),
                    "queue_ms": round(med, 4), "queue_mean_ms": round(mean, 4), "ns_per_frame": round(med * 1e6 / n, 4),
                    "host_1t_ms": round(host_ms[1], 2), "host_16t_ms": round(host_ms[16], 2),
                    "host_1t_over_gpu": round(host_ms[1] / med, 1), "host_16t_over_gpu": round(host_ms[16] / med, 1),
                    "timing": "an event pair around each call, the log restored in front of it", **extra})
        del g
        torch.cuda.empty_cache()
    with open(QUEUE_OUT, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return out


RATE_OUT = os.path.join(REPO, "profiles", "rate_configs.jsonl")


def rate(eng, dev, reps, n=None):
    """The step that closes a sender's tick: ufc_rate_step_varlen for 250,000 and for 2,048 connections (the frame
    queue's groupings).  5 % of the connections await their first send, 25 % are in slow start (half of them before
    their first feedback), 70 % in the throughput equation; 90 % have feedback this tick (30 % of it rate limited;
    in the throughput equation half of it with a higher loss rate, in slow start 5 % with a first loss and so a
    bisection), a few timers have expired; the sets hold 1 to 4 entries in rooms of 8; both
    flush gathers are used.  The call updates the entries in place, so they are restored from a pristine copy before
    every call, outside the timed span: an event pair around each call on the device, wall clock around each call on
    the host (1 and 16 threads, median of 3).  The floor is one device-to-device copy of (bytes read + bytes written)
    / 2 bytes, which reads and writes as much as the call does: per connection the state in and out, the tick, the
    frame queue result, the rate result, two indices, a flush result and a flush_alloc, and the entries read (every
    entry of a connection that looks at its set) and written (one per feedback).  Per grouping one JSON line, also
    written to profiles/rate_configs.jsonl, with every output of the GPU call against the host's."""
    import ctypes
    from uflow_amd import _native as N
    from uflow_amd.frame import (FLUSH_DTYPE, FLUSH_RESULT_DTYPE, FRAME_QUEUE_RESULT_DTYPE, RATE_RESULT_DTYPE,
                                 RATE_STATE_DTYPE, RATE_TICK_DTYPE, new_rate_states)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    c = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, ctx = N.lib(), eng._ctx
    out = []
    for name, nq in (("250,000", 250_000), ("2,048", 2048)):
        rng = np.random.default_rng(13)
        cap, now = 8, 100_000
        states, entries = new_rate_states(nq, 0xFFFFFFFF, cap)
        u = rng.random(nq)
        mode = np.where(u < 0.05, 0, np.where(u < 0.30, 1, 2)).astype(np.uint32)
        fresh = (mode == 1) & (rng.random(nq) < 0.5)                     # slow start before the first feedback
        live = (mode != 0) & ~fresh
        states["mode"] = mode
        states["send_rate"] = np.where(mode == 0, 1472, (10.0 ** rng.uniform(3, 7, nq))).astype(np.uint32)
        states["send_rate_tcp"] = np.where(mode == 2, states["send_rate"], 0)
        states["has_time_last_doubled"] = live & (mode == 1)
        states["time_last_doubled_ms"] = np.where(live & (mode == 1), now - rng.integers(0, 300, nq), 0)
        states["has_nofeedback_exp"] = mode != 0
        states["nofeedback_exp_ms"] = np.where(mode != 0, now + rng.integers(-100, 2000, nq), 0)
        states["nofeedback_idle"] = live & (rng.random(nq) < 0.5)
        rtt = rng.uniform(0.01, 0.3, nq)
        for k in ("has_rtt_s", "has_rtt_ms", "has_rto_ms"):
            states[k] = live
        states["rtt_s"] = np.where(live, rtt, 0.0)
        states["rtt_ms"] = np.where(live, np.round(rtt * 1000), 0).astype(np.uint64)
        states["rto_ms"] = np.where(live, np.round(rtt * 4000), 0).astype(np.uint64)
        states["prev_loss_rate"] = np.where(live, rng.uniform(0, 0.05, nq), 0.0)
        states["now_ms"], states["has_last_flush"] = now, 1
        states["flush_alloc"] = rng.integers(-1500, 20000, nq)
        count = np.where(mode == 0, 0, np.where(fresh, 1, rng.integers(1, 5, nq))).astype(np.uint32)
        states["recv_count"] = count
        entries["timestamp_ms"] = now - rng.integers(0, 300, nq * cap)
        entries["value"] = (10.0 ** rng.uniform(3, 7, nq * cap)).astype(np.uint32)
        first = np.arange(nq) * cap
        entries["value"][first[fresh]], entries["is_initial"][first[fresh]] = 0xFFFFFFFF, 1
        ticks = np.zeros(nq, dtype=RATE_TICK_DTYPE)
        ticks["now_ms"], ticks["delta_time_s"] = now + 20, 0.02
        ticks["alloc_adjust"] = -rng.integers(0, 64, nq)
        fq = np.zeros(nq, dtype=FRAME_QUEUE_RESULT_DTYPE)
        fb = rng.random(nq) < 0.9
        fq["has_feedback"] = fb
        fq["rtt_ms"] = np.where(fb, rng.integers(10, 300, nq), 0)
        fq["receive_rate"] = np.where(fb, (10.0 ** rng.uniform(3, 7, nq)), 0).astype(np.uint32)
        fq["loss_rate"] = np.where(fb & ((mode == 2) | (rng.random(nq) < 0.05)), rng.uniform(0, 0.05, nq), 0.0)
        fq["rate_limited"] = fb & (rng.random(nq) < 0.3)
        fres = np.zeros(nq, dtype=FLUSH_RESULT_DTYPE)
        fres["frame_count"] = rng.integers(0, 3, nq)
        fres["alloc_left"] = rng.integers(-1500, 20000, nq)
        ri = rng.permutation(nq).astype(np.uint32)
        flushes = np.zeros(nq, dtype=FLUSH_DTYPE)
        fi = np.arange(nq, dtype=np.uint32)
        h = {"entries": entries.copy(), "res": np.zeros(nq, dtype=RATE_RESULT_DTYPE), "out": np.zeros(nq, dtype=RATE_STATE_DTYPE),
             "flushes": flushes.copy()}
        h_call = lambda T: lib.ufc_rate_step_host(  # noqa: E731
            c(states), c(ticks), c(fq), nq, c(h["entries"]), h["entries"].size, c(fres), nq, c(ri), c(h["flushes"]), nq, c(fi),
            c(h["res"]), c(h["out"]), T)
        host_ms = {}
        for T in (1, 16):
            ts = []
            for _ in range(3):
                np.copyto(h["entries"], entries)
                t0 = time.perf_counter()
                assert h_call(T) == 0
                ts.append(time.perf_counter() - t0)
            host_ms[T] = float(np.median(ts)) * 1e3
        res = h["res"]
        fed = (res["flags"] & N.UFC_RATE_FEEDBACK) != 0
        looked = fed | ((res["flags"] & N.UFC_RATE_NOFEEDBACK) != 0) & (mode == 2)
        read = nq * (112 + 32 + 80 + 4 + 24 + 4) + 16 * int(count[looked].sum())
        written = nq * (112 + 56 + 8) + 16 * int(fed.sum())
        g = {"states": rows(states, dev), "ticks": rows(ticks, dev), "fq": rows(fq, dev), "entries0": rows(entries, dev),
             "entries": rows(entries, dev), "fres": rows(fres, dev), "ri": rows(ri, dev), "flushes": rows(flushes, dev), "fi": rows(fi, dev),
             "res": zrows(nq, fr.RATE_RESULT_DTYPE, dev), "out": zrows(nq, fr.RATE_STATE_DTYPE, dev),
             "src": torch.zeros((read + written) // 2, dtype=torch.uint8, device=dev),
             "dst": torch.zeros((read + written) // 2, dtype=torch.uint8, device=dev)}
        restore = lambda: g["entries"].copy_(g["entries0"])  # noqa: E731
        f_rate = lambda: lib.ufc_rate_step_varlen(  # noqa: E731
            ctx, p(g["states"]), p(g["ticks"]), p(g["fq"]), nq, p(g["entries"]), g["entries"].shape[0], p(g["fres"]), nq,
            p(g["ri"]), p(g["flushes"]), nq, p(g["fi"]), p(g["res"]), p(g["out"]), st)
        restore()
        assert f_rate() == 0
        torch.cuda.synchronize()
        extra = {}
        if CHECK:
            same = lambda a, b: bool(np.array_equal(a.cpu().numpy().reshape(-1), b.view(np.uint8).reshape(-1)))  # noqa: E731
            extra["equals_host"] = (same(g["res"], h["res"]) and same(g["out"], h["out"]) and same(g["entries"], h["entries"])
                                    and same(g["flushes"], h["flushes"]))
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:                             # (out of idle clocks)
            restore()
            f_rate()
            g["dst"].copy_(g["src"])
            torch.cuda.synchronize()
        s = torch.cuda.current_stream()
        timed = {}
        for what, f in (("rate", f_rate), ("copy", lambda: g["dst"].copy_(g["src"]))):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for e0, e1 in evs:
                restore()
                e0.record(s)
                f()
                e1.record(s)
            torch.cuda.synchronize()
            timed[what] = [a.elapsed_time(b) for a, b in evs]
        med, mean, copy = float(np.median(timed["rate"])), float(np.mean(timed["rate"])), float(np.median(timed["copy"]))
        out.append({"config": f"f10: device send rate step of one tick, {name} connections (rooms of {cap} entries)",
                    "connections": nq, "feedbacks": int(fed.sum()),
                    "nofeedback": int(((res["flags"] & N.UFC_RATE_NOFEEDBACK) != 0).sum()),
                    "resets": int(((res["flags"] & N.UFC_RATE_RESET_ISSUED) != 0).sum()),
                    "inv_iterations": int(res["inv_iterations"].sum()), "stopped": int((res["stop"] != 0).sum()),
                    "bytes_read": read, "bytes_written": written,
                    "rate_ms": round(med, 4), "rate_mean_ms": round(mean, 4), "ns_per_connection": round(med * 1e6 / nq, 3),
                    "copy_ms": round(copy, 4), "rate_over_copy": round(med / copy, 2),
                    "host_1t_ms": round(host_ms[1], 3), "host_16t_ms": round(host_ms[16], 3),
                    "host_1t_over_gpu": round(host_ms[1] / med, 1), "host_16t_over_gpu": round(host_ms[16] / med, 1),
                    "timing": "an event pair around each call, the entries restored in front of it", **extra})
        del g
        torch.cuda.empty_cache()
    with open(RATE_OUT, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return out


RESEND_OUT = os.path.join(REPO, "profiles", "resend_configs.jsonl")
RESEND_GROUPINGS = (("250,000", 250_000), ("2,048", 2048))


def resend(eng, dev, reps):
    """The three resend calls of one tick, ufc_resend_begin_varlen, ufc_resend_place_varlen and
    ufc_resend_commit_varlen, for 250,000 and for 2,048 connections.  The state is what earlier ticks leave: every
    connection has 8 one-fragment Persistent packets of 200 bytes in a window of 16, their 8 entries in its heap (a
    quarter due, a quarter of the fragments acknowledged, independently), 16 live refs in its transmission ring with a
    quarter of their ref_acked marks set, one ack frame that frees two packets, and two new Reliable packets of 300
    bytes in its queue.  Between the calls the emit, the pack and the size pass run on the host once, untimed; the
    device calls take their outputs.  begin changes the heap, the ack bytes and ref_acked and commit the heap, so
    those are restored from pristine copies in front of every call, outside the timed span: an event pair around each
    call on the device, wall clock around each call on the host (1 and 16 threads, median of 3).  The floor is one
    device-to-device copy of (bytes read + bytes written) / 2 of the three calls together, counted from the records:
    per connection the state, sender, queue, flush, rate and result records in and out, its heap entries twice, its
    live refs and marks, its touched table slots and ack bytes, and its items, refs and sent records.  Per grouping
    one JSON line, also written to profiles/resend_configs.jsonl, with every output of the device calls against the
    host calls'."""
    import ctypes
    from uflow_amd import _native as N, frame as fr
    lib = N.lib()
    out = []
    W, K, LIVE, NEW = 16, 8, 16, 2
    for name, nq in RESEND_GROUPINGS:
        rng = np.random.default_rng(29)
        now, rtt = 100_000, 40
        states, A = fr.new_resend_states(nq, W, W * 1448, 2, 1, heap_cap=16, stage_cap=16)
        base = rng.integers(0, 1 << 20, nq).astype(np.uint32)
        senders = np.zeros(nq, dtype=fr.SENDER_DTYPE)
        senders["base_id"], senders["next_id"], senders["window_size"] = base, (base + K) & 0xFFFFF, W
        senders["alloc"], senders["max_alloc"], senders["window_parent_id"] = K * 200, W * 1448, fr.NO_PARENT
        senders["channel_parent_id"], senders["take"] = fr.NO_PARENT, 0xFFFFFFFF
        k = np.arange(K, dtype=np.uint32)
        seq = (base[:, None] + k[None, :]) & 0xFFFFF
        slot = (states["pkt_first"][:, None] + (seq & (W - 1))).astype(np.int64)
        pk = A["pkts"]
        pk["data_offset"][slot], pk["data_len"][slot], pk["frag_first"][slot] = seq * 200 % (1 << 31), 200, k[None, :]
        pk["sequence_id"][slot], pk["resend"][slot] = seq, 1
        A["frag_acked"][(states["frag_first"][:, None] + k[None, :]).astype(np.int64)] = rng.random((nq, K)) < 0.25
        states["frag_next"], states["heap_len"], states["window_bytes"] = K, K, K * 200
        times = np.sort(np.where(rng.random((nq, K)) < 0.25, now - rng.integers(0, 30, (nq, K)), now + rng.integers(1, 150, (nq, K))), axis=1)
        order = np.argsort(rng.random((nq, K)), axis=1).astype(np.uint32)   # which packet holds which heap slot
        hs = (states["heap_first"][:, None] + k[None, :]).astype(np.int64)
        A["heap"]["resend_time_ms"][hs], A["heap"]["send_count"][hs] = times, 1
        A["heap"]["sequence_id"][hs] = (base[:, None] + order) & 0xFFFFF
        j = np.arange(LIVE, dtype=np.uint32)
        ts = (states["tx_first"][:, None] + j[None, :]).astype(np.int64)
        A["tx"]["sequence_id"][ts], A["tx"]["flags"][ts] = (base[:, None] + j[None, :] % K) & 0xFFFFF, fr.TX_RESEND
        A["ref_acked"][ts] = rng.random((nq, LIVE)) < 0.25
        states["tx_head"] = LIVE
        queues, log = fr.new_frame_queues(nq, 2, 1)
        queues["log_next_id"] = 1
        log["ref_first"][queues["log_first"].astype(np.int64)] = states["tx_first"]
        infos = np.zeros(nq, dtype=fr.FRAME_INFO_DTYPE)
        infos["kind"], infos["ok"] = fr.ACK, 1
        infos["f"][:, 1] = (base + 2) & 0xFFFFF
        frame_first = np.arange(nq + 1, dtype=np.uint64)
        rate_r = np.zeros(nq, dtype=fr.RATE_RESULT_DTYPE)
        rate_r["now_ms"], rate_r["rtt_ms"] = now, rtt
        flushes = np.zeros(nq, dtype=fr.FLUSH_DTYPE)
        flushes["flush_alloc"], flushes["kind"], flushes["window_room"], flushes["id0"] = 1 << 30, fr.DATA, 2, 1
        packets = np.zeros(nq * NEW, dtype=fr.PACKET_DTYPE)
        packets["data_offset"], packets["data_len"], packets["mode"] = np.arange(nq * NEW) * 300 % (1 << 31), 300, fr.SEND_RELIABLE
        packet_first = np.arange(nq + 1, dtype=np.uint64) * NEW
        pristine = {n_: A[n_].copy() for n_ in ("heap", "frag_acked", "ref_acked")}

        def restore_host():
            for n_, v in pristine.items():
                np.copyto(A[n_], v)

        host_ms = {}
        for T in (1, 16):
            ts_ = {"begin": [], "place": [], "commit": []}
            for _ in range(3):
                restore_host()
                t0 = time.perf_counter()
                b = fr.resend_begin_host(infos, frame_first, queues, log, rate_r, flushes, states, senders, A, nthreads=T)
                ts_["begin"].append(time.perf_counter() - t0)
                items, flush_first, pres, sres, _, used = fr.emit_packets_host(packets, packet_first, b["senders_out"], nthreads=16)
                t0 = time.perf_counter()
                fr.resend_place_host(b["states_out"], b["results"], A, flush_first, items, nthreads=T)
                ts_["place"].append(time.perf_counter() - t0)
                frames, fres, frames_used = fr.pack_host(items, flush_first, flushes, nthreads=16)
                frames = frames[:frames_used]
                offs = np.zeros(frames_used + 1, dtype=np.uint64)
                assert lib.ufc_build_sizes_host(frames.ctypes.data, items.ctypes.data, items.size, None, 1 << 40, frames_used,
                                                offs.ctypes.data, None, 16) == 0
                heap_mid = A["heap"].copy()
                t0 = time.perf_counter()
                cm = fr.resend_commit_host(fres, frames, offs, frames_used, items, flush_first, packets, packet_first, pres, sres,
                                           b["results"], rate_r, b["states_out"], b["senders_out"], A, nthreads=T)
                ts_["commit"].append(time.perf_counter() - t0)
            host_ms[T] = {k_: float(np.median(v)) * 1e3 for k_, v in ts_.items()}
        br, cr = b["results"], cm["results"]
        n_items = int(used)
        read = nq * (104 + 304 + 192 + 24 + 56 + 32 + 8) + LIVE * nq * 9 + K * nq * (16 + 24 + 1) + \
            n_items * 24 * 3 + nq * (104 + 304 + 48 + 24 + 32 + 56) + nq * NEW * 32 + frames_used * 40 + K * nq * 16
        written = nq * (104 + 304 + 48) + LIVE * nq + K * nq * 16 * 2 + n_items * 24 * 2 + nq * (104 + 304 + 40 + 8) + \
            nq * NEW * 25 + n_items * 8 + frames_used * 24
        host_final = {n_: A[n_].copy() for n_ in pristine}   # (what the host calls left, before the state goes up pristine)
        restore_host()
        g = {"heap": rows(A["heap"], dev), "pkts": rows(A["pkts"], dev), "frag_acked": rows(A["frag_acked"], dev), "tx": rows(A["tx"], dev),
             "ref_acked": rows(A["ref_acked"], dev), "stage": rows(A["stage"], dev)}
        g0 = {n_: g[n_].clone() for n_ in ("heap", "frag_acked", "ref_acked")}
        d = {"infos": rows(infos, dev), "ff": rows(frame_first, dev), "queues": rows(queues, dev), "log": rows(log, dev), "rate": rows(rate_r, dev),
             "flushes": rows(flushes, dev), "states": rows(states, dev), "senders": rows(senders, dev), "packets": rows(packets, dev),
             "pf": rows(packet_first, dev), "pres": rows(pres, dev), "sres": rows(sres, dev), "fres": rows(fres, dev), "frames": rows(frames, dev),
             "offs": rows(offs, dev), "used": torch.tensor([frames_used], dtype=torch.int64, device=dev), "flush_first": rows(flush_first, dev)}
        restore = lambda: [g[n_].copy_(v) for n_, v in g0.items()]  # noqa: E731
        rb = eng.resend_begin(d["infos"], d["ff"], d["queues"], d["log"], d["rate"], d["flushes"], d["states"], d["senders"], g)
        items_d = rows(E_fill(items, flush_first, br), dev)   # (the reserved slots empty, as the emit leaves them)
        f_begin = lambda: eng.resend_begin(d["infos"], d["ff"], d["queues"], d["log"], d["rate"], d["flushes"], d["states"],  # noqa: E731
                                           d["senders"], g, results=rb["results"], states_out=rb["states_out"],
                                           senders_out=rb["senders_out"])
        f_place = lambda: eng.resend_place(rb["states_out"], rb["results"], g, d["flush_first"], items_d)  # noqa: E731
        torch.cuda.synchronize()
        heap_mid_d = g["heap"].clone()
        rc = eng.resend_commit(d["fres"], d["frames"], d["offs"], d["used"], rows(items, dev), d["flush_first"], d["packets"], d["pf"],
                               d["pres"], d["sres"], rb["results"], d["rate"], rb["states_out"], rb["senders_out"], g)
        items_full = rows(items, dev)
        f_commit = lambda: eng.resend_commit(d["fres"], d["frames"], d["offs"], d["used"], items_full, d["flush_first"],  # noqa: E731
                                             d["packets"], d["pf"], d["pres"], d["sres"], rb["results"], d["rate"],
                                             rb["states_out"], rb["senders_out"], g, sent=rc["sent"], results=rc["results"],
                                             states_out=rc["states_out"], retake=rc["retake"])
        f_place()
        torch.cuda.synchronize()
        extra = {}
        if CHECK:
            same = lambda a, b_: bool(np.array_equal(a.cpu().numpy().reshape(-1), np.ascontiguousarray(b_).view(np.uint8).reshape(-1)))  # noqa: E731
            pairs = (("begin results", rb["results"], br), ("begin states", rb["states_out"], b["states_out"]),
                     ("begin senders", rb["senders_out"], b["senders_out"]), ("placed items", items_d, items),
                     ("commit results", rc["results"], cr), ("commit states", rc["states_out"], cm["states_out"]),
                     ("retake", rc["retake"], cm["retake"]), ("sent", rc["sent"], cm["sent"]), ("heap", g["heap"], host_final["heap"]),
                     ("packet table", g["pkts"], A["pkts"]), ("ack bytes", g["frag_acked"], host_final["frag_acked"]),
                     ("tx ring", g["tx"], A["tx"]), ("ref_acked", g["ref_acked"], host_final["ref_acked"]),
                     ("heap after begin", heap_mid_d, heap_mid))
            differs = [n_ for n_, x, y in pairs if not same(x, y)]
            extra["equals_host"] = not differs
            if differs:
                extra["differs"] = differs
        src = torch.zeros((read + written) // 2, dtype=torch.uint8, device=dev)
        dst = torch.zeros_like(src)
        restore_commit = lambda: g["heap"].copy_(heap_mid_d)  # noqa: E731
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:                             # (out of idle clocks)
            restore()
            f_begin()
            f_place()
            f_commit()
            dst.copy_(src)
            torch.cuda.synchronize()
        s = torch.cuda.current_stream()
        timed = {}
        for what, f, pre in (("begin", f_begin, restore), ("place", f_place, lambda: None), ("commit", f_commit, restore_commit),
                             ("copy", lambda: dst.copy_(src), lambda: None)):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for e0, e1 in evs:
                pre()
                e0.record(s)
                f()
                e1.record(s)
            torch.cuda.synchronize()
            timed[what] = float(np.median([a.elapsed_time(b_) for a, b_ in evs]))
        total = timed["begin"] + timed["place"] + timed["commit"]
        out.append({"config": f"f11: device resend calls of one tick, {name} connections (8 heap entries each, a quarter due, "
                              "a quarter acknowledged, a quarter of 16 live refs marked, one ack frame freeing 2 packets)",
                    "connections": nq, "resent": int(br["n_resent"].sum()), "popped_dead": int(br["heap_popped_dead"].sum()),
                    "popped_acked": int(br["heap_popped_acked"].sum()), "refs_acked": int(br["refs_acked"].sum()),
                    "packets_freed": int(br["packets_freed"].sum()), "heap_pushed": int(cr["heap_pushed"].sum()),
                    "items": n_items, "frames": int(frames_used), "stopped": int((br["stop"] != 0).sum() + (cr["stop"] != 0).sum()),
                    "bytes_read": int(read), "bytes_written": int(written),
                    "begin_ms": round(timed["begin"], 4), "place_ms": round(timed["place"], 4), "commit_ms": round(timed["commit"], 4),
                    "three_calls_ms": round(total, 4), "ns_per_connection": round(total * 1e6 / nq, 3),
                    "copy_ms": round(timed["copy"], 4), "calls_over_copy": round(total / timed["copy"], 2),
                    "host_1t_ms": {k_: round(v, 3) for k_, v in host_ms[1].items()},
                    "host_16t_ms": {k_: round(v, 3) for k_, v in host_ms[16].items()},
                    "timing": "an event pair around each call, the heap, ack bytes and marks restored in front of it", **extra})
        del g, g0, d, src, dst
        torch.cuda.empty_cache()
    with open(RESEND_OUT, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return out


def E_fill(items, flush_first, begin_results):
    """The emit's items with the reserved slots zeroed: what the device place call starts from."""
    a = items.copy()
    for c in np.nonzero(begin_results["n_resent"] + begin_results["n_pending_staged"])[0]:
        f0 = int(flush_first[c])
        a[f0: f0 + int(begin_results["n_resent"][c]) + int(begin_results["n_pending_staged"][c])] = 0
    return a


def host(eng, reps=5, n=1_000_000, L=1472):
    res = []
    for kind in ("pinned", "pageable"):
        t = torch.empty(n * L, dtype=torch.uint8, pin_memory=(kind == "pinned"))
        d = synth.fixed_frames(n, L, synth.SEED_CONFIG2, device="cuda")
        eng.seal_fixed(d, L, n=n)
        torch.cuda.synchronize()
        t.copy_(d.cpu())
        del d
        a = t.numpy()
        a[np.arange(0, n, 500) * L + 9] ^= 0x40
        offsets = (np.arange(n + 1, dtype=np.uint64) * L)
        lens = np.full(n, L, dtype=np.uint32)
        for entry, fn in (("ufc_validate_host_varlen (CSR)", lambda: eng.validate_host_varlen(a, offsets)),
                          ("ufc_validate_host_slots (recvmmsg slots, stride 1472)",
                           lambda: eng.validate_host_slots(a, L, lens))):
            fn()  # warm (staging allocation)
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                crc, valid = fn()
                times.append(time.perf_counter() - t0)
            sec = float(np.median(times))
            ok = int(valid.sum()) == n - len(range(0, n, 500))
            res.append({"config": f"5 (GPU leg): host-resident {n} x {L}-B frames, {kind} buffer, H2D + CRC + D2H",
                        "entry": entry, "frames": n, "seconds": round(sec, 5), "GiB_s": round(n * L / sec / 2**30, 2),
                        "frames_per_s": round(n / sec), "valid_ok": ok})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--varlen-kernel", default="auto", choices=["auto", "sorted8"],
                    help="variable-length kernel of the timed runs (the other one is timed beside it)")
    ap.add_argument("--only", default="varlen,shard,seal,seal_varlen,parse,parse_mtu,host")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-check", action="store_true",
                    help="skip the oracle checks and CPU baselines (counter passes of tools/profile_workloads.sh)")
    a = ap.parse_args()
    global CHECK
    CHECK = not a.no_check
    dev = torch.device("cuda", 0)
    eng = FrameCrcEngine(0)
    from uflow_amd import _native as N
    eng.set_option(N.UFC_OPT_VARLEN_KERNEL, {"auto": N.UFC_VARLEN_AUTO, "sorted8": N.UFC_VARLEN_SORTED8}[a.varlen_kernel])
    for what in a.only.split(","):
        if what == "host":
            for r in host(eng):
                print(json.dumps(r), flush=True)
        elif what in ("pack", "emit", "receive", "window", "queue", "rate", "resend"):
            for r in globals()[what](eng, dev, a.reps):
                print(json.dumps(r), flush=True)
        else:
            print(json.dumps(globals()[what](eng, dev, a.reps)), flush=True)
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
