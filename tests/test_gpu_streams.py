"""Scratch the library keeps per stream, under the call patterns of a receive loop: work on two
non-default streams at once, batches of different sizes back to back with no synchronise in between,
release_stream followed by reuse, and the lean fixed kernel's ring of claim counters.  Every result
is compared bit-exactly with the oracle's (gate_expect's cases).

The variable-length gate and seal defer frames past 13 lines to a second launch through a per-stream
list of frame indices, which grows with the batch, and per-workgroup counts, which are zeroed when
allocated and by the second launch only (ufc_api.cpp launch_varlen8).
"""
import numpy as np
import pytest
import torch

import gate_expect as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _upload(case):
    dbuf = G.to_device(case.buf, DEV)
    doff = G.to_device(case.off.view(np.int64), DEV)
    return dbuf, doff


def _new_outputs(n):
    return (torch.full((n,), -1, dtype=torch.int32, device=DEV), torch.full((n,), 7, dtype=torch.uint8, device=DEV))


def _same(what, got, ref):
    got = got.cpu().numpy()
    got = got.view(np.uint32) if got.dtype == np.int32 else got
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, f"{what}: {bad.size} differ from the oracle, first at {bad[:8]}"


class _Job:
    """One gate and one seal of a case on a stream, each into outputs and a copy of its own."""

    def __init__(self, case, dbuf, doff, pairs):
        self.case, self.dbuf, self.doff = case, dbuf, doff
        self.crc, self.valid = _new_outputs(case.n)
        self.seal_buf = dbuf.clone()
        self.seal_crc = torch.full((case.n,), -1, dtype=torch.int32, device=DEV)
        self.pairs = pairs

    def queue(self, engine, stream):
        data = self.dbuf[G.LEAD:]
        if self.pairs is not None:
            engine.crc_pairs(data, self.pairs, crc_out=self.crc, valid_out=self.valid, stream=stream)
        else:
            engine.crc_varlen(data, self.doff, crc_out=self.crc, valid_out=self.valid, stream=stream)
        engine.seal_varlen(self.seal_buf[G.LEAD:], self.doff, crc_out=self.seal_crc, stream=stream)

    def check(self, what):
        c = self.case
        order = slice(None, None, -1) if self.pairs is not None else slice(None)
        _same(f"{what} gate crc", self.crc, c.ref_crc[order])
        _same(f"{what} gate valid", self.valid, c.ref_valid[order])
        live = c.lens >= 4  # a span under 4 bytes gets no trailer and no seal CRC
        got = self.seal_crc.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[live], c.ref_crc[live]), f"{what}: seal crc_out differs from the oracle"
        _same(f"{what} sealed bytes", self.seal_buf, c.sealed)


@pytest.mark.parametrize("entry", ("csr", "pairs"))
def test_two_streams_then_release(engine, entry):
    cases = [G.varlen_case("stream_a"), G.varlen_case("stream_b")]
    dev = [_upload(c) for c in cases]
    pairs = [None, None]
    if entry == "pairs":  # the same frames in reverse order
        for k, c in enumerate(cases):
            p = np.ascontiguousarray(np.stack([c.off[:-1], c.off[1:]], axis=1)[::-1]).astype(np.int64)
            pairs[k] = G.to_device(p, DEV)
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    jobs = [[_Job(cases[k], *dev[k], pairs[k]) for k in range(2)] for _ in range(3)]
    torch.cuda.synchronize()  # inputs and output fills are on the default stream
    for rep in jobs:          # interleaved, nothing waited for until the end
        for k in range(2):
            rep[k].queue(engine, streams[k])
    torch.cuda.synchronize()
    for r, rep in enumerate(jobs):
        for k in range(2):
            rep[k].check(f"{entry} repetition {r} stream {k}")
    del jobs
    # released scratch is allocated (and its counts zeroed) again by the next call on the stream
    for s in streams:
        engine.release_stream(s)
    again = [_Job(cases[k], *dev[k], pairs[k]) for k in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        again[k].queue(engine, streams[k])
    torch.cuda.synchronize()
    for k in range(2):
        again[k].check(f"{entry} after release_stream, stream {k}")
    for s in streams:
        engine.release_stream(s)


def test_grow_and_shrink_on_one_stream(engine):
    """small, large, small, large with no synchronise: the deferred-frame list grows under queued work,
    and the large launches leave counts for workgroups that the small ones do not have."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    large = G.varlen_case("large", ncu)
    assert large.n == 64 * 16 * ncu and G.classes(large.lens)["ge1661"] >= 2000 and large.lens.mean() < 200
    seq = [G.varlen_case("small_64"), large, G.varlen_case("small_200"), large]
    dev = {id(c): _upload(c) for c in seq}
    jobs = [_Job(c, *dev[id(c)], None) for c in seq]
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    for j in jobs:
        j.queue(engine, stream)
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        j.check(f"batch {i} of small/large/small/large ({j.case.n} frames)")
    engine.release_stream(stream)


def test_lean_claim_counter_ring(engine):
    """Six rounds of 32 lean fixed launches over two streams and three shapes, one synchronise per
    round: the launches walk the ring of 64 claim-counter slots three times with fewer than 64 in
    flight, and each finds its slot zeroed by the launch that had it before."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = [(64, 67), (1500, 1001), (250, 4 * 8 * ncu + 5)]
    cases = [G.fixed_case(L, L, n) for L, n in shapes]
    for c in cases:
        assert G.lean_blocks(c.frame_len, c.stride, c.n) > 0
    dbufs = [G.to_device(c.buf, DEV) for c in cases]
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    for rnd in range(6):
        outs = [_new_outputs(cases[i % 3].n) for i in range(32)]
        torch.cuda.synchronize()
        for i in range(32):
            c = cases[i % 3]
            engine.crc_fixed(dbufs[i % 3][G.LEAD:], c.frame_len, c.stride, c.n, crc_out=outs[i][0],
                             valid_out=outs[i][1], stream=streams[i % 2])
        torch.cuda.synchronize()
        for i in range(32):
            c = cases[i % 3]
            what = f"round {rnd} launch {i} ({c.frame_len} B x {c.n})"
            _same(f"{what} crc", outs[i][0], c.ref_crc)
            _same(f"{what} valid", outs[i][1], c.ref_valid)
