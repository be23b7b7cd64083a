"""GPU: the device parse (ufc_parse_batch_varlen) on the named seam and limit cases of tests/parse_expect.py
(DESIGN section 5.15): lone owners on threads 0 and 255, workgroups without items, the rounds of the emit's item
loop, the header slots' 16/17 and 64/65 boundaries, the pool's last entry, the u16 slot limit, item caps through
every kind of frame, and the emit's byte-load path (offsets that go backwards, a workgroup span over 4 GiB).
Expected records come from oracle/codec.py alone; each batch runs twice on the device and must give the same bytes.
Every device buffer has 16 guard bytes behind the batch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import parse_expect
from uflow_amd import _native
from uflow_amd.batch import records
from uflow_amd.frame import FRAME_INFO_DTYPE, ITEM_DTYPE, parse_batch_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16


@functools.lru_cache(maxsize=None)
def _batches():
    out = parse_expect.lane_cases()
    for b in out:
        parse_expect.check_facts(b)
    return out


def _place(data, lead):
    """The batch's bytes `lead` bytes into a device buffer that goes on GUARD bytes behind them."""
    buf = torch.full((lead + data.size + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    buf[lead:lead + data.size] = torch.from_numpy(data).to(DEV)
    return buf, buf[lead:lead + data.size]


def _parse_raw(engine, d, o, n, valid, items, cap, infos=None):
    """ufc_parse_batch_varlen with the caller's item array (a tensor or None) and cap."""
    infos = torch.empty((n, FRAME_INFO_DTYPE.itemsize), dtype=torch.uint8, device=DEV) if infos is None else infos
    used = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    rc = _native.lib().ufc_parse_batch_varlen(
        engine._ctx, ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(o.data_ptr()), n, ctypes.c_void_p(valid.data_ptr()),
        ctypes.c_void_p(infos.data_ptr()), ctypes.c_void_p(items.data_ptr()) if items is not None else None, cap,
        ctypes.c_void_p(used.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return records(infos, FRAME_INFO_DTYPE), int(used.cpu()[0])


def _run_twice(engine, d, o, n, valid, exp_infos, exp_items):
    total = exp_items.size
    got = []
    for _ in range(2):
        items = torch.full((total + 8, ITEM_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=DEV)
        infos, used = _parse_raw(engine, d, o, n, valid, items, total + 8)
        raw = items.cpu().numpy()
        assert used == total
        assert (raw[total:] == 0xA5).all()
        got.append((infos, raw[:total].view(ITEM_DTYPE).reshape(-1)))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    parse_expect.compare(got[0][0], got[0][1], exp_infos, exp_items)
    return got[0]


@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("which", range(5))
def test_lane_cases(engine, which, lead):
    """Every batch of parse_expect.lane_cases at buffer alignments 0 and 3: field for field the oracle's records,
    record for record the host parse's, the same bytes from two runs."""
    batch = _batches()[which]
    exp_infos, exp_items = batch.records()
    data, offsets = batch.arrays()
    buf, d = _place(data, lead)
    o = torch.from_numpy(offsets).to(DEV)
    _, valid = engine.crc_varlen(d, o)
    infos, items = _run_twice(engine, d, o, len(batch.frames), valid, exp_infos, exp_items)
    ref_infos, ref_items = parse_batch_host(data, offsets.astype(np.uint64), None, nthreads=4)
    assert np.array_equal(infos, ref_infos) and np.array_equal(items, ref_items)
    assert (buf[lead + data.size:] == 0xEE).all() and (buf[:lead] == 0xEE).all()


@pytest.mark.parametrize("lead", [0, 3])
def test_caps(engine, lead):
    """mode_mix under item caps of 0, 1, a workgroup's first item, an item inside a slot frame and inside a
    re-walked frame, exactly the total, and no item array at all: infos and items_used as uncapped, the items
    below the cap the oracle's, a 0xA5-filled item array untouched from the cap on."""
    batch = parse_expect.mode_mix()
    parse_expect.check_facts(batch)
    exp_infos, exp_items = batch.records()
    assert exp_items.size == batch.total
    n = len(batch.frames)
    data, offsets = batch.arrays()
    _, d = _place(data, lead)
    o = torch.from_numpy(offsets).to(DEV)
    _, valid = engine.crc_varlen(d, o)
    free_infos, _ = _run_twice(engine, d, o, n, valid, exp_infos, exp_items)
    for cap in batch.caps:
        fill = torch.full((cap + 50, ITEM_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=DEV)
        infos, used = _parse_raw(engine, d, o, n, valid, fill, cap)
        assert used == batch.total, cap
        assert np.array_equal(infos, free_infos), cap
        got = fill.cpu().numpy()
        k = min(cap, batch.total)
        assert np.array_equal(got[:k].view(ITEM_DTYPE).reshape(-1), exp_items[:k]), cap
        assert (got[k:] == 0xA5).all(), cap
    infos, used = _parse_raw(engine, d, o, n, valid, None, 5)
    assert used == batch.total and np.array_equal(infos, free_infos)


@pytest.mark.parametrize("lead", [0, 3])
def test_fallback_backward_offsets(engine, lead):
    """Workgroup 0's bytes lie behind workgroup 1's: offsets[256] < offsets[0], the span test fails for workgroup
    0 and its frames' items come through the emit's byte loads.  The frame that ends the buffer's used bytes ends
    with a micro header, no payload and the trailer: the byte loads stay inside it (GUARD bytes follow all the
    same).  valid is the oracle's."""
    batch, data, offsets, valid = parse_expect.backward_offsets_case()
    parse_expect.check_facts(batch)
    exp_infos, exp_items = batch.records()
    _, d = _place(data, lead)
    o = torch.from_numpy(offsets).to(DEV)
    v = torch.from_numpy(valid).to(DEV)
    _run_twice(engine, d, o, len(batch.frames), v, exp_infos, exp_items)


def test_fallback_span_4gib(engine):
    """One workgroup whose span passes 4 GiB: a hundred frames at the start of a buffer of 2^32 + 8192 bytes, a
    rejected 4-GiB "frame", a hundred frames ending GUARD bytes before the buffer's end.  Only the two ends are
    filled."""
    total = 2 ** 32 + 8192
    batch, front, back, back_at, offsets, valid = parse_expect.span_4gib_case(total, GUARD)
    parse_expect.check_facts(batch)
    exp_infos, exp_items = batch.records()
    big = torch.empty(total, dtype=torch.uint8, device=DEV)
    big[:len(front)] = torch.frombuffer(bytearray(front), dtype=torch.uint8).to(DEV)
    big[back_at:back_at + len(back)] = torch.frombuffer(bytearray(back), dtype=torch.uint8).to(DEV)
    o = torch.from_numpy(offsets).to(DEV)
    v = torch.from_numpy(valid).to(DEV)
    _run_twice(engine, big, o, len(batch.frames), v, exp_infos, exp_items)
    del big
