"""CPU: the batched host pack (ufc_pack_host, uflow_amd.frame.pack_host) against tests/pack_expect.py, the
emitters' push / finalize loop of src/half_connection/emit.rs restated item by item over the codec oracle's
encoded sizes."""
import ctypes
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from uflow_amd import _native
from uflow_amd._build import HIPCC, REPO_DIR
from uflow_amd.frame import FLUSH_DTYPE, FLUSH_RESULT_DTYPE, FRAME_INFO_DTYPE, ITEM_DTYPE, pack_host

import pack_expect as PE


def _run(batch, nthreads=1, **kw):
    items, first, flushes = batch.arrays()
    got = pack_host(items, first, flushes, nthreads=nthreads, **kw)
    PE.check(got, PE.expect(items, first, flushes, kw.get("nonce_bits")), kw.get("frames_cap"))
    return got, (items, first, flushes)


def test_reference_emitter_cases():
    """emit.rs's own tests, re-derived from the wire constants, by their outcome."""
    F = PE.MAX_FRAME_SIZE
    items, first, fl = PE.Flushes().add(PE.DATA, [PE.dgram(PE.MAX_FRAGMENT_SIZE, frag_last=1)] * 2,
                                        flush_alloc=2 * F).arrays()
    infos, res, used = pack_host(items, first, fl)
    assert used == 2 and list(infos["item_count"][:2]) == [1, 1] and res["stop"][0] == PE.DONE
    assert res["alloc_left"][0] == 0  # two frames of MAX_FRAME_SIZE bytes
    len_a, len_b = PE.DATA_FRAME_OVERHEAD + 11, PE.DATA_FRAME_OVERHEAD + 22
    ack_a, ack_b = PE.ACK_FRAME_OVERHEAD + 9, PE.ACK_FRAME_OVERHEAD + 18
    # (flush_alloc, pushes, items in the one frame, limited) of data_size_limited / ack_size_limited
    table = lambda a, b: [(0, 1, 1, 0), (a - 1, 1, 1, 0), (a, 1, 1, 0), (a + 1, 1, 1, 0), (a, 2, 2, 0), (b - 1, 2, 2, 0),  # noqa: E731
                          (b, 2, 2, 0), (b + 1, 2, 2, 0), (b, 3, 3, 0), (0, 2, 1, 1), (a - 1, 2, 1, 1), (a, 2, 2, 0),
                          (a + 1, 2, 2, 0), (a, 3, 2, 1), (b - 1, 3, 2, 1), (b, 3, 3, 0), (b + 1, 3, 3, 0), (b, 4, 3, 1)]
    for kind, item, rows in ((PE.DATA, PE.dgram(5), table(len_a, len_b)), (PE.ACK, PE.group(), table(ack_a, ack_b))):
        for alloc, pushes, held, limited in rows:
            items, first, fl = PE.Flushes().add(kind, [item] * pushes, flush_alloc=alloc).arrays()
            infos, res, used = pack_host(items, first, fl)
            assert used == 1 and infos["item_count"][0] == held == res["items_packed"][0], (kind, alloc, pushes)
            assert res["stop"][0] == (PE.SIZE_LIMITED if limited else PE.DONE), (kind, alloc, pushes)
    items, first, fl = PE.Flushes().add(PE.DATA, [PE.dgram(PE.MAX_FRAGMENT_SIZE, frag_last=1)] * 6,
                                        flush_alloc=6 * F, window_room=5).arrays()
    infos, res, used = pack_host(items, first, fl)
    assert used == 5 and res["stop"][0] == PE.WINDOW_LIMITED and res["items_packed"][0] == 5
    for n, counts in ((161, [161]), (162, [161, 1])):
        items, first, fl = PE.Flushes().add(PE.ACK, [PE.group()] * n, flush_alloc=2 * F).arrays()
        infos, res, used = pack_host(items, first, fl)
        assert list(infos["item_count"][:used]) == counts and res["stop"][0] == PE.DONE


def test_single_cases():
    b = PE.single_cases()
    (infos, res, used), (items, first, flushes) = _run(b)
    # the cases are what they claim to be
    by_flush = lambda j: infos[res["frame_first"][j]:res["frame_first"][j] + res["frame_count"][j]]  # noqa: E731
    assert list(by_flush(0)["item_count"]) == [1, 1]
    n = flushes.size
    wrap = by_flush(n - 3)
    assert [int(x) for x in wrap["f"][:, 0]] == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1]
    assert res["frame_count"][n - 2] == 0 and res["stop"][n - 2] == PE.SIZE_LIMITED and res["alloc_left"][n - 2] == -1
    # with nonce bits, and on several threads
    _run(b, nonce_bits=PE.nonce_words(3, items.size))
    _run(b, nthreads=4, nonce_bits=PE.nonce_words(4, items.size))


def test_count_and_size_limits():
    for cnt, counts in ((127, [127]), (128, [127, 1])):
        items, first, fl = PE.Flushes().add(PE.DATA, [PE.dgram(0)] * cnt).arrays()
        infos, res, used = pack_host(items, first, fl)
        assert list(infos["item_count"][:used]) == counts
    items, first, fl = PE.Flushes().add(PE.DATA, [PE.dgram(10), PE.dgram(20), PE.dgram(3000), PE.dgram(30),
                                                  PE.dgram(40)]).arrays()
    infos, res, used = pack_host(items, first, fl)
    assert list(infos["item_count"][:used]) == [2, 1, 2] and list(infos["item_first"][:used]) == [0, 2, 3]


def test_frames_cap_and_guard():
    b = PE.single_cases()
    items, first, flushes = b.arrays()
    exp = PE.expect(items, first, flushes)
    cap = exp[2] // 2
    guard = np.zeros(cap + 16, dtype=FRAME_INFO_DTYPE)
    guard.view(np.uint8)[:] = 0xA5
    got = pack_host(items, first, flushes, frames_cap=cap, infos=guard)
    PE.check(got, exp, frames_cap=cap)
    assert (guard.view(np.uint8).reshape(-1, 32)[cap:] == 0xA5).all(), "wrote past frames_cap"
    # frames_cap = 0: results and the count alone, no infos
    used = ctypes.c_uint64(0)
    res = np.zeros(flushes.size, dtype=FLUSH_RESULT_DTYPE)
    rc = _native.lib().ufc_pack_host(items.ctypes.data, items.size, first.ctypes.data, flushes.ctypes.data, flushes.size,
                                     None, None, 0, res.ctypes.data, ctypes.byref(used), 1)
    assert rc == 0 and used.value == exp[2]
    PE.check((np.zeros(0, FRAME_INFO_DTYPE), res, used.value), exp, frames_cap=0)


def test_empty_flushes_and_no_flushes():
    rng = random.Random(8)
    b = PE.Flushes()
    for n in (0, 0, 5, 0, 0, 0, 40, 1, 0):
        b.add(PE.DATA, [PE.rand_dgram(rng) for _ in range(n)], flush_alloc=-1 if n == 0 else 1 << 40)
    (infos, res, used), _ = _run(b)
    assert list(res["frame_count"] > 0) == [False, False, True, False, False, False, True, True, False]
    assert (res["stop"] == PE.DONE).all()  # an empty flush pushes nothing, whatever its flush_alloc
    # n_flushes == 0: UFC_OK whatever the pointers
    assert _native.lib().ufc_pack_host(None, 0, None, None, 0, None, None, 0, None, None, 1) == 0
    infos, res, used = pack_host(np.zeros(0, ITEM_DTYPE), np.zeros(1, np.uint64), np.zeros(0, FLUSH_DTYPE))
    assert used == 0 and res.size == 0


def test_argument_checks():
    items, first, flushes = PE.Flushes().add(PE.DATA, [PE.dgram(1)]).arrays()
    infos = np.zeros(1, FRAME_INFO_DTYPE)
    res = np.zeros(1, FLUSH_RESULT_DTYPE)
    used = ctypes.c_uint64(0)
    good = [items.ctypes.data, 1, first.ctypes.data, flushes.ctypes.data, 1, None, infos.ctypes.data, 1, res.ctypes.data,
            ctypes.byref(used), 1]
    assert _native.lib().ufc_pack_host(*good) == 0 and used.value == 1
    for k in (0, 2, 3, 6, 8, 9):  # items, flush_first, flushes, infos, results, frames_used
        bad = list(good)
        bad[k] = None
        assert _native.lib().ufc_pack_host(*bad) == _native.UFC_ERR_INVALID_ARG, k
    for k in (1, 4):  # n_items, n_flushes at 2^31 - 1
        bad = list(good)
        bad[k] = (1 << 31) - 1
        assert _native.lib().ufc_pack_host(*bad) == _native.UFC_ERR_INVALID_ARG, k


def test_bad_ranges_leave_neighbours_alone():
    rng = random.Random(9)
    items = np.array([PE.rand_dgram(rng) for _ in range(60)], dtype=ITEM_DTYPE)
    # flushes: [0, 20), [20, 10) reversed, [10, 30), [30, 61) past n_items, [61, 61) past n_items, [61, 40)
    # reversed and past, [40, 60)
    first = np.array([0, 20, 10, 30, 61, 61, 40, 60], dtype=np.uint64)
    flushes = np.zeros(7, dtype=FLUSH_DTYPE)
    flushes["kind"], flushes["flush_alloc"], flushes["window_room"] = PE.DATA, 5000, 100
    flushes["id0"] = np.arange(7) * 1000
    for nthreads in (1, 4):
        got = pack_host(items, first, flushes, nthreads=nthreads)
        PE.check(got, PE.expect(items, first, flushes))
        res = got[1]
        assert list(res["stop"] == PE.BAD_RANGE) == [False, True, False, True, True, True, False]
        assert (res["frame_count"][[1, 3, 4, 5]] == 0).all() and (res["alloc_left"][[1, 3, 4, 5]] == 5000).all()
        assert (res["frame_count"][[0, 2, 6]] > 0).all()


def test_flush_alloc_sweeps():
    """Every flush_alloc from -1 to the flush's total + 1, for a 3-frame data flush and a 170-group ack flush."""
    (infos, res, used), (items, first, flushes) = _run(PE.sweep_cases())
    assert set(res["stop"]) == {PE.DONE, PE.SIZE_LIMITED}
    assert set(res["frame_count"][flushes["kind"] == PE.DATA]) == {0, 1, 2, 3}
    assert set(res["frame_count"][flushes["kind"] == PE.ACK]) == {0, 1, 2}


@pytest.mark.parametrize("nthreads", [1, 4])
def test_random_batches(nthreads):
    b = PE.random_batch(21, 2000, 60)
    items, _, _ = b.arrays()
    (infos, res, used), _ = _run(b, nthreads=nthreads, nonce_bits=PE.nonce_words(6, items.size))
    assert {PE.DONE, PE.SIZE_LIMITED, PE.WINDOW_LIMITED} == set(res["stop"])


@pytest.mark.parametrize("nthreads", [1, 16])
def test_lane_cases(nthreads):
    """pack_expect.lane_cases: starts, stops and frame ends on lane 63, on lane 0 of the next slot and on item 0
    of the next tile of the chain kernel, and flushes at the seams of the hops kernel's window.  The host call
    runs the serial loop; the facts hold the generator to what it claims (asserted on the model's output)."""
    b = PE.lane_cases()
    items, first, flushes = b.arrays()
    exp = PE.expect(items, first, flushes)
    PE.check_facts(b, exp)
    for name in ("every_item_a_start[513]@7", "window_stop_at[256]@0", "size_stop_at[255]+1@7", "frames_of_64_exact@0",
                 "start_at_255_straddles[covers]@7", "ack_stops[322]@0", "hop_window_seams[last]", "short_beside_long[3]"):
        assert b.facts[name], name  # the named cases exist and carry facts
    nb = PE.nonce_words(63, items.size)
    PE.check(pack_host(items, first, flushes, nthreads=nthreads), exp)
    PE.check(pack_host(items, first, flushes, nthreads=nthreads, nonce_bits=nb), PE.expect(items, first, flushes, nb))
    b = PE.batch_end_case()
    (_, res, _), (items, first, flushes) = _run(b, nthreads=nthreads)
    PE.check_facts(b, PE.expect(items, first, flushes))


def test_pack_core_under_sanitizers():
    """tests/c/pack_host_check.hip: the pack core and the GPU pack's parallel form (prefix sums, hops, chain,
    ranks, stop predicate) as host code under AddressSanitizer and UBSan against the emitters' loop, and the
    kernels' tiling lane by lane over seeded flushes and over pack_expect.lane_cases' numbers with literals; a
    stand-alone program (nothing is loaded into Python under a sanitizer)."""
    src = os.path.join(REPO_DIR, "tests", "c", "pack_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pack_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
