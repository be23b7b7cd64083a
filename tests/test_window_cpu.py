"""CPU: the batched frame window on the host (ufc_frame_window_host, uflow_amd.frame.frame_window_host) against
tests/window_expect.py, ReceiveWindow and FrameAckQueue restated class for class from the reference, and the
hand-traced cases of tests/golden/frame_window_cases.json.  Every output buffer is pre-filled, so bytes the call
should not have written, and bytes it should have, both show.  tests/test_gpu_window.py runs the same scenarios
with the device call in `host`'s place."""
import ctypes
import json
import os

import numpy as np
import pytest

from uflow_amd import frame as fr
from uflow_amd._native import NativeError, UFC_ERR_INVALID_ARG, lib

import window_expect as E

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "frame_window_cases.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
FILL = 0xA5
COUNTS = [0, 1, 63, 64, 65, 130]  # frames per connection: none, one, around a tile, more than two tiles


def host(infos, frame_first, windows, groups_cap, nthreads, frame_accept, groups, group_first, results, windows_out):
    """The call under test (the GPU tests put the device call here)."""
    return fr.frame_window_host(infos, frame_first, windows, groups_cap=groups_cap, nthreads=nthreads,
                                frame_accept=frame_accept, groups=groups, group_first=group_first, results=results,
                                windows_out=windows_out)


def filled(n, dtype):
    return np.frombuffer(bytes([FILL]) * (n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = [k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} records differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


def run(infos, frame_first, windows, groups_cap=None, nthreads=1, in_place=False):
    """One call on pre-filled outputs, compared byte for byte with the expectation.  Returns (outputs, expected)."""
    n, nf = len(windows), len(infos)
    cap = n + nf if groups_cap is None else groups_cap
    pre = {"frame_accept": filled(nf, np.uint8), "groups": filled(cap, fr.ITEM_DTYPE)}
    want = E.expect_batch(infos, frame_first, windows, cap, prefill=pre)
    w_in = windows.copy()
    got = host(infos, frame_first, w_in, cap, nthreads, pre["frame_accept"].copy(), pre["groups"].copy(),
               filled(n + 1, np.uint64), filled(n, fr.FRAME_WINDOW_RESULT_DTYPE),
               w_in if in_place else filled(n, fr.FRAME_WINDOW_DTYPE))
    assert got["groups_used"] == want["groups_used"]
    same(got["group_first"][:n + 1], want["group_first"], "group_first")
    same(got["frame_accept"][:nf], want["frame_accept"], "frame_accept")
    same(got["results"][:n], want["results"], "results")
    same(got["windows_out"][:n], want["windows_out"], "windows_out")
    same(got["groups"][:cap], want["groups"], "groups")
    if not in_place:
        same(w_in, windows, "windows (input)")
    return got, want


def golden_batch(case):
    w = np.zeros(1, dtype=fr.FRAME_WINDOW_DTYPE)
    for k, v in case["state"].items():
        w[0][k] = v
    infos = np.zeros(len(case["frames"]), dtype=fr.FRAME_INFO_DTYPE)
    for k, f in enumerate(case["frames"]):
        infos[k] = E.data_info(f["id"], f["nonce"]) if f["kind"] == "data" else \
            E.sync_info(f["next_frame_id"], f["next_packet_id"])
    return infos, np.array([0, len(infos)], dtype=np.uint64), w


def run_golden(case):
    infos, ff, w = golden_batch(case)
    got, _ = run(infos, ff, w)
    assert got["frame_accept"][:len(infos)].tolist() == case["accept"]
    g = got["groups"][:got["groups_used"]]
    assert [[int(x["id"]), int(x["data_offset"]), int(x["channel_id"])] for x in g] == case["groups"]
    assert all(int(x["form"]) == 3 for x in g)
    out = np.zeros(1, dtype=fr.FRAME_WINDOW_DTYPE)
    for k, v in case["state_out"].items():
        out[0][k] = v
    same(got["windows_out"][:1], out, "state_out")
    for k, v in case["result"].items():
        assert int(got["results"][0][k]) == v, k
    assert int(got["results"][0]["group_count"]) == len(case["groups"]) and int(got["results"][0]["stop"]) == fr.FW_DONE


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"].split(":")[0].split(",")[0] for c in GOLDEN])
def test_golden_cases(case):
    run_golden(case)


def check_generator(facts):
    """What every generated batch must exercise, judged on the expectation's side."""
    assert facts["refused"] >= 1 and facts["sync_moved"] >= 1 and facts["sync_stayed"] >= 1, facts
    assert facts["tail_fold"] >= 1 and facts["tiles_with_rounds"] >= 1 and facts["max_rounds"] >= 2, facts


def scenario_generated(nthreads=1, seed=11, n_connections=None):
    """Seeded traffic over every frame count, every fourth connection hostile (random ids, random state)."""
    rng = np.random.default_rng(seed)
    counts = COUNTS * 2 if n_connections is None else [COUNTS[k % len(COUNTS)] for k in range(n_connections)]
    infos, ff, w = E.make_batch(rng, counts, hostile_every=4)
    _, want = run(infos, ff, w, nthreads=nthreads)
    check_generator(want["facts"])


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("seed", [11, 12])
def test_generated_traffic(nthreads, seed):
    scenario_generated(nthreads, seed)


def test_generated_traffic_70_connections():
    scenario_generated(4, 11, n_connections=70)


def scenario_hostile_sizes():
    """Hostile connections alone: window sizes 1 to 2^31, ids all over the id space, 24 random bytes of state."""
    rng = np.random.default_rng(5)
    infos, ff, w = E.make_batch(rng, [65, 130, 64, 1, 63, 130, 65, 64], hostile_every=1)
    _, want = run(infos, ff, w, nthreads=4)
    assert want["facts"]["max_rounds"] >= 3


def scenario_every_other_refused():
    """One tile in which every other frame is refused (33 rounds), then a tile of ordinary frames behind it."""
    w = fr.new_frame_windows(1, 4096, 1000)
    infos = np.zeros(64 + 40, dtype=fr.FRAME_INFO_DTYPE)
    for k in range(32):
        infos[2 * k] = E.data_info(1000 + k, k & 1)
        infos[2 * k + 1] = E.data_info(1000 + k, 1)  # the frame just seen, again
    for k in range(40):
        infos[64 + k] = E.data_info(1032 + k, k % 3 == 0)
    _, want = run(infos, np.array([0, len(infos)], dtype=np.uint64), w)
    assert want["facts"]["max_rounds"] == 33
    assert int(want["results"][0]["refused"]) == 32 and int(want["results"][0]["accepted"]) == 72


def scenario_ids_that_come_back():
    """size = 2^31: a sync between two data frames lets the same id in twice, into the same group; the second
    time its bit is set and the nonce stays ("only if the bit was clear", literally)."""
    w = fr.new_frame_windows(1, 1 << 31, 5)
    infos = np.array([E.data_info(5, 1), E.data_info(6, 1), E.sync_info((7 + (1 << 31)) & E.M32, None), E.data_info(6, 1),
                      E.data_info(7, 1), E.data_info(4, 1)], dtype=fr.FRAME_INFO_DTYPE)
    got, _ = run(infos, np.array([0, 6], dtype=np.uint64), w)
    assert got["frame_accept"][:6].tolist() == [1, 1, 0, 1, 1, 0]
    g = got["groups"][0]
    assert got["groups_used"] == 1 and (int(g["id"]), int(g["data_offset"]), int(g["channel_id"])) == (5, 7, 1)


def scenario_chained_steps():
    """Three steps chained through windows_out (in place), the tail kept in one chain and cleared in the other."""
    for clear in (False, True):
        rng = np.random.default_rng(21)
        counts = [130, 64, 0, 65, 1, 63]
        w = fr.new_frame_windows(len(counts), 256, 0xFFFFFF80)
        for step in range(3):
            fs = [E.make_connection(rng, c, size=256, base=int(w[r]["base_id"]))[1] for r, c in enumerate(counts)]
            infos = np.concatenate(fs)
            ff = np.zeros(len(counts) + 1, dtype=np.uint64)
            ff[1:] = np.cumsum(counts)
            got, want = run(infos, ff, w, in_place=True, nthreads=2)
            w = got["windows_out"][:len(counts)].copy()
            if step:
                assert clear or want["facts"]["tail_fold"] >= 1
            if clear:
                w["has_tail"] = 0
            counts = counts[1:] + counts[:1]


def scenario_groups_cap():
    """groups_cap below need and zero: the used count is exact, the state advances, nothing beyond the cap is
    written."""
    rng = np.random.default_rng(31)
    infos, ff, w = E.make_batch(rng, [65, 3, 130, 0, 64])
    _, full = run(infos, ff, w)
    need = full["groups_used"]
    assert need > 6
    for cap in (need - 1, need // 2, 1, 0):
        got, _ = run(infos, ff, w, groups_cap=cap)
        assert got["groups_used"] == need
        same(got["windows_out"][:len(w)], full["windows_out"], "state under a cap")


def scenario_bad_state():
    """size > 2^31 (frame_accept of its frames written 0), a reversed range and one outside the batch (nothing of
    theirs written), beside connections that are fine."""
    rng = np.random.default_rng(41)
    infos, ff, w = E.make_batch(rng, [5, 70, 4, 66, 3])
    w[1]["size"] = (1 << 31) + 1
    w[1]["has_tail"] = 1
    got, _ = run(infos, ff, w)
    assert int(got["results"][1]["stop"]) == fr.FW_BAD_STATE and int(got["results"][1]["group_count"]) == 0
    assert not got["frame_accept"][5:75].any()
    # ranges: empty, reversed, empty, all frames from 3 on, one frame past the batch's end; nobody owns frames 0..2
    nf = len(infos)
    ff2 = np.array([5, 5, 3, 3, nf, nf + 1], dtype=np.uint64)
    got, _ = run(infos, ff2, w)
    assert [int(x) for x in got["results"]["stop"][:5]] == [0, 1, 0, 0, 1]
    assert (got["frame_accept"][:3] == FILL).all() and (got["frame_accept"][3:nf] != FILL).all()


def scenario_many_connections():
    """More connections than the device walk's launch grid holds in one pass: 70,000 of 2 frames."""
    n = 70000
    rng = np.random.default_rng(51)
    w = fr.new_frame_windows(n, 64, 0)
    w["base_id"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    infos = np.zeros(2 * n, dtype=fr.FRAME_INFO_DTYPE)
    infos["kind"], infos["ok"], infos["crc_ok"] = fr.DATA, 1, 1
    infos["aux"] = rng.integers(0, 2, 2 * n)
    step = rng.integers(0, 3, n).astype(np.uint32)   # the second frame: a duplicate, the next id, a gap of one
    infos["f"][0::2, 0] = w["base_id"]
    infos["f"][1::2, 0] = w["base_id"] + step
    ff = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    got, _ = run(infos, ff, w)
    assert got["groups_used"] == n
    assert np.array_equal(got["frame_accept"][1:2 * n:2], (step != 0).astype(np.uint8))


# ---- the tiled walk's cross-lane reads on lane 0, on lane 63 and across the tile seam.  The same
# cases, with the same numbers, run in tests/c/window_host_check.hip under three lane orders.  Every case asserts on
# the model's side (facts) that its event sits where it was meant to. ----
def run_one(size, base, frames, tail=None):
    w = fr.new_frame_windows(1, size, base)
    if tail is not None:
        w[0]["has_tail"], (w[0]["tail_base_id"], w[0]["tail_bitfield"], w[0]["tail_nonce"]) = 1, tail
    infos = np.array(frames, dtype=fr.FRAME_INFO_DTYPE)
    got, want = run(infos, np.array([0, len(infos)], dtype=np.uint64), w)
    return got, want, want["facts"], want["results"][0]


def filler(k):
    """A frame that is nothing to the window: a data frame that is not ok, an ack frame."""
    if k % 2:
        return E.data_info(6, 1, ok=0)
    f = np.zeros((), dtype=fr.FRAME_INFO_DTYPE)
    f["kind"], f["ok"], f["crc_ok"] = fr.ACK, 1, 1
    f["f"][0] = 6
    return f


def scenario_duplicate_at_lane_63_and_over_the_seam():
    """A duplicate refused at lane 63 (against the candidate of lane 62), and once more at lane 0 of the next tile
    (against the base carried over the seam)."""
    frames = [E.data_info(1000 + k, k & 1) for k in range(63)] + [E.data_info(1062, 1), E.data_info(1062, 1), E.data_info(1063, 1)]
    _, want, facts, res = run_one(4096, 1000, frames)
    assert facts["refused_at"] == [63, 64] and facts["accepted_at"][-2:] == [62, 65], facts
    assert (int(res["accepted"]), int(res["refused"]), int(want["windows_out"][0]["base_id"])) == (64, 2, 1064)


def scenario_fold_at_lane_63_and_a_group_closed_over_the_seam():
    """Lane 63 folds into the open group and carries its only nonce; lane 0 of the next tile is 32 ids from the
    group's base: it closes the group and opens the next."""
    frames = [E.data_info(1000 + k, int(k == 63)) for k in range(64)] + [E.data_info(1064, 1)]
    got, want, facts, res = run_one(4096, 1000, frames)
    assert facts["groups_opened_at"] == [0, 32, 64] and facts["accepted_at"] == list(range(65)), facts
    assert [(int(g["id"]), int(g["data_offset"]), int(g["channel_id"])) for g in got["groups"][:3]] == \
        [(1000, 0xFFFFFFFF, 0), (1032, 0xFFFFFFFF, 1), (1064, 1, 1)] and got["groups_used"] == 3


def scenario_sync_at_lane_63():
    """A sync at lane 63 moves the base that lane 0 of the next tile is tested against (refused only against the
    moved base); packet syncs at lane 5, at lane 63 and at lane 1 of the next tile."""
    frames, nxt = [], 1000
    for k in range(63):
        if k == 5:
            frames.append(E.sync_info(None, 77))
        else:
            frames.append(E.data_info(nxt, k & 1))
            nxt += 1
    frames += [E.sync_info(nxt + 100, 78), E.data_info(nxt + 50, 1), E.sync_info(None, 79), E.data_info(nxt + 100, 1)]
    _, want, facts, res = run_one(4096, 1000, frames)
    assert facts["sync_moved_at"] == [63] and facts["refused_at"] == [64] and facts["accepted_at"][-1] == 66, facts
    assert E.ReceiveWindow(nxt, 4096).contains(nxt + 50)          # (what the unmoved base would have let in)
    assert (int(res["first_packet_sync"]), int(res["packet_syncs"]), int(res["syncs"])) == (5, 3, 3)
    assert int(want["windows_out"][0]["base_id"]) == nxt + 101


def scenario_64_refused_then_one():
    """Every candidate of a tile refused: 65 window rounds, the 65th on the word behind the 64 lanes' own; then a
    tile with one refusal."""
    frames = [E.data_info(999, k & 1) for k in range(64)] + [E.data_info(1000, 1), E.data_info(1000, 0), E.data_info(1001, 1)]
    got, want, facts, res = run_one(64, 1000, frames)
    assert facts["max_rounds"] == 65 and facts["tiles_with_rounds"] == 2 and facts["refused_at"] == list(range(64)) + [65], facts
    assert (int(res["accepted"]), int(res["refused"])) == (2, 65)
    g = got["groups"][0]
    assert (int(g["id"]), int(g["data_offset"]), int(g["channel_id"])) == (1000, 3, 0)


def scenario_64_groups_in_a_tile():
    """A carried tail out of reach and 64 accepted frames 40 ids apart: every lane closes the group before it (64
    group rounds with a stop test each, the most a tile takes); lane 0 of the next tile folds into the group lane 63
    opened."""
    frames = [E.data_info(1000 + 40 * k, k & 1) for k in range(64)] + [E.data_info(1000 + 40 * 63 + 31, 1)]
    got, want, facts, res = run_one(4096, 1000, frames, tail=(900, 1, 1))
    assert facts["groups_opened_at"] == list(range(64)) and facts["accepted_at"][-1] == 64, facts
    t, g = got["groups"][0], got["groups"][64]
    assert (int(t["id"]), int(t["data_offset"]), int(t["channel_id"])) == (900, 1, 1)
    assert got["groups_used"] == 65 and (int(g["id"]), int(g["data_offset"]), int(g["channel_id"])) == (3520, 0x80000001, 0)


def frames_that_come_back(first6):
    """data 5 | fillers | data 6 at first6 | a sync that moves the base by 2^31 | data 6 again | data 3 (refused)."""
    return [E.data_info(5, 0)] + [filler(k) for k in range(1, first6)] + \
        [E.data_info(6, 1), E.sync_info((7 + (1 << 31)) & E.M32, None), E.data_info(6, 1), E.data_info(3, 1)]


def ids_that_come_back_at(first6):
    got, want, facts, res = run_one(1 << 31, 5, frames_that_come_back(first6))
    assert facts["accepted_at"] == [0, first6, first6 + 2] and facts["groups_opened_at"] == [0], facts
    assert facts["sync_moved_at"] == [first6 + 1] and facts["refused_at"] == [first6 + 3], facts
    g = got["groups"][0]
    # the fold's stop test decides the nonce: with both 6s in one fold both would count as "the bit was clear" (0)
    assert got["groups_used"] == 1 and (int(g["id"]), int(g["data_offset"]), int(g["channel_id"])) == (5, 3, 1)


def scenario_comes_back_at_lane_63():
    """size = 2^31: the returning id 6 is the accepted lane 63, the lane before it among the accepted (61, the first
    6) in the same open group: its bit is set already, the nonce stays."""
    ids_that_come_back_at(61)


def scenario_comes_back_at_lane_0_of_the_next_tile():
    """The same with the first 6 at lane 62, the sync at lane 63 and the returning 6 at lane 0 of the next tile:
    the open group's bits are carried over the seam."""
    ids_that_come_back_at(62)


SCENARIOS = [scenario_hostile_sizes, scenario_every_other_refused, scenario_ids_that_come_back, scenario_chained_steps,
             scenario_groups_cap, scenario_bad_state, scenario_many_connections,
             scenario_duplicate_at_lane_63_and_over_the_seam, scenario_fold_at_lane_63_and_a_group_closed_over_the_seam,
             scenario_sync_at_lane_63, scenario_64_refused_then_one,
             scenario_64_groups_in_a_tile, scenario_comes_back_at_lane_63, scenario_comes_back_at_lane_0_of_the_next_tile]


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[9:])
def test_scenarios(scenario):
    scenario()


def test_record_layouts_and_new_windows():
    assert fr.FRAME_WINDOW_DTYPE.itemsize == 24 and fr.FRAME_WINDOW_RESULT_DTYPE.itemsize == 40
    w = fr.new_frame_windows(3, 4096, 7)
    assert w["base_id"].tolist() == [7, 7, 7] and w["size"].tolist() == [4096] * 3 and not w["has_tail"].any()
    assert not w["sync_reply"].any() and not w["tail_bitfield"].any()


def test_argument_rules():
    infos, ff, w = golden_batch(GOLDEN[1])
    n, nf = 1, len(infos)
    acc, groups = np.zeros(nf, np.uint8), np.zeros(n + nf, fr.ITEM_DTYPE)
    gf, res, wo = np.zeros(n + 1, np.uint64), np.zeros(n, fr.FRAME_WINDOW_RESULT_DTYPE), np.zeros(n, fr.FRAME_WINDOW_DTYPE)
    used = ctypes.c_uint64(0)
    ok = [infos.ctypes.data, nf, ff.ctypes.data, w.ctypes.data, n, acc.ctypes.data, groups.ctypes.data, n + nf,
          gf.ctypes.data, ctypes.addressof(used), res.ctypes.data, wo.ctypes.data, 1]
    call = lib().ufc_frame_window_host
    assert call(*ok) == 0 and used.value == 2
    for k in (0, 2, 3, 5, 6, 8, 9, 10, 11):   # every pointer: NULL is an error (infos and groups: with their counts)
        bad = list(ok)
        bad[k] = None
        assert call(*bad) == UFC_ERR_INVALID_ARG, k
    for k in (1, 4):                          # counts of 2^31 - 1 and beyond
        bad = list(ok)
        bad[k] = (1 << 31) - 1
        assert call(*bad) == UFC_ERR_INVALID_ARG, k
    assert call(None, 0, None, None, 0, None, None, 0, None, None, None, None, 1) == 0   # no windows: whatever the pointers
    nothing = list(ok)
    nothing[0], nothing[1], nothing[6], nothing[7] = None, 0, None, 0     # no frames and no room for groups: fine
    ff0 = np.zeros(2, np.uint64)
    nothing[2] = ff0.ctypes.data
    assert call(*nothing) == 0 and used.value == 0
    with pytest.raises(ValueError):
        fr.frame_window_host(infos, ff[:1], w)
    with pytest.raises(ValueError):
        fr.frame_window_host(infos, ff, w, groups=np.zeros(4, np.uint8))
    d = fr.frame_window_host(infos, ff, w)    # the defaults: the always-enough cap
    assert d["groups_used"] == 2 and len(d["groups"]) == n + nf
    assert isinstance(NativeError(UFC_ERR_INVALID_ARG), RuntimeError)


def test_window_core_under_sanitizers():
    """tests/c/window_host_check.hip: the wave-policy core of the frame window (fw_walk_tiles, the lanes of a phase
    run one after the other: forwards, backwards, shuffled, and on a carried shared block) as host code under AddressSanitizer and UBSan, against the serial walk
    (fw_walk_serial) on ordinary and hostile traffic and on random states, over exact-size buffers; a stand-alone
    program (nothing is loaded into Python under a sanitizer)."""
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(HERE, "c", "window_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "window_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
