"""GPU: the batched frame window (ufc_frame_window_varlen, FrameCrcEngine.frame_window) against
tests/window_expect.py and against the host call, byte for byte on every output: the scenarios and generators of
tests/test_window_cpu.py with the device call in the host call's place, at the smallest shapes that can go wrong;
a call on a second stream; the C ABI's NULL rules; and the whole path on the device, emit -> pack -> build -> seal
-> (frames lost and repeated) -> gate -> parse -> frame_window -> receive_packets, and the window's groups back
through pack -> build -> seal -> parse as ack frames."""
import ctypes

import numpy as np
import pytest
import torch

from uflow_amd import frame as fr
from uflow_amd.batch import records, rows
from uflow_amd.frame import FLUSH_DTYPE, PACKET_DTYPE, SENDER_DTYPE

import window_expect as E
import test_window_cpu as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8 = np.uint8


def _host_out(d):
    return {"frame_accept": d["frame_accept"].cpu().numpy(),
            "groups": records(d["groups"], fr.ITEM_DTYPE),
            "group_first": d["group_first"].cpu().numpy().astype(np.uint64),
            "groups_used": int(d["groups_used"].cpu()[0]),
            "results": records(d["results"], fr.FRAME_WINDOW_RESULT_DTYPE),
            "windows_out": records(d["windows_out"], fr.FRAME_WINDOW_DTYPE)}


def gpu_call(engine, stream=None):
    """test_window_cpu.host's calling convention on the device form.  (group_first and results are the wrapper's
    own tensors: the call writes every entry of both.)"""
    def call(infos, frame_first, windows, groups_cap, nthreads, frame_accept, groups, group_first, results, windows_out):
        d_w = rows(windows, DEV)
        d = engine.frame_window(rows(infos, DEV), rows(frame_first, DEV), d_w, groups_cap=groups_cap,
                                frame_accept=rows(frame_accept, DEV), groups=rows(groups, DEV),
                                windows_out=d_w if windows_out is windows else rows(windows_out, DEV), stream=stream)
        (stream.synchronize if stream is not None else torch.cuda.synchronize)()
        o = _host_out(d)
        if windows_out is windows:
            windows[:] = o["windows_out"]
            o["windows_out"] = windows
        return o
    return call


@pytest.mark.parametrize("case", T.GOLDEN, ids=[c["name"].split(":")[0].split(",")[0] for c in T.GOLDEN])
def test_golden_cases(engine, monkeypatch, case):
    monkeypatch.setattr(T, "host", gpu_call(engine))
    T.run_golden(case)


@pytest.mark.parametrize("scenario", T.SCENARIOS, ids=lambda f: f.__name__[9:])
def test_scenarios(engine, monkeypatch, scenario):
    """The host test's scenarios with the device call in the host call's place: hostile window sizes, the tile
    of 33 rounds, ids that come back, chained steps in place, groups_cap below need, BAD_STATE, and 70,000
    connections (more than the walk's launch grid holds in one pass)."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    scenario()


@pytest.mark.parametrize("n_connections", [1, 3, 70])
def test_generated_traffic(engine, monkeypatch, n_connections):
    """1, 3 and 70 connections of 0, 1, 63, 64, 65 and 130 frames (one of them takes each count in turn)."""
    monkeypatch.setattr(T, "host", gpu_call(engine))
    if n_connections == 70:
        T.scenario_generated(seed=11, n_connections=70)
        return
    for k in range(len(T.COUNTS)):   # every frame count in the first connection's place
        rng = np.random.default_rng(100 + k)
        counts = [T.COUNTS[(k + j) % len(T.COUNTS)] for j in range(n_connections)]
        infos, ff, w = E.make_batch(rng, counts, hostile_every=3)
        T.run(infos, ff, w)


def test_equals_the_host_call(engine):
    """The same batch through ufc_frame_window_host and the device call: every output byte for byte."""
    rng = np.random.default_rng(61)
    infos, ff, w = E.make_batch(rng, T.COUNTS * 3, hostile_every=3)
    h = fr.frame_window_host(infos, ff, w, nthreads=4)
    d = engine.frame_window(rows(infos, DEV), rows(ff, DEV), rows(w, DEV))
    torch.cuda.synchronize()
    o = _host_out(d)
    assert o["groups_used"] == h["groups_used"] > 0
    for k in ("frame_accept", "groups", "group_first", "results", "windows_out"):
        assert o[k].tobytes() == h[k].tobytes(), k


def test_two_streams_two_batches(engine):
    """A call on a non-default stream next to a different batch on another stream: each has its own scratch."""
    rng = np.random.default_rng(71)
    a = E.make_batch(rng, [130, 65, 0, 64] * 40, hostile_every=4)
    b = E.make_batch(rng, [1, 63, 130] * 7, hostile_every=2)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    args = [(rows(x[0], DEV), rows(x[1], DEV), rows(x[2], DEV)) for x in (a, b)]
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        for (i, f, w), s in zip(args, (s1, s2)):
            outs.append(engine.frame_window(i, f, w, stream=s))
    s1.synchronize()
    s2.synchronize()
    for k, d in enumerate(outs):
        x = (a, b)[k % 2]
        want = E.expect_batch(*x)
        o = _host_out(d)
        assert o["groups_used"] == want["groups_used"]
        for key in ("frame_accept", "groups", "group_first", "results", "windows_out"):
            assert o[key].tobytes() == want[key].tobytes(), (k, key)
    engine.release_stream(s1)
    engine.release_stream(s2)


def test_argument_checks(engine):
    infos, ff, w = T.golden_batch(T.GOLDEN[1])
    a = (rows(infos, DEV), rows(ff, DEV), rows(w, DEV))
    with pytest.raises(ValueError):
        engine.frame_window(a[0], a[1][:1], a[2])
    with pytest.raises(ValueError):
        engine.frame_window(a[0], a[1], a[2], groups=torch.zeros((1, fr.ITEM_DTYPE.itemsize), dtype=torch.uint8, device=DEV), groups_cap=2)
    V = ctypes.c_void_p
    st = V(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    ok = [V(a[0].data_ptr()), 3, V(a[1].data_ptr()), V(a[2].data_ptr()), 1, V(p), V(p + 64), 4, V(p + 512), V(p + 640),
          V(p + 1024), V(p + 2048), st]
    call = fr.lib().ufc_frame_window_varlen
    assert call(engine._ctx, *ok) == 0
    for k in (0, 2, 3, 5, 6, 8, 9, 10, 11):
        bad = list(ok)
        bad[k] = None
        assert call(engine._ctx, *bad) == T.UFC_ERR_INVALID_ARG, k
    for k in (1, 4):
        bad = list(ok)
        bad[k] = (1 << 31) - 1
        assert call(engine._ctx, *bad) == T.UFC_ERR_INVALID_ARG, k
    assert call(None, *ok) == T.UFC_ERR_INVALID_ARG
    assert call(engine._ctx, None, 0, None, None, 0, None, None, 0, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert int(buf[640:648].cpu().numpy().view(np.uint64)[0]) == 2
    d = engine.frame_window(a[0][:0], rows(np.zeros(1, np.uint64), DEV), a[2][:0])   # no connections: UFC_OK
    assert d["groups"].shape[0] == 0


def test_whole_path_on_the_device(engine):
    """emit -> pack -> build -> seal for 3 senders; some sealed frames removed, others repeated; gate -> parse ->
    frame_window -> receive_packets(frame_accept): the repeated frames' datagrams are NOT_HANDLED.  Then the
    window's groups through pack (ack flushes) -> build -> seal -> parse: the ack frames carry the new base ids, the
    union of the group bits is exactly the accepted sequence ids, each group's nonce the XOR of those frames'."""
    rng = np.random.default_rng(81)
    n, per, FRAG = 3, 40, fr.MAX_FRAME_SIZE - 24
    packets = np.zeros(n * per, dtype=PACKET_DTYPE)
    sizes = rng.choice([0, 3, 60, 700, FRAG, FRAG + 1], size=packets.size)
    packets["data_len"] = sizes
    packets["data_offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packets["channel_id"] = rng.integers(0, 3, packets.size)
    packets["mode"] = fr.SEND_UNRELIABLE
    payload = rng.integers(0, 256, int(sizes.sum()), dtype=U8)
    senders = np.zeros(n, dtype=SENDER_DTYPE)
    senders["base_id"] = senders["next_id"] = rng.integers(0, 1 << 20, n)
    senders["window_size"], senders["max_alloc"], senders["take"] = 64, 1 << 30, per
    senders["window_parent_id"] = fr.NO_PARENT
    senders["channel_parent_id"] = fr.NO_PARENT
    items, iff, _, _, _, _ = engine.emit_packets(rows(packets, DEV), rows(np.arange(n + 1) * per, DEV), rows(senders, DEV),
                                                 items_cap=int(np.maximum(1, (sizes + FRAG - 1) // FRAG).sum()))
    first_ids = np.array([0xFFFFFFF8, 5, 0x12345678], dtype=np.uint64)   # (the first sender's ids wrap)
    flushes = np.zeros(n, dtype=FLUSH_DTYPE)
    flushes["kind"], flushes["flush_alloc"], flushes["window_room"], flushes["id0"] = fr.DATA, 1 << 40, 1 << 20, first_ids
    nonce_words = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    infos, res, frames_used = engine.pack_flushes(items, iff, rows(flushes, DEV), nonce_bits=rows(nonce_words.view(np.int32), DEV))
    wire, off, _ = engine.build_varlen(infos, items, rows(payload, DEV), seal=True)
    torch.cuda.synchronize()
    nfr = int(frames_used.cpu()[0])
    fres = records(res, fr.FLUSH_RESULT_DTYPE)
    assert (fres["frame_count"] >= 12).all()
    wire_h, off_h = wire.cpu().numpy(), off.cpu().numpy()[:nfr + 1]
    # what arrives: per sender every fifth frame lost, every third of the rest repeated at once, one older frame late
    arrive, owner, repeated = [], [], []
    accepted = [dict() for _ in range(n)]   # sequence id -> nonce
    for s in range(n):
        f0, fc = int(fres["frame_first"][s]), int(fres["frame_count"][s])
        for k in range(fc):
            g = f0 + k
            if k % 5 == 3:
                continue
            arrive.append(g), owner.append(s), repeated.append(False)
            accepted[s][(int(first_ids[s]) + k) & E.M32] = int(nonce_words[g // 32] >> (g % 32)) & 1
            if k % 3 == 1:
                arrive.append(g), owner.append(s), repeated.append(True)
            if k == 7:
                arrive.append(f0 + 2), owner.append(s), repeated.append(True)
    lens = [int(off_h[g + 1] - off_h[g]) for g in arrive]
    off2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wire2 = np.concatenate([wire_h[off_h[g]:off_h[g + 1]] for g in arrive])
    frame_first = np.searchsorted(np.array(owner), np.arange(n + 1)).astype(np.int64)
    d_wire, d_off = rows(wire2, DEV), rows(off2, DEV)
    _, valid = engine.crc_varlen(d_wire, d_off)
    infos2, items2, _ = engine.parse_varlen(d_wire, d_off, valid)
    windows = fr.new_frame_windows(n, 4096, first_ids.astype(np.uint32))
    fw = engine.frame_window(infos2, rows(frame_first, DEV), rows(windows, DEV))
    receivers = fr.new_receivers(n, 64, senders["base_id"])
    slots = torch.zeros((n * 64, fr.RX_SLOT_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    rx = engine.receive_packets(infos2, items2, d_wire, rows(frame_first, DEV), rows(receivers, DEV), slots,
                                rows(np.arange(n + 1) * 64, DEV), torch.zeros(0, dtype=torch.uint8, device=DEV),
                                src_base=d_off[:-1].contiguous(), frame_accept=fw["frame_accept"])
    torch.cuda.synchronize()
    o = _host_out(fw)
    assert valid.cpu().numpy().all()
    assert np.array_equal(o["frame_accept"], 1 - np.array(repeated, dtype=U8))
    h_infos = records(infos2, fr.FRAME_INFO_DTYPE)
    status = rx["item_status"].cpu().numpy()
    for i, f in enumerate(h_infos):
        st = status[int(f["item_first"]): int(f["item_first"]) + int(f["item_count"])]
        assert f["item_count"] > 0 and ((st == fr.RX_NOT_HANDLED).all() if repeated[i] else (st != fr.RX_NOT_HANDLED).all()), i
    # the same window step on the host
    h = fr.frame_window_host(h_infos, frame_first.astype(np.uint64), windows)
    for k in ("frame_accept", "groups", "group_first", "results", "windows_out"):
        assert o[k].tobytes() == h[k].tobytes(), k
    # the acks: one ack flush per connection over the window's groups
    used = o["groups_used"]
    rx_base = records(rx["receivers_out"], fr.RECEIVER_DTYPE)["base_id"]
    ack = np.zeros(n, dtype=FLUSH_DTYPE)
    ack["kind"], ack["flush_alloc"] = fr.ACK, 1 << 40
    ack["id0"], ack["id1"] = o["windows_out"]["base_id"], rx_base
    a_infos, a_res, a_used = engine.pack_flushes(fw["groups"][:used].contiguous(), fw["group_first"], rows(ack, DEV))
    a_wire, a_off, a_status = engine.build_varlen(a_infos, fw["groups"][:used].contiguous(),
                                                  torch.zeros(0, dtype=torch.uint8, device=DEV), seal=True)
    torch.cuda.synchronize()
    na = int(a_used.cpu()[0])
    assert na == n and (a_status.cpu().numpy()[:na] == 0).all()
    a_off = a_off[:na + 1].contiguous()
    _, a_valid = engine.crc_varlen(a_wire, a_off)
    p_infos, p_items, p_used = engine.parse_varlen(a_wire, a_off, a_valid)
    torch.cuda.synchronize()
    p_infos = records(p_infos, fr.FRAME_INFO_DTYPE)
    p_items = records(p_items, fr.ITEM_DTYPE)
    assert int(p_used.cpu()[0]) == used and a_valid.cpu().numpy().all()
    for s in range(n):
        f = p_infos[s]
        assert f["ok"] == 1 and f["kind"] == fr.ACK
        last = max(accepted[s], key=lambda q: (q - int(first_ids[s])) & E.M32)
        assert int(f["f"][0]) == (last + 1) & E.M32 == int(o["windows_out"]["base_id"][s])
        assert int(f["f"][1]) == int(rx_base[s])
        seen = {}
        for g in p_items[int(f["item_first"]): int(f["item_first"]) + int(f["item_count"])]:
            ids = [(int(g["id"]) + b) & E.M32 for b in range(32) if (int(g["data_offset"]) >> b) & 1]
            assert ids and not set(ids) & set(seen)
            nonce = 0
            for q in ids:
                assert q in accepted[s], (s, q)
                nonce ^= accepted[s][q]
                seen[q] = 1
            assert int(g["channel_id"]) == nonce, (s, int(g["id"]))
        assert set(seen) == set(accepted[s])
