"""The batched frame routing on the device (ufc_route_frames_varlen, uflow_amd/csrc/route.hip) in the host call's
place: the scenarios of tests/test_route_cpu.py against the model, and the shapes at which the kernels take another
path against the host call, every output byte for byte.

The counts the shapes are chosen by (route.hip): a lane kernel (init, lookup, classify, gather, finish) launches at
most 1,024 workgroups of 256 lanes = 262,144 lanes, which stride over what lies beyond; a radix pass gives every
workgroup a tile of 1,024 frames (4 rounds of 256, 4 waves each) and launches a workgroup per tile, so it has no grid
to go past; the passes are the bytes of n_conns + 1: one up to 254 connections, two up to 65,534, three from
65,535."""
import numpy as np
import pytest
import torch

from uflow_amd import frame as fr, route as rt
from uflow_amd._native import lib
from uflow_amd.batch import records, rows

import route_expect as E
import test_route_cpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, U32, U64 = np.uint8, np.uint32, np.uint64
OUT_DT = {"route": U32, "cls": U8, "bucket_first": U64, "order": U32, "infos_out": fr.FRAME_INFO_DTYPE,
          "src_base_out": U64, "results": rt.ROUTE_RESULT_DTYPE, "timeout_out": U64}


def _up(a):
    return None if a is None else rows(a, DEV)


def _down(d):
    out = {k: records(d[k], dt) for k, dt in OUT_DT.items()}
    out["first_unknown_control"] = int(records(d["first_unknown_control"], U32)[0])
    return out


def device_args(infos, addrs, offsets, table, conn_active, timeout_in):
    return [_up(infos), _up(addrs), _up(offsets), _up(table.slots), table.seed, table.max_probe,
            _up(np.ascontiguousarray(conn_active, dtype=U8))], _up(np.ascontiguousarray(timeout_in, dtype=U64))


def gpu_route(engine):
    def call(infos, addrs, offsets, table, conn_active, now_ms, active_timeout_ms, timeout_in, nthreads=1,
             timeout_out=None, **kw):
        args, d_tin = device_args(infos, addrs, offsets, table, conn_active, timeout_in)
        kw = {k: _up(v) for k, v in kw.items()}
        d = engine.route_frames(*args, now_ms, active_timeout_ms, d_tin,
                                timeout_out=d_tin if timeout_out is timeout_in else None, **kw)
        torch.cuda.synchronize()
        o = _down(d)
        for given, t in zip((infos, addrs, table.slots), (args[0], args[1], args[3])):      # the inputs are only read
            assert records(t, given.dtype).tobytes() == given.tobytes()
        if timeout_out is timeout_in:   # in place: the input's tensor took the output
            assert d["timeout_out"] is d_tin
            timeout_in[:] = o["timeout_out"]
            o["timeout_out"] = timeout_in
        return o
    return call


@pytest.fixture
def on_gpu(engine, monkeypatch):
    monkeypatch.setattr(T, "route_call", gpu_route(engine))


def vs_host(engine, case, what=""):
    """The device call against the host call (for the batches the sequential model would take long over)."""
    h = rt.route_frames_host(case.infos, case.addrs, case.offsets, case.table, case.active, case.now, case.tmo, case.tin,
                             nthreads=8)
    o = gpu_route(engine)(case.infos, case.addrs, case.offsets, case.table, case.active, case.now, case.tmo, case.tin)
    T.same(o, h, what)
    return o


# ---- the scenarios of the CPU file ----

@pytest.mark.parametrize("control_at", ["first", "middle", "last"])
def test_classification_rows(on_gpu, control_at):
    T.test_classification_rows(control_at)


@pytest.mark.parametrize("known", [7, 4, 1, 0])
def test_keys_are_32_bytes(on_gpu, known):
    T.test_keys_are_32_bytes(known)


@pytest.mark.parametrize("short", [False, True])
def test_chain_wraps_past_the_table_end(on_gpu, short):
    T.test_chain_wraps_past_the_table_end(short)


def test_garbage_table_has_one_answer(on_gpu):
    T.test_garbage_table_has_one_answer()


@pytest.mark.parametrize("seed,n,n_conns", [(1, 1, 1), (2, 64, 3), (3, 500, 40), (4, 2000, 300), (5, 1500, 0)])
def test_random_batches(on_gpu, seed, n, n_conns):
    T.test_random_batches(seed, n, n_conns)


def test_outputs(on_gpu):
    T.test_timeout_wraps_and_may_be_in_place()
    T.test_no_offsets_reads_as_zero()
    T.test_empty_batch()


# ---- shapes ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_batches_around_a_wave_a_round_and_a_tile(engine, n):
    """A wave (64), a round of a tile (256) and a tile (1,024 frames, one workgroup of a pass), each - 1, + 0 and
    + 1, and a third tile with one frame; two passes (300 connections)."""
    o = vs_host(engine, T.scenario_random(100 + n, n, 300), f"n {n}")
    assert sorted(o["order"].tolist()) == list(range(n))


def test_batch_past_the_lane_kernels_grid(engine):
    """263,700 frames: past the 262,144 lanes of the lookup, classify and gather kernels' launch grids, so that their
    first lanes go round again, in 258 tiles; 263,000 connections, most of them silent: past the same grid in the
    init and finish kernels, and three passes."""
    rng = np.random.default_rng(5)
    n, n_conns = 263_700, 263_000
    conn = np.zeros(n_conns, dtype=rt.ADDR_DTYPE)
    conn["family"], conn["port"] = 4, 9000
    conn["ip"][:, :4] = np.arange(n_conns, dtype=">u4").view(U8).reshape(-1, 4)
    table = rt.new_route_table(conn, 99)
    who = np.where(rng.random(n) < 0.5, rng.integers(0, 40, n), rng.integers(0, n_conns, n))
    who[-300:] = n_conns - 1 - np.arange(300) % 7        # the last lanes' frames go to the last connections
    addrs = conn[who]
    addrs["port"][rng.random(n) < 0.05] = 1
    kinds = np.where(rng.random(n) < 0.001, 4, rng.choice([10, 11, 12], n))
    case = T.Case(T.mk_infos(kinds, rng.random(n) > 0.02, rng), addrs, table, rng.random(n_conns) > 0.1)
    o = vs_host(engine, case)
    assert (o["results"]["frames"][-7:] > 0).any() and (o["cls"] == E.DEFERRED).sum() > 100
    assert len(set(o["cls"].tolist())) == 4


@pytest.mark.parametrize("n_conns", [1, 254, 255, 256, 257, 65_534, 65_535, 65_537])
def test_connection_counts_at_the_digit_seams(engine, n_conns):
    """The largest key is n_conns + 1: 254 connections are the last to take one pass, 255 the first to take two,
    65,534 the last with two and 65,535 the first with three.  3,000 frames, most connections silent, the last
    connection and the two buckets behind it in use."""
    rng = np.random.default_rng(n_conns)
    n = 3000
    conn = np.zeros(n_conns, dtype=rt.ADDR_DTYPE)
    conn["family"], conn["port"] = 4, 700
    conn["ip"][:, :4] = np.arange(n_conns, dtype=">u4").view(U8).reshape(-1, 4)
    table = rt.new_route_table(conn, 4242)
    who = rng.integers(0, n_conns, n)
    who[::5] = n_conns - 1
    who[1::5] = (n_conns - 1) & ~255            # keys that differ in a higher digit alone
    addrs = conn[who]
    unknown = rng.random(n) < 0.1
    addrs["port"][unknown] = 1
    kinds = np.where(unknown & (rng.random(n) < 0.1), 0, rng.choice([10, 11, 12], n))   # control from strangers only
    case = T.Case(T.mk_infos(kinds, rng.random(n) > 0.05, rng), addrs, table, np.ones(n_conns, U8))
    o = vs_host(engine, case, f"{n_conns} connections")
    assert o["results"]["frames"][n_conns - 1] > 100 and np.diff(o["bucket_first"].astype(np.int64))[-2:].min() > 0


def _conn_table(n_conns, seed=3):
    conn = rt.addr_records([T.v4(k + 1) for k in range(n_conns)])
    return conn, rt.new_route_table(conn, seed)


@pytest.mark.parametrize("what", ["one connection", "unknown", "dropped", "control"])
def test_one_bucket_takes_every_frame(engine, what):
    """5,000 frames in one bucket: connection 6 of 9, the dropped bucket (unknown addresses; frames that did not
    parse), the control bucket.  Every wave counts one bucket and every digit cursor but one stands still."""
    n = 5000
    conn, table = _conn_table(9)
    addrs = np.repeat(conn[6:7], n)
    infos = T.mk_infos([10] * n)
    if what == "unknown":
        addrs["port"] = 1
    elif what == "dropped":
        infos["ok"] = 0
    elif what == "control":
        infos["kind"] = 2
    o = vs_host(engine, T.Case(infos, addrs, table, np.ones(9, U8)), what)
    bucket = {"one connection": 6, "unknown": 10, "dropped": 10, "control": 9}[what]
    assert np.diff(o["bucket_first"].astype(np.int64)).tolist() == [n if b == bucket else 0 for b in range(11)]
    assert o["order"].tolist() == list(range(n))


@pytest.mark.parametrize("first", [63, 64, 65])
def test_buckets_that_begin_at_lane_63_and_lane_0(engine, first):
    """Connection 0 has `first` frames and connection 1 a single one, so that connection 1's bucket begins at lane 63
    of the first wave of grouped positions, at lane 0 of the second, or at lane 1, and connection 2's one lane on;
    the frames arrive interleaved."""
    rng = np.random.default_rng(first)
    conn, table = _conn_table(4)
    who = np.array([0] * first + [1] + [2] * 200 + [3] * 70)
    who = who[rng.permutation(who.size)]
    o = vs_host(engine, T.Case(T.mk_infos([10] * who.size), conn[who], table, np.ones(4, U8)))
    assert o["bucket_first"].tolist()[:4] == [0, first, first + 1, first + 201]
    assert o["order"].tolist() == np.argsort(who, kind="stable").tolist()


def test_arrays_off_the_16_byte_grid(engine):
    """The records are 4-byte aligned by their types, and the gather reads and writes 16 bytes at a time only where
    it sees infos and infos_out 16-byte aligned: the same call with infos, addrs, slots and infos_out 4 bytes into
    their allocations takes its dword form."""
    case = T.scenario_random(88, 3000, 200)

    def shifted(a, width):
        raw = _up(a).reshape(-1)
        buf = torch.zeros(raw.numel() + 16, dtype=torch.uint8, device=DEV)
        buf[4:4 + raw.numel()] = raw
        t = buf[4:4 + raw.numel()].view(-1, width)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    out = shifted(np.zeros(3000, dtype=fr.FRAME_INFO_DTYPE), 32)
    d = engine.route_frames(shifted(case.infos, 32), shifted(case.addrs, 32), _up(case.offsets),
                            shifted(case.table.slots, 48), case.table.seed, case.table.max_probe, _up(case.active),
                            case.now, case.tmo, _up(case.tin), infos_out=out)
    torch.cuda.synchronize()
    assert d["infos_out"] is out
    T.same(_down(d), rt.route_frames_host(case.infos, case.addrs, case.offsets, case.table, case.active, case.now,
                                          case.tmo, case.tin))


def test_same_call_three_times(engine):
    """The same call twice on one engine and once on a second stream: identical outputs (nothing depends on the
    order in which the atomics land)."""
    case = T.scenario_random(77, 20_000, 500, control=0.05)
    args, d_tin = device_args(case.infos, case.addrs, case.offsets, case.table, case.active, case.tin)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    outs = [engine.route_frames(*args, case.now, case.tmo, d_tin), engine.route_frames(*args, case.now, case.tmo, d_tin),
            engine.route_frames(*args, case.now, case.tmo, d_tin, stream=stream)]
    stream.synchronize()
    torch.cuda.synchronize()
    got = [_down(d) for d in outs]
    T.same(got[1], got[0])
    T.same(got[2], got[0])
    T.same(got[0], rt.route_frames_host(case.infos, case.addrs, case.offsets, case.table, case.active, case.now,
                                        case.tmo, case.tin))
    engine.release_stream(stream)


# ---- the routed batch through the stages behind it, on the device ----

def test_routed_batch_through_window_and_receive(engine):
    """tests/test_route_cpu.py's chained test with every call queued on device tensors: the parse, the routing, the
    frame window and the receive, with no host pass in between; against the host stages over the same frames grouped
    beforehand by a stable argsort."""
    n_conns = 5
    wire, off, owner, arrive = T.chained_traffic(n_conns=n_conns)
    conn = rt.addr_records([T.v4(50 + c, 6000 + c) for c in range(n_conns)])
    table = rt.new_route_table(conn, 424242)
    wire_a, off_a = T.reorder(wire, off, arrive)
    d_wire, d_off = _up(wire_a), _up(off_a)
    _, valid = engine.crc_varlen(d_wire, d_off)
    infos, items, _ = engine.parse_varlen(d_wire, d_off, valid)
    r = engine.route_frames(infos, _up(conn[owner]), d_off[:-1], _up(table.slots), table.seed, table.max_probe,
                            _up(np.ones(n_conns, U8)), 10, 20, _up(np.zeros(n_conns, U64)))
    frame_first = r["bucket_first"][:n_conns + 1]       # unchanged, the stages' frame_first
    windows = fr.new_frame_windows(n_conns, 4096, (1000 * np.arange(n_conns)).astype(U32))
    fw = engine.frame_window(r["infos_out"], frame_first, _up(windows))
    receivers = fr.new_receivers(n_conns, 64, (100 * np.arange(n_conns) + 5).astype(U32))
    slots = torch.zeros((n_conns * 64, fr.RX_SLOT_DTYPE.itemsize), dtype=torch.uint8, device=DEV)
    rx = engine.receive_packets(r["infos_out"], items, d_wire, frame_first, _up(receivers), slots,
                                _up(np.arange(n_conns + 1, dtype=U64) * U64(64)),
                                torch.zeros(0, dtype=torch.uint8, device=DEV), src_base=r["src_base_out"],
                                frame_accept=fw["frame_accept"])
    torch.cuda.synchronize()
    # grouped beforehand, on the host
    grouped = np.argsort(owner, kind="stable")
    assert records(r["order"], U32).tolist() == grouped.tolist()
    wire_g, off_g = T.reorder(wire_a, off_a.astype(np.int64), grouped)
    infos_g, items_g = fr.parse_batch_host(wire_g, off_g)
    ff_g = np.searchsorted(owner[grouped], np.arange(n_conns + 1)).astype(U64)
    fw_g, rx_g = T.stages(infos_g, items_g, wire_g, ff_g, off_g[:-1].copy(), n_conns, fr.frame_window_host,
                          fr.receive_packets_host)
    used = int(fw["groups_used"].cpu()[0])
    fw_h = {"frame_accept": records(fw["frame_accept"], U8), "groups": records(fw["groups"], fr.ITEM_DTYPE)[:used],
            "group_first": records(fw["group_first"], U64), "results": records(fw["results"], fr.FRAME_WINDOW_RESULT_DTYPE),
            "windows_out": records(fw["windows_out"], fr.FRAME_WINDOW_DTYPE)}
    fw_g = dict(fw_g, groups=fw_g["groups"][:used])
    rx_dt = {"packets": fr.RX_PACKET_DTYPE, "packet_first": U64, "out_bytes": U8, "carry_out": U8, "carry_first": U64,
             "results": fr.RECEIVER_RESULT_DTYPE, "receivers_out": fr.RECEIVER_DTYPE, "item_status": U8}
    rx_h = {k: records(rx[k], dt) for k, dt in rx_dt.items()}
    for k in ("packets_used", "out_used", "carry_used"):
        rx_h[k] = int(rx[k].cpu()[0])
    T.compare_stages(fw_h, rx_h, records(r["infos_out"], fr.FRAME_INFO_DTYPE), fw_g, rx_g, infos_g)
    assert rx_h["packets_used"] > 0 and fw_h["frame_accept"].all()


# ---- the wrappers' checks ----

def test_argument_contract(engine):
    """The header's argument rules through the device entry point, on device memory."""
    stream = torch.cuda.current_stream(engine.device).cuda_stream

    def call(**a):
        rc = lib().ufc_route_frames_varlen(engine._ctx, *a.values(), stream)
        torch.cuda.synchronize()
        return rc
    T.argument_contract(call, put=_up, addr=lambda t: t.data_ptr())
    args, _ = T.raw_args(put=_up, addr=lambda t: t.data_ptr())
    assert lib().ufc_route_frames_varlen(None, *args.values(), stream) == T.UFC_ERR_INVALID_ARG


def test_wrapper_refuses_bad_tensors(engine, monkeypatch):
    """Device, row width, dtype and size of every tensor are checked before the C entry point is reached and before
    any output is allocated."""
    from uflow_amd import _native

    def reached(*a):
        raise AssertionError("the C entry point was reached")
    monkeypatch.setattr(_native.lib(), "ufc_route_frames_varlen", reached)
    c = T.scenario_random(41, 6, 3)
    args, d_tin = device_args(c.infos, c.addrs, c.offsets, c.table, c.active, c.tin)
    names = ("infos", "addrs", "offsets", "slots", "seed", "max_probe", "conn_active")
    kw = dict(zip(names, args), now_ms=1, active_timeout_ms=2, timeout_in=d_tin,
              infos_out=torch.zeros((6, 32), dtype=torch.uint8, device=DEV),
              src_base_out=torch.zeros(6, dtype=torch.int64, device=DEV),
              timeout_out=torch.zeros(3, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    for k, v in kw.items():
        if not isinstance(v, torch.Tensor):
            continue
        bads = [v.cpu()] + ([v[:, :-1].contiguous()] if v.dim() == 2 else [v.to(torch.int16)])
        if k not in ("infos", "slots", "conn_active"):      # (these three set the counts)
            bads.append(v[:-1])
        for bad in bads:
            before = torch.cuda.memory_allocated()
            with pytest.raises(ValueError):
                engine.route_frames(**dict(kw, **{k: bad}))
            assert torch.cuda.memory_allocated() == before, k
