"""The batched frame routing in host memory (ufc_route_table_build_host, ufc_route_frames_host,
include/uflow_route.h) against tests/route_expect.py's sequential model, byte for byte on every output; the header
against uflow_amd.records.ROUTE_RECORDS and uflow_amd._native.ROUTE_SYMBOLS; the routed batch through the frame window
and the packet receive.  tests/test_route_gpu.py runs the same scenarios with the device call in the host call's
place."""
import ctypes

import numpy as np
import pytest

from uflow_amd import frame as fr, route as rt
from uflow_amd._native import lib, UFC_ERR_INVALID_ARG, UFC_OK

import receive_expect as RX
import route_expect as E

U8, U32, U64 = np.uint8, np.uint32, np.uint64
OUT_KEYS = ("route", "cls", "bucket_first", "order", "infos_out", "src_base_out", "results", "timeout_out")
DATA, SYNC, ACK = 10, 11, 12


def route_call(infos, addrs, offsets, table, conn_active, now_ms, active_timeout_ms, timeout_in, **kw):
    """The call under test (tests/test_route_gpu.py puts the device call here)."""
    return rt.route_frames_host(infos, addrs, offsets, table, conn_active, now_ms, active_timeout_ms, timeout_in, **kw)


def mk_infos(kinds, ok=None, rng=None):
    """Frame records of the given kinds; the other fields random (they travel with the record, nothing reads them)."""
    n = len(kinds)
    rng = rng or np.random.default_rng(n)
    infos = np.frombuffer(rng.integers(0, 256, n * 32, dtype=U8).tobytes(), dtype=fr.FRAME_INFO_DTYPE).copy()
    infos["kind"] = kinds
    infos["ok"] = 1 if ok is None else ok
    return infos


def v4(k, port=4000):
    return ("10.%d.%d.%d" % ((k >> 16) & 255, (k >> 8) & 255, k & 255), port)


class Case:
    """One call's inputs.  clients: the dict the table stands for, or None when only the table's bytes can say."""

    def __init__(self, infos, addrs, table, active, offsets="iota", now=1000, tmo=5000, tin=None, clients="table"):
        self.infos, self.addrs, self.table = infos, np.ascontiguousarray(addrs, dtype=rt.ADDR_DTYPE), table
        self.active = np.ascontiguousarray(active, dtype=U8)
        n = infos.size
        self.offsets = (np.arange(n, dtype=U64) * U64(1472) + U64(3)) if isinstance(offsets, str) else offsets
        self.now, self.tmo = now, tmo
        self.tin = (np.arange(table.n_conns, dtype=U64) * U64(7) + U64(11)) if tin is None else np.asarray(tin, dtype=U64)
        self.clients = clients

    def call(self, **kw):
        return route_call(self.infos, self.addrs, self.offsets, self.table, self.active, self.now, self.tmo,
                          self.tin.copy(), **kw)

    def expect(self):
        clients = self.clients
        if isinstance(clients, str):    # from the table's own slots: every used slot is a client
            s = self.table.slots[self.table.slots["used"] != 0]
            clients = {E.key_bytes(x["key"]): int(x["conn"]) for x in s}
        t = self.table
        return E.route_frames(self.infos, self.addrs, self.offsets, t.slots, t.seed, t.max_probe, t.n_conns, self.active,
                              self.now, self.tmo, self.tin, clients)


def same(got, want, what=""):
    for k in OUT_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    assert int(got["first_unknown_control"]) == int(want["first_unknown_control"]), what


def check_case(case, what=""):
    o = case.call()
    exp = case.expect()
    same(o, exp, what)
    if case.clients is not None:        # a sane table: the bounded probe finds what the dict finds
        t = case.table
        byt = E.route_frames(case.infos, case.addrs, case.offsets, t.slots, t.seed, t.max_probe, t.n_conns, case.active,
                             case.now, case.tmo, case.tin, None)
        same(byt, exp, what + " (probe)")
    # what every caller relies on
    n, nc = case.infos.size, case.table.n_conns
    bf = o["bucket_first"].astype(np.int64)
    assert bf[0] == 0 and bf[-1] == n and (np.diff(bf) >= 0).all()
    assert sorted(o["order"].tolist()) == list(range(n))
    for b in range(nc + 2):
        seg = o["order"][bf[b]:bf[b + 1]].astype(np.int64)
        assert (np.diff(seg) > 0).all(), (what, b)
    return o


# ---- the table build ----

@pytest.mark.parametrize("n_conns,n_slots", [(0, 1), (1, 2), (5, 8), (5, 16), (100, 128), (1000, None)])
def test_table_build_bytes(n_conns, n_slots):
    addrs = rt.addr_records([v4(k * 7919 + 1, 1000 + k % 50) for k in range(n_conns)])
    t = rt.new_route_table(addrs, 0xC0FFEE11, n_slots)
    slots, max_probe = E.build_table(addrs, 0xC0FFEE11, t.slots.size)
    assert t.slots.tobytes() == slots.tobytes() and t.max_probe == max_probe and t.n_conns == n_conns
    if n_slots is None:
        assert t.slots.size == 2048     # the next power of two >= 2 * n_conns
    assert int((t.slots["used"] != 0).sum()) == n_conns


def test_table_build_duplicate_and_slot_rules():
    addrs = rt.addr_records([v4(k) for k in range(6)])
    addrs[4] = addrs[1]
    with pytest.raises(rt.DuplicateAddress) as e:
        rt.new_route_table(addrs, 5)
    assert e.value.index == 4 and E.build_table(addrs, 5, 16) == ("dup", 4)
    good = rt.addr_records([v4(k) for k in range(6)])
    slots = np.zeros(64, dtype=rt.ROUTE_SLOT_DTYPE)
    mp = np.zeros(1, dtype=U32)
    build = lambda a, n, s, ns, m, d=None: lib().ufc_route_table_build_host(a, n, 1, s, ns, m, d)   # noqa: E731
    A, S, M = good.ctypes.data, slots.ctypes.data, mp.ctypes.data
    assert build(A, 6, S, 8, M) == UFC_OK and build(A, 6, S, 64, M) == UFC_OK
    assert build(A, 6, S, 8, M, None) == UFC_OK          # dup_index is optional
    for ns in (0, 4, 6, 7, 12, 63):                      # not above n_conns, or not a power of two
        assert build(A, 6, S, ns, M) == UFC_ERR_INVALID_ARG, ns
    assert build(None, 6, S, 8, M) == UFC_ERR_INVALID_ARG and build(A, 6, None, 8, M) == UFC_ERR_INVALID_ARG
    assert build(A, 6, S, 8, None) == UFC_ERR_INVALID_ARG
    assert build(None, 0, S, 1, M) == UFC_OK and mp[0] == 0 and not slots[0]["used"]
    assert build(A, 2**31 - 3, S, 2**31, M) == UFC_ERR_INVALID_ARG      # the connection limit


def test_addr_records():
    a = rt.addr_records([("10.1.2.3", 80), ("::ffff:10.1.2.3", 80), ("fe80::1", 81, 5, 9)])
    assert a["family"].tolist() == [4, 6, 6] and a["port"].tolist() == [80, 80, 81]
    assert a["ip"][0].tolist() == [10, 1, 2, 3] + [0] * 12
    assert a["ip"][1].tolist() == [0] * 10 + [255, 255, 10, 1, 2, 3]
    assert (a["flowinfo"][2], a["scope_id"][2]) == (5, 9) and not a["reserved"].any() and not a["reserved2"].any()
    assert len({E.key_bytes(x) for x in a}) == 3
    with pytest.raises(ValueError):
        rt.addr_records([("10.1.2.3", 80, 0, 0)])


# ---- classification ----

def scenario_rows(control_at="middle"):
    """Every row of the header's table.  Connections: 0 active, 1 inactive, 2 active and silent, 3 active."""
    conn = rt.addr_records([v4(k) for k in range(4)])
    unk = rt.addr_records([v4(100), v4(101)])
    t = rt.new_route_table(conn, 77)
    rows = [(DATA, 1, conn[0]), (SYNC, 1, conn[3]), (ACK, 1, conn[1]),       # CONN, CONN, inactive: DROP
            (DATA, 1, unk[0]),                                                # unknown before any control: DROP
            (DATA, 0, conn[0]), (7, 1, conn[0]), (0xFF, 0, conn[0]), (13, 1, conn[3]),   # Frame::read gave None
            (4, 1, unk[1]),                                                   # unknown control (a disconnect)
            (DATA, 1, unk[0]), (ACK, 1, unk[1]),                              # unknown behind it: DEFERRED
            (0, 1, unk[0]),                                                   # a later unknown control: not the first
            (DATA, 1, conn[3]), (ACK, 1, conn[0]),                            # still CONN
            (3, 0, conn[3]),                                                  # a control kind that did not parse: DROP
            (ACK, 1, conn[3])]
    ctl = (5, 1, conn[0])
    if control_at == "first":
        rows = [ctl] + rows             # every session frame of connection 0 is deferred
    elif control_at == "last":
        rows = rows + [ctl]             # none is
    else:
        rows = rows[:1] + [ctl] + rows[1:]   # between two session frames of connection 0
    kinds, ok, addrs = zip(*rows)
    return Case(mk_infos(kinds, ok), np.stack(addrs), t, [1, 0, 1, 1])


@pytest.mark.parametrize("control_at", ["first", "middle", "last"])
def test_classification_rows(control_at):
    c = scenario_rows(control_at)
    o = check_case(c, control_at)
    n = c.infos.size
    at = {"first": 0, "middle": 1, "last": n - 1}[control_at]
    assert o["results"]["first_control"].tolist() == [at, E.NO_PARENT, E.NO_PARENT, E.NO_PARENT]
    s0 = [i for i in range(n) if E.kind_class(c.infos[i]) == "session" and o["route"][i] == 0]
    assert [int(o["cls"][i]) for i in s0] == [E.DEFERRED if i > at else E.CONN for i in s0]
    assert o["results"]["deferred"][0] == sum(i > at for i in s0)
    assert set(o["cls"].tolist()) == {E.DROP, E.CONN, E.CONTROL, E.DEFERRED} or control_at == "first"
    fuc = o["first_unknown_control"]
    assert c.infos["kind"][fuc] == 4 and o["route"][fuc] == E.NO_PARENT
    assert o["results"]["frames"][1] == 0 and o["timeout_out"][1] == c.tin[1]      # inactive: no refresh
    assert o["timeout_out"][3] == c.now + c.tmo and o["timeout_out"][2] == c.tin[2]


def scenario_keys(known):
    """V4 against V4-mapped V6, and keys that differ only in flowinfo, scope_id or port: `known` of them are
    connections, all of them send."""
    keys = rt.addr_records([("10.9.8.7", 500), ("::ffff:10.9.8.7", 500), ("10.9.8.7", 501), ("fe80::5", 500, 0, 0),
                            ("fe80::5", 500, 1, 0), ("fe80::5", 500, 0, 1), ("fe80::5", 501, 0, 0)])
    t = rt.new_route_table(keys[:known], 0xDEADBEEF)
    send = np.concatenate([keys, keys[::-1]])
    return Case(mk_infos([DATA, ACK] * keys.size), send, t, np.ones(known, dtype=U8))


@pytest.mark.parametrize("known", [7, 4, 1, 0])
def test_keys_are_32_bytes(known):
    c = scenario_keys(known)
    o = check_case(c)
    want = [k if k < known else E.NO_PARENT for k in list(range(7)) + list(range(6, -1, -1))]
    assert o["route"].tolist() == want


def scenario_wrapping_chain(short=False):
    """Five addresses whose home is slot 14 of 16, found with the model's hash: the chain runs 14, 15, 0, 1, 2.
    short: max_probe one below the displacement the last of them needs, which then counts as not found (only the
    table's bytes can say so: the model probes them too)."""
    seed = 31337
    conn = rt.addr_records(E.colliding_addrs(seed, 16, 14, 5))
    t = rt.new_route_table(conn, seed, 16)
    assert t.max_probe == 4 and [int(t.slots["conn"][s]) for s in (14, 15, 0, 1, 2)] == [0, 1, 2, 3, 4]
    assert [int(x) for x in t.slots["used"][[14, 15, 0, 1, 2, 3, 13]]] == [1, 1, 1, 1, 1, 0, 0]
    if short:
        t = rt.RouteTable(t.slots, t.seed, 3, t.n_conns)
    return Case(mk_infos([DATA] * 6), conn[[4, 0, 3, 1, 2, 4]], t, np.ones(5, dtype=U8), clients=None if short else "table")


@pytest.mark.parametrize("short", [False, True])
def test_chain_wraps_past_the_table_end(short):
    o = check_case(scenario_wrapping_chain(short))
    last = E.NO_PARENT if short else 4
    assert o["route"].tolist() == [last, 0, 3, 1, 2, last]
    assert o["cls"].tolist() == [E.DROP if short else E.CONN] + [E.CONN] * 4 + [E.DROP if short else E.CONN]


def scenario_garbage_table(seed=9, n_slots=64, n_conns=40, n=300):
    """Any bytes are a table: random slots, none empty, many with conn >= n_conns, a few holding keys that are sent
    (one of them twice, with different connections: the first on the probe's way wins)."""
    rng = np.random.default_rng(seed)
    slots = np.frombuffer(rng.integers(0, 256, n_slots * 48, dtype=U8).tobytes(), dtype=rt.ROUTE_SLOT_DTYPE).copy()
    slots["used"] = rng.integers(1, 256, n_slots)
    slots["conn"] = rng.integers(0, 2 * n_conns, n_slots)
    keys = rt.addr_records([v4(k, 77) for k in range(24)])
    where = rng.choice(n_slots, 24, replace=False)
    slots["key"][where] = keys
    slots["key"][(where[0] + 1) % n_slots] = keys[0]
    send = keys[rng.integers(0, 24, n)]
    kinds = rng.choice([DATA, SYNC, ACK, 0, 4, 9], n, p=[0.5, 0.15, 0.2, 0.05, 0.05, 0.05])
    t = rt.RouteTable(slots, 0x1234567, 0xFFFFFFFF, n_conns)
    return Case(mk_infos(kinds, rng.integers(0, 8, n) != 0, rng), send, t, rng.integers(0, 4, n_conns) != 0,
                clients=None)


def test_garbage_table_has_one_answer():
    c = scenario_garbage_table()
    o = check_case(c)
    assert (o["route"] != E.NO_PARENT).any() and (o["route"] == E.NO_PARENT).any()
    assert (o["route"][o["route"] != E.NO_PARENT] < 40).all()


def scenario_random(seed, n, n_conns, unknown=0.1, control=0.02, inactive=0.2, bad=0.05):
    rng = np.random.default_rng(seed)
    conn = rt.addr_records([v4(k * 131 + 5, 2000 + k % 7) for k in range(n_conns)])
    t = rt.new_route_table(conn, int(rng.integers(0, 2**32)))
    who = rng.integers(0, max(n_conns, 1), n)
    addrs = conn[who] if n_conns else np.zeros(n, dtype=rt.ADDR_DTYPE)
    unk = rng.random(n) < (unknown if n_conns else 1.0)
    addrs["port"][unk] = 9
    kinds = np.where(rng.random(n) < control, rng.integers(0, 6, n), rng.choice([DATA, SYNC, ACK], n))
    kinds = np.where(rng.random(n) < bad, rng.integers(0, 256, n), kinds)
    return Case(mk_infos(kinds, rng.random(n) >= bad, rng), addrs, t, rng.random(n_conns) >= inactive,
                now=int(rng.integers(0, 2**63)), tmo=int(rng.integers(0, 2**40)))


@pytest.mark.parametrize("seed,n,n_conns", [(1, 1, 1), (2, 64, 3), (3, 500, 40), (4, 2000, 300), (5, 1500, 0),
                                            (6, 3000, 2)])
def test_random_batches(seed, n, n_conns):
    check_case(scenario_random(seed, n, n_conns), f"seed {seed}")


def test_threads_give_the_same_bytes():
    c = scenario_random(11, 9000, 70)
    same(c.call(nthreads=4), c.call(nthreads=1))


# ---- outputs ----

def test_timeout_wraps_and_may_be_in_place():
    c = scenario_random(21, 200, 6, unknown=0, control=0, inactive=0, bad=0)
    c.now, c.tmo = 2**64 - 5, 10
    o = check_case(c)
    assert (o["results"]["frames"] > 0).all() and (o["timeout_out"] == 5).all()
    c.active[2] = 0
    tin = c.tin.copy()
    o2 = route_call(c.infos, c.addrs, c.offsets, c.table, c.active, c.now, c.tmo, tin, timeout_out=tin)
    assert o2["timeout_out"] is tin and tin.tolist() == [5, 5, int(c.tin[2]), 5, 5, 5]
    same(o2, c.expect())


def test_no_offsets_reads_as_zero():
    c = scenario_random(22, 300, 9)
    c.offsets = None
    o = check_case(c)
    assert not o["src_base_out"].any()


def test_empty_batch():
    c = scenario_random(23, 0, 5)
    o = check_case(c)
    assert not o["bucket_first"].any() and o["bucket_first"].size == 8
    assert (o["results"]["first_control"] == E.NO_PARENT).all() and not o["results"]["frames"].any()
    assert o["timeout_out"].tobytes() == c.tin.tobytes() and o["first_unknown_control"] == E.NO_PARENT


def raw_args(n=4, n_conns=3, n_slots=4, put=lambda a: a, addr=lambda a: a.ctypes.data):
    """A passing raw call's arguments by name, in the header's order, and the arrays that back them (put / addr: where
    an array goes and its address there; tests/test_route_gpu.py puts them on the device)."""
    c = scenario_random(31, n, n_conns)
    keep = dict(infos=c.infos, addrs=c.addrs, offsets=c.offsets, slots=c.table.slots, conn_active=c.active,
                timeout_in=c.tin, route=np.zeros(n, U32), cls=np.zeros(n, U8), bucket_first=np.zeros(n_conns + 3, U64),
                order=np.zeros(n, U32), infos_out=np.zeros(n, fr.FRAME_INFO_DTYPE), src_base_out=np.zeros(n, U64),
                results=np.zeros(n_conns, rt.ROUTE_RESULT_DTYPE), timeout_out=np.zeros(n_conns, U64), fuc=np.zeros(1, U32))
    keep = {k: put(v) for k, v in keep.items()}
    P = {k: addr(v) for k, v in keep.items()}
    args = dict(infos=P["infos"], addrs=P["addrs"], offsets=P["offsets"], n=n, slots=P["slots"], n_slots=n_slots,
                seed=c.table.seed, max_probe=c.table.max_probe, n_conns=n_conns, conn_active=P["conn_active"], now_ms=1,
                active_timeout_ms=2, timeout_in=P["timeout_in"], route=P["route"], cls=P["cls"],
                bucket_first=P["bucket_first"], order=P["order"], infos_out=P["infos_out"],
                src_base_out=P["src_base_out"], results=P["results"], timeout_out=P["timeout_out"],
                first_unknown_control=P["fuc"])
    return args, keep


def argument_contract(call, **where):
    """The header's argument rules, for a call(**args) -> status."""
    args, keep = raw_args(**where)
    assert call(**args) == UFC_OK
    assert call(**dict(args, offsets=None)) == UFC_OK
    for name in ("infos", "addrs", "slots", "conn_active", "timeout_in", "route", "cls", "bucket_first", "order",
                 "infos_out", "src_base_out", "results", "timeout_out", "first_unknown_control"):
        assert call(**dict(args, **{name: None})) == UFC_ERR_INVALID_ARG, name
    assert call(**dict(args, infos_out=args["infos"])) == UFC_ERR_INVALID_ARG          # no aliasing of the inputs
    assert call(**dict(args, src_base_out=args["offsets"])) == UFC_ERR_INVALID_ARG
    assert call(**dict(args, timeout_out=args["timeout_in"])) == UFC_OK                # but the timeouts may
    for ns in (0, 2, 3, 5, 6):                                                         # 3 connections
        assert call(**dict(args, n_slots=ns)) == UFC_ERR_INVALID_ARG, ns
    assert call(**dict(args, n=2**31 - 1)) == UFC_ERR_INVALID_ARG
    assert call(**dict(args, n_conns=2**31 - 3, n_slots=2**31)) == UFC_ERR_INVALID_ARG
    # n == 0: the frame arrays may be NULL, the connection arrays may not
    none = dict(infos=None, addrs=None, offsets=None, route=None, cls=None, order=None, infos_out=None,
                src_base_out=None)
    assert call(**dict(args, n=0, **none)) == UFC_OK
    assert call(**dict(args, n=0, results=None, **none)) == UFC_ERR_INVALID_ARG
    # no connections: the connection arrays may be NULL
    assert call(**dict(args, n_conns=0, n_slots=1, conn_active=None, timeout_in=None, results=None,
                       timeout_out=None)) == UFC_OK
    return keep


def test_argument_contract():
    argument_contract(lambda **a: lib().ufc_route_frames_host(*a.values(), 1))


def test_wrapper_refuses_bad_arrays():
    c = scenario_random(41, 6, 3)
    n = 6
    for arg, good in (("infos_out", np.zeros(n, fr.FRAME_INFO_DTYPE)), ("src_base_out", np.zeros(n, U64)),
                      ("timeout_out", np.zeros(3, U64))):
        ro = good.copy()
        ro.flags.writeable = False
        for what, value in (("dtype", np.zeros(good.size, "<i2")), ("short", good[:-1].copy()), ("read-only", ro),
                            ("strided", np.zeros(2 * good.size, good.dtype)[::2])):
            with pytest.raises(ValueError) as e:
                c.call(**{arg: value})
            assert arg in str(e.value), (arg, what)
    for arg in ("addrs", "offsets", "active", "tin"):
        bad = Case(c.infos, c.addrs, c.table, c.active, c.offsets, tin=c.tin)
        setattr(bad, arg, getattr(bad, arg)[:-1].copy())
        with pytest.raises(ValueError):
            bad.call()


# ---- the header against the binding ----

def test_route_records_match_the_header(tmp_path):
    """ROUTE_RECORDS against sizeof / offsetof compiled from the header (C99, -pedantic, through uflow_frame_codec.h,
    which brings the header along); uflow_amd.route exports the dtypes; no struct of the header is left out."""
    import os
    import re
    from test_records_cpu import INCLUDE, _header_layout
    from uflow_amd.records import FLUSH_RECORDS, RECORDS, ROUTE_RECORDS
    assert len(ROUTE_RECORDS) == 3 and not set(ROUTE_RECORDS) & (set(RECORDS) | set(FLUSH_RECORDS))
    assert [dt.itemsize for dt in ROUTE_RECORDS.values()] == [32, 48, 16]
    for struct, dt in ROUTE_RECORDS.items():
        assert getattr(rt, struct[len("ufc_"):].upper() + "_DTYPE") is dt
    got = _header_layout(tmp_path, {s: dt.names for s, dt in ROUTE_RECORDS.items()})
    want = {}
    for struct, dt in ROUTE_RECORDS.items():
        want["S", struct] = (dt.itemsize,)
        for f in dt.names:
            want["F", f"{struct}.{f}"] = (dt.fields[f][1], dt.fields[f][0].itemsize)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    with open(os.path.join(INCLUDE, "uflow_route.h")) as f:
        text = f.read()
    assert set(re.findall(r"^\} (ufc_\w+);", text, flags=re.M)) == set(ROUTE_RECORDS)
    consts = dict(re.findall(r"#define\s+(UFC_ROUTE_\w+)\s+(\d+)", text))
    assert len(consts) == 4
    for name, value in consts.items():
        assert getattr(rt, name[len("UFC_"):]) == int(value) == getattr(E, name[len("UFC_ROUTE_"):]), name
    with open(os.path.join(INCLUDE, "uflow_frame_codec.h")) as f:
        assert '#include "uflow_route.h"' in f.read()


def test_route_signatures_match_the_header():
    """Every prototype of the header against _native._ROUTE_SIGNATURES (parameter count, pointer-ness by position),
    and the library exports each."""
    import os
    import re
    from test_records_cpu import INCLUDE
    from uflow_amd import _native
    with open(os.path.join(INCLUDE, "uflow_route.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = {name: [p.strip() for p in params.split(",")]
              for name, params in re.findall(r"\b(ufc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert set(protos) == set(_native._ROUTE_SIGNATURES) == set(_native.ROUTE_SYMBOLS) and len(protos) == 3
    assert not set(protos) & (set(_native.SYMBOLS) | set(_native.FLUSH_SYMBOLS))
    pointer_types = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, (_, argtypes) in _native._ROUTE_SIGNATURES.items():
        assert hasattr(raw, name) and getattr(lib(), name).argtypes == argtypes, name
        assert len(protos[name]) == len(argtypes), (name, len(protos[name]), len(argtypes))
        for k, (p, t) in enumerate(zip(protos[name], argtypes)):
            assert ("*" in p) == issubclass(t, pointer_types), (name, k, p, t)
            if "*" not in p:      # the scalars by width: size_t, uint32_t, uint64_t, int
                width = {"size_t": ctypes.sizeof(ctypes.c_size_t), "uint32_t": 4, "uint64_t": 8, "int": 4}[p.split()[0]]
                assert ctypes.sizeof(t) == width, (name, k, p, t)


# ---- the routed batch through the stages behind it ----

def chained_traffic(seed=7, n_conns=5, packets=14):
    """Real frames of n_conns senders, built on the host, and an arrival order that interleaves the connections
    (every connection's own frames stay in order).  Returns (wire, off) in grouped order, the owner of every frame
    in arrival order and the arrival order as indices into the grouped frames."""
    rng = np.random.default_rng(seed)
    arena = RX.PayloadArena(rng)
    lists = []
    for c in range(n_conns):
        s = RX.GenSender(100 * c + 5)
        dgs = []
        for k in range(packets + c):
            dgs += s.packet(int(rng.integers(0, 3)), bool(k % 3 == 0), bytes(rng.integers(0, 256, int(rng.integers(1, 60)),
                                                                                          dtype=U8)))
        lists.append(RX.datagram_items(arena, dgs))
    infos, items, ff = RX.frames_of(lists, per_frame=3)
    for c in range(n_conns):                     # sequence ids and nonces, per connection
        lo, hi = int(ff[c]), int(ff[c + 1])
        infos["f"][lo:hi, 0] = 1000 * c + np.arange(hi - lo)
        infos["aux"][lo:hi] = rng.integers(0, 2, hi - lo)
    wire, off, status, _ = fr.build_batch_host(infos, items, arena.array())
    assert not status.any()
    owner_grouped = np.repeat(np.arange(n_conns), np.diff(ff.astype(np.int64)))
    owner = owner_grouped[rng.permutation(owner_grouped.size)]      # who sends the i-th arriving frame
    nxt = ff[:-1].astype(np.int64).copy()
    arrive = np.zeros(owner.size, dtype=np.int64)
    for i, c in enumerate(owner):
        arrive[i] = nxt[c]
        nxt[c] += 1
    return wire, off.astype(np.int64), owner, arrive


def reorder(wire, off, idx):
    lens = (off[1:] - off[:-1])[idx]
    off2 = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    return np.concatenate([wire[off[g]:off[g + 1]] for g in idx]), off2


def stages(infos, items, wire, frame_first, src_base, n_conns, window_call, receive_call):
    """The frame window and the packet receive over a grouped batch, from fresh state."""
    windows = fr.new_frame_windows(n_conns, 4096, (1000 * np.arange(n_conns)).astype(U32))
    fw = window_call(infos, frame_first, windows)
    receivers = fr.new_receivers(n_conns, 64, (100 * np.arange(n_conns) + 5).astype(U32))
    slots = np.zeros(n_conns * 64, dtype=fr.RX_SLOT_DTYPE)
    rx = receive_call(infos, items, wire, frame_first, receivers, slots, np.arange(n_conns + 1, dtype=U64) * U64(64),
                      np.zeros(0, U8), src_base=src_base, frame_accept=fw["frame_accept"])
    return fw, rx


def test_routed_batch_through_window_and_receive():
    """An interleaved batch, parsed in arrival order and routed, against the same frames grouped beforehand by a
    stable argsort and parsed in grouped order: the frame window and the receive give the same bytes."""
    n_conns = 5
    wire, off, owner, arrive = chained_traffic(n_conns=n_conns)
    conn = rt.addr_records([v4(50 + c, 6000 + c) for c in range(n_conns)])
    table = rt.new_route_table(conn, 424242)
    # arrival order: parse, route, stages
    wire_a, off_a = reorder(wire, off, arrive)
    infos_a, items_a = fr.parse_batch_host(wire_a, off_a)
    assert infos_a["ok"].all() and (infos_a["kind"] == DATA).all()
    r = route_call(infos_a, conn[owner], off_a[:-1].copy(), table, np.ones(n_conns, U8), 10, 20, np.zeros(n_conns, U64))
    assert (r["cls"] == E.CONN).all() and r["bucket_first"][n_conns] == owner.size
    ff_r = r["bucket_first"][:n_conns + 1].copy()
    fw_r, rx_r = stages(r["infos_out"], items_a, wire_a, ff_r, r["src_base_out"], n_conns, fr.frame_window_host,
                        fr.receive_packets_host)
    # grouped beforehand
    grouped = np.argsort(owner, kind="stable")
    assert r["order"].tolist() == grouped.tolist()
    wire_g, off_g = reorder(wire_a, off_a.astype(np.int64), grouped)
    infos_g, items_g = fr.parse_batch_host(wire_g, off_g)
    ff_g = np.searchsorted(owner[grouped], np.arange(n_conns + 1)).astype(U64)
    assert ff_g.tobytes() == ff_r.tobytes()
    fw_g, rx_g = stages(infos_g, items_g, wire_g, ff_g, off_g[:-1].copy(), n_conns, fr.frame_window_host,
                        fr.receive_packets_host)
    compare_stages(fw_r, rx_r, r["infos_out"], fw_g, rx_g, infos_g)
    assert rx_r["packets_used"] > 0 and rx_r["out_used"] > 0 and fw_r["frame_accept"].all()


def compare_stages(fw_r, rx_r, infos_r, fw_g, rx_g, infos_g):
    for k in ("frame_accept", "groups", "group_first", "results", "windows_out"):
        assert np.asarray(fw_r[k]).tobytes() == np.asarray(fw_g[k]).tobytes(), k
    for k in ("packets", "packet_first", "out_bytes", "carry_out", "carry_first", "results", "receivers_out"):
        assert np.asarray(rx_r[k]).tobytes() == np.asarray(rx_g[k]).tobytes(), k
    for k in ("packets_used", "out_used", "carry_used"):
        assert int(rx_r[k]) == int(rx_g[k]), k
    # the items stay where their parse left them: the statuses agree frame by frame
    for a, b in zip(infos_r, infos_g):
        assert a["item_count"] == b["item_count"]
        sa = rx_r["item_status"][int(a["item_first"]):int(a["item_first"]) + int(a["item_count"])]
        sb = rx_g["item_status"][int(b["item_first"]):int(b["item_first"]) + int(b["item_count"])]
        assert sa.tobytes() == sb.tobytes()


# ---- the stand-alone host check ----

def test_route_core_under_sanitizers():
    """tests/c/route_host_check.hip: the host calls over seeded random batches, sane and arbitrary tables, as host
    code under AddressSanitizer and UBSan, against a plain sequential restatement inside the program, over exact-size
    buffers; a stand-alone program (nothing is loaded into Python under a sanitizer)."""
    import os
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, "c", "route_host_check.hip")
    codec = os.path.join(os.path.dirname(here), "uflow_amd", "csrc", "frame_codec.cpp")
    crc = os.path.join(os.path.dirname(here), "uflow_amd", "csrc", "crc_math.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "route_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, codec, crc, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
