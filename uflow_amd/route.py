"""The batched frame routing in host memory (include/uflow_route.h), beside uflow_amd.frame's stages:

    addr_records(pairs)                        <- SocketAddr values as 32-byte keys
    new_route_table(addrs, seed, n_slots)      <- the keys of Server.clients: HashMap<SocketAddr, ..>
                                                  (src/server/mod.rs:118)
    route_frames_host(infos, addrs, offsets, table, conn_active, now_ms, active_timeout_ms, timeout_in)
                                               <- the address lookup and dispatch of Server::handle_frames
                                                  (src/server/mod.rs:591-602 over :492-589; client/mod.rs:557-583)
    (device-resident: uflow_amd.batch.FrameCrcEngine.route_frames)

The wrappers go through frame.py's one marshalling path (_in, _inout, _p).  The stage has a module of its own
because its C declarations have a header of their own; tests/test_route_cpu.py holds its records, signatures and
argument checks to that header.
"""
import ipaddress
from typing import NamedTuple, Optional

import numpy as np

from ._native import check, lib
# The stage's constants without their prefix: each value is written once, in _native.
from ._native import (  # noqa: F401
    UFC_ERR_INVALID_ARG, UFC_NO_PARENT as NO_PARENT, UFC_ROUTE_CONN as ROUTE_CONN, UFC_ROUTE_CONTROL as ROUTE_CONTROL,
    UFC_ROUTE_DEFERRED as ROUTE_DEFERRED, UFC_ROUTE_DROP as ROUTE_DROP)
from .frame import _U8, _U32, _U64, _in, _inout, _p
from .records import ADDR_DTYPE, FRAME_INFO_DTYPE, ROUTE_RESULT_DTYPE, ROUTE_SLOT_DTYPE  # noqa: F401


class RouteTable(NamedTuple):
    """A built table: the slots (ROUTE_SLOT_DTYPE, plain data to upload) and the three scalars that go with them."""
    slots: np.ndarray
    seed: int
    max_probe: int
    n_conns: int


class DuplicateAddress(ValueError):
    """new_route_table met an address twice; `index` is the second occurrence."""

    def __init__(self, index):
        super().__init__(f"address {index} repeats an earlier one")
        self.index = index


def addr_records(pairs):
    """SocketAddr values as ADDR_DTYPE keys: (ip, port) pairs, and for V6 (ip, port, flowinfo, scope_id) tuples as
    Python's socket module gives them.  ip is a string or an ipaddress object; a V4 address takes ip[0..4), and a
    V4-mapped V6 address stays V6 (the two differ, as Rust's SocketAddr values do).  Everything unused is zero."""
    pairs = list(pairs)
    out = np.zeros(len(pairs), dtype=ADDR_DTYPE)
    for k, p in enumerate(pairs):
        ip = ipaddress.ip_address(p[0])
        if ip.version == 4 and len(p) != 2:
            raise ValueError(f"address {k}: a V4 address is an (ip, port) pair")
        if len(p) not in (2, 4):
            raise ValueError(f"address {k}: expected (ip, port) or (ip, port, flowinfo, scope_id)")
        raw = ip.packed
        out["ip"][k, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        out["port"][k] = p[1]
        out["family"][k] = ip.version
        if len(p) == 4:
            out["flowinfo"][k], out["scope_id"][k] = p[2], p[3]
    return out


def new_route_table(addrs: np.ndarray, seed: int, n_slots: Optional[int] = None) -> RouteTable:
    """ufc_route_table_build_host: connection c gets addrs[c] (ADDR_DTYPE).  seed is the caller's random number, kept
    from the peers: the table's guard against addresses chosen to collide.  n_slots (a power of two above the number
    of connections) defaults to the next power of two >= 2 * n_conns.  Raises DuplicateAddress for a repeated
    address."""
    addrs = _in("addrs", addrs, ADDR_DTYPE)
    n_conns = addrs.size
    if n_slots is None:
        n_slots = 1
        while n_slots < 2 * n_conns or n_slots <= n_conns:
            n_slots *= 2
    n_slots = int(n_slots)
    slots = np.zeros(max(n_slots, 0), dtype=ROUTE_SLOT_DTYPE)
    max_probe = np.zeros(1, dtype=np.uint32)
    dup = np.full(1, np.iinfo(np.uint64).max, dtype=np.uint64)
    rc = lib().ufc_route_table_build_host(_p(addrs), n_conns, int(seed) & 0xFFFFFFFF, _p(slots), n_slots,
                                          max_probe.ctypes.data, dup.ctypes.data)
    if rc == UFC_ERR_INVALID_ARG and dup[0] != np.iinfo(np.uint64).max:
        raise DuplicateAddress(int(dup[0]))
    check(rc, "ufc_route_table_build_host")
    return RouteTable(slots, int(seed) & 0xFFFFFFFF, int(max_probe[0]), n_conns)


def route_frames_host(infos: np.ndarray, addrs: np.ndarray, offsets: Optional[np.ndarray], table: RouteTable,
                      conn_active: np.ndarray, now_ms: int, active_timeout_ms: int, timeout_in: np.ndarray,
                      nthreads: int = 1, infos_out: Optional[np.ndarray] = None,
                      src_base_out: Optional[np.ndarray] = None, timeout_out: Optional[np.ndarray] = None):
    """ufc_route_frames_host: behind parse_batch_host, in front of frame_window_host.  infos (FRAME_INFO_DTYPE) in
    arrival order, addrs (ADDR_DTYPE) their source addresses, offsets (uint64, the parsed batch's CSR offsets or any
    per-frame src_base; None reads as all zero), table (new_route_table's, or any RouteTable), conn_active (uint8 per
    connection: State::Active), timeout_in (uint64 per connection).  Returns a dict: route (uint32, NO_PARENT for not
    found), cls (uint8, ROUTE_*), bucket_first (uint64[n_conns + 3]; its first n_conns + 1 entries are the stages'
    frame_first), order (uint32), infos_out and src_base_out (what the stages take as infos and src_base), results
    (ROUTE_RESULT_DTYPE), timeout_out (may be given as `timeout_in`), first_unknown_control."""
    infos = _in("infos", infos, FRAME_INFO_DTYPE)
    n = infos.size
    addrs = _in("addrs", addrs, ADDR_DTYPE, n)
    if offsets is not None:
        offsets = _in("offsets", offsets, _U64, n)
    slots = _in("slots", table.slots, ROUTE_SLOT_DTYPE)
    n_conns = int(table.n_conns)
    conn_active = _in("conn_active", conn_active, _U8, n_conns)
    timeout_in = _in("timeout_in", timeout_in, _U64, n_conns)
    infos_out = _inout("infos_out", infos_out, FRAME_INFO_DTYPE, n)
    src_base_out = _inout("src_base_out", src_base_out, _U64, n)
    timeout_out = _inout("timeout_out", timeout_out, _U64, n_conns)
    route, cls, order = np.zeros(n, dtype=_U32), np.zeros(n, dtype=_U8), np.zeros(n, dtype=_U32)
    bucket_first = np.zeros(n_conns + 3, dtype=_U64)
    results = np.zeros(n_conns, dtype=ROUTE_RESULT_DTYPE)
    fuc = np.zeros(1, dtype=_U32)
    check(lib().ufc_route_frames_host(_p(infos), _p(addrs), _p(offsets), n, _p(slots), slots.size, table.seed,
                                      table.max_probe, n_conns, _p(conn_active), int(now_ms) & (2**64 - 1),
                                      int(active_timeout_ms) & (2**64 - 1), _p(timeout_in), _p(route), _p(cls),
                                      _p(bucket_first), _p(order), _p(infos_out), _p(src_base_out), _p(results),
                                      _p(timeout_out), _p(fuc), nthreads), "ufc_route_frames_host")
    return {"route": route, "cls": cls, "bucket_first": bucket_first, "order": order, "infos_out": infos_out,
            "src_base_out": src_base_out, "results": results, "timeout_out": timeout_out,
            "first_unknown_control": int(fuc[0])}
