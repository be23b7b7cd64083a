"""The host-buffer entry points past one staging chunk, bit-exact against the oracle.

ufc_validate_host_varlen / ufc_validate_host_slots cut a batch into chunks of at most 64 MB or 2^20
frames that ping-pong over two staging slots and two streams; the seals run the same path.  The
cases (gate_expect.host_varlen_case / host_slots_case; their cuts are checked without a GPU by
test_gate_expect_cpu.py): a cut by frame count, a cut by bytes with h_offsets[0] = 7, a frame that
is a chunk of its own, staging that regrows between calls of either layout, one host output left
out, and both seals.
"""
import numpy as np
import pytest

import gate_expect as G
from uflow_amd import _native as N

pytestmark = pytest.mark.gpu


def _same(what, got, ref):
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, f"{what}: {bad.size} differ from the oracle, first at {bad[:8]}"


def _gate_varlen(engine, name):
    c = G.host_varlen_case(name)
    crc, valid = engine.validate_host_varlen(c.buf, c.off)
    _same(f"host varlen {name} crc", crc, c.ref_crc)
    _same(f"host varlen {name} valid", valid, c.ref_valid)


def _gate_slots(engine, name):
    c = G.host_slots_case(name)
    crc, valid = engine.validate_host_slots(c.slots, c.stride, c.lens)
    _same(f"host slots {name} crc", crc, c.ref_crc)
    _same(f"host slots {name} valid", valid, c.ref_valid)


@pytest.mark.parametrize("name", ("count", "bytes", "solo"))
def test_host_varlen_chunks(engine, name):
    assert len(G.varlen_cuts(G.host_varlen_case(name).off)) - 1 == 3
    _gate_varlen(engine, name)


@pytest.mark.parametrize("name", ("count", "bytes"))
def test_host_slots_chunks(engine, name):
    c = G.host_slots_case(name)
    assert len(G.slots_cuts(c.stride, c.n)) - 1 == 3
    _gate_slots(engine, name)


def test_host_staging_regrows(engine):
    """One chunk, three chunks of 64 MB, one chunk again, in either layout on the shared engine: the
    staging, offsets and result buffers of the two layouts are the same allocations."""
    for name in ("small", "bytes", "small"):
        _gate_varlen(engine, name)
    for name in ("small", "bytes", "small"):
        _gate_slots(engine, name)
    _gate_varlen(engine, "small")


@pytest.mark.parametrize("want", ("crc_only", "valid_only"))
@pytest.mark.parametrize("layout", ("varlen", "slots"))
def test_host_one_output_null(engine, layout, want):
    lib = N.lib()
    if layout == "varlen":
        c = G.host_varlen_case("count")
        args = (engine._ctx, c.buf.ctypes.data, c.off.ctypes.data, c.n)
        call = lib.ufc_validate_host_varlen
    else:
        c = G.host_slots_case("count")
        args = (engine._ctx, c.slots.ctypes.data, c.stride, c.lens.ctypes.data, c.n)
        call = lib.ufc_validate_host_slots
    if want == "crc_only":
        crc = np.full(c.n + 16, G.FILL32, dtype=np.uint32)
        N.check(call(*args, crc.ctypes.data, None), call.__name__)
        _same(f"host {layout} crc alone", crc[:c.n], c.ref_crc)
        assert (crc[c.n:] == G.FILL32).all()
    else:
        valid = np.full(c.n + 64, G.FILL8, dtype=np.uint8)
        N.check(call(*args, None, valid.ctypes.data), call.__name__)
        _same(f"host {layout} valid alone", valid[:c.n], c.ref_valid)
        assert (valid[c.n:] == G.FILL8).all()


def test_seal_host_varlen_chunks(engine):
    c = G.host_varlen_case("bytes")
    data = c.buf.copy()
    crc = engine.seal_host_varlen(data, c.off)
    _same("seal host varlen crc", crc, c.ref_crc)
    _same("seal host varlen bytes", data, c.sealed)


@pytest.mark.parametrize("name", ("count4", "bytes"))
def test_seal_host_slots_chunks(engine, name):
    c = G.host_slots_case(name)
    slots = c.slots.copy()
    crc = engine.seal_host_slots(slots, c.stride, c.lens)
    _same(f"seal host slots {name} crc", crc, c.ref_crc)
    # trailers as the oracle's; the bytes between a datagram's end and its slot's end unchanged
    _same(f"seal host slots {name} bytes", slots, c.sealed)
