"""The gates' and seals' output contract on the GPU, bit-exact against the oracle.

Every entry point runs with each output left out in turn (NULL, `want_crc` / `want_valid`), with
`crc_out` 4-aligned but not 16-aligned and `valid_out` at each byte alignment, both inside guard
bytes (gate_expect.guarded).  After a call the requested outputs equal the oracle's, no byte
outside them changed, and a gate left the whole frame buffer as uploaded; a seal changed the
trailers only (the whole buffer, stride gaps and slack included, equals the oracle's seal).

Frames start 3 bytes into a random buffer with 64 bytes behind the last one; shapes are the
smallest that reach each kernel (gate_expect.fixed_shapes, checked by test_gate_expect_cpu.py).
"""
import numpy as np
import pytest
import torch

import gate_expect as G
from uflow_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("crc", "valid", "both")
VLEADS = (0, 1, 2, 3)
CRC_LEAD = 4


def _outputs(n, mode, vlead):
    c = G.guarded(n, torch.int32, G.FILL32, CRC_LEAD, DEV) if mode != "valid" else (None, None)
    v = G.guarded(n, torch.uint8, G.FILL8, vlead, DEV) if mode != "crc" else (None, None)
    if c[1] is not None:
        assert c[1].data_ptr() % 16 == 4
    if v[1] is not None:
        assert v[1].data_ptr() % 4 == vlead
    return c, v


def _check_outputs(what, c, v, ref_crc, ref_valid):
    """The requested outputs against the oracle, and their guards."""
    torch.cuda.synchronize()
    for name, (raw, view), ref in (("crc", c, ref_crc), ("valid", v, ref_valid)):
        if view is None:
            continue
        got = view.cpu().numpy()
        got = got.view(np.uint32) if name == "crc" else got
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, f"{what}: {bad.size} {name} results differ from the oracle, first at {bad[:8]}"
        G.check_guards(raw, view, f"{what} {name}_out")


def _unchanged(what, dbuf, host):
    bad = np.nonzero(dbuf.cpu().numpy() != host)[0]
    assert bad.size == 0, f"{what}: the call changed {bad.size} bytes of the frame buffer, first at {bad[:8]}"


def _modes_kw(c, v):
    return dict(crc_out=c[1], valid_out=v[1], want_crc=c[1] is not None, want_valid=v[1] is not None)


class _option:
    """Set an engine option for a block and put its old value back."""

    def __init__(self, engine, opt, value):
        self.e, self.opt, self.value = engine, opt, value

    def __enter__(self):
        self.old = self.e.get_option(self.opt)
        self.e.set_option(self.opt, self.value)

    def __exit__(self, *exc):
        self.e.set_option(self.opt, self.old)


# ---- fixed-stride gate ----
@pytest.mark.parametrize("vlead", VLEADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", G.FIXED_KERNELS)
def test_fixed_gate(engine, kernel, mode, vlead):
    forced = kernel == "generic_forced"
    with _option(engine, N.UFC_OPT_FIXED_KERNEL, N.UFC_FIXED_GENERIC if forced else N.UFC_FIXED_AUTO):
        for L, stride, n in G.fixed_shapes(kernel):
            case = G.fixed_case(L, stride, n)
            what = f"fixed gate {kernel} len={L} stride={stride} n={n} {mode} vlead={vlead}"
            dbuf = G.to_device(case.buf, DEV)
            c, v = _outputs(n, mode, vlead)
            got = engine.crc_fixed(dbuf[G.LEAD:], L, stride, n, **_modes_kw(c, v))
            assert (got[0] is None) == (mode == "valid") and (got[1] is None) == (mode == "crc")
            _check_outputs(what, c, v, case.ref_crc, case.ref_valid)
            _unchanged(what, dbuf, case.buf)


# ---- fixed-stride seal ----
@pytest.mark.parametrize("with_crc", (False, True), ids=("crc_null", "crc_guarded"))
@pytest.mark.parametrize("seal_kernel", ("inline", "two_pass"))
@pytest.mark.parametrize("kernel", G.FIXED_KERNELS)
def test_fixed_seal(engine, kernel, seal_kernel, with_crc):
    forced = kernel == "generic_forced"
    seal_opt = N.UFC_SEAL_INLINE if seal_kernel == "inline" else N.UFC_SEAL_TWO_PASS
    with _option(engine, N.UFC_OPT_FIXED_KERNEL, N.UFC_FIXED_GENERIC if forced else N.UFC_FIXED_AUTO), \
            _option(engine, N.UFC_OPT_SEAL_KERNEL, seal_opt):
        for L, stride, n in G.fixed_shapes(kernel, min_len=4):
            case = G.fixed_case(L, stride, n)
            what = f"fixed seal {kernel}/{seal_kernel} len={L} stride={stride} n={n} crc_out={with_crc}"
            dbuf = G.to_device(case.buf, DEV)
            c = G.guarded(n, torch.int32, G.FILL32, CRC_LEAD, DEV) if with_crc else (None, None)
            engine.seal_fixed(dbuf[G.LEAD:], L, stride, n, crc_out=c[1])
            _check_outputs(what, c, (None, None), case.ref_crc, None)
            bad = np.nonzero(dbuf.cpu().numpy() != case.sealed)[0]
            assert bad.size == 0, f"{what}: {bad.size} bytes differ from the oracle's seal, first at {bad[:8]}"


# ---- variable-length gates ----
def _device_batch(case):
    dbuf = G.to_device(case.buf, DEV)
    doff = G.to_device(case.off.view(np.int64), DEV)
    assert dbuf[G.LEAD:].data_ptr() % 4 == 3
    return dbuf, doff


@pytest.mark.parametrize("vlead", VLEADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ("csr", "csr_generic", "pairs"))
def test_varlen_gate(engine, entry, mode, vlead):
    case = G.varlen_case("outputs")
    what = f"varlen gate {entry} {mode} vlead={vlead}"
    dbuf, doff = _device_batch(case)
    c, v = _outputs(case.n, mode, vlead)
    ref_crc, ref_valid = case.ref_crc, case.ref_valid
    generic = entry == "csr_generic"
    with _option(engine, N.UFC_OPT_VARLEN_KERNEL, N.UFC_VARLEN_GENERIC if generic else N.UFC_VARLEN_AUTO):
        if entry == "pairs":  # the same frames in reverse order
            pairs = np.stack([case.off[:-1], case.off[1:]], axis=1)[::-1].astype(np.int64)
            engine.crc_pairs(dbuf[G.LEAD:], G.to_device(np.ascontiguousarray(pairs), DEV), **_modes_kw(c, v))
            ref_crc, ref_valid = ref_crc[::-1], ref_valid[::-1]
        else:
            engine.crc_varlen(dbuf[G.LEAD:], doff, **_modes_kw(c, v))
        _check_outputs(what, c, v, ref_crc, ref_valid)
    _unchanged(what, dbuf, case.buf)


# ---- variable-length seal ----
@pytest.mark.parametrize("with_crc", (False, True), ids=("crc_null", "crc_guarded"))
@pytest.mark.parametrize("entry", ("csr", "csr_generic"))
def test_varlen_seal(engine, entry, with_crc):
    case = G.varlen_case("outputs_seal")
    what = f"varlen seal {entry} crc_out={with_crc}"
    dbuf, doff = _device_batch(case)
    c = G.guarded(case.n, torch.int32, G.FILL32, CRC_LEAD, DEV) if with_crc else (None, None)
    generic = entry == "csr_generic"
    with _option(engine, N.UFC_OPT_VARLEN_KERNEL, N.UFC_VARLEN_GENERIC if generic else N.UFC_VARLEN_AUTO):
        engine.seal_varlen(dbuf[G.LEAD:], doff, crc_out=c[1])
        _check_outputs(what, c, (None, None), case.ref_crc, None)
    bad = np.nonzero(dbuf.cpu().numpy() != case.sealed)[0]
    assert bad.size == 0, f"{what}: {bad.size} bytes differ from the oracle's seal, first at {bad[:8]}"
