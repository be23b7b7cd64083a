"""CPU: the batched host build (ufc_build_sizes_host + ufc_build_batch_host, uflow_amd.frame.build_batch_host)
against the codec oracle.  Expected bytes are always oracle/codec.py frame_write -- of the canonical form of
what frame_read decodes for a source frame, or of a constructed frame -- never the product's own encode,
and never the source bytes (Frame::read accepts non-canonical encodings that re-encode differently).
Records come from tests/parse_expect.oracle_records (tests/build_expect.py).  No GPU here."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import codec as C
from uflow_amd import _native
from uflow_amd.frame import build_batch_host

import build_expect as BE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _run_host(batch, seal, nthreads=1):
    infos, items, payload, src = batch.arrays()
    out, offsets, status, crc = build_batch_host(infos, items, payload, src, seal=seal, nthreads=nthreads)
    BE.check_output(batch, seal, out, offsets, status)
    return out, offsets, status, crc


@pytest.fixture(scope="module")
def parity_batch():
    frames = [C.frame_write(f) for _, f in C.reference_test_frames()]
    frames += BE.codec_frames(2024, 600)
    import random
    frames += [C.frame_write(C.receive_side_data_frame(random.Random(s))) for s in range(8)]
    b = BE.Batch().add_sources(frames)
    skipped = sum(1 for s in b.status if s == BE.SKIPPED)
    assert 100 < skipped < 300, skipped  # damaged, unsealed and truncated frames are in the mix
    return b


@pytest.mark.parametrize("seal", [0, 1])
def test_host_build_matches_oracle(parity_batch, seal):
    """Bytes, offsets and status of the host build over the reference's test frames, 600 seeded frames of
    every kind (damaged, unsealed and resealed ones among them) and receive_side_data_frame; SKIPPED exactly
    where the oracle's frame_read gives None; zero trailers with seal=0, the CRC with seal=1."""
    out, offsets, status, crc = _run_host(parity_batch, seal)
    if seal:
        for i, c in enumerate(parity_batch.crcs()):
            if c is not None:
                assert int(crc[i]) == c, i
    out2, offsets2, status2, _ = _run_host(parity_batch, seal, nthreads=4)
    assert np.array_equal(out, out2) and np.array_equal(offsets, offsets2)


def test_header_form_boundaries():
    """data_len 63/64/255/256/65535, window_parent_lead 127/128, channel_parent_lead 255/256,
    fragment_id_last 0/1 (a fragment_id under last == 0 is dropped with the micro and small forms, as the
    oracle does), 0/127/128 datagrams, 0/1/162/65535/65536 ack groups."""
    b = BE.boundary_batch()
    _run_host(b, 1)
    _run_host(b, 0)
    assert b.status.count(BE.BAD_FIELD) == 2  # 128 datagrams, 65536 ack groups


def test_status_on_bad_input():
    """Every BAD_FIELD rule, and BAD_SRC with a range ending at payload_len (fine) and one byte past it;
    the frames around a rejected frame still come out right."""
    b = BE.bad_input_batch()
    assert b.status.count(BE.BAD_SRC) == 2 and b.status.count(BE.BAD_FIELD) >= 11 and b.status.count(BE.SKIPPED) == 1
    _run_host(b, 1)
    _run_host(b, 0)


def test_host_write_skip_rule_and_arguments():
    """The write call alone: a span whose length disagrees with the frame's size is left untouched, its
    neighbours are written; n == 0 is fine whatever the pointers; missing pointers are refused."""
    import random
    rng = random.Random(5)
    b = BE.Batch()
    for k in range(5):
        b.add(BE.data_frame(rng, [BE.datagram(rng, k % 3, BE.rand_bytes(rng, 30 + k))]))
    infos, items, payload, src = b.arrays()
    exp, off, _ = b.expected(True)
    off = off.copy()
    off[3:] += 1  # frame 2's span one byte too long; the frames after it move along
    out = np.full(int(off[-1]) + 8, 0xA5, dtype=np.uint8)
    lib = _native.lib()
    rc = lib.ufc_build_batch_host(infos.ctypes.data, items.ctypes.data, items.size, src.ctypes.data, payload.ctypes.data,
                                  payload.size, infos.size, off.ctypes.data, out.ctypes.data, int(off[-1]), 1, None, 1)
    assert rc == 0
    eoff = b.expected(True)[1]
    for i in range(5):
        got = out[int(off[i]):int(off[i + 1])]
        if i == 2:
            assert (got == 0xA5).all()
        else:
            assert np.array_equal(got, exp[int(eoff[i]):int(eoff[i + 1])]), i
    assert (out[int(off[-1]):] == 0xA5).all()
    # a buffer that ends inside the last frame: that frame is not written
    out[:] = 0xA5
    rc = lib.ufc_build_batch_host(infos.ctypes.data, items.ctypes.data, items.size, src.ctypes.data, payload.ctypes.data,
                                  payload.size, infos.size, off.ctypes.data, out.ctypes.data, int(off[-1]) - 1, 1, None, 1)
    assert rc == 0 and (out[int(off[4]):] == 0xA5).all() and out[int(off[3])] == 10
    assert lib.ufc_build_batch_host(None, None, 0, None, None, 0, 0, None, None, 0, 1, None, 1) == 0
    assert lib.ufc_build_sizes_host(None, None, 0, None, 0, 0, None, None, 1) == 0
    assert lib.ufc_build_sizes_host(None, None, 0, None, 0, 1, off.ctypes.data, None, 1) == _native.UFC_ERR_INVALID_ARG
    assert lib.ufc_build_batch_host(infos.ctypes.data, None, items.size, None, None, 0, 1, off.ctypes.data,
                                    out.ctypes.data, out.size, 1, None, 1) == _native.UFC_ERR_INVALID_ARG


def _host_write(case, seal=0):
    infos, items, payload, src = case.arrays()
    off = case.given_offsets().astype(np.uint64)
    total = int(off.max())
    out = np.full(total + 64, BE.GUARD, dtype=np.uint8)
    rc = _native.lib().ufc_build_batch_host(infos.ctypes.data, items.ctypes.data, items.size, src.ctypes.data,
                                            payload.ctypes.data, payload.size, infos.size, off.ctypes.data,
                                            out.ctypes.data, total, seal, None, 1)
    assert rc == 0
    return out


@pytest.mark.parametrize("case", BE.table_cases(), ids=lambda c: c.name)
def test_table_cases(case):
    """The table-limit and caller-made-layout cases of build_expect.table_cases: the facts hold
    on the case's own records, the sizes call gives the oracle's sizes, and the host write gives the oracle's bytes
    at the caller's offsets with the guard bytes around them untouched.  With offsets that go backwards the host
    write keeps the documented bounds too (it writes every frame whose span has the frame's size, so where two
    spans overlap the later frame's bytes win)."""
    BE.check_table_facts(case)
    infos, items, payload, src = case.arrays()
    sizes = np.zeros(infos.size + 1, dtype=np.uint64)
    status = np.zeros(infos.size, dtype=np.uint8)
    assert _native.lib().ufc_build_sizes_host(infos.ctypes.data, items.ctypes.data, items.size, src.ctypes.data,
                                              payload.size, infos.size, sizes.ctypes.data, status.ctypes.data, 1) == 0
    assert (status == BE.OK).all()
    assert np.array_equal(sizes.astype(np.int64) + case.first_off, case.sizes())
    out = _host_write(case)
    if case.name == "offsets_backwards":
        BE.check_backward_output(case, out)
    else:
        assert np.array_equal(out, BE.expected_region(case, out.size))


def test_encode_core_under_sanitizers():
    """tests/c/build_host_check.hip: the encode core as host code under AddressSanitizer and UBSan, a
    stand-alone program (nothing is loaded into Python under a sanitizer)."""
    src = os.path.join(REPO, "tests", "c", "build_host_check.hip")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "build_host_check")
        san = "-fsanitize=address,undefined"
        cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", san,
               "-Xarch_host", "-fno-sanitize-recover=all", san, "-fno-gpu-sanitize", src, "-o", exe]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert r.stdout.startswith("ok:"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
