"""The batches of tests/gate_expect.py reach the paths their GPU tests are about (no GPU needed).

Checked from the lengths alone: the deferral classes of every variable-length case, which kernel
takes every fixed shape, and into how many chunks every host batch is cut (the cut rules of
ufc_api.cpp restated in gate_expect.varlen_cuts / slots_cuts).  Checked with the oracle: between
20 % and 80 % of the frames of every gate case pass, so neither an all-0 nor an all-1 `valid` can.
(Fixed frames under 5 bytes cannot pass the gate at all: there the oracle rejects every frame.)
"""
import numpy as np
import pytest

import gate_expect as G


def _mixed(case, what):
    share = G.valid_share(case)
    assert 0.2 <= share <= 0.8, f"{what}: the oracle accepts {share:.3f} of the frames"


@pytest.mark.parametrize("lead", (0, 1, 2, 3, 4))
def test_guards_notice_a_stray_write(lead):
    import torch
    dtype, fill = (torch.int32, G.FILL32) if lead == 4 else (torch.uint8, G.FILL8)
    raw, view = G.guarded(10, dtype, fill, lead, device="cpu")
    assert raw.numel() == 64 + lead + 10 * view.element_size() + 64
    assert view.data_ptr() - raw.data_ptr() == 64 + lead
    assert (view.view(torch.uint8) == G.FILL8).all()
    view.zero_()
    G.check_guards(raw, view)
    end = 64 + lead + 10 * view.element_size()
    for stray in (0, 64 + lead - 1, end, raw.numel() - 1):
        raw[stray] = 0
        with pytest.raises(AssertionError):
            G.check_guards(raw, view)
        raw[stray] = G.FILL8
    G.check_guards(raw, view)


@pytest.mark.parametrize("name", sorted(G.VARLEN_NEED))
def test_varlen_case_classes_and_mix(name):
    c = G.varlen_case(name)
    got = G.classes(c.lens)
    need = G.VARLEN_NEED[name]
    for k, v in need.items():
        assert got[k] >= v, (name, got)
    if need["lt4"] == 0:
        assert got["lt4"] == 0  # seals get no frame without room for a trailer
    assert int(c.off[0]) == 0 and int(c.off[-1]) + G.LEAD + G.TAIL == c.buf.size
    assert c.ref_crc.size == c.n == c.ref_valid.size
    _mixed(c, name)
    assert not np.array_equal(c.sealed, c.buf)


def test_outputs_batch_shape():
    lens = G.outputs_lens()
    assert lens.size == 4099
    assert {70_000, 300_001} <= set(lens.tolist())
    assert set(range(1520, 1680)) <= set(lens.tolist())  # every length across the 13/14-line edge
    assert G.classes(lens)["edge"] >= 128
    assert G.outputs_lens(tiny=False).min() >= 4 and G.outputs_lens(tiny=False).size == 4099 - 300


def test_large_case_fills_every_cu():
    c = G.varlen_case("large")
    assert c.n == 64 * 16 * G.NCU_ASSUMED
    assert c.lens.mean() < 200
    a, b = G.varlen_case("stream_a"), G.varlen_case("stream_b")
    assert a.n != b.n or not np.array_equal(a.lens, b.lens)
    assert not np.array_equal(G.varlen_case("small_64").lens, G.varlen_case("small_200").lens[:64])


@pytest.mark.parametrize("kernel", G.FIXED_KERNELS)
def test_fixed_shapes_reach_their_kernel(kernel):
    shapes = G.fixed_shapes(kernel)
    assert shapes
    for L, stride, n in shapes:
        J = G.lean_blocks(L, stride, n)
        if kernel == "lean":
            assert J == {5: 1, 252: 1, 253: 2, 1472: 6, 1500: 6, 1532: 6}[L], (L, stride, n, J)
            assert n % 4 != 0  # a partial last set
        elif kernel == "generic_forced":
            assert J != 0      # the lean kernel's, unless UFC_FIXED_GENERIC is set
        elif (L, stride, n) == (4, 7, 67):
            assert J == 1      # 4-byte frames at stride 7: enough sets past the edge for the lean kernel
        else:
            assert J == 0, (L, stride, n, J)
    assert {s[0] for s in G.fixed_shapes("generic_lens", min_len=4)} == {4, 1533, 3000, 8192}


@pytest.mark.parametrize("kernel", G.FIXED_KERNELS)
def test_fixed_cases_mix(kernel):
    for L, stride, n in G.fixed_shapes(kernel):
        c = G.fixed_case(L, stride, n)
        assert c.buf.size == G.LEAD + (n - 1) * stride + L + G.TAIL
        if L >= 5:
            _mixed(c, (L, stride, n))
        else:
            assert not c.ref_valid.any()
        if L >= 4:
            d = np.nonzero(c.sealed != c.buf)[0] - G.LEAD
            assert d.size and ((d % stride >= L - 4) & (d % stride < L)).all()  # trailers only


def test_cut_rules():
    off = np.array([7, 7, 7 + G.CHUNK_BYTES, 8 + G.CHUNK_BYTES, 9 + 2 * G.CHUNK_BYTES + 5], dtype=np.uint64)
    assert G.varlen_cuts(off) == [0, 2, 3, 4]  # exactly 64 MB fits; a longer frame goes alone
    assert G.varlen_cuts(np.arange(G.CHUNK_FRAMES + 2, dtype=np.uint64)) == [0, G.CHUNK_FRAMES, G.CHUNK_FRAMES + 1]
    assert G.slots_cuts(1472, 2 * 45590 + 1) == [0, 45590, 91180, 91181]
    assert G.slots_cuts(8, 5) == [0, 5]
    assert G.slots_cuts(128 << 20, 3) == [0, 1, 2, 3]


@pytest.mark.parametrize("name", G.HOST_VARLEN)
def test_host_varlen_case_chunks(name):
    c = G.host_varlen_case(name)
    cuts = G.varlen_cuts(c.off)
    assert len(cuts) - 1 == G.HOST_VARLEN_CHUNKS[name], cuts
    sizes = np.diff(cuts)
    nbytes = np.diff(c.off[cuts].astype(np.int64))
    if name == "count":
        assert sizes.tolist() == [G.CHUNK_FRAMES, G.CHUNK_FRAMES, 5] and nbytes.max() < G.CHUNK_BYTES
    elif name == "bytes":
        assert int(c.off[0]) == 7 and sizes.max() < G.CHUNK_FRAMES
        assert nbytes[0] > G.CHUNK_BYTES - 1472 and nbytes[1] > G.CHUNK_BYTES - 1472 and 0 < nbytes[2] < 3 * 1472
        assert not np.array_equal(c.sealed, c.buf)
    elif name == "solo":
        assert sizes.tolist() == [200, 1, 200] and nbytes[1] == 70 << 20 > G.CHUNK_BYTES
    _mixed(c, name)


@pytest.mark.parametrize("name", G.HOST_SLOTS)
def test_host_slots_case_chunks(name):
    c = G.host_slots_case(name)
    stride, n, lo, _, chunks = G.HOST_SLOTS_SHAPE[name]
    cuts = G.slots_cuts(stride, n)
    assert len(cuts) - 1 == chunks and c.slots.size == n * stride
    assert lo <= int(c.lens.min()) and int(c.lens.max()) <= stride
    if n > 100_000:
        assert int(c.lens.min()) == lo and int(c.lens.max()) == stride  # an empty and a full slot
    if name.startswith("count"):
        assert np.diff(cuts).tolist() == [G.CHUNK_FRAMES, G.CHUNK_FRAMES, 5]
    if name == "bytes":
        assert np.diff(cuts).max() * stride <= G.CHUNK_BYTES < (np.diff(cuts).max() + 1) * stride
    _mixed(c, name)
    if c.sealed is not None:
        # the seal changes trailers only: the bytes between a datagram's end and its slot's end stay
        d = np.nonzero(c.sealed != c.slots)[0]
        i, o = d // stride, d % stride
        assert d.size and ((o >= c.lens[i] - 4) & (o < c.lens[i])).all()
