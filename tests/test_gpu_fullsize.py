"""GPU parity at BASELINE.json's full sizes, every frame compared bit-exact with the CPU oracle
(oracle/crc_oracle.c: crc.rs:94-104 and the gate of serial/mod.rs:675-690), plus the committed
golden fixtures run straight through the HIP path.

  config 2   1M x 1500-B frames generated on the host, sealed by the oracle, one bit flipped in
             every 1000th frame; the GPU gate vs the oracle; the GPU seal of the zero-trailer
             frames vs the oracle's seal (byte-identical batch).
  config 3   10M frames, lengths U[64,1500] (seed 0x5EED0002), sealed by the GPU, every 997th
             frame flipped; the oracle re-validates every frame (so it checks the GPU seal too) and
             its CRC words must equal the GPU gate's.
  config 4   one GPU's shard of the 100M-frame batch: frames [37.5M, 50M) (rank 3 of 8) of seed
             0x5EED0003, 18.75 GB, sealed on the GPU, every 1000th frame flipped; as config 3.
  parse      the parse workload of tools/bench_configs.py (1M uflow frames, 14.5M items), every
             info and item vs the native host parse (itself pinned to the codec oracle on CPU).
The oracle runs multithreaded over the whole batch (16 threads: the GPU box's CPU share).
"""
import json
import os

import numpy as np
import pytest
import torch

import oracle
from uflow_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
THREADS = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _host(t):
    return t.cpu().numpy()


def _compare(crc_d, valid_d, ref_crc, ref_valid, what):
    got_crc = _host(crc_d).view(np.uint32)
    got_valid = _host(valid_d)
    bad = np.nonzero(got_crc != ref_crc)[0]
    assert bad.size == 0, f"{what}: {bad.size} CRC mismatches, first frames {bad[:8]}"
    bad = np.nonzero(got_valid != ref_valid)[0]
    assert bad.size == 0, f"{what}: {bad.size} valid-flag mismatches, first frames {bad[:8]}"


def test_config2_full_batch(engine):
    n, L = 1_000_000, 1500
    rng = np.random.default_rng(synth.SEED_CONFIG2)
    host = rng.integers(0, 256, size=n * L, dtype=np.uint8)
    zero_trailers = host.copy()
    zero_trailers.reshape(n, L)[:, L - 4:] = 0
    oracle.seal_fixed_mt(host, L, L, n, THREADS)
    flipped = np.arange(0, n, 1000)
    host[flipped * L + 17] ^= 0x04
    ref_crc, ref_valid = oracle.validate_fixed_mt(host, L, L, n, THREADS)
    assert int(ref_valid.sum()) == n - flipped.size
    d = torch.from_numpy(host).to(DEV)
    crc, valid = engine.crc_fixed(d, L, n=n)
    torch.cuda.synchronize()
    _compare(crc, valid, ref_crc, ref_valid, "config 2 gate")
    # the encode side: GPU seal of the zero-trailer batch == the oracle's seal, byte for byte
    host[flipped * L + 17] ^= 0x04
    z = torch.from_numpy(zero_trailers).to(DEV)
    crc_out = torch.empty(n, dtype=torch.int32, device=DEV)
    engine.seal_fixed(z, L, n=n, crc_out=crc_out)
    torch.cuda.synchronize()
    assert torch.equal(z, torch.from_numpy(host).to(DEV)), "config 2 seal differs from the oracle's"
    assert np.array_equal(_host(crc_out).view(np.uint32),
                          oracle.validate_fixed_mt(host, L, L, n, THREADS)[0])


def test_config3_full_batch(engine):
    n = 10_000_000
    data, offsets = synth.varlen_batch(n, 64, 1500, synth.SEED_CONFIG3, device=DEV)
    engine.seal_varlen(data, offsets)
    flipped = torch.arange(0, n, 997, device=DEV)
    synth.flip_bits(data, offsets[flipped], byte_in_frame=7, mask=0x20)
    crc, valid = engine.crc_varlen(data, offsets)
    torch.cuda.synchronize()
    h_data, h_off = _host(data), _host(offsets).astype(np.uint64)
    ref_crc, ref_valid = oracle.validate_varlen_mt(h_data, h_off, THREADS)
    expect = np.ones(n, np.uint8)
    expect[_host(flipped)] = 0
    assert np.array_equal(ref_valid, expect), "the GPU seal left frames the oracle rejects"
    _compare(crc, valid, ref_crc, ref_valid, "config 3 gate")


def test_config4_shard_full(engine):
    world, rank, total, L = 8, 3, 100_000_000, 1500
    lo, hi = total * rank // world, total * (rank + 1) // world
    n = hi - lo
    frames = synth.fixed_frames(n, L, synth.SEED_CONFIG4, first_frame=lo, device=DEV)
    engine.seal_fixed(frames, L, n=n)
    flipped = torch.arange(0, n, 1000, device=DEV)
    synth.flip_bits(frames, flipped * L)
    crc, valid = engine.crc_fixed(frames, L, n=n)
    torch.cuda.synchronize()
    host = _host(frames)
    del frames
    torch.cuda.empty_cache()
    ref_crc, ref_valid = oracle.validate_fixed_mt(host, L, L, n, THREADS)
    expect = np.ones(n, np.uint8)
    expect[_host(flipped)] = 0
    assert np.array_equal(ref_valid, expect), "the GPU seal left frames the oracle rejects"
    _compare(crc, valid, ref_crc, ref_valid, "config 4 shard gate")


# ---- the committed golden fixtures, straight through the HIP path ----

def _csr(frames):
    offsets = np.zeros(len(frames) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(f) for f in frames])
    return np.frombuffer(b"".join(frames), dtype=np.uint8).copy(), offsets


def _gpu_varlen(engine, data, offsets):
    crc, valid = engine.crc_varlen(torch.from_numpy(data).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV))
    torch.cuda.synchronize()
    return _host(crc).view(np.uint32), _host(valid)


def _gpu_seal_varlen(engine, data, offsets):
    d = torch.from_numpy(data.copy()).to(DEV)
    crc_out = torch.empty(offsets.size - 1, dtype=torch.int32, device=DEV)
    engine.seal_varlen(d, torch.from_numpy(offsets.astype(np.int64)).to(DEV), crc_out=crc_out)
    torch.cuda.synchronize()
    return _host(d), _host(crc_out).view(np.uint32)


def test_golden_random_frames_fixture(engine):
    """tests/golden/random_frames.npz: 120 frames of 0..1600 B, every 7th bit-flipped."""
    z = np.load(os.path.join(GOLDEN, "random_frames.npz"))
    crc, valid = _gpu_varlen(engine, z["data"], z["offsets"])
    assert np.array_equal(crc, z["crc"])
    assert np.array_equal(valid, z["valid"])


def test_golden_crc_ramp_fixture(engine):
    """tests/golden/crc_lengths.json: crc(bytes(i % 256 for i in range(n))) for n = 0..300 and the
    constant patterns, as frames body + BE trailer: the GPU gate returns the fixture CRC and accepts
    every frame of >= 5 bytes; the GPU seal of the zero-trailer frames writes the fixture CRC."""
    with open(os.path.join(GOLDEN, "crc_lengths.json")) as f:
        g = json.load(f)
    bodies = [(bytes(i % 256 for i in range(n)), int(c, 16)) for n, c in g["ramp"]]
    pat = g["patterns"]
    bodies += [(b"\x00" * 1500, int(pat["zeros_1500"], 16)), (b"\xff" * 1500, int(pat["ones_1500"], 16)),
               (b"\xa5" * 1472, int(pat["a5_1472"], 16)), (b"123456789", int(pat["ascii_123456789"], 16))]
    frames = [b + c.to_bytes(4, "big") for b, c in bodies]
    data, offsets = _csr(frames)
    crc, valid = _gpu_varlen(engine, data, offsets)
    assert [int(x) for x in crc] == [c for _, c in bodies]
    assert [int(v) for v in valid] == [1 if len(f) >= 5 else 0 for f in frames]
    zeroed = data.copy()
    for i in range(len(frames)):
        zeroed[offsets[i + 1] - 4:offsets[i + 1]] = 0
    sealed, seal_crc = _gpu_seal_varlen(engine, zeroed, offsets)
    assert np.array_equal(sealed, data)
    assert [int(x) for x in seal_crc] == [c for _, c in bodies]
    # the same bodies of one length as a fixed-stride batch (lean / generic fixed kernels)
    for n in (1, 5, 251, 252, 253, 300):
        fr = frames[n]
        batch = np.frombuffer(fr * 4099, dtype=np.uint8).copy()
        c, v = engine.crc_fixed(torch.from_numpy(batch).to(DEV), len(fr), n=4099)
        torch.cuda.synchronize()
        assert set(_host(c).view(np.uint32).tolist()) == {bodies[n][1]}
        assert set(_host(v).tolist()) == {1 if len(fr) >= 5 else 0}


def test_golden_reference_frames_fixture(engine):
    """tests/golden/frames.json: the reference tests' fixed-value frames (serial/mod.rs:760-925),
    gated and sealed on the GPU; their truncations (serial/mod.rs:751-758) and one extra byte
    (:738-749) are rejected."""
    with open(os.path.join(GOLDEN, "frames.json")) as f:
        fx = json.load(f)["frames"]
    frames = [bytes.fromhex(x["hex"]) for x in fx]
    data, offsets = _csr(frames)
    crc, valid = _gpu_varlen(engine, data, offsets)
    assert [int(c) for c in crc] == [int(x["crc"], 16) for x in fx]
    assert valid.tolist() == [x["valid"] for x in fx]
    zeroed = data.copy()
    for i in range(len(frames)):
        zeroed[offsets[i + 1] - 4:offsets[i + 1]] = 0
    sealed, _ = _gpu_seal_varlen(engine, zeroed, offsets)
    assert np.array_equal(sealed, data)
    bad = [fr[:k] for fr in frames for k in range(len(fr))] + [fr + b"\x00" for fr in frames]
    d2, o2 = _csr(bad)
    _, v2 = _gpu_varlen(engine, d2, o2)
    assert not v2.any()


def _parse_workload_base(mtu):
    """tools/bench_configs.py's parse workloads: 600 distinct frames from the codec oracle (mtu: each data
    frame cut to the datagrams that fit MAX_FRAME_SIZE)."""
    import random
    from oracle import codec as C
    rng = random.Random(5)

    def fit(fr):
        while mtu and fr["kind"] == "data" and fr["datagrams"] and len(C.frame_write(fr)) > C.MAX_FRAME_SIZE:
            fr["datagrams"].pop()
        return C.frame_write(fr)
    return [fit(C.random_data_frame(rng) if i % 3 == 0 else C.receive_side_data_frame(rng)
                if i % 3 == 1 else C.random_ack_frame(rng, 20)) for i in range(600)]


@pytest.mark.parametrize("mtu", [False, True], ids=["test_generators", "mtu"])
def test_parse_bench_workload_full(engine, mtu):
    """The parse workloads tools/bench_configs.py times (1M uflow frames: data frames with
    micro/small/large datagrams, receive-side data frames and ack frames, 600 distinct frames from the
    codec oracle tiled; 1.41 GB, or 0.60 GB with every frame <= MAX_FRAME_SIZE), with one bit flipped in
    every 997th frame: the GPU gate + GPU parse against the codec oracle.  The 600
    distinct frames are decoded by oracle/codec.py frame_read and laid out as the C ABI's records; the
    1M frames' expected infos and items are those records expanded over the tiling (a flipped frame:
    not ok, no items), and every info and every item of the GPU output is compared with them."""
    import parse_expect
    from uflow_amd.frame import FRAME_INFO_DTYPE, ITEM_DTYPE
    from uflow_amd.batch import records
    n = 1_000_000
    base = _parse_workload_base(mtu)
    lens = np.array([len(base[i % 600]) for i in range(n)], dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lens)
    blob = np.frombuffer(b"".join(base), dtype=np.uint8)
    data = np.concatenate([blob] * (n // 600 + 1))[: int(offsets[-1])].copy()
    flipped = np.arange(0, n, 997)
    data[offsets[flipped] + (lens[flipped] // 2)] ^= 0x10
    d = torch.from_numpy(data).to(DEV)
    o = torch.from_numpy(offsets).to(DEV)
    _, valid = engine.crc_varlen(d, o)
    infos, items, used = engine.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    k = int(used.cpu()[0])
    got_infos = records(infos, FRAME_INFO_DTYPE)
    got_items = records(items[:k], ITEM_DTYPE)
    b_infos, b_items = parse_expect.oracle_records(base)
    assert b_infos["ok"].all()
    dead = np.zeros(n, dtype=bool)
    dead[flipped] = True
    exp_infos, exp_items = parse_expect.tile_records(b_infos, b_items, np.arange(n) % 600, dead)
    assert int(got_infos["crc_ok"].sum()) == n - flipped.size
    assert k == exp_items.size and k > (11_000_000 if mtu else 14_000_000), k
    parse_expect.compare(got_infos, got_items, exp_infos, exp_items)


def test_parse_datagram_validity_flags(engine):
    """The GPU parse's UFC_ITEM_VALID flags == datagram_is_valid (packet_receiver/mod.rs:12-30) of
    the oracle's decode, on datagrams covering every branch of the check."""
    import random
    from oracle import codec as C
    from uflow_amd.frame import FRAME_INFO_DTYPE, ITEM_DTYPE
    from uflow_amd.batch import records
    rng = random.Random(4321)
    frames = [C.frame_write(C.receive_side_data_frame(rng)) for _ in range(3000)]
    data, offsets = _csr(frames)
    d = torch.from_numpy(data).to(DEV)
    o = torch.from_numpy(offsets).to(DEV)
    _, valid = engine.crc_varlen(d, o)
    infos, items, used = engine.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    infos = records(infos, FRAME_INFO_DTYPE)
    items = records(items, ITEM_DTYPE)
    k = 0
    counts = {True: 0, False: 0}
    for i, fb in enumerate(frames):
        ref = C.frame_read(fb)
        assert infos[i]["ok"] == 1 and int(infos[i]["item_first"]) == k
        for it, dg in zip(items[k:k + int(infos[i]["item_count"])], ref["datagrams"]):
            want = C.datagram_is_valid(dg)
            assert bool(it["flags"] & 1) == want, (i, dg)
            counts[want] += 1
        k += int(infos[i]["item_count"])
    assert int(_host(used)[0]) == k
    assert counts[True] > 1000 and counts[False] > 1000, counts


def test_varlen_claimed_runs_with_slow_sets(engine):
    """Many runs per wave (claimed from the workgroup's LDS counter, each sorted inside the kernel)
    with byte-path sets at every position of a run: 2M frames of 0..1700 B (frames over 1532 B,
    under 4 B and empty frames take the byte path, which re-sorts its run), a partial last run,
    every 101st frame flipped.  CSR, (start, end) pairs of the same frames in reverse order, and
    the seal, each against the oracle."""
    n = 2_000_003
    rng = np.random.default_rng(0x5EED00C1)
    lens = rng.integers(0, 1701, size=n).astype(np.uint64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    host = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    ref_sealed = host.copy()
    oracle.seal_varlen_mt(ref_sealed, off, THREADS)  # frames < 4 B are left alone
    d = torch.from_numpy(host).to(DEV)
    offs = torch.from_numpy(off.view(np.int64)).to(DEV)
    engine.seal_varlen(d, offs)
    torch.cuda.synchronize()
    assert torch.equal(d, torch.from_numpy(ref_sealed).to(DEV)), "seal differs from the oracle's"
    live = np.nonzero(lens > 0)[0]
    flipped = live[::101]
    ref_sealed[off[flipped] + (lens[flipped] - 1) // 2] ^= 0x40
    d = torch.from_numpy(ref_sealed).to(DEV)
    ref_crc, ref_valid = oracle.validate_varlen_mt(ref_sealed, off, THREADS)
    crc, valid = engine.crc_varlen(d, offs)
    torch.cuda.synchronize()
    _compare(crc, valid, ref_crc, ref_valid, "claimed runs, CSR")
    rev = np.arange(n - 1, -1, -1)
    pairs = np.stack([off[:-1][rev], off[1:][rev]], axis=1).astype(np.int64)
    crc, valid = engine.crc_pairs(d, torch.from_numpy(pairs).to(DEV))
    torch.cuda.synchronize()
    _compare(crc, valid, ref_crc[rev], ref_valid[rev], "claimed runs, pairs")


def test_parse_large_batch(engine):
    """A 4.32M-frame parse (the codec test batch tiled 7200 times, 16875 workgroups, 1.3 GB): every
    frame's info and every item against the codec oracle (the 600 distinct frames decoded by
    oracle/codec.py frame_read, expanded over the tiling), and against the native host parse gating
    on its own (valid = None: nothing of the GPU's output goes into the reference)."""
    import parse_expect
    from test_gpu_parity import _codec_batch
    from uflow_amd.frame import FRAME_INFO_DTYPE, ITEM_DTYPE, parse_batch_host
    from uflow_amd.batch import records
    frames, data, offsets = _codec_batch(10, 600)
    reps = 7200
    lens = np.diff(offsets)
    big = np.tile(data, reps)
    offs = np.zeros(len(lens) * reps + 1, dtype=np.int64)
    offs[1:] = np.cumsum(np.tile(lens, reps))
    n = offs.size - 1
    d = torch.from_numpy(big).to(DEV)
    o = torch.from_numpy(offs).to(DEV)
    _, valid = engine.crc_varlen(d, o)
    infos, items, used = engine.parse_varlen(d, o, valid)
    torch.cuda.synchronize()
    k = int(used.cpu()[0])
    got = records(infos, FRAME_INFO_DTYPE)
    got_items = records(items[:k], ITEM_DTYPE)
    b_infos, b_items = parse_expect.oracle_records(frames)
    exp_infos, exp_items = parse_expect.tile_records(b_infos, b_items, np.arange(n) % 600, np.zeros(n, dtype=bool))
    assert k == exp_items.size
    parse_expect.compare(got, got_items, exp_infos, exp_items)
    ref, ref_items = parse_batch_host(big, offs.astype(np.uint64), None, nthreads=THREADS)
    bad = np.nonzero((got.view(np.uint8).reshape(n, -1) != ref.view(np.uint8).reshape(n, -1)).any(1))[0]
    assert bad.size == 0, f"{bad.size} frame infos differ from the host parse, first frames {bad[:8]}"
    assert k == ref_items.size


def test_varlen_long_frames_deferred(engine):
    """Frames of 0..8192 B (the reference's test generators and crc_flips go up to 8192 B,
    serial/mod.rs:932-992, 1054-1080) and a few of 64 KiB - 1 MiB: the ones longer than the
    variable-length kernel's 13-line fast path are deferred by its byte path to the second launch
    (frame_crc_long8_kernel).  Every length near the 13/14-line edge at every start offset mod 128, a
    seal, CSR and reversed (start, end) pairs, each against the oracle, called back to back (the
    per-stream counts the second launch zeroes)."""
    rng = np.random.default_rng(0x5EED8192)
    edge = np.arange(1520, 1680)  # the 13/14-line edge (P = ceil((len + r + 4) / 128), r = (start - 4) mod 128)
    lens = np.concatenate([rng.integers(0, 8193, size=200_000), np.tile(edge, 130),
                           rng.integers(0, 64, size=20_000), np.array([65_536, 200_001, 1 << 20, 1533, 1532])])
    rng.shuffle(lens)
    lens = lens.astype(np.uint64)
    n = lens.size
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    host = rng.integers(0, 256, size=int(off[-1]) + 3, dtype=np.uint8)
    ref_sealed = host.copy()
    oracle.seal_varlen_mt(ref_sealed[: int(off[-1])], off, THREADS)
    d = torch.from_numpy(host).to(DEV)
    offs = torch.from_numpy(off.view(np.int64)).to(DEV)
    crc_s = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    engine.seal_varlen(d, offs, crc_out=crc_s)
    torch.cuda.synchronize()
    assert torch.equal(d, torch.from_numpy(ref_sealed).to(DEV)), "seal differs from the oracle's"
    live = np.nonzero(lens >= 5)[0]
    flipped = live[::7]
    ref_sealed[off[flipped] + (lens[flipped] - 1) // 2] ^= 0x04
    d = torch.from_numpy(ref_sealed).to(DEV)
    ref_crc, ref_valid = oracle.validate_varlen_mt(ref_sealed[: int(off[-1])], off, THREADS)
    for rep in range(3):
        crc, valid = engine.crc_varlen(d, offs)
        torch.cuda.synchronize()
        _compare(crc, valid, ref_crc, ref_valid, f"long frames, CSR, call {rep}")
    assert int(ref_valid.sum()) == live.size - flipped.size
    rev = np.arange(n - 1, -1, -1)
    pairs = np.stack([off[:-1][rev], off[1:][rev]], axis=1).astype(np.int64)
    crc, valid = engine.crc_pairs(d, torch.from_numpy(pairs).to(DEV))
    torch.cuda.synchronize()
    _compare(crc, valid, ref_crc[rev], ref_valid[rev], "long frames, pairs")
    got = _host(crc_s).view(np.uint32)  # the seal's CRC words: the CRC of each frame's first len - 4 bytes
    sealed_ok = lens >= 4
    ref_c, _ = oracle.validate_varlen_mt(host[: int(off[-1])], off, THREADS)
    assert np.array_equal(got[sealed_ok], ref_c[sealed_ok])
