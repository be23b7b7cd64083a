"""Seeded batches and output guards shared by test_gpu_outputs.py, test_gpu_streams.py and
test_gpu_host_chunks.py (and checked without a GPU by test_gate_expect_cpu.py).  Not a test module.

Every batch is random bytes in which some frames carry the oracle's trailer (`seal_period` /
`seal_keep`: frames i with i % period < keep) and every fifth of those has one flipped bit, so the
oracle's gate accepts a part of the frames only: an all-0 or all-1 `valid` cannot pass.  The
expected CRC words and flags come from the oracle alone; a case is generated once per process and
its arrays are read-only.
"""
import functools
from types import SimpleNamespace

import numpy as np

import oracle

FILL8 = 0xA5
FILL32 = 0xA5A5A5A5
GUARD = 64           # bytes of pattern before and after a guarded output
LEAD, TAIL = 3, 64   # device batches: bytes before the first frame and after the last
NCU_ASSUMED = 256    # the CPU checks' CU count (the GPU tests take the device's)

# ---- deferral classes of the 8-lane variable-length kernel (frame_crc_varlen8.hip, slow_set) ----
# A frame goes to the second launch when len + r > 128 * 13 - 4 with r < 128 the frame's alignment:
# always at 1661 B and more, never at 1532 B and less.
NEVER_DEFERRED_MAX = 1532
ALWAYS_DEFERRED_MIN = 1661


def classes(lens):
    """Frames per deferral class: under 4 B (no trailer), 4..1532 B (fast path at any alignment),
    1533..1660 (depends on alignment), 1661 B and more (second launch at any alignment)."""
    lens = np.asarray(lens, dtype=np.int64)
    return {"lt4": int((lens < 4).sum()),
            "mid": int(((lens >= 4) & (lens <= NEVER_DEFERRED_MAX)).sum()),
            "edge": int(((lens > NEVER_DEFERRED_MAX) & (lens < ALWAYS_DEFERRED_MIN)).sum()),
            "ge1661": int((lens >= ALWAYS_DEFERRED_MIN).sum())}


# ---- the host entry points' chunk cuts, restated (ufc_api.cpp: validate_host_varlen_impl,
# validate_host_slots_impl) ----
CHUNK_BYTES = 64 << 20
CHUNK_FRAMES = 1 << 20


def varlen_cuts(off):
    """Frame-index boundaries of the chunks of a host CSR batch: a chunk takes frames while it
    holds fewer than 2^20 of them and at most 64 MB, and at least one frame."""
    off = np.asarray(off, dtype=np.uint64)
    n = off.size - 1
    cuts = [0]
    while cuts[-1] < n:
        a = cuts[-1]
        by_bytes = int(np.searchsorted(off, off[a] + np.uint64(CHUNK_BYTES), side="right")) - 1
        cuts.append(max(a + 1, min(by_bytes, a + CHUNK_FRAMES, n)))
    return cuts


def slots_cuts(stride, n):
    """Whole slots, at most 64 MB and 2^20 of them per chunk."""
    per = max(1, min(CHUNK_FRAMES, CHUNK_BYTES // stride))
    return list(range(0, n, per)) + [n]


# ---- guarded outputs ----
def guarded(n, dtype, fill, lead, device="cuda:0"):
    """(raw, view): a device tensor of 64 + lead + n * itemsize + 64 bytes holding the pattern and
    the view of its n elements of `dtype` at byte offset 64 + lead."""
    import torch
    item = torch.empty(0, dtype=dtype).element_size()
    assert fill == (FILL8 if item == 1 else FILL32)
    raw = torch.full((GUARD + lead + n * item + GUARD,), FILL8, dtype=torch.uint8, device=device)
    view = raw[GUARD + lead:GUARD + lead + n * item].view(dtype)
    assert view.data_ptr() == raw.data_ptr() + GUARD + lead and view.numel() == n
    return raw, view


def to_device(a, device="cuda:0"):
    """A device copy of a (read-only) numpy array."""
    import torch
    return torch.tensor(a, device=device)


def check_guards(raw, view, what=""):
    """Every byte of `raw` outside `view` still holds the pattern."""
    lo = view.data_ptr() - raw.data_ptr()
    hi = lo + view.numel() * view.element_size()
    h = raw.cpu().numpy()
    before = np.nonzero(h[:lo] != FILL8)[0]
    after = np.nonzero(h[hi:] != FILL8)[0]
    assert before.size == 0, f"{what}: wrote {lo - int(before[-1])} bytes before the output"
    assert after.size == 0, f"{what}: wrote {int(after[-1]) + 1} bytes past the output"


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return ns


def _mix(buf, sealed, start, lens, rng, period, keep):
    """Into random `buf`: the trailers of `sealed` (the same bytes sealed by the oracle) for frames
    i % period < keep of at least 4 bytes, then one flipped bit in every fifth of those."""
    n = lens.size
    idx = np.nonzero((np.arange(n) % period < keep) & (lens >= 4))[0]
    end = (start[idx] + lens[idx]).astype(np.int64)
    t = (end[:, None] - 4 + np.arange(4)[None, :]).ravel()
    buf[t] = sealed[t]
    flip = idx[4::5]
    pos = start[flip].astype(np.int64) + (rng.random(flip.size) * lens[flip]).astype(np.int64)
    buf[pos] ^= (1 << rng.integers(0, 8, size=flip.size)).astype(np.uint8)


# ---- fixed-stride batches ----
@functools.lru_cache(maxsize=None)
def fixed_case(frame_len, stride, n):
    """n frames of frame_len at `stride`, from byte LEAD of a random buffer with TAIL bytes after the
    last frame.  ref_crc / ref_valid: the oracle's gate; `sealed`: the oracle's seal of the buffer."""
    rng = np.random.default_rng([11, frame_len, stride, n])
    size = LEAD + (n - 1) * stride + frame_len + TAIL
    buf = rng.integers(0, 256, size=size, dtype=np.uint8)
    sealed = buf.copy()
    if frame_len >= 4:
        oracle.seal_fixed(sealed[LEAD:], stride, frame_len, n)
        start = LEAD + np.arange(n, dtype=np.int64) * stride
        _mix(buf, sealed, start, np.full(n, frame_len, dtype=np.int64), rng, 3, 1)
        sealed = buf.copy()
        oracle.seal_fixed(sealed[LEAD:], stride, frame_len, n)
    ref_crc, ref_valid = oracle.validate_fixed(buf[LEAD:], stride, frame_len, n)
    return _freeze(SimpleNamespace(buf=buf, sealed=sealed, frame_len=frame_len, stride=stride, n=n,
                                   ref_crc=ref_crc, ref_valid=ref_valid))


LEAN_LENS = (5, 252, 253, 1472, 1500, 1532)   # J = 1, 1, 2, 6, 6, 6 blocks of 256 B
LEAN_NS = (67, 1001, 4099)
GENERIC_LENS = (0, 3, 4, 1533, 3000, 8192)
GENERIC_NS = (5, 67)
FORCED_LENS = (64, 1500)
FORCED_N = 1001


def lean_blocks(frame_len, stride, n):
    """ufc_api.cpp lean_fixed_blocks with default options: J when the lean kernel takes the batch."""
    if frame_len < 4:
        return 0
    J = (frame_len + 4 + 255) // 256
    if J > 6 or stride >= 1 << 28:
        return 0
    pad = 256 * J - frame_len
    s_edge = (pad + 4 * stride - 1) // (4 * stride)
    return J if n // 4 > s_edge else 0


def fixed_shapes(kernel, min_len=0):
    """(frame_len, stride, n) of the fixed cases of one kernel group."""
    if kernel == "lean":
        g = [(L, L + x, n) for L in LEAN_LENS for x in (0, 3) for n in LEAN_NS]
    elif kernel == "generic_small_n":
        g = [(L, L + x, 3) for L in LEAN_LENS for x in (0, 3)]
    elif kernel == "generic_lens":
        g = [(L, L + x, n) for L in GENERIC_LENS for x in (0, 3) for n in GENERIC_NS]
    elif kernel == "generic_forced":
        g = [(L, L + x, FORCED_N) for L in FORCED_LENS for x in (0, 3)]
    else:
        raise KeyError(kernel)
    return [s for s in g if s[0] >= min_len]


FIXED_KERNELS = ("lean", "generic_small_n", "generic_lens", "generic_forced")


# ---- variable-length batches ----
def _varlen(lens, seed, base, tail, period=3, keep=1, want_sealed=True, mt=False):
    lens = np.asarray(lens, dtype=np.uint64)
    rng = np.random.default_rng(seed)
    off = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    off += np.uint64(base)
    buf = rng.integers(0, 256, size=int(off[-1]) + tail, dtype=np.uint8)
    seal = oracle.seal_varlen_mt if mt else oracle.seal_varlen
    sealed = buf.copy()
    seal(sealed, off)
    _mix(buf, sealed, off[:-1].astype(np.int64), lens.astype(np.int64), rng, period, keep)
    if want_sealed:
        sealed[:] = buf
        seal(sealed, off)
    else:
        sealed = None
    ref_crc, ref_valid = (oracle.validate_varlen_mt if mt else oracle.validate_varlen)(buf, off)
    return _freeze(SimpleNamespace(buf=buf, off=off, lens=lens, n=lens.size, sealed=sealed, ref_crc=ref_crc,
                                   ref_valid=ref_valid))


def _shuffled(rng, *parts):
    lens = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
    rng.shuffle(lens)
    return lens


def outputs_lens(tiny=True):
    """The 4,099 frames of test_gpu_outputs.py: 3,037 of 4..1532 B, 300 under 4 B, one each of
    1520..1679 B (the 13/14-line edge), 600 of 1661..8192 B, one of 70,000 and one of 300,001 B."""
    rng = np.random.default_rng(4099)
    parts = [rng.integers(4, 1533, size=3037), rng.integers(0, 4, size=300), np.arange(1520, 1680),
             rng.integers(1661, 8193, size=600), [70_000, 300_001]]
    lens = _shuffled(rng, *parts)
    return lens if tiny else lens[lens >= 4]


# What each variable-length case needs at least, per deferral class (checked by test_gate_expect_cpu.py).
VARLEN_NEED = {
    "outputs": {"lt4": 300, "mid": 3050, "ge1661": 621},
    "outputs_seal": {"lt4": 0, "mid": 3050, "ge1661": 621},
    "stream_a": {"lt4": 100, "mid": 4000, "ge1661": 500},
    "stream_b": {"lt4": 100, "mid": 4000, "ge1661": 500},
    "small_64": {"lt4": 0, "mid": 54, "ge1661": 10},
    "small_200": {"lt4": 0, "mid": 170, "ge1661": 30},
    "large": {"lt4": 0, "mid": 2000, "ge1661": 2000},
}


def large_frames(ncu):
    """One run of 64 frames per wave of a 16-wave workgroup on every CU."""
    return 64 * 16 * ncu


@functools.lru_cache(maxsize=None)
def varlen_case(name, ncu=NCU_ASSUMED):
    """A device CSR batch by name (VARLEN_NEED): offsets from 0 into buf[LEAD:], TAIL bytes behind."""
    rng = np.random.default_rng([21, sorted(VARLEN_NEED).index(name)])
    if name in ("outputs", "outputs_seal"):
        lens = outputs_lens(tiny=name == "outputs")
    elif name in ("stream_a", "stream_b"):
        k = 520 if name == "stream_a" else 700
        lens = _shuffled(rng, rng.integers(4, 1533, size=4900 - k), rng.integers(0, 4, size=100),
                         rng.integers(1661, 6001, size=k))
    elif name == "small_64":
        lens = _shuffled(rng, rng.integers(4, 1533, size=54), rng.integers(1661, 4001, size=10))
    elif name == "small_200":
        lens = _shuffled(rng, rng.integers(4, 1533, size=170), rng.integers(1661, 4001, size=30))
    elif name == "large":
        n = large_frames(ncu)
        lens = _shuffled(rng, rng.integers(4, 301, size=n - 2000), rng.integers(1661, 2501, size=2000))
    else:
        raise KeyError(name)
    c = _varlen(lens, [22, sorted(VARLEN_NEED).index(name)], LEAD, TAIL, mt=name == "large")
    # the device calls take buf[LEAD:] as the bytes: offsets relative to it
    c.off.flags.writeable = True
    c.off -= np.uint64(LEAD)
    return _freeze(c)


# ---- host batches (numpy arrays handed to the host entry points) ----
HOST_VARLEN = ("count", "bytes", "solo", "small")
HOST_VARLEN_CHUNKS = {"count": 3, "bytes": 3, "solo": 3, "small": 1}
N_COUNT = (1 << 21) + 5


@functools.lru_cache(maxsize=None)
def host_varlen_case(name):
    rng = np.random.default_rng([31, HOST_VARLEN.index(name)])
    base = 0
    if name == "count":     # cut by frame count: 2^20 + 2^20 + 5 frames
        lens = rng.integers(5, 9, size=N_COUNT)
    elif name == "bytes":   # cut by bytes: just over 128 MB, the bytes start 7 into the array
        lens = rng.integers(1400, 1473, size=96_000)
        lens = lens[:int(np.searchsorted(np.cumsum(lens), 2 * CHUNK_BYTES, side="right")) + 1]
        base = 7
    elif name == "solo":    # a 70 MB frame between two groups of 200: a chunk of its own
        lens = np.concatenate([rng.integers(100, 1501, size=200), [70 << 20], rng.integers(100, 1501, size=200)])
    elif name == "small":
        lens = rng.integers(100, 1501, size=1000)
    else:
        raise KeyError(name)
    return _varlen(lens, [32, HOST_VARLEN.index(name)], base, 0, want_sealed=name == "bytes", mt=True)


HOST_SLOTS = ("count", "count4", "bytes", "small")
HOST_SLOTS_SHAPE = {  # stride, n, shortest datagram, (seal_period, seal_keep), chunks
    "count": (8, N_COUNT, 0, (4, 3), 3),      # lengths 0..8: 4 in 9 can pass the gate at all
    "count4": (8, N_COUNT, 4, (4, 3), 3),     # the same for the seal (at least 4 bytes)
    "bytes": (1472, 2 * 45590 + 1, 4, (3, 1), 3),
    "small": (1472, 1000, 4, (3, 1), 1),
}


@functools.lru_cache(maxsize=None)
def host_slots_case(name):
    """Datagrams of lens[i] bytes at the start of slot i (recvmmsg layout).  The oracle sees the
    datagrams packed into a CSR batch and its results are scattered back into the slots."""
    stride, n, lo, (period, keep), _ = HOST_SLOTS_SHAPE[name]
    rng = np.random.default_rng([41, HOST_SLOTS.index(name)])
    lens = rng.integers(lo, stride + 1, size=n).astype(np.uint32)
    slots = rng.integers(0, 256, size=n * stride, dtype=np.uint8)
    mask = np.arange(stride, dtype=np.uint32)[None, :] < lens[:, None]
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    packed = slots.reshape(n, stride)[mask]
    sealed_p = packed.copy()
    oracle.seal_varlen_mt(sealed_p, off)
    _mix(packed, sealed_p, off[:-1].astype(np.int64), lens.astype(np.int64), rng, period, keep)
    slots.reshape(n, stride)[mask] = packed
    ref_crc, ref_valid = oracle.validate_varlen_mt(packed, off)
    sealed = None
    if lo >= 4:
        oracle.seal_varlen_mt(packed, off)
        sealed = slots.copy()
        sealed.reshape(n, stride)[mask] = packed
    return _freeze(SimpleNamespace(slots=slots, lens=lens, stride=stride, n=n, sealed=sealed, ref_crc=ref_crc,
                                   ref_valid=ref_valid))


def valid_share(case):
    return float(case.ref_valid.mean())
