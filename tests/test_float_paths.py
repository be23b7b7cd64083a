"""The float helpers of the send rate control and of the frame queue's feedback as 64 bits (tests/c/float_paths_gpu.hip,
built with the flags uflow_amd/_build.py gives send_rate.hip): the square root and the division as the core's
statements compile them, rate_round, rate_max, the casts, rate_s_to_ms, rate_initial_send_rate, rate_update_rto, the
throughput equation's value before its cast, its inverse, fq_loss_rate, fq_reset_length and fq_receive_rate, on the
host and on the device, against tests/rate_expect.py and tests/queue_expect.py.  The two primitives of that reference
are themselves held against exact rationals on the very inputs used: a root y of x is correctly rounded if and only if
((y + pred y) / 2)^2 < x < ((y + succ y) / 2)^2, a quotient is float(Fraction(a) / Fraction(b)).  The reference's side
also shows that the inputs can tell: a share of the (rtt, p) pairs changes the bits of the equation's value, and a
share of the loss interval lists the loss rate, when a multiplication and an addition are fused.

Every result is compared as bits, a NaN's sign and payload included, and there is no tolerance."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from uflow_amd import _build

import queue_expect as Q
import rate_expect as E

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "float_paths_gpu.hip")
MAGIC = 0x3153485441504C46
IN_DTYPE = np.dtype([("op", "<u4"), ("n", "<u4"), ("a", "<u8"), ("b", "<u8"), ("len", "<u4", (8,))])
OUT_DTYPE = np.dtype([("r0", "<u8"), ("r1", "<u8")])
(SQRT, DIV, ROUND, MAX, TO_U32, TO_U64, TO_I64, S_TO_MS, INITIAL_RATE, UPDATE_RTO, THROUGHPUT, THROUGHPUT_INV, LOSS_RATE,
 RESET_LENGTH, RECEIVE_RATE) = range(15)
NAMES = ["sqrt", "div", "round", "max", "to_u32", "to_u64", "to_i64", "s_to_ms", "initial_rate", "update_rto", "throughput",
         "throughput_inv", "loss_rate", "reset_length", "receive_rate"]
M64 = E.M64


def bits(v):
    return int(np.float64(v).view(np.uint64))


def with_neighbours(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])


# ---- the inputs ----
def root_inputs(rng):
    """About 60,000: decades 1e-320 .. 1e300, perfect squares scaled by 2^-60, denormals, each with its two
    neighbours; p * 2 / 3 and p * 3 / 8 of the sweep's loss rates (negative, infinite and NaN ones among them)."""
    with np.errstate(all="ignore"):
        decades = 10.0 ** rng.uniform(-320, 300, 11000)
        squares = (rng.integers(1, 1 << 26, 3000).astype(np.float64) ** 2) / 2.0 ** 60
        denormals = rng.integers(1, 1 << 52, 3000).astype(np.uint64).view(np.float64)
        _, loss = E.sweep_values()
        sweep = np.concatenate([(loss * 2.0) / 3.0, (loss * 3.0) / 8.0])
    edges = np.array([0.0, -0.0, 1.0, 2.0, 4.0, 0.25, np.inf, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308])
    return np.concatenate([with_neighbours(decades), with_neighbours(squares), with_neighbours(denormals), sweep, edges])


def quotient_inputs(rng, pairs):
    """20,000 (a, b): the shapes the code divides, and quotients that are denormal."""
    n = 3300
    rtt, p = pairs[:n, 0], pairs[:n, 1]
    with np.errstate(all="ignore"):
        f_p = np.sqrt(p * 2.0 / 3.0) + 12.0 * np.sqrt(p * 3.0 / 8.0) * p * (1.0 + 32.0 * p * p)
        i0 = np.floor(10.0 ** rng.uniform(0, 10.2, n))
        shapes = [(np.full(n, 1472.0), rtt * f_p), (np.full(n, 4380.0), 10.0 ** rng.uniform(-4, 1, n)),
                  (np.floor(10.0 ** rng.uniform(0, 19, n)), np.full(n, 1000.0)), (np.ones(n), 10.0 ** rng.uniform(-9, 0, n)),
                  (rng.choice([1.0, 2.0, 3.0, 4.0, 4.8, 5.4, 5.8, 6.0], n), i0 + rng.choice([0.0, 0.8, 0.6, 0.4, 0.2], n) * 7),
                  (10.0 ** rng.uniform(-300, -295, n), 10.0 ** rng.uniform(9, 27, n))]
    a = np.concatenate([s[0] for s in shapes] + [np.array([2944.0] * 100)])
    b = np.concatenate([s[1] for s in shapes] + [np.floor(10.0 ** rng.uniform(0, 9.6, 100))])
    extra = 20000 - len(a)
    a = np.concatenate([a, 10.0 ** rng.uniform(-30, 30, extra)])
    b = np.concatenate([b, 10.0 ** rng.uniform(-30, 30, extra)])
    return a, b


EDGES = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 1e-320, -1e-320, 0.3, -0.3,
         2147483647.5, 2147483648.0, 4294967294.5, 4294967295.0, 4294967295.5, 4294967296.0, -4294967296.0,
         4503599627370495.5, 4503599627370496.0, 4503599627370497.0, -4503599627370495.5, 9007199254740993.0,
         9223372036854774784.0, 9223372036854775808.0, -9223372036854775808.0, -9223372036854777856.0,
         18446744073709549568.0, 18446744073709551616.0, 3.6893488147419103e19, 1e300, -1e300, np.inf, -np.inf, np.nan]


def build_inputs():
    """The records, in one array; and the parts the checks on the reference's side need."""
    rng = np.random.default_rng(613)
    recs = []

    def add(op, a=None, b=None, ints=False, lens=None):
        count = len(a) if a is not None else len(lens)
        r = np.zeros(count, dtype=IN_DTYPE)
        r["op"] = op
        if a is not None:
            r["a"] = np.asarray(a, dtype=np.uint64) if ints else np.asarray(a, dtype=np.float64).view(np.uint64)
        if b is not None:
            b = np.asarray(b)
            r["b"] = b.astype(np.uint64) if b.dtype.kind in "ui" else b.astype(np.float64).view(np.uint64)
        if lens is not None:
            for k, row in enumerate(lens):
                r["n"][k] = len(row)
                r["len"][k][:len(row)] = row
        recs.append(r)

    pairs = np.stack([10.0 ** rng.uniform(-3, 0, 8000), 10.0 ** rng.uniform(-6, 0, 8000)], axis=1)
    roots = root_inputs(rng)
    add(SQRT, roots)
    qa, qb = quotient_inputs(rng, pairs)
    add(DIV, qa, qb)
    edges = with_neighbours(np.array(EDGES))
    spread = np.concatenate([edges, rng.uniform(-10, 10, 500), np.round(rng.uniform(-1e6, 1e6, 500)) + 0.5,
                             10.0 ** rng.uniform(0, 20, 500), -(10.0 ** rng.uniform(0, 20, 500))])
    for op in (ROUND, TO_U32, TO_U64, TO_I64):
        add(op, spread)
    add(MAX, np.repeat(edges, len(edges)), np.tile(edges, len(edges)))
    add(S_TO_MS, np.concatenate([spread / 1000.0, 10.0 ** rng.uniform(-5, 2, 1000), (np.arange(1000) + 0.5) / 1000.0]))
    rtts = np.concatenate([edges, 10.0 ** rng.uniform(-5, 1, 1000), np.arange(1, 500) / 1000.0])
    add(INITIAL_RATE, rtts)
    rates = np.resize(np.array(E.EDGE_U32 + [int(10 ** x) for x in rng.uniform(0, 9.6, 500)], dtype=np.uint64), len(rtts))
    add(UPDATE_RTO, rtts, rates)
    add(THROUGHPUT, pairs[:, 0], pairs[:, 1])
    sweep_rtt, sweep_loss = E.sweep_values()
    add(THROUGHPUT, sweep_rtt.astype(np.float64) / 1000.0, sweep_loss)
    inv_rtt = np.concatenate([[0.01, 0.05, 0.1, np.nan], 10.0 ** rng.uniform(-3, 0, 3996)])
    inv_target = np.concatenate([[5, 11, 7360, 100], np.floor(10.0 ** rng.uniform(0, 9.6, 3996))]).astype(np.uint64)
    add(THROUGHPUT_INV, inv_rtt, inv_target)
    lists = [np.floor(10.0 ** rng.uniform(0, 9.6, int(rng.integers(6, 9)))).astype(np.uint32) for _ in range(4000)]
    lists += [np.array(x, dtype=np.uint32) for x in ([], [1], [0], [E.M32], [E.M32] * 8, [0] * 8, [1, 0], [0, 5, 0])]
    add(LOSS_RATE, lens=lists)
    add(RESET_LENGTH, np.concatenate([edges, 10.0 ** rng.uniform(-12, 0, 2000), 1.0 / (np.arange(1, 500) + 0.5)]))
    totals = np.concatenate([np.array([0, 1, M64, 1 << 53, (1 << 53) + 1], dtype=np.uint64),
                             rng.integers(0, 1 << 40, 1995, dtype=np.uint64)])
    deltas = np.concatenate([np.array([0, 1, M64, 1000, 3], dtype=np.uint64), rng.integers(0, 100000, 1995, dtype=np.uint64)])
    add(RECEIVE_RATE, totals, deltas, ints=True)
    return {"records": np.concatenate(recs), "pairs": pairs, "lists": lists[:4000]}


# ---- the reference ----
def reference(recs):
    out = np.zeros(len(recs), dtype=OUT_DTYPE)
    a_f, b_f = recs["a"].view(np.float64), recs["b"].view(np.float64)
    with np.errstate(all="ignore"):
        m = recs["op"] == SQRT
        out["r0"][m] = np.sqrt(a_f[m]).view(np.uint64)
        m = recs["op"] == DIV
        out["r0"][m] = (a_f[m] / b_f[m]).view(np.uint64)
    for k in np.nonzero(recs["op"] > DIV)[0]:
        op, a, b = int(recs["op"][k]), float(a_f[k]), float(b_f[k])
        r1 = 0
        if op == ROUND:
            r0 = bits(E.f64_round(a))
        elif op == MAX:
            r0 = bits(E.f64_max(a, b))
        elif op == TO_U32:
            r0 = E.as_u32(a)
        elif op == TO_U64:
            r0 = E.as_u64(a)
        elif op == TO_I64:
            r0 = E.as_isize(a) & M64
        elif op == S_TO_MS:
            r0 = E.s_to_ms(a)
        elif op == INITIAL_RATE:
            r0 = E.compute_initial_send_rate(a)
        elif op == UPDATE_RTO:
            comp = E.SendRateComp(0)
            r0 = bits(comp.update_rto(a, int(recs["b"][k])))
            r1 = comp.rto_ms
        elif op == THROUGHPUT:
            r0, r1 = bits(E.eval_tcp_throughput_f64(a, b)), E.eval_tcp_throughput(a, b)
        elif op == THROUGHPUT_INV:
            c, iterations, stalled = E.eval_tcp_throughput_inv(a, int(recs["b"][k]), stall_rule=True)
            r0, r1 = bits(c), iterations | (1 << 32 if stalled else 0)
        elif op == LOSS_RATE:
            q = Q.LossIntervalQueue()
            q.entries.extend(Q.LossInterval(0, int(x)) for x in recs["len"][k][:int(recs["n"][k])])
            r0 = bits(q.compute_loss_rate())
        elif op == RESET_LENGTH:
            q = Q.LossIntervalQueue()
            q.entries.append(Q.LossInterval(0, 7))
            q.reset(a)
            r0 = q.entries[0].length
        else:
            gen = Q.FeedbackGen(0, 64)
            gen.ack_data, gen.last_feedback_ms = Q.AckData(0, int(recs["a"][k]), False), 0
            r0 = gen.get_feedback(int(recs["b"][k])).receive_rate
        out[k] = (r0, r1)
    return out


def assert_same(recs, got, want, what):
    bad = np.nonzero((got["r0"] != want["r0"]) | (got["r1"] != want["r1"]))[0]
    if len(bad):
        per_op = {NAMES[op]: int((recs["op"][bad] == op).sum()) for op in np.unique(recs["op"][bad])}
        first = [(NAMES[int(recs["op"][k])], float(recs["a"][k:k + 1].view(np.float64)[0]), hex(int(recs["a"][k])),
                  hex(int(recs["b"][k])), recs["len"][k].tolist(), [hex(int(x)) for x in got[k]], [hex(int(x)) for x in want[k]])
                 for k in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} of {len(recs)} results differ, by operation {per_op}; the first: {first}")


# ---- exact rationals ----
def frac(v):
    return Fraction(*float(v).as_integer_ratio())


def fma(a, b, c):
    """round(a * b + c), the product not rounded (finite operands)."""
    return float(frac(a) * frac(b) + frac(c))


def root_is_correctly_rounded(x, y):
    if x != x or x < 0.0:
        return y != y
    if x == 0.0 or math.isinf(x):
        return bits(y) == bits(x)
    lo, hi = (frac(y) + frac(math.nextafter(y, -math.inf))) / 2, (frac(y) + frac(math.nextafter(y, math.inf))) / 2
    return y > 0.0 and lo * lo < frac(x) < hi * hi


def throughput_contracted(rtt, p, which):
    """eval_tcp_throughput_f64 with one of the two places a compiler could contract fused: 1 + (32 p) p, or
    r0 + t1 u2."""
    r0 = E.f64_sqrt(p * 2.0 / 3.0)
    t1 = 12.0 * E.f64_sqrt(p * 3.0 / 8.0) * p
    u2 = fma(32.0 * p, p, 1.0) if which == 0 else 1.0 + 32.0 * p * p
    f_p = fma(t1, u2, r0) if which == 1 else r0 + t1 * u2
    return 1472.0 / (rtt * f_p)


def loss_rate_contracted(lens):
    W = Q.LossIntervalQueue.WEIGHTS
    i0 = i1 = w = 0.0
    for i in range(len(lens) - 1):
        i0 = fma(float(lens[i]), W[i], i0)
        w += W[i]
    for i in range(1, len(lens)):
        i1 = fma(float(lens[i]), W[i - 1], i1)
    return w / max(i0, i1)


# ---- fixtures ----
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("float_paths")
    w = build_inputs()
    w["dir"], w["input"] = d, str(d / "input.bin")
    with open(w["input"], "wb") as f:
        f.write(np.array([MAGIC, len(w["records"])], dtype="<u8").tobytes())
        f.write(w["records"].tobytes())
    w["reference"] = reference(w["records"])
    return w


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program, compiled with what _native_identity() gives send_rate.hip: a flag added there reaches this test."""
    _, flags, per_source, _ = _build._native_identity()
    exe = str(tmp_path_factory.mktemp("float_paths_bin") / "float_paths_gpu")
    cmd = flags + per_source.get("send_rate.hip", []) + ["-I", _build.CSRC, "-I", os.path.join(_build.REPO_DIR, "include"),
                                                         SRC, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(program, work, mode, timeout):
    path = str(work["dir"] / (mode + ".bin"))
    r = subprocess.run([program, mode, work["input"], path], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip() == "ok: %d" % len(work["records"]), r.stdout
    out = np.fromfile(path, dtype=OUT_DTYPE)
    assert len(out) == len(work["records"])
    return out


@pytest.fixture(scope="module")
def host_out(program, work):
    return run(program, work, "host", 120)


# ---- the tests ----
def test_the_inputs(work):
    recs = work["records"]
    counts = np.bincount(recs["op"], minlength=15)
    assert counts[SQRT] > 59000 and counts[DIV] == 20000 and counts[THROUGHPUT] == 8000 + 4096, counts
    assert counts[THROUGHPUT_INV] == 4000 and counts[LOSS_RATE] == 4008 and (counts > 0).all(), counts
    assert all(6 <= len(x) <= 8 for x in work["lists"])
    inv = work["reference"][recs["op"] == THROUGHPUT_INV]
    assert (inv["r1"][:2] == (54 | 1 << 32)).all() and inv["r0"][0] == bits(1.0)      # the two documented stalls
    assert (inv["r1"] >> 32).sum() >= 3 and ((inv["r1"] >> 32) == 0).sum() > 3000


def test_reference_roots_and_quotients_are_correctly_rounded(work):
    """The reference's two primitives against exact rationals, on the very inputs the program gets."""
    recs, ref = work["records"], work["reference"]
    m = recs["op"] == SQRT
    x, y = recs["a"][m].view(np.float64), ref["r0"][m].view(np.float64)
    bad = [k for k in range(len(x)) if not root_is_correctly_rounded(float(x[k]), float(y[k]))]
    assert not bad, (len(bad), [(x[k], y[k]) for k in bad[:5]])
    m = recs["op"] == DIV
    a, b, q = recs["a"][m].view(np.float64), recs["b"][m].view(np.float64), ref["r0"][m].view(np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (b != 0).all()
    bad = [k for k in range(len(a)) if bits(float(frac(a[k]) / frac(b[k]))) != bits(q[k])]
    assert not bad, (len(bad), [(a[k], b[k], q[k]) for k in bad[:5]])
    tiny = np.abs(q) < 2.2250738585072014e-308
    assert (tiny & (q != 0)).sum() > 500          # denormal quotients


def test_the_inputs_tell_a_contraction(work):
    """Were a multiplication fused with the addition behind it, the bits would change: for at least 3 % of the
    (rtt, p) pairs in the equation's value, for at least 2 % of the lists in the loss rate."""
    pairs, lists = work["pairs"], work["lists"]
    changed = 0
    for rtt, p in pairs:
        v = bits(E.eval_tcp_throughput_f64(float(rtt), float(p)))
        changed += any(bits(throughput_contracted(float(rtt), float(p), w)) != v for w in (0, 1))
    assert changed >= 0.03 * len(pairs), (changed, len(pairs))
    recs, ref = work["records"], work["reference"]
    rates = ref["r0"][recs["op"] == LOSS_RATE][:len(lists)]
    moved = sum(bits(loss_rate_contracted(x)) != int(r) for x, r in zip(lists, rates))
    assert moved >= 0.02 * len(lists), (moved, len(lists))
    print(f"contraction changes {changed} of {len(pairs)} pairs, {moved} of {len(lists)} lists")


def test_host_mode_equals_the_reference(work, host_out):
    assert_same(work["records"], host_out, work["reference"], "host against the reference")


@pytest.mark.gpu
def test_device_mode_equals_the_reference_and_the_host(program, work, host_out):
    """One run of the device mode, as a child process with a time limit."""
    got = run(program, work, "device", 60)
    assert_same(work["records"], got, work["reference"], "device against the reference")
    assert_same(work["records"], got, host_out, "device against the host")
