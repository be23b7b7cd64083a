"""CPU: every *_host wrapper of uflow_amd.frame refuses a bad caller-supplied array before the C call sees it.

One table: for each wrapper a call that passes (fresh state, empty traffic) and the arguments the C side writes into.
Each of those is then given with the wrong dtype, one entry short, non-contiguous and read-only, and every time the
wrapper raises a ValueError that names the argument.  The CSRs (and the per-record inputs) one entry short raise too.
"""
import numpy as np
import pytest

from uflow_amd import _native, frame as fr

U64 = np.uint64


def Z(n, dt):
    return np.zeros(n, dtype=dt)


def _senders(n):
    s = Z(n, fr.SENDER_DTYPE)
    s["window_size"] = 8
    s["max_alloc"] = 1 << 16
    s["window_parent_id"] = fr.NO_PARENT
    s["channel_parent_id"] = fr.NO_PARENT
    return s


def _table(n):
    """(name, function, keyword arguments of a passing call, {written argument: entries it must hold}, inputs that
    are one entry short when their last entry is cut).  "arenas.heap" is arenas["heap"]."""
    csr = lambda: Z(n + 1, U64)  # noqa: E731
    no_infos, no_items = Z(0, fr.FRAME_INFO_DTYPE), Z(0, fr.ITEM_DTYPE)
    queues, log = fr.new_frame_queues(n, 8, 4)
    rate, entries = fr.new_rate_states(n, 100000, 4)
    states, arenas = fr.new_resend_states(n, 8, 1 << 16, 8, 4, heap_cap=8, stage_cap=16)
    arena_sizes = {"arenas." + name: 0 for name, _ in fr.RESEND_ARENAS}
    yield ("build_batch_host", fr.build_batch_host,
           dict(infos=Z(n, fr.FRAME_INFO_DTYPE), items=no_items, payload=Z(0, np.uint8), src_base=Z(n, U64)), {},
           ["src_base"])
    yield ("pack_host", fr.pack_host,
           dict(items=Z(n, fr.ITEM_DTYPE), flush_first=csr(), flushes=Z(n, fr.FLUSH_DTYPE), frames_cap=n,
                nonce_bits=Z(1, np.uint32), infos=Z(n, fr.FRAME_INFO_DTYPE)), {"infos": n}, ["flush_first", "nonce_bits"])
    yield ("emit_packets_host", fr.emit_packets_host,
           dict(packets=Z(0, fr.PACKET_DTYPE), packet_first=csr(), senders=_senders(n), items_cap=n,
                items=Z(n, fr.ITEM_DTYPE), senders_out=Z(n, fr.SENDER_DTYPE)), {"items": n, "senders_out": n},
           ["packet_first"])
    yield ("receive_packets_host", fr.receive_packets_host,
           dict(infos=Z(n, fr.FRAME_INFO_DTYPE), items=no_items, payload=Z(0, np.uint8), frame_first=csr(),
                receivers=fr.new_receivers(n, 8), slots=Z(8 * n, fr.RX_SLOT_DTYPE), slot_first=np.arange(n + 1, dtype=U64) * U64(8),
                carry_in=Z(0, np.uint8), src_base=Z(n, U64), frame_accept=Z(n, np.uint8), carry_out=Z(4, np.uint8),
                out_bytes=Z(4, np.uint8), packets=Z(4, fr.RX_PACKET_DTYPE), receivers_out=Z(n, fr.RECEIVER_DTYPE)),
           {"slots": 0, "carry_out": 0, "out_bytes": 0, "packets": 0, "receivers_out": n},
           ["frame_first", "slot_first", "src_base", "frame_accept"])
    yield ("frame_window_host", fr.frame_window_host,
           dict(infos=Z(n, fr.FRAME_INFO_DTYPE), frame_first=csr(), windows=fr.new_frame_windows(n, 8), groups_cap=2 * n,
                frame_accept=Z(n, np.uint8), groups=Z(2 * n, fr.ITEM_DTYPE), group_first=csr(),
                results=Z(n, fr.FRAME_WINDOW_RESULT_DTYPE), windows_out=Z(n, fr.FRAME_WINDOW_DTYPE)),
           {"frame_accept": n, "groups": 2 * n, "group_first": n + 1, "results": n, "windows_out": n}, ["frame_first"])
    yield ("frame_queue_host", fr.frame_queue_host,
           dict(infos=no_infos, items=no_items, frame_first=csr(), sent=Z(0, fr.SENT_FRAME_DTYPE), sent_first=csr(),
                queues=queues, steps=Z(n, fr.FRAME_QUEUE_STEP_DTYPE), log=log, ref_acked=Z(4, np.uint8),
                results=Z(n, fr.FRAME_QUEUE_RESULT_DTYPE), queues_out=Z(n, fr.FRAME_QUEUE_DTYPE)),
           {"log": 0, "ref_acked": 0, "results": n, "queues_out": n}, ["frame_first", "sent_first", "steps"])
    yield ("rate_begin_host", fr.rate_begin_host,
           dict(states=rate, now_ms=Z(n, U64), extra_flags=Z(n, np.uint32), steps=Z(n, fr.FRAME_QUEUE_STEP_DTYPE),
                states_out=Z(n, fr.RATE_STATE_DTYPE)), {"steps": n, "states_out": n}, ["now_ms", "extra_flags"])
    yield ("rate_step_host", fr.rate_step_host,
           dict(states=rate, ticks=Z(n, fr.RATE_TICK_DTYPE), fq_results=Z(n, fr.FRAME_QUEUE_RESULT_DTYPE), entries=entries,
                flush_results=Z(n, fr.FLUSH_RESULT_DTYPE), result_index=np.full(n, fr.NO_INDEX, dtype=np.uint32),
                flushes=Z(n, fr.FLUSH_DTYPE), flush_index=np.full(n, fr.NO_INDEX, dtype=np.uint32),
                results=Z(n, fr.RATE_RESULT_DTYPE), states_out=Z(n, fr.RATE_STATE_DTYPE)),
           {"entries": 0, "flushes": 0, "results": n, "states_out": n},
           ["ticks", "fq_results", "result_index", "flush_index"])
    yield ("resend_begin_host", fr.resend_begin_host,
           dict(infos=no_infos, frame_first=csr(), queues=queues, log=log, rate=Z(n, fr.RATE_RESULT_DTYPE),
                flushes=Z(n, fr.FLUSH_DTYPE), states=states, senders=_senders(n), arenas=arenas, flags=Z(n, np.uint32),
                results=Z(n, fr.RESEND_RESULT_DTYPE), states_out=Z(n, fr.RESEND_DTYPE), senders_out=Z(n, fr.SENDER_DTYPE)),
           dict(arena_sizes, results=n, states_out=n, senders_out=n),
           ["frame_first", "queues", "rate", "flushes", "senders", "flags"])
    yield ("resend_place_host", fr.resend_place_host,
           dict(states=states, begin_results=Z(n, fr.RESEND_RESULT_DTYPE), arenas=arenas, flush_first=csr(),
                items=Z(n, fr.ITEM_DTYPE)), {"items": 0, "arenas.stage": 0}, ["flush_first", "begin_results"])
    yield ("resend_commit_host", fr.resend_commit_host,
           dict(flush_results=Z(n, fr.FLUSH_RESULT_DTYPE), infos=no_infos, out_offsets=Z(1, U64), frames_used=0,
                items=no_items, flush_first=csr(), packets=Z(0, fr.PACKET_DTYPE), packet_first=csr(),
                packet_results=Z(0, fr.PACKET_RESULT_DTYPE), sender_results=Z(n, fr.SENDER_RESULT_DTYPE),
                begin_results=Z(n, fr.RESEND_RESULT_DTYPE), rate=Z(n, fr.RATE_RESULT_DTYPE), states=states,
                senders=_senders(n), arenas=arenas, sent=Z(2, fr.SENT_FRAME_DTYPE), next_extra_flags=Z(n, np.uint32),
                results=Z(n, fr.RESEND_COMMIT_RESULT_DTYPE), states_out=Z(n, fr.RESEND_DTYPE),
                retake=Z(n, fr.SENDER_DTYPE)),
           dict({k: v for k, v in arena_sizes.items() if k.split(".")[1] in ("heap", "pkts", "frag_acked", "tx")},
                sent=0, next_extra_flags=n, results=n, states_out=n, retake=n),
           ["flush_first", "packet_first", "out_offsets", "flush_results", "sender_results", "begin_results", "rate",
            "senders"])


def _with(kw, name, value):
    kw = dict(kw)
    if name.startswith("arenas."):
        kw["arenas"] = dict(kw["arenas"], **{name.split(".")[1]: value})
    else:
        kw[name] = value
    return kw


def _get(kw, name):
    return kw["arenas"][name.split(".")[1]] if name.startswith("arenas.") else kw[name]


WRAPPERS = ["build_batch_host", "pack_host", "emit_packets_host", "receive_packets_host", "frame_window_host",
            "frame_queue_host", "rate_begin_host", "rate_step_host", "resend_begin_host", "resend_place_host",
            "resend_commit_host"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_host_wrapper_refuses_bad_arguments(wrapper, n):
    (name, f, kw, written, short), = [row for row in _table(n) if row[0] == wrapper]
    try:  # the table's call itself passes the wrapper's checks (what C makes of the state is not this test's matter)
        f(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    except _native.NativeError:
        pass
    for arg, need in written.items():
        good = _get(kw, arg)
        ro = good.copy()
        ro.flags.writeable = False
        bad = {"wrong dtype": np.zeros(good.size, dtype="<i2"),
               "non-contiguous": np.zeros(2 * max(good.size, 2), dtype=good.dtype)[::2],
               "read-only": ro}
        if need:
            bad["one entry short"] = good[:need - 1].copy()
        for what, value in bad.items():
            with pytest.raises(ValueError) as e:
                f(**_with(kw, arg, value))
            assert arg.split(".")[-1] in str(e.value), (name, arg, what, str(e.value))
    for arg in short:
        with pytest.raises(ValueError):
            f(**_with(kw, arg, kw[arg][:-1].copy()))


def test_parse_batch_host_coerces_its_inputs():
    """parse_batch_host takes no array to write into; its inputs are coerced like every wrapper's."""
    infos, items = fr.parse_batch_host([0] * 4, [0, 4], valid=[0])
    assert infos.dtype == fr.FRAME_INFO_DTYPE and infos.size == 1 and items.size == 0
    infos, items = fr.parse_batch_host(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    assert infos.size == 0 and items.size == 0


def test_table_covers_every_host_wrapper():
    names = {k for k in vars(fr) if k.endswith("_host")}
    assert names == set(WRAPPERS) | {"parse_batch_host"}
