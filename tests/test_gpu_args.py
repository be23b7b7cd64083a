"""MI355X: the stage methods of FrameCrcEngine refuse a bad record tensor before anything is queued, and
uflow_amd.batch.rows / records carry records to the device and back bit for bit.

One table: for each of the 13 stage methods a set of arguments of the right types (zeroed records).  Every record
tensor among them is then given with rows one byte narrow, and on the CPU; each time the method raises ValueError, the
C entry point is not reached (it is patched to fail the test) and no output is allocated.  No kernel runs here.
"""
import numpy as np
import pytest
import torch

from uflow_amd import _native, frame as fr
from uflow_amd.batch import records, rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _table(n):
    """{method: keyword arguments}: device tensors of the right dtypes and sizes for n connections of one frame each."""
    R = lambda dt, k=n: rows(np.zeros(k, dtype=dt), DEV)  # noqa: E731
    I64 = lambda k: torch.zeros(k, dtype=torch.int64, device=DEV)  # noqa: E731
    I32 = lambda k: torch.zeros(k, dtype=torch.int32, device=DEV)  # noqa: E731
    U8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=DEV)  # noqa: E731
    arenas = lambda: {name: R(dt, 4) for name, dt in fr.RESEND_ARENAS}  # noqa: E731
    infos, items = lambda: R(fr.FRAME_INFO_DTYPE), lambda: R(fr.ITEM_DTYPE)  # noqa: E731
    return {
        "parse_varlen": dict(data=U8(8), offsets=I64(n + 1), valid=U8(n)),
        "build_sizes_varlen": dict(infos=infos(), items=items(), payload_len=0),
        "build_varlen": dict(infos=infos(), items=items(), payload=U8(0)),
        "pack_flushes": dict(items=items(), flush_first=I64(n + 1), flushes=R(fr.FLUSH_DTYPE)),
        "emit_packets": dict(packets=R(fr.PACKET_DTYPE), packet_first=I64(n + 1), senders=R(fr.SENDER_DTYPE), items_cap=n,
                             items=items(), senders_out=R(fr.SENDER_DTYPE)),
        "receive_packets": dict(infos=infos(), items=items(), payload=U8(0), frame_first=I64(n + 1),
                                receivers=R(fr.RECEIVER_DTYPE), slots=R(fr.RX_SLOT_DTYPE, 8 * n), slot_first=I64(n + 1),
                                carry_in=U8(0), carry_cap=0, out_cap=0, packets_cap=0, packets=R(fr.RX_PACKET_DTYPE),
                                receivers_out=R(fr.RECEIVER_DTYPE)),
        "frame_window": dict(infos=infos(), frame_first=I64(n + 1), windows=R(fr.FRAME_WINDOW_DTYPE),
                             groups=R(fr.ITEM_DTYPE, 2 * n), windows_out=R(fr.FRAME_WINDOW_DTYPE)),
        "frame_queue": dict(infos=infos(), items=items(), frame_first=I64(n + 1), sent=R(fr.SENT_FRAME_DTYPE),
                            sent_first=I64(n + 1), queues=R(fr.FRAME_QUEUE_DTYPE), steps=R(fr.FRAME_QUEUE_STEP_DTYPE),
                            log=R(fr.SENT_FRAME_DTYPE, 8), queues_out=R(fr.FRAME_QUEUE_DTYPE)),
        "rate_begin": dict(states=R(fr.RATE_STATE_DTYPE), now_ms=I64(n), steps=R(fr.FRAME_QUEUE_STEP_DTYPE),
                           states_out=R(fr.RATE_STATE_DTYPE)),
        "rate_step": dict(states=R(fr.RATE_STATE_DTYPE), ticks=R(fr.RATE_TICK_DTYPE),
                          fq_results=R(fr.FRAME_QUEUE_RESULT_DTYPE), entries=R(fr.RECV_RATE_ENTRY_DTYPE, 4),
                          flush_results=R(fr.FLUSH_RESULT_DTYPE), result_index=I32(n), flushes=R(fr.FLUSH_DTYPE),
                          flush_index=I32(n), results=R(fr.RATE_RESULT_DTYPE), states_out=R(fr.RATE_STATE_DTYPE)),
        "resend_begin": dict(infos=infos(), frame_first=I64(n + 1), queues=R(fr.FRAME_QUEUE_DTYPE),
                             log=R(fr.SENT_FRAME_DTYPE, 8), rate=R(fr.RATE_RESULT_DTYPE), flushes=R(fr.FLUSH_DTYPE),
                             states=R(fr.RESEND_DTYPE), senders=R(fr.SENDER_DTYPE), arenas=arenas(),
                             results=R(fr.RESEND_RESULT_DTYPE), states_out=R(fr.RESEND_DTYPE),
                             senders_out=R(fr.SENDER_DTYPE)),
        "resend_place": dict(states=R(fr.RESEND_DTYPE), begin_results=R(fr.RESEND_RESULT_DTYPE),
                             arenas={"stage": R(fr.ITEM_DTYPE, 4)}, flush_first=I64(n + 1), items=items()),
        "resend_commit": dict(flush_results=R(fr.FLUSH_RESULT_DTYPE), infos=infos(), out_offsets=I64(n + 1),
                              frames_used=I64(1), items=items(), flush_first=I64(n + 1), packets=R(fr.PACKET_DTYPE),
                              packet_first=I64(n + 1), packet_results=R(fr.PACKET_RESULT_DTYPE),
                              sender_results=R(fr.SENDER_RESULT_DTYPE), begin_results=R(fr.RESEND_RESULT_DTYPE),
                              rate=R(fr.RATE_RESULT_DTYPE), states=R(fr.RESEND_DTYPE), senders=R(fr.SENDER_DTYPE),
                              arenas={k: v for k, v in arenas().items() if k in ("heap", "pkts", "frag_acked", "tx")},
                              sent=R(fr.SENT_FRAME_DTYPE), results=R(fr.RESEND_COMMIT_RESULT_DTYPE),
                              states_out=R(fr.RESEND_DTYPE), retake=R(fr.SENDER_DTYPE)),
    }


METHODS = sorted(["parse_varlen", "build_sizes_varlen", "build_varlen", "pack_flushes", "emit_packets", "receive_packets",
                  "frame_window", "frame_queue", "rate_begin", "rate_step", "resend_begin", "resend_place",
                  "resend_commit"])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("method", METHODS)
def test_stage_method_refuses_bad_record_tensors(engine, monkeypatch, method, n):
    def reached(*a):
        raise AssertionError("the C entry point was reached")
    for sym in _native.SYMBOLS:
        if sym.endswith("_varlen"):
            monkeypatch.setattr(_native.lib(), sym, reached)
    table = _table(n)
    assert sorted(table) == METHODS and len(METHODS) == 13
    kw = table[method]
    tensors = [(k, v) for k, v in kw.items() if isinstance(v, torch.Tensor)]
    tensors += [("arenas." + k, v) for k, v in kw.get("arenas", {}).items()]
    cases = [(k, "on the CPU", v.cpu()) for k, v in tensors]
    cases += [(k, "one byte narrow", v[:, :-1].contiguous()) for k, v in tensors if v.dim() == 2 and v.shape[1] > 1]
    assert any(what == "one byte narrow" for _, what, _ in cases) or method == "parse_varlen"
    torch.cuda.synchronize()
    for name, what, bad in cases:
        a = dict(kw)
        if name.startswith("arenas."):
            a["arenas"] = dict(kw["arenas"], **{name.split(".")[1]: bad})
        else:
            a[name] = bad
        before = torch.cuda.memory_allocated()
        with pytest.raises(ValueError):
            getattr(engine, method)(**a)
        assert torch.cuda.memory_allocated() == before, (method, name, what, "an output was allocated")


@pytest.mark.parametrize("n", [0, 1, 3])
def test_rows_and_records_round_trip_on_the_device(n):
    q, _ = fr.new_frame_queues(n, 8, 4, base_id=0xFFFFFFF0)
    if n:
        q["li_end_time_ms"][-1] = np.arange(9, dtype=np.uint64) + np.uint64(2 ** 63)
        q["ack_total_size"] = np.uint64(2 ** 64 - 1)
    t = rows(q, DEV)
    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (n, fr.FRAME_QUEUE_DTYPE.itemsize)
    back = records(t, fr.FRAME_QUEUE_DTYPE)
    assert back.dtype == fr.FRAME_QUEUE_DTYPE and back.shape == (n,) and back.tobytes() == q.tobytes()
    csr = np.arange(n + 1, dtype=np.uint64) * np.uint64(5) + np.uint64(2 ** 63)
    t = rows(csr, DEV)
    assert t.is_cuda and t.dtype == torch.int64 and tuple(t.shape) == (n + 1,)
    assert records(t, np.uint64).tobytes() == csr.tobytes()
    t[:] = 0  # (the tensor is a copy: the host array keeps its values)
    assert csr[0] == np.uint64(2 ** 63)
