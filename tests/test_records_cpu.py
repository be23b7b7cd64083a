"""CPU: the Python binding's copies of the C ABI agree with the headers themselves.

  * every record dtype of uflow_amd/records.py, and the four ctypes structures _native.py keeps (with ufc_item, which
    Frame.read and datagram_is_valid instantiate), against sizeof / offsetof compiled from include/*.h;
  * every argtypes list of _native._SIGNATURES against the prototypes: parameter count, and pointer-ness by position;
  * uflow_amd.batch.rows / records, the one record <-> device-row conversion, round trip on the CPU.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from uflow_amd import _native, frame as fr
from uflow_amd.records import RECORDS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")
CTYPES_STRUCTS = {"ufc_frame_info": _native.FrameInfo, "ufc_item": _native.Item, "ufc_builder": _native.Builder,
                  "ufc_datagram_ref": _native.DatagramRef, "ufc_xfer": _native.Xfer}


def _header_layout(tmp_path, fields):
    """{line prefix: numbers} printed by a C99 program compiled against the headers: "S <struct>" -> (sizeof,) and
    "F <struct>.<field>" -> (offsetof, member size) for `fields`, a {struct: [field names]}."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "uflow_frame_crc.h"', '#include "uflow_frame_codec.h"',
             "int main(void) {"]
    for struct, names in fields.items():
        lines.append(f'  printf("S {struct} %lu\\n", (unsigned long)sizeof({struct}));')
        for f in names:
            lines.append(f'  printf("F {struct}.{f} %lu %lu\\n", (unsigned long)offsetof({struct}, {f}), '
                         f"(unsigned long)sizeof((({struct} *)0)->{f}));")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {}
    for line in out.splitlines():
        kind, name, *nums = line.split()
        assert (kind, name) not in got, line
        got[kind, name] = tuple(int(v) for v in nums)
    return got


def test_record_table_matches_header(tmp_path):
    assert len(RECORDS) == 28
    for struct, dt in RECORDS.items():  # the mapping is by name: FOO_BAR_DTYPE is ufc_foo_bar, and frame.py exports it
        assert getattr(fr, struct[len("ufc_"):].upper() + "_DTYPE") is dt
    got = _header_layout(tmp_path, {s: dt.names for s, dt in RECORDS.items()})
    want = {}
    for struct, dt in RECORDS.items():
        want["S", struct] = (dt.itemsize,)
        for f in dt.names:
            want["F", f"{struct}.{f}"] = (dt.fields[f][1], dt.fields[f][0].itemsize)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    # no struct of the codec header is left out of the table but the two the batched calls never take
    with open(os.path.join(INCLUDE, "uflow_frame_codec.h")) as f:
        declared = set(re.findall(r"^\} (ufc_\w+);", f.read(), flags=re.M))
    assert declared - set(RECORDS) == {"ufc_builder", "ufc_datagram_ref"}


def test_ctypes_structures_match_header(tmp_path):
    got = _header_layout(tmp_path, {s: [f for f, _ in c._fields_] for s, c in CTYPES_STRUCTS.items()})
    want = {}
    for struct, c in CTYPES_STRUCTS.items():
        want["S", struct] = (ctypes.sizeof(c),)
        for f, _ in c._fields_:
            want["F", f"{struct}.{f}"] = (getattr(c, f).offset, getattr(c, f).size)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    # the two structures that exist in both forms agree with each other too
    for struct in ("ufc_frame_info", "ufc_item"):
        assert ctypes.sizeof(CTYPES_STRUCTS[struct]) == RECORDS[struct].itemsize


def test_no_ctypes_structure_without_a_user():
    """_native.py keeps a ctypes.Structure only where Python builds one; everything else is a numpy dtype."""
    kept = {n for n, v in vars(_native).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    assert kept == {c.__name__ for c in CTYPES_STRUCTS.values()}


def _prototypes():
    """{function: [parameter text]} of both headers, comments stripped."""
    text = ""
    for h in ("uflow_frame_crc.h", "uflow_frame_codec.h"):
        with open(os.path.join(INCLUDE, h)) as f:
            text += f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = {}
    for name, params in re.findall(r"\b(ufc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        protos[name] = [] if params == ["void"] else params
    return protos


def test_signatures_match_prototypes():
    protos = _prototypes()
    assert set(protos) == set(_native._SIGNATURES) and len(protos) == 73
    pointer_types = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
    for name, (_, argtypes) in _native._SIGNATURES.items():
        params = protos[name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (p, t) in enumerate(zip(params, argtypes)):
            # (an array parameter, uint8_t id[UFC_COMM_ID_BYTES], is a pointer)
            assert ("*" in p or "[" in p) == issubclass(t, pointer_types), (name, k, p, t)


def test_rows_and_records_round_trip_on_the_cpu():
    import torch
    from uflow_amd.batch import records, rows

    def alias(t, a):
        return np.shares_memory(t.numpy(), a)

    for n in (0, 1, 3):
        q, _ = fr.new_frame_queues(n, 8, 4, base_id=7)  # uint64, float64-sized and sub-array fields
        if n:
            q["li_end_time_ms"][-1] = np.arange(9, dtype=np.uint64) + np.uint64(2 ** 63)
            q["rb_frames"][0] = (0xFFFFFFFF, 5)
        t = rows(q, "cpu")
        assert t.dtype == torch.uint8 and tuple(t.shape) == (n, fr.FRAME_QUEUE_DTYPE.itemsize) and not alias(t, q)
        back = records(t, fr.FRAME_QUEUE_DTYPE)
        assert back.dtype == fr.FRAME_QUEUE_DTYPE and back.shape == (n,) and back.tobytes() == q.tobytes()
        assert not alias(t, back)
        steps = np.zeros(n, dtype=fr.FRAME_QUEUE_STEP_DTYPE)  # a float64 field
        steps["reset_loss_rate"] = -0.0
        assert records(rows(steps, "cpu"), fr.FRAME_QUEUE_STEP_DTYPE).tobytes() == steps.tobytes()
        csr = (np.arange(n + 1, dtype=np.uint64) * np.uint64(3)) + np.uint64(2 ** 63 if n else 0)
        t = rows(csr, "cpu")
        assert t.dtype == torch.int64 and tuple(t.shape) == (n + 1,) and not alias(t, csr)
        assert records(t, np.uint64).tobytes() == csr.tobytes()
    u32 = np.array([2 ** 31, 2 ** 32 - 1, 5], dtype=np.uint32)
    t = rows(u32, "cpu")
    assert t.dtype == torch.int32 and t.tolist() == [-2 ** 31, -1, 5] and not alias(t, u32)
    assert records(t, np.uint32).tobytes() == u32.tobytes()
    u8 = np.arange(5, dtype=np.uint8)
    t = rows(u8, "cpu")
    assert t.dtype == torch.uint8 and not alias(t, u8) and records(t, np.uint8).tobytes() == u8.tobytes()
    q, _ = fr.new_frame_queues(5, 8, 4)
    q["log_base_id"] = np.arange(5)
    t = rows(q[::2], "cpu")  # a non-contiguous slice
    assert tuple(t.shape) == (3, fr.FRAME_QUEUE_DTYPE.itemsize)
    assert records(t, fr.FRAME_QUEUE_DTYPE)["log_base_id"].tolist() == [0, 2, 4] and not alias(t, q)
    ro = np.arange(4, dtype=np.uint64)
    ro.flags.writeable = False
    assert records(rows(ro, "cpu"), np.uint64).tolist() == [0, 1, 2, 3]
