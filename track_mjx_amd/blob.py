"""Flat "model blob": the binary hand-off between the host (Python) and the C-ABI.

Layout (little endian):
    u32 magic 'TMJX' (0x584a4d54), u32 version, u32 n_entries, u32 pad
    per entry: char name[32]; i32 dtype (0 = int32, 1 = float64); i32 count;
               payload, zero padded to a multiple of 8 bytes.

Text form (`*.tmjx.txt`): the same entries, lossless and diffable — a header line "<name> int32|float64 <count>" per entry, then
its values, float64 written as Python's shortest round-trip repr.  `load` reads either form by file name; `pack` of what it reads
gives the same bytes as the binary form of the same entries.

Both the HIP library (track_mjx_amd/csrc/blob_reader.h) and the oracle
(oracle/tmjx_oracle.c) look entries up by name; float64 payloads are narrowed to
fp32 by the consumer (MJX's put_model does the same narrowing of MuJoCo's
float64 model: reference call site track_mjx/environment/task/single_clip_tracking.py:91).
"""
from __future__ import annotations

import struct
from collections import OrderedDict

import numpy as np

MAGIC = 0x584A4D54
VERSION = 1


def pack(entries: "OrderedDict[str, np.ndarray]") -> bytes:
    out = [struct.pack("<IIII", MAGIC, VERSION, len(entries), 0)]
    for name, arr in entries.items():
        arr = np.asarray(arr)
        if arr.dtype.kind in "iub":
            code, data = 0, np.ascontiguousarray(arr, dtype="<i4")
        else:
            code, data = 1, np.ascontiguousarray(arr, dtype="<f8")
        bname = name.encode()
        if len(bname) > 31:
            raise ValueError(f"blob entry name too long: {name}")
        payload = data.tobytes()
        pad = (-len(payload)) % 8
        out.append(bname.ljust(32, b"\0"))
        out.append(struct.pack("<ii", code, data.size))
        out.append(payload + b"\0" * pad)
    return b"".join(out)


def unpack(buf: bytes) -> "OrderedDict[str, np.ndarray]":
    magic, version, n, _ = struct.unpack_from("<IIII", buf, 0)
    if magic != MAGIC or version != VERSION:
        raise ValueError("not a TMJX model blob")
    off = 16
    entries: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for _ in range(n):
        name = buf[off:off + 32].split(b"\0", 1)[0].decode()
        code, count = struct.unpack_from("<ii", buf, off + 32)
        off += 40
        if code == 0:
            arr = np.frombuffer(buf, dtype="<i4", count=count, offset=off).copy()
            nbytes = 4 * count
        else:
            arr = np.frombuffer(buf, dtype="<f8", count=count, offset=off).copy()
            nbytes = 8 * count
        off += nbytes + ((-nbytes) % 8)
        entries[name] = arr
    return entries


TEXT_SUFFIX = ".tmjx.txt"


def to_text(entries: "OrderedDict[str, np.ndarray]") -> str:
    out = ["# TMJX model blob, text form (track_mjx_amd/blob.py): per entry a line '<name> int32|float64 <count>', then its values"]
    for name, arr in entries.items():
        arr = np.asarray(arr).ravel()
        ints = arr.dtype.kind in "iub"
        vals = [str(int(v)) for v in arr] if ints else [repr(float(v)) for v in arr]
        out.append(f"{name} {'int32' if ints else 'float64'} {arr.size}")
        out += [" ".join(vals[i:i + 8]) for i in range(0, len(vals), 8)]
    return "\n".join(out) + "\n"


def from_text(text: str) -> "OrderedDict[str, np.ndarray]":
    tokens = [t for ln in text.splitlines() if not ln.startswith("#") for t in ln.split()]
    entries: "OrderedDict[str, np.ndarray]" = OrderedDict()
    i = 0
    while i < len(tokens):
        name, kind, count = tokens[i], tokens[i + 1], int(tokens[i + 2])
        vals = tokens[i + 3:i + 3 + count]
        if kind not in ("int32", "float64") or len(vals) != count:
            raise ValueError(f"malformed text blob entry {name!r}")
        entries[name] = np.array([int(v) for v in vals], dtype=np.int32) if kind == "int32" else np.array([float(v) for v in vals], dtype=np.float64)
        i += 3 + count
    return entries


def load(path) -> "OrderedDict[str, np.ndarray]":
    if str(path).endswith(TEXT_SUFFIX):
        with open(path) as f:
            return from_text(f.read())
    with open(path, "rb") as f:
        return unpack(f.read())


def save(path, entries) -> None:
    if str(path).endswith(TEXT_SUFFIX):
        with open(path, "w") as f:
            f.write(to_text(entries))
        return
    with open(path, "wb") as f:
        f.write(pack(entries))


def stem(path) -> str:
    """File name without .tmjx / .tmjx.txt (side files of a blob are named after it)."""
    name = str(path).rsplit("/", 1)[-1]
    for suf in (TEXT_SUFFIX, ".tmjx"):
        if name.endswith(suf):
            return name[:-len(suf)]
    return name.rsplit(".", 1)[0]
