"""Building and loading the TEST-ONLY host emulation libraries of tests/hostemu: one loader for every wrapper here."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

from track_mjx_amd import hip

HERE = Path(__file__).resolve().parent
_loaded: dict = {}


def build(source: str) -> Path:
    """The library of tests/hostemu/<source> (lib<stem>.so beside it), rebuilt when any file the source includes, directly or not, is newer than it."""
    src = HERE / source
    so = HERE / f"lib{src.stem}.so"
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in hip.include_closure(src)):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)], check=True, capture_output=True)
    return so


def load(source: str) -> C.CDLL:
    """`build(source)` loaded, one handle per library; the entry points that carry a C-ABI name get the types of hip.SIGNATURES."""
    so = build(source)
    if so not in _loaded:
        _loaded[so] = hip.declare(C.CDLL(str(so)))      # (ctypes' default binding is local: the product library may be loaded beside it)
    return _loaded[so]


def build_main(source: str, define: str, out: Path, flags=()) -> Path:
    """tests/hostemu/<source> as a stand-alone program (its own main, behind -D<define>), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-std=c++17", f"-D{define}", *flags, "-o", str(out), str(HERE / source)], check=True, capture_output=True)
    return out
