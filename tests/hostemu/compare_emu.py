"""The representation-comparison calls on the CPU: track_mjx_amd.analysis.backend.Backend on numpy arrays against the TEST-ONLY host emulation
tests/hostemu/compare_emu.cpp (a library of its own: the analysis emulation plus tmjx_compare_workspace, tmjx_cka_linear, tmjx_rdm_corr, tmjx_cca
and tmjx_compare_svd).  `B` is that backend; `over` and `workspace` are analysis_emu's, on this library."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

from tests.hostemu import analysis_emu as E
from tests.hostemu import loader
from track_mjx_amd.analysis.backend import Backend

SOURCE = "compare_emu.cpp"
ARRAYS = E.NumpyArrays(loader.load(SOURCE))
B = Backend(ARRAYS)


def over(entry: str, **substitutes) -> Backend:
    """analysis_emu.over on this library's backend."""
    return E.over(entry, on=B, **substitutes)


def workspace(*dims) -> int:
    """The floats tmjx_compare_workspace reports for (n, d1, d2)."""
    floats = C.c_int64(0)
    ARRAYS.check(ARRAYS.library.tmjx_compare_workspace(*dims, C.byref(floats)), "tmjx_compare_workspace")
    return int(floats.value)


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main behind -DCOMPARE_EMU_MAIN)."""
    return loader.build_main(SOURCE, "COMPARE_EMU_MAIN", out, flags)
