"""The LSTM-decoder-dynamics calls on the CPU: track_mjx_amd.analysis.backend.Backend on numpy arrays against the TEST-ONLY host emulation
tests/hostemu/lstm_dynamics_emu.cpp (a library of its own: the LSTM Jacobian, Jacobian, comparison and analysis emulations plus
tmjx_lstm_tangent_workspace, tmjx_lstm_tangent_step and tmjx_lstm_lyapunov).  `B` is that backend; `over` is analysis_emu's, on this library."""
from __future__ import annotations

from pathlib import Path

from tests.hostemu import analysis_emu as E
from tests.hostemu import loader
from track_mjx_amd.analysis.backend import Backend

SOURCE = "lstm_dynamics_emu.cpp"
ARRAYS = E.NumpyArrays(loader.load(SOURCE))
B = Backend(ARRAYS)


def over(entry: str, **substitutes) -> Backend:
    """analysis_emu.over on this library's backend."""
    return E.over(entry, on=B, **substitutes)


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main behind -DLSTM_DYNAMICS_EMU_MAIN)."""
    return loader.build_main(SOURCE, "LSTM_DYNAMICS_EMU_MAIN", out, flags)
