"""Rodent walker: host-side mirror of the reference walker interface.

Reference: track_mjx/environment/walker/rodent.py:16-114 (constructor arguments, name -> id
tables) and walker/base.py:70-88 (index properties).  The MuJoCo compile step is replaced by
pre-compiled model blobs (tools/compile_model.py), one per (torque_actuators, rescale_factor)
pair in `BLOBS` (binary `.tmjx`, or its lossless text form `.tmjx.txt`: blob.py; the sensor entries, when the model has sensors, in the text
side file `<stem>.sensors.tmjx.txt`, the render tables in `<stem>.render.tmjx.txt`, both appended to the loaded entries):
  - (True, 0.9)  `assets/rodent_model.tmjx`: the torque-actuator rewrite and the 0.9 rescale of
    rodent-full-clips.yaml:116-117 (the default walker of both named configurations);
  - (False, 0.8) `assets/rodent_model_pos080.tmjx.txt`: rodent.xml's position servos kept as written
    (affine bias: force = gain * act + b0 + b1 * length) and the 0.8 rescale of
    rodent-sps-per-actor.yaml:108-109.
"""
from __future__ import annotations

from collections import OrderedDict
from pathlib import Path
from typing import Sequence

import numpy as np

from . import blob as _blob

_ASSETS = Path(__file__).parent / "assets"

# (torque_actuators, rescale_factor) -> model blob under assets/ (with <stem>.names.txt and <stem>_dump.txt beside it)
BLOBS = {
    (True, 0.9): "rodent_model.tmjx",
    (False, 0.8): "rodent_model_pos080.tmjx.txt",
}


def blob_file(torque_actuators: bool, rescale_factor: float) -> str:
    for (tq, s), fname in BLOBS.items():
        if bool(torque_actuators) == tq and abs(float(rescale_factor) - s) <= 1e-12:
            return fname
    have = ", ".join(f"(torque_actuators={tq}, rescale_factor={s})" for tq, s in BLOBS)
    raise NotImplementedError(
        f"no model blob is compiled for torque_actuators={torque_actuators}, rescale_factor={rescale_factor} (shipped: {have}); "
        f"compile one with: python tools/compile_model.py --rescale {rescale_factor}"
        + ("" if torque_actuators else " --no-torque --affine-bias")
        + f" --out track_mjx_amd/assets/<stem>.tmjx.txt, and add it to walker.BLOBS")


class Rodent:
    def __init__(self, joint_names: Sequence[str], body_names: Sequence[str], end_eff_names: Sequence[str],
                 *, torque_actuators: bool = False, rescale_factor: float = 0.9):
        fname = blob_file(torque_actuators, rescale_factor)
        self.torque_actuators = bool(torque_actuators)
        self.rescale_factor = float(rescale_factor)
        self.actuator_mode = "torque" if self.torque_actuators else "position"
        self.blob_path = _ASSETS / fname
        self._torso_name = "torso"
        self._joint_names = list(joint_names)
        self._body_names = list(body_names)
        self._end_eff_names = list(end_eff_names)
        self.model = _blob.load(self.blob_path)
        # render tables (tools/compile_model.py render_entries): the text side file <stem>.render.tmjx.txt, appended behind the blob's own entries and in front of the sensor entries, which stay last
        rend = _ASSETS / f"{_blob.stem(fname)}.render{_blob.TEXT_SUFFIX}"
        if rend.exists():
            extra = _blob.load(rend)
            clash = [k for k in extra if k in self.model]
            if clash:
                raise ValueError(f"{rend.name}: entries {clash} are already in {fname}")
            self.model.update(extra)
        # sensors (tools/compile_model.py sensor_entries): a text side file <stem>.sensors.tmjx.txt appended behind the blob's own entries
        sens = _ASSETS / f"{_blob.stem(fname)}.sensors{_blob.TEXT_SUFFIX}"
        if sens.exists():
            extra = _blob.load(sens)
            clash = [k for k in extra if k in self.model]
            if clash:
                raise ValueError(f"{sens.name}: entries {clash} are already in {fname}")
            self.model.update(extra)
        self.names = {"body": {}, "joint": {}, "actuator": {}, "site": {}, "sensor": {}}   # site / sensor: blobs that carry sensors
        with open(_ASSETS / f"{_blob.stem(fname)}.names.txt") as f:
            for line in f:
                kind, idx, name = line.split()
                self.names[kind][name] = int(idx)
        dims = self.model["dims"]
        self.nbody, self.njnt, self.nq, self.nv, self.nu, self.ncon = (int(x) for x in dims)
        self._initialize_indices()

    def sensor_table(self) -> "list[tuple[str, int, int]]":
        """(name, sensordata address, width) of every sensor of the blob in sensordata order; [] for a blob without sensors."""
        if "sensor_adr" not in self.model:
            return []
        names = sorted(self.names["sensor"], key=self.names["sensor"].get)
        adr = [int(a) for a in self.model["sensor_adr"]]
        ends = adr[1:] + [self.nsensordata]
        return [(n, a, e - a) for n, a, e in zip(names, adr, ends)]

    def render_table(self) -> "dict[str, np.ndarray]":
        """The visible geoms of the blob in XML order: body, type, group [n], size, pos [n, 3], quat, rgba [n, 4]; {} for a blob without
        render tables."""
        if "rgeom_type" not in self.model:
            return {}
        n = len(self.model["rgeom_type"])
        out = {k: np.asarray(self.model[f"rgeom_{k}"]) for k in ("body", "type", "group")}
        out.update({k: np.asarray(self.model[f"rgeom_{k}"], np.float64).reshape(n, w) for k, w in (("size", 3), ("pos", 3), ("quat", 4), ("rgba", 4))})
        return out

    def cameras(self) -> "dict[str, dict]":
        """name -> {body, mode ('fixed' | 'track' | 'trackcom'), pos, quat (body-local), fovy (degrees), off0, wquat0 (a trackcom camera's world
        offset from its body's subtree centre of mass and world orientation at qpos0)}, in XML order; {} for a blob without cameras."""
        if "rcam_name" not in self.model:
            return {}
        names = np.asarray(self.model["rcam_name"]).reshape(-1, 32)
        modes = {0: "fixed", 1: "track", 2: "trackcom"}
        out = {}
        for i, row in enumerate(names):
            name = bytes(int(c) for c in row if c).decode()
            out[name] = dict(body=int(self.model["rcam_body"][i]), mode=modes[int(self.model["rcam_mode"][i])],
                             pos=np.asarray(self.model["rcam_pos"], np.float64).reshape(-1, 3)[i],
                             quat=np.asarray(self.model["rcam_quat"], np.float64).reshape(-1, 4)[i], fovy=float(self.model["rcam_fovy"][i]),
                             off0=np.asarray(self.model["rcam_off0"], np.float64).reshape(-1, 3)[i],
                             wquat0=np.asarray(self.model["rcam_wquat0"], np.float64).reshape(-1, 4)[i])
        return out

    @property
    def nsensordata(self) -> int:
        """Floats of sensordata per env (every supported sensor type is 3 wide: tools/compile_model.py SENSOR_DIM)."""
        return 3 * len(self.model["sensor_adr"]) if "sensor_adr" in self.model else 0

    def _initialize_indices(self) -> None:
        self._joint_idxs = np.array([self.names["joint"][j] for j in self._joint_names], dtype=np.int32)
        self._body_idxs = np.array([self.names["body"][b] for b in self._body_names], dtype=np.int32)
        self._endeff_idxs = np.array([self.names["body"][e] for e in self._end_eff_names], dtype=np.int32)
        self._torso_idx = int(self.names["body"][self._torso_name])

    def describe(self) -> str:
        """One line naming the walker: actuator mode, scale, blob file."""
        return f"walker: rodent, {self.actuator_mode} actuators, rescale_factor={self.rescale_factor:g}, model blob {self.blob_path.name}"

    joint_idxs = property(lambda self: self._joint_idxs)
    body_idxs = property(lambda self: self._body_idxs)
    endeff_idxs = property(lambda self: self._endeff_idxs)
    torso_idx = property(lambda self: self._torso_idx)


def build_blob(walker: Rodent, *, n_frames: int, iterations: int, ls_iterations: int, timestep: float,
               mocap_hz: int, clip_length: int, traj_length: int, window: int, episode_length: int,
               reward_f: np.ndarray, tolerance: float = 1e-8, ls_tolerance: float = 0.01,
               impratio: float = 1.0, auto_reset: bool = True) -> bytes:
    """Model constants + env/task configuration -> the blob `tmjx_model_create` consumes."""
    e = OrderedDict(walker.model)
    e["opt_f"] = np.array([timestep, tolerance, ls_tolerance, impratio], dtype=np.float64)
    e["opt_i"] = np.array([iterations, ls_iterations, n_frames], dtype=np.int32)
    e["env_i"] = np.array([mocap_hz, clip_length, traj_length, window, walker.torso_idx, episode_length, int(auto_reset)], dtype=np.int32)
    e["joint_idxs"] = walker.joint_idxs
    e["body_idxs"] = walker.body_idxs
    e["endeff_idxs"] = walker.endeff_idxs
    e["reward_f"] = np.asarray(reward_f, dtype=np.float64)
    return _blob.pack(e)
