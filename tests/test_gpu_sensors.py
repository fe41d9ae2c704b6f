"""GPU: the recording physics kernel (k_physics_wave_sensors: tmjx_step_sensors / tmjx_physics_sensors) and log_sensor_data roll-outs — the same
state / obs / reward bits as tmjx_step, sensor outputs against the host emulation of the same kernel body, the keys and shapes of the reference's
roll-out dict, batch independence, and the CLI's .h5 datasets."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.common import make_env_and_oracle, spread_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]


def _envs(n):
    out = []
    for _ in range(2):
        env, _, cl = make_env_and_oracle(num_envs=n, wrappers=False, seed=0)
        env.reset(torch.Generator().manual_seed(1))
        out.append(env)
    return out, cl


def test_step_sensors_is_step_bit_for_bit():
    """4096 envs, 6 control steps: tmjx_step_sensors leaves state, obs, reward, done, truncation and metrics bit-identical to tmjx_step, and
    writes finite sensor outputs (the world body's cfrc_ext row exactly 0)."""
    n = 4096
    (a, b), _ = _envs(n)
    sd, cf = b.sensor_buffers()
    assert sd.shape == (12, n) and cf.shape == (68 * 6, n)
    g = torch.Generator().manual_seed(4)
    for _ in range(6):
        act = (torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1).to(DEV)
        a.step(None, act)
        b.step_sensors(act.contiguous(), sd, cf)
        torch.cuda.synchronize()
        for name in ("state_buf", "istate_buf", "obs_buf", "reward_buf", "done_buf", "trunc_buf", "metrics_buf"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), name
        fin = torch.isfinite(b.rows("qpos")).all(0)
        assert fin.sum() > n * 0.9
        assert torch.isfinite(sd[:, fin]).all() and torch.isfinite(cf[:, fin]).all()
        assert torch.all(cf[:6] == 0)
    assert (cf[6:].abs().amax(0) > 0).sum() > 0, "no env in contact"


def test_sensor_outputs_vs_host_emulation():
    """One substep of 1024 envs through tmjx_physics_sensors against the host emulation of the same kernel body (tests/hostemu/sensors_emu.cpp)
    on sampled envs, from the same starting state.  GPU and emulation differ in fp32 rounding only (FMA contraction, reduction order); the
    bound is 1e-3 of each sensor's / cfrc_ext's scale over the sample (measured: accelerometer 1.0e-4, the velocity sensors <= 1.3e-6,
    cfrc_ext 1.9e-4 — the accelerations and contact forces go through the solver, whose fp32 rounding differs).  Then the no-contact invariants: raised 0.5 with zero velocity, cfrc_ext and the velocity sensors are 0."""
    sys.path.insert(0, str(ROOT / "tests" / "hostemu"))
    from emu import Emu
    from sensors_emu import SensorEmu
    n = 1024
    (env, _), _ = _envs(n)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        env.step(None, (torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1).to(DEV))
    idx = spread_sample(n, 24)
    names = ("qpos", "qvel", "act", "qacc_warmstart", "time")
    torch.cuda.synchronize()
    pre = {k: env.rows(k)[:, idx].cpu().numpy().copy() for k in names}
    act = (torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1).to(DEV).contiguous()
    sd, cf = env.sensor_buffers()
    env.physics_sensors(act, 1, sd, cf)
    torch.cuda.synchronize()
    gsd, gcf = sd[:, idx].cpu().numpy(), cf[:, idx].cpu().numpy()
    E, S = Emu(env._blob, len(idx)), SensorEmu(env._blob)
    for k in names:
        E.rows(k)[:] = pre[k]
    esd, ecf = S.physics(E, act[:, idx].cpu().numpy(), 1)
    ok = np.isfinite(pre["qvel"]).all(0) & (np.abs(pre["qvel"]).max(0) < 50)
    assert ok.sum() >= len(idx) // 2
    e_s = np.abs(gsd - esd)[:, ok].reshape(4, 3, -1).max(axis=(1, 2)) / (np.abs(esd[:, ok]).reshape(4, 3, -1).max(axis=(1, 2)) + 1e-12)
    e_c = np.abs(gcf - ecf)[:, ok].max() / (np.abs(ecf[:, ok]).max() + 1e-12)
    print(f"GPU vs emulation: sensors {e_s}, cfrc_ext {e_c:.3g}")
    assert e_s.max() < 1e-3 and e_c < 1e-3, (e_s, e_c)
    # no contact, no motion (envs whose state is finite: an untrained random action sequence blows a few up, as it would in MJX)
    env.rows("qpos")[2] += 0.5
    env.rows("qvel").zero_()
    fin = torch.isfinite(env.rows("qpos")).all(0) & torch.isfinite(env.rows("act")).all(0)
    assert fin.sum() > n * 0.9
    env.physics_sensors(None, 1, sd, cf)
    torch.cuda.synchronize()
    free = fin & (env.rows("con_dist") > 0).all(0)         # (the launch's own contact distances: no slot penetrating)
    print(f"raised: {int(fin.sum())} finite envs, {int(free.sum())} without a penetrating contact slot")
    assert free.sum() > n * 0.8
    assert torch.all(cf[:, free] == 0)
    assert torch.all(sd[3:, fin] == 0) and torch.isfinite(sd[:3, fin]).all()


def test_sensor_entries_refuse_bad_buffers():
    (env, _), _ = _envs(64)
    sd, cf = env.sensor_buffers()
    with pytest.raises(ValueError, match="cfrc_ext"):
        env.physics_sensors(None, 1, sd, cf[:10])
    with pytest.raises(ValueError, match="sensordata"):
        env.physics_sensors(None, 1, None, cf)
    from track_mjx_amd import hip as _hip
    L = _hip.lib()
    assert L.tmjx_physics_sensors(env._handle, env.state_buf.data_ptr(), None, 1, sd.data_ptr(), None, None, 64, None) == -22
    assert b"cfrc_ext" in L.tmjx_last_error()
    assert L.tmjx_physics_sensors(env._handle, env.state_buf.data_ptr(), None, 0, sd.data_ptr(), cf.data_ptr(), None, 64, None) == -22


# ---------------------------------------------------------------------------------------------------------------- roll-outs
from tests.test_gpu_rollout import lstm_ckpt, mlp_ckpt  # noqa: E402,F401  (the roll-out tests' checkpoint fixtures)


def _gens(path):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import create_environment, create_rollout_generator
    cfg = ck.load_config_from_checkpoint(path)
    fn = ck.load_inference_fn(cfg, ck.load_policy(path, cfg))
    env = create_environment(cfg, 1, DEV)
    plain = create_rollout_generator(cfg, env, fn, model=fn.model)
    sens = create_rollout_generator(cfg, env, fn, model=fn.model, log_sensor_data=True)
    return plain, sens


@pytest.mark.parametrize("which", ["mlp", "lstm"])
def test_rollout_log_sensor_data(which, mlp_ckpt, lstm_ckpt):  # noqa: F811
    path = (mlp_ckpt if which == "mlp" else lstm_ckpt)[0]
    plain, sens = _gens(path)
    T = sens.T
    r = sens(3)
    assert set(r) == {"qposes_ref", "qposes_rollout", "ctrl", "state_rewards", "joint_forces", "sensor_readings"}
    assert r["joint_forces"].shape == (T - 1, 68, 6) and r["sensor_readings"].shape == (T - 1, 12)
    assert r["joint_forces"].dtype == np.float32 and np.isfinite(r["joint_forces"][:50]).all() and np.isfinite(r["sensor_readings"][:50]).all()
    assert np.all(r["joint_forces"][:, 0] == 0)
    p = plain(3)
    for k in ("qposes_rollout", "ctrl", "state_rewards", "qposes_ref"):
        assert np.array_equal(r[k], p[k], equal_nan=True), k
    # a clip alone and the same clip inside a batch
    clips = [0, 3, 5, 1]
    rb = sens(clips)
    assert rb["joint_forces"].shape == (4, T - 1, 68, 6) and rb["sensor_readings"].shape == (4, T - 1, 12)
    for k in ("joint_forces", "sensor_readings", "qposes_rollout"):
        assert np.array_equal(rb[k][1], r[k], equal_nan=True), k


def test_cli_writes_sensor_datasets(tmp_path, mlp_ckpt):  # noqa: F811
    from track_mjx_amd.analysis.utils import load_from_h5py
    out = tmp_path / "rollouts"
    res = subprocess.run([sys.executable, "-m", "track_mjx_amd.analysis.rollout", f"checkpoint={mlp_ckpt[0]}", "clips=0:2", f"out={out}",
                          "log_sensor_data=true", "log_activations=false"], capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    _, sens = _gens(mlp_ckpt[0])
    for c in (0, 1):
        got = load_from_h5py(out / f"clip_{c}.h5")
        want = sens(c, seed=42)
        assert got["joint_forces"].shape == want["joint_forces"].shape and got["sensor_readings"].shape == want["sensor_readings"].shape
        assert np.array_equal(got["joint_forces"], want["joint_forces"], equal_nan=True)
        assert np.array_equal(got["sensor_readings"], want["sensor_readings"], equal_nan=True)
        meta = got["meta"]
        assert bytes(meta["sensor_names"]) == b"accelerometer,velocimeter,gyro,torso"
        assert list(meta["sensor_adr"]) == [0, 3, 6, 9]
        assert b"cfrc_ext" in bytes(meta["joint_forces_convention"])
