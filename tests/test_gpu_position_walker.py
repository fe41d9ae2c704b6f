"""GPU: the position-actuator, 0.8-scale rodent (walker.BLOBS (False, 0.8): affine actuator bias) on the HIP kernels.

  * teacher-forced single substeps at full launch size (4096 envs in bench.py's three env groups) for the product kernel and the
    generic-tree kernel (TMJX_WAVE_DYNAMIC=1), three action scales, against the UNMODIFIED float64 / float32 oracles with the bias
    substituted into the activation (tests/affine_bias.py); the qfrc_actuator row against the numpy restatement, act against the filter;
  * reward / observation (K3) on arbitrary states of the position walker against the oracle's reward/obs stage; reset, step, auto-reset;
  * two PPO training steps through train.main with `--config-name rodent-sps-per-actor` and the two walker overrides;
  * the lane-per-env cross-check build refuses the bias model (it has no bias path).
"""
import numpy as np
import pytest
import torch

from tests.affine_bias import POS_OVERRIDES, Actuation, collect, oracle_substep, position_config
from tests.common import PHYS_ROWS, make_oracle, rel_err, spread_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _groups(n=4096):
    from track_mjx_amd import clips as _clips
    from track_mjx_amd.agent import ppo
    from track_mjx_amd.environment import wrap
    from track_mjx_amd.train import build_env
    from track_mjx_amd.walker import Rodent
    cfg = position_config()
    w = Rodent(**cfg["walker_config"])
    table = _clips.make_synthetic_clips(w.model, 64, n_frames=cfg["reference_config"]["clip_length"], mocap_hz=cfg["env_config"]["env_args"]["mocap_hz"])
    sizes = ppo.group_sizes(n, 3)
    assert sizes == [1368, 1364, 1364]
    envs = [wrap(build_env(cfg, sizes[0], DEV, reference_clip=table), episode_length=195)]
    envs += [wrap(build_env(cfg, sz, DEV, reference_clip=table, share_clips_with=envs[0]), episode_length=195) for sz in sizes[1:]]
    return w, cfg, table, envs


@pytest.mark.parametrize("variant", ["product", "generic"])
def test_full_launch_substeps_against_the_substituted_oracle(variant, monkeypatch):
    if variant == "generic":
        monkeypatch.setenv("TMJX_WAVE_DYNAMIC", "1")
    w, cfg, table, envs = _groups()
    assert all(e.walker.actuator_mode == "position" for e in envs)
    A = Actuation(w.model)
    h = cfg["env_config"]["env_args"]["mj_model_timestep"]
    O32, O64 = make_oracle(envs[0]._blob, table, "f32"), make_oracle(envs[0]._blob, table, "f64")
    g = torch.Generator().manual_seed(3)
    states = [env.reset(g) for env in envs]
    for s in range(3):          # into contact, on the product path
        for k, env in enumerate(envs):
            states[k] = env.step(states[k], (torch.randn((38, env.num_envs), generator=g) * 0.5).clamp(-1, 1).to(DEV))
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    errs = {k: ([], []) for k in ("qpos", "qvel")}
    qfrc_err, act_err = [], []
    for scale in (0.03, 0.3, 1.0):
        for _ in range(2):
            for env in envs:
                n = env.num_envs
                idx = spread_sample(n, 22)
                ti = torch.as_tensor(idx, device=env.device)
                st = {k: env.rows(k)[:, ti].cpu().numpy().astype(np.float64) for k in PHYS_ROWS}
                ok = [j for j in range(len(idx)) if all(np.isfinite(st[k][:, j]).all() for k in PHYS_ROWS)]
                a = np.clip(rng.normal(size=(38, n)) * scale, -1, 1).astype(np.float32)
                env.physics(torch.from_numpy(a).to(env.device), 1)
                torch.cuda.synchronize()
                got = {k: env.rows(k)[:, ti].cpu().numpy() for k in ("qpos", "qvel", "act", "qfrc_actuator")}
                for j in ok:
                    s1 = {k: v[:, j] for k, v in st.items()}
                    ctrl = a[:, idx[j]]
                    ref = A.qfrc_actuator(s1["act"], s1["qpos"])
                    qfrc_err.append(np.abs(got["qfrc_actuator"][:, j] - ref).max() / np.abs(ref).max())
                    act_err.append(np.abs(got["act"][:, j] - A.next_act(s1["act"], ctrl, h)).max())
                    r64 = oracle_substep(O64, A, s1, ctrl)
                    if not all(np.isfinite(v).all() for v in r64.values()):
                        continue
                    collect(errs, {k: got[k][:, j] for k in ("qpos", "qvel")}, r64, oracle_substep(O32, A, s1, ctrl))
    assert max(qfrc_err) <= 1e-5, max(qfrc_err)
    assert max(act_err) <= 1e-6, max(act_err)
    fac = 1.0 if variant == "product" else 4.0      # the generic path's plain float32 factorisation (tests/test_hostemu_parity.py)
    for k, (gl, fl) in errs.items():
        gv, fv = np.array(gl), np.array(fl)
        fin = np.isfinite(fv)
        assert fin.sum() >= 300 and np.isfinite(gv[fin]).all(), (k, fin.sum())
        gv, fv = gv[fin], fv[fin]
        print(f"\n{variant} {k}: {len(gv)} env-substeps, median {np.median(gv):.2e} (f32 oracle {np.median(fv):.2e}), "
              f"q99 {np.quantile(gv, 0.99):.2e} ({np.quantile(fv, 0.99):.2e}), worst {gv.max():.2e} ({fv.max():.2e})")
        assert np.median(gv) <= 1e-5, (k, np.median(gv))
        assert np.median(gv) <= 2 * fac * np.median(fv) + 1e-7, (k, np.median(gv), np.median(fv))
        assert np.quantile(gv, 0.99) <= 3 * fac * np.quantile(fv, 0.99) + 1e-5, (k, np.quantile(gv, 0.99), np.quantile(fv, 0.99))
        assert gv.max() <= 4 * fac * fv.max() + 1e-4, (k, gv.max(), fv.max())


def _env(n, episode_length=195):
    from track_mjx_amd import clips as _clips
    from track_mjx_amd.environment import MultiClipTracking, RewardConfig, wrap
    from track_mjx_amd.walker import Rodent
    cfg = position_config()
    w = Rodent(**cfg["walker_config"])
    cl = _clips.make_synthetic_clips(w.model, 4, seed=0)
    env = MultiClipTracking(cl, w, RewardConfig(**cfg["env_config"]["reward_weights"]), **cfg["env_config"]["env_args"], **cfg["reference_config"],
                            num_envs=n, device=DEV)
    env = wrap(env, episode_length=episode_length)
    return env, make_oracle(env._blob, cl, "f32"), cl


def test_reward_obs_on_position_walker_states():
    """K3 alone on arbitrary state rows of the position walker (qfrc_actuator among them) against the oracle's reward/obs stage."""
    n = 64
    env, O, cl = _env(n)
    rng = np.random.default_rng(7)
    g = torch.Generator().manual_seed(7)
    clip_t = torch.randint(0, 4, (n,), generator=g, dtype=torch.int32); start_t = torch.randint(0, 44, (n,), generator=g, dtype=torch.int32)
    env.reset(g, clip_t, start_frame=start_t, qpos_noise=torch.zeros((74, n)), qvel_noise=torch.zeros((73, n)))
    envs = O.new_envs(n)
    clip = clip_t.numpy(); start = start_t.numpy()
    L = env.layout
    vals = {"qpos": rng.normal(size=(74, n)) * 0.3, "qvel": rng.normal(size=(73, n)), "xpos": rng.normal(size=(204, n)) * 0.1,
            "qfrc_actuator": rng.normal(size=(73, n)), "time": rng.integers(0, 190, size=(1, n)) * np.float32(0.01)}
    xmat = rng.normal(size=(9, n))
    # odd envs: the pose the reset put them in (arbitrary velocities and actuator forces): these are not terminated, so their reward / observation
    # are the step's own; even envs: arbitrary rows everywhere (terminated, auto-reset)
    near = np.arange(n) % 2 == 1
    for k in ("qpos", "xpos"):
        vals[k][:, near] = env.rows(k).cpu().numpy()[:, near]
    xmat[:, near] = env.rows("xmat_torso").cpu().numpy()[:, near]
    vals["time"][:, near] = 0.0
    buf = rng.uniform(-1, 1, size=(50 * 38, n)); bidx = rng.integers(0, 50, size=n)
    for k, v in vals.items():
        env.rows(k).copy_(torch.from_numpy(v.astype(np.float32)))
    env.rows("xmat_torso").copy_(torch.from_numpy(xmat.astype(np.float32)))
    env.state_buf[L.action_buffer:L.action_buffer + 1900].copy_(torch.from_numpy(buf.astype(np.float32)))
    env.istate_buf[L.i_buffer_index].copy_(torch.from_numpy(bidx.astype(np.int32)))
    a = rng.uniform(-1, 1, size=(38, n)).astype(np.float32)
    zero = np.zeros(74)
    for e in range(n):
        O.env_reset(envs, e, int(clip[e]), int(start[e]), zero, zero[:73])
        for k, v in vals.items():
            O.env_set(envs, e, k, v[:, e].astype(np.float32))
        xm = np.zeros(68 * 9); xm[3 * 9:4 * 9] = xmat[:, e].astype(np.float32)
        O.env_set(envs, e, "xmat", xm)
        O.env_set(envs, e, "action_buffer", buf[:, e].astype(np.float32)); O.env_set(envs, e, "buffer_index", [bidx[e]])
        O.env_post(envs, e, a[:, e])
    st = env.reward_obs(torch.from_numpy(a).to(DEV)); torch.cuda.synchronize()
    done_o = np.array([O.env_get(envs, e, "done")[0] for e in range(n)])
    obs_o = np.stack([O.env_get(envs, e, "obs") for e in range(n)], 0)
    rew_o = np.array([O.env_get(envs, e, "reward")[0] for e in range(n)])
    assert (st.done.cpu().numpy() == done_o).all()
    # a done env is overwritten by its reset snapshot on both sides; the snapshots differ by design: the observation carries qfrc_actuator,
    # which at reset (act = 0) is the bias alone on the GPU and zero in the oracle (no bias path).  Done envs are compared with their own snapshot
    keep = done_o == 0
    assert keep.sum() >= 16 and (~keep).sum() >= 16, keep.sum()
    obs = st.obs.cpu().numpy()
    assert rel_err(obs[keep], obs_o[keep]) < 1e-5
    assert np.array_equal(obs[~keep], st.info["first_obs"].cpu().numpy()[~keep])
    assert np.abs(st.reward.cpu().numpy() - rew_o).max() < 1e-4 * max(1.0, np.abs(rew_o).max())


def test_reset_step_autoreset_on_position_walker():
    """wrap(env): reset, steps through the episode limit, auto-reset back to the snapshot; the reset's qfrc_actuator row carries the bias."""
    n = 256
    env, _, _ = _env(n, episode_length=4)
    A = Actuation(env.walker.model)
    g = torch.Generator().manual_seed(1)
    st = env.reset(g)
    torch.cuda.synchronize()
    q0, a0 = env.rows("qpos").cpu().numpy().astype(np.float64), env.rows("act").cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(env.rows("qfrc_actuator").cpu().numpy(), A.qfrc_actuator(a0, q0), rtol=1e-5, atol=1e-5 * np.abs(A.qfrc_actuator(a0, q0)).max())
    assert np.abs(A.qfrc_actuator(a0, q0)).max() > 1e-3           # act = 0 at reset: the force is the bias alone
    first_obs = st.obs.clone()
    was_done = torch.zeros(n, dtype=torch.bool, device=DEV)
    for s in range(4):
        st = env.step(st, (torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1).to(DEV))
        torch.cuda.synchronize()
        assert torch.isfinite(st.obs).all() and torch.isfinite(st.reward).all()
        done = st.done > 0
        assert torch.equal(st.obs[done], first_obs[done])        # a done env is back at its reset snapshot
        if s < 3:
            was_done |= done
    # the 4th step hits the episode limit: every env that ran its whole episode is done (truncated) and auto-reset
    assert bool((st.done[~was_done] == 1).all()) and int((~was_done).sum()) > 0
    assert float(st.info["truncation"].sum()) > 0


def test_train_entrypoint_trains_the_position_walker(tmp_path, capsys):
    """python -m track_mjx_amd.train --config-name rodent-sps-per-actor walker_config.torque_actuators=false walker_config.rescale_factor=0.8:
    the first log line names the walker; two PPO training steps leave finite parameters and losses."""
    import json
    from track_mjx_amd import train
    d = tmp_path / "ck"
    train.main(["--config-name", "rodent-sps-per-actor", *POS_OVERRIDES,
                "train_setup.train_config.num_envs=256", "train_setup.train_config.batch_size=64", "train_setup.train_config.num_minibatches=4",
                "train_setup.train_config.unroll_length=5", "train_setup.train_config.num_updates_per_batch=2", "network_config.encoder_layer_sizes=[64,64]",
                "network_config.decoder_layer_sizes=[64,64]", "network_config.critic_layer_sizes=[64,64]", "train_setup.train_config.num_timesteps=6400",
                "train_setup.eval_every=640", "train_setup.reset_every=640", "n_synthetic_clips=4", "train_setup.train_config.num_eval_envs=0",
                f"checkpoint_path={d}", "max_training_steps=2"])
    out = capsys.readouterr().out
    first = out.splitlines()[0]
    assert first.startswith("[train] config=rodent-sps-per-actor") and "position actuators" in first and "rodent_model_pos080.tmjx.txt" in first, first
    assert "nan" not in out.lower().replace("nan_count", "")
    cfg = json.loads((d / "2" / "config" / "metadata").read_text())
    assert cfg["walker_config"]["torque_actuators"] is False and cfg["walker_config"]["rescale_factor"] == 0.8
    with np.load(d / "2" / "train_state.npz") as z:
        floats = [k for k in z.files if z[k].dtype.kind == "f"]
        assert len(floats) > 10 and all(np.isfinite(z[k]).all() for k in floats), [k for k in floats if not np.isfinite(z[k]).all()]
        assert int(z["iteration"]) == 2


def test_lane_build_refuses_the_bias_model(monkeypatch):
    import ctypes as C
    from pathlib import Path
    from tests.common import default_blob
    from track_mjx_amd import hip
    from track_mjx_amd.walker import Rodent
    so = Path(__file__).resolve().parent / "lane" / "libtmjx_hip_lane.so"
    L = hip.load(so)
    cfg = position_config()
    blob = default_blob(Rodent(**cfg["walker_config"]), cfg)
    monkeypatch.setenv("TMJX_IMPL", "lane")
    h = C.c_void_p()
    rc = L.tmjx_model_create(blob, len(blob), C.byref(h))
    assert rc == -22, rc                                              # TMJX_EINVAL (include/tmjx.h)
    assert b"bias" in L.tmjx_last_error()
    monkeypatch.delenv("TMJX_IMPL")
    rc = L.tmjx_model_create(blob, len(blob), C.byref(h))             # the same build's wave kernel takes it
    assert rc == 0, L.tmjx_last_error()
    L.tmjx_model_destroy(h)
