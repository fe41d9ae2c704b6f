"""CPU: bench.py --dump-outputs writes what the last timed training step computed (bench.dump_outputs on a learner over StubEnv, its roll-out
buffers filled by the test), and bench.py refuses a step count that would time nothing."""
import os

import numpy as np
import pytest
import torch

from tests.common import StubEnv

_T, _NLOC, _OBS, _REF, _NU = 4, 512, 24, 16, 3
_NETS = dict(encoder_layers=[16, 16], decoder_layers=[16, 16], critic_layers=[16, 16], latents=4)


def _bench():
    had = "HSA_ENABLE_IPC_MODE_LEGACY" in os.environ
    import bench
    if not had:                     # (bench.py sets it for the ranks it starts; this process keeps its own environment)
        os.environ.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
    return bench


def _learner():
    from track_mjx_amd.agent.ppo import PPOLearner
    ln = PPOLearner(StubEnv(_NLOC, _OBS, _REF, _NU), **_NETS, unroll_length=_T, batch_size=256, num_minibatches=8, num_updates_per_batch=1,
                    use_graph=False, seed=3)
    g = torch.Generator().manual_seed(7)
    for v in ln.buf.values():
        v.copy_(torch.randn(v.shape, generator=g))
    return ln


def test_dump_outputs_writes_the_step_as_float32_with_a_seeded_row_sample(tmp_path):
    bench = _bench()
    ln = _learner()
    rows = ln.buf["reward"].shape[1]
    assert rows > bench.DUMP_ROWS          # the sample is a strict subset
    metrics = {k: torch.tensor(float(i) + 0.5) for i, k in enumerate(ln.METRIC_KEYS)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), ln, metrics)
    bench.dump_outputs(str(tmp_path / "b"), ln, metrics)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(f"{k}.npy" for k in shapes)
    assert {f"metric.{k}.npy" for k in ln.METRIC_KEYS} <= set(files)
    assert {f"policy.{n}.npy" for n, _ in ln.policy.named_parameters()} <= set(files)
    assert {f"value.{n}.npy" for n, _ in ln.value.named_parameters()} <= set(files)
    assert {"normalizer.mean.npy", "normalizer.std.npy", "normalizer.count.npy"} <= set(files)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f        # same learner state -> identical files (the row sample is fixed)
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    for i, k in enumerate(ln.METRIC_KEYS):
        assert np.load(tmp_path / "a" / f"metric.{k}.npy") == np.float32(i + 0.5)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "policy.fc2.weight.npy"), ln.policy.fc2.weight.detach().numpy())
    pick = np.sort(np.random.default_rng(0).choice(rows, bench.DUMP_ROWS, replace=False))
    assert len(np.unique(pick)) == bench.DUMP_ROWS
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rollout.reward.npy"), ln.buf["reward"].numpy()[:, pick])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rollout.raw_action.npy"), ln.buf["raw_action"].numpy()[:, pick])
    obs = np.load(tmp_path / "a" / "rollout.observation.npy")
    assert obs.shape == (_T, bench.DUMP_OBS_ROWS, _OBS)
    np.testing.assert_array_equal(obs, ln.buf["observation"].numpy()[:, pick[:bench.DUMP_OBS_ROWS]])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rollout.next_observation_last.npy"),
                                  ln.buf["next_observation_last"].numpy()[pick[:bench.DUMP_OBS_ROWS]])


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_steps_that_time_nothing(args):
    bench = _bench()
    with pytest.raises(SystemExit) as e:
        bench.main(args)
    assert e.value.code == 2
