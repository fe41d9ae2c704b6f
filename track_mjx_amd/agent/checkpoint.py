"""Parameter export / import in the reference's flax naming (first half).

The reference checkpoints `(normalizer_params, policy_params)` with orbax (track_mjx/agent/checkpointing.py:165-198); the
policy's flax tree is {'params': {'encoder': {hidden_i, LayerNorm_i, fc2_mean, fc2_logvar}, 'decoder': {hidden_i, LayerNorm_i}}}
(agent/mlp_ppo/intention_network.py:32-44,68-76: Dense kernels are [in, out], LayerNorm has scale / bias, the decoder's last
`hidden_L` is the un-activated output layer) and the value net is brax's MLP {'params': {hidden_i}}.  orbax / tensorstore are not in
this image, so the container here is a flat .npz whose keys are the '/'-joined tree paths — the tree a reference-side loader needs
to hand to orbax, three lines with `flax.traverse_util.unflatten_dict`.  `from_flax_tree` loads such a tree back (e.g. a
reference checkpoint converted the other way), so policies can move in both directions.
"""
from __future__ import annotations

import numpy as np
import torch

from .networks import DecoderNet, IntentionPolicy, RunningStatistics, ValueNet


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def _ident(p):
    return p


LSTM_GATES = "ifgo"          # flax nn.LSTMCell gate order: rows [g H, (g + 1) H) of w_ih / w_hh / b_hh


def _encoder_to_flax(policy, get) -> dict:
    enc = {}
    for i, blk in enumerate(policy.encoder):
        enc[f"hidden_{i}"] = {"kernel": _np(get(blk.dense.weight).t()), "bias": _np(get(blk.dense.bias))}
        enc[f"LayerNorm_{i}"] = {"scale": _np(get(blk.norm.weight)), "bias": _np(get(blk.norm.bias))}
    Z = policy.latents
    w, b = get(policy.fc2.weight), get(policy.fc2.bias)
    enc["fc2_mean"] = {"kernel": _np(w[:Z].t()), "bias": _np(b[:Z])}
    enc["fc2_logvar"] = {"kernel": _np(w[Z:].t()), "bias": _np(b[Z:])}
    return enc


def lstm_policy_to_flax(policy, get=_ident) -> dict:
    """LSTMIntentionPolicy -> the reference's lstm_ppo IntentionNetwork tree: {encoder, lstm_decoder: {lstm_{k}: {ii, if, ig, io: {kernel}, hi, hf,
    hg, ho: {kernel, bias}}, lstm_projection: {kernel, bias}}} (flax kernels are [in, out])."""
    H = policy.hidden_state_size
    dec = {}
    for k in range(policy.hidden_layer_num):
        wi, wh, bh = get(policy.w_ih[k]), get(policy.w_hh[k]), get(policy.b_hh[k])
        cell = {}
        for g, name in enumerate(LSTM_GATES):
            rows = slice(g * H, (g + 1) * H)
            cell["i" + name] = {"kernel": _np(wi[rows].t())}
            cell["h" + name] = {"kernel": _np(wh[rows].t()), "bias": _np(bh[rows])}
        dec[f"lstm_{k}"] = cell
    dec["lstm_projection"] = {"kernel": _np(get(policy.projection.weight).t()), "bias": _np(get(policy.projection.bias))}
    return {"params": {"encoder": _encoder_to_flax(policy, get), "lstm_decoder": dec}}


@torch.no_grad()
def lstm_policy_from_flax(policy, tree: dict, get=_ident) -> None:
    p = tree["params"]
    dev = policy.fc2.weight.device

    def put(dst: torch.Tensor, src) -> None:
        dst.copy_(torch.as_tensor(np.ascontiguousarray(src), dtype=dst.dtype, device=dev))

    _encoder_from_flax(policy, p["encoder"], get, put)
    H = policy.hidden_state_size
    for k in range(policy.hidden_layer_num):
        cell = p["lstm_decoder"][f"lstm_{k}"]
        wi, wh, bh = get(policy.w_ih[k]), get(policy.w_hh[k]), get(policy.b_hh[k])
        for g, name in enumerate(LSTM_GATES):
            rows = slice(g * H, (g + 1) * H)
            put(wi[rows], np.asarray(cell["i" + name]["kernel"]).T)
            put(wh[rows], np.asarray(cell["h" + name]["kernel"]).T)
            put(bh[rows], cell["h" + name]["bias"])
    proj = p["lstm_decoder"]["lstm_projection"]
    put(get(policy.projection.weight), np.asarray(proj["kernel"]).T)
    put(get(policy.projection.bias), proj["bias"])


def _encoder_from_flax(policy, enc: dict, get, put) -> None:
    for i, blk in enumerate(policy.encoder):
        put(get(blk.dense.weight), np.asarray(enc[f"hidden_{i}"]["kernel"]).T)
        put(get(blk.dense.bias), enc[f"hidden_{i}"]["bias"])
        put(get(blk.norm.weight), enc[f"LayerNorm_{i}"]["scale"])
        put(get(blk.norm.bias), enc[f"LayerNorm_{i}"]["bias"])
    Z = policy.latents
    w, b = get(policy.fc2.weight), get(policy.fc2.bias)
    put(w[:Z], np.asarray(enc["fc2_mean"]["kernel"]).T)
    put(w[Z:], np.asarray(enc["fc2_logvar"]["kernel"]).T)
    put(b[:Z], enc["fc2_mean"]["bias"])
    put(b[Z:], enc["fc2_logvar"]["bias"])


def policy_to_flax(policy: IntentionPolicy, get=_ident) -> dict:
    """`get(parameter) -> tensor of the same shape`: identity = the parameter values; the optimiser export passes the parameter's view
    of a moment buffer, so mu / nu come out as trees with the parameters' own names (optax ScaleByAdamState.mu / .nu)."""
    if hasattr(policy, "w_hh"):
        return lstm_policy_to_flax(policy, get)
    enc, dec = {}, {}
    for i, blk in enumerate(policy.encoder):
        enc[f"hidden_{i}"] = {"kernel": _np(get(blk.dense.weight).t()), "bias": _np(get(blk.dense.bias))}
        enc[f"LayerNorm_{i}"] = {"scale": _np(get(blk.norm.weight)), "bias": _np(get(blk.norm.bias))}
    Z = policy.latents
    w, b = get(policy.fc2.weight), get(policy.fc2.bias)            # the two heads are the halves of one GEMM here
    enc["fc2_mean"] = {"kernel": _np(w[:Z].t()), "bias": _np(b[:Z])}
    enc["fc2_logvar"] = {"kernel": _np(w[Z:].t()), "bias": _np(b[Z:])}
    for i, blk in enumerate(policy.decoder):
        dec[f"hidden_{i}"] = {"kernel": _np(get(blk.dense.weight).t()), "bias": _np(get(blk.dense.bias))}
        dec[f"LayerNorm_{i}"] = {"scale": _np(get(blk.norm.weight)), "bias": _np(get(blk.norm.bias))}
    dec[f"hidden_{len(policy.decoder)}"] = {"kernel": _np(get(policy.head.weight).t()), "bias": _np(get(policy.head.bias))}
    return {"params": {"encoder": enc, "decoder": dec}}


def value_to_flax(value: ValueNet, get=_ident) -> dict:
    dense = [m for m in value.net if isinstance(m, torch.nn.Linear)]
    return {"params": {f"hidden_{i}": {"kernel": _np(get(l.weight).t()), "bias": _np(get(l.bias))} for i, l in enumerate(dense)}}


def normalizer_to_flax(n: RunningStatistics) -> dict:
    """brax RunningStatisticsState fields (count, mean, summed_variance, std)."""
    return {"count": _np(n.count), "mean": _np(n.mean), "summed_variance": _np(n.summed_variance), "std": _np(n.std)}


@torch.no_grad()
def policy_from_flax(policy: IntentionPolicy, tree: dict, get=_ident) -> None:
    """In place.  `get(parameter)` = the destination tensor (identity: the parameter; the optimiser import passes moment-buffer views)."""
    if hasattr(policy, "w_hh"):
        return lstm_policy_from_flax(policy, tree, get)
    p = tree["params"]
    dev = policy.fc2.weight.device

    def put(dst: torch.Tensor, src) -> None:
        dst.copy_(torch.as_tensor(np.ascontiguousarray(src), dtype=dst.dtype, device=dev))

    for i, blk in enumerate(policy.encoder):
        put(get(blk.dense.weight), np.asarray(p["encoder"][f"hidden_{i}"]["kernel"]).T)
        put(get(blk.dense.bias), p["encoder"][f"hidden_{i}"]["bias"])
        put(get(blk.norm.weight), p["encoder"][f"LayerNorm_{i}"]["scale"])
        put(get(blk.norm.bias), p["encoder"][f"LayerNorm_{i}"]["bias"])
    Z = policy.latents
    w, b = get(policy.fc2.weight), get(policy.fc2.bias)
    put(w[:Z], np.asarray(p["encoder"]["fc2_mean"]["kernel"]).T)
    put(w[Z:], np.asarray(p["encoder"]["fc2_logvar"]["kernel"]).T)
    put(b[:Z], p["encoder"]["fc2_mean"]["bias"])
    put(b[Z:], p["encoder"]["fc2_logvar"]["bias"])
    decoder_from_flax(policy, p["decoder"], get, check=False)


def decoder_flax_params(policy: IntentionPolicy) -> dict:
    """{"hidden_i/kernel": parameter, ...}: the decoder's entries of the flax tree (params/decoder: every block's hidden_i and LayerNorm_i, the
    action head as the last hidden_L) -> the parameters of `policy` they live in.  Kernels are stored [in, out], the parameters [out, in]."""
    out = {}
    for i, blk in enumerate(policy.decoder):
        out[f"hidden_{i}/kernel"], out[f"hidden_{i}/bias"] = blk.dense.weight, blk.dense.bias
        out[f"LayerNorm_{i}/scale"], out[f"LayerNorm_{i}/bias"] = blk.norm.weight, blk.norm.bias
    L = len(policy.decoder)
    out[f"hidden_{L}/kernel"], out[f"hidden_{L}/bias"] = policy.head.weight, policy.head.bias
    return out


def check_decoder_tree(policy: IntentionPolicy, dec: dict) -> None:
    """ValueError unless the flax decoder tree `dec` (params/decoder of a checkpoint) has exactly the entries and shapes of `policy`'s decoder and
    head — they follow from decoder_layer_sizes, intention_size, the proprioceptive observation width and the action size."""
    want = decoder_flax_params(policy)
    have = flatten(dec)
    extra = sorted(set(have) - set(want))
    if extra:
        raise ValueError(f"checkpoint decoder has decoder/{extra[0]}, which this run's decoder ({len(policy.decoder)} blocks + head) does not")
    for name, prm in want.items():
        if name not in have:
            raise ValueError(f"checkpoint decoder has no decoder/{name} (this run's decoder has {len(policy.decoder)} blocks + head)")
        shape = tuple(prm.shape[::-1]) if name.endswith("/kernel") else tuple(prm.shape)
        if tuple(have[name].shape) != shape:
            raise ValueError(f"checkpoint decoder/{name} has shape {tuple(have[name].shape)}, this run's has {shape} "
                             "(decoder_layer_sizes, intention_size, the proprioceptive observation width and the action size must match)")


@torch.no_grad()
def decoder_from_flax(policy: IntentionPolicy, dec: dict, get=_ident, check: bool = True) -> None:
    """The decoder half of policy_from_flax: params/decoder (blocks and the action head hidden_L) into `policy`, in place.  `check`: the shapes
    are verified first (check_decoder_tree), so a mismatched checkpoint is refused before anything is written."""
    if check:
        check_decoder_tree(policy, dec)
    dev = policy.head.weight.device
    for name, prm in decoder_flax_params(policy).items():
        layer, leaf = name.split("/")
        src = np.asarray(dec[layer][leaf])
        get(prm).copy_(torch.as_tensor(np.ascontiguousarray(src.T if leaf == "kernel" else src), dtype=prm.dtype, device=dev))


@torch.no_grad()
def normalizer_from_flax(n: RunningStatistics, tree: dict) -> None:
    for k in ("count", "mean", "summed_variance", "std"):
        getattr(n, k).copy_(torch.as_tensor(np.asarray(tree[k]), dtype=torch.float32, device=n.mean.device).reshape(getattr(n, k).shape))


@torch.no_grad()
def value_from_flax(value: ValueNet, tree: dict, get=_ident) -> None:
    """brax value MLP {'params': {hidden_i: {kernel [in, out], bias}}} -> the Linear layers of ValueNet, in place (flat-buffer views
    and hipGraph pointers of a live learner stay valid)."""
    p = tree["params"]
    dense = [m for m in value.net if isinstance(m, torch.nn.Linear)]
    if len(dense) != len(p):
        raise ValueError(f"value tree has {len(p)} layers, the network {len(dense)}")
    for i, lin in enumerate(dense):
        get(lin.weight).copy_(torch.as_tensor(np.asarray(p[f"hidden_{i}"]["kernel"]).T.copy(), dtype=lin.weight.dtype, device=lin.weight.device))
        get(lin.bias).copy_(torch.as_tensor(np.asarray(p[f"hidden_{i}"]["bias"]), dtype=lin.bias.dtype, device=lin.bias.device))


def flatten(tree: dict, prefix: str = "") -> dict:
    out = {}
    for k, v in tree.items():
        key = f"{prefix}/{k}" if prefix else str(k)
        if isinstance(v, dict):
            out.update(flatten(v, key))
        else:
            out[key] = np.asarray(v)
    return out


def unflatten(flat: dict) -> dict:
    tree: dict = {}
    for key, v in flat.items():
        node = tree
        parts = key.split("/")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = np.asarray(v)
    return tree


def _moment_view(learner, buf: torch.Tensor):
    """parameter -> its (un-padded) view of a flat moment buffer: the export is independent of the flat layout's pad rule."""
    from .ppo import _flat_view
    segs = {id(p): seg for p, seg in zip(learner.grads.params, learner.grads.segs)}
    return lambda p: _flat_view(buf, segs[id(p)], p)


def rng_tree(learner) -> dict:
    """The noise-stream positions a resumed run continues from: the SGD step's device-side Philox draw counter (`_mb_state[0]`), the
    acting streams' counters (one per env group, in creation order) and the torch generators' states (shuffles, the non-default noise)."""
    out = {"sgd_draw_counter": _np(learner._mb_state[:1]), "rank": np.asarray(int(getattr(learner, "rank", 0)), dtype=np.int64),
           "torch_generators": {str(i): g.get_state().cpu().numpy().copy() for i, g in enumerate(learner.gens)}}
    by_gen = {id(g): i for i, g in enumerate(learner.gens)}
    out["act_counters"] = {str(by_gen[k]): _np(v[0]) for k, v in learner._act_rng.items() if k in by_gen}
    return out


@torch.no_grad()
def rng_from_tree(learner, tree: dict) -> None:
    learner._mb_state[:1].copy_(torch.as_tensor(np.asarray(tree["sgd_draw_counter"]), device=learner._mb_state.device))
    # the generator states are the SAVING rank's (rank 0 writes the checkpoint): that rank continues its streams exactly; every other rank
    # derives its own continuation from (saved state, rank) — restoring rank 0's states everywhere would make all ranks draw identical
    # shuffles / noise from here on (the learner seeds them seed * 1000 + 17 + rank).  The device-side Philox counters below are shared on
    # purpose: their KEYS are per rank
    saved_rank, rank = int(np.asarray(tree.get("rank", 0))), int(getattr(learner, "rank", 0))
    for i, st in tree.get("torch_generators", {}).items():
        if int(i) < len(learner.gens):
            st = np.asarray(st).astype(np.uint8)
            if rank == saved_rank:
                learner.gens[int(i)].set_state(torch.as_tensor(st, dtype=torch.uint8))
            else:
                import hashlib
                h = int.from_bytes(hashlib.blake2b(st.tobytes() + rank.to_bytes(4, "little") + int(i).to_bytes(4, "little"), digest_size=8).digest(), "little")
                learner.gens[int(i)].manual_seed(h & (2 ** 63 - 1))
    for i, v in tree.get("act_counters", {}).items():
        if int(i) < len(learner.gens):
            rs = learner._act_rng_state(learner.gens[int(i)])
            rs[0].copy_(torch.as_tensor(np.asarray(v).astype(np.int64), device=rs[0].device))


def learner_tree(learner) -> dict:
    """Everything a resumed run needs, in the reference's tree naming: (normalizer, policy, value) as the reference checkpoints them
    (checkpointing.py:280-299: `policy` = (normalizer_params, policy_params), `train_state` also holds the value params and the
    optimizer state) plus the Adam state as optax's ScaleByAdamState (count, mu, nu; mu / nu are trees named like the parameters,
    un-padded) and the noise-stream positions."""
    opt = learner.opt
    mu, nu = _moment_view(learner, opt.exp_avg), _moment_view(learner, opt.exp_avg_sq)
    return {"normalizer": normalizer_to_flax(learner.normalizer), "policy": policy_to_flax(learner.policy), "value": value_to_flax(learner.value),
            "optimizer": {"count": np.asarray(opt.t, dtype=np.int64),
                          "mu": {"policy": policy_to_flax(learner.policy, mu), "value": value_to_flax(learner.value, mu)},
                          "nu": {"policy": policy_to_flax(learner.policy, nu), "value": value_to_flax(learner.value, nu)}},
            "rng": rng_tree(learner), **carry_tree(learner)}


def carry_tree(learner) -> dict:
    """The recurrent learner's roll-out carry (TrainingState.hidden_state of lstm_ppo/ppo.py), resets applied: {"hidden_state": {h, c}} [n, L, H]."""
    if not hasattr(learner, "settle_carry"):
        return {}
    learner.settle_carry()
    return {"hidden_state": {"h": _np(learner.h_carry), "c": _np(learner.c_carry)}}


@torch.no_grad()
def carry_from_tree(learner, tree: dict) -> None:
    if not hasattr(learner, "settle_carry") or "hidden_state" not in tree:
        return
    hs = tree["hidden_state"]
    for dst, k in ((learner.h_carry, "h"), (learner.c_carry, "c")):
        src = np.asarray(hs[k])
        if src.shape != tuple(dst.shape):
            raise ValueError(f"checkpoint carry {k} has shape {src.shape}, the learner {tuple(dst.shape)}")
        dst.copy_(torch.as_tensor(src, dtype=dst.dtype, device=dst.device))
    learner._pending_reset.zero_()


def _atomic_savez(path, flat: dict, overwrite: bool) -> None:
    """np.savez to a temporary file in the same directory, then os.replace: a crash mid-write never leaves a truncated checkpoint under
    the final name.  An existing file is refused unless `overwrite` (orbax refuses to save an existing step)."""
    import os
    import tempfile
    path = str(path)
    if os.path.exists(path) and not overwrite:
        raise FileExistsError(f"{path} exists: a checkpoint is never overwritten (resume into a new directory, or pass overwrite=True)")
    fd, tmp = tempfile.mkstemp(prefix=".tmp-", suffix=".npz", dir=os.path.dirname(path) or ".")
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez(f, **flat)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def save_npz(path, learner, config: dict | None = None, step: int | None = None, iteration: int | None = None, overwrite: bool = False) -> None:
    """One flat .npz: learner_tree() + optionally the run's config as JSON (the reference embeds it: checkpointing.py:292-296), the
    env-step counter (TrainingState.env_steps) and the eval iteration (the reference's checkpoint step, ppo.py:787-795)."""
    import json
    flat = flatten(learner_tree(learner))
    if config is not None:
        flat["config_json"] = np.frombuffer(json.dumps(config, default=str).encode(), dtype=np.uint8)
    if step is not None:
        flat["env_steps"] = np.asarray(step, dtype=np.int64)
    if iteration is not None:
        flat["iteration"] = np.asarray(iteration, dtype=np.int64)
    _atomic_savez(path, flat, overwrite)


def load_npz(path, learner, load_optimizer: bool = True) -> dict:
    """Restore normaliser, policy, value and (if present) the optimiser moments and noise-stream positions of a learner IN PLACE;
    returns {config, env_steps, iteration}."""
    import json
    with np.load(path) as z:
        flat = {k: z[k] for k in z.files}
    extra = {"config": json.loads(bytes(flat.pop("config_json")).decode()) if "config_json" in flat else None,
             "env_steps": int(flat.pop("env_steps")) if "env_steps" in flat else None,
             "iteration": int(flat.pop("iteration")) if "iteration" in flat else None}
    tree = unflatten(flat)
    normalizer_from_flax(learner.normalizer, tree["normalizer"])
    policy_from_flax(learner.policy, tree["policy"])
    if "value" in tree:
        value_from_flax(learner.value, tree["value"])
    if load_optimizer and "optimizer" in tree:
        o = tree["optimizer"]
        with torch.no_grad():
            for name, buf in (("mu", learner.opt.exp_avg), ("nu", learner.opt.exp_avg_sq)):
                buf.zero_()                                   # (pad columns stay exactly zero)
                view = _moment_view(learner, buf)
                policy_from_flax(learner.policy, o[name]["policy"], view)
                value_from_flax(learner.value, o[name]["value"], view)
        learner.opt.t = int(o["count"])
    if load_optimizer and "rng" in tree:
        rng_from_tree(learner, tree["rng"])
    if load_optimizer:
        carry_from_tree(learner, tree)
    if hasattr(learner, "_refresh_padded_weights"):
        learner._refresh_padded_weights()
    return extra


# ---- the reference's checkpoint DIRECTORY layout (checkpointing.py:280-306: ocp.args.Composite(policy=StandardSave, train_state=StandardSave,
# config=JsonSave) under <directory>/<step>/) ------------------------------------------------------------------------------------------
def save_step_dir(directory, step: int, learner, config: dict | None = None, env_steps: int | None = None) -> str:
    """<directory>/<step>/{policy.npz, train_state.npz, config/metadata}: the three items of the reference's Composite save under the
    reference's names, `step` = the eval iteration (ppo.py:700-711 saves step 0, :787-795 step `it`).

    * `config/metadata` is the JSON file orbax's JsonCheckpointHandler writes for `JsonSave(config)`;
    * `policy` = the pair (normalizer_params, policy_params) the reference hands to StandardSave — here `policy.npz` with keys
      `0/{count,mean,summed_variance,std}` and `1/params/{encoder,decoder}/...` (a tuple's items are numbered by orbax);
    * `train_state` = brax-style TrainingState(optimizer_state, params{policy, value}, normalizer_params, env_steps) — `train_state.npz`.

    The two pytree items are NOT orbax containers: StandardSave writes a tensorstore OCDBT / zarr store whose byte format is defined by
    tensorstore (not in this image, not stated anywhere in the reference), so it cannot be restated or pinned here; INTEGRATION.md holds
    the five-line reference-side conversion (np.load -> unflatten -> ckpt_mgr.save).  The directory is built under a temporary name and
    renamed into place; an existing step is refused (as orbax does)."""
    import json
    import os
    import tempfile
    directory = str(directory)
    final = os.path.join(directory, str(int(step)))
    if os.path.exists(final):
        raise FileExistsError(f"checkpoint step {step} already exists in {directory}")
    os.makedirs(directory, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix=f".{int(step)}.tmp-", dir=directory)
    try:
        tree = learner_tree(learner)
        _atomic_savez(os.path.join(tmp, "policy.npz"), flatten({"0": tree["normalizer"], "1": tree["policy"]}), True)
        ts = {"optimizer_state": tree["optimizer"], "params": {"policy": tree["policy"], "value": tree["value"]},
              "normalizer_params": tree["normalizer"], "env_steps": np.asarray(0 if env_steps is None else env_steps, dtype=np.int64),
              "rng": tree["rng"], "iteration": np.asarray(int(step), dtype=np.int64)}
        if "hidden_state" in tree:
            ts["hidden_state"] = tree["hidden_state"]
        _atomic_savez(os.path.join(tmp, "train_state.npz"), flatten(ts), True)
        os.makedirs(os.path.join(tmp, "config"))
        with open(os.path.join(tmp, "config", "metadata"), "w") as f:
            json.dump(config if config is not None else {}, f, default=str)
        os.rename(tmp, final)
    except BaseException:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
        raise
    return final


def latest_step(directory) -> int | None:
    """orbax CheckpointManager.latest_step(): the largest all-digit sub-directory name."""
    import os
    try:
        steps = [int(d) for d in os.listdir(str(directory)) if d.isdigit() and os.path.isdir(os.path.join(str(directory), d))]
    except FileNotFoundError:
        return None
    return max(steps) if steps else None


def load_step_dir(path, learner, load_optimizer: bool = True) -> dict:
    """Restore from <directory>/<step>/ (or from <directory>: its latest step) written by save_step_dir; returns {config, env_steps, iteration}
    (checkpointing.load_training_state restores the whole TrainingState incl. env_steps: ppo.py:561-567)."""
    import json
    import os
    path = str(path)
    if not os.path.exists(os.path.join(path, "train_state.npz")):
        st = latest_step(path)
        if st is None:
            raise FileNotFoundError(f"no checkpoint step under {path}")
        path = os.path.join(path, str(st))
    with np.load(os.path.join(path, "train_state.npz")) as z:
        ts = unflatten({k: z[k] for k in z.files})
    normalizer_from_flax(learner.normalizer, ts["normalizer_params"])
    policy_from_flax(learner.policy, ts["params"]["policy"])
    value_from_flax(learner.value, ts["params"]["value"])
    if load_optimizer:
        o = ts["optimizer_state"]
        with torch.no_grad():
            for name, buf in (("mu", learner.opt.exp_avg), ("nu", learner.opt.exp_avg_sq)):
                buf.zero_()
                view = _moment_view(learner, buf)
                policy_from_flax(learner.policy, o[name]["policy"], view)
                value_from_flax(learner.value, o[name]["value"], view)
        learner.opt.t = int(o["count"])
        if "rng" in ts:
            rng_from_tree(learner, ts["rng"])
        carry_from_tree(learner, ts)
    if hasattr(learner, "_refresh_padded_weights"):
        learner._refresh_padded_weights()
    cfg = None
    if os.path.exists(os.path.join(path, "config", "metadata")):
        with open(os.path.join(path, "config", "metadata")) as f:
            cfg = json.load(f)
    return {"config": cfg, "env_steps": int(ts["env_steps"]), "iteration": int(ts["iteration"])}


def restore(path, learner, load_optimizer: bool = True) -> dict:
    """A .npz file, a step directory, or a checkpoint directory (latest step)."""
    import os
    return load_step_dir(path, learner, load_optimizer) if os.path.isdir(str(path)) else load_npz(path, learner, load_optimizer)


# ---- the analysis side (checkpointing.py:110-218 of the reference: load_config_from_checkpoint, load_policy, load_inference_fn): a trained policy
# for roll-outs, without a training env or a learner ---------------------------------------------------------------------------------------------
def resolve_step_dir(path, step: int | None = None) -> str:
    """<run dir>/<step>/ (the latest step when `step` is None) or a step directory itself."""
    import os
    path = str(path)
    if step is None and os.path.exists(os.path.join(path, "policy.npz")):
        return path
    st = latest_step(path) if step is None else int(step)
    if st is None or not os.path.exists(os.path.join(path, str(st), "policy.npz")):
        raise FileNotFoundError(f"no checkpoint step {'' if step is None else step} with a policy.npz under {path}")
    return os.path.join(path, str(st))


def load_config_from_checkpoint(path, step: int | None = None) -> dict:
    """The run's config saved with the checkpoint (config/metadata of the step directory)."""
    import json
    import os
    d = resolve_step_dir(path, step)
    meta = os.path.join(d, "config", "metadata")
    if not os.path.exists(meta):
        raise FileNotFoundError(f"{d} has no config/metadata")
    with open(meta) as f:
        return json.load(f)


def load_policy(path, cfg: dict | None = None, step: int | None = None) -> tuple:
    """(normalizer_params, policy_params) of a step's policy.npz: the normaliser tree {count, mean, summed_variance, std} and the flax policy tree."""
    import os
    d = resolve_step_dir(path, step)
    with np.load(os.path.join(d, "policy.npz")) as z:
        tree = unflatten({k: z[k] for k in z.files})
    return tree["0"], tree["1"]


def load_freeze_source(path) -> tuple:
    """(normalizer_params, policy_params, step) that a freeze_decoder run takes its decoder and pinned normaliser columns from
    (checkpointing.load_policy at ppo.py:569-572 of the reference): the latest step of a checkpoint directory, a step directory, or a .npz
    of save_npz (step: its iteration, None if it has none)."""
    import os
    if os.path.isdir(str(path)):
        d = resolve_step_dir(path)
        norm, pol = load_policy(d)
        return norm, pol, int(os.path.basename(os.path.normpath(d)))
    with np.load(str(path)) as z:
        flat = {k: z[k] for k in z.files if k not in ("config_json",)}
    step = int(flat.pop("iteration")) if "iteration" in flat else None
    flat.pop("env_steps", None)
    tree = unflatten(flat)
    return tree["normalizer"], tree["policy"], step


def load_inference_fn(cfg: dict, policy: tuple, deterministic: bool = True, get_activation: bool = True, device="cuda"):
    """The deterministic inference function of (normalizer_params, policy_params) (make_inference_fn(...)(params, deterministic=True,
    get_activation=...)): an analysis.rollout.RolloutPolicy holding the policy module with fp32 weights on `device`.  Layer sizes come from the
    parameter tree; train_config.use_lstm picks the LSTM-decoder policy.  A bf16-trained (mlp_gemm_inputs=bf16) policy runs in fp32."""
    from ..analysis.rollout import RolloutPolicy
    if not deterministic:
        raise NotImplementedError("load_inference_fn: only the deterministic policy (the roll-out's) is built")
    norm, ptree = policy
    p = ptree["params"]
    enc = p["encoder"]
    n_enc = len([k for k in enc if k.startswith("hidden_")])
    enc_sizes = [int(np.asarray(enc[f"hidden_{i}"]["kernel"]).shape[1]) for i in range(n_enc)]
    ref = int(np.asarray(enc["hidden_0"]["kernel"]).shape[0])
    Z = int(np.asarray(enc["fc2_mean"]["kernel"]).shape[1])
    W = int(np.asarray(norm["mean"]).shape[-1])
    dev = torch.device(device)
    use_lstm = "lstm_decoder" in p
    if use_lstm != bool(cfg.get("train_setup", {}).get("train_config", {}).get("use_lstm", use_lstm)):
        raise ValueError("load_inference_fn: train_config.use_lstm does not match the checkpoint's policy tree")
    if use_lstm:
        from .lstm import LSTMIntentionPolicy
        dec = p["lstm_decoder"]
        L = len([k for k in dec if k.startswith("lstm_") and k != "lstm_projection"])
        H = int(np.asarray(dec["lstm_0"]["hi"]["kernel"]).shape[0])
        A2 = int(np.asarray(dec["lstm_projection"]["kernel"]).shape[1])
        module = LSTMIntentionPolicy(W, ref, A2 // 2, Z, enc_sizes, hidden_state_size=H, hidden_layer_num=L)
    else:
        dec = p["decoder"]
        n_dec = len([k for k in dec if k.startswith("hidden_")]) - 1
        dec_sizes = [int(np.asarray(dec[f"hidden_{i}"]["kernel"]).shape[1]) for i in range(n_dec)]
        A2 = int(np.asarray(dec[f"hidden_{n_dec}"]["kernel"]).shape[1])
        module = IntentionPolicy(W, ref, A2 // 2, Z, enc_sizes, dec_sizes)
    module = module.to(dev).float().eval()
    for q in module.parameters():
        q.requires_grad_(False)
    policy_from_flax(module, ptree)
    mean = std = None
    if bool(cfg.get("train_setup", {}).get("train_config", {}).get("normalize_observations", True)):
        mean = torch.as_tensor(np.asarray(norm["mean"], dtype=np.float32), device=dev).reshape(-1).contiguous()
        std = torch.as_tensor(np.asarray(norm["std"], dtype=np.float32), device=dev).reshape(-1).contiguous()
    gi = "bf16" if str(cfg.get("mlp_gemm_inputs", "f32")).lower() in ("bf16", "bfloat16") else "f32"
    return RolloutPolicy(module, mean, std, "lstm" if use_lstm else "mlp", get_activation=get_activation, trained_gemm_inputs=gi)


# ---- the decoder-only policy (ppo_networks.py:193-238 make_decoder_policy_fn, intention_network.py:194-222 make_decoder_policy): the pretrained
# motor module on its own, driven with latents — what environment.wrappers.HighLevelWrapper puts inside an env ---------------------------------------
class DecoderPolicy:
    """policy(x) with x [n, Z + prop] = [latents | RAW proprioceptive observation] -> (action [n, A] = tanh(loc), extras): only the trailing
    `prop` columns are normalised (intention_network.py:206-214), with the normaliser's columns [reference_obs_size:] — the only ones kept
    (ppo_networks.py:225-234).  Plain torch on a CPU tensor; on the GPU the blocks' modules run their HIP kernels, and HighLevelWrapper runs the
    whole policy as a launch list on the env's buffers.  A bf16-trained policy runs in fp32."""

    def __init__(self, net: DecoderNet, mean: torch.Tensor | None, std: torch.Tensor | None, latent_size: int, reference_obs_size: int,
                 trained_gemm_inputs: str = "f32"):
        if (mean is None) != (std is None):
            raise ValueError("DecoderPolicy: mean and std together")
        self.net, self.mean, self.std = net, mean, std
        self.latent_size, self.reference_obs_size, self.action_size = int(latent_size), int(reference_obs_size), int(net.action_size)
        first = net.decoder[0].dense if len(net.decoder) else net.head
        self.proprioceptive_obs_size = int(first.in_features) - self.latent_size
        self.decoder_layer_sizes = tuple(int(b.dense.out_features) for b in net.decoder)
        self.device = net.head.weight.device
        self.trained_gemm_inputs = trained_gemm_inputs
        if mean is not None and (mean.shape != (self.proprioceptive_obs_size,) or std.shape != mean.shape):
            raise ValueError(f"DecoderPolicy: mean / std must hold the {self.proprioceptive_obs_size} proprioceptive columns")

    @torch.no_grad()
    def logits(self, x: torch.Tensor) -> torch.Tensor:
        Z, P = self.latent_size, self.proprioceptive_obs_size
        if x.shape[-1] != Z + P:
            raise ValueError(f"DecoderPolicy: the input has {x.shape[-1]} columns, not latents + proprioception = {Z} + {P}")
        x = x.to(device=self.device, dtype=torch.float32)
        prop = x[..., Z:]
        if self.mean is not None:
            prop = (prop - self.mean) / self.std
        return self.net(torch.cat([x[..., :Z], prop], dim=-1))

    def __call__(self, x: torch.Tensor, key=None):
        return torch.tanh(self.logits(x)[..., :self.action_size]), {}


def decoder_policy_from_trees(norm: dict | None, ptree: dict, normalize_observations: bool = True, device="cuda",
                              trained_gemm_inputs: str = "f32") -> DecoderPolicy:
    """DecoderPolicy of (normalizer_params, policy_params): sizes from the parameter tree (Z = fc2_mean's width, proprioceptive width = the first
    decoder layer's input - Z, reference_obs_size = the normaliser's width - that), params/decoder only, mean / std columns [reference_obs_size:] only."""
    p = ptree.get("params", {})
    if "lstm_decoder" in p:
        raise NotImplementedError("make_decoder_policy_fn: the checkpoint holds an LSTM decoder (params/lstm_decoder); the decoder-only policy is built "
                                  "for the MLP decoder only")
    if "decoder" not in p:
        raise ValueError("make_decoder_policy_fn: the checkpoint's policy tree has no params/decoder")
    dec = p["decoder"]
    n_dec = len([k for k in dec if k.startswith("hidden_")]) - 1
    if n_dec < 0:
        raise ValueError("make_decoder_policy_fn: params/decoder has no hidden_<i> layer")
    if "encoder" not in p or "fc2_mean" not in p["encoder"]:
        raise ValueError("make_decoder_policy_fn: the intention size is read from params/encoder/fc2_mean, which the checkpoint does not have")
    sizes = [int(np.asarray(dec[f"hidden_{i}"]["kernel"]).shape[1]) for i in range(n_dec)]
    A2 = int(np.asarray(dec[f"hidden_{n_dec}"]["kernel"]).shape[1])
    in0 = int(np.asarray(dec["hidden_0"]["kernel"]).shape[0])
    dev = torch.device(device)
    Z, ref, mean, std = _decoder_sizes_and_norm("make_decoder_policy_fn", p, norm, in0, A2, normalize_observations, dev)
    net = DecoderNet(in0, A2 // 2, sizes).to(dev).float().eval()
    for q in net.parameters():
        q.requires_grad_(False)
    decoder_from_flax(net, dec)
    return DecoderPolicy(net, mean, std, Z, ref, trained_gemm_inputs)


def _decoder_sizes_and_norm(who: str, p: dict, norm: dict | None, in0: int, A2: int, normalize_observations: bool, dev) -> tuple:
    """(Z, reference_obs_size, mean, std) of a decoder-only policy whose first layer takes `in0` columns and whose head has `A2`: Z = fc2_mean's
    width, proprioceptive width = in0 - Z, reference_obs_size = the normaliser's width - that; mean / std: the normaliser's columns
    [reference_obs_size:] on `dev`, or None without normalize_observations."""
    Z = int(np.asarray(p["encoder"]["fc2_mean"]["kernel"]).shape[1])
    prop = in0 - Z
    if prop < 0 or A2 % 2:
        raise ValueError(f"{who}: decoder input width {in0} < intention size {Z}, or an odd head width {A2}")
    if norm is None or "mean" not in norm:
        raise ValueError(f"{who}: the checkpoint has no normaliser (its width gives reference_obs_size)")
    W = int(np.asarray(norm["mean"]).shape[-1])
    ref = W - prop
    if ref < 0:
        raise ValueError(f"{who}: the normaliser has {W} columns, fewer than the decoder's {prop} proprioceptive inputs")
    mean = std = None
    if normalize_observations:
        mean, std = (torch.as_tensor(np.asarray(norm[k], dtype=np.float32).reshape(-1)[ref:].copy(), device=dev).contiguous() for k in ("mean", "std"))
    return Z, ref, mean, std


def make_decoder_policy_fn(ckpt_path, step: int | None = None, device="cuda") -> DecoderPolicy:
    """The decoder-only inference function of a checkpoint (ppo_networks.py:193-238): a run directory (latest step, or `step`), a step directory, or
    a .npz of save_npz.  normalize_observations=false in the saved config means no normaliser."""
    norm, ptree, cfg = _policy_trees_and_config(ckpt_path, step, "make_decoder_policy_fn")
    tc = (cfg.get("train_setup") or {}).get("train_config") or {}
    gi = "bf16" if str(cfg.get("mlp_gemm_inputs", "f32")).lower() in ("bf16", "bfloat16") else "f32"
    return decoder_policy_from_trees(norm, ptree, bool(tc.get("normalize_observations", True)), device, gi)


# ---- the decoder-only policy of an LSTM checkpoint (the lstm_ppo counterpart of the above: params/lstm_decoder driven with latents and a carried
# (h, c); the reference's lstm_ppo/ppo_networks.py:240 names such a function but its module defines no make_decoder_policy and has no place for the
# carry — this follows the LSTM roll-out step, agent/lstm.py LSTMIntentionPolicy.step, without its encoder) ------------------------------------------
class LSTMDecoderPolicy:
    """policy(x, hidden_state=None, reset=None) with x [n, Z + prop] = [latents | RAW proprioceptive observation] -> (action [n, A] = tanh(loc),
    extras, (h, c) [n, L, H]): only the trailing `prop` columns are normalised, with the normaliser's columns [reference_obs_size:].
    hidden_state None = a zero carry; reset [n]: non-zero rows start from a zero carry.  The carry passed in is not modified.  Plain torch (CPU
    tensors: agent.lstm._torch_lstm_layer); on the GPU, HighLevelWrapper runs the policy as a launch list on the env's buffers.  Weights of layer k:
    w_ih[k] [4H, in_k], w_hh[k] [4H, H], b_hh[k] [4H] (gate rows i | f | g | o), projection w_p [2A, H], b_p [2A]."""

    def __init__(self, w_ih, w_hh, b_hh, w_p: torch.Tensor, b_p: torch.Tensor, mean: torch.Tensor | None, std: torch.Tensor | None, latent_size: int,
                 reference_obs_size: int, trained_gemm_inputs: str = "f32"):
        if (mean is None) != (std is None):
            raise ValueError("LSTMDecoderPolicy: mean and std together")
        if not (len(w_ih) == len(w_hh) == len(b_hh) >= 1):
            raise ValueError("LSTMDecoderPolicy: one (w_ih, w_hh, b_hh) per layer, at least one layer")
        self.w_ih, self.w_hh, self.b_hh, self.w_p, self.b_p = list(w_ih), list(w_hh), list(b_hh), w_p, b_p
        self.mean, self.std = mean, std
        self.hidden_layer_num, self.hidden_state_size = len(self.w_ih), int(self.w_hh[0].shape[1])
        self.latent_size, self.reference_obs_size, self.action_size = int(latent_size), int(reference_obs_size), int(w_p.shape[0]) // 2
        self.proprioceptive_obs_size = int(self.w_ih[0].shape[1]) - self.latent_size
        self.device = w_p.device
        self.trained_gemm_inputs = trained_gemm_inputs
        if mean is not None and (mean.shape != (self.proprioceptive_obs_size,) or std.shape != mean.shape):
            raise ValueError(f"LSTMDecoderPolicy: mean / std must hold the {self.proprioceptive_obs_size} proprioceptive columns")

    def zero_carry(self, n: int, device=None, dtype=torch.float32) -> tuple:
        shape = (int(n), self.hidden_layer_num, self.hidden_state_size)
        dev = self.device if device is None else device
        return torch.zeros(shape, dtype=dtype, device=dev), torch.zeros(shape, dtype=dtype, device=dev)

    @torch.no_grad()
    def logits(self, x: torch.Tensor, hidden_state=None, reset=None, dtype=torch.float32):
        """(logits [n, 2A], (h, c)) of one step; `dtype`: the precision it is evaluated in (float64: the restatement the kernels are held to)."""
        from .lstm import _torch_lstm_layer
        Z, P = self.latent_size, self.proprioceptive_obs_size
        if x.dim() != 2 or x.shape[-1] != Z + P:
            raise ValueError(f"LSTMDecoderPolicy: the input is {tuple(x.shape)}, not [n, latents + proprioception = {Z} + {P}]")
        cv = lambda t: t.detach().to(device="cpu", dtype=dtype)      # noqa: E731
        x = cv(x)
        prop = x[:, Z:]
        if self.mean is not None:
            prop = (prop - cv(self.mean)) / cv(self.std)
        a = torch.cat([x[:, :Z], prop], dim=-1)
        n = x.shape[0]
        if hidden_state is None:
            h, c = self.zero_carry(n, "cpu", dtype)
        else:
            h, c = cv(hidden_state[0]).clone(), cv(hidden_state[1]).clone()
            if h.shape != (n, self.hidden_layer_num, self.hidden_state_size) or c.shape != h.shape:
                raise ValueError(f"LSTMDecoderPolicy: hidden_state must be (h, c) of shape [{n}, {self.hidden_layer_num}, {self.hidden_state_size}]")
        rs = None if reset is None else cv(reset).reshape(1, n)
        for k in range(self.hidden_layer_num):
            hn, cn = _torch_lstm_layer((a @ cv(self.w_ih[k]).t()).unsqueeze(0), cv(self.w_hh[k]), cv(self.b_hh[k]), h[:, k], c[:, k], rs)
            h[:, k], c[:, k] = hn[0], cn[0]
            a = hn[0]
        return torch.nn.functional.linear(a, cv(self.w_p), cv(self.b_p)), (h, c)      # (nn.Linear's expression: LSTMIntentionPolicy.projection)

    def __call__(self, x: torch.Tensor, hidden_state=None, reset=None, key=None):
        lg, (h, c) = self.logits(x, hidden_state, reset)
        dev = x.device
        return torch.tanh(lg[:, :self.action_size]).to(dev), {}, (h.to(dev), c.to(dev))


def lstm_decoder_policy_from_trees(norm: dict | None, ptree: dict, normalize_observations: bool = True, device="cuda",
                                   trained_gemm_inputs: str = "f32") -> LSTMDecoderPolicy:
    """LSTMDecoderPolicy of (normalizer_params, policy_params): Z = fc2_mean's width, H and L from params/lstm_decoder/lstm_<k>, A from lstm_projection,
    proprioceptive width = lstm_0's input - Z, reference_obs_size = the normaliser's width - that; weights converted as lstm_policy_from_flax does."""
    who = "make_lstm_decoder_policy_fn"
    p = ptree.get("params", {})
    if "lstm_decoder" not in p:
        if "decoder" in p:
            raise ValueError(f"{who}: the checkpoint holds an MLP decoder (params/decoder): use make_decoder_policy_fn")
        raise ValueError(f"{who}: the checkpoint's policy tree has no params/lstm_decoder")
    dec = p["lstm_decoder"]
    L = len([k for k in dec if k.startswith("lstm_") and k != "lstm_projection"])
    if L < 1 or any(f"lstm_{k}" not in dec for k in range(L)):
        raise ValueError(f"{who}: params/lstm_decoder has no lstm_<k> layers 0 .. L-1")
    if "lstm_projection" not in dec:
        raise ValueError(f"{who}: params/lstm_decoder has no lstm_projection")
    if "encoder" not in p or "fc2_mean" not in p["encoder"]:
        raise ValueError(f"{who}: the intention size is read from params/encoder/fc2_mean, which the checkpoint does not have")
    H = int(np.asarray(dec["lstm_0"]["hi"]["kernel"]).shape[0])
    in0 = int(np.asarray(dec["lstm_0"]["ii"]["kernel"]).shape[0])
    A2 = int(np.asarray(dec["lstm_projection"]["kernel"]).shape[1])
    dev = torch.device(device)
    Z, ref, mean, std = _decoder_sizes_and_norm(who, p, norm, in0, A2, normalize_observations, dev)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=dev).contiguous()      # noqa: E731
    w_ih, w_hh, b_hh = [], [], []
    for k in range(L):
        cell = dec[f"lstm_{k}"]
        w_ih.append(t(np.concatenate([np.asarray(cell["i" + g]["kernel"]).T for g in LSTM_GATES], 0)))
        w_hh.append(t(np.concatenate([np.asarray(cell["h" + g]["kernel"]).T for g in LSTM_GATES], 0)))
        b_hh.append(t(np.concatenate([np.asarray(cell["h" + g]["bias"]).reshape(-1) for g in LSTM_GATES], 0)))
        want = in0 if k == 0 else H
        if w_ih[k].shape != (4 * H, want) or w_hh[k].shape != (4 * H, H) or b_hh[k].shape != (4 * H,):
            raise ValueError(f"{who}: lstm_{k} is not an LSTM cell of {want} inputs and {H} hidden units")
    proj = dec["lstm_projection"]
    w_p, b_p = t(np.asarray(proj["kernel"]).T), t(np.asarray(proj["bias"]).reshape(-1))
    if w_p.shape != (A2, H):
        raise ValueError(f"{who}: lstm_projection takes {w_p.shape[1]} inputs, the cells have {H} hidden units")
    return LSTMDecoderPolicy(w_ih, w_hh, b_hh, w_p, b_p, mean, std, Z, ref, trained_gemm_inputs)


def _policy_trees_and_config(ckpt_path, step, who: str) -> tuple:
    import json
    import os
    path = str(ckpt_path)
    if os.path.isdir(path):
        d = resolve_step_dir(path, step)
        norm, ptree = load_policy(d)
        meta = os.path.join(d, "config", "metadata")
        cfg = {}
        if os.path.exists(meta):
            with open(meta) as f:
                cfg = json.load(f) or {}
    else:
        if step is not None:
            raise ValueError(f"{who}: `step` selects a step of a checkpoint directory; a .npz file holds one policy")
        norm, ptree, _ = load_freeze_source(path)
        with np.load(path) as z:
            cfg = json.loads(bytes(z["config_json"]).decode()) if "config_json" in z.files else {}
    return norm, ptree, cfg


def make_lstm_decoder_policy_fn(ckpt_path, step: int | None = None, device="cuda") -> LSTMDecoderPolicy:
    """The decoder-only inference function of a use_lstm checkpoint: a run directory (latest step, or `step`), a step directory, or a .npz of
    save_npz.  normalize_observations=false in the saved config means no normaliser."""
    norm, ptree, cfg = _policy_trees_and_config(ckpt_path, step, "make_lstm_decoder_policy_fn")
    tc = (cfg.get("train_setup") or {}).get("train_config") or {}
    gi = "bf16" if str(cfg.get("mlp_gemm_inputs", "f32")).lower() in ("bf16", "bfloat16") else "f32"
    return lstm_decoder_policy_from_trees(norm, ptree, bool(tc.get("normalize_observations", True)), device, gi)
