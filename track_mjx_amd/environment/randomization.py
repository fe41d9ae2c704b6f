"""Per-env domain randomisation: three scalars per env (friction, actuator strength, joint damping) and the env's gravity vector.

The reference hands `wrap(..., randomization_fn=fn)` to brax's DomainRandomizationVmapWrapper (track_mjx/environment/wrappers.py:44-47), which
steps every env with its own copy of the mjx.Model.  The physics kernel here reads ONE model from constant memory and runs one wavefront per
env, so a per-env *scalar* is wave-uniform and costs one scalar load per launch (csrc/tmjx_wave_rand.hip); `randomization_fn` therefore returns a
`DomainRandomization` — per-env scales of the model's sliding friction, actuator force and dof damping — instead of a batched model.  Per-env
models, masses and per-geom / per-dof / per-actuator vectors are not supported.  Gravity is three more wave-uniform floats per env
(include/tmjx.h: tmjx_set_env_gravity): a shorter vector is body-weight support, a tilted one — in this model's flat world — an inclined floor.

`uniform_scales` draws the scales from a jax PRNG key (threefry, jax_random.py): the same key gives the same scales on every rank and on
resume, as the reference gives all devices the same randomisation rng (agent/mlp_ppo/ppo.py:458-460); a rank takes its shard of the one draw.
"""
from __future__ import annotations

from collections.abc import Mapping
from types import MappingProxyType

import numpy as np

SCALE_NAMES = ("friction", "actuator", "damping")      # row order of the [3][n_env] device array (include/tmjx.h: tmjx_set_env_scales)


class DomainRandomization:
    """Per-env scales of the model constants: `friction` multiplies every contact's sliding friction, `actuator` the actuators' gain and
    affine bias (ctrlrange and the activation dynamics are not scaled), `damping` the dofs' damping.  Each is None (ones) or a length-num_envs
    array-like of finite values > 0; the length is fixed by the first array given (all must agree), or by `num_envs` when all are None.
    `gravity` is None (the model's gravity) or [num_envs, 3]: each env's gravity vector in the world frame, m/s^2, finite, stored as float32."""

    def __init__(self, friction=None, actuator=None, damping=None, num_envs: int | None = None, gravity=None):
        vals, n = {}, None if num_envs is None else int(num_envs)
        if gravity is not None:
            if hasattr(gravity, "detach"):
                gravity = gravity.detach().cpu().numpy()
            g = np.asarray(gravity, dtype=np.float64)
            if g.ndim != 2 or g.shape[1] != 3 or g.shape[0] < 1:
                raise ValueError(f"DomainRandomization: gravity must be [num_envs, 3] (one world-frame vector per env), got shape {g.shape}")
            if n is not None and g.shape[0] != n:
                raise ValueError(f"DomainRandomization: gravity has {g.shape[0]} vectors, expected {n} (one per env)")
            n = g.shape[0]
            with np.errstate(over="ignore"):
                g32 = g.astype(np.float32)
            if not (np.isfinite(g).all() and np.isfinite(g32).all()):
                raise ValueError("DomainRandomization: gravity has non-finite components")
            gravity = np.ascontiguousarray(g32)
            gravity.setflags(write=False)
        self.gravity = gravity
        for name, v in zip(SCALE_NAMES, (friction, actuator, damping)):
            if v is None:
                vals[name] = None
                continue
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            a = np.asarray(v, dtype=np.float64)
            if a.ndim != 1 or a.size < 1:
                raise ValueError(f"DomainRandomization: {name} must be a 1-d array with one scale per env, got shape {a.shape}")
            if n is not None and a.size != n:
                raise ValueError(f"DomainRandomization: {name} has {a.size} scales, expected {n} (one per env)")
            n = a.size
            if not np.isfinite(a).all():
                raise ValueError(f"DomainRandomization: {name} has non-finite scales")
            if not (a > 0).all():
                raise ValueError(f"DomainRandomization: {name} scales must be > 0 (min {a.min()})")
            a32 = a.astype(np.float32)
            if not (np.isfinite(a32).all() and (a32 > 0).all()):
                raise ValueError(f"DomainRandomization: {name} scales leave the float32 range")
            vals[name] = a32
        if n is None:
            raise ValueError("DomainRandomization: give at least one scale array, or num_envs")
        if n < 1:
            raise ValueError("DomainRandomization: num_envs must be >= 1")
        self.num_envs = n
        self.has_scales = any(v is not None for v in vals.values())     # False: only gravity (or nothing) was given; the scales are ones
        for name in SCALE_NAMES:
            a = np.ones(n, np.float32) if vals[name] is None else vals[name]
            a.setflags(write=False)
            setattr(self, name, a)

    def table(self) -> np.ndarray:
        """[3][num_envs] float32: what tmjx_set_env_scales reads (rows friction | actuator | damping)."""
        return np.ascontiguousarray(np.stack([self.friction, self.actuator, self.damping], 0), dtype=np.float32)

    def gravity_table(self) -> np.ndarray | None:
        """[3][num_envs] float32, rows gx | gy | gz: what tmjx_set_env_gravity reads (None: no per-env gravity)."""
        return None if self.gravity is None else np.ascontiguousarray(self.gravity.T, dtype=np.float32)

    def shard(self, lo: int, hi: int) -> "DomainRandomization":
        """The scales of envs lo .. hi of this draw (a rank's or an env group's slice of the global draw)."""
        if not 0 <= lo < hi <= self.num_envs:
            raise ValueError(f"DomainRandomization.shard: [{lo}, {hi}) outside the {self.num_envs} envs")
        sc = [getattr(self, name)[lo:hi] if self.has_scales else None for name in SCALE_NAMES]
        return DomainRandomization(*sc, num_envs=hi - lo, gravity=None if self.gravity is None else self.gravity[lo:hi])

    def __eq__(self, other):
        if not (isinstance(other, DomainRandomization) and np.array_equal(self.table(), other.table())):
            return False
        if self.gravity is None or other.gravity is None:
            return self.gravity is None and other.gravity is None
        return np.array_equal(self.gravity, other.gravity)

    __hash__ = None

    def __repr__(self):
        r = lambda a: f"[{a.min():.4g}, {a.max():.4g}]"      # noqa: E731
        g = "" if self.gravity is None else f", |gravity|={r(np.linalg.norm(self.gravity.astype(np.float64), axis=1))}"
        return f"DomainRandomization(num_envs={self.num_envs}, friction={r(self.friction)}, actuator={r(self.actuator)}, damping={r(self.damping)}{g})"


def _range(name: str, r):
    if r is None:
        return None
    try:
        lo, hi = (float(x) for x in r)
    except (TypeError, ValueError):
        raise ValueError(f"{name} range must be (lo, hi), got {r!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo <= 0 or hi < lo:
        raise ValueError(f"{name} range must be finite with 0 < lo <= hi, got ({lo}, {hi})")
    return lo, hi


def _tilt_range(name: str, r):
    if r is None:
        return None
    try:
        lo, hi = (float(x) for x in r)
    except (TypeError, ValueError):
        raise ValueError(f"{name} range must be (lo, hi) in degrees, got {r!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo < 0 or hi < lo or hi > 90:
        raise ValueError(f"{name} range must be finite with 0 <= lo <= hi <= 90 degrees, got ({lo}, {hi})")
    return lo, hi


DEFAULT_GRAVITY = (0.0, 0.0, -9.81)


def gravity_vectors(gravity, scale, tilt_deg, azimuth) -> np.ndarray:
    """[n, 3] float32: `scale` |g| along the model's gravity direction tilted by `tilt_deg` toward the azimuth `azimuth` (radians, measured in
    the plane across g from the world x axis projected into it; for g along -z: azimuth 0 tilts toward +x, pi / 2 toward -y).  Built in float64."""
    g0 = np.asarray(gravity, dtype=np.float64).reshape(3)
    mag = float(np.linalg.norm(g0))
    if not (np.isfinite(mag) and mag > 0):
        raise ValueError(f"the model's gravity {g0.tolist()} has no direction to scale or tilt")
    u = g0 / mag
    ax = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = ax - (ax @ u) * u
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    s, t, az = (np.asarray(x, dtype=np.float64) for x in (scale, np.deg2rad(np.asarray(tilt_deg, dtype=np.float64)), azimuth))
    d = np.cos(t)[:, None] * u + np.sin(t)[:, None] * (np.cos(az)[:, None] * e1 + np.sin(az)[:, None] * e2)
    return (s[:, None] * mag * d).astype(np.float32)


def uniform_scales(num_envs: int, key, friction=None, actuator=None, damping=None, gravity_scale=None, gravity_tilt_deg=None,
                   gravity=DEFAULT_GRAVITY) -> DomainRandomization:
    """Scales drawn uniformly from the given (lo, hi) ranges (None: that scale stays 1) with jax.random's threefry `uniform`: `key` (a jax PRNG
    key, [2] uint32, or an int seed) is split in three, one sub-key per scale in the order friction, actuator, damping, whether or not the scale
    is drawn — the same key gives the same scales wherever it is evaluated.

    `gravity_scale` (lo, hi): each env's |gravity| as a multiple of the model's; `gravity_tilt_deg` (lo, hi): the angle between the env's
    gravity and the model's, with the azimuth uniform in [0, 2 pi).  `gravity` is the model's gravity vector (model["gravity"] of a
    randomization_fn's argument).  Their three sub-keys (scale, tilt, azimuth) are split from fold_in(key, 3), behind the three above: the
    friction / actuator / damping draws of a key do not depend on whether gravity is drawn.  Both None: no per-env gravity."""
    from .. import jax_random as jr
    n = int(num_envs)
    if n < 1:
        raise ValueError("uniform_scales: num_envs must be >= 1")
    key = jr.PRNGKey(int(key)) if isinstance(key, (int, np.integer)) else np.asarray(key, dtype=np.uint32)
    if key.shape != (2,):
        raise ValueError("uniform_scales: key must be a jax PRNG key ([2] uint32) or an int seed")
    keys = jr.split(key, 3)
    out = []
    for k, name, r in zip(keys, SCALE_NAMES, (friction, actuator, damping)):
        r = _range(name, r)
        # (lo == hi: jax's uniform returns max(lo, f * 0 + lo) = lo)
        out.append(None if r is None else np.clip(jr.uniform(k, (n,), r[0], r[1]), np.float32(r[0]), np.float32(r[1])))
    gs, gt = _range("gravity_scale", gravity_scale), _tilt_range("gravity_tilt_deg", gravity_tilt_deg)
    gvec = None
    if gs is not None or gt is not None:
        ks, kt, ka = jr.split(jr.fold_in(key, 3), 3)
        one = lambda k, r: np.clip(jr.uniform(k, (n,), r[0], r[1]), np.float32(r[0]), np.float32(r[1]))      # noqa: E731
        scale = np.ones(n) if gs is None else one(ks, gs)
        tilt = np.zeros(n) if gt is None else one(kt, gt)
        az = jr.uniform(ka, (n,), 0.0, 2.0 * np.pi)
        gvec = gravity_vectors(gravity, scale, tilt, az)
    return DomainRandomization(*out, num_envs=n, gravity=gvec)


def shard_scales(dr: DomainRandomization | None, rank: int, world: int) -> DomainRandomization | None:
    """Rank `rank` of `world`'s contiguous, equal share of the global draw (None stays None)."""
    if dr is None:
        return None
    if world < 1 or not 0 <= rank < world or dr.num_envs % world:
        raise ValueError(f"shard_scales: {dr.num_envs} envs do not split over rank {rank} of {world}")
    per = dr.num_envs // world
    return dr.shard(rank * per, (rank + 1) * per)


def model_view(env, num_envs: int | None = None) -> Mapping:
    """What a randomization_fn is called with: a read-only mapping of the walker's blob entries (model constants by the names
    tools/compile_model.py writes: con_friction, act_gain, dof_damping, ...) plus `num_envs` (the env's own count, or the given one:
    ppo.train asks for the GLOBAL draw and shards it)."""
    from .. import blob as _blob
    entries = dict(_blob.unpack(env._blob))
    for v in entries.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    entries["num_envs"] = int(env.num_envs if num_envs is None else num_envs)
    return MappingProxyType(entries)


def apply_randomization_fn(env, randomization_fn) -> None:
    """wrap(env, randomization_fn=fn): fn(model) -> DomainRandomization, applied to the env.  Anything else — the model itself, a brax-style
    (sys, in_axes) tuple — is a per-env MODEL, which is not supported."""
    out = randomization_fn(model_view(env))
    if not isinstance(out, DomainRandomization):
        raise NotImplementedError(
            "domain randomisation with a per-env model is not supported (the device model is one constant per handle); per-env SCALES are: "
            "return an environment.DomainRandomization(friction=, actuator=, damping=, gravity=) from randomization_fn (environment.uniform_scales draws one), "
            f"not {type(out).__name__}")
    env.set_domain_randomization(out)


def uniform_randomization_fn(friction=None, actuator=None, damping=None, gravity_scale=None, gravity_tilt_deg=None):
    """A `randomization_fn` for ppo.train drawing uniform_scales from the given ranges: fn(model, rng) -> DomainRandomization for
    model["num_envs"] envs from the key ppo.train hands it (key_env for the training envs, eval_key for the evaluator's).  All ranges None: None.
    `fn.ranges` names the three scales' ranges, and `gravity_scale` / `gravity_tilt_deg` when they are drawn (about model["gravity"])."""
    ranges = dict(friction=_range("friction", friction), actuator=_range("actuator", actuator), damping=_range("damping", damping))
    grav = dict(gravity_scale=_range("gravity_scale", gravity_scale), gravity_tilt_deg=_tilt_range("gravity_tilt_deg", gravity_tilt_deg))
    grav = {k: v for k, v in grav.items() if v is not None}
    if all(v is None for v in ranges.values()) and not grav:
        return None

    def fn(model, rng):
        if not grav:
            return uniform_scales(int(model["num_envs"]), rng, **ranges)
        if "gravity" not in model:
            raise ValueError("uniform_randomization_fn: gravity ranges need the model's `gravity` entry")
        return uniform_scales(int(model["num_envs"]), rng, **ranges, **grav, gravity=np.asarray(model["gravity"], dtype=np.float64))
    fn.ranges = dict(ranges, **grav)
    return fn


def randomization_keys(seed: int):
    """(key_env, eval_key) as the reference's ppo.train derives them from `seed` (agent/mlp_ppo/ppo.py:443-447) for process 0: the randomisation
    draw is GLOBAL — every rank evaluates the same key and takes its shard (ppo.py:458-460: all devices get the same randomisation rng)."""
    from .. import jax_random as jr
    _, local_key = jr.split(jr.PRNGKey(int(seed)))
    local_key = jr.fold_in(local_key, 0)
    _, key_env, eval_key = jr.split(local_key, 3)
    return key_env, eval_key


def draw_for_training(randomization_fn, env, rng, num_envs: int) -> DomainRandomization:
    """randomization_fn(model, rng) for `num_envs` envs of `env`'s model, checked."""
    out = randomization_fn(model_view(env, num_envs), rng)
    if not isinstance(out, DomainRandomization):
        raise NotImplementedError("ppo.train: randomization_fn(model, rng) must return an environment.DomainRandomization (per-env scales); a per-env "
                                  f"model is not supported, got {type(out).__name__}")
    if out.num_envs != int(num_envs):
        raise ValueError(f"ppo.train: randomization_fn returned scales for {out.num_envs} envs, asked for {num_envs}")
    return out
