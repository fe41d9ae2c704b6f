/* include/tmjx.h — C-ABI of libtmjx_hip.so: the MI355X-native hot path of talmolab/track-mjx.
 *
 * The reference has no FFI/plugin boundary for this path (it is 100 % Python on JAX/XLA); the
 * entry points below are what a binding for the reference's Python interfaces would call.
 * Each entry cites the reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - return 0 on success, a negative TMJX_E* code on failure; never throws; the message of the
 *     last failure on the calling thread is available from tmjx_last_error().
 *   - every per-env buffer is CALLER-OWNED DEVICE memory (e.g. a torch tensor's data_ptr) laid
 *     out structure-of-arrays with the ENV INDEX CONTIGUOUS:  buf[field_index * n_env + env].
 *   - the library owns only the immutable model constants and the clip table of a handle, plus ONE
 *     piece of per-handle device scratch: the physics kernel's per-env copy of the inertia matrix
 *     (4.5 KB per env for the rodent), allocated at the first launch and re-allocated only when a
 *     later launch has more envs (that one call synchronises the device; every other call enqueues only).
 *   - all work is enqueued on the caller's HIP stream; no hidden synchronisation (see above).
 *   - one handle per host thread / GPU AND per stream: launches of one handle must not overlap
 *     (thread-compatible, not thread-safe; pipelined env groups use one handle each).
 *   - `stream` is a hipStream_t passed as void* so that this header needs no HIP include.
 */
#ifndef TMJX_H
#define TMJX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMJX_OK 0
#define TMJX_EINVAL (-22)
#define TMJX_ENOMEM (-12)
#define TMJX_EHIP (-5)

typedef struct tmjx_model tmjx_model;

/* Float state layout (rows of the `state` buffer, each row n_env floats). Query with tmjx_layout(). */
typedef struct tmjx_layout_t {
  int32_t nq, nv, nu, nbody, ncon, nefc, obs_size, ref_obs_size, n_metrics, window;
  /* rows of the float state buffer */
  int32_t qpos, qvel, act, qacc_warmstart, time;          /* physics state (mjx.Data fields carried)      */
  int32_t xpos, xmat_torso, qfrc_actuator;                 /* outputs of the last mjx.forward read by K3   */
  int32_t prev_ctrl, action_buffer, done, steps_f;         /* task info (single_clip_tracking.py:227-234)  */
  int32_t first_phys, first_obs, first_prev_ctrl;          /* auto-reset snapshot (wrappers.py:93-95)       */
  int32_t state_rows;                                      /* total float rows                              */
  /* rows of the int32 state buffer */
  int32_t i_clip_idx, i_start_frame, i_buffer_index, i_nan_count, istate_rows;
  int32_t ws_rows;                                         /* float rows of the scratch workspace           */
} tmjx_layout_t;

/* Model handle from the compiled blob (model constants + env/task configuration).
 * Replaces: SingleClipTracking.__init__ (track_mjx/environment/task/single_clip_tracking.py:25-92:
 * solver options, mjcf load, mjx.put_model) and RewardConfig (task/reward.py:15-54). */
int tmjx_model_create(const void *blob, size_t nbytes, tmjx_model **out);
void tmjx_model_destroy(tmjx_model *m);
int tmjx_layout(const tmjx_model *m, tmjx_layout_t *out);

/* Episode / auto-reset wrapper semantics of the handle: wrappers.wrap(env, episode_length, ...) (track_mjx/environment/wrappers.py:18-56:
 * brax EpisodeWrapper's step counter / truncation at `episode_length`, and the (LSTM)AutoResetWrapperTracking restore on done).  Only
 * the two constants change; the clip table of the handle stays resident.  Blocking; not to be called with launches in flight. */
int tmjx_set_wrappers(tmjx_model *m, int episode_length, int auto_reset);
/* What tmjx_step / tmjx_step_sensors do, after the last action repeat, with an env whose step ended with done set (terminated or truncated):
 *   TMJX_DONE_NONE   nothing: the env keeps stepping from where it is (tmjx_set_wrappers(m, L, 0));
 *   TMJX_DONE_RESET  (LSTM)AutoResetWrapperTracking: physics state, observation and prev_ctrl <- the snapshot of the last tmjx_reset
 *                    (tmjx_set_wrappers(m, L, 1));
 *   TMJX_DONE_ALIGN  AutoAlignWrapperTracking (track_mjx/environment/wrappers.py:328-381): qpos <- position | quaternion | joints and
 *                    qvel <- velocity | angular_velocity | joints_velocity of the clip frame the step computed its reward against
 *                    (floor(time * mocap_hz + start_frame), clamped to the clip's last frame), no noise; kinematics on that state (xpos, torso
 *                    xmat); the observation rebuilt from it with the unchanged clip / start frame.  time is not rewound; act, qacc_warmstart,
 *                    qfrc_actuator, prev_ctrl, the action buffer, reward, done, truncation and metrics stay those of the terminated step.
 *                    The step counter is zeroed by the next step's prologue, as under the other policies.  Envs that are not done come out
 *                    bit for bit as under TMJX_DONE_NONE.  Needs the wave-per-env implementation and tmjx_clips_upload_velocities; where K3
 *                    runs as one kernel (tmjx_reward_frame, tmjx_reward_obs without a workspace) the policy is refused with an error.
 * tmjx_set_wrappers sets NONE / RESET as its auto_reset argument says; call this after it.  Blocking; not with launches in flight. */
#define TMJX_DONE_NONE 0
#define TMJX_DONE_RESET 1
#define TMJX_DONE_ALIGN 2
int tmjx_set_done_policy(tmjx_model *m, int policy);
/* Per-env domain randomisation: brax's DomainRandomizationVmapWrapper (track_mjx/environment/wrappers.py:44-47), restricted to three SCALARS per
 * env.  `scales_dev` is DEVICE memory, float32 [3][n_env]: row 0 scales every contact's sliding friction, row 1 the actuators' force (gain and
 * the affine bias pair; ctrlrange and the activation time constant are not scaled), row 2 the dofs' damping (passive force and the
 * timestep * damping diagonal of the implicit Euler step).  Env e of a launch reads column e.  The scale multiplies the MODEL CONSTANT before it
 * is used, so a power-of-two scale reproduces bit for bit a handle whose blob was scaled on the host.  The handle stores the pointer and the
 * count; the caller owns the memory and keeps it alive and unchanged while launches read it.  Nothing on the device is validated.  NULL clears
 * the scales: the handle then launches exactly what it launched before (the product kernel; the RAND kernel, csrc/tmjx_wave_rand.hip, runs only
 * while scales are set).  Honoured by every launch of the physics kernel: tmjx_step (each action repeat, under all three done-policies),
 * tmjx_physics, tmjx_physics_step, and the forward pass of tmjx_forward / tmjx_reset; a launch of more envs than `n_env` fails with
 * TMJX_EINVAL.  The reward / observation kernels and the align policy's epilogue read no scaled constant and are unchanged.
 * tmjx_physics_sensors / tmjx_step_sensors refuse a handle with scales (the recording kernel has no RAND build), as does a handle of the
 * lane-per-env cross-check implementation.  Per-env models, masses and per-geom / per-dof / per-actuator vectors are not supported. */
int tmjx_set_env_scales(tmjx_model *m, const float *scales_dev, int n_env);
/* Per-env gravity, the second table of the same kernel: `gravity_dev` is DEVICE memory, float32 [3][n_env], rows gx, gy, gz in the world frame
 * (m/s^2).  Env e of a launch integrates with column e in place of the model's `gravity`, which the physics reads in one place — the root
 * acceleration of the bias-force pass —, so env e reproduces bit for bit a handle created from the blob with `gravity` set to that column.  A
 * tilted vector is, in this model's flat world, an inclined floor; a shorter one body-weight support.  The contract is tmjx_set_env_scales':
 * the caller owns the memory and keeps it alive and unchanged while launches read it, nothing on the device is validated, n_env >= 1, NULL
 * clears the table, the wave-per-env implementation is needed.  The two tables are independent: the RAND kernel runs while either is set and
 * takes unit scales / the model's gravity for the one that is not; with both cleared the handle launches the product kernel again.  Honoured by
 * every launch of the physics kernel (tmjx_step under all three done-policies, tmjx_physics, tmjx_physics_step, the forward pass of
 * tmjx_forward / tmjx_reset, split launches with their env offset); a launch of more envs than `n_env` fails with TMJX_EINVAL before anything is
 * enqueued.  tmjx_physics_sensors / tmjx_step_sensors refuse a handle with a gravity table (the recording kernel's sensor stage reads the
 * model's gravity). */
int tmjx_set_env_gravity(tmjx_model *m, const float *gravity_dev, int n_env);
/* `action_repeat` of wrappers.wrap (track_mjx/environment/wrappers.py:21,43 -> brax EpisodeWrapper.step [3P]): tmjx_step then runs the
 * tracking env's own step `action_repeat` times with the same action (no termination check in between), returns the SUM of the repeats'
 * rewards, advances the episode's step counter by `action_repeat`, and takes observation / done / truncation / metrics from the last
 * repeat; the auto-reset follows the last repeat.  Default 1.  Host-side only (nothing is copied); tmjx_reward_obs, the K3-alone entry,
 * is one inner step whatever the repeat count. */
int tmjx_set_action_repeat(tmjx_model *m, int action_repeat);

/* Upload the ReferenceClip table (HOST pointers, float32, shapes (C,F,3) (C,F,4) (C,F,nq-7)
 * (C,F,nbody-1,3) (C,F,3)); the table becomes a resident device constant of the handle.
 * Replaces: the `reference_clip` constructor argument (task/multi_clip_tracking.py:16-72) whose
 * leaves are laid out by track_mjx/io/load.py:16-38,105-137. */
int tmjx_clips_upload(tmjx_model *m, const float *position, const float *quaternion, const float *joints,
                      const float *body_positions, const float *angular_velocity, int n_clips, int n_frames);

/* reset: MultiClipTracking.reset -> reset_from_clip (task/multi_clip_tracking.py:74-96,
 * task/single_clip_tracking.py:121-205) + the wrappers' reset (wrappers.py:88-102, brax
 * EpisodeWrapper.reset).  (clip_idx, start_frame, noise) are inputs because JAX's threefry stream
 * is outside this path; qpos_noise is [nq][n_env], qvel_noise [nv][n_env].  Writes obs [obs][n_env]. */
int tmjx_reset(tmjx_model *m, float *state, int32_t *istate, const int32_t *clip_idx, const int32_t *start_frame,
               const float *qpos_noise, const float *qvel_noise, float *obs, float *workspace, int n_env, void *stream);

/* step: wrappers.wrap(env).step = LSTMAutoResetWrapperTracking.step ∘ VmapWrapper ∘ EpisodeWrapper.step ∘
 * MultiClipTracking.step (wrappers.py:104-144; task/single_clip_tracking.py:207-320).
 * action [nu][n_env]; outputs obs [obs][n_env], reward/done/truncation [n_env], metrics [20][n_env]. */
int tmjx_step(tmjx_model *m, float *state, int32_t *istate, const float *action, float *obs, float *reward,
              float *done, float *truncation, float *metrics, float *workspace, int n_env, void *stream);

/* The physics part of tmjx_step alone: n_frames substeps with the handle's configuration, through the same launches
 * (state -> env-major record, wave-per-env kernel, record -> state; the record lives in `workspace`).  bench.py times this. */
int tmjx_physics_step(tmjx_model *m, float *state, const float *action, float *workspace, int n_env, void *stream);

/* K2 alone: `n_substeps` x (ctrl = action; mjx.step) on the physics rows of `state`
 * (brax PipelineEnv.pipeline_step, called at task/single_clip_tracking.py:219). */
int tmjx_physics(tmjx_model *m, float *state, const float *action, int n_substeps, float *workspace, int n_env,
                 void *stream);
/* Sensor outputs (checkpoint roll-outs with log_sensor_data; reference: track_mjx/analysis/rollout.py), through the RECORDING physics
 * kernel — K2 with a sensor stage between the solve and Euler of the last substep (mjx.step = forward, then euler: the values belong to the
 * last substep's starting qpos / qvel and to its solve's qacc / efc_force, like qfrc_actuator).  Both outputs are [row][n_env], device memory:
 *   sensordata [nsensordata][n_env]: the model's sensors in blob order (rodent: head accelerometer, velocimeter, gyro in the site frame,
 *              torso subtreelinvel in the world frame); may be NULL when the model has no sensors;
 *   cfrc_ext   [nbody * 6][n_env]: per body [torque(3), force(3)] of the contact forces about subtree_com[body_rootid] (mj_rnePostConstraint:
 *              minus on geom 1's body, plus on geom 2's; row block 0, the world, stays 0).
 * tmjx_sensor_info: sizes of the two (nsensordata = 0 for a model without sensors). */
int tmjx_sensor_info(const tmjx_model *m, int *nsensordata, int *nbody);
/* tmjx_physics through the recording kernel (n_substeps >= 1). */
int tmjx_physics_sensors(tmjx_model *m, float *state, const float *action, int n_substeps, float *sensordata, float *cfrc_ext,
                         float *workspace, int n_env, void *stream);
/* tmjx_step through the recording kernel: the same launches and results (state, obs, reward, done, truncation, metrics bit for bit);
 * with action_repeat R the outputs are those of the last repeat's last substep; with auto-reset on, those of the physics that ran,
 * before K3 restores a done env. */
int tmjx_step_sensors(tmjx_model *m, float *state, int32_t *istate, const float *action, float *obs, float *reward, float *done,
                      float *truncation, float *metrics, float *workspace, float *sensordata, float *cfrc_ext, int n_env, void *stream);
/* mjx.forward alone on the physics rows of `state` (pipeline_init, task/single_clip_tracking.py:163). */
int tmjx_forward(tmjx_model *m, float *state, float *workspace, int n_env, void *stream);

/* K3 alone: everything in step() except the physics substeps: frame index, clip gather, rewards,
 * observation, done/NaN guard, episode + auto-reset wrappers (task/single_clip_tracking.py:220-320,
 * task/reward.py:359-485, wrappers.py:104-144).
 * `workspace` (>= 2*nu rows) receives the per-(action dim, env) window partials; NULL computes them inline. */
int tmjx_reward_obs(tmjx_model *m, float *state, int32_t *istate, const float *action, float *obs, float *reward,
                    float *done, float *truncation, float *metrics, float *workspace, int n_env, void *stream);

/* compute_tracking_rewards as the reference calls it (task/reward.py:359-366; call site task/single_clip_tracking.py:239-246): the
 * reward / termination part of K3 with the CALLER's gathered reference frame per env instead of the handle's own gather from the resident
 * clip table.  frame_* are device pointers, row-major per env: position [n][3], quaternion [n][4], joints [n][nq-7], body_positions
 * [n][nbody-1][3], angular_velocity [n][3] (ReferenceClip leaves of one frame, track_mjx/io/load.py:16-38).  Everything else as
 * tmjx_reward_obs with workspace = NULL (the observation's trajectory part still reads the resident table). */
int tmjx_reward_frame(tmjx_model *m, float *state, int32_t *istate, const float *action, const float *frame_pos,
                      const float *frame_quat, const float *frame_joints, const float *frame_bodypos, const float *frame_angvel,
                      float *obs, float *reward, float *done, float *truncation, float *metrics, int n_env, void *stream);

/* GAE reverse scan: compute_gae (track_mjx/agent/mlp_ppo/losses.py:39-100). All arrays [T][B] row-major
 * (B contiguous), bootstrap [B]; outputs vs, advantages [T][B]. */
int tmjx_gae(const float *truncation, const float *termination, const float *rewards, const float *values,
             const float *bootstrap, float lambda_, float discount, float *vs, float *advantages, int T, int B,
             void *stream);

/* PPO loss head, forward and gradients w.r.t. the network outputs in one call: compute_ppo_loss
 * (track_mjx/agent/mlp_ppo/losses.py:103-245) from the policy logits on: NormalTanh log-prob / entropy, GAE
 * (losses.py:39-100), advantage normalisation, clipped surrogate, value loss, AR(1)-prior latent KL.
 * Row-major device arrays: logits [T][B][2A], raw_action / noise [T][B][A], behaviour_logp / baseline / reward /
 * discount / truncation [T][B], bootstrap [B], fc2 = latent mean | logvar [T][B][2Z]; outputs dlogits, dbaseline,
 * dfc2 (same shapes as their inputs) = d total / d input; out[8] = total, policy_loss, v_loss, entropy_loss,
 * kl_latent_loss, advantage mean, advantage std, entropy; scratch >= tmjx_ppo_scratch_floats(T, B) floats. */
typedef struct {
  int32_t T, B, A, Z;
  float reward_scaling, discounting, gae_lambda, clip_eps, entropy_cost, kl_weight;
  int32_t normalize_advantage;
  int32_t accumulate;              /* 1: out[0..7] += this call's values (a running sum over the minibatch steps of an update), 0: out = values */
} tmjx_ppo_cfg_t;
int tmjx_ppo_scratch_floats(int T, int B);
int tmjx_ppo_loss(const tmjx_ppo_cfg_t *cfg, const float *logits, const float *raw_action, const float *behaviour_logp,
                  const float *noise, const float *baseline, const float *bootstrap, const float *reward, const float *discount,
                  const float *truncation, const float *fc2, float *dlogits, float *dbaseline, float *dfc2, float *scratch,
                  float *out, void *stream);

/* The same loss head in phases, for a caller that runs the policy and the value network on two streams: A (log-prob, entropy, KL sums) reads the policy's
 * outputs only, B (GAE, advantage statistics, value loss) the value network's only, C (surrogate + every gradient) both, D writes out[8].  Each call launches
 * the phases of its mask on its stream; the caller orders them (A, B before C; C before D).  unroll_length T <= 24.  Gradients: the bits of tmjx_ppo_loss;
 * the entropy / KL scalars are added up in another order. */
#define TMJX_PPO_PHASE_A 1
#define TMJX_PPO_PHASE_B 2
#define TMJX_PPO_PHASE_C 4
#define TMJX_PPO_PHASE_D 8
int tmjx_ppo_loss_phases(const tmjx_ppo_cfg_t *cfg, const float *logits, const float *raw_action, const float *behaviour_logp,
                         const float *noise, const float *baseline, const float *bootstrap, const float *reward, const float *discount,
                         const float *truncation, const float *fc2, float *dlogits, float *dbaseline, float *dfc2, float *scratch,
                         float *out, int phases, void *stream);

/* Dense -> SiLU -> LayerNorm epilogue of the intention network's hidden layers (intention_network.py:14-88):
 * y = LayerNorm_{gamma,beta,eps}(silu(z + bias)), z [rows][H] = the GEMM output, H in {64, 128, 256, 512, 1024}.
 * fwd also writes stats [rows][2] = mean, rstd; bwd returns dz and grads [3][H] = d_gamma | d_beta | d_bias;
 * partial >= tmjx_silu_ln_partial_floats(rows, H) floats of scratch. */
int tmjx_silu_ln_partial_floats(int rows, int H);
int tmjx_silu_ln_fwd(const float *z, const float *bias, const float *gamma, const float *beta, float *y, float *stats, int rows, int H,
                     float eps, void *stream);
int tmjx_silu_ln_bwd(const float *dy, const float *z, const float *bias, const float *gamma, const float *stats, float *dz, float *grads,
                     float *partial, int rows, int H, void *stream);
/* The same two kernels with a bf16 result (y16 / dz16: [rows][ld >= H], round to nearest even) for consumers that are bf16-operand GEMMs
 * (tmjx_bgemm_*: the 1024-wide first encoder block of the rodent-mc-intention nets, which is not one GEMM tile wide): the bits those GEMMs would have
 * made of the fp32 result when they stage it, without the fp32 round trip through memory.  Statistics and column sums stay fp32. */
int tmjx_silu_ln_fwd_bf16(const float *z, const float *bias, const float *gamma, const float *beta, uint16_t *y16, int ldy16, float *stats, int rows, int H,
                          float eps, void *stream);
int tmjx_silu_ln_bwd_bf16(const float *dy, const float *z, const float *bias, const float *gamma, const float *stats, uint16_t *dz16, int lddz16, float *grads,
                          float *partial, int rows, int H, void *stream);

/* Minibatch gather fused with the observation normaliser (ppo.py:306-311 + running_statistics.normalize):
 * out[t][b][:] = (src[t][idx[b]][:] - mean) / std; src [T][R][W], idx int64 [B], out [T][B][W], W % 4 == 0. */
int tmjx_gather_normalize(const float *src, const int64_t *idx, const float *mean, const float *std, float *out, int T, int R, int B,
                          int W, void *stream);
/* The whole minibatch of one SGD step in one launch (ppo.py:304-317: the same permutation slice indexes every leaf of the roll-out data):
 * obs_n [T][B][W] = (obs[t][idx[b]] - mean) / std, next_n [B][W] likewise from next_last [R][W], raw_action_g [T][B][A] = raw_action[t][idx[b]],
 * scalars_g [4][T][B] = (log_prob, reward, discount, truncation)[t][idx[b]].  idx: int64 [B] on the device, values in [0, R). */
int tmjx_gather_minibatch(const float *obs, const float *next_last, const float *raw_action, const float *log_prob, const float *reward, const float *discount,
                          const float *truncation, const int64_t *idx, const float *mean, const float *std, float *obs_n, float *next_n, float *raw_action_g,
                          float *scalars_g, int T, int R, int B, int W, int A, void *stream);
/* The same launch as the first kernel of a SELF-ADVANCING SGD step (a captured hipGraph replays it without any host input): the rows are
 * perm[slot B .. slot B + B) with slot = state[1]; the launch also draws the step's two N(0, 1) arrays — eps [T B Z] (the latent sample of
 * intention_network.py:78-88) and noise [T B A] (the entropy sample of losses.py:222) — from Philox4x32-10 keyed by `seed`, counter state[0],
 * and, with `advance`, adds 1 to state[0] and state[1] once every workgroup is done (state: device int64[TMJX_MINIBATCH_STATE_WORDS], {draw counter, slot, 0, 0, ...}:
 * words 2 .. are the launch's completion tickets and must be zero).
 * The host resets state[1] and refills `perm` once per epoch (ppo.py:304-311: one permutation per update over the batch). */
#define TMJX_MINIBATCH_STATE_WORDS (16 + 16 * 64)
typedef struct tmjx_minibatch_t {
  const float *obs, *next_last, *raw_action, *log_prob, *reward, *discount, *truncation;
  const int64_t *perm;
  const float *mean, *std;
  float *obs_n, *next_n, *raw_action_g, *scalars_g;
  float *eps, *noise;            /* may be NULL */
  int64_t *state;                /* may be NULL when eps, noise are NULL and advance == 0 (then slot = 0) */
  uint64_t seed;
  int32_t T, R, B, W, A, Z, advance;
} tmjx_minibatch_t;
int tmjx_minibatch_begin(const tmjx_minibatch_t *mb, void *stream);
/* The same launch with a bf16 TWIN of obs_n next to it (bf16 GEMM-input mode): obs_n16 [T B][ld16 >= W], the normalised observation rounded to
 * nearest even — the operand the first layers' bf16 GEMMs (tmjx_bgemm_*) would have made of obs_n when they stage it.  Columns W .. ld16 - 1 are
 * not written (the caller keeps them zero, so that a contraction may run to the next multiple of 64 by LDS-DMA). */
int tmjx_minibatch_begin_bf16(const tmjx_minibatch_t *mb, uint16_t *obs_n16, int ld16, void *stream);
/* Philox4x32-10 of (counter[4], key[2]) = six device words -> four device words: the generator above, exposed for its known-answer test */
int tmjx_philox4x32_10(const uint32_t *ctr_key_dev, uint32_t *out_dev, void *stream);

/* Backward of the latent sample inside tmjx_latent_concat (reparameterize, intention_network.py:78-88): from d x [n][dx_stride]
 * to d fc2 [n][2 Z] = [d mean | d logvar]. */
int tmjx_latent_concat_bwd(const float *dx, const float *eps, const float *fc2, float *dfc2, int n, int Z, int dx_stride, void *stream);
/* The same with a second gradient of fc2 summed in (`add` [n][2 Z]: the KL term's, compute_ppo_loss's kl_latent_loss, losses.py:196-237): d fc2 =
 * add + the sample's gradient, as jax.grad sums the two uses of the encoder's output (intention_network.py:128-139). */
int tmjx_latent_concat_bwd_add(const float *dx, const float *eps, const float *fc2, const float *add, float *dfc2, int n, int Z, int dx_stride,
                               void *stream);

/* Policy inference tails (ppo_networks.py:46-96, intention_network.py:78-88).
 * tmjx_latent_concat: x[i] = [ mean_i + eps_i * exp(logvar_i / 2) | obs_i[ref_w:] ], fc2 [n][2Z] = mean | logvar, eps [n][Z], obs
 *   addressed as obs[i * obs_s0 + c * obs_s1] (so the [obs][n_env] buffer of tmjx_step can be passed as is) and normalised with
 *   (. - mean[c]) / std[c] when mean != NULL, x [n][x_stride >= Z + obs_w - ref_w] (columns beyond are written as zeros).
 * tmjx_sample_action: raw = loc + (softplus(raw_scale) + 0.001) * noise; action = tanh(raw) written as [A][n] (the layout
 *   tmjx_step takes); logp = NormalTanh log-prob of the sample; logits [n][2A], noise / raw [n][A], logp [n].
 * eps == NULL / noise == NULL: the N(0, 1) draws are made on the device, Philox4x32-10 streams 2 / 3 of (seed, draw counter rng_state[0]);
 *   rng_state = device int64[2] {draw counter, 0}; tmjx_sample_action then advances the counter once all its workgroups are done, so one
 *   inference = tmjx_latent_concat ... tmjx_sample_action on the same stream uses one counter value and a captured graph of it replays
 *   with fresh noise and no host input. */
int tmjx_latent_concat(const float *fc2, const float *eps, const float *obs, float *x, int n, int Z, int obs_w, int ref_w,
                       int64_t obs_s0, int64_t obs_s1, const float *mean, const float *std, int x_stride, uint64_t seed, const int64_t *rng_state,
                       void *stream);
int tmjx_sample_action(const float *logits, const float *noise, float *raw, float *action_t, float *logp, int n, int A, uint64_t seed,
                       int64_t *rng_state, void *stream);

/* The acting policy's dense layer (brax acting.actor_step through make_inference_fn, track_mjx/agent/mlp_ppo/ppo_networks.py:46-96; layers of
 * intention_network.py:32-44,68-76) through a 20 KB LDS tile — what the CUs have free next to twelve resident physics workgroups since round 5:
 * C[M][N] = op(A) W^T (+ bias), A row-major [M][lda], W [N][ldw], op = identity or (A - mean[k]) * inv_std[k] (mean / inv_std: both or neither).
 * tmjx_linear_act_ok: 1 when the operands qualify (K % 4 == 0, 16-byte aligned rows); otherwise use tmjx_linear_nolds. */
int tmjx_linear_act_ok(const float *A, int64_t lda, const float *W, int ldw, int K);
int tmjx_linear_act(const float *A, int64_t lda, const float *W, int ldw, const float *bias, float *C, int M, int N, int K,
                    const float *mean, const float *inv_std, void *stream);
/* LDS-free dense layer (policy inference next to the physics kernel, which owns every CU's LDS):
 * C[M][N] = A W^T + bias (bias may be NULL); W [N][K] row-major; A[i][k] at A[i * sa_row + k * sa_k] with either sa_k == 1
 * (row-major activations) or sa_row == 1 (the [obs][n_env] buffer; M % 4 == 0 and 16-byte aligned columns required). */
int tmjx_linear_nolds(const float *A, int64_t sa_row, int64_t sa_k, const float *W, const float *bias, float *C, int M, int N, int K,
                      void *stream);
/* The same with the operand normalised while it is loaded: C = ((A - mean[k]) * inv_std[k]) W^T + bias (mean, inv_std: [K] device vectors) — the
 * acting policy's first layer reading the env's RAW observation buffer (brax running_statistics.normalize, track_mjx/agent/mlp_ppo/ppo_networks.py:46-60).
 * Matrix-core variant only: K % 4 == 0, 16-byte aligned operands. */
int tmjx_linear_nolds_norm(const float *A, int64_t sa_row, int64_t sa_k, const float *W, const float *bias, float *C, int M, int N, int K,
                           const float *mean, const float *inv_std, void *stream);

/* The LDS-free dense layer in bf16 GEMM-input mode (BASELINE config 5): the fp32 activations are rounded to bf16 in registers, W is the layer's
 * resident bf16 shadow [N][ldw] (tmjx_bf16_shadow: rows zero padded to ldw, a multiple of 64), fp32 accumulate on v_mfma_f32_16x16x32_bf16 — the
 * operand rounding of the learner's tmjx_bgemm_* forward pass, so that the roll-out's behaviour log-prob and the learner's first-pass log-prob
 * agree (reference: one jitted policy serves both, track_mjx/agent/mlp_ppo/ppo_networks.py:46-96).  mean / inv_std: NULL or the operand's
 * normaliser as in tmjx_linear_nolds_norm. */
int tmjx_linear_nolds_bf16(const float *A, int64_t sa_row, int64_t sa_k, const uint16_t *W, int ldw, const float *bias, float *C, int M, int N, int K,
                           const float *mean, const float *inv_std, void *stream);

/* out[width] = column sums of the row-major src[rows][width] (the bias gradient dy.sum(0) of a dense layer: flax nn.Dense's bias in
 * track_mjx/agent/mlp_ppo/intention_network.py:32-44 and brax's value MLP); `scratch`: tmjx_colsum_scratch_floats(width) floats. */
int tmjx_colsum_scratch_floats(int width);
int tmjx_colsum(const float *src, float *out, float *scratch, int rows, int width, void *stream);

/* Up to 16 independent column sums (out[width] = sum over `rows` rows of partial[rows][width]) in one launch: the per-workgroup
 * (d gamma | d beta | d bias) partials of every LayerNorm block of a backward pass (tmjx_gemm_nn_ln_bwd), reduced once behind it.
 * `problems` is a HOST array (copied into the launch). */
typedef struct tmjx_colsum_problem_t { const float *partial; float *out; int32_t rows, width; } tmjx_colsum_problem_t;
int tmjx_colsum_grouped(const tmjx_colsum_problem_t *problems, int n, void *stream);

/* optax.chain(optax.clip_by_global_norm(max_norm), optax.adam(lr)) (track_mjx/agent/mlp_ppo/ppo.py:517-520) on FLAT fp32 device
 * buffers of n elements: param -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps) with the gradient scaled by max_norm / max(max_norm,
 * *grad_norm); `grad_norm` is a device scalar (the caller's ||grad||_2 of the averaged gradient), bias_correction{1,2} = 1 - beta^t. */
int tmjx_adam_clip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *grad_norm, long long n, float lr,
                   float beta1, float beta2, float eps, float bias_correction1, float bias_correction2, float max_norm, void *stream);
/* The same step with the global norm computed by the library itself: tmjx_adam_norm_floats() per-workgroup sums of squares (fixed
 * summation order: bit-identical on every rank for the same averaged gradient) into norm_scratch, added up inside the Adam kernel;
 * norm_out (may be NULL) receives ||grad||_2.  grad 16-byte aligned. */
int tmjx_adam_norm_floats(void);
int tmjx_adam_clip_norm(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *norm_scratch, float *norm_out, long long n, float lr,
                        float beta1, float beta2, float eps, float bias_correction1, float bias_correction2, float max_norm, void *stream);
/* tmjx_adam_clip_norm with the parameter updates of the flat range [frozen_lo, frozen_hi) zeroed: the reference's freeze_decoder optimiser
 * optax.chain(optax.chain(clip_by_global_norm, adam), freeze(mask)) (track_mjx/agent/mlp_ppo/ppo.py:594-617; the mask is True exactly for
 * policy.params.decoder, agent/network_masks.py:6-19).  The global norm covers ALL n gradients and exp_avg / exp_avg_sq are updated
 * everywhere, as there (clipping and Adam come before the freeze); only `param` inside the range is never written.  Outside the range every
 * element is bit-identical to tmjx_adam_clip_norm.  0 <= frozen_lo <= frozen_hi <= n, both multiples of 4 (flat segments start on 16-byte
 * boundaries); frozen_lo == frozen_hi freezes nothing.  No host synchronisation: capturable in a hipGraph. */
int tmjx_adam_clip_norm_frozen(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *norm_scratch, float *norm_out, long long n,
                               long long frozen_lo, long long frozen_hi, float lr, float beta1, float beta2, float eps, float bias_correction1,
                               float bias_correction2, float max_norm, void *stream);

/* Dense layers of the learner on the matrix cores, fp32 in / fp32 accumulate (flax nn.Dense of the intention network,
 * track_mjx/agent/mlp_ppo/intention_network.py:32-44,68-76, and brax's value MLP, ppo_networks.py:180-184; the gradients are those of
 * compute_ppo_loss, losses.py:103-245).  Row-major device matrices with leading dimensions (floats); any sizes; 16-byte aligned rows
 * (pointer and leading dimension multiples of 4 floats) take the vector-load path.
 *   tmjx_gemm_nt: C[M][N] = A[M][K] W[N][K]^T + bias[N] (bias may be NULL)      y = x W^T + b
 *   tmjx_gemm_nn: C[M][N] = A[M][K] W[K][N]                                     dx = dy W
 *   tmjx_gemm_dw: dW[N][K] = dY[M][N]^T X[M][K] (dW dense, leading dimension K) and, if db != NULL, db[N] = column sums of dY;
 *                 scratch >= tmjx_gemm_dw_scratch_floats(M, N, K) floats (row-range slabs, reduced by a second launch). */
int tmjx_gemm_nt(const float *A, int lda, const float *W, int ldw, const float *bias, float *C, int ldc, int M, int N, int K, void *stream);
int tmjx_gemm_nn(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K, void *stream);
/* One Dense -> SiLU -> LayerNorm block of the intention network (intention_network.py:32-40,68-74) forward in ONE launch, for layers exactly
 * one tile wide (N = 64, 128 or 256) with 16-byte aligned operand rows (tmjx_gemm_nt_silu_ln_ok says whether a call qualifies):
 *   Z = A W^T (no bias: the operand of tmjx_silu_ln_bwd), Y = LayerNorm(silu(Z + bias)) * gamma + beta, stats[row] = (mean, 1 / std).
 * Same arithmetic as tmjx_gemm_nt followed by tmjx_silu_ln_fwd. */
int tmjx_gemm_nt_silu_ln_ok(const float *A, int lda, const float *W, int ldw, int N);
int tmjx_gemm_nt_silu_ln(const float *A, int lda, const float *W, int ldw, const float *bias, const float *gamma, const float *beta, float *Z, float *Y,
                         int ldc, float *stats, int M, int N, int K, float eps, void *stream);
/* The input gradient of a layer whose INPUT is the output of a Dense -> SiLU -> LayerNorm block of width N = 256, with that block's LayerNorm +
 * SiLU backward applied in the epilogue (tmjx_gemm_nn followed by tmjx_silu_ln_bwd in one launch): dz[M][256] = d loss / d z of the block,
 * given dY[M][K] (gradient of this layer's output), W[K][256], and the block's saved z (without bias), bias, gamma, stats (mean, 1 / std).
 * partial (>= tmjx_gemm_nn_ln_bwd_partial_floats(M, 256) floats) receives one row of [d gamma | d beta | d bias] column sums per 80-row
 * workgroup: sum its rows (tmjx_colsum over (M + 79) / 80 rows of width 768). */
int tmjx_gemm_nn_ln_bwd_ok(const float *dY, int ldy, const float *W, int ldw, int N);
long long tmjx_gemm_nn_ln_bwd_partial_floats(int M, int N);
int tmjx_gemm_nn_ln_bwd(const float *dY, int ldy, const float *W, int ldw, const float *z, const float *bias, const float *gamma, const float *stats,
                        float *dz, float *partial, int M, int N, int K, void *stream);
/* Dense -> SiLU (brax value MLP, track_mjx/agent/mlp_ppo/ppo_networks.py:180-184: swish activations, no LayerNorm).  tmjx_gemm_nt_silu: Z[M][ldc] = A W^T
 * (WITHOUT the bias) and Y = silu(Z + bias) in one launch (operand rows 16-byte aligned: tmjx_gemm_nt_silu_ok); tmjx_silu_fwd: the activation alone;
 * tmjx_silu_bwd: dz = dy silu'(z + bias), dense [rows][N] arrays. */
int tmjx_gemm_nt_silu_ok(const float *A, int lda, const float *W, int ldw);
int tmjx_gemm_nt_silu(const float *A, int lda, const float *W, int ldw, const float *bias, float *Z, float *Y, int ldc, int M, int N, int K, void *stream);
int tmjx_silu_fwd(const float *z, const float *bias, float *y, long long rows, int N, void *stream);
int tmjx_silu_bwd(const float *dy, const float *z, const float *bias, float *dz, long long rows, int N, void *stream);
/* The backward pass of the value MLP without an element-wise launch between its GEMMs (brax make_value_network, ppo_networks.py:180-184: Dense -> swish ... Dense(1)):
 * tmjx_gemm_nn_silu_bwd: dZ[M][N] = (dY[M][K] W[K][N]) silu'(z + bias) — the input gradient of a hidden layer's consumer with THAT layer's SiLU backward on the
 *   accumulators (z, dZ dense [M][N]; operand rows 16-byte aligned: tmjx_gemm_nn_silu_bwd_ok);
 * tmjx_silu_bwd_rank1: dz[m][k] = (dy1[m] w1[k]) silu'(z[m][k] + bias[k]) — the same for the 1-wide head, whose input gradient is an outer product;
 * tmjx_head_dw: the head's gradients dw[k] = sum_m dy1[m] x[m][k], db[0] = sum_m dy1[m] (a matrix-vector product; scratch >= tmjx_head_dw_scratch_floats). */
int tmjx_gemm_nn_silu_bwd_ok(const float *dY, int ldy, const float *W, int ldw);
int tmjx_gemm_nn_silu_bwd(const float *dY, int ldy, const float *W, int ldw, const float *z, const float *bias, float *dZ, int M, int N, int K, void *stream);
int tmjx_silu_bwd_rank1(const float *dy1, const float *w1, const float *z, const float *bias, float *dz, long long rows, int N, void *stream);
long long tmjx_head_dw_scratch_floats(int M, int K);
int tmjx_head_dw(const float *dy1, const float *x, int ldx, float *dw, float *db, float *scratch, int M, int K, void *stream);
/* ---- whole-chain kernels (csrc/mlp_chain.h) for nets whose hidden layers are exactly 256 wide (BASELINE configs[1] / configs[2]: encoder, decoder and
 * critic = [256, 256]).  ONE launch runs a whole chain of the reference's layers — the encoder's Dense -> silu -> LayerNorm blocks + fc2_mean | fc2_logvar,
 * the decoder's blocks + the action head (track_mjx/agent/mlp_ppo/intention_network.py:32-44,68-76,128-139), or brax's value MLP
 * (ppo_networks.py:180-184) — on one workgroup's row tile: a layer's output goes to global memory exactly as the layer-by-layer entry points
 * leave it (tmjx_gemm_nt_silu_ln / tmjx_gemm_nt_silu: z without the bias, y, stats = (mean, 1 / std) per row) AND stays on the CU as the next layer's
 * operand.  Results are bit-identical to tmjx_gemm_nt_silu_ln / tmjx_gemm_nt_silu / tmjx_gemm_nt / tmjx_head_fwd called layer by layer.
 *   epi 1: hidden layers are Dense -> SiLU -> LayerNorm blocks;  epi 3: Dense -> SiLU layers (no gamma / beta / stats).
 *   Wf != NULL: an un-activated last layer outf[M][Nf] = y_last Wf^T + bf with Nf <= 128 (fc2, the action head); Nf == 1 (epi 3): the value
 *   head as a dot product (Wf = its weight row of 256 floats, outf[M]).  hidden[0].K = the input width (<= lda); hidden[l > 0].K = 256.
 * All rows 16-byte aligned (tmjx_chain_fwd_ok says whether a call qualifies); z, y dense [M][256]. */
#define TMJX_CHAIN_MAX_HIDDEN 4
typedef struct { const float *W, *bias, *gamma, *beta; float *z, *y, *stats; int32_t K, ldw; } tmjx_chain_layer_t;
typedef struct {
  const float *A; int32_t lda, M, n_hidden, epi;
  tmjx_chain_layer_t hidden[TMJX_CHAIN_MAX_HIDDEN];
  const float *Wf, *bf; float *outf; int32_t Nf, ldwf, ldof;
  float eps;
  int32_t rows_alloc;   /* rows every y buffer holds: >= tmjx_chain_rows(M) (a y that feeds the next layer of the launch is stored as whole row tiles) */
  void *prof;     /* NULL; or 16 uint64 per workgroup ((M + rows per tile - 1) / rows per tile workgroups): in-kernel clock stamps (tools/chain_stamps.py) */
} tmjx_chain_fwd_t;
int tmjx_chain_rows(int M);      /* M rounded up to the row tile (80 or 32 rows) the chain kernels take for M rows */
int tmjx_chain_fwd_ok(const tmjx_chain_fwd_t *chain);
int tmjx_chain_fwd(const tmjx_chain_fwd_t *chain, void *stream);
/* The backward pass of such a chain in ONE launch: the input-gradient GEMMs from the last layer's output gradient G[M][Kg] down to the first
 * hidden layer, each with the PRODUCING block's backward in its epilogue (what tmjx_gemm_nn_ln_bwd / tmjx_gemm_nn_silu_bwd do layer by layer),
 * d loss / d z of every hidden layer written to global memory (dz: the operand of the weight gradients, tmjx_gemm_dw_grouped) and kept on the CU as
 * the next GEMM's operand.  stage[0]: W = the LAST layer's weight [Kg][256], (z, bias, gamma, stats) = the last hidden block's saved tensors;
 * stage[s > 0]: W = the weight [256][256] of hidden layer (n - s), block = hidden layer (n - 1 - s).  epi 2: Dense -> SiLU -> LayerNorm blocks
 * (partial: >= tmjx_gemm_nn_ln_bwd_partial_floats(M, 256) floats per stage, one row of [d gamma | d beta | d bias] per workgroup: reduce with
 * tmjx_colsum_grouped);  epi 4: Dense -> SiLU layers.  Kg == 1 (epi 4): the value head — G = dy1[M], stage[0].W = the head's weight row, stage 0 has
 * no GEMM (tmjx_silu_bwd_rank1's expression).  W0 != NULL: a trailing GEMM dx[M][dx_cols] = dz_first W0[256][:dx_cols] (the decoder's first block:
 * d loss / d latent, dx_cols <= 128).  Bit-identical to the layer-by-layer entry points. */
typedef struct { const float *W; int32_t ldw; const float *z, *bias, *gamma, *stats; float *dz, *partial; } tmjx_chain_bwd_stage_t;
typedef struct {
  const float *G; int32_t ldg, Kg, M, n_stages, epi;
  tmjx_chain_bwd_stage_t stage[TMJX_CHAIN_MAX_HIDDEN];
  const float *W0; int32_t ldw0, dx_cols; float *dx; int32_t lddx;
  int32_t rows_alloc;   /* rows every dz buffer holds: >= tmjx_chain_rows(M) */
  void *prof;
} tmjx_chain_bwd_t;
int tmjx_chain_bwd_ok(const tmjx_chain_bwd_t *chain);
int tmjx_chain_bwd(const tmjx_chain_bwd_t *chain, void *stream);

/* The 1-wide head's forward pass y[m] = x[m][:K] . w + bias[0] as a matrix-vector product (bias may be NULL; K % 4 == 0, 16-byte aligned rows: tmjx_head_fwd_ok). */
int tmjx_head_fwd_ok(const float *x, int ldx, const float *w, int K);
int tmjx_head_fwd(const float *x, int ldx, const float *w, const float *bias, float *y, int M, int K, void *stream);
long long tmjx_gemm_dw_scratch_floats(int M, int N, int K);
int tmjx_gemm_dw(const float *dY, int ldy, const float *X, int ldx, float *dW, float *db, float *scratch, int M, int N, int K, void *stream);
/* All weight (+ bias) gradients of one backward pass as ONE launch + one reduction launch: up to 16 independent problems of tmjx_gemm_dw,
 * each with its own scratch (>= tmjx_gemm_dw_scratch_floats(M, N, K) floats) and a leading dimension `lddw` for dW (so the result can land
 * in a row-padded view of a flat gradient buffer); dY and X need 16-byte aligned rows.  `problems` is a HOST array (copied into the launch). */
typedef struct tmjx_dw_problem_t {
  const float *dY, *X;
  float *dW, *db, *scratch;       /* db may be NULL */
  int32_t ldy, ldx, lddw, M, N, K;
} tmjx_dw_problem_t;
int tmjx_gemm_dw_grouped(const tmjx_dw_problem_t *problems, int n, void *stream);

/* ---- bf16 GEMM-input mode (BASELINE config 5 "bf16 MLP on MFMA"; layers: track_mjx/agent/mlp_ppo/intention_network.py:14-142, sizes
 * track_mjx/config/rodent-full-clips.yaml:50-57): operands bf16, accumulation and results fp32, v_mfma_f32_16x16x32_bf16 (csrc/gemm_bf16.h).
 * Activations are either fp32 (converted when they are staged: no cast pass) or bf16 written by a producing kernel; weights come from bf16
 * SHADOWS of the fp32 master parameters. */
/* Shadows of up to 24 weight matrices src[N][K] (fp32, leading dimension ld_src) in ONE launch: dst[N][ld_dst] (ld_dst >= ceil64(K), zero
 * beyond K: the forward operand) and / or dst_t[K][ld_dst_t] (ld_dst_t >= ceil64(N), zero beyond N: the input gradient's operand).  bf16 =
 * round to nearest even of the fp32 value.  `items` is a HOST array (copied into the launch). */
typedef struct tmjx_bf16_shadow_t {
  const float *src;
  uint16_t *dst, *dst_t;           /* either may be NULL */
  int32_t N, K, ld_src, ld_dst, ld_dst_t;
} tmjx_bf16_shadow_t;
int tmjx_bf16_shadow(const tmjx_bf16_shadow_t *items, int n, void *stream);
/* C[M][N] = A[M][K] . B[N][K]^T (+ bias[N]):  A fp32 (a_is_f32 = 1; lda % 4 == 0) or bf16 (lda % 8 == 0), B a bf16 shadow whose rows hold
 * ceil64(K) elements (zero beyond K; ldb % 8 == 0); C fp32.  Forward pass: B = the weight's shadow; input gradient: A = dY, B = the
 * transposed shadow (K and N exchange roles).  All base pointers 16-byte aligned. */
int tmjx_bgemm_nt(const void *A, int a_is_f32, int lda, const uint16_t *B, int ldb, const float *bias, float *C, int ldc, int M, int N, int K,
                  void *stream);
/* The same GEMM with a block epilogue on the accumulators (the hidden activations then exist in memory only as bf16, the operand format of
 * the next GEMM, and so does z = the pre-activation WITHOUT the bias, saved for the backward pass — BASELINE config 5 is a bf16 MLP; Y and the row
 * statistics are computed from the fp32 accumulators, the backward kernels evaluate silu' / the normalised activation from the bf16 z: 2 instead
 * of 4 bytes written per element here and read, twice, there).  Row tiles are 80 rows high.  ldz in bf16 elements, a multiple of 4.
 *   tmjx_bgemm_ln_fwd   Dense -> SiLU -> LayerNorm forward (intention_network.py:32-44,68-76), N = 128, 256 or 512 (tmjx_bgemm_row_tile_ok):
 *                       Z16[M][ldz] = A B^T as bf16;  Y16 = LayerNorm(silu(A B^T + bias)) * gamma + beta as bf16;  stats[M][2] = (mean, 1 / std).
 *   tmjx_bgemm_ln_bwd   A = dY[M][K] = gradient of the CONSUMER layer's output, Bt = the consumer's transposed shadow (N = the block's width):
 *                       the tile A Bt^T is d loss / d y of the block; stores dZ16[M][lddz] = d loss / d z of the block (its LayerNorm + SiLU
 *                       backward from z, bias, gamma, stats) as bf16 and partial[(M + 79) / 80][3][N] = the row tiles' column sums
 *                       (d gamma | d beta | d bias): reduce them with tmjx_colsum_grouped (rows = (M + 79) / 80, width = 3 N).
 *   tmjx_bgemm_silu_fwd Dense -> SiLU forward (brax value MLP, ppo_networks.py:180-184), any N: Z16 = A B^T as bf16, Y16 (or Yf, fp32) = silu(A B^T + bias).
 *   tmjx_bgemm_silu_bwd its backward in the consumer's input-gradient GEMM: dZ16 = (A Bt^T) silu'(z + bias), partial[(M + 79) / 80][N] = column sums
 *                       of dZ (d bias).
 * tmjx_bgemm_partial_floats(M, N, sums): floats of `partial` for sums = 3 (ln) or 1 (silu). */
int tmjx_bgemm_row_tile_ok(int N);
/* Element size of the SAVED PRE-ACTIVATIONS these entries exchange (`Z16` / `z16` below): 2 = bf16 (the product build: BASELINE configs[4] is a
 * "bf16 MLP on MFMA"), 4 = float (a library built with -DTMJX_BF16_Z_F32: SURVEY a16's narrower "bf16 only for GEMM inputs"; the pointers then
 * point to floats, leading dimensions stay in elements). */
int tmjx_bf16_z_bytes(void);
long long tmjx_bgemm_partial_floats(int M, int N, int sums);
int tmjx_bgemm_ln_fwd(const void *A, int a_is_f32, int lda, const uint16_t *B, int ldb, const float *bias, const float *gamma, const float *beta, uint16_t *Z16, int ldz,
                      uint16_t *Y16, int ldy16, float *stats, int M, int N, int K, float eps, void *stream);
int tmjx_bgemm_ln_bwd(const void *dY, int dy_is_f32, int ldy, const uint16_t *Bt, int ldb, const uint16_t *z16, int ldz, const float *bias, const float *gamma,
                      const float *stats, uint16_t *dZ16, int lddz, float *partial, int M, int N, int K, void *stream);
int tmjx_bgemm_silu_fwd(const void *A, int a_is_f32, int lda, const uint16_t *B, int ldb, const float *bias, uint16_t *Z16, int ldz, uint16_t *Y16, int ldy16,
                        float *Yf, int ldyf, int M, int N, int K, void *stream);
int tmjx_bgemm_silu_bwd(const void *dY, int dy_is_f32, int ldy, const uint16_t *Bt, int ldb, const uint16_t *z16, int ldz, const float *bias, uint16_t *dZ16, int lddz,
                        float *partial, int M, int N, int K, void *stream);
/* The Dense -> SiLU backward alone (the block's consumer is not a bf16 GEMM): dZ16 = dY silu'(z16 + bias) as bf16 (z16: what tmjx_bgemm_silu_fwd saved), partial[(M + 79) / 80][N] = column
 * sums of dZ per 80-row tile. */
int tmjx_bf_silu_bwd(const float *dY, int ldy, const uint16_t *z16, int ldz, const float *bias, uint16_t *dZ16, int lddz, float *partial, int M, int N, void *stream);
/* The same when the block's consumer is a 1-WIDE un-activated layer (the value head, brax make_value_network: MLP(hidden..., 1)): its input gradient
 * is the outer product dy1[M] (d loss / d head output) x w1[N] (the head's weight row), formed inside the kernel — no [M][N] gradient array, no GEMM with
 * a contraction length of one.  N a multiple of 4 up to 1024, 16-byte aligned rows. */
int tmjx_bf_silu_bwd_rank1(const float *dy1, const float *w1, const uint16_t *z16, int ldz, const float *bias, uint16_t *dZ16, int lddz, float *partial, int M, int N,
                           void *stream);
/* dW[N][lddw] = dY[M][N]^T . X[M][K] and db[N] = column sums of dY (NULL: no bias gradient; sums are taken over the values AS STORED, in
 * fp32) with bf16 operands (each of dY / X fp32 or bf16 in memory, rows 16-byte aligned); scratch >= tmjx_bgemm_dw_scratch_floats(M, N, K). */
long long tmjx_bgemm_dw_scratch_floats(int M, int N, int K);
int tmjx_bgemm_dw(const void *dY, int y_is_f32, int ldy, const void *X, int x_is_f32, int ldx, float *dW, int lddw, float *db, float *scratch,
                  int M, int N, int K, void *stream);
/* All weight (+ bias) gradients of one backward pass in bf16 GEMM-input mode as ONE launch + one reduction launch: up to 24 problems of tmjx_bgemm_dw, each
 * with its own scratch (>= tmjx_bgemm_dw_scratch_floats(M, N, K) floats); the slab count of every problem is capped so that the whole launch is about
 * `target_wgs` workgroups (0: the default, 2048), in multiples of eight slabs (one per XCD).  The reference computes every layer's weight gradient inside one jax.value_and_grad
 * (track_mjx/agent/mlp_ppo/ppo.py:286-300); `problems` is a HOST array (copied into the launch). */
typedef struct tmjx_bdw_problem_t {
  const void *dY, *X;
  float *dW, *db, *scratch;       /* db may be NULL */
  int32_t y_is_f32, x_is_f32, ldy, ldx, lddw, M, N, K;
} tmjx_bdw_problem_t;
int tmjx_bgemm_dw_grouped(const tmjx_bdw_problem_t *problems, int n, int target_wgs, void *stream);

/* The stores of one env-group step into the roll-out buffers in one launch (the Transition of brax acting.actor_step, as the learner of
 * track_mjx/agent/mlp_ppo/ppo.py:330-348 collects it): obs [W][n] (env-minor) -> up to three row-major [n][W] destinations; raw [n][A],
 * logp [n], reward [n], trunc [n] copied; discount_dst = 1 - done.  Any destination may be NULL (skipped).  No LDS. */
typedef struct tmjx_rollout_store_t {
  const float *obs; float *obs_dst0, *obs_dst1;
  const float *raw; float *raw_dst;
  const float *logp; float *logp_dst;
  const float *reward; float *reward_dst;
  const float *done; float *discount_dst;
  const float *trunc; float *trunc_dst;
  int32_t n, W, A;
  float *obs_dst2;      /* a third row-major destination (the acting policy's staging copy of the new observation), may be NULL */
} tmjx_rollout_store_t;
int tmjx_rollout_store(const tmjx_rollout_store_t *s, void *stream);
/* The two ReferenceClip leaves only TMJX_DONE_ALIGN reads: velocity (C,F,3) and joints_velocity (C,F,nv-6), HOST pointers, float32, for the
 * table already uploaded on this handle (same C, F).  A later tmjx_clips_upload drops them; tmjx_clips_share shares them when the owner has them. */
int tmjx_clips_upload_velocities(tmjx_model *m, const float *velocity, const float *joints_velocity, int n_clips, int n_frames);
/* `m` reads `owner`'s resident clip table instead of holding a copy of its own (the env groups of one rank: one upload per rank).  `owner`
 * must outlive every launch of `m`. */
int tmjx_clips_share(tmjx_model *m, const tmjx_model *owner);

/* Observation normaliser update (brax running_statistics.update as called at track_mjx/agent/mlp_ppo/ppo.py:357-361; math:
 * track_mjx/agent/masked_running_statistics.py:161-214) in one pass over src [rows][W] (W % 4 == 0):
 *   tmjx_stats_sums:  sums[0..W) = sum_rows(x - mean), sums[W..2W) = sum_rows((x - mean)^2); scratch >= tmjx_stats_scratch_floats(W).
 *   (multi-GPU: all-reduce `sums` here — replaces the reference's psums of mean_update and variance_update, same totals)
 *   tmjx_stats_apply: count += n_added; mean += S1 / count; summed_variance += S2 - (S1 / count) S1; std = clip(sqrt(max(sv, 0) / count)).
 * n_added = rows summed over all ranks. */
int tmjx_stats_scratch_floats(int W);
int tmjx_stats_sums(const float *src, const float *mean, float *sums, float *scratch, long long rows, int W, void *stream);
int tmjx_stats_apply(const float *sums, float n_added, float *count, float *mean, float *summed_variance, float *std, int W, float std_min,
                     float std_max, void *stream);
/* tmjx_stats_apply for columns [0, pin_lo) only: columns [pin_lo, W) keep mean, summed_variance and std; count += n_added as usual.  The
 * reference's freeze_decoder run pins the proprioceptive columns (the decoder's input) to the checkpoint's statistics and writes them back
 * after every running_statistics.update (track_mjx/agent/mlp_ppo/ppo.py:357-377,586-593).  `sums` is the [2][W] output of tmjx_stats_sums
 * (after the optional all-reduce), unchanged.  0 <= pin_lo <= W.  No host synchronisation: capturable in a hipGraph. */
int tmjx_stats_apply_pinned(const float *sums, float n_added, float *count, float *mean, float *summed_variance, float *std, int W, int pin_lo,
                            float std_min, float std_max, void *stream);

/* Debug/test access: copy a named per-env workspace/intermediate array of the last tmjx_forward /
 * tmjx_physics call into `out` (device pointer, [count][n_env]); returns count or a negative code.
 * Names: "qM" (sparse rows), "qfrc_smooth", "qacc", "qacc_smooth", "efc_D", "efc_aref", "con_dist", ...;
 * "solver_stats" = [CG iterations (mjx data.solver_niter), line-search iterations summed, constraint rows that entered the solver,
 * of which joint limits] of the last substep; "efc_in" [nefc] = 1 for the original rows that entered the solver. */
int tmjx_debug_rows(const tmjx_model *m, const char *name, int *row0, int *count);

/* ---- LSTM decoder recurrence (csrc/lstm_kernels.h) of the recurrent learner (track_mjx/agent/lstm_ppo/intention_network.py: flax
 * nn.LSTMCell, gate order i, f, g, o):  gate = x W_i^T + h W_h^T + b_h;  c' = sig(f) c + sig(i) tanh(g);  h' = sig(o) tanh(c').
 * One launch runs T steps of ONE layer over `rows` independent sequences; the input part x W_i^T is precomputed for every step (one GEMM,
 * tmjx_gemm_nt) and passed as xg.  reset (optional, [T][ldr >= rows] floats): non-zero at (t, row) zeroes the carry (h, c) BEFORE step t —
 * the roll-out's done of the previous step, the loss scan's 1 - discount[t - 1].  Rows are independent: each workgroup owns 8 rows for all
 * T steps.  H = 32, 64, 128 or 256 (tmjx_lstm_hidden_ok). */
typedef struct {
  const float *xg; int32_t ldx;      /* [T][rows][ldx >= 4H]: x W_i^T, gate-major columns i | f | g | o */
  const float *Wh; int32_t ldw;      /* [4H][ldw >= H], 16-byte aligned rows (ldw % 4 == 0) */
  const float *bh;                   /* [4H] */
  const float *h0, *c0; int32_t ld0; /* initial carry [rows][ld0 >= H] */
  const float *reset; int32_t ldr;   /* optional */
  float *h, *c; int32_t ldo;         /* h_t, c_t of every step: [T][rows][ldo >= H] (step stride rows * ldo); may alias h0 / c0 when T == 1 */
  float *gates;                      /* optional [T][rows][4H]: sig(i) | sig(f) | tanh(g) | sig(o) (what tmjx_lstm_seq_bwd needs) */
  float *h_prev;                     /* optional [T][rows][ldo]: the carry h each step read, resets applied (the operand of dW_h) */
  int32_t T, rows, H;
} tmjx_lstm_fwd_t;
/* The reverse recurrence: dh [T][rows][ldd] = d loss / d h_t from above -> dgates [T][rows][4H] = d loss / d (pre-activation gates) (the
 * operand of dx = dgates W_i, dW_i, dW_h = dgates^T h_prev and db = colsum(dgates)) and, optionally, d loss / d (h0, c0) [rows][ld0].
 * gates / c / c0 / reset are the forward call's; a reset stops the gradient exactly where the forward pass stopped the carry. */
typedef struct {
  const float *dh; int32_t ldd;
  const float *Wh; int32_t ldw;
  const float *gates;
  const float *c; int32_t ldo;
  const float *c0; int32_t ld0;
  const float *reset; int32_t ldr;
  float *dgates;
  float *dh0, *dc0;                  /* optional */
  int32_t T, rows, H;
} tmjx_lstm_bwd_t;
int tmjx_lstm_hidden_ok(int H);
int tmjx_lstm_seq_fwd(const tmjx_lstm_fwd_t *args, void *stream);
int tmjx_lstm_seq_bwd(const tmjx_lstm_bwd_t *args, void *stream);

/* ---- Roll-out recorder (csrc/rollout_kernels.h) of checkpoint roll-outs (track_mjx/analysis/rollout.py:73-269: generate_rollout's scan
 * stacks the state, ctrl and activations of every step).  ONE launch per control step copies K streams into clip-major records
 * dst[env][T][w] at row t0 + t: each env's record of a stream is one contiguous block.  The copy never rounds: recorded values are the
 * source's bits.  A stream's source is either
 *   SoA       src[r * ld + env], r < src_extent (the env's [field][n_env] state / metrics buffers): transposed through LDS so that each env's
 *             w floats are written as one coalesced run;
 *   row-major src[env * ld + c], c < src_extent (the policy's layer outputs): 16-byte loads / stores when src, ld, w and dst allow.
 * n_idx > 0 selects rows (SoA) / columns (row-major) idx[0..w) of the source instead of 0..w (e.g. metrics in METRIC_NAMES order). */
#define TMJX_RECORD_SOA 0
#define TMJX_RECORD_ROWMAJOR 1
#define TMJX_RECORD_MAX_STREAMS 64
#define TMJX_RECORD_MAX_IDX 32
#define TMJX_RECORD_MAX_W 4096
typedef struct tmjx_record_stream_t {
  const float *src;
  float *dst;                  /* [n_env][T][w], 16-byte aligned for the vector path */
  int32_t layout;              /* TMJX_RECORD_SOA | TMJX_RECORD_ROWMAJOR */
  int32_t ld;                  /* SoA: >= n_env; row-major: >= src_extent */
  int32_t w;                   /* floats per env per row, 1 .. TMJX_RECORD_MAX_W */
  int32_t src_extent;          /* rows (SoA) / columns (row-major) of the source: the bound of every index read */
  int32_t T, t0;               /* rows per env record; the launch's t writes row t0 + t */
  int32_t n_idx;               /* 0, or w (<= TMJX_RECORD_MAX_IDX): idx[0..w) are source rows / columns */
  int32_t idx[TMJX_RECORD_MAX_IDX];
  int32_t pad_;
} tmjx_record_stream_t;
/* Host-side validation of a stream table for launches with 0 <= t < T (no device call): null or misaligned (4-byte) pointers, w / ld /
 * index bounds, t0 + T beyond a stream's record.  Run once before the table is copied to the device. */
int tmjx_record_check(const tmjx_record_stream_t *table, int k, int n_env, int T);
/* One launch: row t of every stream of `device_table` (a device copy of a table that passed tmjx_record_check with the same k, n_env, T;
 * 16-byte aligned).  Grid (ceil(n_env / 32), k) of 256 threads, 32 envs per workgroup. */
int tmjx_record_step(const tmjx_record_stream_t *device_table, int k, int n_env, int t, int T, void *stream);

/* Deterministic policy step (make_inference_fn(..., deterministic=True), intention_network.py:102-123):
 * tmjx_latent_concat_det: x[i] = [ fc2[i][0..Z) | (obs_i[c] - mean[c]) / std[c] for c in [ref_w, obs_w) ], written as [n][ldx] (columns
 *   beyond Z + obs_w - ref_w are zeroed) — z = latent_mean exactly (no mean + 0 * exp(logvar / 2), which is NaN where exp overflows);
 *   with `traj` also traj[i][c] = (obs_i[c] - mean[c]) / std[c] for c < ref_w ([n][ldt]: the normalised reference half the reference logs).
 *   obs_i[c] at obs[i * obs_s0 + c * obs_s1]; fc2 [n][ldf >= 2Z]; mean / std may both be NULL (no normaliser).
 * tmjx_action_mode: NormalTanh mode, a = tanh(logits[i][j]) for j < A (logits [n][ldl >= 2A]) written as ctrl [n][A] (recorded) and
 *   action_t [A][n] (the layout tmjx_step takes). */
int tmjx_latent_concat_det(const float *fc2, int ldf, const float *obs, int64_t obs_s0, int64_t obs_s1, const float *mean, const float *std,
                           float *x, int ldx, float *traj, int ldt, int n, int Z, int obs_w, int ref_w, void *stream);
int tmjx_action_mode(const float *logits, int ldl, float *ctrl, float *action_t, int n, int A, void *stream);

/* ---- Decoder policy of a high-level env (make_decoder_policy, intention_network.py:194-222; HighLevelWrapper, environment/wrappers.py:384-412):
 * the env is stepped with an intention vector per env, the pretrained decoder turns it into controls.
 * tmjx_decoder_input: tmjx_latent_concat_det's launch (the same kernel, the same bits) for latents that are NOT the front of an fc2 buffer:
 *   x[i] = [ latents[i][0..Z) | (obs_i[c] - mean[c]) / std[c] for c in [ref_w, obs_w) | 0 .. ], latents [n][ldz >= Z], x [n][ldx]. */
int tmjx_decoder_input(const float *latents, int ldz, const float *obs, int64_t obs_s0, int64_t obs_s1, const float *mean, const float *std,
                       float *x, int ldx, int n, int Z, int obs_w, int ref_w, void *stream);
/* tmjx_decoder_act (csrc/decoder_act.h): the whole decoder policy as ONE launch —
 *   [latents | normalised proprioception] -> n_blocks Dense -> SiLU -> LayerNorm blocks, 256 wide -> action head (2A <= 128 columns) -> tanh.
 * latents [n][ldz >= Z]; obs_i[c] at obs[i * obs_s0 + c * obs_s1]: the env's raw [obs][n_env] buffer as tmjx_step leaves it goes in as
 * (obs_s0, obs_s1) = (1, n_env), no staging copy; mean / std of the whole observation [obs_w], or both NULL (no normaliser); Z + obs_w - ref_w <= 320.
 * block[0].W [256][ldw >= Z + obs_w - ref_w rounded up to 4], block[l > 0].W [256][ldw >= 256], Wf [2A][ldwf >= 256]: rows 16-byte aligned;
 * bias / gamma / beta 16-byte aligned [256]; bf [2A] or NULL.
 * Outputs: action_t [A][n] (the layout tmjx_step takes); optionally ctrl [n][A] and logits [n][ldl >= 2A] (NULL: not written).  Nothing else
 * reaches global memory.  logits are bit-identical to tmjx_latent_concat_det -> tmjx_chain_fwd (epi 1) on the same inputs, action_t / ctrl to
 * tmjx_action_mode of those logits.  Any n >= 1.  tmjx_decoder_act_ok says whether a descriptor qualifies (no error recorded, no device call). */
typedef struct { const float *W, *bias, *gamma, *beta; int32_t width, ldw; } tmjx_decoder_block_t;
typedef struct {
  const float *latents; int32_t ldz;
  const float *obs; int64_t obs_s0, obs_s1;
  const float *mean, *std;
  int32_t n, Z, obs_w, ref_w, n_blocks;
  tmjx_decoder_block_t block[TMJX_CHAIN_MAX_HIDDEN];
  const float *Wf, *bf; int32_t ldwf, A;
  float eps;
  float *action_t, *ctrl, *logits; int32_t ldl;
} tmjx_decoder_act_t;
int tmjx_decoder_act_ok(const tmjx_decoder_act_t *a);
int tmjx_decoder_act(const tmjx_decoder_act_t *a, void *stream);

/* tmjx_lstm_decoder_act (csrc/lstm_decoder_act.h): the LSTM decoder policy as ONE launch —
 *   x_0 = [latents | normalised proprioception] (tmjx_decoder_input's expression);  per layer k < L: (h_k, c_k) zeroed where reset != 0,
 *   gates = x_k W_i,k^T + h_k W_h,k^T + b_h,k (i | f | g | o), c_k' = sig(f) c_k + sig(i) tanh(g), h_k' = sig(o) tanh(c_k'), x_{k+1} = h_k';
 *   logits = x_L W_p^T + b_p;  action = tanh(logits[0..A)).
 * latents, obs, obs_s0 / obs_s1, mean / std, Z, obs_w, ref_w: as tmjx_decoder_act.  reset [n] or NULL: non-zero zeroes that row's carry of EVERY
 * layer before the step (tmjx_lstm_fwd_t.reset at T = 1).  layer[k].Wi [4H][ldwi >= the layer's input width rounded up to 4], layer[k].Wh
 * [4H][ldwh >= H], Wp [2A][ldwp >= H]: rows 16-byte aligned (ld % 4 == 0); bh [4H], bp [2A] or NULL.
 * The carry h, c [n][ld >= L H] (layer k in columns [k H, (k + 1) H): the [n, L, H] layout) is read and overwritten in place.
 * Outputs: action_t [A][n]; optionally ctrl [n][A] and logits [n][ldl >= 2A] (NULL: not written).  Nothing else reaches global memory; pad columns
 * of h / c / logits and rows >= n are never touched.
 * Qualifying shapes: H == 128, 1 <= L <= 4, Z + obs_w - ref_w <= 320, 2A <= 128, any n >= 1.  tmjx_lstm_decoder_act_ok says whether a descriptor
 * qualifies (no error recorded, no device call); the entry point returns TMJX_EINVAL with the reason before any device call. */
#define TMJX_LSTM_DECODER_MAX_LAYERS 4
typedef struct { const float *Wi, *Wh, *bh; int32_t ldwi, ldwh; } tmjx_lstm_decoder_layer_t;
typedef struct {
  const float *latents; int32_t ldz;
  const float *obs; int64_t obs_s0, obs_s1;
  const float *mean, *std;
  const float *reset;
  int32_t n, Z, obs_w, ref_w, L, H;
  tmjx_lstm_decoder_layer_t layer[TMJX_LSTM_DECODER_MAX_LAYERS];
  const float *Wp, *bp; int32_t ldwp, A;
  float *h, *c; int32_t ld;
  float *action_t, *ctrl, *logits; int32_t ldl;
} tmjx_lstm_decoder_act_t;
int tmjx_lstm_decoder_act_ok(const tmjx_lstm_decoder_act_t *a);
int tmjx_lstm_decoder_act(const tmjx_lstm_decoder_act_t *a, void *stream);

/* ---- The acting policy as ONE small-footprint launch (csrc/policy_act.h, csrc/tmjx_act.hip; make_inference_fn, ppo_networks.py:46-96; the intention
 * network's encoder, reparameterize and decoder, intention_network.py:32-44,68-88):
 *   h = encoder blocks((obs[:, :ref_w] - mean) * inv_std);  fc2 = h W2^T + b2 = [latent mean | latent logvar];
 *   x = [ mean + eps exp(logvar / 2) | (obs[:, ref_w:] - nmean) / nstd | 0 .. ];  logits = decoder blocks(x) Wh^T + bh;
 *   raw = loc + scale noise, action = tanh(raw), logp = log-prob of the sample — every block Dense -> SiLU -> LayerNorm, 256 wide.
 * It replaces, with the same bits in every output, the launches tmjx_linear_act / tmjx_silu_ln_fwd (per block), tmjx_linear_act (fc2),
 * tmjx_latent_concat, the decoder's blocks, tmjx_linear_act (head) and tmjx_sample_action.  One workgroup of 256 threads owns 16 rows through the whole
 * policy: <= 96 registers and 18 944 bytes of LDS, so that it runs next to a full house of physics waves; no activation leaves the CU.
 * obs: the raw observation, row-major [n][ldo] with 16-byte aligned rows.  K0 = ref_w rounded up to a multiple of 4: the row length of enc[0].W, whose
 * columns [ref_w, K0) are zero, and of mean / inv_std (both or neither; pad 0 / 0).  nmean / nstd [obs_w] (both or neither): the normaliser of the
 * proprioceptive columns, applied as a division.  enc[0].W [256][ldw >= K0], dec[0].W [256][ldw >= Z + obs_w - ref_w rounded up to 4] (pad columns
 * zero), every other block [256][ldw >= 256], W2 [2Z][ldw2 >= 256], Wh [2A][ldwh >= 256]: rows 16-byte aligned; bias / gamma / beta 16-byte aligned.
 * eps [n][Z] and noise [n][A]: the caller's N(0, 1) draws, or both NULL: Philox streams 2 and 3 of (seed, rng_state[0]), and the launch advances
 * rng_state[0] by one (rng_state [2] int64: draw counter, ticket) as tmjx_sample_action does.
 * Outputs: fc2 [n][2Z], logits [n][2A], raw [n][A], action_t [A][n] (the layout tmjx_step takes), logp [n].
 * Qualifying shapes: every block width == 256, 1 .. TMJX_CHAIN_MAX_HIDDEN blocks per stack, Z + obs_w - ref_w <= 288, 2Z <= 256, 2A <= 256, any n >= 1.
 * tmjx_policy_act_ok says whether a descriptor qualifies (no error recorded, no device call); the entry point returns TMJX_EINVAL with the reason
 * before any device call. */
typedef struct {
  const float *obs; int64_t ldo;
  const float *mean, *inv_std, *nmean, *nstd;
  int32_t n, K0, Z, obs_w, ref_w, A, n_enc, n_dec;
  tmjx_decoder_block_t enc[TMJX_CHAIN_MAX_HIDDEN], dec[TMJX_CHAIN_MAX_HIDDEN];
  const float *W2, *b2; int32_t ldw2, ldwh; const float *Wh, *bh;
  const float *eps, *noise; uint64_t seed; int64_t *rng_state;
  float ln_eps; int32_t pad_;
  float *fc2, *logits, *raw, *action_t, *logp;
} tmjx_policy_act_t;
int tmjx_policy_act_ok(const tmjx_policy_act_t *a);
int tmjx_policy_act(const tmjx_policy_act_t *a, void *stream);

/* ---- Rendering roll-outs (csrc/tmjx_render.hip, csrc/render_core.h; DESIGN.md "Rendering"): a ray-caster for the model's analytic primitives
 * (plane, sphere, capsule, ellipsoid, box: the visible geoms of the blob's rgeom_* entries, tools/compile_model.py render_entries), the walker at
 * `qpos` and optionally a translucent ghost at `qpos_ghost`, seen from one camera.  A handle whose blob carries no rgeom_* entries has no render
 * tables: every entry point that takes the handle returns TMJX_EINVAL.  All device memory is the caller's, everything runs on the caller's stream,
 * nothing synchronises.
 *   Stage A (tmjx_render_pose): qpos [F][nq] row-major (and qpos_ghost [F_ghost][nq] or NULL; F_ghost must equal F) -> the workspace:
 *     [F][cam_floats] camera records | [F][nprim][rec_floats] world-space primitive tables (at prims_offset) | the stage's scratch.
 *     primitive record (20 floats): centre [3], rotation world-from-local row-major [9], size [3], rgb [3], type | id << 8 (int32 bits), ghost flag
 *     (int32 bits; non-zero: drawn translucent grey);  camera record (16 floats): origin [3], X [3], Y [3], Z [3], tan(fovy / 2), 3 unused.
 *   Stage B (tmjx_render_prims): tables prims [F][P][20] (16-byte aligned, 1 <= P <= 256) and cameras cams [F][16] -> rgba uint8 [F][H][W][4]
 *     (alpha 255), optionally depth float [F][H][W] (distance along the ray of the nearest surface, inf on a miss) and geom_id int32 [F][H][W]
 *     (the nearest surface's id: the visible-geom index, + ngeom where the ghost is nearest; -1 on a miss); NULL: not written.
 *   tmjx_render: A then B (the same launches, the same bits).
 * Camera: looks along -Z of its frame, +X right, +Y up, fovy the vertical field of view in degrees.  TMJX_CAMERA_TRACKCOM: origin =
 * subtree_com(body) + offset, `quat` the orientation in WORLD axes (it does not turn with the body); TMJX_CAMERA_FIXED: offset and quat in the
 * body's frame.  TMJX_CAMERA_TRACK is refused by name.  tmjx_render_camera fills the struct for one of the blob's named cameras (a trackcom
 * camera with the offset and world orientation it has at qpos0); callers may also fill one themselves.
 * Errors are returned before any launch: no render tables, unknown camera name, W or H < 1, F < 1, F_ghost != F, a body out of range. */
#define TMJX_CAMERA_FIXED 0
#define TMJX_CAMERA_TRACK 1
#define TMJX_CAMERA_TRACKCOM 2
typedef struct { int32_t body, mode; float offset[3], quat[4], fovy; } tmjx_camera_t;
typedef struct {
  int32_t ngeom, ncam;             /* visible geoms, named cameras */
  int32_t rec_floats, cam_floats;  /* floats per primitive / camera record */
  int32_t nprim;                   /* primitives per frame for the (F, ghost) asked about */
  int64_t prims_offset;            /* workspace float index of the primitive tables (the cameras are at 0) */
  int64_t workspace_floats;
} tmjx_render_info_t;
int tmjx_render_info(const tmjx_model *m, int F, int ghost, tmjx_render_info_t *out);
int tmjx_render_camera(const tmjx_model *m, const char *name, tmjx_camera_t *out);
int tmjx_render_pose(const tmjx_model *m, const float *qpos, const float *qpos_ghost, int F, int F_ghost, const tmjx_camera_t *cam, float *workspace,
                     void *stream);
int tmjx_render_prims(const float *prims, const float *cams, int F, int P, int W, int H, uint8_t *rgba, float *depth, int32_t *geom_id, void *stream);
int tmjx_render(const tmjx_model *m, const float *qpos, const float *qpos_ghost, int F, int F_ghost, const tmjx_camera_t *cam, int W, int H,
                float *workspace, uint8_t *rgba, float *depth, int32_t *geom_id, void *stream);

/* ---- PCA of recorded activations and the progression panel (csrc/tmjx_pca.hip, csrc/pca_core.h; DESIGN.md "PCA").  No model handle; all device
 * memory is the caller's; everything runs on the caller's stream.
 *   tmjx_pca_workspace: *floats = the float count of the workspace tmjx_pca_fit needs for an [n][d] input.
 *   tmjx_pca_fit: x [n][ldx] float32 (the first d columns are used, ldx >= d: a column slice of a wider buffer is fine) -> mean [d],
 *     components [d][d] (row j: the unit-norm principal axis of the j-th largest variance, its largest-magnitude coefficient positive, the lowest
 *     index winning a tie) and variance [d] (eigenvalues of the covariance with divisor n - 1, clamped at 0, descending).  Two passes over x (column
 *     means in float64; the centred Gram matrix in float32 per PCA_ROWS_PER_WG = 256 rows, the partials added in a fixed order in float64: no
 *     atomics, the same bits on every run), then one workgroup of parallel-ordered cyclic Jacobi on the float32 covariance.  The call WAITS for the
 *     stream (it reads the solver's report back) and fills *info; a solver that reaches its sweep limit without off(A) <= 2^-24 ||A||_F (a NaN in x
 *     does that) returns TMJX_ENOCONV, with mean / components / variance written but not to be used.  Zero total variance: variance 0, components
 *     the identity.  Refused before any launch (TMJX_EINVAL): d < 1, d > 128 (by name, with the limit), n < 2, ldx < d, a null pointer, a workspace
 *     that is not 16-byte aligned.
 *   tmjx_pca_transform: out [n][ldo], columns [0, k) = (x - mean) . components[c] for the first k rows of components [k..][d] (row stride d);
 *     nothing synchronises.  Refused: d < 1, d > 128, n < 1, ldx < d, k < 1, k > d, ldo < k, a null pointer.
 *   tmjx_plot_strips: the progression panel, rgba uint8 [F][H][W][4] (alpha 255, the renderer's layout), one thread per pixel.  proj [T][ldp] (device),
 *     k <= 8 curves; frame f shows the timesteps [0, i), i = frame_idx[f] clamped to [0, T] (frame_idx [F] int32, device); flags [F] uint8 (device, or
 *     NULL for none): bit 0 draws the "terminated" line at x = i.  The geometry (plot rectangle, scrolling x range, lines as distance to segments,
 *     markers, draw order) is fixed in DESIGN.md "PCA".  No text.  Refused: T < 1, k outside 1 .. 8, ldp < k, F < 1, W or H < 1, window < 1, a y range
 *     that is not finite and increasing, margins that leave less than 3 x 3 pixels, a line half-width outside (0, 1e4], a null pointer. */
#define TMJX_ENOCONV (-34)
typedef struct {
  int32_t sweeps;              /* Jacobi sweeps run */
  int32_t converged;           /* 0: the sweep limit was reached first (the call returns TMJX_ENOCONV) */
  float off_rel;               /* final off(A) / ||A||_F */
  float moments_ms, jacobi_ms; /* device time of the two moment passes with their reductions, and of the eigen-solver */
} tmjx_pca_info_t;
typedef struct {
  int32_t margin_left, margin_right, margin_top, margin_bottom;   /* pixels between the panel's edge and the plot rectangle */
  float line_half_width, marker_radius;                           /* pixels */
  uint8_t colour[8][4];                                           /* r g b (a ignored) of curve c */
  uint8_t background[4], axes[4], terminated[4];
} tmjx_strip_style_t;
int tmjx_pca_workspace(int n, int d, int64_t *floats);
int tmjx_pca_fit(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info,
                 void *stream);
int tmjx_pca_transform(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo, void *stream);
int tmjx_plot_strips(const float *proj, int T, int k, int64_t ldp, const int32_t *frame_idx, const uint8_t *flags, int F, float ymin, float ymax, int window,
                     const tmjx_strip_style_t *style, int W, int H, uint8_t *rgba, void *stream);

/* ---- Wide PCA, 129 <= d <= 1024 (csrc/tmjx_pca_wide.hip, csrc/pca_wide_core.h; DESIGN.md "PCA", wide fit): the argument lists, outputs and
 * conventions of tmjx_pca_workspace / tmjx_pca_fit / tmjx_pca_transform.  For d <= 128 the three forward to those and give their bits.
 *   tmjx_pca_wide_workspace: the float count tmjx_pca_fit_wide needs.  The row split of the moments is fixed by n alone (at most 16 super-chunks of
 *     256-row chunks), so the size grows with d^2 only: 137 MiB at d = 1024, whatever n is.
 *   tmjx_pca_fit_wide: float64 column sums; the centred Gram matrix in 128 x 128 tiles (float32 FMAs within a chunk, float64 across chunks and
 *     super-chunks, a fixed order, no atomics: the same bits on every run); then block Jacobi on the covariance in global memory — blocks of 64
 *     columns (the last may be smaller; nothing is padded), paired by the round-robin tournament; a pair's sub-matrix (at most 128 x 128) is
 *     diagonalised by the narrow fit's one-workgroup solver and its eigenvector rows rotate the pair's rows of A and V^T, then its columns of A.
 *     After every block sweep the call WAITS for the stream and reads off(A)^2 and ||A||_F^2 back (float64); it stops at off(A) <= 2^-24 ||A||_F
 *     (info->sweeps: the block sweeps; jacobi_ms: the whole iteration) or returns TMJX_ENOCONV after 30 block sweeps.  A covariance that is not
 *     finite (a NaN in x) is refused after the moment pass, before any rotation is launched: TMJX_EINVAL, "non-finite".  Refused before any launch
 *     (TMJX_EINVAL): d < 1, d > 1024 ("exceeds the wide PCA limit of 1024"), n < 2, ldx < d, a null pointer, a workspace not 16-byte aligned.
 *   tmjx_pca_transform_wide: as tmjx_pca_transform, 1 <= k <= d <= 1024; one fmaf chain per output in ascending feature order. */
#define PCA_WIDE_MAX_D 1024
int tmjx_pca_wide_workspace(int n, int d, int64_t *floats);
int tmjx_pca_fit_wide(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info,
                      void *stream);
int tmjx_pca_transform_wide(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo,
                            void *stream);

/* ---- Linear readout: ridge regression from recorded activations x [n][d] (d <= 1024) to targets y [n][m] (m <= 512), for up to 16 penalties at once
 * (csrc/tmjx_readout.hip, csrc/readout_core.h; DESIGN.md "Readout").  No model handle; all device memory is the caller's; everything runs on the
 * caller's stream.  x and y are float32 and may be column slices of wider buffers (ldx >= d, ldy >= m).
 *   tmjx_readout_workspace: *floats = the float count that covers a fit, the weights and a score of up to n rows: every call of 2 <= n' <= n rows with
 *     the same d, m and at most n_lambda penalties stays inside it (the layouts of fewer rows are not all smaller; the size allows for that).
 *   tmjx_readout_fit: mean_x [d], components [d][d] and variance [d] are tmjx_pca_fit_wide's for the same x, to the bit (it is called as it is, the
 *     narrow fit for d <= 128; *info is its report, and TMJX_ENOCONV or its "non-finite" refusal pass through unchanged); mean_y [m] from float64 column
 *     sums; C = (x - mean_x)^T (y - mean_y) / (n - 1) by the row split of the wide PCA's moments (float32 FMAs within a chunk of 256 rows, float64
 *     across chunks and super-chunks, a fixed order, no atomics); z [d][m] = components . C.  The call WAITS for the stream.
 *   tmjx_readout_weights: w [L][d][m], w[i] = components^T diag(1 / (variance_j + lambdas[i])) z; lambdas [L] is HOST memory, absolute penalties.
 *     Nothing synchronises.
 *   tmjx_readout_predict: out [n][ldo], columns [0, m) = (x - mean_x) w + mean_y for ONE w [d][m]; one fmaf chain per output in ascending feature order.
 *   tmjx_readout_score: for every penalty i and target c, sse [L][m] = sum_r (y[r][c] - yhat_i[r][c])^2 over the n rows given (yhat: what
 *     tmjx_readout_predict stores; it is never written to memory) and sst [m] = sum_r (y[r][c] - mean(y[:, c]))^2 with the float64 column mean of
 *     these rows; float64, device memory, reduced in a fixed order.  R^2 = 1 - sse / sst is the caller's.  w: [L][d][m].  Nothing synchronises.
 *   Refused before any launch (TMJX_EINVAL, the message names the value): d < 1, d > 1024, m < 1, m > 512, n_lambda outside 1 .. 16, n < 2 (fit, score,
 *   workspace) or n < 1 (predict), ldx < d, ldy < m, ldo < m, a lambda that is not finite or not > 0 once rounded to float32 (as
 *   the kernels take it: 1e-50 rounds to 0 and is refused), a null pointer, a workspace not 16-byte aligned. */
#define READOUT_MAX_M 512
#define READOUT_MAX_L 16
int tmjx_readout_workspace(int n, int d, int m, int n_lambda, int64_t *floats);
int tmjx_readout_fit(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, float *mean_x, float *components, float *variance,
                     float *mean_y, float *z, float *workspace, tmjx_pca_info_t *info, void *stream);
int tmjx_readout_weights(const float *components, const float *variance, const float *z, int d, int m, const double *lambdas, int n_lambda, float *w,
                         void *stream);
int tmjx_readout_predict(const float *x, int n, int d, int64_t ldx, const float *mean_x, const float *w, const float *mean_y, int m, float *out, int64_t ldo,
                         void *stream);
int tmjx_readout_score(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, const float *mean_x, const float *w, const float *mean_y,
                       int n_lambda, double *sse, double *sst, float *workspace, void *stream);

/* ---- k-means of recorded activations x [n][d] (1 <= d <= 1024) into 1 <= k <= 256 clusters, k <= n: Lloyd's iteration with k-means++ seeding
 * (csrc/tmjx_kmeans.hip, csrc/kmeans_core.h; DESIGN.md "Clustering").  No model handle; all device memory is the caller's; everything runs on the
 * caller's stream.  x is float32 and may be a column slice of a wider buffer (ldx >= d).  Fixed-order arithmetic, no floating-point atomics: the same
 * bits on every run.
 *   tmjx_kmeans_workspace: *floats = the size of the scratch every call below takes for these n, d, k (it does not scale with n k d).
 *   tmjx_kmeans_assign: labels [n] = the nearest centroid of every row, the lowest index on a tie; the [n][k] distances are never written.  Scores
 *     are cnorm_j - 2 (x - mean) . (c_j - mean) with the float64 column mean of x rounded to float32, one fmaf chain per pair in ascending feature
 *     order; dist2 [n] (optional) = max(0, ||x - mean||^2 + score) of the chosen one; *inertia (device float64) = the sum of the float32 dist2 in a
 *     fixed order; *changed (device int32, optional) = the rows whose label differs from labels_prev [n] (all n when labels_prev is null;
 *     labels_prev may not be the labels buffer itself).
 *   tmjx_kmeans_update: every non-empty cluster's centroid = the mean of its rows, accumulated in float64 from the first add in a fixed order and
 *     rounded once; an empty cluster keeps its bits; counts [k] (device int32) = the rows of each.  A label outside [0, k) is skipped.
 *   tmjx_kmeans_seed: k-means++.  u [k] (HOST, uniforms in [0, 1)); centre 0 is row min(floor(u_0 n), n - 1); before centre j >= 1 every row's
 *     d2 = min(d2, ||x - c_(j-1)||^2) in float32, then the smallest row i with cum[i] > u_j total is taken, cum the float64 prefix sum of d2 in row
 *     order (total == 0: row min(floor(u_j n), n - 1)).  One pass over x per centre; index [k] (HOST, out) are the rows chosen.  WAITS for the stream.
 *   tmjx_kmeans_fit: from the centroids given, iterations of assign then update until no label changed, or the inertia fell by no more than
 *     tol x the previous inertia, or max_iter; then one assign against the final centroids, whose labels, dist2 (optional) and inertia are returned.
 *     It reads one int32 and one float64 back per iteration and WAITS for the stream.  info->n_iter counts the assigns of the loop.
 *   Refused before any launch (TMJX_EINVAL, the message names the value): n < 1, d outside 1 .. 1024, k outside 1 .. 256, k > n, ldx < d, a null
 *   required pointer, a workspace not 16-byte aligned, a u outside [0, 1), max_iter < 1, tol < 0 or NaN. */
#define KMEANS_MAX_D 1024
#define KMEANS_MAX_K 256
typedef struct { int32_t n_iter, changed; double inertia; float assign_ms, update_ms; } tmjx_kmeans_info_t;
int tmjx_kmeans_workspace(int n, int d, int k, int64_t *floats);
int tmjx_kmeans_assign(const float *x, int n, int d, int64_t ldx, const float *centroids, int k, const int32_t *labels_prev, int32_t *labels, float *dist2,
                       double *inertia, int32_t *changed, float *workspace, void *stream);
int tmjx_kmeans_update(const float *x, int n, int d, int64_t ldx, const int32_t *labels, int k, float *centroids, int32_t *counts, float *workspace,
                       void *stream);
int tmjx_kmeans_seed(const float *x, int n, int d, int64_t ldx, int k, const double *u, float *centroids, int32_t *index, float *workspace, void *stream);
int tmjx_kmeans_fit(const float *x, int n, int d, int64_t ldx, int k, float *centroids, int32_t *labels, float *dist2, int max_iter, double tol,
                    tmjx_kmeans_info_t *info, float *workspace, void *stream);

/* ---- A hidden Markov model over recorded activations x [n][d] (1 <= d <= 1024): 1 <= k <= 128 states with diagonal-covariance Gaussian emissions
 * (csrc/tmjx_hmm.hip, csrc/hmm_core.h; DESIGN.md "Sequence model").  The conventions of tmjx_kmeans_*: no model handle; all device memory is the
 * caller's; everything runs on the caller's stream; x is float32 and may be a column slice of a wider buffer (ldx >= d); fixed-order arithmetic, no
 * floating-point atomics: the same bits on every run.  The model: means [k][d], vars [k][d], transmat [k][k] (rows sum to 1), startprob [k], float32
 * on the device.  The rows form S sequences given by seq_start [S + 1] (HOST int32: seq_start[0] = 0, strictly increasing, seq_start[S] = n); no
 * transition crosses a sequence boundary.  The offsets are checked on the host and copied to the workspace on the stream: the array must stay
 * valid until the work the call queued has run (tmjx_hmm_fit waits itself).
 *   tmjx_hmm_workspace: *floats = the size of the scratch every call below takes for these n, d, k.  UNLIKE the k-means' it scales with n k: it holds
 *     logb, the scaled forward variables, the backward weights and gamma, [n][k] float32 each, and the [n][k] uint8 back-pointers (S sizes nothing).
 *   tmjx_hmm_emission: logb [n][k] = c_j - 1/2 sum_c (x_tc - mu_jc)^2 / var_jc.  The quadratic form is written directly, v = x - mu,
 *     q = fma(v, v (1 / var), q), one chain per (row, state) in ascending feature order: every term is non-negative, nothing cancels.
 *     c_j = -1/2 sum_c log(2 pi var_jc) in float64, rounded once.
 *   tmjx_hmm_forward_backward: the scaled recursion from logb, one workgroup per sequence.  With m_t = max_j logb_t(j) and
 *     bt_t(j) = exp(logb_t(j) - m_t) the forward variables are normalised every step by c_t and the backward ones scaled by the same c_t.
 *     gamma [n][k] float32 (every row normalised to sum 1); xi [k][k] float64 = A o (ahat^T W), W_t(j) = bt_(t+1)(j) bhat_(t+1)(j) / c_(t+1) inside a
 *     sequence: the expected transition counts, the products summed in float64 in row order over fixed row parts, the parts in part order, A
 *     multiplied in once; start [k] float64 = the sum of gamma at each sequence's first row, in sequence order; loglik [S] float64 =
 *     sum_t (log c_t + m_t), and *total their sum in sequence order.  All on the device.  A sequence the model gives probability zero (some
 *     c_t == 0) reports loglik = -inf and gamma rows of zeros (all of its rows) and adds nothing to xi and start: a defined result, not an error.
 *   tmjx_hmm_mstep: weight [k] (device float64) = sum_t gamma_tk; with m the float32 column mean of x (as tmjx_kmeans_assign forms it)
 *     S1 = sum gamma (x - m), S2 = sum gamma (x - m)^2 in float64 in row order over fixed row parts, the parts in part order; mu = m + S1 / w,
 *     var = max(S2 / w - (S1 / w)^2, min_var), rounded once.  A state with w < min_weight (or w == 0) keeps the bits of its mu and var.
 *   tmjx_hmm_transitions: transmat_ij = (xi_ij + prior + kappa [i == j]) / sum_j (...), startprob_j = (start_j + prior) / sum_j (...), float64,
 *     rounded once; prior, kappa >= 0 are Dirichlet pseudo-counts (kappa on the diagonal: a "sticky" model); a row whose denominator is 0 keeps its bits.
 *   tmjx_hmm_viterbi: delta_0(j) = log pi_j + logb_0(j), delta_t(j) = logb_t(j) + max_i (delta_(t-1)(i) + log A_ij) in float32, the lowest i on a tie,
 *     log 0 = -inf; labels [n] int32 = the best path of every sequence, path_logprob [S] (device float64) its score.  logspace != 0: transmat and
 *     startprob already hold logarithms.
 *   tmjx_hmm_fit: EM from the parameters given: emission and forward-backward, the read-back of the total loglik (one float64 per iteration: the only
 *     synchronisation), stop when it > 0 and loglik - previous <= tol |previous| or after max_iter iterations, else mstep and transitions and
 *     repeat; after max_iter M-steps one more emission and forward-backward; then Viterbi.  The parameters are updated in place; gamma [n][k]
 *     (optional), labels [n] and info describe the final parameters.  It WAITS for the stream.
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for n < 1, d or k outside the limits, S < 1 or S > n, a
 * seq_start that breaks the rules, ldx < d, a null required pointer, a workspace that is not 16-byte aligned, max_iter < 1, or a tol, prior, kappa,
 * min_var or min_weight that is negative or NaN. */
#define HMM_MAX_D 1024
#define HMM_MAX_K 128
typedef struct { int32_t n_iter, converged; double loglik; float emission_ms, fb_ms, mstep_ms, viterbi_ms; } tmjx_hmm_info_t;
int tmjx_hmm_workspace(int n, int d, int k, int S, int64_t *floats);
int tmjx_hmm_emission(const float *x, int n, int d, int64_t ldx, const float *means, const float *vars, int k, float *logb, float *workspace, void *stream);
int tmjx_hmm_forward_backward(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob, float *gamma,
                              double *xi, double *start, double *loglik, double *total, float *workspace, void *stream);
int tmjx_hmm_mstep(const float *x, int n, int d, int64_t ldx, const float *gamma, int k, double min_var, double min_weight, float *means, float *vars,
                   double *weight, float *workspace, void *stream);
int tmjx_hmm_transitions(const double *xi, const double *start, int k, double prior, double kappa, float *transmat, float *startprob, void *stream);
int tmjx_hmm_viterbi(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob, int logspace,
                     int32_t *labels, double *path_logprob, float *workspace, void *stream);
int tmjx_hmm_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int k, float *means, float *vars, float *transmat,
                 float *startprob, float *gamma, int32_t *labels, int max_iter, double tol, double prior, double kappa, double min_var, double min_weight,
                 tmjx_hmm_info_t *info, float *workspace, void *stream);

/* ---- An autoregressive hidden Markov model over recorded signals x [n][d] (1 <= d <= 32): every one of 1 <= k <= 128 states is its own linear
 * law x_t ~ A_j x_(t-1) + .. + b_j with diagonal noise (csrc/tmjx_arhmm.hip, csrc/arhmm_core.h; DESIGN.md "Autoregressive sequence model").  The
 * conventions of tmjx_hmm_*: no model handle; all device memory is the caller's; everything runs on the caller's stream; ldx >= d; seq_start
 * [S + 1] is a HOST array, checked there and copied to the workspace on the stream (it must stay valid until the queued work has run;
 * tmjx_arhmm_fit waits itself); fixed-order arithmetic, no floating-point atomics: the same bits on every run and at every row stride.
 *   Rows and scoring: 0 <= lags <= 4, lags d <= 128, warmup >= lags.  Row t of a sequence starting at t0 is SCORED when t - t0 >= warmup.  An
 *     unscored row has logb = 0 for every state and adds nothing to the moments: the model conditions on it, the chain still runs through it.  No
 *     lag reads across a sequence boundary; a sequence of `warmup` rows or fewer is entirely unscored (a defined result).
 *   Coordinates: xc = x - center in float32, rounded once; center [d] (device) may be null: zeros.
 *   Regressor: phi_t = [xc_(t-1); ..; xc_(t-lags); 1], p = lags d + 1 columns: column l d + c multiplies feature c at lag l + 1, the last column is
 *     the intercept.  psi_t = [phi_t; xc_t], q = p + d columns.
 *   Parameters (device float32): weights [k][d][p], vars [k][d], center [d].
 *   tmjx_arhmm_workspace: *floats = the scratch of every call below for these n, d, lags, k, S, with what the reused tmjx_hmm_* steps take
 *     (tmjx_hmm_workspace(n, 1, k, S)).  The row split of the moment sums depends on n, k and q only.
 *   tmjx_arhmm_emission: logb [n][k].  Per (row, state), the features c in ascending order: pred = the intercept, one fmaf per regressor column in
 *     ascending column order, r = xc - pred, q = fmaf(r, r (1 / var), q); logb = fmaf(-1/2, q, c_j), c_j = -1/2 sum_c log(2 pi var_jc) in float64
 *     rounded once.  With lags = 0, warmup = 0, a null center and the intercepts as means this gives the bits of tmjx_hmm_emission.
 *   tmjx_arhmm_moments: moments [k][q][q] (device float64) = sum over the scored rows of gamma_tj psi_t psi_t^T, weight [k] (device float64) =
 *     sum over the scored rows of gamma_tj.  Float64 from the first product (gamma psi_a in double, one fma with psi_b), summed in row order over
 *     fixed row parts, the parts in part order; both triangles are written and hold the same bits.
 *   tmjx_arhmm_solve: per state, in float64: G = M[:p,:p] + ridge diag(1, .., 1, 0) (the intercept is not penalised), C = M[p:, :p]; Cholesky in a
 *     fixed order, W = C G^-1, var_c = max((M_xx[c][c] - W_c . C_c) / w, min_var), means_j = center + C[:, p - 1] / w (the state's weighted mean of
 *     x; means [k][d] is optional); everything rounded once.  status [k] (device int32): 0 updated, 1 light (w < min_weight or w <= 0), 2 a
 *     pivot <= 0.  A state with status 1 or 2 keeps the bits of its weights, vars and means.
 *   tmjx_arhmm_fit: EM exactly as tmjx_hmm_fit runs it (the same stopping rule, one read-back per iteration, the final emission, forward-backward
 *     and Viterbi), with tmjx_arhmm_emission where the Gaussian emission stood and tmjx_arhmm_moments + tmjx_arhmm_solve where the M-step stood.
 *     The parameters are updated in place; gamma [n][k] and status [k] are optional; info->n_singular counts the states the last M-step found
 *     singular.  It WAITS for the stream.
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for n < 1, d, lags, lags d or k outside the limits,
 * warmup < lags, S < 1 or S > n, a seq_start that breaks the rules, ldx < d, a null required pointer, a workspace that is not 16-byte aligned,
 * max_iter < 1, or a tol, prior, kappa, ridge, min_var or min_weight that is negative or NaN. */
#define ARHMM_MAX_D 32
#define ARHMM_MAX_LAGS 4
typedef struct { int32_t n_iter, converged; double loglik; float emission_ms, fb_ms, mstep_ms, viterbi_ms; int32_t n_singular, pad_; } tmjx_arhmm_info_t;
int tmjx_arhmm_workspace(int n, int d, int lags, int k, int S, int64_t *floats);
int tmjx_arhmm_emission(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center,
                        const float *weights, const float *vars, int k, float *logb, float *workspace, void *stream);
int tmjx_arhmm_moments(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center,
                       const float *gamma, int k, double *moments, double *weight, float *workspace, void *stream);
int tmjx_arhmm_solve(const double *moments, const double *weight, int k, int d, int lags, const float *center, double ridge, double min_var, double min_weight,
                     float *weights, float *vars, float *means, int32_t *status, float *workspace, void *stream);
int tmjx_arhmm_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center, int k, float *weights,
                   float *vars, float *transmat, float *startprob, float *gamma, int32_t *labels, int32_t *status, int max_iter, double tol, double prior,
                   double kappa, double ridge, double min_var, double min_weight, tmjx_arhmm_info_t *info, float *workspace, void *stream);

/* ---- A behaviour map of recorded features: exact k nearest neighbours, perplexity-calibrated affinities, an exact t-SNE embedding in two
 * dimensions and the placement of further rows on it (csrc/tmjx_tsne.hip, csrc/tsne_core.h; DESIGN.md "Behaviour map").  The conventions of
 * tmjx_kmeans_*: no model handle; all device memory is the caller's; everything runs on the caller's stream; rows of x and q are float32 and may
 * carry a stride (ldx, ldq >= d); fixed-order arithmetic, every division correctly rounded, every sum across points, tiles or workgroups float64
 * in a fixed order, no floating-point or integer atomics: the same bits on every run.  Limits: 1 <= d <= 1024, 2 <= n <= 65536 reference or
 * training rows, 1 <= k <= 128 neighbours, m >= 1 queries.
 *   tmjx_tsne_workspace: *floats = the scratch every call below takes for these n, m, d, k; one sized for (n, m, d, k) also serves the calls that
 *     know n only.  It scales with n + m + n d / 256, never with n n or m n.
 *   tmjx_knn: idx [m][k] (int32), dist2 [m][k] = the k nearest rows of x [n][d] to every row of q [m][d].  With mean = the float64 column mean of
 *     x rounded to float32 (as tmjx_kmeans_assign forms it), qc = q - mean, xc_j = x_j - mean: score_j = ||xc_j||^2 - 2 qc . xc_j, the dot product
 *     one fmaf chain per pair in ascending feature order, dist2 = max(0, ||qc||^2 + score_j).  Every list is sorted ascending by (dist2, index):
 *     ties go to the lowest index.  The pass is fused: a workgroup owns 128 queries, walks the reference tiles staged in LDS and keeps every
 *     query's running k best in LDS; the [m][n] distances are never written.  Row i is left out of query i's list when exclude_self != 0 AND the
 *     search is of x against itself (q == x, m == n, ldq == ldx): then k <= n - 1; otherwise k <= n and exclude_self changes nothing.
 *   tmjx_tsne_affinities: per row of dist2 [m][k], a bisection on beta of 100 iterations from beta = 1, so that the entropy of
 *     p_j ~ exp(-beta (dist2_j - min_j dist2_j)) equals log(perplexity); float32 exponentials, float64 sums in list order; p [m][k] rounded once,
 *     beta [m].  A row whose distances are all equal is the uniform row with beta = 1; a row whose entropy cannot fall to the target (too many
 *     zeros) ends at beta = 2^100 and is uniform over its nearest.  1 <= perplexity < k.
 *   tmjx_tsne_gradient: P is a symmetric CSR (row_ptr [n + 1] HOST int32: row_ptr[0] = 0, non-decreasing, row_ptr[n] = nnz, checked there and
 *     copied to the workspace on the stream, so it must stay valid until the queued work has run; col [nnz] int32 ascending in a row, val [nnz]
 *     float32, both on the device; a column outside [0, n) is skipped).  With dx, dy = y_i - y_j, q_ij = fma(dy, dy, fma(dx, dx, 1)) and
 *     w_ij = 1 / q_ij in float32:  rep_i = sum_{j != i} (w w) (dx, dy) and Z = sum_{i != j} w, float32 products summed in float64 in index order
 *     over fixed parts of the walk, the parts in part order, the points in point order (an all-pairs kernel: a workgroup owns 256 points and
 *     walks tiles of 256 points staged in LDS);  attr_i = sum_j (P_ij w) (dx, dy) over the row in order, float64 sums;
 *     grad_i = 4 (exaggeration attr_i - rep_i / Z) in float64, rounded once; *kl = sum P_ij log(P_ij Z / w_ij) over the stored entries with
 *     P_ij > 0, float64, the unexaggerated P; *z = Z.  z and kl are device float64.
 *   tmjx_tsne_update: delta-bar-delta.  Per component: gain += 0.2 where sign(grad) != sign(velocity), gain *= 0.8 where they agree, then
 *     gain = max(gain, min_gain); velocity = momentum velocity - (eta gain) grad; y += velocity: single float32 operations, none fused.  y is then
 *     recentred: its float64 column means (block sums in point order, blocks in block order) are subtracted in float64, rounded once.
 *   tmjx_tsne_fit: n_iter iterations of gradient then update on the host side of the ABI: the first exaggeration_iters with `exaggeration`
 *     and momentum_early, the rest with exaggeration 1 and momentum_late; then one more gradient at exaggeration 1, whose kl and z describe the y
 *     returned (info->kl, info->z).  y, velocity and gains [n][2] are updated in place.  It equals its own steps bit for bit.  It WAITS for the
 *     stream.
 *   tmjx_tsne_place: y_out_i = sum_j p_ij y_train[idx_ij] in list order, a float32 product and a float32 add per term, none fused; an index
 *     outside [0, n) is skipped.
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for n, m, d or k outside the limits, k above the candidate
 * rows, ldx or ldq < d, a perplexity outside [1, k), a row_ptr that breaks the rules or disagrees with nnz, an exaggeration or eta that is not
 * positive and finite, a momentum outside [0, 1), a negative min_gain, n_iter outside 0 .. 100000, a null required pointer, a workspace that is
 * not 16-byte aligned, or a misaligned array. */
#define TSNE_MAX_D 1024
#define TSNE_MAX_N 65536
#define TSNE_MAX_K 128
typedef struct { int32_t n_iter, pad_; double kl, z; float gradient_ms, update_ms; } tmjx_tsne_info_t;
int tmjx_tsne_workspace(int n, int64_t m, int d, int k, int64_t *floats);
int tmjx_knn(const float *x, int n, int d, int64_t ldx, const float *q, int64_t m, int64_t ldq, int exclude_self, int k, int32_t *idx, float *dist2,
             float *workspace, void *stream);
int tmjx_tsne_affinities(const float *dist2, int64_t m, int k, double perplexity, float *p, float *beta, void *stream);
int tmjx_tsne_gradient(const float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz, double exaggeration, float *grad,
                       double *z, double *kl, float *workspace, void *stream);
int tmjx_tsne_update(float *y, const float *grad, float *velocity, float *gains, int n, float momentum, float eta, float min_gain, float *workspace,
                     void *stream);
int tmjx_tsne_fit(float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz, int n_iter, double exaggeration,
                  int exaggeration_iters, float momentum_early, float momentum_late, float eta, float min_gain, float *velocity, float *gains,
                  tmjx_tsne_info_t *info, float *workspace, void *stream);
int tmjx_tsne_place(const int32_t *idx, const float *p, int64_t m, int k, const float *y_train, int n, float *y_out, void *stream);

/* ---- How two representations of the same n time steps relate: linear CKA, the correlation of two dissimilarity matrices and canonical
 * correlations (csrc/tmjx_compare.hip, csrc/compare_core.h; DESIGN.md "Representation comparison").  The conventions of tmjx_knn: no model handle;
 * all device memory is the caller's; everything runs on the caller's stream; x [n][d1] and y [n][d2] are float32 and may be column slices of wider
 * buffers (ldx >= d1, ldy >= d2), and may be the same buffer; fixed-order arithmetic, every sum across rows, pairs, tiles or workgroups float64 in
 * a fixed order, no atomics of any kind: the same bits on every run.  Limits: n >= 3, 1 <= d1, d2 <= 1024, n <= 32768 for tmjx_rdm_corr.  Both
 * sides are centred by the float64 column means (rounded once to float32, as tmjx_readout_fit forms them) before anything else.
 *   tmjx_compare_workspace: *floats = the scratch every call below takes at these sizes.
 *   tmjx_cka_linear: out[0..2] (device float64) = ||Cxy||_F^2, ||Cxx||_F^2, ||Cyy||_F^2 of the centred covariances (divisor n - 1).  The moments
 *     are split by rows as tmjx_readout_fit's cross moment: float32 FMAs inside a chunk of 256 rows, float64 across chunks and super-chunks; a
 *     row of a moment is squared and summed in float64 by one workgroup (a fixed tree), the rows in row order.  No [d1][d2] matrix leaves the
 *     device.  Linear CKA = out[0] / sqrt(out[1] out[2]) is the caller's; a side without variance gives out[1] or out[2] = 0.
 *   tmjx_rdm_corr: over every pair i < j of the n rows, with Dx_ij and Dy_ij the dissimilarities of rows i, j of x and of y:
 *     sums[0..4] (device float64) = sum Dx, sum Dy, sum Dx^2, sum Dy^2, sum Dx Dy; the Pearson correlation of the two matrices' upper triangles
 *     is the caller's.  Metrics: 0 squared Euclidean, 1 Euclidean, 2 correlation distance (1 - the Pearson correlation of the two column-centred
 *     rows across the features; a row whose centred norm is 0 is at distance 1 from every other row; d >= 2), 3 label mismatch (d = 1: the
 *     column holds integers stored as floats, read as it is; D = 0 where equal, else 1).  A row is staged as ((x - mean) - shift) scale (metric
 *     2: shift its mean across the features, scale 1 / its centred norm, both from float64 sums; else 0 and 1), and a pair is the chain
 *     s = fmaf(a_f - b_f, a_f - b_f, s) over the features in ascending order: D = s, sqrt(s) or s / 2, in float64.  Duplicate rows are at
 *     distance exactly 0.  An all-pairs kernel: a workgroup owns 128 rows i and 64 rows j, stages both in LDS, first for x, then for y, and
 *     leaves five float64 sums (a fixed tree over its threads); the tiles are added in a fixed order.  Neither n x n matrix is ever written.
 *   tmjx_cca: tmjx_pca_fit_wide of both sides as it is; on each side the leading components whose cumulative variance first reaches var_keep,
 *     at least 1, at most max_rank <= 128, never one whose eigenvalue is <= 2^-20 of the largest (info->kx, ky); the whitened cross matrix
 *     M = Wx Cxy Wy^T [kx][ky] in float64 (Cxy: the moment above); its singular value decomposition by tmjx_compare_svd's kernel.  The PCA's
 *     float32 eigenvalues pick the components and do not scale them: with E the kept rows of the components, S = E Cxx E^T [k][k] (float64,
 *     the moment above) = Q diag(s) Q^T by the same kernel and W = diag(s)^-1/2 Q^T E, which has the singular values of
 *     Lx^-1/2 Ux Cxy Uy^T Ly^-1/2 in exact arithmetic and whitens the kept span to float64.  Where a side drops components (k < d), the cut is
 *     sharpened first: the window of at most 128 components around it (64 to each side where there is room) is re-diagonalised against the
 *     float64 Cxx by the same kernel, and its leading Ritz vectors replace the kept rows of the window.  info->converged covers every
 *     decomposition of the call (up to five).
 *     rho [r] (r = min(kx, ky)), descending; a [r][d1], b [r][d2]: the canonical directions in feature space, (x - mean) . a_i of unit variance;
 *     the caller's buffers hold min(max_rank, d1, d2) rows.  It WAITS for the stream.  The PCA's refusals and TMJX_ENOCONV (the PCA's or the
 *     decomposition's) pass through; a side without variance is TMJX_EINVAL.
 *   tmjx_compare_svd: a [rows][cols] float64 (device, row stride lda), rows, cols <= 128 -> sigma [r] descending, u [r][rows], v [r][cols]
 *     (rows: the singular vectors), r = min(rows, cols), all device float64.  One-sided (Hestenes) Jacobi in ONE workgroup, the matrix in LDS in
 *     float64 (transposed when rows < cols), the accumulated rotations in the workspace (2 r^2 + 4 floats; a tmjx_compare_workspace buffer
 *     serves); pairs in round-robin order, four threads a pair; a pair turns while |g_p . g_q| > 2^-40 ||g_p|| ||g_q||, a sweep without a turn ends
 *     it, 60 sweeps without one are TMJX_ENOCONV.  The vector of the longer side that belongs to sigma = 0 is zero.  *sweeps (host): the sweeps
 *     run.  It WAITS for the stream.
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for n < 3, n > 32768 (tmjx_rdm_corr), d1 or d2 outside
 * 1 .. 1024, ldx < d1 or ldy < d2, a metric outside 0 .. 3, metric 3 with d != 1, metric 2 with d < 2, var_keep outside (0, 1], max_rank outside
 * 1 .. 128, rows or cols outside 1 .. 128, a null pointer, a workspace that is not 16-byte aligned, or a misaligned array. */
#define COMPARE_MAX_D 1024
#define COMPARE_MAX_N 32768
#define COMPARE_MAX_RANK 128
typedef struct { int32_t kx, ky, sweeps, converged; float pca_ms, cross_ms, svd_ms, pad_; } tmjx_cca_info_t;
int tmjx_compare_workspace(int n, int d1, int d2, int64_t *floats);
int tmjx_cka_linear(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, double *out, float *workspace, void *stream);
int tmjx_rdm_corr(const float *x, int n, int d1, int64_t ldx, int metric_x, const float *y, int d2, int64_t ldy, int metric_y, double *sums, float *workspace,
                  void *stream);
int tmjx_cca(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, double var_keep, int max_rank, float *rho, float *a, float *b,
             tmjx_cca_info_t *info, float *workspace, void *stream);
int tmjx_compare_svd(const double *a, int rows, int cols, int64_t lda, double *sigma, double *u, double *v, int32_t *sweeps, float *workspace, void *stream);

/* ---- The decoder's Jacobian at recorded steps: the local linearisation of ctrl = tanh(loc) with respect to columns of the decoder's input row
 * (csrc/tmjx_jacobian.hip, csrc/jacobian_core.h; DESIGN.md "Decoder Jacobian").  The conventions of tmjx_knn: no model handle; all device memory
 * is the caller's; everything runs on the caller's stream; fixed-order arithmetic, no atomics: the same bits on every run, and the bits of a row's
 * outputs depend neither on m nor on where the row stands in the list.
 *   The descriptor: L blocks Dense -> SiLU -> LayerNorm (1 <= L <= 8; layer l: W [width][K] with row stride ldw >= K, K = d_in for the first and
 *     the width before it otherwise, b, gamma, beta [width], 1 <= width <= 1024; eps of the LayerNorm, biased variance), the head Wh [2A][H_L]
 *     with row stride ldwh whose first A rows are loc (1 <= A <= 64; only they are read), bh, and the differentiated input columns
 *     [wrt_col0, wrt_col0 + wrt_cols), 1 <= wrt_cols <= 128 inside d_in.
 *   tmjx_jacobian_workspace: *floats = the scratch a call with this descriptor and m rows takes (it stops growing at 1024 rows: the list is worked
 *     through in passes of 1024).
 *   tmjx_decoder_jacobian: x [n][d_in] float32 (row stride ldx); row_index: device int32 [m], the rows to evaluate in that order (null: 0 .. m - 1,
 *     which needs m <= n; an index outside 0 .. n - 1 reads as a row of zeros); mode 0: d ctrl / d x, 1: d loc / d x; scale (optional) [n][wrt_cols]
 *     with row stride ld_scale: the standard deviation of each differentiated input at that row.  Outputs, each optional by null except sums, per-row
 *     ones at position i of the list: ctrl_out [m][A] = tanh(loc), jac [m][A][wrt_cols], gain [m] = ||J_i||_F^2, col2 [m][wrt_cols] = sum_a J_aj^2,
 *     row2 [m][A] = sum_j J_aj^2, action_var [m][A] = sum_j (J_aj scale_j)^2 (needs scale); sums: device float64 [A wrt_cols | wrt_cols^2 | A^2] =
 *     the sums over the m rows of J, J^T J and J J^T (per row float32 chains, across rows float64: groups of 32 rows in row order, the groups in
 *     order).  Forward: u = W h + b (the chain fmaf(W_jk, h_k, .) from 0 in ascending k, then the bias), s = u / (1 + expf(-u)), the LayerNorm by
 *     two fixed trees; reverse for the A rows at once: G = diag(1 - ctrl^2) Wh[:A], per block q = g gamma, du = r (q - mean(q) - xhat mean(q xhat))
 *     silu'(u), g = du W, at the first layer over the wrt columns of W only.
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for a limit above exceeded, a null required pointer, ldx < d_in,
 * a weight stride below its width, ld_scale < wrt_cols, m < 1, n < 1, m > n without row_index, a mode outside 0 .. 1, action_var without scale, a
 * workspace that is not 16-byte aligned, or a misaligned array. */
#define TMJX_JACOBIAN_MAX_LAYERS 8
typedef struct { const float *W, *b, *gamma, *beta; int32_t width, ldw; } tmjx_jacobian_layer_t;
typedef struct {
  int32_t L, d_in;
  tmjx_jacobian_layer_t layer[TMJX_JACOBIAN_MAX_LAYERS];
  float eps;
  int32_t A;
  const float *Wh, *bh;
  int32_t ldwh, wrt_col0, wrt_cols, pad_;
} tmjx_jacobian_desc_t;
int tmjx_jacobian_workspace(const tmjx_jacobian_desc_t *desc, int m, int64_t *floats);
int tmjx_decoder_jacobian(const tmjx_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const int32_t *row_index, int m, const float *scale,
                          int64_t ld_scale, int mode, float *ctrl_out, float *jac, float *gain, float *col2, float *row2, float *action_var, double *sums,
                          float *workspace, void *stream);

/* ---- The LSTM decoder's Jacobian at recorded steps: the local linearisation of one step of the stacked-LSTM decoder, ctrl = tanh(loc), with
 * respect to columns of its input row and to the carry (h, c) entering the step (csrc/tmjx_lstm_jacobian.hip, csrc/lstm_jacobian_core.h; DESIGN.md
 * "LSTM decoder Jacobian").  The conventions of tmjx_decoder_jacobian word for word: no model handle; all device memory is the caller's; everything
 * runs on the caller's stream; the list is worked through in passes of 1024 rows; fixed-order arithmetic, no atomics: the same bits on every run,
 * and the bits of a row's outputs depend neither on m nor on where the row stands in the list.
 *   The descriptor: L stacked cells of H units (1 <= L <= 4, H one of 32, 64, 128, 256; layer k: W_ih [4H][in_k] with row stride ldwi >= in_k,
 *     in_0 = d_in (1 <= d_in <= 1024) and in_k = H above, W_hh [4H][H] with row stride ldwh >= H, b_hh [4H]; gate rows i | f | g | o), the
 *     projection Wp [2A][H] with row stride ldwp whose first A rows are loc (1 <= A <= 64; only they are read), bp, and the differentiated input
 *     columns [wrt_col0, wrt_col0 + wrt_cols), 1 <= wrt_cols <= 128 inside d_in.
 *   tmjx_lstm_jacobian_workspace: *floats = the scratch a call with this descriptor and m rows takes (it stops growing at 1024 rows).
 *   tmjx_lstm_decoder_jacobian: x [n][d_in] (row stride ldx); h_in, c_in [n][L H] (row stride ld_carry >= L H): the carry ENTERING the step, layer k
 *     in the columns [k H, (k + 1) H); row_index, m, mode, scale, ld_scale as in tmjx_decoder_jacobian (an index outside 0 .. n - 1 reads x and the
 *     carry as zeros); carry_scale (optional) [2 L H]: one factor per carry column, the h columns then the c columns (null: ones).  Forward per
 *     row: x_0 = the row; pre = (W_ih[k] x_k + b_hh[k]) + W_hh[k] h_k (each product the chain fmaf from 0 in ascending index), c'_k = sig(f) c_k +
 *     sig(i) tanh(g), h'_k = sig(o) tanh(c'_k), x_{k+1} = h'_k; loc = Wp[:A] h'_{L-1} + bp[:A].  Reverse for the A rows at once: G = diag(1 -
 *     ctrl^2) Wp[:A] (mode 1: Wp[:A]); per layer from the top, Gc = Gh sig(o) (1 - tanh(c')^2), D = [Gc tanh(g) sig'(i) | Gc c_k sig'(f) | Gc sig(i)
 *     (1 - tanh(g)^2) | Gh tanh(c') sig'(o)], d / d c_k = Gc sig(f), d / d h_k = D W_hh[k], d / d x_k = D W_ih[k] (the next Gh; at k = 0 over the
 *     wrt columns only).  Outputs, each optional by null except sums: ctrl_out, jac, gain, col2, row2, action_var with the meaning they have in
 *     tmjx_decoder_jacobian; carry_jac [m][A][2 L H]: the h blocks of every layer, then the c blocks, unscaled; carry_gain [m][2 L]: the squared
 *     Frobenius norm of each layer's block of carry_jac diag(carry_scale), the h layers then the c layers; sums: device float64 [A wrt_cols |
 *     wrt_cols^2 | A^2 | A 2 L H] = the sums over the m rows of J, J^T J, J J^T and carry_jac (across rows float64: groups of 32 rows in row order,
 *     the groups in order).  The bits of the input-side outputs do not depend on which carry outputs are asked for.
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for a limit above exceeded, a null required pointer, ldx < d_in,
 * ld_carry < L H, a weight stride below its width, ld_scale < wrt_cols, m < 1, n < 1, m > n without row_index, a mode outside 0 .. 1, action_var
 * without scale, a workspace that is not 16-byte aligned, or a misaligned array. */
#define TMJX_LSTM_JACOBIAN_MAX_LAYERS 4
typedef struct { const float *W_ih, *W_hh, *b_hh; int32_t ldwi, ldwh; } tmjx_lstm_jacobian_layer_t;
typedef struct {
  int32_t L, H, d_in, A;
  tmjx_lstm_jacobian_layer_t layer[TMJX_LSTM_JACOBIAN_MAX_LAYERS];
  const float *Wp, *bp;
  int32_t ldwp, wrt_col0, wrt_cols, pad_;
} tmjx_lstm_jacobian_desc_t;
int tmjx_lstm_jacobian_workspace(const tmjx_lstm_jacobian_desc_t *desc, int m, int64_t *floats);
int tmjx_lstm_decoder_jacobian(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                               const int32_t *row_index, int m, const float *scale, int64_t ld_scale, const float *carry_scale, int mode, float *ctrl_out,
                               float *jac, float *gain, float *col2, float *row2, float *action_var, float *carry_jac, float *carry_gain, double *sums,
                               float *workspace, void *stream);

/* ---- The LSTM decoder's recurrent dynamics at recorded steps: the carry-to-carry map J_t = d (h', c') / d (h, c) of one step of the stacked-LSTM
 * decoder, applied to tangent rows, and the Lyapunov spectrum of its product along recorded sequences (csrc/tmjx_lstm_tangent.hip,
 * csrc/lstm_tangent_core.h; DESIGN.md "LSTM decoder dynamics").  The conventions of tmjx_lstm_decoder_jacobian: no model handle; all device memory
 * is the caller's; everything runs on the caller's stream; fixed-order float32 chains (a product: fmaf from 0 in ascending index), no atomics: the
 * same bits on every run.  The descriptor is tmjx_lstm_jacobian_desc_t with the same limits on L, H, d_in and the layers; Wp, bp, ldwp, A and the
 * wrt columns are not read.  The input row is held as recorded: these are the CONDITIONAL dynamics of the decoder driven by its recorded input.
 *   The carry space has W = 2 L H columns: the h blocks of every layer, then the c blocks (the layout of carry_jac).  A tangent is a row [W].
 *   The tangent map at a row (x, h, c), for a tangent (dh_k, dc_k per layer): the forward is tmjx_lstm_decoder_jacobian's, with gi, gf, gg, go the
 *     gates, tc = tanh(c'), and per unit ka = go (1 - tc^2), ki = gg gi (1 - gi), kf = c gf (1 - gf), kg = gi (1 - gg^2), ko = tc go (1 - go).  For
 *     k = 0 .. L - 1:  dpre = W_ih[k] dh'_(k-1) + W_hh[k] dh_k (the input product first, the recurrent product added to it; at k = 0 the recurrent
 *     product alone: dx_0 = 0);  dc'_k = fmaf(kg, dpre_g, fmaf(kf, dpre_f, fmaf(ki, dpre_i, gf dc_k)));  dh'_k = fmaf(ka, dc'_k, ko dpre_o).
 *   tmjx_lstm_tangent_workspace: *floats = the scratch for S rows a step (the S sequences of tmjx_lstm_lyapunov; min(n, 1024) rows for
 *     tmjx_lstm_tangent_step) and K tangents each.  It grows with S, K, H and L only, not with n.
 *   tmjx_lstm_tangent_step: x [n][d_in] (row stride ldx); h_in, c_in [n][L H] (row stride ld_carry): the carry ENTERING the step; v [n][K][W]:
 *     K tangents a row; out [n][K][W] = J_row v, row by row, in passes of 1024 rows.  The bits of a row depend neither on n nor on its place.
 *   tmjx_lstm_lyapunov: the n rows form S sequences given by seq_start [S + 1] (HOST int32: seq_start[0] = 0, ascending, no empty sequence,
 *     seq_start[S] = n; the host schedules by length, and the array must stay valid until the queued work has run); 1 <= K <= 32 tangents; q0
 *     [q0_per_seq ? S : 1][K][W]: the first basis of every sequence (of all of them), meant to be orthonormal and not checked.  Per sequence
 *     Q := q0; then for each of its rows t in order V = J_t Q, V = Q' R, Q := Q'.  The factorisation is modified Gram-Schmidt twice: two sweeps over
 *     the columns j in order, in each  r = sqrtf(sum v_j^2),  q_j = v_j / r,  and for every later i:  v_i = fmaf(-(q_j . v_i), q_j, v_i); the dots
 *     and norms are the chains of 256 threads over the elements tid, tid + 256, ... and a fixed tree; column j never reads a later column.
 *     R_jj = r1 r2 and the local exponent is logf(r1) + logf(r2).  A column whose norm is not at least FLT_MIN in either sweep (zero, subnormal, not
 *     a number) becomes a zero column and stays one: its local exponent is -inf from there on and the sequence's status is 1.  Outputs, each
 *     optional by null except sums: local [n][K] = the local exponents at that row; energy [n][K][2 L] = the squared norm of each column of Q'
 *     inside each layer's h block, then each c block; q_out [S][K][W] = the basis behind each sequence's last row; status int32 [S] (0: every
 *     column alive); sums, device float64 [S][K]: per sequence the sum of `local` over its rows t >= warmup (t counted inside the sequence), in row
 *     order, -inf counted as it is; the rows before are propagated and not summed.  The sequences advance in lockstep, ordered by descending
 *     length inside the call only: a sequence's outputs have the same bits alone, among others and at any position of seq_start.
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for L, H, d_in outside the descriptor's limits, K outside
 * 1 .. 32, S < 1, S > 65536, n < 1, a seq_start that breaks the rules, warmup < 0, q0_per_seq outside 0 .. 1, ldx < d_in,
 * ld_carry < L H, a weight stride below its width, a null required pointer, a workspace, v, out, q0 or q_out that is not 16-byte aligned, sums that
 * is not 8-byte aligned, or another array that is not 4-byte aligned. */
#define TMJX_LSTM_TANGENT_MAX_K 32
int tmjx_lstm_tangent_workspace(const tmjx_lstm_jacobian_desc_t *desc, int S, int K, int64_t *floats);
int tmjx_lstm_tangent_step(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                           const float *v, int K, float *out, float *workspace, void *stream);
int tmjx_lstm_lyapunov(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                       const int32_t *seq_start, int S, const float *q0, int q0_per_seq, int K, int warmup, float *local, float *energy, float *q_out,
                       int32_t *status, double *sums, float *workspace, void *stream);

/* ---- Morlet wavelet spectrograms of recorded signals x [n][C] (1 <= C <= 1024) at 1 <= F <= 64 centre frequencies (csrc/tmjx_spectrogram.hip,
 * csrc/spectrogram_core.h; DESIGN.md "Spectrogram").  The conventions of tmjx_hmm_*: no model handle; all device memory is the caller's; everything
 * runs on the caller's stream; x is float32 and may be a column slice of a wider buffer (ldx >= C); the rows form S sequences given by
 * seq_start [S + 1] (HOST int32: seq_start[0] = 0, strictly increasing, seq_start[S] = n); fixed-order arithmetic, no atomics: the same bits on
 * every run, and the bits of a sequence's rows do not depend on where it sits in the call or on what else is in it.
 *   The bank (HOST functions, float64 rounded once to float32): for frequency f_j at sampling rate `rate`, sigma_j = omega0 rate / (2 pi f_j)
 *     samples, R_j = ceil(support sigma_j), and for tau = -R_j .. R_j   g_j[tau] = exp(-tau^2 / (2 sigma_j^2)),
 *     wr_j[tau] = g_j[tau] cos(2 pi f_j tau / rate),  wi_j[tau] = -g_j[tau] sin(2 pi f_j tau / rate).  bank holds, for every frequency in turn, the
 *     tables g, wr, wi of 2 R_j + 1 floats each; offset [F + 1] says where each frequency starts (offset[F] = the size), radius [F] = R_j.
 *     tmjx_wavelet_bank_size gives *floats = offset[F]; tmjx_wavelet_bank fills bank, offset and radius (host memory).  Refused: F outside 1 .. 64,
 *     a frequency outside (0, rate / 2], an R_j above 4096, rate, omega0 or support not positive and finite, a null pointer.
 *   tmjx_spectrogram: bank is that table on the DEVICE; offset and radius stay on the HOST (checked there, copied to the workspace on the stream,
 *     like seq_start: the arrays must stay valid until the queued work has run).  With detrend != 0, m_sc = the mean of channel c over sequence s
 *     (float64 sums of the row classes t mod 4 in row order, the classes added in order, the quotient rounded to float32) and xt = x - m in
 *     float32; otherwise xt = x.  For row t of a sequence of T rows (t counted inside it) only the taps inside the sequence are taken:
 *     lo = max(-R_j, -t), hi = min(R_j, T - 1 - t),
 *       re = sum_{tau = lo .. hi} wr_j[tau] xt[t + tau][c],  im likewise with wi_j  (one float32 FMA chain each, ascending tau),
 *       G = sum_{tau = lo .. hi} g_j[tau]  (a difference of the float64 prefix sums of g_j, rounded once),  A = 2 sqrt(re^2 + im^2) / G.
 *     out [n][ldo >= F C] float32, column j C + c (frequency-major): A with TMJX_SPECTROGRAM_AMPLITUDE, ln(max(A, log_floor)) with
 *     TMJX_SPECTROGRAM_LOG (log_floor > 0); columns beyond F C are not written.  coverage [n][F] = G / (the sum of all of g_j): the share of the
 *     window inside the sequence, exactly 1 where it fits.  A unit sinusoid at f_j gives A = 1, also near an edge.  A NaN in a sequence makes
 *     that sequence's outputs NaN and no other's.
 *   tmjx_spectrogram_workspace: *floats = the scratch for these C, F, S (the sequence means and tables; n sizes nothing).
 * Each returns TMJX_EINVAL before any launch, with a message that names the value, for n < 1, C or F outside the limits, S < 1 or S > n, a
 * seq_start that breaks the rules, ldx < C, ldo < F C, a radius outside 0 .. 4096, offsets that do not follow from the radii, an unknown
 * output_kind, a log_floor that is not positive (log output), a null pointer, a workspace that is not 16-byte aligned. */
#define TMJX_SPECTROGRAM_MAX_C 1024
#define TMJX_SPECTROGRAM_MAX_F 64
#define TMJX_SPECTROGRAM_MAX_R 4096
#define TMJX_SPECTROGRAM_AMPLITUDE 0
#define TMJX_SPECTROGRAM_LOG 1
int tmjx_wavelet_bank_size(double rate, const double *freqs, int F, double omega0, double support, int64_t *floats);
int tmjx_wavelet_bank(double rate, const double *freqs, int F, double omega0, double support, float *bank, int32_t *offset, int32_t *radius);
int tmjx_spectrogram_workspace(int n, int C, int F, int S, int64_t *floats);
int tmjx_spectrogram(const float *x, int n, int C, int64_t ldx, const int32_t *seq_start, int S, const float *bank, const int32_t *offset,
                     const int32_t *radius, int F, int detrend, int output_kind, float log_floor, float *out, int64_t ldo, float *coverage, float *workspace,
                     void *stream);

/* ---- Activation intervention (csrc/tmjx_intervene.hip, csrc/intervene_core.h; DESIGN.md "Interventions"): one launch that edits, in place, the
 * columns [0, w) of the rows h [n][ld] — a layer's output buffer, or a column slice of one — between two launches of a policy step.  Row r at step t:
 *   subspace mode:  p_k = sum_j (h_j - c_j) v_kj;  e_j = sum_k ((g_k - 1) p_k + o_k) v_kj;  h'_j = h_j + dose_r e_j   (dirs [K][ldv], gain / offset [K])
 *   units mode:     h'_j = h_j + dose_r ((g_j - 1)(h_j - c_j) + o_j)                                                   (gain / offset [w])
 * A row is ON when t_on[r] <= t < t_off[r] and dose[r] != 0; an OFF row is never stored to.  proj (optional, subspace mode) receives p_k of EVERY
 * row at every call, ON or OFF.  One wave per row, the row in registers, read once; per-lane partial sums over j = lane, lane + 64, .. ascending,
 * a fixed cross-lane tree, k ascending, no atomics: a row's bits do not depend on n, its position or the other rows' gates.
 * Refused before any device call (TMJX_EINVAL, the message names the value): a null descriptor or required pointer, a pointer that is not 4-byte
 * aligned, w outside 1 .. 1024, ld < w, n < 1, an unknown mode, K outside 1 .. 16, ldv < w, ldp < K, proj in units mode.  center may be null (0). */
#define TMJX_INTERVENE_SUBSPACE 0
#define TMJX_INTERVENE_UNITS 1
typedef struct {
  float *h; int32_t ld, w;           /* target rows [n][ld >= w] */
  int32_t n, mode;
  const float *dirs; int32_t K, ldv; /* subspace mode: [K][ldv >= w] */
  const float *center;               /* optional [w] */
  const float *gain, *offset;        /* [K] (subspace) or [w] (units) */
  const float *dose;                 /* [n] */
  const int32_t *t_on, *t_off;       /* [n] */
  float *proj; int32_t ldp, pad_;    /* optional [n][ldp >= K], subspace mode only */
} tmjx_intervene_t;
int tmjx_intervene_ok(const tmjx_intervene_t *d);            /* 1 / 0, reason in tmjx_last_error */
int tmjx_intervene(const tmjx_intervene_t *d, int t, void *stream);

const char *tmjx_last_error(void);
const char *tmjx_version(void);

#ifdef __cplusplus
}
#endif
#endif
