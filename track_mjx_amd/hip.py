"""ctypes binding of libtmjx_hip.so (the C-ABI declared in include/tmjx.h).

The HIP library is the product: there is no CPU fallback.  Importing this module never fails
(so host-only tooling keeps working), but `lib()` raises if the shared object is missing or does
not load, and every entry point raises `TmjxError` on a non-zero return code.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
SO_PATH = Path(os.environ.get("TMJX_SO", str(_PKG / "libtmjx_hip.so")))  # TMJX_SO: alternative build (profiling)
CSRC = _PKG / "csrc"
SOURCES = (CSRC / "tmjx_hip.hip", CSRC / "tmjx_bf16.hip", CSRC / "tmjx_wave.hip", CSRC / "tmjx_chain.hip", CSRC / "tmjx_lstm.hip",
           CSRC / "tmjx_rollout.hip", CSRC / "tmjx_wave_sensors.hip", CSRC / "tmjx_wave_align.hip", CSRC / "tmjx_wave_rand.hip", CSRC / "tmjx_render.hip", CSRC / "tmjx_act.hip", CSRC / "tmjx_pca.hip", CSRC / "tmjx_pca_wide.hip", CSRC / "tmjx_readout.hip", CSRC / "tmjx_intervene.hip", CSRC / "tmjx_kmeans.hip", CSRC / "tmjx_hmm.hip", CSRC / "tmjx_spectrogram.hip", CSRC / "tmjx_arhmm.hip", CSRC / "tmjx_tsne.hip", CSRC / "tmjx_compare.hip", CSRC / "tmjx_jacobian.hip", CSRC / "tmjx_lstm_jacobian.hip", CSRC / "tmjx_lstm_tangent.hip")
# per-source compiler flags: the physics kernel's unit is built without machine LICM (csrc/tmjx_wave.hip says why)
SOURCE_FLAGS = {"tmjx_wave.hip": ("-mllvm", "-disable-machine-licm"),
                "tmjx_wave_sensors.hip": ("-mllvm", "-disable-machine-licm"),      # (the recording kernel: the same loop body)
                "tmjx_wave_rand.hip": ("-mllvm", "-disable-machine-licm"),         # (the domain-randomisation kernel: likewise)
                "tmjx_jacobian.hip": ("-ffp-contract=off",),      # (the Jacobian states its order: only the fmaf it writes is fused, as on the host)
                "tmjx_lstm_jacobian.hip": ("-ffp-contract=off",),      # (the LSTM decoder's likewise)
                "tmjx_lstm_tangent.hip": ("-ffp-contract=off",)}      # (and its recurrent dynamics)


class TmjxError(RuntimeError):
    pass


class Layout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "nq", "nv", "nu", "nbody", "ncon", "nefc", "obs_size", "ref_obs_size", "n_metrics", "window",
        "qpos", "qvel", "act", "qacc_warmstart", "time", "xpos", "xmat_torso", "qfrc_actuator",
        "prev_ctrl", "action_buffer", "done", "steps_f", "first_phys", "first_obs", "first_prev_ctrl", "state_rows",
        "i_clip_idx", "i_start_frame", "i_buffer_index", "i_nan_count", "istate_rows", "ws_rows")]


class Minibatch(C.Structure):
    """tmjx_minibatch_t (include/tmjx.h)."""
    _fields_ = ([(k, C.c_void_p) for k in ("obs", "next_last", "raw_action", "log_prob", "reward", "discount", "truncation", "perm", "mean", "std", "obs_n", "next_n",
                                           "raw_action_g", "scalars_g", "eps", "noise", "state")] + [("seed", C.c_uint64)] +
                [(k, C.c_int32) for k in ("T", "R", "B", "W", "A", "Z", "advance")])


class ColsumProblem(C.Structure):
    """tmjx_colsum_problem_t (include/tmjx.h)."""
    _fields_ = [("partial", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int32), ("width", C.c_int32)]


class DwProblem(C.Structure):
    """tmjx_dw_problem_t (include/tmjx.h)."""
    _fields_ = [("dY", C.c_void_p), ("X", C.c_void_p), ("dW", C.c_void_p), ("db", C.c_void_p), ("scratch", C.c_void_p),
                ("ldy", C.c_int32), ("ldx", C.c_int32), ("lddw", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32)]


class BdwProblem(C.Structure):
    """tmjx_bdw_problem_t (include/tmjx.h)."""
    _fields_ = [("dY", C.c_void_p), ("X", C.c_void_p), ("dW", C.c_void_p), ("db", C.c_void_p), ("scratch", C.c_void_p),
                ("y_is_f32", C.c_int32), ("x_is_f32", C.c_int32), ("ldy", C.c_int32), ("ldx", C.c_int32), ("lddw", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32)]


class RolloutStore(C.Structure):
    """tmjx_rollout_store_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("obs", "obs_dst0", "obs_dst1", "raw", "raw_dst", "logp", "logp_dst", "reward", "reward_dst", "done", "discount_dst",
                                          "trunc", "trunc_dst")] + [(k, C.c_int32) for k in ("n", "W", "A")] + [("obs_dst2", C.c_void_p)]


class Bf16Shadow(C.Structure):
    """tmjx_bf16_shadow_t (include/tmjx.h)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("dst_t", C.c_void_p), ("N", C.c_int32), ("K", C.c_int32), ("ld_src", C.c_int32),
                ("ld_dst", C.c_int32), ("ld_dst_t", C.c_int32)]


class ChainLayer(C.Structure):
    """tmjx_chain_layer_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("W", "bias", "gamma", "beta", "z", "y", "stats")] + [("K", C.c_int32), ("ldw", C.c_int32)]


class ChainFwd(C.Structure):
    """tmjx_chain_fwd_t (include/tmjx.h)."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int32), ("M", C.c_int32), ("n_hidden", C.c_int32), ("epi", C.c_int32), ("hidden", ChainLayer * 4),
                ("Wf", C.c_void_p), ("bf", C.c_void_p), ("outf", C.c_void_p), ("Nf", C.c_int32), ("ldwf", C.c_int32), ("ldof", C.c_int32), ("eps", C.c_float), ("rows_alloc", C.c_int32),
                ("prof", C.c_void_p)]


CHAIN_MAX_HIDDEN = 4         # TMJX_CHAIN_MAX_HIDDEN (include/tmjx.h)


class DecoderBlock(C.Structure):
    """tmjx_decoder_block_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("W", "bias", "gamma", "beta")] + [("width", C.c_int32), ("ldw", C.c_int32)]


class DecoderAct(C.Structure):
    """tmjx_decoder_act_t (include/tmjx.h)."""
    _fields_ = [("latents", C.c_void_p), ("ldz", C.c_int32), ("obs", C.c_void_p), ("obs_s0", C.c_int64), ("obs_s1", C.c_int64), ("mean", C.c_void_p),
                ("std", C.c_void_p), ("n", C.c_int32), ("Z", C.c_int32), ("obs_w", C.c_int32), ("ref_w", C.c_int32), ("n_blocks", C.c_int32),
                ("block", DecoderBlock * CHAIN_MAX_HIDDEN), ("Wf", C.c_void_p), ("bf", C.c_void_p), ("ldwf", C.c_int32), ("A", C.c_int32), ("eps", C.c_float),
                ("action_t", C.c_void_p), ("ctrl", C.c_void_p), ("logits", C.c_void_p), ("ldl", C.c_int32)]


class PolicyAct(C.Structure):
    """tmjx_policy_act_t (include/tmjx.h)."""
    _fields_ = ([("obs", C.c_void_p), ("ldo", C.c_int64)] + [(k, C.c_void_p) for k in ("mean", "inv_std", "nmean", "nstd")] +
                [(k, C.c_int32) for k in ("n", "K0", "Z", "obs_w", "ref_w", "A", "n_enc", "n_dec")] +
                [("enc", DecoderBlock * CHAIN_MAX_HIDDEN), ("dec", DecoderBlock * CHAIN_MAX_HIDDEN), ("W2", C.c_void_p), ("b2", C.c_void_p),
                 ("ldw2", C.c_int32), ("ldwh", C.c_int32), ("Wh", C.c_void_p), ("bh", C.c_void_p), ("eps", C.c_void_p), ("noise", C.c_void_p),
                 ("seed", C.c_uint64), ("rng_state", C.c_void_p), ("ln_eps", C.c_float), ("pad_", C.c_int32)] +
                [(k, C.c_void_p) for k in ("fc2", "logits", "raw", "action_t", "logp")])


LSTM_DECODER_MAX_LAYERS = 4  # TMJX_LSTM_DECODER_MAX_LAYERS (include/tmjx.h)


class LstmDecoderLayer(C.Structure):
    """tmjx_lstm_decoder_layer_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("Wi", "Wh", "bh")] + [("ldwi", C.c_int32), ("ldwh", C.c_int32)]


class LstmDecoderAct(C.Structure):
    """tmjx_lstm_decoder_act_t (include/tmjx.h)."""
    _fields_ = [("latents", C.c_void_p), ("ldz", C.c_int32), ("obs", C.c_void_p), ("obs_s0", C.c_int64), ("obs_s1", C.c_int64), ("mean", C.c_void_p),
                ("std", C.c_void_p), ("reset", C.c_void_p), ("n", C.c_int32), ("Z", C.c_int32), ("obs_w", C.c_int32), ("ref_w", C.c_int32), ("L", C.c_int32),
                ("H", C.c_int32), ("layer", LstmDecoderLayer * LSTM_DECODER_MAX_LAYERS), ("Wp", C.c_void_p), ("bp", C.c_void_p), ("ldwp", C.c_int32),
                ("A", C.c_int32), ("h", C.c_void_p), ("c", C.c_void_p), ("ld", C.c_int32), ("action_t", C.c_void_p), ("ctrl", C.c_void_p),
                ("logits", C.c_void_p), ("ldl", C.c_int32)]


class ChainBwdStage(C.Structure):
    """tmjx_chain_bwd_stage_t (include/tmjx.h)."""
    _fields_ = [("W", C.c_void_p), ("ldw", C.c_int32)] + [(k, C.c_void_p) for k in ("z", "bias", "gamma", "stats", "dz", "partial")]


class ChainBwd(C.Structure):
    """tmjx_chain_bwd_t (include/tmjx.h)."""
    _fields_ = [("G", C.c_void_p), ("ldg", C.c_int32), ("Kg", C.c_int32), ("M", C.c_int32), ("n_stages", C.c_int32), ("epi", C.c_int32), ("stage", ChainBwdStage * 4),
                ("W0", C.c_void_p), ("ldw0", C.c_int32), ("dx_cols", C.c_int32), ("dx", C.c_void_p), ("lddx", C.c_int32), ("rows_alloc", C.c_int32), ("prof", C.c_void_p)]


class LstmFwd(C.Structure):
    """tmjx_lstm_fwd_t (include/tmjx.h)."""
    _fields_ = [("xg", C.c_void_p), ("ldx", C.c_int32), ("Wh", C.c_void_p), ("ldw", C.c_int32), ("bh", C.c_void_p), ("h0", C.c_void_p), ("c0", C.c_void_p),
                ("ld0", C.c_int32), ("reset", C.c_void_p), ("ldr", C.c_int32), ("h", C.c_void_p), ("c", C.c_void_p), ("ldo", C.c_int32),
                ("gates", C.c_void_p), ("h_prev", C.c_void_p), ("T", C.c_int32), ("rows", C.c_int32), ("H", C.c_int32)]


class LstmBwd(C.Structure):
    """tmjx_lstm_bwd_t (include/tmjx.h)."""
    _fields_ = [("dh", C.c_void_p), ("ldd", C.c_int32), ("Wh", C.c_void_p), ("ldw", C.c_int32), ("gates", C.c_void_p), ("c", C.c_void_p), ("ldo", C.c_int32),
                ("c0", C.c_void_p), ("ld0", C.c_int32), ("reset", C.c_void_p), ("ldr", C.c_int32), ("dgates", C.c_void_p), ("dh0", C.c_void_p),
                ("dc0", C.c_void_p), ("T", C.c_int32), ("rows", C.c_int32), ("H", C.c_int32)]


DONE_NONE, DONE_RESET, DONE_ALIGN = 0, 1, 2      # TMJX_DONE_* (include/tmjx.h)
RECORD_SOA, RECORD_ROWMAJOR, RECORD_MAX_STREAMS, RECORD_MAX_IDX = 0, 1, 64, 32


class RecordStream(C.Structure):
    """tmjx_record_stream_t (include/tmjx.h)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)] + [(k, C.c_int32) for k in ("layout", "ld", "w", "src_extent", "T", "t0", "n_idx")] + \
               [("idx", C.c_int32 * RECORD_MAX_IDX), ("pad_", C.c_int32)]


CAMERA_FIXED, CAMERA_TRACK, CAMERA_TRACKCOM = 0, 1, 2      # TMJX_CAMERA_* (include/tmjx.h)


class Camera(C.Structure):
    """tmjx_camera_t (include/tmjx.h)."""
    _fields_ = [("body", C.c_int32), ("mode", C.c_int32), ("offset", C.c_float * 3), ("quat", C.c_float * 4), ("fovy", C.c_float)]


class RenderInfo(C.Structure):
    """tmjx_render_info_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_int32) for k in ("ngeom", "ncam", "rec_floats", "cam_floats", "nprim")] + [("prims_offset", C.c_int64), ("workspace_floats", C.c_int64)]


ENOCONV = -34                     # TMJX_ENOCONV (include/tmjx.h)
PCA_MAX_D, PCA_ROWS_PER_WG, PCA_MAX_K = 128, 256, 8      # csrc/pca_core.h
PCA_WIDE_MAX_D, PCA_WIDE_BLOCK, PCA_WIDE_MAX_SUPER = 1024, 64, 16      # csrc/pca_wide_core.h
READOUT_MAX_M, READOUT_MAX_L = 512, 16      # csrc/readout_core.h
KMEANS_MAX_D, KMEANS_MAX_K = 1024, 256      # csrc/kmeans_core.h


class KMeansInfo(C.Structure):
    """tmjx_kmeans_info_t (include/tmjx.h)."""
    _fields_ = [("n_iter", C.c_int32), ("changed", C.c_int32), ("inertia", C.c_double), ("assign_ms", C.c_float), ("update_ms", C.c_float)]


HMM_MAX_D, HMM_MAX_K = 1024, 128      # csrc/hmm_core.h
SPECTROGRAM_MAX_C, SPECTROGRAM_MAX_F, SPECTROGRAM_MAX_R = 1024, 64, 4096      # csrc/spectrogram_core.h
SPECTROGRAM_AMPLITUDE, SPECTROGRAM_LOG = 0, 1      # TMJX_SPECTROGRAM_* (include/tmjx.h)


class HmmInfo(C.Structure):
    """tmjx_hmm_info_t (include/tmjx.h)."""
    _fields_ = [("n_iter", C.c_int32), ("converged", C.c_int32), ("loglik", C.c_double), ("emission_ms", C.c_float), ("fb_ms", C.c_float),
                ("mstep_ms", C.c_float), ("viterbi_ms", C.c_float)]


ARHMM_MAX_D, ARHMM_MAX_LAGS = 32, 4      # csrc/arhmm_core.h


class ArhmmInfo(C.Structure):
    """tmjx_arhmm_info_t (include/tmjx.h)."""
    _fields_ = HmmInfo._fields_ + [("n_singular", C.c_int32), ("pad_", C.c_int32)]


TSNE_MAX_D, TSNE_MAX_N, TSNE_MAX_K = 1024, 65536, 128      # csrc/tsne_core.h


class TsneInfo(C.Structure):
    """tmjx_tsne_info_t (include/tmjx.h)."""
    _fields_ = [("n_iter", C.c_int32), ("pad_", C.c_int32), ("kl", C.c_double), ("z", C.c_double), ("gradient_ms", C.c_float), ("update_ms", C.c_float)]


COMPARE_MAX_D, COMPARE_MAX_N, COMPARE_MAX_RANK = 1024, 32768, 128      # csrc/compare_core.h
COMPARE_SQEUCLIDEAN, COMPARE_EUCLIDEAN, COMPARE_CORRELATION, COMPARE_LABEL = 0, 1, 2, 3      # the metrics of tmjx_rdm_corr (include/tmjx.h)


class CcaInfo(C.Structure):
    """tmjx_cca_info_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_int32) for k in ("kx", "ky", "sweeps", "converged")] + [(k, C.c_float) for k in ("pca_ms", "cross_ms", "svd_ms", "pad_")]


JACOBIAN_MAX_LAYERS, JACOBIAN_MAX_WIDTH, JACOBIAN_MAX_A, JACOBIAN_MAX_WRT, JACOBIAN_CHUNK = 8, 1024, 64, 128, 1024      # csrc/jacobian_core.h
JACOBIAN_CTRL, JACOBIAN_LOC = 0, 1      # the modes of tmjx_decoder_jacobian (include/tmjx.h)


class JacobianLayer(C.Structure):
    """tmjx_jacobian_layer_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("W", "b", "gamma", "beta")] + [("width", C.c_int32), ("ldw", C.c_int32)]


class JacobianDesc(C.Structure):
    """tmjx_jacobian_desc_t (include/tmjx.h)."""
    _fields_ = [("L", C.c_int32), ("d_in", C.c_int32), ("layer", JacobianLayer * JACOBIAN_MAX_LAYERS), ("eps", C.c_float), ("A", C.c_int32), ("Wh", C.c_void_p),
                ("bh", C.c_void_p), ("ldwh", C.c_int32), ("wrt_col0", C.c_int32), ("wrt_cols", C.c_int32), ("pad_", C.c_int32)]


LSTM_JACOBIAN_MAX_LAYERS, LSTM_JACOBIAN_MAX_DIN = 4, 1024      # csrc/lstm_jacobian_core.h (H: agent.lstm.LSTM_HIDDEN_SIZES; A, wrt, the pass: the MLP's)
LSTM_TANGENT_MAX_K = 32      # csrc/lstm_tangent_core.h: the tangents of a sequence (tmjx_lstm_tangent_step, tmjx_lstm_lyapunov)


class LstmJacobianLayer(C.Structure):
    """tmjx_lstm_jacobian_layer_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("W_ih", "W_hh", "b_hh")] + [("ldwi", C.c_int32), ("ldwh", C.c_int32)]


class LstmJacobianDesc(C.Structure):
    """tmjx_lstm_jacobian_desc_t (include/tmjx.h)."""
    _fields_ = [("L", C.c_int32), ("H", C.c_int32), ("d_in", C.c_int32), ("A", C.c_int32), ("layer", LstmJacobianLayer * LSTM_JACOBIAN_MAX_LAYERS), ("Wp", C.c_void_p),
                ("bp", C.c_void_p), ("ldwp", C.c_int32), ("wrt_col0", C.c_int32), ("wrt_cols", C.c_int32), ("pad_", C.c_int32)]


INTERVENE_SUBSPACE, INTERVENE_UNITS, INTERVENE_MAX_W, INTERVENE_MAX_K = 0, 1, 1024, 16      # include/tmjx.h, csrc/intervene_core.h


class Intervene(C.Structure):
    """tmjx_intervene_t (include/tmjx.h)."""
    _fields_ = [("h", C.c_void_p), ("ld", C.c_int32), ("w", C.c_int32), ("n", C.c_int32), ("mode", C.c_int32), ("dirs", C.c_void_p), ("K", C.c_int32),
                ("ldv", C.c_int32), ("center", C.c_void_p), ("gain", C.c_void_p), ("offset", C.c_void_p), ("dose", C.c_void_p), ("t_on", C.c_void_p),
                ("t_off", C.c_void_p), ("proj", C.c_void_p), ("ldp", C.c_int32), ("pad_", C.c_int32)]


class PcaInfo(C.Structure):
    """tmjx_pca_info_t (include/tmjx.h)."""
    _fields_ = [("sweeps", C.c_int32), ("converged", C.c_int32), ("off_rel", C.c_float), ("moments_ms", C.c_float), ("jacobi_ms", C.c_float)]


class StripStyle(C.Structure):
    """tmjx_strip_style_t (include/tmjx.h)."""
    _fields_ = [(k, C.c_int32) for k in ("margin_left", "margin_right", "margin_top", "margin_bottom")] + \
               [("line_half_width", C.c_float), ("marker_radius", C.c_float), ("colour", (C.c_uint8 * 4) * 8)] + \
               [(k, C.c_uint8 * 4) for k in ("background", "axes", "terminated")]


class PpoCfg(C.Structure):
    """tmjx_ppo_cfg_t (include/tmjx.h)."""
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("A", C.c_int32), ("Z", C.c_int32), ("reward_scaling", C.c_float),
                ("discounting", C.c_float), ("gae_lambda", C.c_float), ("clip_eps", C.c_float), ("entropy_cost", C.c_float),
                ("kl_weight", C.c_float), ("normalize_advantage", C.c_int32), ("accumulate", C.c_int32)]


_i, _i64, _u64, _f, _d, _vp, _s, _P = C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p, C.c_char_p, C.POINTER
# entry point -> (argument types, return type), one for one with the prototypes of include/tmjx.h (tests/test_abi.py compares the two).  Data
# pointers are void pointers (tensor addresses are passed as integers); a pointer the host fills or reads keeps its type
SIGNATURES = {
    "tmjx_model_create": ([_s, C.c_size_t, _P(_vp)], _i),
    "tmjx_model_destroy": ([_vp], None),
    "tmjx_layout": ([_vp, _P(Layout)], _i),
    "tmjx_clips_upload": ([_vp] * 6 + [_i, _i], _i),
    "tmjx_reset": ([_vp] * 9 + [_i, _vp], _i),
    "tmjx_step": ([_vp] * 10 + [_i, _vp], _i),
    "tmjx_physics": ([_vp, _vp, _vp, _i, _vp, _i, _vp], _i),
    "tmjx_physics_step": ([_vp] * 4 + [_i, _vp], _i),
    "tmjx_forward": ([_vp, _vp, _vp, _i, _vp], _i),
    "tmjx_reward_obs": ([_vp] * 10 + [_i, _vp], _i),
    "tmjx_reward_frame": ([_vp] * 14 + [_i, _vp], _i),
    "tmjx_gae": ([_vp] * 5 + [_f, _f, _vp, _vp, _i, _i, _vp], _i),
    "tmjx_ppo_scratch_floats": ([_i, _i], _i),
    "tmjx_ppo_loss": ([_P(PpoCfg)] + [_vp] * 16, _i),
    "tmjx_ppo_loss_phases": ([_P(PpoCfg)] + [_vp] * 15 + [_i, _vp], _i),
    "tmjx_silu_ln_partial_floats": ([_i, _i], _i),
    "tmjx_silu_ln_fwd": ([_vp] * 6 + [_i, _i, _f, _vp], _i),
    "tmjx_silu_ln_bwd": ([_vp] * 8 + [_i, _i, _vp], _i),
    "tmjx_silu_ln_fwd_bf16": ([_vp] * 5 + [_i, _vp, _i, _i, _f, _vp], _i),
    "tmjx_silu_ln_bwd_bf16": ([_vp] * 6 + [_i, _vp, _vp, _i, _i, _vp], _i),
    "tmjx_minibatch_begin_bf16": ([_P(Minibatch), _vp, _i, _vp], _i),
    "tmjx_gather_normalize": ([_vp] * 5 + [_i] * 4 + [_vp], _i),
    "tmjx_latent_concat": ([_vp] * 4 + [_i] * 4 + [_i64, _i64, _vp, _vp, _i, _u64, _vp, _vp], _i),
    "tmjx_latent_concat_bwd": ([_vp] * 4 + [_i, _i, _i, _vp], _i),
    "tmjx_latent_concat_bwd_add": ([_vp] * 5 + [_i, _i, _i, _vp], _i),
    "tmjx_sample_action": ([_vp] * 5 + [_i, _i, _u64, _vp, _vp], _i),
    "tmjx_linear_nolds": ([_vp, _i64, _i64, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "tmjx_linear_act": ([_vp, _i64, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp], _i),
    "tmjx_linear_act_ok": ([_vp, _i64, _vp, _i, _i], _i),
    "tmjx_linear_nolds_norm": ([_vp, _i64, _i64, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp], _i),
    "tmjx_linear_nolds_bf16": ([_vp, _i64, _i64, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp], _i),
    "tmjx_adam_clip": ([_vp] * 5 + [_i64] + [_f] * 7 + [_vp], _i),
    "tmjx_adam_clip_norm": ([_vp] * 6 + [_i64] + [_f] * 7 + [_vp], _i),
    "tmjx_adam_clip_norm_frozen": ([_vp] * 6 + [_i64, _i64, _i64] + [_f] * 7 + [_vp], _i),
    "tmjx_adam_norm_floats": ([], _i),
    "tmjx_colsum_scratch_floats": ([_i], _i),
    "tmjx_colsum": ([_vp, _vp, _vp, _i, _i, _vp], _i),
    "tmjx_gather_minibatch": ([_vp] * 14 + [_i] * 5 + [_vp], _i),
    "tmjx_minibatch_begin": ([_P(Minibatch), _vp], _i),
    "tmjx_philox4x32_10": ([_vp, _vp, _vp], _i),
    "tmjx_gemm_nt": ([_vp, _i, _vp, _i, _vp, _vp] + [_i] * 4 + [_vp], _i),
    "tmjx_gemm_nt_silu_ln": ([_vp, _i, _vp, _i] + [_vp] * 5 + [_i, _vp, _i, _i, _i, _f, _vp], _i),
    "tmjx_gemm_nt_silu_ln_ok": ([_vp, _i, _vp, _i, _i], _i),
    "tmjx_gemm_nn": ([_vp, _i, _vp, _i, _vp] + [_i] * 4 + [_vp], _i),
    "tmjx_colsum_grouped": ([_P(ColsumProblem), _i, _vp], _i),
    "tmjx_gemm_nn_ln_bwd": ([_vp, _i, _vp, _i] + [_vp] * 6 + [_i, _i, _i, _vp], _i),
    "tmjx_gemm_nn_ln_bwd_ok": ([_vp, _i, _vp, _i, _i], _i),
    "tmjx_gemm_nn_ln_bwd_partial_floats": ([_i, _i], _i64),
    "tmjx_gemm_dw": ([_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "tmjx_gemm_dw_grouped": ([_P(DwProblem), _i, _vp], _i),
    "tmjx_gemm_dw_scratch_floats": ([_i, _i, _i], _i64),
    "tmjx_set_wrappers": ([_vp, _i, _i], _i),
    "tmjx_set_action_repeat": ([_vp, _i], _i),
    "tmjx_stats_scratch_floats": ([_i], _i),
    "tmjx_stats_sums": ([_vp] * 4 + [_i64, _i, _vp], _i),
    "tmjx_stats_apply": ([_vp, _f] + [_vp] * 4 + [_i, _f, _f, _vp], _i),
    "tmjx_stats_apply_pinned": ([_vp, _f] + [_vp] * 4 + [_i, _i, _f, _f, _vp], _i),
    "tmjx_rollout_store": ([_P(RolloutStore), _vp], _i),
    "tmjx_clips_share": ([_vp, _vp], _i),
    "tmjx_gemm_nt_silu": ([_vp, _i, _vp, _i, _vp, _vp, _vp] + [_i] * 4 + [_vp], _i),
    "tmjx_gemm_nt_silu_ok": ([_vp, _i, _vp, _i], _i),
    "tmjx_silu_fwd": ([_vp, _vp, _vp, _i64, _i, _vp], _i),
    "tmjx_silu_bwd": ([_vp] * 4 + [_i64, _i, _vp], _i),
    "tmjx_gemm_nn_silu_bwd_ok": ([_vp, _i, _vp, _i], _i),
    "tmjx_gemm_nn_silu_bwd": ([_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "tmjx_silu_bwd_rank1": ([_vp] * 5 + [_i64, _i, _vp], _i),
    "tmjx_head_dw_scratch_floats": ([_i, _i], _i64),
    "tmjx_head_dw": ([_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp], _i),
    "tmjx_head_fwd_ok": ([_vp, _i, _vp, _i], _i),
    "tmjx_head_fwd": ([_vp, _i, _vp, _vp, _vp, _i, _i, _vp], _i),
    "tmjx_bf16_shadow": ([_P(Bf16Shadow), _i, _vp], _i),
    "tmjx_bgemm_nt": ([_vp, _i, _i, _vp, _i, _vp, _vp] + [_i] * 4 + [_vp], _i),
    "tmjx_bgemm_dw": ([_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp], _i),
    "tmjx_bgemm_dw_grouped": ([_P(BdwProblem), _i, _i, _vp], _i),
    "tmjx_bgemm_dw_scratch_floats": ([_i, _i, _i], _i64),
    "tmjx_bgemm_row_tile_ok": ([_i], _i),
    "tmjx_bf16_z_bytes": ([], _i),
    "tmjx_bgemm_partial_floats": ([_i, _i, _i], _i64),
    "tmjx_bgemm_ln_fwd": ([_vp, _i, _i, _vp, _i] + [_vp] * 4 + [_i, _vp, _i, _vp, _i, _i, _i, _f, _vp], _i),
    "tmjx_bgemm_ln_bwd": ([_vp, _i, _i, _vp, _i, _vp, _i] + [_vp] * 4 + [_i, _vp, _i, _i, _i, _vp], _i),
    "tmjx_bgemm_silu_fwd": ([_vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp] + [_i] * 4 + [_vp], _i),
    "tmjx_bgemm_silu_bwd": ([_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _vp], _i),
    "tmjx_bf_silu_bwd": ([_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp], _i),
    "tmjx_bf_silu_bwd_rank1": ([_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp], _i),
    "tmjx_chain_rows": ([_i], _i),
    "tmjx_chain_fwd_ok": ([_P(ChainFwd)], _i),
    "tmjx_chain_fwd": ([_P(ChainFwd), _vp], _i),
    "tmjx_chain_bwd_ok": ([_P(ChainBwd)], _i),
    "tmjx_chain_bwd": ([_P(ChainBwd), _vp], _i),
    "tmjx_lstm_hidden_ok": ([_i], _i),
    "tmjx_lstm_seq_fwd": ([_P(LstmFwd), _vp], _i),
    "tmjx_lstm_seq_bwd": ([_P(LstmBwd), _vp], _i),
    "tmjx_record_check": ([_P(RecordStream), _i, _i, _i], _i),
    "tmjx_record_step": ([_vp] + [_i] * 4 + [_vp], _i),
    "tmjx_latent_concat_det": ([_vp, _i, _vp, _i64, _i64, _vp, _vp, _vp, _i, _vp] + [_i] * 5 + [_vp], _i),
    "tmjx_action_mode": ([_vp, _i, _vp, _vp, _i, _i, _vp], _i),
    "tmjx_decoder_input": ([_vp, _i, _vp, _i64, _i64, _vp, _vp, _vp] + [_i] * 5 + [_vp], _i),
    "tmjx_decoder_act_ok": ([_P(DecoderAct)], _i),
    "tmjx_decoder_act": ([_P(DecoderAct), _vp], _i),
    "tmjx_lstm_decoder_act_ok": ([_P(LstmDecoderAct)], _i),
    "tmjx_lstm_decoder_act": ([_P(LstmDecoderAct), _vp], _i),
    "tmjx_policy_act_ok": ([_P(PolicyAct)], _i),
    "tmjx_policy_act": ([_P(PolicyAct), _vp], _i),
    "tmjx_sensor_info": ([_vp, _P(_i), _P(_i)], _i),
    "tmjx_physics_sensors": ([_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp], _i),
    "tmjx_step_sensors": ([_vp] * 12 + [_i, _vp], _i),
    "tmjx_set_done_policy": ([_vp, _i], _i),
    "tmjx_clips_upload_velocities": ([_vp, _vp, _vp, _i, _i], _i),
    "tmjx_set_env_scales": ([_vp, _vp, _i], _i),
    "tmjx_set_env_gravity": ([_vp, _vp, _i], _i),
    "tmjx_render_info": ([_vp, _i, _i, _P(RenderInfo)], _i),
    "tmjx_render_camera": ([_vp, _s, _P(Camera)], _i),
    "tmjx_render_pose": ([_vp, _vp, _vp, _i, _i, _P(Camera), _vp, _vp], _i),
    "tmjx_render_prims": ([_vp, _vp] + [_i] * 4 + [_vp] * 4, _i),
    "tmjx_render": ([_vp, _vp, _vp, _i, _i, _P(Camera), _i, _i] + [_vp] * 5, _i),
    "tmjx_pca_workspace": ([_i, _i, _P(_i64)], _i),
    "tmjx_pca_fit": ([_vp, _i, _i, _i64] + [_vp] * 4 + [_P(PcaInfo), _vp], _i),
    "tmjx_pca_transform": ([_vp, _i, _i, _i64, _vp, _vp, _i, _vp, _i64, _vp], _i),
    "tmjx_plot_strips": ([_vp, _i, _i, _i64, _vp, _vp, _i, _f, _f, _i, _P(StripStyle), _i, _i, _vp, _vp], _i),
    "tmjx_pca_wide_workspace": ([_i, _i, _P(_i64)], _i),
    "tmjx_pca_fit_wide": ([_vp, _i, _i, _i64] + [_vp] * 4 + [_P(PcaInfo), _vp], _i),
    "tmjx_pca_transform_wide": ([_vp, _i, _i, _i64, _vp, _vp, _i, _vp, _i64, _vp], _i),
    "tmjx_readout_workspace": ([_i] * 4 + [_P(_i64)], _i),
    "tmjx_readout_fit": ([_vp, _i, _i, _i64, _vp, _i, _i64] + [_vp] * 6 + [_P(PcaInfo), _vp], _i),
    "tmjx_readout_weights": ([_vp, _vp, _vp, _i, _i, _P(_d), _i, _vp, _vp], _i),
    "tmjx_readout_predict": ([_vp, _i, _i, _i64, _vp, _vp, _vp, _i, _vp, _i64, _vp], _i),
    "tmjx_readout_score": ([_vp, _i, _i, _i64, _vp, _i, _i64, _vp, _vp, _vp, _i] + [_vp] * 4, _i),
    "tmjx_intervene_ok": ([_P(Intervene)], _i),
    "tmjx_intervene": ([_P(Intervene), _i, _vp], _i),
    "tmjx_kmeans_workspace": ([_i, _i, _i, _P(_i64)], _i),
    "tmjx_kmeans_assign": ([_vp, _i, _i, _i64, _vp, _i] + [_vp] * 7, _i),
    "tmjx_kmeans_update": ([_vp, _i, _i, _i64, _vp, _i] + [_vp] * 4, _i),
    "tmjx_kmeans_seed": ([_vp, _i, _i, _i64, _i, _P(_d), _vp, _P(_i), _vp, _vp], _i),
    "tmjx_kmeans_fit": ([_vp, _i, _i, _i64, _i, _vp, _vp, _vp, _i, _d, _P(KMeansInfo), _vp, _vp], _i),
    "tmjx_hmm_workspace": ([_i] * 4 + [_P(_i64)], _i),
    "tmjx_hmm_emission": ([_vp, _i, _i, _i64, _vp, _vp, _i, _vp, _vp, _vp], _i),
    "tmjx_hmm_forward_backward": ([_vp, _i, _i, _P(_i), _i] + [_vp] * 9, _i),
    "tmjx_hmm_mstep": ([_vp, _i, _i, _i64, _vp, _i, _d, _d] + [_vp] * 5, _i),
    "tmjx_hmm_transitions": ([_vp, _vp, _i, _d, _d, _vp, _vp, _vp], _i),
    "tmjx_hmm_viterbi": ([_vp, _i, _i, _P(_i), _i, _vp, _vp, _i] + [_vp] * 4, _i),
    "tmjx_hmm_fit": ([_vp, _i, _i, _i64, _P(_i), _i, _i] + [_vp] * 6 + [_i] + [_d] * 5 + [_P(HmmInfo), _vp, _vp], _i),
    "tmjx_arhmm_workspace": ([_i] * 5 + [_P(_i64)], _i),
    "tmjx_arhmm_emission": ([_vp, _i, _i, _i64, _P(_i), _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp], _i),
    "tmjx_arhmm_moments": ([_vp, _i, _i, _i64, _P(_i), _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp], _i),
    "tmjx_arhmm_solve": ([_vp, _vp, _i, _i, _i, _vp, _d, _d, _d] + [_vp] * 6, _i),
    "tmjx_arhmm_fit": ([_vp, _i, _i, _i64, _P(_i), _i, _i, _i, _vp, _i] + [_vp] * 7 + [_i] + [_d] * 6 + [_P(ArhmmInfo), _vp, _vp], _i),
    "tmjx_tsne_workspace": ([_i, _i64, _i, _i, _P(_i64)], _i),
    "tmjx_knn": ([_vp, _i, _i, _i64, _vp, _i64, _i64, _i, _i, _vp, _vp, _vp, _vp], _i),
    "tmjx_tsne_affinities": ([_vp, _i64, _i, _d, _vp, _vp, _vp], _i),
    "tmjx_tsne_gradient": ([_vp, _i, _P(_i), _vp, _vp, _i64, _d, _vp, _vp, _vp, _vp, _vp], _i),
    "tmjx_tsne_update": ([_vp, _vp, _vp, _vp, _i, _f, _f, _f, _vp, _vp], _i),
    "tmjx_tsne_fit": ([_vp, _i, _P(_i), _vp, _vp, _i64, _i, _d, _i, _f, _f, _f, _f, _vp, _vp, _P(TsneInfo), _vp, _vp], _i),
    "tmjx_tsne_place": ([_vp, _vp, _i64, _i, _vp, _i, _vp, _vp], _i),
    "tmjx_compare_workspace": ([_i, _i, _i, _P(_i64)], _i),
    "tmjx_cka_linear": ([_vp, _i, _i, _i64, _vp, _i, _i64, _vp, _vp, _vp], _i),
    "tmjx_rdm_corr": ([_vp, _i, _i, _i64, _i, _vp, _i, _i64, _i, _vp, _vp, _vp], _i),
    "tmjx_cca": ([_vp, _i, _i, _i64, _vp, _i, _i64, _d, _i, _vp, _vp, _vp, _P(CcaInfo), _vp, _vp], _i),
    "tmjx_compare_svd": ([_vp, _i, _i, _i64, _vp, _vp, _vp, _P(_i), _vp, _vp], _i),
    "tmjx_jacobian_workspace": ([_P(JacobianDesc), _i, _P(_i64)], _i),
    "tmjx_decoder_jacobian": ([_P(JacobianDesc), _vp, _i, _i64, _vp, _i, _vp, _i64, _i] + [_vp] * 9, _i),
    "tmjx_lstm_jacobian_workspace": ([_P(LstmJacobianDesc), _i, _P(_i64)], _i),
    "tmjx_lstm_decoder_jacobian": ([_P(LstmJacobianDesc), _vp, _i, _i64, _vp, _vp, _i64, _vp, _i, _vp, _i64, _vp, _i] + [_vp] * 11, _i),
    "tmjx_lstm_tangent_workspace": ([_P(LstmJacobianDesc), _i, _i, _P(_i64)], _i),
    "tmjx_lstm_tangent_step": ([_P(LstmJacobianDesc), _vp, _i, _i64, _vp, _vp, _i64, _vp, _i, _vp, _vp, _vp], _i),
    "tmjx_lstm_lyapunov": ([_P(LstmJacobianDesc), _vp, _i, _i64, _vp, _vp, _i64, _P(_i), _i, _vp, _i, _i, _i] + [_vp] * 7, _i),
    "tmjx_wavelet_bank_size": ([_d, _P(_d), _i, _d, _d, _P(_i64)], _i),
    "tmjx_wavelet_bank": ([_d, _P(_d), _i, _d, _d, _vp, _P(_i), _P(_i)], _i),
    "tmjx_spectrogram_workspace": ([_i] * 4 + [_P(_i64)], _i),
    "tmjx_spectrogram": ([_vp, _i, _i, _i64, _P(_i), _i, _vp, _P(_i), _P(_i), _i, _i, _i, _f, _vp, _i64, _vp, _vp, _vp], _i),
    "tmjx_debug_rows": ([_vp, _s, _P(_i), _P(_i)], _i),
    "tmjx_last_error": ([], _s),
    "tmjx_version": ([], _s),
}
EXPORTS = tuple(SIGNATURES)

_lib = None


def include_closure(path: Path, seen: dict | None = None) -> dict:
    """{file: text} of a source and every file it includes with quotes, recursively (what a rebuild of it depends on)."""
    import re
    seen = {} if seen is None else seen
    path = Path(path).resolve()
    if path in seen or not path.exists():
        return seen
    seen[path] = text = path.read_text()
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M):
        include_closure(path.parent / inc, seen)
    return seen


def build(verbose: bool = False, out: Path | None = None, defines: tuple = ()) -> Path:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU).  `out` / `defines`: alternative builds for
    tests (-DTMJX_LANE_IMPL: with the lane-per-env cross-check kernels) and profiling (-DTMW_PROFILE)."""
    # -fno-slp-vectorize: the SLP vectoriser packs the two dof slots of the row products into v_pk_* with more v_mov shuffles than
    # it saves (measured 1.8 % on the physics kernel); the explicitly packed FMAs of the chain kernels are not affected
    out = SO_PATH if out is None else Path(out)
    # three translation units compiled side by side (each hipcc run is single-threaded per offload arch), then linked into ONE library.
    # Objects are cached next to the library, keyed by a hash of the flags and of the source with every header it includes (recursively):
    # editing one kernel family recompiles one unit
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC", "-Wno-unused-value", *[f"-D{d}" for d in defines],
             *os.environ.get("TMJX_EXTRA_HIPCC_FLAGS", "").split()]          # (tuning experiments: A/B builds with extra compiler flags)

    cache = out.parent / ".build"
    cache.mkdir(exist_ok=True)
    objs = []
    def flags_of(src):
        return [*flags, *SOURCE_FLAGS.get(src.name, ())]

    for src in SOURCES:
        h = hashlib.sha256(" ".join(flags_of(src)).encode())
        for pth, text in sorted(include_closure(src).items()):
            h.update(str(pth.name).encode()); h.update(text.encode())
        objs.append(cache / f"{src.stem}.{h.hexdigest()[:16]}.o")

    def compile_one(src, obj):
        if obj.exists():
            return
        for stale in cache.glob(f"{src.stem}.*.o"):
            if len(list(cache.glob(f"{src.stem}.*.o"))) > 6:
                stale.unlink(missing_ok=True)
        tmp = obj.with_suffix(f".tmp{os.getpid()}.o")
        cmd = ["hipcc", *flags_of(src), "-c", "-o", str(tmp), str(src)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise TmjxError(f"hipcc failed on {src.name}:\n" + res.stderr[-4000:])
        tmp.replace(obj)
        if verbose:
            print(" ".join(cmd))
    with ThreadPoolExecutor(len(SOURCES)) as ex:
        for f in [ex.submit(compile_one, s, o) for s, o in zip(SOURCES, objs)]:
            f.result()
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(out), *[str(o) for o in objs]]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise TmjxError("hipcc link failed:\n" + res.stderr[-4000:])
    # the build id: a hash of WHAT was compiled (flags + every source with its include closure, the object cache keys), written next to the
    # library.  hipcc's objects are not bit-reproducible, so a hash of the .so would change with every recompilation of unchanged sources —
    # and the counters under profiles/ are tied to a build by this id (tools/buildid.py, bench.py)
    Path(str(out) + ".id").write_text(hashlib.sha256(" ".join(o.name for o in objs).encode()).hexdigest()[:16] + "\n")
    return out


def build_id(path: Path | None = None) -> str:
    """Id of a built library: the source-derived id `build` wrote next to it, else (a library from elsewhere) the hash of its bytes."""
    import hashlib
    path = Path(SO_PATH if path is None else path)
    side = Path(str(path) + ".id")
    try:
        if side.exists() and side.stat().st_mtime >= path.stat().st_mtime - 1:
            return side.read_text().strip()
        return hashlib.sha256(path.read_bytes()).hexdigest()[:16]
    except OSError:
        return "missing"


def lib():
    global _lib
    if _lib is not None:
        return _lib
    _lib = load(SO_PATH)
    return _lib


def declare(L, names=None):
    """Give the entry points of SIGNATURES (or `names` of them) that library `L` exports their argument and return types.  A library may export a
    subset (the oracle's ABI twin has no learner kernels, the tests' host emulation only the analyses): calling a missing one raises."""
    for name in SIGNATURES if names is None else names:
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = SIGNATURES[name]
    return L


def load(path: Path):
    """dlopen a build of the library and declare its entry points (lib() = the product build; tests load the lane cross-check build)."""
    path = Path(path)
    if not path.exists():
        raise TmjxError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path.")
    try:
        L = C.CDLL(str(path))
    except OSError as e:  # e.g. no ROCm runtime on this machine
        raise TmjxError(f"cannot load {path}: {e}") from e
    declare(L)
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise TmjxError(f"{what} failed ({rc}): {lib().tmjx_last_error().decode()}")


def block_override() -> str | None:
    return os.environ.get("TMJX_BLOCK")
