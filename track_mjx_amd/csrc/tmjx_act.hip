// csrc/tmjx_act.hip — translation unit of libtmjx_hip.so: the acting policy as one small-footprint launch (csrc/policy_act.h) and its C-ABI entry
// points (include/tmjx.h "tmjx_policy_act").  Compiled next to the other units (track_mjx_amd/hip.py:build) and linked into the same library.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "policy_act.h"

static bool rows16(const void *p, long long ld) { return al16(p) && !(ld & 3); }

static_assert(PA_MAX_BLOCKS == TMJX_CHAIN_MAX_HIDDEN, "tmjx_policy_act_t: block arrays");
static_assert(sizeof(tmjx_policy_act_t) == 520, "tmjx_policy_act_t: the layout hip.PolicyAct declares");
static const char *policy_act_why(const tmjx_policy_act_t *c) {
  if (!c || !c->obs || !c->W2 || !c->Wh || !c->fc2 || !c->logits || !c->raw || !c->action_t || !c->logp) return "null argument (obs / W2 / Wh / outputs)";
  if (c->n < 1 || c->Z < 1 || c->A < 1 || c->ref_w < 1 || c->obs_w < c->ref_w) return "n, Z, A, ref_w >= 1 and obs_w >= ref_w";
  if (c->n_enc < 1 || c->n_enc > TMJX_CHAIN_MAX_HIDDEN || c->n_dec < 1 || c->n_dec > TMJX_CHAIN_MAX_HIDDEN) return "1 .. 4 blocks per stack";
  if (2 * (long long)c->Z > PA_H || 2 * (long long)c->A > PA_H) return "2 Z <= 256 and 2 A <= 256";
  const long long Wd = (long long)c->Z + c->obs_w - c->ref_w, Kd = (Wd + 3) & ~3ll;
  if (Wd > PA_W) return "Z + obs_w - ref_w <= 288";
  if ((c->K0 & 3) || c->K0 != ((c->ref_w + 3) & ~3)) return "K0: the first layer's row length = ref_w rounded up to a multiple of 4";
  if (!rows16(c->obs, c->ldo) || c->ldo < c->obs_w || c->ldo < c->K0) return "the observation's rows must be row-major, 16-byte aligned, ldo >= obs_w and K0";
  if (!c->mean != !c->inv_std || !al16(c->mean) || !al16(c->inv_std)) return "mean and inv_std together, 16-byte aligned";
  if (!c->nmean != !c->nstd || !al4(c->nmean) || !al4(c->nstd)) return "nmean and nstd together";
  for (int s = 0; s < 2; s++)
    for (int l = 0; l < (s ? c->n_dec : c->n_enc); l++) {
      const tmjx_decoder_block_t &h = s ? c->dec[l] : c->enc[l];
      if (h.width != PA_H) return "every block is 256 wide";
      if (!h.W || !h.bias || !h.gamma || !h.beta) return "null block argument";
      if (!rows16(h.W, h.ldw) || !al16(h.bias) || !al16(h.gamma) || !al16(h.beta)) return "block operands must be 16-byte aligned";
      const long long K = l ? PA_H : (s ? Kd : c->K0);
      if (h.ldw < K) return "block ldw: at least the input width rounded up to 4";
      if (h.ldw > PA_MAX_LD) return "block ldw: at most 1048576 (weight rows are addressed with 32-bit byte offsets)";
    }
  if (!rows16(c->W2, c->ldw2) || c->ldw2 < PA_H || !rows16(c->Wh, c->ldwh) || c->ldwh < PA_H) return "fc2 / head weight rows must be 16-byte aligned with ld >= 256";
  if (c->ldw2 > PA_MAX_LD || c->ldwh > PA_MAX_LD) return "fc2 / head ld: at most 1048576 (weight rows are addressed with 32-bit byte offsets)";
  if (!c->eps != !c->noise) return "eps and noise together (the caller's draws), or neither (the device stream)";
  if (!c->eps && !c->rng_state) return "eps == noise == NULL needs rng_state";
  if (!al4(c->b2) || !al4(c->bh) || !al4(c->eps) || !al4(c->noise) || ((uintptr_t)c->rng_state & 7) || !al4(c->fc2) || !al4(c->logits) || !al4(c->raw) ||
      !al4(c->action_t) || !al4(c->logp)) return "float pointers must be 4-byte aligned (rng_state 8-byte)";
  return nullptr;
}

extern "C" {
int tmjx_policy_act_ok(const tmjx_policy_act_t *c) { return policy_act_why(c) == nullptr; }
int tmjx_policy_act(const tmjx_policy_act_t *c, void *stream) {
  if (const char *why = policy_act_why(c)) return fail(TMJX_EINVAL, std::string("tmjx_policy_act: ") + why);
  PolicyAct P{};
  P.obs = c->obs; P.ldo = c->ldo; P.mean = c->mean; P.inv_std = c->inv_std; P.nmean = c->nmean; P.nstd = c->nstd;
  P.M = c->n; P.K0 = c->K0; P.Z = c->Z; P.obs_w = c->obs_w; P.ref_w = c->ref_w; P.A = c->A; P.ne = c->n_enc; P.nd = c->n_dec;
  for (int l = 0; l < c->n_enc; l++) P.enc[l] = PolicyActBlock{c->enc[l].W, c->enc[l].bias, c->enc[l].gamma, c->enc[l].beta, c->enc[l].ldw};
  for (int l = 0; l < c->n_dec; l++) P.dec[l] = PolicyActBlock{c->dec[l].W, c->dec[l].bias, c->dec[l].gamma, c->dec[l].beta, c->dec[l].ldw};
  P.W2 = c->W2; P.b2 = c->b2; P.ldw2 = c->ldw2; P.Wh = c->Wh; P.bh = c->bh; P.ldwh = c->ldwh; P.ln_eps = c->ln_eps;
  P.eps = c->eps; P.noise = c->noise; P.seed = c->seed; P.rng_state = c->eps ? nullptr : (long long *)c->rng_state;
  P.fc2 = c->fc2; P.logits = c->logits; P.raw = c->raw; P.action_t = c->action_t; P.logp = c->logp;
  hipLaunchKernelGGL(k_policy_act, dim3((c->n + PA_ROWS - 1) / PA_ROWS), dim3(256), 0, (hipStream_t)stream, P);
  return check_launch("k_policy_act");
}
}  // extern "C"
