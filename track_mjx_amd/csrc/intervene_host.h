// csrc/intervene_host.h — the argument checks tmjx_intervene shares with the host emulation (tests/hostemu/intervene_emu.cpp).  An empty string:
// accepted.  Nothing is dereferenced but the descriptor itself.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "intervene_core.h"

namespace tmjx_host {

static inline bool iv_al4(const void *p) { return !((uintptr_t)p & 3); }

static inline std::string intervene_check(const tmjx_intervene_t *d) {
  if (!d) return "null descriptor";
  if (d->mode != TMJX_INTERVENE_SUBSPACE && d->mode != TMJX_INTERVENE_UNITS)
    return "unknown mode " + std::to_string(d->mode) + " (TMJX_INTERVENE_SUBSPACE = 0, TMJX_INTERVENE_UNITS = 1)";
  if (d->w < 1 || d->w > IV_MAX_W) return "w = " + std::to_string(d->w) + " outside 1 .. " + std::to_string(IV_MAX_W);
  if (d->ld < d->w) return "ld = " + std::to_string(d->ld) + " is smaller than w = " + std::to_string(d->w);
  if (d->n < 1) return "n must be >= 1 (got " + std::to_string(d->n) + ")";
  const bool sub = d->mode == TMJX_INTERVENE_SUBSPACE;
  if (sub) {
    if (d->K < 1 || d->K > IV_MAX_K) return "K = " + std::to_string(d->K) + " outside 1 .. " + std::to_string(IV_MAX_K);
    if (d->ldv < d->w) return "ldv = " + std::to_string(d->ldv) + " is smaller than w = " + std::to_string(d->w);
    if (d->proj && d->ldp < d->K) return "ldp = " + std::to_string(d->ldp) + " is smaller than K = " + std::to_string(d->K);
  } else if (d->proj) {
    return "proj is given in units mode (projections exist in subspace mode only)";
  }
  if (!d->h || !d->gain || !d->offset || !d->dose || !d->t_on || !d->t_off || (sub && !d->dirs)) return "null argument";
  if (!iv_al4(d->h) || !iv_al4(d->dirs) || !iv_al4(d->center) || !iv_al4(d->gain) || !iv_al4(d->offset) || !iv_al4(d->dose) || !iv_al4(d->t_on) ||
      !iv_al4(d->t_off) || !iv_al4(d->proj))
    return "every pointer must be 4-byte aligned";
  return "";
}

}  // namespace tmjx_host
