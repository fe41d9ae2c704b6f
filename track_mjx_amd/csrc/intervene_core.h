// csrc/intervene_core.h — the arithmetic of the activation intervention (DESIGN.md "Interventions"; include/tmjx.h: tmjx_intervene): an in-place
// linear edit of the columns [0, w) of the rows h [n][ld] between two launches of a policy step.  Every expression here compiles on the device
// (csrc/tmjx_intervene.hip) and on the host (tests/hostemu/intervene_emu.cpp).  Every product that is added to something is an explicit fmaf and
// no other product stands next to an addition, so neither compiler has anything left to contract: the two give the same bits.
//
// One wave owns a row.  Lane l holds the columns j = l + 64 i (i = 0 .. 15, masked by j < w) in registers; a dot product is the lane's partial
// sum over its columns in ascending i, then the butterfly of iv_tree_step over the lane distances 32, 16, 8, 4, 2, 1 (a + b is commutative, so both
// partners of a pair hold the same bits after every step and every lane ends with the same sum).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IV_HD __host__ __device__ static inline
#else
#define IV_HD static inline
#endif

#define IV_LANES 64
#define IV_PER_LANE 16           // columns of a row per lane: w <= IV_LANES * IV_PER_LANE
#define IV_MAX_W 1024
#define IV_MAX_K 16
#define IV_ROWS_PER_WG 4         // waves of a workgroup, one row each (they share nothing)

// A row is ON at step t when t_on <= t < t_off and its dose is not zero.  An OFF row is never stored to.
IV_HD bool iv_on(int t, int t_on, int t_off, float dose) { return t_on <= t && t < t_off && dose != 0.f; }

// The centred value of column j (center: nullable, null = 0).
IV_HD float iv_centred(float h, const float *center, int j) { return h - (center ? center[j] : 0.f); }

// One term of a lane's partial dot product, taken in ascending i.
IV_HD float iv_dot_term(float xc, float v, float acc) { return fmaf(xc, v, acc); }

// One step of the cross-lane tree: mine + the partner's (the lane at distance `off`, lane ^ off).
IV_HD float iv_tree_step(float mine, float partner) { return mine + partner; }

// The coefficient of direction k in the edit: (g - 1) p + o.
IV_HD float iv_coef(float g, float p, float o) { return fmaf(g - 1.f, p, o); }

// One term of e_j = sum_k coef_k v_kj, taken in ascending k.
IV_HD float iv_edit_term(float coef, float v, float e) { return fmaf(coef, v, e); }

// h' = h + dose e.
IV_HD float iv_apply(float h, float dose, float e) { return fmaf(dose, e, h); }

// Units mode: h' = h + dose ((g - 1)(h - c) + o).
IV_HD float iv_unit(float h, float xc, float g, float o, float dose) { return fmaf(dose, fmaf(g - 1.f, xc, o), h); }
