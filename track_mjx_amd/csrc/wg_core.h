// csrc/wg_core.h — the discipline every analysis body is written in, so that it also compiles on the host (tests/hostemu/*_emu.cpp).  Two kinds
// of function:
//   TM_DEV  — one thread's work (a projection, a pixel of the panel): the host runs one loop iteration where the GPU has one thread;
//   PCA_WG  — one workgroup's work, written as PCA_PAR loops (one iteration per thread) between PCA_SYNC barriers.  On the GPU a PCA_PAR body runs
//             once per thread and PCA_SYNC is __syncthreads; on the host PCA_PAR is a serial loop over the thread ids and PCA_SYNC nothing, which is
//             the same computation because no PCA_PAR body reads what another iteration of the same loop writes.  State a thread keeps across
//             a barrier is declared with PCA_PRIVATE (registers on the GPU, one slot per thread id on the host).
// With them the two reductions the analyses share: the fixed tree over the workgroup's threads (wg_tree) and the ordered float64 sum (wg_sum).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef TM_DEV
#define TM_DEV __device__ __forceinline__
#endif

#define PCA_ROWS_PER_WG 256    // rows of one workgroup's partial moments: the fixed split that makes the reduction order independent of the grid
#define PCA_THREADS 256        // workgroup size of the moment, transform and panel kernels

#ifdef TM_HOST_EMU
#define PCA_WG static inline
#define PCA_PAR(tid, nt) for (int tid = 0; tid < (nt); tid++)
#define PCA_SYNC() ((void)0)
#define PCA_PRIVATE(T, name, n) T name##_all_[PCA_THREADS][n]
#define PCA_MINE(name, tid) name##_all_[tid]
#define PCA_HD static inline
#else
#define PCA_HD __host__ __device__ static inline
#define PCA_WG __device__ __forceinline__
#define PCA_PAR(tid, nt) for (int tid = threadIdx.x, once_ = 1; once_; once_ = 0)
#define PCA_SYNC() __syncthreads()
#define PCA_PRIVATE(T, name, n) T name##_all_[1][n]
#define PCA_MINE(name, tid) name##_all_[0]
#endif

// the slot of thread tid in an array declared with PCA_PRIVATE and handed to a function as a pointer
#ifdef TM_HOST_EMU
#define COMPARE_SLOT(tid) (tid)
#else
#define COMPARE_SLOT(tid) 0
#endif

PCA_HD int pca_nwg(int n) { return (n + PCA_ROWS_PER_WG - 1) / PCA_ROWS_PER_WG; }

// The K interleaved sums s_red[k * PCA_THREADS + tid] of the workgroup's threads, each in a fixed binary tree; the totals are
// s_red[k * PCA_THREADS] behind it.  The caller's barrier stands between its stores and this.
template <int K, class T>
PCA_WG void wg_tree(T *s_red) {
  for (int half = PCA_THREADS / 2; half >= 1; half >>= 1) {
    PCA_PAR(tid, PCA_THREADS) {
      if (tid < half)
#pragma unroll
        for (int k = 0; k < K; k++) s_red[k * PCA_THREADS + tid] += s_red[k * PCA_THREADS + tid + half];
    }
    PCA_SYNC();
  }
}

// `count` partials `stride` apart added in index order, in float64
template <class T>
TM_DEV double wg_sum(const T *partial, int count, int64_t stride) {
  double s = 0.0;
  for (int i = 0; i < count; i++) s += (double)partial[i * stride];
  return s;
}
