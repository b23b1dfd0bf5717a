// g2k_fullcov_draw.h — the full-covariance head's draw (g2k_fullcov.hip holds
// the definition): one copy for the sampler, the fused best-of-K
// (g2k_fullcov.hip) and the joint best-of-K (g2k_fullcov_joint.hip), so that
// the three agree bit for bit.
#pragma once
#include "g2k_common.h"

namespace g2k {
namespace {

// Lt (LDS) = the factor transposed: Lt[j * 24 + i] = L[i][j], j <= i (entries
// above the diagonal are not read from memory)
__device__ __forceinline__ void fullcov_load_lt(const float* __restrict__ chol, float* Lt, int tid,
                                                int nthreads) {
  for (int idx = tid; idx < kL2 * kL2; idx += nthreads) {
    const int i = idx / kL2, j = idx - i * kL2;
    float v = 0.f;
    if (j <= i) v = chol[idx];
    Lt[j * kL2 + i] = v;
  }
}

// step t of a draw: column 2t's terms into the rows >= 2t, then column 2t+1's
// into the rows >= 2t+1; a[2t], a[2t+1] are final afterwards (t a constant
// after unrolling: every index is one)
__device__ __forceinline__ void fullcov_advance(const float* Lt, int t, float z0, float z1,
                                                float (&a)[kL2]) {
  // a step's columns are read when the step is reached: the compiler may not
  // gather the 300 reads of a draw ahead of the draw loop
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < kL2; ++i)
    if (i >= 2 * t) a[i] = fmaf(Lt[(2 * t) * kL2 + i], z0, a[i]);
#pragma unroll
  for (int i = 0; i < kL2; ++i)
    if (i >= 2 * t + 1) a[i] = fmaf(Lt[(2 * t + 1) * kL2 + i], z1, a[i]);
}

}  // namespace
}  // namespace g2k
