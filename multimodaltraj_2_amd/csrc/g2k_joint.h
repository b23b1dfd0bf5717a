// g2k_joint.h — what the joint best-of-K kernels of the two heads share
// (g2k_joint.hip: the per-step head, and the definition; g2k_fullcov_joint.hip:
// the full-covariance head): the unit geometry, the unit row format and the
// four-wave pair pass.  One copy, so that the two agree on KD, on the rows
// that g2k_joint_rows_kernel merges and on every collision count.
#pragma once
#include "g2k_common.h"

namespace g2k {
namespace {

constexpr int kJtMaxDeal = 8;        // units per scene-frame at most
constexpr int kJtRow = 10;           // int32 words per unit row
constexpr int kJtTileJ = 32;         // columns (j) per pair-pass tile
constexpr int kJtWaves = 4;          // waves of a unit when Nmax > 64

struct JointGeom { int waves, KD; };

int joint_kd_max(const g2k_dims& d) {
  const int64_t sf = (int64_t)d.S * d.F;
  const int64_t fill = d.Nmax <= 64 ? 2048 : 512;      // waves / workgroups that fill 256 CUs
  int64_t kd = sf > 0 ? (fill + sf - 1) / sf : 1;
  if (kd > kJtMaxDeal) kd = kJtMaxDeal;
  return (int)kd;
}

JointGeom joint_geom(const g2k_dims& d, int K) {
  JointGeom g;
  g.waves = d.Nmax <= 64 ? 1 : kJtWaves;
  g.KD = joint_kd_max(d);
  const int two = (K + 1) / 2;                          // >= 2 draws per unit (K = 1: one unit)
  if (g.KD > two) g.KD = two;
  return g;
}

__device__ __forceinline__ float sgpr_f(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Collisions of the LDS sample `buf` (xy[i][24], P members) among this wave's
// tiles: tile (b, c) = rows 64 b .. 64 b + 63 x columns 32 c .. 32 c + 31,
// c >= 2 b (the upper triangle), tile number % kJtWaves == w.
__device__ __forceinline__ int pair_pass(const float4* __restrict__ buf, int P, int w, int lane,
                                         float r2) {
  const int NB = (P + 63) >> 6, NC = (P + kJtTileJ - 1) / kJtTileJ;
  int cnt = 0, tix = 0;
  for (int b = 0; b < NB; ++b) {
    bool loaded = false;
    float xi[kL], yi[kL];
    const int i = (b << 6) + lane;
    for (int c = 2 * b; c < NC; ++c, ++tix) {
      if ((tix & (kJtWaves - 1)) != w) continue;
      if (!loaded) {                                      // this row block's coordinates
        const float4* pi = buf + (size_t)min(i, P - 1) * 6;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 a = pi[q], bq = pi[3 + q];
          xi[4 * q] = a.x; xi[4 * q + 1] = a.y; xi[4 * q + 2] = a.z; xi[4 * q + 3] = a.w;
          yi[4 * q] = bq.x; yi[4 * q + 1] = bq.y; yi[4 * q + 2] = bq.z; yi[4 * q + 3] = bq.w;
        }
        loaded = true;
      }
      const int j0 = max(c * kJtTileJ, (b << 6) + 1), j1 = min((c + 1) * kJtTileJ, P);
      for (int j = j0; j < j1; ++j) {                     // uniform: every lane reads member j
        const float4* pj = buf + (size_t)j * 6;
        float m = __builtin_inff();
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 a = pj[q], bq = pj[3 + q];
          const float xj[4] = {a.x, a.y, a.z, a.w}, yj[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float dx = xi[4 * q + u] - xj[u], dy = yi[4 * q + u] - yj[u];
            m = fminf(m, fmaf(dx, dx, dy * dy));
          }
        }
        cnt += (i < j && m < r2) ? 1 : 0;                 // rows >= P: i < j never holds
      }
    }
  }
  return cnt;
}

}  // namespace
}  // namespace g2k
