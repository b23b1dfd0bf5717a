// g2k_modes.hip — fused k-means reduction of a probabilistic head's samples to
// M modes and the scores of the M centres.  ONE kernel,
// sample_modes_kernel<Head>, instantiated for the per-step head
// (g2k_sample_modes_f32), the full-covariance head
// (g2k_fullcov_sample_modes_f32) and the mixture head
// (g2k_mix_sample_modes_f32); the heads are the policies of g2k_head_draw.h.
// The C entry points are at the end of this file, declared in
// include/g2k_modes.h (added after ABI 11: bound by symbol), which holds the
// definition.  The build's: the reference has no probabilistic head, so PARITY
// UNPINNED; pinned against tests/modes_ref.py.
//
// Everything after the draw is double precision (the definition's: Lloyd's
// argmin is not reproducible in f32).  The draws themselves stay f32 in LDS,
// as in g2k_scores.hip, and are widened where they are used.
//
// Geometry and pass scaffold: the drawn-once family's (g2k_drawn.h), with a
// cap of its own on the pairs of a pass, G = min(256 / K, 64 / M, 32)
// (modes_max_g below): the M centres of every pair of the pass are in
// LDS as doubles, cen[G * M][24] (12 KB at G M = 64, which with the draws'
// 24 KB and the mixture head's 19 KB stays below 64 KB: two workgroups per
// CU), and a lane per pair finishes (32).  Per pass:
//   draw     the lane draws X_k and stores it in its slot           1 barrier
//   start    the G M 24 centre coordinates, dealt to the lanes, are copied
//            from the first M slots of their pair                   1 barrier
//   iters x  assign: the lane keeps X_k in registers and walks its pair's M
//            centres (ds_read_b128 of two doubles: a broadcast within the
//            pair's lanes), the lowest m of the smallest d2 goes to asg[tid]
//            update: item (pair, m, j) walks the pair's K slots in k order,
//            adds X_k[j] where asg = m, counts, divides       2 barriers each
//   final    one more assign, which also keeps d2 of the lane's own centre
//   items    (pair, m): n_m and the centre's A_m, F_m against the target;
//            (pair): the inertia, the K lanes' d2 in k order        1 barrier
//   finish   lane tid < G takes pair tid: the two argmins, per_ped and the
//            lane's eight double sums; all lanes write the pass's centres and
//            weights, pair index fastest (adjacent lanes, adjacent n)
// Control flow is uniform: there is no convergence test.
// Scene sums: every finishing lane's eight doubles go to LDS at the end, eight
// lanes add the 32 rows in lane order; per-workgroup rows [S * C][8] of doubles
// in the caller's workspace, then drawn_rows8_kernel adds a scene's C rows in
// chunk order and rounds once; C == 1 rounds and writes out directly.
#include <math.h>

#include "g2k_drawn.h"

namespace g2k {
namespace {

constexpr int kMoThreads = kDrThreads, kMoMaxG = kDrMaxG, kMoPitch = kDrPitch;
constexpr int kMoMaxGM = 64;                  // centres per pass: the LDS budget
// xy, cen, dmin, stat {A, F}, cnt, asg, iner, sums
constexpr int kMoLdsBytes = kMoThreads * kMoPitch * 4 + kMoMaxGM * kL2 * 8 + kMoThreads * 8 +
                            kMoMaxGM * 2 * 8 + kMoMaxGM * 4 + kMoThreads + kMoMaxG * 8 +
                            kMoMaxG * 8 * 8;

// drawn_geom's cap: the pass's G M centres fit
inline int modes_max_g(int M) { return kMoMaxGM / M < kMoMaxG ? kMoMaxGM / M : kMoMaxG; }

// the lane's draw against its pair's M centres: the lowest m of the smallest
// d2 (j ascending), and that d2
__device__ __forceinline__ int assign_lane(const float (&x)[kL2], const double* __restrict__ c, int M,
                                           double& best) {
  int a = 0;
  best = 0.0;
#pragma nounroll
  for (int m = 0; m < M; ++m) {
    const double2* c2 = reinterpret_cast<const double2*>(c + m * kL2);
    double d2 = 0.0;
#pragma unroll
    for (int q = 0; q < kL2 / 2; ++q) {
      const double2 v = c2[q];
      const double e0 = (double)x[2 * q] - v.x, e1 = (double)x[2 * q + 1] - v.y;
      d2 += e0 * e0;
      d2 += e1 * e1;
    }
    if (m == 0 || d2 < best) { best = d2; a = m; }
  }
  return a;
}

template <class Head>
__global__ void __launch_bounds__(kMoThreads) sample_modes_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int FC, int C, int G, int K, int M, int iters, uint32_t seed_lo, uint32_t seed_hi,
    int shared_targets, double miss_radius, float* __restrict__ per_ped, float* __restrict__ centres,
    float* __restrict__ weights, float* __restrict__ out, double* __restrict__ rows) {
  __shared__ typename Head::Lds hlds;
  __shared__ __attribute__((aligned(16))) float xy[kMoThreads * kMoPitch];
  __shared__ __attribute__((aligned(16))) double cen[kMoMaxGM * kL2];
  __shared__ double dmin[kMoThreads];
  __shared__ double statA[kMoMaxGM], statF[kMoMaxGM];
  __shared__ int cnt[kMoMaxGM];
  __shared__ uint8_t asg[kMoThreads];
  __shared__ double iner[kMoMaxG];
  __shared__ double sums[kMoMaxG][8];
  const int tid = threadIdx.x;
  const DrawnChunk ch = drawn_chunk(n_active, n_frames, ped_mask, F, Nmax, FC, C);
  const int s = ch.s, f0 = ch.f0, fcn = ch.fcn, nact = ch.nact;
  const uint8_t* mask = ch.mask;

  Head::template stage<kMoThreads>(head_params, hlds, tid);
  // non-pairs: zeros in per_ped, centres and weights (one loop over the three,
  // so not drawn_zero_per_ped)
  if (per_ped || centres || weights) {
    const int rows_c = centres ? M * kL2 : 0, rows_w = weights ? M : 0, rows_p = per_ped ? 1 : 0;
    const int nrows = rows_c + rows_w + rows_p;
    for (int idx = tid; idx < fcn * nrows * Nmax; idx += kMoThreads) {
      const int n = idx % Nmax;
      const int r = (idx / Nmax) % nrows, fl = idx / (Nmax * nrows);
      if (drawn_is_pair(ch, fl, n)) continue;
      const size_t sf = drawn_frame(ch, fl);
      if (r < rows_c) {
        centres[(sf * M * kL2 + r) * Nmax + n] = 0.f;
      } else if (r < rows_c + rows_w) {
        weights[(sf * M + (r - rows_c)) * Nmax + n] = 0.f;
      } else {
        float4* o = reinterpret_cast<float4*>(per_ped) + (sf * Nmax + n) * 2;
        o[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
  __syncthreads();
  Head head;
  head.bind(hlds);

  const DrawnLane ln = drawn_lane(tid, K, seed_lo, seed_hi);
  const int npairs = drawn_npairs(ch);
  const int g = ln.g;
  const double dK = (double)K;                             // w_m = n_m / K, the inertia = sum / K: divided, as defined
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0;
#pragma nounroll
  for (int base = 0; base < npairs; base += G) {           // uniform trip count
    // ---- draw ----
    const DrawnItem it = drawn_item(ch, base, G, g);
    const int gp = it.gp;
    const bool valid = it.valid, on = it.on;
    float x[kL2];
    if (on) {
      const size_t sf = drawn_frame(ch, it.fl);
      const int64_t e0 = drawn_elem0(ch, sf, it.n);        // element of step 0
      float mu[kL2], tg[kL2];
      load_mu_tg(true, pred, targets, sf, shared_targets ? (size_t)s : sf, it.n, Nmax, mu, tg);
      head.draw(ln.lo, ln.hi, e0, it.n, Nmax, mu, [&](int t, float px, float py) {
        x[2 * t] = px;
        x[2 * t + 1] = py;
      });
      store_draw(xy + tid * kMoPitch, x);
    } else {
      zero_draw(x);
    }
    __syncthreads();
    // ---- start: c_m = X_m ----
    const int ncoord = gp * M * kL2;
    for (int idx = tid; idx < ncoord; idx += kMoThreads) {
      const int gm = idx / kL2, j = idx - gm * kL2;
      const int gi = gm / M, m = gm - gi * M;
      const int pp = base + gi;
      const int n2 = pp % nact;
      double v = 0.0;
      if (mask ? mask[n2] != 0 : true) v = (double)xy[(gi * K + m) * kMoPitch + j];
      cen[idx] = v;
    }
    __syncthreads();
    // ---- Lloyd ----
    const double* mine = cen + (valid ? g : 0) * M * kL2;
    double best = 0.0;
#pragma nounroll
    for (int it = 0; it < iters; ++it) {
      if (on) asg[tid] = (uint8_t)assign_lane(x, mine, M, best);
      __syncthreads();
      for (int idx = tid; idx < ncoord; idx += kMoThreads) {
        const int gm = idx / kL2, j = idx - gm * kL2;
        const int gi = gm / M, m = gm - gi * M;
        const int pp = base + gi;
        const int n2 = pp % nact;
        if (mask ? mask[n2] != 0 : true) {
          const int slot0 = gi * K;
          double sum = 0.0;
          int nm = 0;
          // both reads unconditional and the term selected (adding 0.0 leaves the
          // sum as it is): no branch in the walk, the reads of several slots in flight
#pragma unroll 8
          for (int kk = 0; kk < K; ++kk) {
            const bool in = asg[slot0 + kk] == m;
            const double v = (double)xy[(slot0 + kk) * kMoPitch + j];
            sum += in ? v : 0.0;
            nm += in ? 1 : 0;
          }
          if (nm > 0) cen[idx] = sum / (double)nm;       // an empty cluster keeps its centre
        }
      }
      __syncthreads();
    }
    // ---- final assignment ----
    if (on) {
      asg[tid] = (uint8_t)assign_lane(x, mine, M, best);
      dmin[tid] = best;
    }
    __syncthreads();
    // ---- items: (pair, m) and (pair) ----
    for (int idx = tid; idx < gp * (M + 1); idx += kMoThreads) {
      const int gi = idx / (M + 1), m = idx - gi * (M + 1);
      const int pp = base + gi;
      const int fl2 = pp / nact, n2 = pp - fl2 * nact;
      if (mask ? mask[n2] != 0 : true) {
        const int slot0 = gi * K;
        if (m < M) {
          int nm = 0;
#pragma nounroll
          for (int kk = 0; kk < K; ++kk) nm += asg[slot0 + kk] == m ? 1 : 0;
          const size_t tf2 = shared_targets ? (size_t)s : (size_t)s * F + f0 + fl2;
          const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf2 * Nmax + n2) * kL;
          const double* cm = cen + (gi * M + m) * kL2;
          double a = 0.0, f = 0.0;
#pragma unroll
          for (int t = 0; t < kL; ++t) {
            const float2 y = t2[t];
            const double dx = cm[2 * t] - (double)y.x, dy = cm[2 * t + 1] - (double)y.y;
            f = sqrt(dx * dx + dy * dy);
            a += f;
          }
          statA[gi * M + m] = a / 12.0;
          statF[gi * M + m] = f;
          cnt[gi * M + m] = nm;
        } else {
          double sum = 0.0;
#pragma nounroll
          for (int kk = 0; kk < K; ++kk) sum += dmin[slot0 + kk];
          iner[gi] = sum / dK;
        }
      }
    }
    __syncthreads();
    // ---- finish: lane tid < gp takes pair base + tid
    if (tid < gp) {
      const int pp = base + tid;
      const int fl3 = pp / nact, n3 = pp - fl3 * nact;
      if (mask ? mask[n3] != 0 : true) {
        double cA = statA[tid * M], cF = statF[tid * M];
        int mA = 0, mF = 0, live = 0;
#pragma nounroll
        for (int m = 0; m < M; ++m) {
          const double a = statA[tid * M + m], f = statF[tid * M + m];
          if (a < cA) { cA = a; mA = m; }
          if (f < cF) { cF = f; mF = m; }
          live += cnt[tid * M + m] > 0 ? 1 : 0;
        }
        const double wA = (double)cnt[tid * M + mA] / dK, wF = (double)cnt[tid * M + mF] / dK;
        const double in = iner[tid];
        if (per_ped) {
          const size_t sf = (size_t)s * F + f0 + fl3;
          float4* o = reinterpret_cast<float4*>(per_ped) + (sf * Nmax + n3) * 2;
          o[0] = make_float4((float)cA, (float)cF, (float)mA, (float)mF);
          o[1] = make_float4((float)wA, (float)wF, (float)in, (float)live);
        }
        acc[0] += cA;
        acc[1] += cF;
        acc[2] += (1.0 - wA) * (1.0 - wA);
        acc[3] += (1.0 - wF) * (1.0 - wF);
        acc[4] += cF > miss_radius ? 1.0 : 0.0;
        acc[5] += in;
        acc[6] += (double)live;
        acc[7] += 1.0;
      }
    }
    // the pass's centres and weights: pair index fastest
    if (centres) {
      for (int idx = tid; idx < ncoord; idx += kMoThreads) {
        const int gi = idx % gp, r = idx / gp;             // r = m * 24 + row
        const int m = r / kL2, row = r - m * kL2;
        const int pp = base + gi;
        const int fl4 = pp / nact, n4 = pp - fl4 * nact;
        if (mask ? mask[n4] != 0 : true) {
          const size_t sf = (size_t)s * F + f0 + fl4;
          const int j = row < kL ? 2 * row : 2 * (row - kL) + 1;   // pred's rows: x then y
          centres[((sf * M + m) * kL2 + row) * Nmax + n4] = (float)cen[(gi * M + m) * kL2 + j];
        }
      }
    }
    if (weights) {
      for (int idx = tid; idx < gp * M; idx += kMoThreads) {
        const int gi = idx % gp, m = idx / gp;
        const int pp = base + gi;
        const int fl4 = pp / nact, n4 = pp - fl4 * nact;
        if (mask ? mask[n4] != 0 : true) {
          const size_t sf = (size_t)s * F + f0 + fl4;
          weights[(sf * M + m) * Nmax + n4] = (float)((double)cnt[gi * M + m] / dK);
        }
      }
    }
    // no barrier here: the next pass's draw writes xy, which no lane reads past
    // the items' barrier; cen, cnt and the statistics are next written behind
    // the next pass's first barrier
  }
  // the workgroup's row: the finishing lanes' sums in lane order
  if (tid < kMoMaxG) {
#pragma unroll
    for (int i = 0; i < 8; ++i) sums[tid][i] = acc[i];
  }
  __syncthreads();
  if (tid < 8) {
    double v = 0.0;
#pragma nounroll
    for (int l = 0; l < kMoMaxG; ++l) v += sums[l][tid];
    if (rows) rows[(size_t)blockIdx.x * 8 + tid] = v;
    else out[(size_t)blockIdx.x * 8 + tid] = (float)v;
  }
}

template <class Head>
int sample_modes_launch(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* head_params, uint64_t seed, int K, int M, int iters,
                        float miss_radius, float* per_ped, float* centres, float* weights, float* out,
                        double* rows, hipStream_t st) {
  DrawnLaunch L;
  if (const int rc = drawn_launch(d, drawn_geom(*d, K, modes_max_g(M)), seed, Head::kPrefix,
                                  "sample_modes", L))
    return rc;
  const DrawnGeom& g = L.g;
  hipLaunchKernelGGL(sample_modes_kernel<Head>, dim3((unsigned)L.wgs), dim3(kMoThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.FC, g.C, g.G,
                     K, M, iters, L.seed_lo, L.seed_hi, L.shared_targets, (double)miss_radius, per_ped,
                     centres, weights, out, L.direct ? (double*)nullptr : rows);
  const int rc = check_launch("sample_modes_kernel");
  if (rc || L.direct) return rc;
  return drawn_rows8(rows, d->S, g.C, out, st);
}

// one row [8] of doubles per (scene, chunk); FC >= 1 frame per chunk, so at most F chunks
int64_t modes_ws_bytes(const g2k_dims* d) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * 8 * 8;
}

int modes_params_ok(int32_t K, int32_t M) {
  if (M < 1 || M > G2K_MODES_MMAX) return set_err(G2K_EINVAL, "M=%d (1..%d)", M, G2K_MODES_MMAX);
  if (K < M || K > G2K_MODES_KMAX)
    return set_err(G2K_EINVAL, "K=%d (M=%d..%d)", K, M, G2K_MODES_KMAX);
  return G2K_OK;
}

// the argument checks, before any HIP call; G2K_OK with S > 0: launch
int modes_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                   const void* n_active, const void* head, int32_t K, int32_t M, int32_t iters,
                   float miss_radius, const void* per_ped, const void* out, const void* workspace,
                   int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "%s: flags %d (0 or G2K_STEP_TARGETS_SHARED)", name, d->flags);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = modes_params_ok(K, M)) return rc;
  if (iters < 0 || iters > G2K_MODES_ITERS_MAX)
    return set_err(G2K_EINVAL, "iters=%d (0..%d)", iters, G2K_MODES_ITERS_MAX);
  if (!(miss_radius >= 0.f) || !isfinite(miss_radius))
    return set_err(G2K_EINVAL, "miss_radius=%g (finite, >= 0)", (double)miss_radius);
  if (const int rc = check_required({pred, targets, n_active, head, out})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_per_ped(per_ped)) return rc;
  return check_workspace(d, workspace, workspace_bytes, modes_ws_bytes(d), 8);   // rows of doubles
}

template <class Head>
int sample_modes(const char* name, const g2k_dims* d, const float* pred, const float* targets,
                 const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                 const float* head, uint64_t seed, int32_t K, int32_t M, int32_t iters,
                 float miss_radius, float* per_ped, float* centres, float* weights, float* out,
                 void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = modes_validate(name, d, pred, targets, n_active, head, K, M, iters, miss_radius,
                                per_ped, out, workspace, workspace_bytes);
  if (rc || d->S == 0) return rc;
  return sample_modes_launch<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K, M,
                                   iters, miss_radius, per_ped, centres, weights, out,
                                   static_cast<double*>(workspace), (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

int64_t g2k_sample_modes_workspace_bytes(const g2k_dims* d) {
  if (!d || !pair_sizes_ok(d)) return -1;
  return modes_ws_bytes(d);
}

// the launch geometry (drawn_geom: host arithmetic, no HIP call), as the
// launcher works it out
int g2k_sample_modes_geometry(const g2k_dims* d, int32_t K, int32_t M, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = modes_params_ok(K, M)) return rc;
  return drawn_write_geom(drawn_geom(*d, K, modes_max_g(M)), K, kMoLdsBytes, out);
}

int g2k_sample_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames,
                         const uint8_t* ped_mask, const float* head, uint64_t seed, int32_t K,
                         int32_t M, int32_t iters, float miss_radius, float* per_ped,
                         float* centres, float* weights, float* out, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  return sample_modes<PerStepHead>("sample_modes", d, pred, targets, n_active, n_frames, ped_mask,
                                   head, seed, K, M, iters, miss_radius, per_ped, centres, weights,
                                   out, workspace, workspace_bytes, stream);
}

int g2k_fullcov_sample_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                                 const int32_t* n_active, const int32_t* n_frames,
                                 const uint8_t* ped_mask, const float* chol, uint64_t seed,
                                 int32_t K, int32_t M, int32_t iters, float miss_radius,
                                 float* per_ped, float* centres, float* weights, float* out,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  return sample_modes<FullCovHead>("fullcov_sample_modes", d, pred, targets, n_active, n_frames,
                                   ped_mask, chol, seed, K, M, iters, miss_radius, per_ped, centres,
                                   weights, out, workspace, workspace_bytes, stream);
}

int g2k_mix_sample_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                             const int32_t* n_active, const int32_t* n_frames,
                             const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                             int32_t M, int32_t iters, float miss_radius, float* per_ped,
                             float* centres, float* weights, float* out, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  return sample_modes<MixHead>("mix_sample_modes", d, pred, targets, n_active, n_frames, ped_mask,
                               mix, seed, K, M, iters, miss_radius, per_ped, centres, weights, out,
                               workspace, workspace_bytes, stream);
}

}  // extern "C"
