// g2k_bestk.hip — fused best-of-K sampling evaluation (minADE_K / minFDE_K)
// of a probabilistic head: ONE kernel, best_of_k_kernel<Head>, instantiated
// for the per-step bivariate-Gaussian head (g2k_best_of_k_f32), for the
// full-covariance trajectory head (g2k_fullcov_best_of_k_f32) and for the
// Gaussian-mixture head (g2k_mix_best_of_k_f32, include/g2k_mix.h); the heads
// are the policies of g2k_head_draw.h.  The C entry points, their validator
// and g2k_best_of_k_geometry are at the end of this file.  The build's: the
// reference has no probabilistic head, so PARITY UNPINNED; tests/bestk_ref.py
// restates the definition over oracle/g2k_ref.py gauss_sample,
// tests/fullcov_ref.py the full-covariance draw.
//
// Definition.  Inputs as g2k_nll_f32: pred [S, F, 2L, Nmax] (band layout),
// targets [S, F, Nmax, L, 2] ([S, 1, Nmax, L, 2] with G2K_STEP_TARGETS_SHARED),
// n_active [S], n_frames [S] or NULL, ped_mask [S, Nmax] or NULL, the head's
// parameters (head [3, 12] or chol [24, 24]), seed (uint64), K in [1, 4096].
// A pair is (s, f, n) with f < n_frames[s], n < n_active[s], ped_mask[s][n] !=
// 0 (the pairs of the a9 errors and of both train losses).
//   draw k (k = 0..K-1) = what the head's sampler (g2k_gauss_sample_f32,
//     g2k_fullcov_sample_f32) writes for seed (seed + k) mod 2^64: element
//     e = ((s F + f) 12 + t) Nmax + n through the sampler's own code
//   ADE_k(s,f,n) = 1/12 sum_t ||draw_k(t) - target(t)||_2
//   FDE_k        = ||draw_k(11) - target(11)||_2
//   minADE = min_k ADE_k, minFDE = min_k FDE_k (independently); kA / kF the
//     lowest k attaining each (ties to the lowest index: the result does not
//     depend on how the draws are shared out over lanes)
// Outputs: per_ped [S, F, Nmax, 4] = {minADE, minFDE, kA, kF} (zeros for
// non-pairs, every element written) or NULL; best [S, F, 2L, Nmax] = draw kA
// for pairs, pred elsewhere (every element written; the draw is regenerated
// from the counter, never stored along the way) or NULL; out [S, 8] =
// {sum minADE, sum minFDE, pairs, sum ADE(pred), sum FDE(pred), K, 0, 0} over
// the scene's pairs (ADE / FDE(pred): the same formulas on the mean, the fused
// step's metrics[3] / [4]), fixed summation order.
//
// Geometry.  One workgroup of 256 threads per (scene, chunk of FC frames).  A
// work item is (pair, slice): the K draws of a pair are dealt round-robin to
// KS = 2^j adjacent lanes (k = slice, slice + KS, ...); each lane holds the
// pair's 24 means and 24 target coordinates in registers (time-major, [2t +
// c]), draws in registers and keeps its running minima; the KS lanes' minima
// are combined by a butterfly on (value, index), lexicographic, so the lowest k
// wins a tie whatever KS is.
// KS and FC come from the shapes alone (bestk_geom, g2k_bestk_geom.h, shared
// with g2k_kde.hip): KS grows until the launch
// has ~2 * 256 CUs * 1024 items or K is used up, FC fills the 256 threads —
// S 256 x F 20 x Nmax 32 runs KS 4, FC 2 (2560 workgroups), real-data
// evaluation (F 1, n_active down to 2, K 20) runs KS 16 (a pair per quarter
// wave).  The items of a chunk are its PAIRS' (columns >= n_active and frames
// >= n_frames never reach the hash); non-pairs only get their zeros / copy.
// Scene sums: per-workgroup rows [S * C][8] in the caller's workspace, then
// g2k_bestk_rows_kernel adds a scene's C rows in chunk order (no atomics);
// C == 1 writes out directly.
#include "g2k_bestk_geom.h"
#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_head_draw.h"
#include "g2k_mix.h"

namespace g2k {
namespace {

template <class Head>
__global__ void __launch_bounds__(kBkThreads) best_of_k_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int FC, int C, int ks_log2, int K, uint32_t seed_lo, uint32_t seed_hi, int shared_targets,
    float* __restrict__ per_ped, float* __restrict__ best, float* __restrict__ rows) {
  __shared__ typename Head::Lds hlds;
  __shared__ float part[kBkThreads / 64][5];
  const int tid = threadIdx.x;
  const int s = blockIdx.x / C, c = blockIdx.x - s * C;
  const int f0 = c * FC;
  const int fcn = min(FC, F - f0);                         // frames of this chunk (0 when F == 0)
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  const int nfc = clampi(nf - f0, 0, fcn);                 // ... of them below n_frames
  const uint8_t* mask = ped_mask ? ped_mask + (size_t)s * Nmax : nullptr;

  Head::template stage<kBkThreads>(head_params, hlds, tid);
  // non-pairs: zeros in per_ped, pred in best
  if (per_ped || best) {
    for (int idx = tid; idx < fcn * Nmax; idx += kBkThreads) {
      const int fl = idx / Nmax, n = idx - fl * Nmax;
      const bool pair = fl < nfc && n < nact && (mask ? mask[n] != 0 : true);
      if (pair) continue;
      const size_t sf = (size_t)s * F + f0 + fl;
      if (per_ped) reinterpret_cast<float4*>(per_ped)[sf * Nmax + n] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (best) {
        const size_t pb = sf * kL2 * Nmax + n;
#pragma unroll
        for (int r = 0; r < kL2; ++r) best[pb + (size_t)r * Nmax] = pred[pb + (size_t)r * Nmax];
      }
    }
  }
  __syncthreads();
  Head head;
  head.bind(hlds);

  const int KS = 1 << ks_log2;
  const int j = tid & (KS - 1);                            // this lane's slice of the draws
  const int items = (nfc * nact) << ks_log2;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int base = 0; base < items; base += kBkThreads) {   // uniform trip count
    const int p = (base + tid) >> ks_log2;
    const bool valid = p < nfc * nact;
    const int fl = valid ? p / nact : 0, n = valid ? p - fl * nact : 0;
    const bool on = valid && (mask ? mask[n] != 0 : true);
    const size_t sf = (size_t)s * F + f0 + fl;
    const size_t pb = sf * kL2 * Nmax + n;
    const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;      // element of step 0
    float mu[kL2], tg[kL2];
    load_mu_tg(on, pred, targets, sf, shared_targets ? (size_t)s : sf, n, Nmax, mu, tg);
    float pa = 0.f, pf = 0.f;                              // ADE / FDE of the mean prediction
    if (on) {
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        const float dx = mu[2 * t] - tg[2 * t], dy = mu[2 * t + 1] - tg[2 * t + 1];
        pf = sqrtf(fmaf(dx, dx, dy * dy));
        pa += pf;
      }
      pa *= 1.0f / 12.0f;
    }
    float bA = __builtin_inff(), bF = __builtin_inff();
    int kA = 0, kF = 0;
    // pass 0: this lane's draws (k = j, j + KS, ...) and their running minima,
    // then the slices' combine; pass 1 (best only): slice 0 makes draw kA
    // again and stores it.  One loop body for both, so one copy of the draw.
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
      int k = pass ? kA : j;
      const int kend = pass ? (on && j == 0 ? kA + 1 : kA) : (on ? K : 0);
      const int kstep = pass ? 1 : KS;
#pragma nounroll
      for (; k < kend; k += kstep) {
        const uint32_t lo = seed_lo + (uint32_t)k;         // (seed + k) mod 2^64
        const uint32_t hi = seed_hi + (lo < seed_lo ? 1u : 0u);
        float ade = 0.f, dl = 0.f;
        // the stores' base, opaque to the compiler: the 24 store addresses
        // that it otherwise forms ahead of the loop and keeps across the draws
        // of pass 0 cost registers
        size_t sb = pb;
        asm volatile("" : "+v"(sb));
        head.draw(lo, hi, e0, n, Nmax, mu, [&](int t, float x, float y) {
          if (pass) {
            best[sb + (size_t)t * Nmax] = x;
            best[sb + (size_t)(kL + t) * Nmax] = y;
          }
          const float dx = x - tg[2 * t], dy = y - tg[2 * t + 1];
          dl = sqrtf(fmaf(dx, dx, dy * dy));
          ade += dl;
        });
        ade *= 1.0f / 12.0f;
        if (!pass) {
          if (ade < bA) { bA = ade; kA = k; }              // ascending k, strict: the lowest k stays
          if (dl < bF) { bF = dl; kF = k; }
        }
      }
      if (pass) break;
      for (int off = 1; off < KS; off <<= 1) {             // every lane takes part
        const float oA = __shfl_xor(bA, off), oF = __shfl_xor(bF, off);
        const int okA = __shfl_xor(kA, off), okF = __shfl_xor(kF, off);
        if (oA < bA || (oA == bA && okA < kA)) { bA = oA; kA = okA; }
        if (oF < bF || (oF == bF && okF < kF)) { bF = oF; kF = okF; }
      }
      if (!best) break;
    }
    if (on && j == 0) {
      if (per_ped)
        reinterpret_cast<float4*>(per_ped)[sf * Nmax + n] = make_float4(bA, bF, (float)kA, (float)kF);
      acc[0] += bA; acc[1] += bF; acc[2] += 1.f; acc[3] += pa; acc[4] += pf;
    }
  }
  // the workgroup's row: lanes by butterfly, waves in order
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const float v = wave_sum(acc[i]);
    if ((tid & 63) == 0) part[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < 8) {
    float v = 0.f;
    if (tid < 5) v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (tid == 5) v = (float)K;
    rows[(size_t)blockIdx.x * 8 + tid] = v;
  }
}

// out[s][i] = sum over the scene's C chunk rows, in chunk order
__global__ void __launch_bounds__(256) g2k_bestk_rows_kernel(const float* __restrict__ rows, int S,
                                                             int C, int K, float* __restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)S * 8) return;
  const int64_t s = id >> 3;
  const int i = (int)(id & 7);
  float v = 0.f;
  if (i < 5)
    for (int c = 0; c < C; ++c) v += rows[((size_t)s * C + c) * 8 + i];
  if (i == 5) v = (float)K;
  out[id] = v;
}

template <class Head>
int best_of_k_launch_as(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* head_params, uint64_t seed, int K, float* per_ped, float* best,
                        float* out, float* rows, hipStream_t st) {
  const BestkGeom g = bestk_geom(*d, K);
  const int64_t wgs = (int64_t)d->S * g.C;
  if (wgs > 0x7fffffff)
    return set_err(G2K_EINVAL, "%sbest_of_k: %lld workgroups", Head::kPrefix, (long long)wgs);
  hipLaunchKernelGGL(best_of_k_kernel<Head>, dim3((unsigned)wgs), dim3(kBkThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.FC, g.C,
                     g.ks_log2, K, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0, per_ped, best,
                     g.C == 1 ? out : rows);
  int rc = check_launch("best_of_k_kernel");
  if (rc || g.C == 1) return rc;
  hipLaunchKernelGGL(g2k_bestk_rows_kernel, dim3((unsigned)(((int64_t)d->S * 8 + 255) / 256)), dim3(256),
                     0, st, rows, d->S, g.C, K, out);
  return check_launch("g2k_bestk_rows_kernel");
}

// one row [8] per (scene, chunk); FC >= 1 frame per chunk, so at most F chunks
int64_t best_of_k_ws_bytes(const g2k_dims* d) {
  if (!d || d->S < 0 || d->F < 0) return -1;
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * 8 * 4;
}

// the argument checks, before any HIP call; `name` is the entry point's in the
// message; G2K_OK with S > 0: launch
int best_of_k_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                       const void* n_active, const void* head, int32_t K, const void* per_ped,
                       const void* out, const void* workspace, int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & G2K_STEP_PRED_PED_MAJOR)
    return set_err(G2K_EUNSUPPORTED, "%s reads pred_path_band [S, F, 2L, Nmax]", name);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (K < 1 || K > 4096) return set_err(G2K_EINVAL, "K=%d (1..4096)", K);
  if (const int rc = check_required({pred, targets, n_active, head, out})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_per_ped(per_ped)) return rc;
  return check_workspace(d, workspace, workspace_bytes, best_of_k_ws_bytes(d), 4);   // rows of floats
}

template <class Head>
int best_of_k(const char* name, const g2k_dims* d, const float* pred, const float* targets,
              const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
              const float* head, uint64_t seed, int32_t K, float* per_ped, float* best, float* out,
              void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = best_of_k_validate(name, d, pred, targets, n_active, head, K, per_ped, out, workspace,
                                    workspace_bytes);
  if (rc || d->S == 0) return rc;
  return best_of_k_launch_as<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K,
                                   per_ped, best, out, static_cast<float*>(workspace),
                                   (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

// the three heads share the geometry, so the workspace too
int64_t g2k_best_of_k_workspace_bytes(const g2k_dims* d) { return best_of_k_ws_bytes(d); }
int64_t g2k_fullcov_best_of_k_workspace_bytes(const g2k_dims* d) { return best_of_k_ws_bytes(d); }
int64_t g2k_mix_best_of_k_workspace_bytes(const g2k_dims* d) { return best_of_k_ws_bytes(d); }

// the launch geometry of the per-pair sampled evaluations (bestk_geom: host
// arithmetic, no HIP call), as the launchers work it out
int g2k_best_of_k_geometry(const g2k_dims* d, int32_t K, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (K < 1 || K > 4096) return set_err(G2K_EINVAL, "K=%d (1..4096)", K);
  if (!out) return set_err(G2K_EINVAL, "out is NULL");
  const BestkGeom g = bestk_geom(*d, K);
  out[0] = 1 << g.ks_log2;
  out[1] = g.FC;
  out[2] = g.C;
  return G2K_OK;
}

// The full-covariance head's comes first in each of the three families of
// this kind (here, g2k_joint.hip, g2k_kde.hip): a kernel is emitted where its
// instantiation is first named, and that is the order the code objects have
// always had.
int g2k_fullcov_best_of_k_f32(const g2k_dims* d, const float* pred, const float* targets,
                              const int32_t* n_active, const int32_t* n_frames,
                              const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                              float* per_ped, float* best, float* out, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  return best_of_k<FullCovHead>("fullcov_best_of_k", d, pred, targets, n_active, n_frames, ped_mask,
                                chol, seed, K, per_ped, best, out, workspace, workspace_bytes, stream);
}

int g2k_best_of_k_f32(const g2k_dims* d, const float* pred, const float* targets,
                      const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                      const float* head, uint64_t seed, int32_t K, float* per_ped, float* best,
                      float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  return best_of_k<PerStepHead>("best_of_k", d, pred, targets, n_active, n_frames, ped_mask, head, seed,
                                K, per_ped, best, out, workspace, workspace_bytes, stream);
}

// mix [8][608] (include/g2k_mix.h)
int g2k_mix_best_of_k_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames,
                          const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                          float* per_ped, float* best, float* out, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  return best_of_k<MixHead>("mix_best_of_k", d, pred, targets, n_active, n_frames, ped_mask, mix, seed,
                            K, per_ped, best, out, workspace, workspace_bytes, stream);
}

}  // extern "C"
