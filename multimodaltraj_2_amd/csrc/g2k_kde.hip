// g2k_kde.hip — fused KDE-NLL evaluation of a probabilistic head's samples
// (the KDE-NLL of Trajectron++): ONE kernel, kde_nll_kernel<Head>, instantiated
// for the per-step bivariate-Gaussian head (g2k_kde_nll_f32), for the
// full-covariance trajectory head (g2k_fullcov_kde_nll_f32) and for the
// Gaussian-mixture head (g2k_mix_kde_nll_f32, include/g2k_mix.h); the heads are
// the policies of g2k_head_draw.h.  The C entry points and their validator are
// at the end of this file.  The build's: the reference has no probabilistic
// head, so PARITY UNPINNED; pinned against scipy.stats.gaussian_kde through
// tests/kde_ref.py.
//
// Definition.  Inputs and pairs as g2k_best_of_k_f32 (g2k_bestk.hip), K in
// [4, 4096], log_floor finite.  Draw k = what the head's sampler writes for
// seed (seed + k) mod 2^64.  For a pair and a step t, x_k the K drawn 2-D
// positions, y the target:
//   c      = sample covariance of the x_k, divisor K - 1
//   H      = K^(-1/3) c           (Scott's factor K^(-1/(d + 4)) squared, d = 2)
//   logp_t = log(1/K sum_k exp(-1/2 (y - x_k)^T H^-1 (y - x_k))) - log 2 pi
//            - 1/2 log det H
//   term_t = max(logp_t, log_floor); the step is CLIPPED when logp_t <
//            log_floor or det H is not a positive finite number (term_t =
//            log_floor then)
//   kde_nll = -1/12 sum_t term_t,  kde_nll_final = -term_11
// Outputs: per_ped [S, F, Nmax, 4] = {kde_nll, kde_nll_final, clipped steps, 0}
// (zeros for non-pairs, every element written) or NULL; out [S, 8] = {sum
// kde_nll, sum kde_nll_final, pairs, sum clipped steps, K, log_floor, 0, 0}
// over the scene's pairs, fixed summation order, no atomics.
//
// Geometry: best_of_k_kernel's (g2k_bestk_geom.h) — one workgroup of 256
// threads per (scene, chunk of FC frames), an item is (pair, slice), the K
// draws dealt round-robin to KS = 2^j adjacent lanes, the pair's 24 means and 24
// targets in registers, time-major.  Two passes over the same K draws, none
// stored: the second pass makes the draws again from the counter.
//   pass 0   per step the five moments of d = x - mu (sum dx, dy, dx^2, dy^2,
//            dx dy; fp32; centred on the mean so that the sums stay small).
//            The mixture head (Head::kKdeRunningMean; g2k_mix_kde_nll_f32)
//            draws around mu + b_m with |b_m| many times the spread, where
//            sum d^2 - (sum d)^2 / K cancels in fp32: its lanes keep a running
//            mean of d and the sums of the centred products (Welford's update),
//            and the butterfly merges them by Chan's formula; the covariance
//            is then the centred sum / (K - 1) with nothing subtracted
//   combine  the KS lanes' moments by a butterfly (every lane of the group ends
//            with the same bits), then per step IN DOUBLE: covariance, Scott's
//            factor, determinant, inverse and the constant -log K - log 2 pi -
//            1/2 log det H (the determinant's cancellation is where fp32 loses
//            the answer); the three inverse entries and the constant rounded
//            to fp32
//   pass 1   a_k = -1/2 (y - x_k)^T H^-1 (y - x_k) and an online (running max,
//            scaled sum) log-sum-exp per step, fp32; the KS lanes' (max, sum)
//            by a butterfly; slice 0 forms the terms, the clip count and the
//            pair's figures
// Per step a lane keeps SIX registers, w[t][0..5]: the five moments in pass 0,
// and after the combine — when the moments are dead — the same registers hold
// the inverse's three entries, the constant, the running max and the scaled
// sum.  One loop body serves both passes: one copy of the draw code.
// Scene sums: per-workgroup rows [S * C][8] in the caller's workspace, then
// g2k_kde_rows_kernel adds a scene's C rows in chunk order; C == 1 writes out
// directly.
#include "g2k_bestk_geom.h"
#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_head_draw.h"
#include "g2k_mix.h"

namespace g2k {
namespace {

constexpr float kKdeLow = -3.0e38f;   // "no term yet": finite, so that no difference of maxima is NaN

template <class Head>
__global__ void __launch_bounds__(kBkThreads) kde_nll_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int FC, int C, int ks_log2, int K, uint32_t seed_lo, uint32_t seed_hi, int shared_targets,
    float log_floor, double scott, double cst0, float* __restrict__ per_ped,
    float* __restrict__ rows) {
  __shared__ typename Head::Lds hlds;
  __shared__ float part[kBkThreads / 64][4];
  const int tid = threadIdx.x;
  const int s = blockIdx.x / C, c = blockIdx.x - s * C;
  const int f0 = c * FC;
  const int fcn = min(FC, F - f0);                         // frames of this chunk (0 when F == 0)
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  const int nfc = clampi(nf - f0, 0, fcn);                 // ... of them below n_frames
  const uint8_t* mask = ped_mask ? ped_mask + (size_t)s * Nmax : nullptr;

  Head::template stage<kBkThreads>(head_params, hlds, tid);
  // non-pairs: zeros in per_ped
  if (per_ped) {
    for (int idx = tid; idx < fcn * Nmax; idx += kBkThreads) {
      const int fl = idx / Nmax, n = idx - fl * Nmax;
      const bool pair = fl < nfc && n < nact && (mask ? mask[n] != 0 : true);
      if (pair) continue;
      const size_t sf = (size_t)s * F + f0 + fl;
      reinterpret_cast<float4*>(per_ped)[sf * Nmax + n] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  Head head;
  head.bind(hlds);

  const int KS = 1 << ks_log2;
  const int j = tid & (KS - 1);                            // this lane's slice of the draws
  const int items = (nfc * nact) << ks_log2;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int base = 0; base < items; base += kBkThreads) {   // uniform trip count
    const int p = (base + tid) >> ks_log2;
    const bool valid = p < nfc * nact;
    const int fl = valid ? p / nact : 0, n = valid ? p - fl * nact : 0;
    const bool on = valid && (mask ? mask[n] != 0 : true);
    const size_t sf = (size_t)s * F + f0 + fl;
    const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;      // element of step 0
    float mu[kL2], tg[kL2];
    load_mu_tg(on, pred, targets, sf, shared_targets ? (size_t)s : sf, n, Nmax, mu, tg);
    // pass 0: {sum dx, sum dy, sum dx^2, sum dy^2, sum dx dy}; pass 1: {H^-1 xx,
    // H^-1 yy, H^-1 xy, constant, running max, scaled sum}
    float w[kL][6];
#pragma unroll
    for (int t = 0; t < kL; ++t) {
#pragma unroll
      for (int i = 0; i < 6; ++i) w[t][i] = 0.f;
    }
    const int kend = on ? K : 0;
    float cnt = 0.f;                                       // kKdeRunningMean: this lane's draws so far
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma nounroll
      for (int k = j; k < kend; k += KS) {
        const uint32_t lo = seed_lo + (uint32_t)k;         // (seed + k) mod 2^64
        const uint32_t hi = seed_hi + (lo < seed_lo ? 1u : 0u);
        float rc = 0.f;
        if constexpr (Head::kKdeRunningMean) {
          if (!pass) { cnt += 1.f; rc = 1.0f / cnt; }
        }
        head.draw(lo, hi, e0, n, Nmax, mu, [&](int t, float x, float y) {
          if (!pass) {
            const float dx = x - mu[2 * t], dy = y - mu[2 * t + 1];
            if constexpr (Head::kKdeRunningMean) {
              // {mean dx, mean dy, sum of centred dx^2, dy^2, dx dy} of the
              // lane's draws so far (Welford's update)
              const float ux = dx - w[t][0], uy = dy - w[t][1];
              w[t][0] = fmaf(ux, rc, w[t][0]);
              w[t][1] = fmaf(uy, rc, w[t][1]);
              const float vx = dx - w[t][0], vy = dy - w[t][1];
              w[t][2] = fmaf(ux, vx, w[t][2]);
              w[t][3] = fmaf(uy, vy, w[t][3]);
              w[t][4] = fmaf(ux, vy, w[t][4]);
            } else {
              w[t][0] += dx;
              w[t][1] += dy;
              w[t][2] = fmaf(dx, dx, w[t][2]);
              w[t][3] = fmaf(dy, dy, w[t][3]);
              w[t][4] = fmaf(dx, dy, w[t][4]);
            }
          } else {
            const float ex = tg[2 * t] - x, ey = tg[2 * t + 1] - y;
            const float q = fmaf(ex, fmaf(w[t][0], ex, 2.f * w[t][2] * ey), w[t][1] * ey * ey);
            const float a = fmaxf(-0.5f * q, kKdeLow);     // a NaN or -inf distance counts as far away
            const float m = w[t][4];
            const float e = __expf(fminf(m, a) - fmaxf(m, a));
            w[t][5] = a > m ? fmaf(w[t][5], e, 1.f) : w[t][5] + e;
            w[t][4] = fmaxf(m, a);
          }
        });
      }
      if (pass) break;
      // the group's moments, the same bits in each of its lanes
      for (int off = 1; off < KS; off <<= 1) {             // every lane takes part
        if constexpr (Head::kKdeRunningMean) {
          // Chan's merge of two lanes' (count, means, centred sums); A is the
          // lane whose bit `off` is clear, in both lanes of the exchange, so
          // that both form the same bits.  A lane without a draw has count 0
          // and zeros: the other lane's values pass through unchanged.
          const float ocnt = __shfl_xor(cnt, off);
          const bool low = !(tid & off);
          const float nA = low ? cnt : ocnt, nB = low ? ocnt : cnt;
          cnt = nA + nB;
          const float fB = cnt > 0.f ? nB / cnt : 0.f;     // nB / n
          const float fAB = nA * fB;                       // nA nB / n
#pragma unroll
          for (int t = 0; t < kL; ++t) {
            float A[5], B[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
              const float o = __shfl_xor(w[t][i], off);
              A[i] = low ? w[t][i] : o;
              B[i] = low ? o : w[t][i];
            }
            const float ex = B[0] - A[0], ey = B[1] - A[1];
            w[t][0] = fmaf(ex, fB, A[0]);
            w[t][1] = fmaf(ey, fB, A[1]);
            w[t][2] = fmaf(ex * ex, fAB, A[2] + B[2]);
            w[t][3] = fmaf(ey * ey, fAB, A[3] + B[3]);
            w[t][4] = fmaf(ex * ey, fAB, A[4] + B[4]);
          }
        } else {
#pragma unroll
          for (int t = 0; t < kL; ++t) {
#pragma unroll
            for (int i = 0; i < 5; ++i) w[t][i] += __shfl_xor(w[t][i], off);
          }
        }
      }
      // the bandwidth, in double; its registers take the moments' place
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        const double sx = w[t][0], sy = w[t][1];
        const double rk = 1.0 / (double)K, rk1 = scott / (double)(K - 1);
        // kKdeRunningMean: the sums are centred already
        const double hxx = ((double)w[t][2] - (Head::kKdeRunningMean ? 0.0 : sx * sx * rk)) * rk1;
        const double hyy = ((double)w[t][3] - (Head::kKdeRunningMean ? 0.0 : sy * sy * rk)) * rk1;
        const double hxy = ((double)w[t][4] - (Head::kKdeRunningMean ? 0.0 : sx * sy * rk)) * rk1;
        const double det = hxx * hyy - hxy * hxy;
        const bool ok = det > 0.0 && det < __builtin_inf();
        const double rdet = 1.0 / (ok ? det : 1.0);
        const float ixx = (float)(hyy * rdet), iyy = (float)(hxx * rdet), ixy = (float)(-hxy * rdet);
        const float cst = (float)(cst0 - 0.5 * log(ok ? det : 1.0));
        // a singular step: every term far away, the constant below any floor
        w[t][0] = ok ? ixx : 0.f;
        w[t][1] = ok ? iyy : 0.f;
        w[t][2] = ok ? ixy : 0.f;
        w[t][3] = ok ? cst : -__builtin_inff();
        w[t][4] = kKdeLow;
        w[t][5] = 0.f;
      }
    }
    // the group's log-sum-exp per step
    for (int off = 1; off < KS; off <<= 1) {               // every lane takes part
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        const float om = __shfl_xor(w[t][4], off), os = __shfl_xor(w[t][5], off);
        const float hi = fmaxf(w[t][4], om);
        w[t][5] = fmaf(w[t][5], __expf(w[t][4] - hi), os * __expf(om - hi));
        w[t][4] = hi;
      }
    }
    if (on && j == 0) {
      float sum = 0.f, last = 0.f, clipped = 0.f;
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        const float logp = w[t][3] + (w[t][4] + logf(w[t][5]));
        const bool clip = !(logp >= log_floor);            // a NaN clips too
        last = clip ? log_floor : logp;
        sum += last;
        clipped += clip ? 1.f : 0.f;
      }
      const float nll = -sum * (1.0f / 12.0f);
      if (per_ped)
        reinterpret_cast<float4*>(per_ped)[sf * Nmax + n] = make_float4(nll, -last, clipped, 0.f);
      acc[0] += nll; acc[1] -= last; acc[2] += 1.f; acc[3] += clipped;
    }
  }
  // the workgroup's row: lanes by butterfly, waves in order
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v = wave_sum(acc[i]);
    if ((tid & 63) == 0) part[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < 8) {
    float v = 0.f;
    if (tid < 4) v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (tid == 4) v = (float)K;
    if (tid == 5) v = log_floor;
    rows[(size_t)blockIdx.x * 8 + tid] = v;
  }
}

// out[s][i] = sum over the scene's C chunk rows, in chunk order
__global__ void __launch_bounds__(256) g2k_kde_rows_kernel(const float* __restrict__ rows, int S,
                                                           int C, int K, float log_floor,
                                                           float* __restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)S * 8) return;
  const int64_t s = id >> 3;
  const int i = (int)(id & 7);
  float v = 0.f;
  if (i < 4)
    for (int c = 0; c < C; ++c) v += rows[((size_t)s * C + c) * 8 + i];
  if (i == 4) v = (float)K;
  if (i == 5) v = log_floor;
  out[id] = v;
}

template <class Head>
int kde_nll_launch_as(const g2k_dims* d, const float* pred, const float* targets,
                      const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                      const float* head_params, uint64_t seed, int K, float log_floor, float* per_ped,
                      float* out, float* rows, hipStream_t st) {
  const BestkGeom g = bestk_geom(*d, K);
  const int64_t wgs = (int64_t)d->S * g.C;
  if (wgs > 0x7fffffff)
    return set_err(G2K_EINVAL, "%skde_nll: %lld workgroups", Head::kPrefix, (long long)wgs);
  const double scott = pow((double)K, -1.0 / 3.0);
  const double cst0 = -log((double)K) - log(6.283185307179586476925286766559);
  hipLaunchKernelGGL(kde_nll_kernel<Head>, dim3((unsigned)wgs), dim3(kBkThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.FC, g.C,
                     g.ks_log2, K, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0, log_floor, scott, cst0, per_ped,
                     g.C == 1 ? out : rows);
  int rc = check_launch("kde_nll_kernel");
  if (rc || g.C == 1) return rc;
  hipLaunchKernelGGL(g2k_kde_rows_kernel, dim3((unsigned)(((int64_t)d->S * 8 + 255) / 256)), dim3(256),
                     0, st, rows, d->S, g.C, K, log_floor, out);
  return check_launch("g2k_kde_rows_kernel");
}

// one row [8] per (scene, chunk); FC >= 1 frame per chunk, so at most F chunks
int64_t kde_nll_ws_bytes(const g2k_dims* d) {
  if (!d || d->S < 0 || d->F < 0) return -1;
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * 8 * 4;
}

// the argument checks, before any HIP call; `name` is the entry point's in the
// message; G2K_OK with S > 0 and F > 0: launch
int kde_nll_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                     const void* n_active, const void* head, int32_t K, float log_floor,
                     const void* per_ped, const void* out, const void* workspace,
                     int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & G2K_STEP_PRED_PED_MAJOR)
    return set_err(G2K_EUNSUPPORTED, "%s reads pred_path_band [S, F, 2L, Nmax]", name);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (K < 4 || K > 4096) return set_err(G2K_EINVAL, "K=%d (4..4096)", K);
  if (!(log_floor >= -3.402823466e38f && log_floor <= 3.402823466e38f))
    return set_err(G2K_EINVAL, "log_floor=%g (finite)", (double)log_floor);
  if (const int rc = check_required({pred, targets, n_active, head, out})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_per_ped(per_ped)) return rc;
  return check_workspace(d, workspace, workspace_bytes, kde_nll_ws_bytes(d), 4);   // rows of floats
}

// S == 0 or F == 0 launches nothing
template <class Head>
int kde_nll(const char* name, const g2k_dims* d, const float* pred, const float* targets,
            const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
            const float* head, uint64_t seed, int32_t K, float log_floor, float* per_ped, float* out,
            void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = kde_nll_validate(name, d, pred, targets, n_active, head, K, log_floor, per_ped, out,
                                  workspace, workspace_bytes);
  if (rc || d->S == 0 || d->F == 0) return rc;
  return kde_nll_launch_as<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K,
                                 log_floor, per_ped, out, static_cast<float*>(workspace),
                                 (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

// the three heads share the geometry, so the workspace too
int64_t g2k_kde_nll_workspace_bytes(const g2k_dims* d) { return kde_nll_ws_bytes(d); }
int64_t g2k_fullcov_kde_nll_workspace_bytes(const g2k_dims* d) { return kde_nll_ws_bytes(d); }
int64_t g2k_mix_kde_nll_workspace_bytes(const g2k_dims* d) { return kde_nll_ws_bytes(d); }

// the full-covariance head's first: see g2k_bestk.hip
int g2k_fullcov_kde_nll_f32(const g2k_dims* d, const float* pred, const float* targets,
                            const int32_t* n_active, const int32_t* n_frames,
                            const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                            float log_floor, float* per_ped, float* out, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  return kde_nll<FullCovHead>("fullcov_kde_nll", d, pred, targets, n_active, n_frames, ped_mask, chol,
                              seed, K, log_floor, per_ped, out, workspace, workspace_bytes, stream);
}

int g2k_kde_nll_f32(const g2k_dims* d, const float* pred, const float* targets,
                    const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                    const float* head, uint64_t seed, int32_t K, float log_floor, float* per_ped,
                    float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  return kde_nll<PerStepHead>("kde_nll", d, pred, targets, n_active, n_frames, ped_mask, head, seed, K,
                              log_floor, per_ped, out, workspace, workspace_bytes, stream);
}

// mix [8][608] (include/g2k_mix.h); the kernel keeps running-mean moments
// for this head (Head::kKdeRunningMean)
int g2k_mix_kde_nll_f32(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* mix, uint64_t seed, int32_t K, float log_floor, float* per_ped,
                        float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  return kde_nll<MixHead>("mix_kde_nll", d, pred, targets, n_active, n_frames, ped_mask, mix, seed, K,
                          log_floor, per_ped, out, workspace, workspace_bytes, stream);
}

}  // extern "C"
