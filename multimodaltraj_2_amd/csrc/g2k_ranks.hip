// g2k_ranks.hip — fused rank-histogram calibration of a probabilistic head's
// samples (the multivariate rank histogram of Gneiting et al. 2008): per pair
// the target's rank among the K draws under a per-step density pre-rank and a
// trajectory-level energy pre-rank.  ONE kernel, sample_ranks_kernel<Head>,
// instantiated for the per-step head (g2k_sample_ranks_f32), the
// full-covariance head (g2k_fullcov_sample_ranks_f32) and the mixture head
// (g2k_mix_sample_ranks_f32); the heads are the policies of g2k_head_draw.h.
// The C entry points are at the end of this file, declared in
// include/g2k_ranks.h (added after ABI 11: bound by symbol).  The build's: the
// reference has no probabilistic head, so PARITY UNPINNED; pinned against
// tests/ranks_ref.py.
//
// Definition.  Inputs and pairs as g2k_best_of_k_f32 (g2k_bestk.hip), K in
// [4, 255], B bins in [1, 64] with (K + 1) % B == 0.  Draw k = what the head's
// sampler writes for seed (seed + k) mod 2^64.  Z = {Y, X_0, ..., X_{K-1}} the
// target pooled with the draws.  Per step t:
//   c_t      = sample covariance of the K + 1 positions Z(t), divisor K
//   H_t      = (K + 1)^(-1/3) c_t
//   rho_t(z) = sum over the other K points z' of exp(-1/2 (z - z')^T H_t^-1 (z - z'))
//   r_t      = #{k : rho_t(X_k) > rho_t(Y)}; -1 when det H_t is not a positive
//              finite number (a DEGENERATE step: in no histogram, counted)
// and per trajectory rho_traj(z) = sum over the other K points of ||z - z'||
// over the 24 coordinates, r_traj = #{k : rho_traj(X_k) < rho_traj(Y)}.
// per_ped [S, F, Nmax, 16] (or NULL) = {r_0..r_11, r_traj, degenerate steps, 0,
// 0}, zeros for non-pairs, every element written; hist [S, 13, B] int32 = the
// pairs' ranks in bins floor(r B / (K + 1)); tot [S, 4] int64 = {pairs,
// degenerate steps, sum r_t, sum r_traj}.  Integers only across pairs.
//
// Geometry and pass scaffold: the drawn-once family's (g2k_drawn.h); the draws
// in xy[slot][24], time-major (the pitch of g2k_scores.hip, where 28 floats
// measured the same).  Per pass, six barriers:
//   draw     the lane draws X_k into registers and its slot; draw 0's lane puts
//            the pair's target and means next to them
//   moments  12 items per pair dealt to the 256 lanes: a step's five pooled
//            moments over the K slots and the target, centred as
//            kde_nll_kernel centres them (Head::kKdeRunningMean), then the
//            covariance, Scott's factor, the determinant and the Cholesky
//            factor of the bandwidth, ALL IN DOUBLE (an item's walk is 1 / K
//            of a lane's: fp32 sums would save nothing and cost two digits of
//            rho); the three entries of the factor's inverse go to LDS in fp32
//            scaled by sqrt(1/2 log2 e), with the step's "not degenerate" flag
//   walk     the lane takes its pair's 36 scaled entries into registers and
//            walks the partners k + 1, ..., k + K - 1 (mod K) from LDS, 6
//            ds_read_b128 each: per step one quadratic form (fp32, a sum of
//            two squares: rk_term) and one v_exp_f32, and the 24-D norm; then
//            the same against the target.  Unlike the scores' couples every
//            lane needs its own sums: the full range, K (K - 1) terms a pair
//            and not half of them.  The lane keeps rho_0..11 and rho_traj in
//            registers
//   terms    (the slots are dead) the lane leaves its 13 terms against the
//            target in its own slot
//   target   13 items per pair: the target's sums over the K slots, in k order
//   compare  the lane compares its 13 sums with the target's: 13 bits
//   count    14 items per pair: row i < 13 counts bit i over the K lanes, in k
//            order, writes the rank and bumps the workgroup's LDS histogram
//            (integer atomics: the order cannot show); item 13 counts the
//            degenerate steps and the pair
// The 32-pair cap is the LDS budget: with the mixture head's 19 KB of factors
// next to the 24 KB of draws, the per-pair arrays (target, means, inverse
// factors, the target's sums) leave 32 pairs below 64 KB.  Using the dead slots for the
// terms against the target costs the fourth barrier and saves [13][256] floats,
// without which the cap would be 8.
// Scene sums: per-workgroup integer rows in the caller's workspace (tot
// [S * C][4] int64, then hist [S * C][13 B] int32), then drawn_hist_rows_kernel
// adds a scene's C rows in chunk order; C == 1 writes hist and tot directly.
#include "g2k_drawn.h"

namespace g2k {
namespace {

constexpr int kRkThreads = kDrThreads, kRkMaxG = kDrMaxG, kRkPitch = kDrPitch;
constexpr int kRkRows = G2K_RANKS_ROWS;       // 13: the steps' ranks and the trajectory's
constexpr int kRkItems = kRkRows + 1;         // the count stage: the rows, then the pair's own item
constexpr int kRkTot = 4;
constexpr int kRkLdsBytes = (kRkThreads * kRkPitch + 2 * kRkMaxG * kL2 + kRkMaxG * kL * 4 +
                             kRkMaxG * kRkRows + kRkThreads + kRkRows * G2K_RANKS_BMAX + 4) * 4;
constexpr float kRkFar = -3.0e38f;            // a NaN exponent counts as far away (kde_nll_kernel's)

__device__ __forceinline__ float rk_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float rk_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// one kernel term of the density pre-rank, exp(-1/2 e^T H^-1 e) = 2^-(u^2 + v^2):
// (u, v) = sqrt(1/2 log2 e) l^-1 e for H = l l^T, whose rows are (a, 0), (b, c).
// A sum of two squares: where H is nearly singular the form a' ex^2 + b' ex ey
// + c' ey^2 loses to cancellation ten times what this one does, at the same
// five instructions
__device__ __forceinline__ float rk_term(float ex, float ey, float a, float b, float c) {
  const float u = a * ex, v = fmaf(b, ex, c * ey);
  return rk_exp2(fmaxf(-fmaf(u, u, v * v), kRkFar));
}

// two waves a SIMD (the LDS lets two workgroups share a CU): at most 256 VGPRs
template <class Head>
__global__ void __launch_bounds__(kRkThreads, 2) sample_ranks_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int FC, int C, int G, int K, int B, uint32_t seed_lo, uint32_t seed_hi, int shared_targets,
    double scott, float* __restrict__ per_ped, int32_t* __restrict__ hist_rows,
    int64_t* __restrict__ tot_rows) {
  __shared__ typename Head::Lds hlds;
  __shared__ __attribute__((aligned(16))) float xy[kRkThreads * kRkPitch];
  __shared__ __attribute__((aligned(16))) float tgs[kRkMaxG * kL2];    // the pairs' targets, time-major
  __shared__ __attribute__((aligned(16))) float mus[kRkMaxG * kL2];    // ... means
  __shared__ float4 hinv[kRkMaxG * kL];       // per (pair, step) {a, b, c of rk_term, 0 = degenerate or 1}
  __shared__ float rhoy[kRkMaxG * kRkRows];   // the target's 13 sums
  __shared__ uint32_t cmp[kRkThreads];        // bit i: the lane's sum i puts its draw ahead of the target
  __shared__ int lh[kRkRows * G2K_RANKS_BMAX];
  __shared__ int lt[4];
  const int tid = threadIdx.x;
  const DrawnChunk ch = drawn_chunk(n_active, n_frames, ped_mask, F, Nmax, FC, C);
  const int s = ch.s, f0 = ch.f0, nact = ch.nact;
  const uint8_t* mask = ch.mask;

  Head::template stage<kRkThreads>(head_params, hlds, tid);
  for (int i = tid; i < kRkRows * B; i += kRkThreads) lh[i] = 0;
  if (tid < 4) lt[tid] = 0;
  if (per_ped) drawn_zero_per_ped<4>(ch, per_ped, tid);               // 16 columns
  __syncthreads();
  Head head;
  head.bind(hlds);

  const DrawnLane ln = drawn_lane(tid, K, seed_lo, seed_hi);
  const int npairs = drawn_npairs(ch);
  const int g = ln.g, k = ln.k;
  const int binw = (K + 1) / B;                            // ranks per bin
  const double rK = 1.0 / (double)K, rK1 = 1.0 / (double)(K + 1);
#pragma nounroll
  for (int base = 0; base < npairs; base += G) {           // uniform trip count
    // ---- draw ----
    const DrawnItem it = drawn_item(ch, base, G, g);
    const int gp = it.gp;
    const bool on = it.on;
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
      store_draw(xy + tid * kRkPitch, x);
      if (k == 0) {
        store_draw(tgs + g * kL2, tg);
        store_draw(mus + g * kL2, mu);
      }
    } else {
      zero_draw(x);
    }
    __syncthreads();
    // ---- moments: item (pair, step), the K slots and then the target ----
    for (int idx = tid; idx < gp * kL; idx += kRkThreads) {
      const int gi = idx / kL, t = idx - gi * kL;
      const int pp = base + gi;
      const int n2 = pp - (pp / nact) * nact;
      if (!(mask ? mask[n2] != 0 : true)) continue;
      const float* row = xy + gi * K * kRkPitch + 2 * t;
      const float2 y = *reinterpret_cast<const float2*>(tgs + gi * kL2 + 2 * t);
      // the centred sums of products, IN DOUBLE: the differences in fp32, their
      // products and sums in double (fp32 sums leave 1e-4 of relative error in
      // rho where the pooled points are nearly collinear: tests/ranks_ref.py)
      double cxx, cyy, cxy;
      if constexpr (Head::kKdeRunningMean) {
        // {mean, centred sums} of the points so far (Welford's update)
        double mx = 0.0, my = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma nounroll
        for (int kk = 0; kk <= K; ++kk) {
          const float2 z = kk < K ? *reinterpret_cast<const float2*>(row + kk * kRkPitch) : y;
          const double rc = 1.0 / (double)(kk + 1);
          const double ux = (double)z.x - mx, uy = (double)z.y - my;
          mx = fma(ux, rc, mx);
          my = fma(uy, rc, my);
          const double vx = (double)z.x - mx, vy = (double)z.y - my;
          sxx = fma(ux, vx, sxx);
          syy = fma(uy, vy, syy);
          sxy = fma(ux, vy, sxy);
        }
        cxx = sxx; cyy = syy; cxy = sxy;
      } else {
        // plain sums of d = z - mu: the draws sit around the means
        const float2 m = *reinterpret_cast<const float2*>(mus + gi * kL2 + 2 * t);
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma nounroll
        for (int kk = 0; kk <= K; ++kk) {
          const float2 z = kk < K ? *reinterpret_cast<const float2*>(row + kk * kRkPitch) : y;
          const double dx = (double)(z.x - m.x), dy = (double)(z.y - m.y);
          sx += dx;
          sy += dy;
          sxx = fma(dx, dx, sxx);
          syy = fma(dy, dy, syy);
          sxy = fma(dx, dy, sxy);
        }
        cxx = sxx - sx * sx * rK1;
        cyy = syy - sy * sy * rK1;
        cxy = sxy - sx * sy * rK1;
      }
      // the bandwidth H = l l^T and the rows of sqrt(1/2 log2 e) l^-1
      const double w = scott * rK;
      const double hxx = cxx * w, hyy = cyy * w, hxy = cxy * w;
      const double det = hxx * hyy - hxy * hxy;
      const bool ok = det > 0.0 && det < __builtin_inf();
      const double l11 = sqrt(ok ? hxx : 1.0), l21 = hxy / l11, l22 = sqrt(ok ? det : 1.0) / l11;
      const double sc = 0.84932180028801904272;            // sqrt(1/2 log2 e)
      hinv[idx] = ok ? make_float4((float)(sc / l11), (float)(-sc * l21 / (l11 * l22)),
                                   (float)(sc / l22), 1.f)
                     : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    // ---- walk: the lane's sums over its K - 1 partners and the target ----
    float rho[kRkRows], te[kRkRows];
#pragma unroll
    for (int i = 0; i < kRkRows; ++i) { rho[i] = 0.f; te[i] = 0.f; }
    if (on) {
      float ha[kL], hb[kL], hc[kL];
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        const float4 v = hinv[g * kL + t];
        ha[t] = v.x; hb[t] = v.y; hc[t] = v.z;
      }
      int l = k;
#pragma nounroll
      for (int j = 1; j < K; ++j) {
        l = l + 1 == K ? 0 : l + 1;
        const float4* q4 = reinterpret_cast<const float4*>(xy + (g * K + l) * kRkPitch);
        float r2 = 0.f;
#pragma unroll
        for (int q = 0; q < kL2 / 4; ++q) {
          const float4 v = q4[q];
          const float ax = x[4 * q] - v.x, ay = x[4 * q + 1] - v.y;
          const float bx = x[4 * q + 2] - v.z, by = x[4 * q + 3] - v.w;
          rho[2 * q] += rk_term(ax, ay, ha[2 * q], hb[2 * q], hc[2 * q]);
          rho[2 * q + 1] += rk_term(bx, by, ha[2 * q + 1], hb[2 * q + 1], hc[2 * q + 1]);
          r2 += fmaf(ax, ax, ay * ay) + fmaf(bx, bx, by * by);
        }
        rho[kL] += rk_sqrt(r2);
      }
      const float4* q4 = reinterpret_cast<const float4*>(tgs + g * kL2);
      float r2 = 0.f;
#pragma unroll
      for (int q = 0; q < kL2 / 4; ++q) {
        const float4 v = q4[q];
        const float ax = x[4 * q] - v.x, ay = x[4 * q + 1] - v.y;
        const float bx = x[4 * q + 2] - v.z, by = x[4 * q + 3] - v.w;
        te[2 * q] = rk_term(ax, ay, ha[2 * q], hb[2 * q], hc[2 * q]);
        te[2 * q + 1] = rk_term(bx, by, ha[2 * q + 1], hb[2 * q + 1], hc[2 * q + 1]);
        r2 += fmaf(ax, ax, ay * ay) + fmaf(bx, bx, by * by);
      }
      te[kL] = rk_sqrt(r2);
#pragma unroll
      for (int i = 0; i < kRkRows; ++i) rho[i] += te[i];
    }
    __syncthreads();
    // ---- terms: the slots are dead; the lane's terms against the target ----
    if (on) {
      float4* o = reinterpret_cast<float4*>(xy + tid * kRkPitch);
      o[0] = make_float4(te[0], te[1], te[2], te[3]);
      o[1] = make_float4(te[4], te[5], te[6], te[7]);
      o[2] = make_float4(te[8], te[9], te[10], te[11]);
      xy[tid * kRkPitch + kL] = te[kL];
    }
    __syncthreads();
    // ---- target: item (pair, row), the K terms in k order ----
    for (int idx = tid; idx < gp * kRkRows; idx += kRkThreads) {
      const int gi = idx / kRkRows, i = idx - gi * kRkRows;
      const float* col = xy + gi * K * kRkPitch + i;
      float sum = 0.f;
#pragma nounroll
      for (int kk = 0; kk < K; ++kk) sum += col[kk * kRkPitch];
      rhoy[idx] = sum;                                     // a masked pair's: never looked at
    }
    __syncthreads();
    // ---- compare ----
    {
      uint32_t bits = 0;
      if (on) {
        const float* ry = rhoy + g * kRkRows;
#pragma unroll
        for (int t = 0; t < kL; ++t) bits |= rho[t] > ry[t] ? 1u << t : 0u;
        bits |= rho[kL] < ry[kL] ? 1u << kL : 0u;
      }
      cmp[tid] = bits;
    }
    __syncthreads();
    // ---- count: item (pair, row); the rows' ranks, then the pair's own item.
    // What it reads (cmp, hinv) is next written after the following pass's
    // barriers
    for (int idx = tid; idx < gp * kRkItems; idx += kRkThreads) {
      const int gi = idx / kRkItems, i = idx - gi * kRkItems;
      const int pp = base + gi;
      const int fl2 = pp / nact, n2 = pp - fl2 * nact;
      if (!(mask ? mask[n2] != 0 : true)) continue;
      const size_t sf = (size_t)s * F + f0 + fl2;
      float* o = per_ped ? per_ped + (sf * Nmax + n2) * 16 : nullptr;
      if (i < kRkRows) {
        const bool ok = i == kL || hinv[gi * kL + i].w != 0.f;
        int r = -1;
        if (ok) {
          r = 0;
          const uint32_t* cw = cmp + gi * K;
#pragma nounroll
          for (int kk = 0; kk < K; ++kk) r += (int)((cw[kk] >> i) & 1u);
          atomicAdd(&lh[i * B + r / binw], 1);
          atomicAdd(&lt[i == kL ? 3 : 2], r);
        }
        if (o) o[i] = (float)r;
      } else {
        int deg = 0;
#pragma unroll
        for (int t = 0; t < kL; ++t) deg += hinv[gi * kL + t].w != 0.f ? 0 : 1;
        atomicAdd(&lt[0], 1);
        if (deg) atomicAdd(&lt[1], deg);
        if (o) { o[kRkRows] = (float)deg; o[kRkRows + 1] = 0.f; o[kRkRows + 2] = 0.f; }
      }
    }
  }
  // the workgroup's rows
  __syncthreads();
  for (int i = tid; i < kRkRows * B; i += kRkThreads)
    hist_rows[(size_t)blockIdx.x * (kRkRows * B) + i] = lh[i];
  if (tid < 4) tot_rows[(size_t)blockIdx.x * 4 + tid] = (int64_t)lt[tid];
}

template <class Head>
int sample_ranks_launch(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* head_params, uint64_t seed, int K, int B, float* per_ped,
                        int32_t* hist, int64_t* tot, void* workspace, hipStream_t st) {
  if (d->F == 0) {
    // no frame: no kernel (its staging would read the head's parameters), zeros
    if (hipMemsetAsync(hist, 0, (size_t)d->S * kRkRows * B * 4, st) != hipSuccess ||
        hipMemsetAsync(tot, 0, (size_t)d->S * kRkTot * 8, st) != hipSuccess)
      return set_err(G2K_ELAUNCH, "%ssample_ranks: zeroing the outputs failed", Head::kPrefix);
    return G2K_OK;
  }
  DrawnLaunch L;
  if (const int rc = drawn_launch(d, drawn_geom(*d, K), seed, Head::kPrefix, "sample_ranks", L))
    return rc;
  const DrawnGeom& g = L.g;
  const int HB = kRkRows * B;
  // the workgroups' rows: tot [S * C][4] int64, then hist [S * C][13 B] int32
  int64_t* tot_rows = static_cast<int64_t*>(workspace);
  int32_t* hist_rows = reinterpret_cast<int32_t*>(tot_rows + L.wgs * kRkTot);
  const double scott = pow((double)(K + 1), -1.0 / 3.0);
  hipLaunchKernelGGL(sample_ranks_kernel<Head>, dim3((unsigned)L.wgs), dim3(kRkThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.FC, g.C, g.G,
                     K, B, L.seed_lo, L.seed_hi, L.shared_targets, scott, per_ped,
                     L.direct ? hist : hist_rows, L.direct ? tot : tot_rows);
  const int rc = check_launch("sample_ranks_kernel");
  if (rc || L.direct) return rc;
  return drawn_hist_rows<kRkTot, 0>(hist_rows, tot_rows, nullptr, d->S, g.C, HB, hist, tot, nullptr,
                                    st);
}

inline bool ranks_bins_ok(int32_t B) { return B >= 1 && B <= G2K_RANKS_BMAX; }

// one row (tot [4] int64, hist [13 B] int32) per (scene, chunk); FC >= 1 frame
// per chunk, so at most F chunks
int64_t ranks_ws_bytes(const g2k_dims* d, int32_t B) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * (4 * 8 + kRkRows * B * 4);
}

int check_ranks_k(int32_t K) {
  if (K < G2K_RANKS_KMIN || K > G2K_RANKS_KMAX)
    return set_err(G2K_EINVAL, "K=%d (%d..%d)", K, G2K_RANKS_KMIN, G2K_RANKS_KMAX);
  return G2K_OK;
}

// the argument checks, before any HIP call; G2K_OK with S > 0: launch
int ranks_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                   const void* n_active, const void* head, int32_t K, int32_t B, const void* per_ped,
                   const void* hist, const void* tot, const void* workspace,
                   int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "%s: flags %d (0 or G2K_STEP_TARGETS_SHARED)", name, d->flags);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_ranks_k(K)) return rc;
  if (!ranks_bins_ok(B) || (K + 1) % B)
    return set_err(G2K_EINVAL, "B=%d (1..%d, a divisor of K + 1 = %d)", B, G2K_RANKS_BMAX, K + 1);
  if (const int rc = check_required({pred, targets, n_active, head, hist, tot})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_per_ped(per_ped)) return rc;
  if (((uintptr_t)hist) & 3) return set_err(G2K_EINVAL, "hist must be 4-byte aligned");
  if (((uintptr_t)tot) & 7) return set_err(G2K_EINVAL, "tot must be 8-byte aligned");
  return check_workspace(d, workspace, workspace_bytes, ranks_ws_bytes(d, B), 8);   // rows of int64 first
}

template <class Head>
int sample_ranks(const char* name, const g2k_dims* d, const float* pred, const float* targets,
                 const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                 const float* head, uint64_t seed, int32_t K, int32_t B, float* per_ped,
                 int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                 void* stream) {
  const int rc = ranks_validate(name, d, pred, targets, n_active, head, K, B, per_ped, hist, tot,
                                workspace, workspace_bytes);
  if (rc || d->S == 0) return rc;
  return sample_ranks_launch<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K, B,
                                   per_ped, hist, tot, workspace, (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

int64_t g2k_sample_ranks_workspace_bytes(const g2k_dims* d, int32_t B) {
  if (!d || !pair_sizes_ok(d) || !ranks_bins_ok(B)) return -1;
  return ranks_ws_bytes(d, B);
}

// the launch geometry (drawn_geom: host arithmetic, no HIP call), as the
// launcher works it out
int g2k_sample_ranks_geometry(const g2k_dims* d, int32_t K, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_ranks_k(K)) return rc;
  return drawn_write_geom(drawn_geom(*d, K), K, kRkLdsBytes, out);
}

int g2k_sample_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames,
                         const uint8_t* ped_mask, const float* head, uint64_t seed, int32_t K,
                         int32_t B, float* per_ped, int32_t* hist, int64_t* tot, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  return sample_ranks<PerStepHead>("sample_ranks", d, pred, targets, n_active, n_frames, ped_mask,
                                   head, seed, K, B, per_ped, hist, tot, workspace, workspace_bytes,
                                   stream);
}

int g2k_fullcov_sample_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                                 const int32_t* n_active, const int32_t* n_frames,
                                 const uint8_t* ped_mask, const float* chol, uint64_t seed,
                                 int32_t K, int32_t B, float* per_ped, int32_t* hist, int64_t* tot,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  return sample_ranks<FullCovHead>("fullcov_sample_ranks", d, pred, targets, n_active, n_frames,
                                   ped_mask, chol, seed, K, B, per_ped, hist, tot, workspace,
                                   workspace_bytes, stream);
}

int g2k_mix_sample_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                             const int32_t* n_active, const int32_t* n_frames,
                             const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                             int32_t B, float* per_ped, int32_t* hist, int64_t* tot, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  return sample_ranks<MixHead>("mix_sample_ranks", d, pred, targets, n_active, n_frames, ped_mask,
                               mix, seed, K, B, per_ped, hist, tot, workspace, workspace_bytes, stream);
}

}  // extern "C"
