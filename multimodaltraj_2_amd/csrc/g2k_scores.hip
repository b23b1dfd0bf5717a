// g2k_scores.hip — fused trajectory-level scores of a probabilistic head's
// samples: the energy score's two terms (with the ADE, the FDE and the 24-D
// norm), the APD and the variogram score of order 1/2.  ONE kernel,
// sample_scores_kernel<Head>, instantiated for the per-step head
// (g2k_sample_scores_f32), the full-covariance head
// (g2k_fullcov_sample_scores_f32) and the mixture head
// (g2k_mix_sample_scores_f32); the heads are the policies of g2k_head_draw.h.
// The C entry points are at the end of this file, declared in
// include/g2k_scores.h (added after ABI 11: bound by symbol).  The build's: the
// reference has no probabilistic head, so PARITY UNPINNED; pinned against
// tests/scores_ref.py.
//
// Definition.  Inputs and pairs as g2k_best_of_k_f32 (g2k_bestk.hip), K in
// [2, 256].  Draw k = what the head's sampler writes for seed (seed + k) mod
// 2^64.  X_k(t) draw k's position at step t, Y(t) the target; for two
// trajectories A, B:
//   a(A, B) = 1/12 sum_t ||A(t) - B(t)||    f(A, B) = ||A(11) - B(11)||
//   r(A, B) = ||A - B|| over the 24 coordinates
// per_ped [S, F, Nmax, 8] (or NULL), per pair:
//   0..2  mA, mF, mR = 1/K sum_k {a, f, r}(X_k, Y)
//   3..5  pA, pF, pR = 2/(K (K - 1)) sum_{k<l} {a, f, r}(X_k, X_l)
//   6     vs = sum_{t<u} (||Y(t) - Y(u)||^(1/2) - 1/K sum_k ||X_k(t) - X_k(u)||^(1/2))^2
//   7     0
// zeros for non-pairs, every element written; out [S, 8] = the sums of columns
// 0..6 over the scene's pairs and the pair count, fixed summation order, no
// atomics.  The host forms es_traj = mR - pR / 2 (the fair energy score of the
// 24-D law), es_ade = mA - pA / 2, es_fde = mF - pF / 2.
//
// Geometry and pass scaffold: the drawn-once family's (g2k_drawn.h) — every
// couple of a pair's K draws is compared, so the draws are all live at once,
// xy[slot][24] (time-major; a pitch of 28 floats, which spreads the 16 lanes
// of a ds_read_b128 group over 16 different bank quads where 24 collides two
// ways, measured the same to within 1 %: DESIGN.md §6j — the walk is not bound
// by LDS reads).  Per pass, three barriers:
//   draw     the lane draws X_k into registers, takes a, f, r against the
//            target and stores X_k in its slot
//   couples  the lane walks the partners l = k + 1, ..., k + h (mod K) from
//            LDS, 6 ds_read_b128 each, the circular half range
//            (drawn_partners).  The lane's six sums go to val[6][256]
//   items    72 items per pair dealt to the 256 lanes: 66 step pairs (t, u),
//            each a walk over the K slots (2 ds_read_b64 and two square roots
//            per draw) and the squared difference from the target's variogram;
//            6 column sums over the K lanes' val entries, in k order
//   finish   one lane per pair adds the 66 terms in order, scales the six sums
//            and writes the pair's 8 figures
// The 32-pair cap is the LDS budget (the items' rows [32][73] and, for the
// mixture head, 19 KB of factors next to the 24 KB of draws: 58 KB); it leaves
// lanes idle only below K = 8.  Square roots: sqrtf against the target (as
// g2k_bestk.hip), v_sqrt_f32 (1 ulp) among the draws and in the variogram.
// Scene sums: per-workgroup rows [S * C][8] in the caller's workspace, then
// drawn_rows8_kernel adds a scene's C rows in chunk order; C == 1 writes out
// directly.
#include "g2k_drawn.h"

namespace g2k {
namespace {

constexpr int kScThreads = kDrThreads, kScMaxG = kDrMaxG, kScPitch = kDrPitch;
constexpr int kScStepPairs = kL * (kL - 1) / 2;   // 66
constexpr int kScItems = kScStepPairs + 6;    // per pair: the step pairs, then the six column sums
constexpr int kScVtPitch = kScItems + 1;      // odd: the finishing lanes' reads do not collide
constexpr int kScLdsBytes = (kScThreads * kScPitch + 6 * kScThreads + kScMaxG * kScVtPitch + 4 * 8) * 4;

__device__ __forceinline__ float sqrt_ulp(float x) { return __builtin_amdgcn_sqrtf(x); }

template <class Head>
__global__ void __launch_bounds__(kScThreads) sample_scores_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int FC, int C, int G, int K, uint32_t seed_lo, uint32_t seed_hi, int shared_targets, float invK,
    float invKK, float* __restrict__ per_ped, float* __restrict__ rows) {
  __shared__ typename Head::Lds hlds;
  __shared__ __attribute__((aligned(16))) float xy[kScThreads * kScPitch];
  __shared__ float val[6][kScThreads];
  __shared__ float vt[kScMaxG * kScVtPitch];
  __shared__ float part[kScThreads / 64][8];
  const int tid = threadIdx.x;
  const DrawnChunk ch = drawn_chunk(n_active, n_frames, ped_mask, F, Nmax, FC, C);
  const int s = ch.s, f0 = ch.f0, nact = ch.nact;
  const uint8_t* mask = ch.mask;

  Head::template stage<kScThreads>(head_params, hlds, tid);
  if (per_ped) drawn_zero_per_ped<2>(ch, per_ped, tid);
  __syncthreads();
  Head head;
  head.bind(hlds);

  const DrawnLane ln = drawn_lane(tid, K, seed_lo, seed_hi);
  const int npairs = drawn_npairs(ch);
  const int g = ln.g, k = ln.k;
  const int h = drawn_partners(K, k);
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma nounroll
  for (int base = 0; base < npairs; base += G) {           // uniform trip count
    // ---- draw ----
    const DrawnItem it = drawn_item(ch, base, G, g);
    const int gp = it.gp;
    const bool on = it.on;
    float x[kL2];
    float ta = 0.f, tf = 0.f, tr = 0.f;
    if (on) {
      const size_t sf = drawn_frame(ch, it.fl);
      const int64_t e0 = drawn_elem0(ch, sf, it.n);        // element of step 0
      float mu[kL2], tg[kL2];
      load_mu_tg(true, pred, targets, sf, shared_targets ? (size_t)s : sf, it.n, Nmax, mu, tg);
      head.draw(ln.lo, ln.hi, e0, it.n, Nmax, mu, [&](int t, float px, float py) {
        x[2 * t] = px;
        x[2 * t + 1] = py;
        const float dx = px - tg[2 * t], dy = py - tg[2 * t + 1];
        const float d2 = fmaf(dx, dx, dy * dy);
        tf = sqrtf(d2);
        ta += tf;
        tr += d2;
      });
      tr = sqrtf(tr);
      store_draw(xy + tid * kScPitch, x);
    } else {
      zero_draw(x);
    }
    __syncthreads();
    // ---- couples ----
    float pa = 0.f, pf = 0.f, pr = 0.f;
    if (on) {
      int l = k;
#pragma nounroll
      for (int j = 0; j < h; ++j) {
        l = l + 1 == K ? 0 : l + 1;
        const float4* q4 = reinterpret_cast<const float4*>(xy + (g * K + l) * kScPitch);
        float r2 = 0.f, sa = 0.f, last = 0.f;
#pragma unroll
        for (int q = 0; q < kL2 / 4; ++q) {
          const float4 v = q4[q];
          const float ax = x[4 * q] - v.x, ay = x[4 * q + 1] - v.y;
          const float bx = x[4 * q + 2] - v.z, by = x[4 * q + 3] - v.w;
          const float a2 = fmaf(ax, ax, ay * ay), b2 = fmaf(bx, bx, by * by);
          last = sqrt_ulp(b2);
          sa += sqrt_ulp(a2) + last;
          r2 += a2 + b2;
        }
        pa += sa;
        pf += last;
        pr += sqrt_ulp(r2);
      }
    }
    val[0][tid] = ta; val[1][tid] = tf; val[2][tid] = tr;
    val[3][tid] = pa; val[4][tid] = pf; val[5][tid] = pr;
    __syncthreads();
    // ---- items ----
    for (int idx = tid; idx < gp * kScItems; idx += kScThreads) {
      const int gi = idx / kScItems, i = idx - gi * kScItems;
      const int pp = base + gi;
      const int fl2 = pp / nact, n2 = pp - fl2 * nact;
      float v = 0.f;
      if (mask ? mask[n2] != 0 : true) {
        const int slot0 = gi * K;
        float sum = 0.f;
        if (i < kScStepPairs) {
          int t = 0, r = i;                                // item i = the i-th (t, u), t < u
          while (r >= kL - 1 - t) { r -= kL - 1 - t; ++t; }
          const int u = t + 1 + r;
          const float* row = xy + slot0 * kScPitch;
#pragma nounroll
          for (int kk = 0; kk < K; ++kk) {
            const float2 a = *reinterpret_cast<const float2*>(row + kk * kScPitch + 2 * t);
            const float2 b = *reinterpret_cast<const float2*>(row + kk * kScPitch + 2 * u);
            const float dx = a.x - b.x, dy = a.y - b.y;
            sum += sqrt_ulp(sqrt_ulp(fmaf(dx, dx, dy * dy)));
          }
          const size_t tf2 = shared_targets ? (size_t)s : (size_t)s * F + f0 + fl2;
          const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf2 * Nmax + n2) * kL;
          const float2 ya = t2[t], yb = t2[u];
          const float dx = ya.x - yb.x, dy = ya.y - yb.y;
          const float e = sqrt_ulp(sqrt_ulp(fmaf(dx, dx, dy * dy))) - sum * invK;
          v = e * e;
        } else {
          const float* col = val[i - kScStepPairs] + slot0;
#pragma nounroll
          for (int kk = 0; kk < K; ++kk) sum += col[kk];
          v = sum;
        }
      }
      vt[gi * kScVtPitch + i] = v;
    }
    __syncthreads();
    // ---- finish: lane tid < gp takes pair base + tid (vt is next written after
    // the following pass's two barriers)
    if (tid < gp) {
      const int pp = base + tid;
      const int fl3 = pp / nact, n3 = pp - fl3 * nact;
      if (mask ? mask[n3] != 0 : true) {
        const float* w = vt + tid * kScVtPitch;
        float vs = 0.f;
#pragma unroll 6
        for (int i = 0; i < kScStepPairs; ++i) vs += w[i];
        const float sa = invK * (1.0f / 12.0f), pa12 = invKK * (1.0f / 12.0f);
        const float4 m = make_float4(w[kScStepPairs] * sa, w[kScStepPairs + 1] * invK,
                                     w[kScStepPairs + 2] * invK, w[kScStepPairs + 3] * pa12);
        const float4 q = make_float4(w[kScStepPairs + 4] * invKK, w[kScStepPairs + 5] * invKK, vs, 0.f);
        if (per_ped) {
          const size_t sf = (size_t)s * F + f0 + fl3;
          float4* o = reinterpret_cast<float4*>(per_ped) + (sf * Nmax + n3) * 2;
          o[0] = m;
          o[1] = q;
        }
        acc[0] += m.x; acc[1] += m.y; acc[2] += m.z; acc[3] += m.w;
        acc[4] += q.x; acc[5] += q.y; acc[6] += q.z; acc[7] += 1.f;
      }
    }
  }
  // the workgroup's row: lanes by butterfly, waves in order
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float v = wave_sum(acc[i]);
    if ((tid & 63) == 0) part[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < 8)
    rows[(size_t)blockIdx.x * 8 + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

template <class Head>
int sample_scores_launch(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                         const float* head_params, uint64_t seed, int K, float* per_ped, float* out,
                         float* rows, hipStream_t st) {
  DrawnLaunch L;
  if (const int rc = drawn_launch(d, drawn_geom(*d, K), seed, Head::kPrefix, "sample_scores", L))
    return rc;
  const DrawnGeom& g = L.g;
  const float invK = (float)(1.0 / (double)K);
  const float invKK = (float)(2.0 / ((double)K * (double)(K - 1)));
  hipLaunchKernelGGL(sample_scores_kernel<Head>, dim3((unsigned)L.wgs), dim3(kScThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.FC, g.C, g.G,
                     K, L.seed_lo, L.seed_hi, L.shared_targets, invK, invKK, per_ped,
                     L.direct ? out : rows);
  const int rc = check_launch("sample_scores_kernel");
  if (rc || L.direct) return rc;
  return drawn_rows8(rows, d->S, g.C, out, st);
}

// one row [8] per (scene, chunk); FC >= 1 frame per chunk, so at most F chunks
int64_t scores_ws_bytes(const g2k_dims* d) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * 8 * 4;
}

int check_scores_k(int32_t K) {
  if (K < G2K_SCORES_KMIN || K > G2K_SCORES_KMAX)
    return set_err(G2K_EINVAL, "K=%d (%d..%d)", K, G2K_SCORES_KMIN, G2K_SCORES_KMAX);
  return G2K_OK;
}

// the argument checks, before any HIP call; G2K_OK with S > 0: launch
int scores_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                    const void* n_active, const void* head, int32_t K, const void* per_ped,
                    const void* out, const void* workspace, int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "%s: flags %d (0 or G2K_STEP_TARGETS_SHARED)", name, d->flags);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_scores_k(K)) return rc;
  if (const int rc = check_required({pred, targets, n_active, head, out})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_per_ped(per_ped)) return rc;
  return check_workspace(d, workspace, workspace_bytes, scores_ws_bytes(d), 4);   // rows of floats
}

template <class Head>
int sample_scores(const char* name, const g2k_dims* d, const float* pred, const float* targets,
                  const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                  const float* head, uint64_t seed, int32_t K, float* per_ped, float* out,
                  void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = scores_validate(name, d, pred, targets, n_active, head, K, per_ped, out, workspace,
                                 workspace_bytes);
  if (rc || d->S == 0) return rc;
  return sample_scores_launch<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K,
                                    per_ped, out, static_cast<float*>(workspace), (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

int64_t g2k_sample_scores_workspace_bytes(const g2k_dims* d) {
  if (!d || !pair_sizes_ok(d)) return -1;
  return scores_ws_bytes(d);
}

// the launch geometry (drawn_geom: host arithmetic, no HIP call), as the
// launcher works it out
int g2k_sample_scores_geometry(const g2k_dims* d, int32_t K, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_scores_k(K)) return rc;
  return drawn_write_geom(drawn_geom(*d, K), K, kScLdsBytes, out);
}

int g2k_sample_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames,
                          const uint8_t* ped_mask, const float* head, uint64_t seed, int32_t K,
                          float* per_ped, float* out, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  return sample_scores<PerStepHead>("sample_scores", d, pred, targets, n_active, n_frames, ped_mask,
                                    head, seed, K, per_ped, out, workspace, workspace_bytes, stream);
}

int g2k_fullcov_sample_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                                  const int32_t* n_active, const int32_t* n_frames,
                                  const uint8_t* ped_mask, const float* chol, uint64_t seed,
                                  int32_t K, float* per_ped, float* out, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  return sample_scores<FullCovHead>("fullcov_sample_scores", d, pred, targets, n_active, n_frames,
                                    ped_mask, chol, seed, K, per_ped, out, workspace, workspace_bytes,
                                    stream);
}

int g2k_mix_sample_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                              const int32_t* n_active, const int32_t* n_frames,
                              const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                              float* per_ped, float* out, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  return sample_scores<MixHead>("mix_sample_scores", d, pred, targets, n_active, n_frames, ped_mask,
                                mix, seed, K, per_ped, out, workspace, workspace_bytes, stream);
}

}  // extern "C"
