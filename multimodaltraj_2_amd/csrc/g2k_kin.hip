// g2k_kin.hip — fused kinematic scores of a probabilistic head's samples: 32
// scalar features of a trajectory (11 speeds, 10 accelerations, 10 longitudinal
// accelerations, the straightness), per pair the target's PIT rank among the K
// draws' and the two terms of the fair CRPS, per group of features.  ONE
// kernel, sample_kin_kernel<Head>, instantiated for the per-step head
// (g2k_sample_kin_f32), the full-covariance head (g2k_fullcov_sample_kin_f32)
// and the mixture head (g2k_mix_sample_kin_f32); the heads are the policies of
// g2k_head_draw.h.  The C entry points are at the end of this file, declared in
// include/g2k_kin.h (added after ABI 11: bound by symbol), which states the
// definition.  The build's: the reference has no probabilistic head, so PARITY
// UNPINNED; pinned against tests/kin_ref.py.
//
// The features are single fp32 operations in a stated order (kn_* below, under
// "fp contract(off)": no compiler setting can fuse a product into the add that
// follows it), so a rank, a comparison of two fp32 values, is an integer that
// the float32 restatement reproduces exactly.  The sums m, p, d, y are plain
// fp32 accumulations.
//
// Geometry and pass scaffold: the drawn-once family's (g2k_drawn.h), but for
// the draw stage.  A draw's positions are never kept: the step callback of the
// draw forms the features from the previous position, velocity and speed.  Of the
// 32 features 22 go to the slot, ft[slot][24] = {s_0..s_10, a_0..a_9, st, 0, 0}
// (96 B, ds_read_b128 aligned: the scores kernel's xy footprint); l_t is one
// exact subtraction of two stored speeds.  Per pass, five barriers:
//   draw     draw 0's lane forms the features of the pair's target from memory
//            (tgf), then every lane draws X_k, forms its features and stores
//            them in its slot
//   couples  the lane compares its features with the target's (32 bits in one
//            word, its terms of m and d), then walks the partners l = k + 1,
//            ..., k + h (mod K) from LDS, 6 ds_read_b128 each, the circular
//            half range (drawn_partners): its terms of p
//   terms    (the slots are dead) the lane leaves its 12 terms and its word in
//            its own slot: a val[13][256] next to the slots would put the
//            mixture head's workgroup above 64 KB
//   items    48 items per pair dealt to the 256 lanes: 32 rank counts, each a
//            walk over the K words in k order, which write the rank and bump
//            the workgroup's LDS histogram (integer atomics: the order cannot
//            show); 12 column sums over the K lanes' terms, in k order; the 4
//            group sums of the target's features
//   finish   one lane per pair scales the 16 sums and writes them
// Scene sums: per-workgroup rows in the caller's workspace (tot [S * C][8]
// int64, sums [S * C][16] f32, hist [S * C][32 B] int32), then
// drawn_hist_rows_kernel adds a scene's C rows in chunk order; C == 1 writes
// the outputs directly.
#include "g2k_drawn.h"

namespace g2k {
namespace {

constexpr int kKnThreads = kDrThreads, kKnMaxG = kDrMaxG, kKnPitch = kDrPitch;
constexpr int kKnRows = G2K_KIN_ROWS;         // 32 features
constexpr int kKnGroups = G2K_KIN_GROUPS;
constexpr int kKnCols = G2K_KIN_COLS;         // per_ped's columns
constexpr int kKnNS = kL - 1, kKnNA = kL - 2; // 11 speeds, 10 accelerations
constexpr int kKnOffA = kKnNS, kKnOffSt = kKnNS + kKnNA;   // in a slot: a at 11, st at 21
constexpr int kKnStored = kKnOffSt + 1;       // 22 floats of a slot are features
constexpr int kKnWord = 12;                   // the terms stage: 12 terms, then the rank bits
constexpr int kKnSums = 16;                   // m, p, d, y per group
constexpr int kKnItems = kKnRows + kKnSums;   // per pair: the rank counts, then the sums
constexpr int kKnVtPitch = kKnSums + 1;       // odd: the finishing lanes' reads do not collide
constexpr int kKnTot = 8;
constexpr int kKnLdsBytes = (kKnThreads * kKnPitch + kKnMaxG * kKnPitch + kKnMaxG * kKnVtPitch +
                             kKnRows * G2K_KIN_BMAX + kKnTot + (kKnThreads / 64) * kKnSums) * 4;

// ---- the features' arithmetic: one IEEE operation each, never contracted ----
__device__ __forceinline__ float kn_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float kn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
// sqrt(x x + y y): two products, one add, one correctly rounded square root
__device__ __forceinline__ float kn_norm(float x, float y) {
#pragma clang fp contract(off)
  const float xx = x * x;
  const float yy = y * y;
  const float q = xx + yy;
  return sqrtf(q);
}
// net / len, correctly rounded; 1 for a trajectory that never moves
__device__ __forceinline__ float kn_straight(float net, float len) {
#pragma clang fp contract(off)
  return len == 0.f ? 1.f : net / len;
}

// A trajectory's 22 stored features, formed step by step from the previous
// position, velocity and speed (t is a constant after unrolling: every index
// is one).
struct KinFeat {
  float f[kKnStored];
  float x0, y0, px, py, vx, vy, len;
  __device__ __forceinline__ void step(int t, float x, float y) {
    if (t == 0) {
      x0 = x; y0 = y;
    } else {
      const float nvx = kn_sub(x, px), nvy = kn_sub(y, py);
      const float s = kn_norm(nvx, nvy);
      f[t - 1] = s;
      if (t == 1) {
        len = s;
      } else {
        len = kn_add(len, s);
        f[kKnOffA + t - 2] = kn_norm(kn_sub(nvx, vx), kn_sub(nvy, vy));
      }
      vx = nvx; vy = nvy;
      if (t == kL - 1) f[kKnOffSt] = kn_straight(kn_norm(kn_sub(x, x0), kn_sub(y, y0)), len);
    }
    px = x; py = y;
  }
  __device__ __forceinline__ void store(float* slot) const {
    float4* o = reinterpret_cast<float4*>(slot);
#pragma unroll
    for (int q = 0; q < 5; ++q) o[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
    o[5] = make_float4(f[20], f[21], 0.f, 0.f);
  }
};

// the 22 stored features of a slot into registers
__device__ __forceinline__ void kn_load(const float* slot, float (&v)[kKnPitch]) {
  const float4* q4 = reinterpret_cast<const float4*>(slot);
#pragma unroll
  for (int q = 0; q < kKnPitch / 4; ++q) {
    const float4 w = q4[q];
    v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
  }
}

// the group of row j and the rows of group g
__device__ __forceinline__ int kn_group(int j) {
  return j < kKnNS ? 0 : j < kKnNS + kKnNA ? 1 : j < kKnNS + 2 * kKnNA ? 2 : 3;
}

template <class Head>
__global__ void __launch_bounds__(kKnThreads) sample_kin_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int FC, int C, int G, int K, int B, uint32_t seed_lo, uint32_t seed_hi, int shared_targets,
    float invK, float invKK, float* __restrict__ per_ped, float* __restrict__ sum_rows,
    int32_t* __restrict__ hist_rows, int64_t* __restrict__ tot_rows) {
  __shared__ typename Head::Lds hlds;
  __shared__ __attribute__((aligned(16))) float ft[kKnThreads * kKnPitch];
  __shared__ __attribute__((aligned(16))) float tgf[kKnMaxG * kKnPitch];   // the targets' features
  __shared__ float vt[kKnMaxG * kKnVtPitch];
  __shared__ int lh[kKnRows * G2K_KIN_BMAX];
  __shared__ int lt[kKnTot];
  __shared__ float part[kKnThreads / 64][kKnSums];
  const int tid = threadIdx.x;
  const DrawnChunk ch = drawn_chunk(n_active, n_frames, ped_mask, F, Nmax, FC, C);
  const int s = ch.s, f0 = ch.f0, nact = ch.nact;
  const uint8_t* mask = ch.mask;

  Head::template stage<kKnThreads>(head_params, hlds, tid);
  for (int i = tid; i < kKnRows * B; i += kKnThreads) lh[i] = 0;
  if (tid < kKnTot) lt[tid] = 0;
  if (per_ped) drawn_zero_per_ped<kKnCols / 4>(ch, per_ped, tid);
  __syncthreads();
  Head head;
  head.bind(hlds);

  const DrawnLane ln = drawn_lane(tid, K, seed_lo, seed_hi);
  const int npairs = drawn_npairs(ch);
  const int g = ln.g, k = ln.k;
  const int h = drawn_partners(K, k);
  const int binw = (K + 1) / B;                            // ranks per bin
  float acc[kKnSums];
#pragma unroll
  for (int i = 0; i < kKnSums; ++i) acc[i] = 0.f;
#pragma nounroll
  for (int base = 0; base < npairs; base += G) {           // uniform trip count
    // ---- draw: its own, not the family's (below) ----
    const DrawnItem it = drawn_item(ch, base, G, g);
    const int gp = it.gp, n = it.n;
    const bool on = it.on;
    KinFeat x;
    if (on) {
      const size_t sf = drawn_frame(ch, it.fl);
      const int64_t e0 = drawn_elem0(ch, sf, n);        // element of step 0
      // the target's features first, by draw 0's lane alone, and out of the
      // registers before the draw: 24 coordinates held across the draw (as
      // load_mu_tg would) put the full-covariance instantiation past 256 VGPRs
      if (k == 0) {
        const size_t tf = shared_targets ? (size_t)s : sf;
        const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf * Nmax + n) * kL;
        KinFeat y;
#pragma unroll
        for (int t = 0; t < kL; ++t) {
          const float2 v = t2[t];
          y.step(t, v.x, v.y);
        }
        y.store(tgf + g * kKnPitch);
      }
      float mu[kL2];
      {
        const size_t pb = sf * kL2 * Nmax + n;             // load_mu_tg's means
#pragma unroll
        for (int t = 0; t < kL; ++t) {
          mu[2 * t] = pred[pb + (size_t)t * Nmax];
          mu[2 * t + 1] = pred[pb + (size_t)(kL + t) * Nmax];
        }
      }
      head.draw(ln.lo, ln.hi, e0, n, Nmax, mu, [&](int t, float px, float py) { x.step(t, px, py); });
      x.store(ft + tid * kKnPitch);
    } else {
#pragma unroll
      for (int i = 0; i < kKnStored; ++i) x.f[i] = 0.f;
    }
    __syncthreads();
    // ---- couples: against the target, then the partners ----
    float tm[kKnGroups], tp[kKnGroups], td[kKnGroups];
#pragma unroll
    for (int i = 0; i < kKnGroups; ++i) { tm[i] = 0.f; tp[i] = 0.f; td[i] = 0.f; }
    uint32_t bits = 0;
    if (on) {
      float xl[kKnNA];                                     // the lane's longitudinal accelerations
#pragma unroll
      for (int j = 0; j < kKnNA; ++j) xl[j] = kn_sub(x.f[j + 1], x.f[j]);
      {
        float y[kKnPitch];
        kn_load(tgf + g * kKnPitch, y);
#pragma unroll
        for (int j = 0; j < kKnNS; ++j) {
          bits |= x.f[j] < y[j] ? 1u << j : 0u;
          tm[0] += fabsf(x.f[j] - y[j]);
          td[0] += x.f[j];
        }
#pragma unroll
        for (int j = 0; j < kKnNA; ++j) {
          const float xa = x.f[kKnOffA + j], ya = y[kKnOffA + j];
          bits |= xa < ya ? 1u << (kKnNS + j) : 0u;
          tm[1] += fabsf(xa - ya);
          td[1] += xa;
          const float yl = kn_sub(y[j + 1], y[j]);
          bits |= xl[j] < yl ? 1u << (kKnNS + kKnNA + j) : 0u;
          tm[2] += fabsf(xl[j] - yl);
          td[2] += xl[j];
        }
        bits |= x.f[kKnOffSt] < y[kKnOffSt] ? 1u << (kKnRows - 1) : 0u;
        tm[3] = fabsf(x.f[kKnOffSt] - y[kKnOffSt]);
        td[3] = x.f[kKnOffSt];
      }
      int l = k;
#pragma nounroll
      for (int j = 0; j < h; ++j) {
        l = l + 1 == K ? 0 : l + 1;
        float v[kKnPitch];
        kn_load(ft + (g * K + l) * kKnPitch, v);
        float ps = 0.f, pa = 0.f, pl = 0.f;
#pragma unroll
        for (int i = 0; i < kKnNS; ++i) ps += fabsf(x.f[i] - v[i]);
#pragma unroll
        for (int i = 0; i < kKnNA; ++i) {
          pa += fabsf(x.f[kKnOffA + i] - v[kKnOffA + i]);
          pl += fabsf(xl[i] - kn_sub(v[i + 1], v[i]));
        }
        tp[0] += ps;
        tp[1] += pa;
        tp[2] += pl;
        tp[3] += fabsf(x.f[kKnOffSt] - v[kKnOffSt]);
      }
    }
    __syncthreads();
    // ---- terms: the slots are dead; the lane's 12 terms and its word ----
    if (on) {
      float4* o = reinterpret_cast<float4*>(ft + tid * kKnPitch);
      o[0] = make_float4(tm[0], tm[1], tm[2], tm[3]);
      o[1] = make_float4(tp[0], tp[1], tp[2], tp[3]);
      o[2] = make_float4(td[0], td[1], td[2], td[3]);
      ft[tid * kKnPitch + kKnWord] = __uint_as_float(bits);
    }
    __syncthreads();
    // ---- items: item (pair, i); the rank counts, then the sums.  What they
    // read (ft, tgf) is next written after the following barrier
    for (int idx = tid; idx < gp * kKnItems; idx += kKnThreads) {
      const int gi = idx / kKnItems, i = idx - gi * kKnItems;
      const int pp = base + gi;
      const int fl2 = pp / nact, n2 = pp - fl2 * nact;
      if (!(mask ? mask[n2] != 0 : true)) continue;
      const float* slot0 = ft + gi * K * kKnPitch;
      if (i < kKnRows) {
        int r = 0;
#pragma nounroll
        for (int kk = 0; kk < K; ++kk)
          r += (int)((__float_as_uint(slot0[kk * kKnPitch + kKnWord]) >> i) & 1u);
        atomicAdd(&lh[i * B + r / binw], 1);
        atomicAdd(&lt[1 + kn_group(i)], r);
        if (per_ped) {
          const size_t sf = (size_t)s * F + f0 + fl2;
          per_ped[(sf * Nmax + n2) * kKnCols + i] = (float)r;
        }
      } else if (i < kKnRows + 12) {
        const float* col = slot0 + (i - kKnRows);
        float sum = 0.f;
#pragma nounroll
        for (int kk = 0; kk < K; ++kk) sum += col[kk * kKnPitch];
        vt[gi * kKnVtPitch + (i - kKnRows)] = sum;
      } else {
        const int gr = i - kKnRows - 12;                   // the target's group sum
        const float* y = tgf + gi * kKnPitch;
        float sum = 0.f;
        if (gr == 0) {
          for (int j = 0; j < kKnNS; ++j) sum += y[j];
          atomicAdd(&lt[0], 1);                            // the pair itself
        } else if (gr == 1) {
          for (int j = 0; j < kKnNA; ++j) sum += y[kKnOffA + j];
        } else if (gr == 2) {
          for (int j = 0; j < kKnNA; ++j) sum += kn_sub(y[j + 1], y[j]);
        } else {
          sum = y[kKnOffSt];
        }
        vt[gi * kKnVtPitch + 12 + gr] = sum;
      }
    }
    __syncthreads();
    // ---- finish: lane tid < gp takes pair base + tid (vt is next written after
    // the following pass's three barriers)
    if (tid < gp) {
      const int pp = base + tid;
      const int fl3 = pp / nact, n3 = pp - fl3 * nact;
      if (mask ? mask[n3] != 0 : true) {
        const float* w = vt + tid * kKnVtPitch;
        const float rn[kKnGroups] = {1.0f / kKnNS, 1.0f / kKnNA, 1.0f / kKnNA, 1.0f};
        float o16[kKnSums];
#pragma unroll
        for (int q = 0; q < kKnGroups; ++q) {
          o16[q] = w[q] * (invK * rn[q]);
          o16[4 + q] = w[4 + q] * (invKK * rn[q]);
          o16[8 + q] = w[8 + q] * (invK * rn[q]);
          o16[12 + q] = w[12 + q] * rn[q];
        }
        if (per_ped) {
          const size_t sf = (size_t)s * F + f0 + fl3;
          float4* o = reinterpret_cast<float4*>(per_ped + (sf * Nmax + n3) * kKnCols + kKnRows);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            o[q] = make_float4(o16[4 * q], o16[4 * q + 1], o16[4 * q + 2], o16[4 * q + 3]);
        }
#pragma unroll
        for (int i = 0; i < kKnSums; ++i) acc[i] += o16[i];
      }
    }
  }
  // the workgroup's rows: lanes by butterfly, waves in order
#pragma unroll
  for (int i = 0; i < kKnSums; ++i) {
    const float v = wave_sum(acc[i]);
    if ((tid & 63) == 0) part[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < kKnSums)
    sum_rows[(size_t)blockIdx.x * kKnSums + tid] =
        ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  for (int i = tid; i < kKnRows * B; i += kKnThreads)
    hist_rows[(size_t)blockIdx.x * (kKnRows * B) + i] = lh[i];
  if (tid < kKnTot) tot_rows[(size_t)blockIdx.x * kKnTot + tid] = (int64_t)lt[tid];
}

template <class Head>
int sample_kin_launch(const g2k_dims* d, const float* pred, const float* targets,
                      const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                      const float* head_params, uint64_t seed, int K, int B, float* per_ped,
                      float* sums, int32_t* hist, int64_t* tot, void* workspace, hipStream_t st) {
  if (d->F == 0) {
    // no frame: no kernel (its staging would read the head's parameters), zeros
    if (hipMemsetAsync(sums, 0, (size_t)d->S * kKnSums * 4, st) != hipSuccess ||
        hipMemsetAsync(hist, 0, (size_t)d->S * kKnRows * B * 4, st) != hipSuccess ||
        hipMemsetAsync(tot, 0, (size_t)d->S * kKnTot * 8, st) != hipSuccess)
      return set_err(G2K_ELAUNCH, "%ssample_kin: zeroing the outputs failed", Head::kPrefix);
    return G2K_OK;
  }
  DrawnLaunch L;
  if (const int rc = drawn_launch(d, drawn_geom(*d, K), seed, Head::kPrefix, "sample_kin", L))
    return rc;
  const DrawnGeom& g = L.g;
  const int HB = kKnRows * B;
  // the workgroups' rows: tot [S * C][8] int64, sums [S * C][16] f32, then hist
  // [S * C][32 B] int32
  int64_t* tot_rows = static_cast<int64_t*>(workspace);
  float* sum_rows = reinterpret_cast<float*>(tot_rows + L.wgs * kKnTot);
  int32_t* hist_rows = reinterpret_cast<int32_t*>(sum_rows + L.wgs * kKnSums);
  const float invK = (float)(1.0 / (double)K);
  const float invKK = (float)(2.0 / ((double)K * (double)(K - 1)));
  hipLaunchKernelGGL(sample_kin_kernel<Head>, dim3((unsigned)L.wgs), dim3(kKnThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.FC, g.C, g.G,
                     K, B, L.seed_lo, L.seed_hi, L.shared_targets, invK, invKK, per_ped,
                     L.direct ? sums : sum_rows, L.direct ? hist : hist_rows,
                     L.direct ? tot : tot_rows);
  const int rc = check_launch("sample_kin_kernel");
  if (rc || L.direct) return rc;
  return drawn_hist_rows<kKnTot, kKnSums>(hist_rows, tot_rows, sum_rows, d->S, g.C, HB, hist, tot,
                                          sums, st);
}

inline bool kin_bins_ok(int32_t B) { return B >= 1 && B <= G2K_KIN_BMAX; }

// one row (tot [8] int64, sums [16] f32, hist [32 B] int32) per (scene, chunk);
// FC >= 1 frame per chunk, so at most F chunks
int64_t kin_ws_bytes(const g2k_dims* d, int32_t B) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * (kKnTot * 8 + kKnSums * 4 + kKnRows * B * 4);
}

int check_kin_k(int32_t K) {
  if (K < G2K_KIN_KMIN || K > G2K_KIN_KMAX)
    return set_err(G2K_EINVAL, "K=%d (%d..%d)", K, G2K_KIN_KMIN, G2K_KIN_KMAX);
  return G2K_OK;
}

// the argument checks, before any HIP call; G2K_OK with S > 0: launch
int kin_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                 const void* n_active, const void* head, int32_t K, int32_t B, const void* per_ped,
                 const void* sums, const void* hist, const void* tot, const void* workspace,
                 int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "%s: flags %d (0 or G2K_STEP_TARGETS_SHARED)", name, d->flags);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_kin_k(K)) return rc;
  if (!kin_bins_ok(B) || (K + 1) % B)
    return set_err(G2K_EINVAL, "B=%d (1..%d, a divisor of K + 1 = %d)", B, G2K_KIN_BMAX, K + 1);
  if (const int rc = check_required({pred, targets, n_active, head, sums, hist, tot})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_per_ped(per_ped)) return rc;
  if (((uintptr_t)sums) & 3) return set_err(G2K_EINVAL, "sums must be 4-byte aligned");
  if (((uintptr_t)hist) & 3) return set_err(G2K_EINVAL, "hist must be 4-byte aligned");
  if (((uintptr_t)tot) & 7) return set_err(G2K_EINVAL, "tot must be 8-byte aligned");
  return check_workspace(d, workspace, workspace_bytes, kin_ws_bytes(d, B), 8);   // rows of int64 first
}

template <class Head>
int sample_kin(const char* name, const g2k_dims* d, const float* pred, const float* targets,
               const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
               const float* head, uint64_t seed, int32_t K, int32_t B, float* per_ped, float* sums,
               int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = kin_validate(name, d, pred, targets, n_active, head, K, B, per_ped, sums, hist, tot,
                              workspace, workspace_bytes);
  if (rc || d->S == 0) return rc;
  return sample_kin_launch<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K, B,
                                 per_ped, sums, hist, tot, workspace, (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

int64_t g2k_sample_kin_workspace_bytes(const g2k_dims* d, int32_t B) {
  if (!d || !pair_sizes_ok(d) || !kin_bins_ok(B)) return -1;
  return kin_ws_bytes(d, B);
}

// the launch geometry (drawn_geom: host arithmetic, no HIP call), as the
// launcher works it out
int g2k_sample_kin_geometry(const g2k_dims* d, int32_t K, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_kin_k(K)) return rc;
  return drawn_write_geom(drawn_geom(*d, K), K, kKnLdsBytes, out);
}

int g2k_sample_kin_f32(const g2k_dims* d, const float* pred, const float* targets,
                       const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                       const float* head, uint64_t seed, int32_t K, int32_t B, float* per_ped,
                       float* sums, int32_t* hist, int64_t* tot, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return sample_kin<PerStepHead>("sample_kin", d, pred, targets, n_active, n_frames, ped_mask, head,
                                 seed, K, B, per_ped, sums, hist, tot, workspace, workspace_bytes,
                                 stream);
}

int g2k_fullcov_sample_kin_f32(const g2k_dims* d, const float* pred, const float* targets,
                               const int32_t* n_active, const int32_t* n_frames,
                               const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                               int32_t B, float* per_ped, float* sums, int32_t* hist, int64_t* tot,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  return sample_kin<FullCovHead>("fullcov_sample_kin", d, pred, targets, n_active, n_frames, ped_mask,
                                 chol, seed, K, B, per_ped, sums, hist, tot, workspace,
                                 workspace_bytes, stream);
}

int g2k_mix_sample_kin_f32(const g2k_dims* d, const float* pred, const float* targets,
                           const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                           const float* mix, uint64_t seed, int32_t K, int32_t B, float* per_ped,
                           float* sums, int32_t* hist, int64_t* tot, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return sample_kin<MixHead>("mix_sample_kin", d, pred, targets, n_active, n_frames, ped_mask, mix,
                             seed, K, B, per_ped, sums, hist, tot, workspace, workspace_bytes, stream);
}

}  // extern "C"
