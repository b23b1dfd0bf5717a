// g2k_scene_modes.hip — fused k-medoid reduction of a probabilistic head's
// JOINT samples to M scene modes: per scene-frame the K joint draws clustered by
// their joint displacement distance (PAM BUILD, then alternating rounds), every
// mode one of the draws, and the modes scored against the targets (minJADE_M /
// minJFDE_M, the clusters' weights, the scene-level miss).  ONE kernel template,
// scene_modes_kernel<Head>, over the heads of g2k_head_draw.h
// (g2k_scene_modes_f32, g2k_fullcov_scene_modes_f32, g2k_mix_scene_modes_f32;
// g2k_coupled_scene_modes_f32 of include/g2k_coupled.h).  The C entry points
// are at the end of this file, declared in include/g2k_scene_modes.h (added
// after ABI 11: bound by symbol), which states the definition.  The build's:
// the reference has no probabilistic head, so PARITY UNPINNED; pinned against
// tests/scene_modes_ref.py.
//
// Every figure is double arithmetic on the fp32 draws in a stated order (the
// fma's are written out, under "fp contract(off)"), so repeated calls are
// bit-identical and the float64 restatement differs by summation order alone.
//
// Geometry: scene_ranks_kernel's (g2k_scene_ranks.hip), which this unit restates
// and leaves alone.  ONE workgroup of 256 lanes owns a scene-frame whatever P;
// the compacted members are walked in TILES of TM (16 for K <= 31, 8 above), a
// tile's K + 1 ITEMS (the K joint draws, then the targets) made once into LDS
// through the policy's draw, slot (member, item) of xy at (member (K + 1) +
// item) * 28 floats (24 used: the pitch keeps the pair loop's ds_read_b128 off
// one bank).  The K (K + 1) / 2 item pairs (j < l) are dealt to the lanes in
// the order p = l (l - 1) / 2 + j; a lane keeps its pairs' A (9 at most) as
// double accumulators in registers across the tiles — a root per member and
// step, twelve to a slot pair — and lane k < K the final-step sum Fn and
// maximum Mx of draw k against the targets; the loops over them are unrolled,
// no per-thread array is indexed at run time: no scratch.  After the last tile
// A goes to LDS (over xy) as a full (K + 1) x (K + 1) matrix and the clustering
// runs there: lane j is draw j (sums over k in ascending order), the argmin /
// argmax over the draws is a butterfly over wave 0 on (value, index), lane m <
// M is mode m in the medoid update.  Every loop bound and every break is
// uniform over the workgroup, so every barrier is met by all 256 lanes.
//   Every workgroup leaves one row of 88 + 8 M bytes in the caller's workspace
// (8 doubles, {P or 0, mA, mF, rounds, missed, 0}, the M medoids, the M
// counts); scene_mode_rows_kernel adds a scene's rows in frame order.  No float
// atomics, no waits between workgroups.
#include <cmath>

#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_coupled.h"
#include "g2k_head_draw.h"
#include "g2k_mix.h"
#include "g2k_scene_modes.h"

namespace g2k {
namespace {

constexpr int kSmThreads = 256;
constexpr int kSmKTall = 31;                  // K <= 31: TM = 16; above: TM = 8
constexpr int kSmSlots = 520;                 // item slots of a tile: TM (K + 1) at most
constexpr int kSmPitch = 28;                  // floats of a slot (24 used)
constexpr int kSmNI = G2K_SCENE_MODES_KMAX + 1;
constexpr int kSmMaxPairs = G2K_SCENE_MODES_KMAX * kSmNI / 2;                      // 2080
constexpr int kSmAPT = (kSmMaxPairs + kSmThreads - 1) / kSmThreads;                // 9
constexpr int kSmSums = G2K_SCENE_MODES_SUMS;
constexpr int kSmRowInts = 6;                 // P or 0, mA, mF, rounds, missed, 0
constexpr int kSmRowHead = kSmSums * 8 + kSmRowInts * 4;                           // 88
constexpr int kSmLdsBytes = kSmSlots * kSmPitch * 4 + kSmThreads * 4 + 4 * 4;
static_assert(16 * (kSmKTall + 1) <= kSmSlots && 8 * kSmNI <= kSmSlots, "a tile's items fit xy");
// what goes over xy after the last tile: A [NI][NI], Fn, Mx, dmin, cost [4][64] doubles, then
// asg [64], med, cnt, ch [3][32] ints
static_assert((kSmNI * kSmNI + 4 * 64) * 8 + (64 + 3 * 32) * 4 <= kSmSlots * kSmPitch * 4,
              "the end fits xy");

inline int sm_row_bytes(int M) { return kSmRowHead + 8 * M; }

struct SmGeom { int TM, DR, tiles, pairs, apt; };

inline SmGeom sm_geom(const g2k_dims& d, int K) {
  SmGeom g;
  g.TM = K <= kSmKTall ? 16 : 8;
  g.DR = kSmThreads / g.TM;
  g.tiles = (d.Nmax + g.TM - 1) / g.TM;
  g.pairs = K * (K + 1) / 2;
  g.apt = (g.pairs + kSmThreads - 1) / kSmThreads;
  return g;
}

__device__ __forceinline__ void sm_store(float* slot, const float (&x)[kL2]) {
  float4* o = reinterpret_cast<float4*>(slot);
#pragma unroll
  for (int q = 0; q < kL2 / 4; ++q) o[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}

// one step's displacement between two items: sqrt(fma(dy, dy, dx dx))
__device__ __forceinline__ double sm_e(float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
  const double dx = (double)ax - (double)bx;
  const double dy = (double)ay - (double)by;
  return sqrt(__builtin_fma(dy, dy, dx * dx));
}

// a slot against another, both time-major (6 ds_read_b128 each): 12 roots in step order
__device__ __forceinline__ double sm_path(const float* sa, const float* sb, double acc) {
#pragma clang fp contract(off)
  const float4* pa = reinterpret_cast<const float4*>(sa);
  const float4* pb = reinterpret_cast<const float4*>(sb);
#pragma unroll
  for (int u = 0; u < kL2 / 4; ++u) {
    const float4 a = pa[u], b = pb[u];
    acc = acc + sm_e(a.x, a.y, b.x, b.y);
    acc = acc + sm_e(a.z, a.w, b.z, b.w);
  }
  return acc;
}

// pair p = l (l - 1) / 2 + j, j < l
__device__ __forceinline__ void sm_pair(int p, int& j, int& l) {
  l = (int)((1.f + sqrtf(1.f + 8.f * (float)p)) * 0.5f);
  if (l * (l - 1) / 2 > p) --l;
  if ((l + 1) * l / 2 <= p) ++l;
  j = p - l * (l - 1) / 2;
}

// the best (value, index) over the 64 lanes of a wave, the lowest index on an exact tie; every
// lane gets it
template <bool kMax>
__device__ __forceinline__ int sm_wave_best(double v, int idx) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(idx, off);
    const bool better = kMax ? (ov > v || (ov == v && oi < idx)) : (ov < v || (ov == v && oi < idx));
    if (better) { v = ov; idx = oi; }
  }
  return idx;
}

template <class Head>
__global__ void __launch_bounds__(kSmThreads, 2) scene_modes_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int K, int M, int iters, int TM, uint32_t seed_lo, uint32_t seed_hi, int shared_targets,
    double miss_radius, unsigned char* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ typename Head::Lds hlds;
  __shared__ __attribute__((aligned(16))) float xy[kSmSlots * kSmPitch];
  __shared__ int midx[kSmThreads];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sfi = blockIdx.x;
  const int s = sfi / F, f = sfi - s * F;
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  const int rowb = kSmRowHead + 8 * M;
  unsigned char* row = rows + (size_t)sfi * rowb;
  double* rowd = reinterpret_cast<double*>(row);
  int32_t* rowi = reinterpret_cast<int32_t*>(row + kSmSums * 8);

  Head::template stage<kSmThreads>(head_params, hlds, tid);
  // compact the members: member i = column midx[i]
  bool mem = f < nf && tid < nact;
  if (mem && ped_mask) mem = ped_mask[(size_t)s * Nmax + tid] != 0;
  const unsigned long long bal = __ballot(mem);
  const int pre = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wcnt[wv] = __popcll(bal);
  __syncthreads();
  int base = 0, P = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int c = wcnt[v];
    if (v < wv) base += c;
    P += c;
  }
  if (mem) midx[base + pre] = tid;
  __syncthreads();
  if (P < 1) {                                             // uniform over the workgroup: not scored
    if (tid < rowb / 4) reinterpret_cast<int32_t*>(row)[tid] = 0;
    return;
  }
  Head head;
  head.bind(hlds);

  const int NI = K + 1;                                    // items: the draws, then the targets
  const int NP = K * NI / 2;                               // item pairs j < l
  const int m = tid & (TM - 1), kk = tid / TM;             // the lane's member slot and item of a round
  const int DR = kSmThreads / TM;
  const size_t sf = (size_t)sfi;
  const size_t tf = shared_targets ? (size_t)s : sf;
  // the lane's pairs p = tid + 256 i: (j, l) is worked out again where it is needed (a float root
  // against the 12 double roots of every member), which leaves the registers to the accumulators
  double acc[kSmAPT];
#pragma unroll
  for (int i = 0; i < kSmAPT; ++i) acc[i] = 0.0;
  double fn = 0.0, mx = 0.0;                               // lane k < K: draw k against the targets
  const int mstride = NI * kSmPitch;                       // floats from a member's slots to the next's

#pragma nounroll
  for (int m0 = 0; m0 < P; m0 += TM) {
    const int tc = P - m0 < TM ? P - m0 : TM;              // the tile's members
    const bool mon = m < tc;
    const int n = mon ? midx[m0 + m] : 0;
    const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;      // element of step 0
    float mu[kL2];
    if (mon) {
      const size_t pb = sf * kL2 * Nmax + n;               // load_mu_tg's means
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        mu[2 * t] = pred[pb + (size_t)t * Nmax];
        mu[2 * t + 1] = pred[pb + (size_t)(kL + t) * Nmax];
      }
    } else {
#pragma unroll
      for (int r = 0; r < kL2; ++r) mu[r] = 0.f;
    }
    // ---- the tile's items: item r0 + kk of member slot m ----
#pragma nounroll
    for (int r0 = 0; r0 < NI; r0 += DR) {
      const int k = r0 + kk;
      if (mon && k < NI) {
        float c[kL2];
        if (k < K) {
          const uint32_t lo = seed_lo + (uint32_t)k;       // (seed + k) mod 2^64
          const uint32_t hi = seed_hi + (lo < seed_lo ? 1u : 0u);
          head.draw(lo, hi, e0, n, Nmax, mu, [&](int t, float x, float y) {
            c[2 * t] = x; c[2 * t + 1] = y;
          });
        } else {
          const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf * Nmax + n) * kL;
#pragma unroll
          for (int t = 0; t < kL; ++t) {
            const float2 v = t2[t];
            c[2 * t] = v.x; c[2 * t + 1] = v.y;
          }
        }
        sm_store(xy + (m * NI + k) * kSmPitch, c);
      }
    }
    __syncthreads();
    // ---- the pairs: members ascending, steps ascending ----
#pragma unroll
    for (int i = 0; i < kSmAPT; ++i) {
      if (tid + i * kSmThreads < NP) {
        double a = acc[i];
        int j, l;
        sm_pair(tid + i * kSmThreads, j, l);
        const float* za = xy + j * kSmPitch;               // the items' slots of member 0
        const float* zb = xy + l * kSmPitch;
#pragma nounroll
        for (int mm = 0; mm < tc; ++mm) a = sm_path(za + mm * mstride, zb + mm * mstride, a);
        acc[i] = a;
      }
    }
    // ---- the final step of draw tid against the targets ----
    if (tid < K) {
      const float* za = xy + tid * kSmPitch + (kL2 - 2);
      const float* zb = xy + K * kSmPitch + (kL2 - 2);
#pragma nounroll
      for (int mm = 0; mm < tc; ++mm) {
        const float2 a = *reinterpret_cast<const float2*>(za + mm * mstride);
        const float2 b = *reinterpret_cast<const float2*>(zb + mm * mstride);
        const double e = sm_e(a.x, a.y, b.x, b.y);
        fn = fn + e;
        mx = e > mx ? e : mx;
      }
    }
    __syncthreads();                                       // xy is written again by the next tile
  }

  // ---- the end: the accumulators over xy ----
  double* dA = reinterpret_cast<double*>(xy);              // [NI][NI], symmetric, the diagonal 0
  double* dFn = dA + kSmNI * kSmNI;                        // [64]
  double* dMx = dFn + 64;                                  // [64]
  double* dMin = dMx + 64;                                 // [64] a draw's distance to its nearest medoid
  double* dC = dMin + 64;                                  // [64] a draw's sum within its cluster
  int* asg = reinterpret_cast<int*>(dC + 64);              // [64] a(k)
  int* med = asg + 64;                                     // [32]
  int* cnt = med + 32;                                     // [32]
  int* ch = cnt + 32;                                      // [32] the mode's medoid moved this round
#pragma unroll
  for (int i = 0; i < kSmAPT; ++i) {
    if (tid + i * kSmThreads < NP) {
      // opaque: formed here, not ahead of the tile loop and kept in registers across it
      int p = tid + i * kSmThreads, j, l;
      asm volatile("" : "+v"(p));
      sm_pair(p, j, l);
      dA[j * NI + l] = acc[i];
      dA[l * NI + j] = acc[i];
    }
  }
  if (tid < NI) dA[tid * NI + tid] = 0.0;
  if (tid < K) {
    dFn[tid] = fn;
    dMx[tid] = mx;
  }
  __syncthreads();
  const bool isk = tid < K;                                // lane j is draw j
  const double* arow = dA + (isk ? tid : 0) * NI;          // A(tid, .)
  const double kInf = __builtin_huge_val();

  // ---- PAM BUILD ----
  if (tid < 64) {
    double rs = kInf;
    if (isk) {
      rs = 0.0;
      for (int k = 0; k < K; ++k) rs = rs + arow[k];
    }
    const int b = sm_wave_best<false>(rs, tid);
    if (tid == 0) med[0] = b;
  }
  __syncthreads();
  bool chosen = false;
  double dm = 0.0;
  if (isk) {
    const int b = med[0];
    dm = arow[b];
    dMin[tid] = dm;
    chosen = tid == b;
  }
  __syncthreads();
#pragma nounroll
  for (int i = 1; i < M; ++i) {
    if (tid < 64) {
      double g = -kInf;
      if (isk && !chosen) {
        g = 0.0;
        for (int k = 0; k < K; ++k) {
          const double v = dMin[k] - arow[k];
          g = g + (v > 0.0 ? v : 0.0);
        }
      }
      const int b = sm_wave_best<true>(g, tid);
      if (tid == 0) med[i] = b;
    }
    __syncthreads();
    if (isk) {
      const int b = med[i];
      const double v = arow[b];
      dm = v < dm ? v : dm;
      dMin[tid] = dm;
      chosen = chosen || tid == b;
    }
    __syncthreads();
  }

  // ---- the alternating rounds ----
  int rounds = 0;
#pragma nounroll
  for (int it = 0; it < iters; ++it) {
    int a = 0;
    if (isk) {
      double best = arow[med[0]];
      for (int q = 1; q < M; ++q) {
        const double v = arow[med[q]];
        if (v < best) { best = v; a = q; }
      }
      asg[tid] = a;
    }
    __syncthreads();
    if (isk) {
      double c = 0.0;
      for (int k = 0; k < K; ++k)
        if (asg[k] == a) c = c + arow[k];
      dC[tid] = c;
    }
    __syncthreads();
    if (tid < M) {
      double best = 0.0;
      int bj = -1;
      for (int j = 0; j < K; ++j) {
        if (asg[j] == tid) {
          const double c = dC[j];
          if (bj < 0 || c < best) { best = c; bj = j; }
        }
      }
      const bool moved = bj >= 0 && bj != med[tid];
      if (moved) med[tid] = bj;
      ch[tid] = moved ? 1 : 0;
    }
    __syncthreads();
    int any = 0;
    for (int q = 0; q < M; ++q) any |= ch[q];
    ++rounds;
    if (!any) break;                                       // uniform: every lane read the same flags
    __syncthreads();                                       // ch is written again by the next round
  }
  __syncthreads();

  // ---- the final assignment ----
  if (isk) {
    int a = 0;
    double best = arow[med[0]];
    for (int q = 1; q < M; ++q) {
      const double v = arow[med[q]];
      if (v < best) { best = v; a = q; }
    }
    asg[tid] = a;
    dC[tid] = best;                                        // A(k, med_a(k))
  }
  __syncthreads();
  int32_t* rmed = rowi + kSmRowInts;
  int32_t* rcnt = rmed + M;
  if (tid < M) {
    int c = 0;
    for (int k = 0; k < K; ++k) c += asg[k] == tid ? 1 : 0;
    cnt[tid] = c;
    rmed[tid] = med[tid];
    rcnt[tid] = c;
  }
  __syncthreads();

  // ---- the scoring ----
  const double p12 = (double)(12 * P);
  if (tid == 0) {
    int mA = 0, mF = 0;
    double bA = dA[med[0] * NI + K], bF = dFn[med[0]], bM = dMx[med[0]];
    for (int q = 1; q < M; ++q) {
      const int b = med[q];
      const double vA = dA[b * NI + K], vF = dFn[b], vM = dMx[b];
      if (vA < bA) { bA = vA; mA = q; }
      if (vF < bF) { bF = vF; mF = q; }
      bM = vM < bM ? vM : bM;
    }
    rowd[0] = bA / p12;
    rowd[1] = bF / (double)P;
    rowd[2] = (double)cnt[mA] / (double)K;
    rowd[3] = (double)cnt[mF] / (double)K;
    rowd[7] = bM;
    rowi[0] = P;
    rowi[1] = mA;
    rowi[2] = mF;
    rowi[3] = rounds;
    rowi[4] = bM > miss_radius ? 1 : 0;
    rowi[5] = 0;
  } else if (tid == 64) {
    double c = 0.0;
    for (int k = 0; k < K; ++k) c = c + dC[k];
    rowd[4] = c / (double)(12 * K * P);
  } else if (tid == 128) {
    double raw = dA[K], all;
    for (int k = 1; k < M; ++k) {
      const double v = dA[k * NI + K];
      raw = v < raw ? v : raw;
    }
    all = raw;
    for (int k = M; k < K; ++k) {
      const double v = dA[k * NI + K];
      all = v < all ? v : all;
    }
    rowd[5] = raw / p12;
    rowd[6] = all / p12;
  }
}

// Column j of a scene's rows, the frames in frame order: j < 8 the sums, then the four totals,
// then the M medoids and the M counts (copied, frame by frame).
__global__ void __launch_bounds__(256) scene_mode_rows_kernel(
    const unsigned char* __restrict__ rows, int S, int F, int M, int32_t* __restrict__ per_frame_i,
    double* __restrict__ per_frame_d, int32_t* __restrict__ medoids, int32_t* __restrict__ counts,
    double* __restrict__ sums, long long* __restrict__ tot) {
#pragma clang fp contract(off)
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per = kSmSums + G2K_SCENE_MODES_TOT + 2 * M;
  if (id >= (int64_t)S * per) return;
  const int64_t s = id / per;
  const int j = (int)(id - s * per);
  const int rowb = kSmRowHead + 8 * M;
  const unsigned char* r0 = rows + (size_t)s * F * rowb;
  if (j < kSmSums) {
    double all = 0.0;
    for (int f = 0; f < F; ++f) {
      const unsigned char* r = r0 + (size_t)f * rowb;
      const double v = reinterpret_cast<const double*>(r)[j];
      const int P = reinterpret_cast<const int32_t*>(r + kSmSums * 8)[0];
      if (per_frame_d) per_frame_d[((size_t)s * F + f) * kSmSums + j] = v;
      double term = 0.0;
      if (j == 2 || j == 3) {
        const double t = 1.0 - v;
        term = P > 0 ? t * t : 0.0;
      } else if (j < 7) {
        term = (double)P * v;
      }
      all = all + term;
    }
    sums[s * kSmSums + j] = all;
  } else if (j < kSmSums + G2K_SCENE_MODES_TOT) {
    const int col = j - kSmSums;
    long long all = 0;
    for (int f = 0; f < F; ++f) {
      const int32_t* ri = reinterpret_cast<const int32_t*>(r0 + (size_t)f * rowb + kSmSums * 8);
      if (per_frame_i) per_frame_i[((size_t)s * F + f) * G2K_SCENE_MODES_TOT + col] = ri[col];
      all += col == 0 ? (ri[0] > 0 ? 1 : 0) : col == 1 ? ri[0] : col == 2 ? ri[4] : ri[3];
    }
    tot[s * G2K_SCENE_MODES_TOT + col] = all;
  } else {
    const int c = j - kSmSums - G2K_SCENE_MODES_TOT;      // c < M: medoid c; above: count c - M
    int32_t* dst = c < M ? medoids : counts;
    if (!dst) return;
    const int q = c < M ? c : c - M;
    for (int f = 0; f < F; ++f) {
      const int32_t* ri = reinterpret_cast<const int32_t*>(r0 + (size_t)f * rowb + kSmSums * 8);
      dst[((size_t)s * F + f) * M + q] = ri[kSmRowInts + c];
    }
  }
}

template <class Head>
int scene_modes_launch(const g2k_dims* d, const float* pred, const float* targets,
                       const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                       const float* head_params, uint64_t seed, int K, int M, int iters,
                       float miss_radius, int32_t* per_frame_i, double* per_frame_d, int32_t* medoids,
                       int32_t* counts, double* sums, int64_t* tot, unsigned char* rows,
                       hipStream_t st) {
  const SmGeom g = sm_geom(*d, K);
  const int64_t units = (int64_t)d->S * d->F;
  if (units > 0x7fffffff)
    return set_err(G2K_EINVAL, "%sscene_modes: %lld workgroups", Head::kPrefix, (long long)units);
  if (units > 0) {
    const int shared = (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0;
    hipLaunchKernelGGL((scene_modes_kernel<Head>), dim3((unsigned)units), dim3(kSmThreads), 0, st, pred,
                       targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, K, M, iters,
                       g.TM, (uint32_t)seed, (uint32_t)(seed >> 32), shared, (double)miss_radius, rows);
    const int rc = check_launch("scene_modes_kernel");
    if (rc) return rc;
  }
  const int64_t ids = (int64_t)d->S * (kSmSums + G2K_SCENE_MODES_TOT + 2 * M);
  hipLaunchKernelGGL(scene_mode_rows_kernel, dim3((unsigned)((ids + 255) / 256)), dim3(256), 0, st, rows,
                     d->S, d->F, M, per_frame_i, per_frame_d, medoids, counts, sums,
                     reinterpret_cast<long long*>(tot));
  return check_launch("scene_mode_rows_kernel");
}

inline bool sm_m_ok(int32_t M) { return M >= 1 && M <= G2K_SCENE_MODES_MMAX; }
inline bool sm_k_ok(int32_t K, int32_t M) {
  return K >= (M > G2K_SCENE_MODES_KMIN ? M : G2K_SCENE_MODES_KMIN) && K <= G2K_SCENE_MODES_KMAX;
}

int check_sm_mk(int32_t K, int32_t M) {
  if (!sm_m_ok(M)) return set_err(G2K_EINVAL, "M=%d (1..%d)", M, G2K_SCENE_MODES_MMAX);
  if (!sm_k_ok(K, M))
    return set_err(G2K_EINVAL, "K=%d (%d..%d)", K, M > G2K_SCENE_MODES_KMIN ? M : G2K_SCENE_MODES_KMIN,
                   G2K_SCENE_MODES_KMAX);
  return G2K_OK;
}

// one row of 88 + 8 M bytes per scene-frame
int64_t sm_ws_bytes(const g2k_dims* d, int M) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * sm_row_bytes(M);
}

int check_align(const void* p, int align, const char* what) {
  if (((uintptr_t)p) & (uintptr_t)(align - 1))
    return set_err(G2K_EINVAL, "%s must be %d-byte aligned", what, align);
  return G2K_OK;
}

// the argument checks, before any HIP call; G2K_OK with S > 0: launch
int sm_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                const void* n_active, const void* head, int32_t K, int32_t M, int32_t iters,
                float miss_radius, const void* per_frame_i, const void* per_frame_d, const void* medoids,
                const void* counts, const void* sums, const void* tot, const void* workspace,
                int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "%s: flags %d (0 or G2K_STEP_TARGETS_SHARED)", name, d->flags);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_sm_mk(K, M)) return rc;
  if (iters < 0 || iters > G2K_SCENE_MODES_ITERS_MAX)
    return set_err(G2K_EINVAL, "iters=%d (0..%d)", iters, G2K_SCENE_MODES_ITERS_MAX);
  if (!(miss_radius >= 0.f) || !std::isfinite(miss_radius))
    return set_err(G2K_EINVAL, "miss_radius=%g (finite, >= 0)", (double)miss_radius);
  if (const int rc = check_required({pred, targets, n_active, head, sums, tot})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_align(per_frame_i, 4, "per_frame_i")) return rc;
  if (const int rc = check_align(per_frame_d, 8, "per_frame_d")) return rc;
  if (const int rc = check_align(medoids, 4, "medoids")) return rc;
  if (const int rc = check_align(counts, 4, "counts")) return rc;
  if (const int rc = check_align(sums, 8, "sums")) return rc;
  if (const int rc = check_align(tot, 8, "tot")) return rc;
  return check_workspace(d, workspace, workspace_bytes, sm_ws_bytes(d, M), 8);   // rows of doubles
}

template <class Head>
int scene_modes(const char* name, const g2k_dims* d, const float* pred, const float* targets,
                const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                const float* head, uint64_t seed, int32_t K, int32_t M, int32_t iters,
                float miss_radius, int32_t* per_frame_i, double* per_frame_d, int32_t* medoids,
                int32_t* counts, double* sums, int64_t* tot, void* workspace, int64_t workspace_bytes,
                void* stream) {
  const int rc = sm_validate(name, d, pred, targets, n_active, head, K, M, iters, miss_radius,
                             per_frame_i, per_frame_d, medoids, counts, sums, tot, workspace,
                             workspace_bytes);
  if (rc || d->S == 0) return rc;
  return scene_modes_launch<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K, M, iters,
                                  miss_radius, per_frame_i, per_frame_d, medoids, counts, sums, tot,
                                  static_cast<unsigned char*>(workspace), (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

// the heads share the geometry, so the workspace too
int64_t g2k_scene_modes_workspace_bytes(const g2k_dims* d, int32_t K, int32_t M) {
  if (!d || !pair_sizes_ok(d) || !sm_m_ok(M) || !sm_k_ok(K, M)) return -1;
  return sm_ws_bytes(d, M);
}

// the launch geometry (sm_geom: host arithmetic, no HIP call), as the launcher works it out
int g2k_scene_modes_geometry(const g2k_dims* d, int32_t K, int32_t M, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_sm_mk(K, M)) return rc;
  if (!out) return set_err(G2K_EINVAL, "out is NULL");
  const SmGeom g = sm_geom(*d, K);
  out[G2K_SCENE_MODES_GEOM_TM] = g.TM;
  out[G2K_SCENE_MODES_GEOM_DR] = g.DR;
  out[G2K_SCENE_MODES_GEOM_TILES] = g.tiles;
  out[G2K_SCENE_MODES_GEOM_W] = 1;
  out[G2K_SCENE_MODES_GEOM_PAIRS] = g.pairs;
  out[G2K_SCENE_MODES_GEOM_APT] = g.apt;
  out[G2K_SCENE_MODES_GEOM_ROW_BYTES] = sm_row_bytes(M);
  out[G2K_SCENE_MODES_GEOM_LDS_BYTES] = kSmLdsBytes;
  return G2K_OK;
}

#define G2K_SM_ARGS                                                                                   \
  const g2k_dims *d, const float *pred, const float *targets, const int32_t *n_active,                \
      const int32_t *n_frames, const uint8_t *ped_mask, const float *head, uint64_t seed, int32_t K,  \
      int32_t M, int32_t iters, float miss_radius, int32_t *per_frame_i, double *per_frame_d,         \
      int32_t *medoids, int32_t *counts, double *sums, int64_t *tot, void *workspace,                 \
      int64_t workspace_bytes, void *stream
#define G2K_SM_PASS                                                                                   \
  d, pred, targets, n_active, n_frames, ped_mask, head, seed, K, M, iters, miss_radius, per_frame_i,  \
      per_frame_d, medoids, counts, sums, tot, workspace, workspace_bytes, stream

int g2k_scene_modes_f32(G2K_SM_ARGS) { return scene_modes<PerStepHead>("scene_modes", G2K_SM_PASS); }

int g2k_fullcov_scene_modes_f32(G2K_SM_ARGS) {
  return scene_modes<FullCovHead>("fullcov_scene_modes", G2K_SM_PASS);
}

int g2k_mix_scene_modes_f32(G2K_SM_ARGS) { return scene_modes<MixHead>("mix_scene_modes", G2K_SM_PASS); }

int g2k_coupled_scene_modes_f32(G2K_SM_ARGS) {
  return scene_modes<CoupledHead>("coupled_scene_modes", G2K_SM_PASS);
}

#undef G2K_SM_ARGS
#undef G2K_SM_PASS

}  // extern "C"
