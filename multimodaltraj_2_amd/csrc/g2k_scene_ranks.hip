// g2k_scene_ranks.hip — fused scene-level rank calibration of a probabilistic
// head's JOINT samples: per scene-frame the targets' configuration pooled with
// the K joint draws and ranked among them by typicality, common mode and
// within-scene spread, and the two terms of the fair energy score of the
// scene's joint law from the same distance matrix.  ONE kernel template,
// scene_ranks_kernel<Head>, over the heads of g2k_head_draw.h
// (g2k_scene_ranks_f32, g2k_fullcov_scene_ranks_f32, g2k_mix_scene_ranks_f32;
// g2k_coupled_scene_ranks_f32 of include/g2k_coupled.h).  The C entry points
// are at the end of this file, declared in include/g2k_scene_ranks.h (added
// after ABI 11: bound by symbol), which states the definition.  The build's:
// the reference has no probabilistic head, so PARITY UNPINNED; pinned against
// tests/scene_ranks_ref.py.
//
// Every figure is double arithmetic on the fp32 draws in a stated order (the
// fma's are written out, under "fp contract(off)"), so repeated calls are
// bit-identical and the float64 restatement differs by summation order alone.
//
// Geometry.  A rank needs every member of its scene-frame, so ONE workgroup of
// 256 lanes owns a scene-frame whatever P.  The members are compacted as in
// joint_kernel (g2k_joint.hip) and walked in TILES of TM (16 for K <= 31, 8
// above: TM (K + 1) <= 520 item slots).  A tile's K + 1 ITEMS (the K joint
// draws, then the targets) are made once into LDS through the policy's draw,
// 256 / TM items to a round, lane (member tid % TM, item tid / TM): slot
// (member, item) of xy sits at (member (K + 1) + item) * 28 floats — no draw
// reaches global memory, and each serves K pair sums.  The slot pitch of 28
// dwords (24 used) is what keeps the pair loop's ds_read_b128 off one bank: the
// K (K + 1) / 2 item pairs (j < l) are dealt to the lanes in the order p =
// l (l - 1) / 2 + j, so the 16 lanes of a read group mostly share l (one
// address, a broadcast) and hold 16 different j whose slots, 28 j dwords
// apart, start on 16 different 4-bank slots of the 64 banks (28 j mod 64 takes
// 16 values; a pitch of 24 takes 8: two-way conflicts).  A lane keeps its pairs'
// D^2 (9 at most) and its share of the 25 (K + 1) sums s and q (7 at most) as
// double accumulators in registers across the tiles; the loops over them are
// unrolled, no per-thread array is indexed at run time: no scratch.  Only after
// the last tile the accumulators go to LDS (over xy), every lane takes the
// roots of its pairs, lane j the features of item j, then lanes 0..5 the
// ranks and the row's six doubles.
//   Every workgroup leaves one row of 64 bytes in the caller's workspace (6
// doubles, then {P or 0, r_typ, r_loc, r_spr}); scene_rows_kernel adds a
// scene's rows in frame order and counts the histograms.  No float atomics, no
// waits between workgroups.
#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_coupled.h"
#include "g2k_head_draw.h"
#include "g2k_mix.h"
#include "g2k_scene_ranks.h"

namespace g2k {
namespace {

constexpr int kSrThreads = 256;
constexpr int kSrKTall = 31;                  // K <= 31: TM = 16; above: TM = 8
constexpr int kSrSlots = 520;                 // item slots of a tile: TM (K + 1) at most
constexpr int kSrPitch = 28;                  // floats of a slot (24 used: see above)
constexpr int kSrNI = G2K_SCENE_RANKS_KMAX + 1;
constexpr int kSrMaxPairs = G2K_SCENE_RANKS_KMAX * kSrNI / 2;                      // 2080
constexpr int kSrAPT = (kSrMaxPairs + kSrThreads - 1) / kSrThreads;                // 9
constexpr int kSrAFT = (25 * kSrNI + kSrThreads - 1) / kSrThreads;                 // 7
constexpr int kSrSums = G2K_SCENE_RANKS_SUMS;
constexpr int kSrRowBytes = 64;               // 6 doubles, 4 int32
constexpr int kSrLdsBytes = kSrSlots * kSrPitch * 4 + 16 * kSrPitch * 4 + kSrThreads * 4 + 4 * 4;
static_assert(16 * (kSrKTall + 1) <= kSrSlots && 8 * kSrNI <= kSrSlots, "a tile's items fit xy");
// what goes over xy after the last tile: D [pairs], s and q [25 NI], t / loc / spr / u [4][NI]
static_assert((kSrMaxPairs + 25 * kSrNI + 4 * kSrNI) * 8 <= kSrSlots * kSrPitch * 4, "the end fits xy");

struct SceneGeom { int TM, DR, tiles, pairs, apt, aft; };

inline SceneGeom scene_geom(const g2k_dims& d, int K) {
  SceneGeom g;
  g.TM = K <= kSrKTall ? 16 : 8;
  g.DR = kSrThreads / g.TM;
  g.tiles = (d.Nmax + g.TM - 1) / g.TM;
  g.pairs = K * (K + 1) / 2;
  g.apt = (g.pairs + kSrThreads - 1) / kSrThreads;
  g.aft = (25 * (K + 1) + kSrThreads - 1) / kSrThreads;
  return g;
}

__device__ __forceinline__ void sr_store(float* slot, const float (&x)[kL2]) {
  float4* o = reinterpret_cast<float4*>(slot);
#pragma unroll
  for (int q = 0; q < kL2 / 4; ++q) o[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}

// one coordinate's term of a squared distance or of q: d = a - b, acc = fma(d, d, acc)
__device__ __forceinline__ double sr_sq(float a, float b, double acc) {
#pragma clang fp contract(off)
  const double d = (double)a - (double)b;
  return __builtin_fma(d, d, acc);
}

// a slot against another, both time-major (6 ds_read_b128 each): 24 terms in coordinate order
__device__ __forceinline__ double sr_dist2(const float* sa, const float* sb, double acc) {
  const float4* pa = reinterpret_cast<const float4*>(sa);
  const float4* pb = reinterpret_cast<const float4*>(sb);
#pragma unroll
  for (int u = 0; u < kL2 / 4; ++u) {
    const float4 a = pa[u], b = pb[u];
    acc = sr_sq(a.x, b.x, acc);
    acc = sr_sq(a.y, b.y, acc);
    acc = sr_sq(a.z, b.z, acc);
    acc = sr_sq(a.w, b.w, acc);
  }
  return acc;
}

template <class Head>
__global__ void __launch_bounds__(kSrThreads, 2) scene_ranks_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int K, int TM, uint32_t seed_lo, uint32_t seed_hi, int shared_targets,
    unsigned char* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ typename Head::Lds hlds;
  __shared__ __attribute__((aligned(16))) float xy[kSrSlots * kSrPitch];
  __shared__ __attribute__((aligned(16))) float mul[16 * kSrPitch];
  __shared__ int midx[kSrThreads];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sfi = blockIdx.x;
  const int s = sfi / F, f = sfi - s * F;
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  double* rowd = reinterpret_cast<double*>(rows + (size_t)sfi * kSrRowBytes);
  int32_t* rowi = reinterpret_cast<int32_t*>(rowd + kSrSums);

  Head::template stage<kSrThreads>(head_params, hlds, tid);
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
  if (P < 2) {                                             // uniform over the workgroup: not scored
    if (tid < kSrSums) rowd[tid] = 0.0;
    else if (tid < kSrSums + 4) rowi[tid - kSrSums] = 0;
    return;
  }
  Head head;
  head.bind(hlds);

  const int NI = K + 1;                                    // items: the draws, then the targets
  const int NP = K * NI / 2;                               // item pairs j < l
  const int NF = 25 * NI;                                  // s [24] and q per item
  const int m = tid & (TM - 1), kk = tid / TM;             // the lane's member slot and item of a round
  const int DR = kSrThreads / TM;
  const size_t sf = (size_t)sfi;
  const size_t tf = shared_targets ? (size_t)s : sf;
  // the lane's pairs: p = l (l - 1) / 2 + j, as offsets of the items' slots of member 0
  int pj[kSrAPT], pl[kSrAPT];
  double acc[kSrAPT];
#pragma unroll
  for (int i = 0; i < kSrAPT; ++i) {
    const int p = tid + i * kSrThreads;
    int l = (int)((1.f + sqrtf(1.f + 8.f * (float)p)) * 0.5f);
    if (l * (l - 1) / 2 > p) --l;
    if ((l + 1) * l / 2 <= p) ++l;
    pj[i] = (p - l * (l - 1) / 2) * kSrPitch;
    pl[i] = l * kSrPitch;
    acc[i] = 0.0;
  }
  // the lane's sums: idx = 25 item + c, c < 24: s[c], c = 24: q
  int fo[kSrAFT];
  double fa[kSrAFT];
#pragma unroll
  for (int i = 0; i < kSrAFT; ++i) {
    const int idx = tid + i * kSrThreads;
    const int it = idx / 25;
    fo[i] = it * kSrPitch + (idx - it * 25);               // item's slot of member 0, + c
    fa[i] = 0.0;
  }
  const int mstride = NI * kSrPitch;                       // floats from a member's slots to the next's

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
      if (kk == 0) sr_store(mul + m * kSrPitch, mu);
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
        sr_store(xy + (m * NI + k) * kSrPitch, c);
      }
    }
    __syncthreads();
    // ---- the pairs: members ascending, coordinates ascending ----
#pragma unroll
    for (int i = 0; i < kSrAPT; ++i) {
      if (tid + i * kSrThreads < NP) {
        double a = acc[i];
        const float* za = xy + pj[i];
        const float* zb = xy + pl[i];
#pragma nounroll
        for (int mm = 0; mm < tc; ++mm) a = sr_dist2(za + mm * mstride, zb + mm * mstride, a);
        acc[i] = a;
      }
    }
    // ---- the sums of the residuals ----
#pragma unroll
    for (int i = 0; i < kSrAFT; ++i) {
      const int idx = tid + i * kSrThreads;
      if (idx < NF) {
        double a = fa[i];
        const int c = idx % 25;
        if (c < kL2) {
          const float* z = xy + fo[i];
#pragma nounroll
          for (int mm = 0; mm < tc; ++mm) a = a + ((double)z[mm * mstride] - (double)mul[mm * kSrPitch + c]);
        } else {
          const float* z = xy + (fo[i] - kL2);
#pragma nounroll
          for (int mm = 0; mm < tc; ++mm) a = sr_dist2(z + mm * mstride, mul + mm * kSrPitch, a);
        }
        fa[i] = a;
      }
    }
    __syncthreads();                                       // xy and mul are written again by the next tile
  }

  // ---- the end: the accumulators over xy ----
  double* dD = reinterpret_cast<double*>(xy);              // [NP] D2, then D
  double* dF = dD + NP;                                    // [25 NI] s and q
  double* dT = dF + NF;                                    // [4][NI] t, loc, spr, u
#pragma unroll
  for (int i = 0; i < kSrAPT; ++i)
    if (tid + i * kSrThreads < NP) dD[tid + i * kSrThreads] = sqrt(acc[i]);
#pragma unroll
  for (int i = 0; i < kSrAFT; ++i)
    if (tid + i * kSrThreads < NF) dF[tid + i * kSrThreads] = fa[i];
  __syncthreads();
  if (tid < NI) {
    const int j = tid;
    double t = 0.0, u = 0.0;
    for (int l = 0; l < j; ++l) {
      const double v = dD[j * (j - 1) / 2 + l];
      t = t + v;
      u = u + v;                                           // u_j: the items before j
    }
    for (int l = j + 1; l < NI; ++l) t = t + dD[l * (l - 1) / 2 + j];
    double ss = 0.0;
    for (int c = 0; c < kL2; ++c) {
      const double v = dF[j * 25 + c];
      ss = __builtin_fma(v, v, ss);
    }
    const double loc = ss / (double)P;
    dT[j] = t;
    dT[NI + j] = loc;
    dT[2 * NI + j] = dF[j * 25 + kL2] - loc;
    dT[3 * NI + j] = u;
  }
  __syncthreads();
  if (tid < 3) {                                           // the ranks: strict comparisons
    const double* g = dT + tid * NI;
    const double y = g[K];
    int r = 0;
    for (int k = 0; k < K; ++k) r += g[k] < y ? 1 : 0;
    rowi[1 + tid] = r;
  } else if (tid == 3) {
    rowi[0] = P;
    rowd[0] = dT[K] / (double)K;                           // m
  } else if (tid == 4) {
    double u = 0.0;
    for (int l = 1; l < K; ++l) u = u + dT[3 * NI + l];
    rowd[1] = 2.0 * u / ((double)K * (double)(K - 1));     // p
  } else if (tid < 7) {                                    // loc (5), spr (6): the draws' mean, the targets'
    const double* g = dT + (tid - 4) * NI;
    double a = 0.0;
    for (int k = 0; k < K; ++k) a = a + g[k];
    rowd[2 + 2 * (tid - 5)] = a / (double)K;
    rowd[3 + 2 * (tid - 5)] = g[K];
  }
}

// Column j of a scene's rows, the frames in frame order: j < 6 the doubles, then
// the four totals, then the 3 B bins.
__global__ void __launch_bounds__(256) scene_rows_kernel(
    const unsigned char* __restrict__ rows, int S, int F, int K, int B, int32_t* __restrict__ per_frame_i,
    double* __restrict__ per_frame_d, double* __restrict__ sums, int32_t* __restrict__ hist,
    long long* __restrict__ tot) {
#pragma clang fp contract(off)
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per = kSrSums + G2K_SCENE_RANKS_TOT + 3 * B;
  if (id >= (int64_t)S * per) return;
  const int64_t s = id / per;
  const int j = (int)(id - s * per);
  const unsigned char* r0 = rows + (size_t)s * F * kSrRowBytes;
  if (j < kSrSums) {
    double all = 0.0;
    for (int f = 0; f < F; ++f) {
      const double v = reinterpret_cast<const double*>(r0 + (size_t)f * kSrRowBytes)[j];
      if (per_frame_d) per_frame_d[((size_t)s * F + f) * kSrSums + j] = v;
      all = all + v;
    }
    sums[s * kSrSums + j] = all;
  } else if (j < kSrSums + G2K_SCENE_RANKS_TOT) {
    const int col = j - kSrSums;
    long long all = 0;
    for (int f = 0; f < F; ++f) {
      const int v = reinterpret_cast<const int32_t*>(r0 + (size_t)f * kSrRowBytes + kSrSums * 8)[col];
      if (per_frame_i) per_frame_i[((size_t)s * F + f) * G2K_SCENE_RANKS_TOT + col] = v;
      all += col == 0 ? (v > 0 ? 1 : 0) : v;
    }
    tot[s * G2K_SCENE_RANKS_TOT + col] = all;
  } else {
    const int g = (j - kSrSums - G2K_SCENE_RANKS_TOT) / B, b = (j - kSrSums - G2K_SCENE_RANKS_TOT) - g * B;
    const int binw = (K + 1) / B;                          // ranks per bin
    int v = 0;
    for (int f = 0; f < F; ++f) {
      const int32_t* ri = reinterpret_cast<const int32_t*>(r0 + (size_t)f * kSrRowBytes + kSrSums * 8);
      v += (ri[0] > 0 && ri[1 + g] / binw == b) ? 1 : 0;
    }
    hist[(s * 3 + g) * B + b] = v;
  }
}

template <class Head>
int scene_ranks_launch(const g2k_dims* d, const float* pred, const float* targets,
                       const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                       const float* head_params, uint64_t seed, int K, int B, int32_t* per_frame_i,
                       double* per_frame_d, double* sums, int32_t* hist, int64_t* tot,
                       unsigned char* rows, hipStream_t st) {
  const SceneGeom g = scene_geom(*d, K);
  const int64_t units = (int64_t)d->S * d->F;
  if (units > 0x7fffffff)
    return set_err(G2K_EINVAL, "%sscene_ranks: %lld workgroups", Head::kPrefix, (long long)units);
  if (units > 0) {
    const int shared = (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0;
    hipLaunchKernelGGL((scene_ranks_kernel<Head>), dim3((unsigned)units), dim3(kSrThreads), 0, st, pred,
                       targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, K, g.TM,
                       (uint32_t)seed, (uint32_t)(seed >> 32), shared, rows);
    const int rc = check_launch("scene_ranks_kernel");
    if (rc) return rc;
  }
  const int64_t ids = (int64_t)d->S * (kSrSums + G2K_SCENE_RANKS_TOT + 3 * B);
  hipLaunchKernelGGL(scene_rows_kernel, dim3((unsigned)((ids + 255) / 256)), dim3(256), 0, st, rows,
                     d->S, d->F, K, B, per_frame_i, per_frame_d, sums, hist,
                     reinterpret_cast<long long*>(tot));
  return check_launch("scene_rows_kernel");
}

inline bool scene_k_ok(int32_t K) { return K >= G2K_SCENE_RANKS_KMIN && K <= G2K_SCENE_RANKS_KMAX; }
inline bool scene_bins_ok(int32_t B) { return B >= 1 && B <= G2K_SCENE_RANKS_BMAX; }

int check_scene_k(int32_t K) {
  if (!scene_k_ok(K))
    return set_err(G2K_EINVAL, "K=%d (%d..%d)", K, G2K_SCENE_RANKS_KMIN, G2K_SCENE_RANKS_KMAX);
  return G2K_OK;
}

// one row of 64 bytes per scene-frame
int64_t scene_ws_bytes(const g2k_dims* d) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * kSrRowBytes;
}

int check_align(const void* p, int align, const char* what) {
  if (((uintptr_t)p) & (uintptr_t)(align - 1))
    return set_err(G2K_EINVAL, "%s must be %d-byte aligned", what, align);
  return G2K_OK;
}

// the argument checks, before any HIP call; G2K_OK with S > 0: launch
int scene_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                   const void* n_active, const void* head, int32_t K, int32_t B,
                   const void* per_frame_i, const void* per_frame_d, const void* sums, const void* hist,
                   const void* tot, const void* workspace, int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "%s: flags %d (0 or G2K_STEP_TARGETS_SHARED)", name, d->flags);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_scene_k(K)) return rc;
  if (!scene_bins_ok(B) || (K + 1) % B)
    return set_err(G2K_EINVAL, "B=%d (1..%d, a divisor of K + 1 = %d)", B, G2K_SCENE_RANKS_BMAX, K + 1);
  if (const int rc = check_required({pred, targets, n_active, head, sums, hist, tot})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_align(per_frame_i, 4, "per_frame_i")) return rc;
  if (const int rc = check_align(per_frame_d, 8, "per_frame_d")) return rc;
  if (const int rc = check_align(sums, 8, "sums")) return rc;
  if (const int rc = check_align(hist, 4, "hist")) return rc;
  if (const int rc = check_align(tot, 8, "tot")) return rc;
  return check_workspace(d, workspace, workspace_bytes, scene_ws_bytes(d), 8);   // rows of doubles
}

template <class Head>
int scene_ranks(const char* name, const g2k_dims* d, const float* pred, const float* targets,
                const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                const float* head, uint64_t seed, int32_t K, int32_t B, int32_t* per_frame_i,
                double* per_frame_d, double* sums, int32_t* hist, int64_t* tot, void* workspace,
                int64_t workspace_bytes, void* stream) {
  const int rc = scene_validate(name, d, pred, targets, n_active, head, K, B, per_frame_i, per_frame_d,
                                sums, hist, tot, workspace, workspace_bytes);
  if (rc || d->S == 0) return rc;
  return scene_ranks_launch<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K, B,
                                  per_frame_i, per_frame_d, sums, hist, tot,
                                  static_cast<unsigned char*>(workspace), (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

// the heads share the geometry, so the workspace too
int64_t g2k_scene_ranks_workspace_bytes(const g2k_dims* d, int32_t K, int32_t B) {
  if (!d || !pair_sizes_ok(d) || !scene_k_ok(K) || !scene_bins_ok(B)) return -1;
  return scene_ws_bytes(d);
}

// the launch geometry (scene_geom: host arithmetic, no HIP call), as the
// launcher works it out
int g2k_scene_ranks_geometry(const g2k_dims* d, int32_t K, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_scene_k(K)) return rc;
  if (!out) return set_err(G2K_EINVAL, "out is NULL");
  const SceneGeom g = scene_geom(*d, K);
  out[G2K_SCENE_RANKS_GEOM_TM] = g.TM;
  out[G2K_SCENE_RANKS_GEOM_DR] = g.DR;
  out[G2K_SCENE_RANKS_GEOM_TILES] = g.tiles;
  out[G2K_SCENE_RANKS_GEOM_W] = 1;
  out[G2K_SCENE_RANKS_GEOM_PAIRS] = g.pairs;
  out[G2K_SCENE_RANKS_GEOM_APT] = g.apt;
  out[G2K_SCENE_RANKS_GEOM_AFT] = g.aft;
  out[G2K_SCENE_RANKS_GEOM_LDS_BYTES] = kSrLdsBytes;
  return G2K_OK;
}

int g2k_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* head, uint64_t seed, int32_t K, int32_t B, int32_t* per_frame_i,
                        double* per_frame_d, double* sums, int32_t* hist, int64_t* tot, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  return scene_ranks<PerStepHead>("scene_ranks", d, pred, targets, n_active, n_frames, ped_mask, head,
                                  seed, K, B, per_frame_i, per_frame_d, sums, hist, tot, workspace,
                                  workspace_bytes, stream);
}

int g2k_fullcov_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                                const int32_t* n_active, const int32_t* n_frames,
                                const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                                int32_t B, int32_t* per_frame_i, double* per_frame_d, double* sums,
                                int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  return scene_ranks<FullCovHead>("fullcov_scene_ranks", d, pred, targets, n_active, n_frames, ped_mask,
                                  chol, seed, K, B, per_frame_i, per_frame_d, sums, hist, tot, workspace,
                                  workspace_bytes, stream);
}

int g2k_mix_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                            const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                            const float* mix, uint64_t seed, int32_t K, int32_t B, int32_t* per_frame_i,
                            double* per_frame_d, double* sums, int32_t* hist, int64_t* tot,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  return scene_ranks<MixHead>("mix_scene_ranks", d, pred, targets, n_active, n_frames, ped_mask, mix,
                              seed, K, B, per_frame_i, per_frame_d, sums, hist, tot, workspace,
                              workspace_bytes, stream);
}

int g2k_coupled_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                                const int32_t* n_active, const int32_t* n_frames,
                                const uint8_t* ped_mask, const float* cpl, uint64_t seed, int32_t K,
                                int32_t B, int32_t* per_frame_i, double* per_frame_d, double* sums,
                                int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  return scene_ranks<CoupledHead>("coupled_scene_ranks", d, pred, targets, n_active, n_frames, ped_mask,
                                  cpl, seed, K, B, per_frame_i, per_frame_d, sums, hist, tot, workspace,
                                  workspace_bytes, stream);
}

}  // extern "C"
