// g2k_couples.hip — fused couple-distance scores of a probabilistic head's
// JOINT samples: per couple of a scene-frame's members the closest approach and
// the final separation under the K joint draws, the target's PIT rank among
// them and the two terms of the fair CRPS.  ONE kernel template,
// couple_scores_kernel<Head, TR>, over the heads of g2k_head_draw.h
// (g2k_couple_scores_f32, g2k_fullcov_couple_scores_f32,
// g2k_mix_couple_scores_f32; g2k_coupled_couple_scores_f32 of
// include/g2k_coupled.h) and the two tile heights.  The C entry points are
// at the end of this file, declared in include/g2k_couples.h (added after ABI
// 11: bound by symbol), which states the definition.  The build's: the
// reference has no probabilistic head, so PARITY UNPINNED; pinned against
// tests/couples_ref.py.
//
// The features are single fp32 operations in a stated order (cp_q below, under
// "fp contract(off)"), so a rank, a comparison of two fp32 values, is an
// integer that the float32 restatement reproduces exactly.
//
// Geometry.  The members of a scene-frame are compacted as in joint_kernel
// (g2k_joint.hip).  A PASS is one TILE of TR row members x 16 column members,
// CP = 16 TR couples (those with a < b); only tiles that hold a couple exist,
// and they are dealt round-robin to the scene-frame's W workgroups (W from the
// shapes alone: enough workgroups to fill the device, at most 8, at most the
// tiles of P = Nmax).  A tile's K + 2 ITEMS are the K joint draws, then the
// targets and the mean prediction; a ROUND makes 8 of them: lane (member m =
// tid % 32, item tid / 32) draws its member once into LDS, xy[8][32][24] — no
// draw reaches global memory and each serves up to 16 couples — then the CP x 8
// (couple, item) cells are dealt to the 256 lanes, which park {qmin, qfin} in
// vals[item][couple] (8 B per cell: K + 2 <= 24 items of 256 couples, or <= 66
// of 128; that is what sets TR).  After the last round thread c owns couple c:
// the ranks against the target's squared values, the roots in place, m and d in
// k order, then the spread term over k < l from its own column of vals (lanes
// of a wave read consecutive cells: no bank conflict).  Sums stay in registers
// over the passes; at the end lanes by butterfly, waves in order.
//   Every workgroup leaves one row [12 + 2 B] in the caller's workspace (8 float
// sums, scored, sum r_min, sum r_fin, P, the two histograms);
// couple_rows_kernel adds a scene-frame's W rows in workgroup order and the
// scene's frames in frame order.  No float atomics, no waits between
// workgroups.
#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_coupled.h"
#include "g2k_couples.h"
#include "g2k_head_draw.h"
#include "g2k_mix.h"

namespace g2k {
namespace {

constexpr int kCpThreads = 256;
constexpr int kCpTC = 16;                     // column members of a tile
constexpr int kCpDR = 8;                      // items of a round
constexpr int kCpSlots = 32;                  // member slots of an item in xy (TR + TC <= 32)
constexpr int kCpKTall = 22;                  // K <= 22: TR = 16; above: TR = 8
constexpr int kCpMaxW = 8;                    // workgroups per scene-frame at most
constexpr int kCpFill = 2048;                 // workgroups that fill 256 CUs four deep (LDS: two are resident)
constexpr int kCpRowHead = 12;                // words of a row before the histograms
constexpr int kCpSums = G2K_COUPLES_SUMS;

constexpr int cp_items(int TR) { return (TR == 16 ? kCpKTall : G2K_COUPLES_KMAX) + 2; }
constexpr int cp_lds_bytes(int TR) {
  return kCpDR * kCpSlots * kL2 * 4 + cp_items(TR) * TR * kCpTC * 8 + 2 * kCpThreads * 4 + 4 * 4 +
         2 * G2K_COUPLES_BMAX * 4 + 4 * kCpSums * 4 + 4 * 4 * 4;
}

// tile (rb, cb) holds a couple a < b < P: a in the row block, b in the column block
__host__ __device__ inline bool cp_tile_live(int rb, int cb, int TR, int P) {
  const int b0 = cb * kCpTC > rb * TR + 1 ? cb * kCpTC : rb * TR + 1;
  const int b1 = (cb + 1) * kCpTC < P ? (cb + 1) * kCpTC : P;
  return b0 < b1;
}

struct CoupleGeom { int TR, CP, tiles, W, passes; };

inline int cp_tiles(int P, int TR) {
  int n = 0;
  for (int rb = 0; rb * TR < P; ++rb)
    for (int cb = (rb * TR + 1) / kCpTC; cb * kCpTC < P; ++cb) n += cp_tile_live(rb, cb, TR, P) ? 1 : 0;
  return n;
}

inline CoupleGeom couple_geom(const g2k_dims& d, int K) {
  CoupleGeom g;
  g.TR = K <= kCpKTall ? 16 : 8;
  g.CP = g.TR * kCpTC;
  g.tiles = cp_tiles(d.Nmax, g.TR);
  const int64_t sf = (int64_t)d.S * d.F;
  int64_t w = sf > 0 ? (kCpFill + sf - 1) / sf : 1;
  if (w > kCpMaxW) w = kCpMaxW;
  if (w > g.tiles) w = g.tiles;
  if (w < 1) w = 1;
  g.W = (int)w;
  g.passes = (g.tiles + g.W - 1) / g.W;
  return g;
}

// one step's squared distance: two differences, two products, one add
__device__ __forceinline__ float cp_q(float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
  const float dx = ax - bx;
  const float dy = ay - by;
  const float xx = dx * dx;
  const float yy = dy * dy;
  return xx + yy;
}

// a slot of xy (time-major, 6 ds_read_b128) against another: {qmin, qfin}
__device__ __forceinline__ float2 cp_features(const float* sa, const float* sb) {
  const float4* pa = reinterpret_cast<const float4*>(sa);
  const float4* pb = reinterpret_cast<const float4*>(sb);
  float qmin = __builtin_inff(), q = 0.f;
#pragma unroll
  for (int u = 0; u < kL2 / 4; ++u) {
    const float4 a = pa[u], b = pb[u];
    q = cp_q(a.x, a.y, b.x, b.y);
    qmin = fminf(qmin, q);
    q = cp_q(a.z, a.w, b.z, b.w);
    qmin = fminf(qmin, q);
  }
  return make_float2(qmin, q);
}

__device__ __forceinline__ void cp_store(float* slot, const float (&x)[kL2]) {
  float4* o = reinterpret_cast<float4*>(slot);
#pragma unroll
  for (int q = 0; q < kL2 / 4; ++q) o[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}

template <class Head, int TR>
__global__ void __launch_bounds__(kCpThreads) couple_scores_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int W, int K, int B, uint32_t seed_lo, uint32_t seed_hi, int shared_targets, float r2,
    int every, float invK, float invKK, int32_t* __restrict__ per_couple, int32_t* __restrict__ rows) {
  constexpr int CP = TR * kCpTC, TM = TR + kCpTC, NV = cp_items(TR);
  __shared__ typename Head::Lds hlds;
  __shared__ __attribute__((aligned(16))) float xy[kCpDR * kCpSlots * kL2];
  __shared__ float2 vals[NV * CP];
  __shared__ int midx[kCpThreads];
  __shared__ int ismem[kCpThreads];
  __shared__ int wcnt[4];
  __shared__ int lh[2 * G2K_COUPLES_BMAX];
  __shared__ float partf[4][kCpSums];
  __shared__ int parti[4][4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sfi = blockIdx.x / W, wg = blockIdx.x - sfi * W;
  const int s = sfi / F, f = sfi - s * F;
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  const int RW = kCpRowHead + 2 * B;
  int32_t* row = rows + (size_t)blockIdx.x * RW;

  Head::template stage<kCpThreads>(head_params, hlds, tid);
  if (tid < 2 * B) lh[tid] = 0;
  // compact the members: member i = column midx[i]
  bool mem = f < nf && tid < nact;
  if (mem && ped_mask) mem = ped_mask[(size_t)s * Nmax + tid] != 0;
  ismem[tid] = mem ? 1 : 0;
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
  // every element that is no member couple: zero (the member couples are
  // written by the workgroup that takes their tile)
  int32_t* pc = per_couple ? per_couple + (size_t)sfi * Nmax * Nmax : nullptr;
  if (pc) {
    for (int idx = wg * kCpThreads + tid; idx < Nmax * Nmax; idx += W * kCpThreads) {
      const int i = idx / Nmax, j = idx - i * Nmax;
      if (!(i < j && ismem[i] && ismem[j])) pc[idx] = 0;
    }
  }
  __syncthreads();
  if (P < 2) {                                             // uniform over the workgroup
    if (tid < RW) row[tid] = tid == kCpRowHead - 1 ? P : 0;
    return;
  }
  Head head;
  head.bind(hlds);

  const int m = tid & (kCpSlots - 1), kk = tid >> 5;       // the lane's member slot and item of a round
  const int NI = K + 2;                                    // items: the draws, the targets, the mean
  const int binw = (K + 1) / B;                            // ranks per bin
  const size_t sf = (size_t)sfi;
  const size_t tf = shared_targets ? (size_t)s : sf;
  float acc[kCpSums];
#pragma unroll
  for (int i = 0; i < kCpSums; ++i) acc[i] = 0.f;
  int nsc = 0, srmin = 0, srfin = 0;
  int tix = 0;
#pragma nounroll
  for (int rb = 0; rb * TR < P; ++rb) {
#pragma nounroll
    for (int cb = (rb * TR + 1) / kCpTC; cb * kCpTC < P; ++cb) {
      if (!cp_tile_live(rb, cb, TR, P)) continue;
      const bool mine = tix % W == wg;
      ++tix;
      if (!mine) continue;                                 // uniform
      // ---- the tile's members: rows first, then columns ----
      const int mi = m < TR ? rb * TR + m : cb * kCpTC + (m - TR);
      const bool mon = m < TM && mi < P;
      const int n = mon ? midx[mi] : 0;
      const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;    // element of step 0
      float mu[kL2];
      if (mon) {
        const size_t pb = sf * kL2 * Nmax + n;             // load_mu_tg's means
#pragma unroll
        for (int t = 0; t < kL; ++t) {
          mu[2 * t] = pred[pb + (size_t)t * Nmax];
          mu[2 * t + 1] = pred[pb + (size_t)(kL + t) * Nmax];
        }
      } else {
#pragma unroll
        for (int r = 0; r < kL2; ++r) mu[r] = 0.f;
      }
#pragma nounroll
      for (int r0 = 0; r0 < NI; r0 += kCpDR) {
        // ---- draw: item r0 + kk of member slot m ----
        const int k = r0 + kk;
        if (mon && k < NI) {
          float c[kL2];
          if (k < K) {
            const uint32_t lo = seed_lo + (uint32_t)k;     // (seed + k) mod 2^64
            const uint32_t hi = seed_hi + (lo < seed_lo ? 1u : 0u);
            head.draw(lo, hi, e0, n, Nmax, mu, [&](int t, float x, float y) {
              c[2 * t] = x; c[2 * t + 1] = y;
            });
          } else if (k == K) {
            const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf * Nmax + n) * kL;
#pragma unroll
            for (int t = 0; t < kL; ++t) {
              const float2 v = t2[t];
              c[2 * t] = v.x; c[2 * t + 1] = v.y;
            }
          } else {
#pragma unroll
            for (int r = 0; r < kL2; ++r) c[r] = mu[r];
          }
          cp_store(xy + (kk * kCpSlots + m) * kL2, c);
        }
        __syncthreads();
        // ---- cells: (couple, item) dealt to the lanes ----
#pragma unroll 2
        for (int idx = tid; idx < CP * kCpDR; idx += kCpThreads) {
          const int c = idx & (CP - 1), kq = idx / CP;
          const int k2 = r0 + kq;
          const int ar = c >> 4, bc = c & (kCpTC - 1);
          const int a = rb * TR + ar, b = cb * kCpTC + bc;
          if (k2 < NI && a < b && b < P)
            vals[k2 * CP + c] = cp_features(xy + (kq * kCpSlots + ar) * kL2,
                                            xy + (kq * kCpSlots + TR + bc) * kL2);
        }
        __syncthreads();
      }
      // ---- the couple: thread c owns column c of vals ----
      if (tid < CP) {
        const int c = tid;
        const int ar = c >> 4, bc = c & (kCpTC - 1);
        const int a = rb * TR + ar, b = cb * kCpTC + bc;
        if (a < b && b < P) {
          const float2 qY = vals[K * CP + c];
          const float qM = vals[(K + 1) * CP + c].x;
          int code = 0;
          if (every || qM < r2) {
            const float yl = sqrtf(qY.x), yf = sqrtf(qY.y);
            int rl = 0, rf = 0;
            float ml = 0.f, mf = 0.f, dl = 0.f, df = 0.f;
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
              const float2 q = vals[k * CP + c];
              rl += q.x < qY.x ? 1 : 0;
              rf += q.y < qY.y ? 1 : 0;
              const float sl = sqrtf(q.x), sn = sqrtf(q.y);
              vals[k * CP + c] = make_float2(sl, sn);     // the roots in place: this thread's own cells
              ml += fabsf(sl - yl); mf += fabsf(sn - yf);
              dl += sl; df += sn;
            }
            float pl = 0.f, pf = 0.f;
#pragma nounroll
            for (int k = 0; k + 1 < K; ++k) {
              const float2 sk = vals[k * CP + c];
#pragma unroll 8
              for (int l = k + 1; l < K; ++l) {
                const float2 v = vals[l * CP + c];
                pl += fabsf(sk.x - v.x);
                pf += fabsf(sk.y - v.y);
              }
            }
            acc[0] += ml * invK; acc[1] += mf * invK;
            acc[2] += pl * invKK; acc[3] += pf * invKK;
            acc[4] += dl * invK; acc[5] += df * invK;
            acc[6] += yl; acc[7] += yf;
            ++nsc; srmin += rl; srfin += rf;
            atomicAdd(&lh[rl / binw], 1);                  // integers: the order cannot show
            atomicAdd(&lh[B + rf / binw], 1);
            code = 1 + rl + 256 * rf;
          }
          if (pc) pc[(size_t)midx[a] * Nmax + midx[b]] = code;
        }
      }
      // vals and xy are next written after the following tile's first barrier,
      // which every thread reaches after its couple
    }
  }
  // the workgroup's row: lanes by butterfly, waves in order
#pragma unroll
  for (int i = 0; i < kCpSums; ++i) {
    const float v = wave_sum(acc[i]);
    if (lane == 0) partf[wv][i] = v;
  }
  {
    const int a = wave_sum_i(nsc), b = wave_sum_i(srmin), c = wave_sum_i(srfin);
    if (lane == 0) { parti[wv][0] = a; parti[wv][1] = b; parti[wv][2] = c; }
  }
  __syncthreads();
  if (tid < kCpSums)
    row[tid] = (int32_t)__float_as_uint(((partf[0][tid] + partf[1][tid]) + partf[2][tid]) + partf[3][tid]);
  else if (tid < kCpSums + 3)
    row[tid] = parti[0][tid - kCpSums] + parti[1][tid - kCpSums] + parti[2][tid - kCpSums] +
               parti[3][tid - kCpSums];
  else if (tid == kCpRowHead - 1)
    row[tid] = P;
  if (tid < 2 * B) row[kCpRowHead + tid] = lh[tid];
}

// Column j of a scene's rows: a scene-frame's W rows in workgroup order, the
// frames in frame order.
__global__ void __launch_bounds__(256) couple_rows_kernel(
    const int32_t* __restrict__ rows, int S, int F, int W, int B, float* __restrict__ per_frame_f,
    int32_t* __restrict__ per_frame_i, float* __restrict__ sums, int32_t* __restrict__ hist,
    long long* __restrict__ tot) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per = kCpRowHead + 2 * B;
  if (id >= (int64_t)S * per) return;
  const int64_t s = id / per;
  const int j = (int)(id - s * per);
  const int32_t* r0 = rows + (size_t)s * F * W * per + j;
  if (j < kCpSums) {
    float all = 0.f;
    for (int f = 0; f < F; ++f) {
      float v = 0.f;
      for (int w = 0; w < W; ++w) v += __uint_as_float((uint32_t)r0[((size_t)f * W + w) * per]);
      if (per_frame_f) per_frame_f[((size_t)s * F + f) * kCpSums + j] = v;
      all += v;
    }
    sums[s * kCpSums + j] = all;
  } else if (j < kCpRowHead) {
    const int col = j - kCpSums;                           // 3: P of the first row -> PP
    long long all = 0;
    for (int f = 0; f < F; ++f) {
      int v = 0;
      if (col < 3) {
        for (int w = 0; w < W; ++w) v += r0[((size_t)f * W + w) * per];
      } else {
        const int P = r0[(size_t)f * W * per];
        v = P * (P - 1) / 2;
      }
      if (per_frame_i) per_frame_i[((size_t)s * F + f) * G2K_COUPLES_TOT + col] = v;
      all += v;
    }
    tot[s * G2K_COUPLES_TOT + col] = all;
  } else {
    int v = 0;
    for (int f = 0; f < F; ++f)
      for (int w = 0; w < W; ++w) v += r0[((size_t)f * W + w) * per];
    hist[s * 2 * B + (j - kCpRowHead)] = v;
  }
}

template <class Head, int TR>
void couple_scores_start(int64_t units, hipStream_t st, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                         const float* head_params, const g2k_dims* d, int W, int K, int B, uint64_t seed,
                         float r2, int every, int32_t* per_couple, int32_t* rows) {
  const int shared = (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0;
  const float invK = (float)(1.0 / (double)K);
  const float invKK = (float)(2.0 / ((double)K * (double)(K - 1)));
  hipLaunchKernelGGL((couple_scores_kernel<Head, TR>), dim3((unsigned)units), dim3(kCpThreads), 0, st,
                     pred, targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, W, K, B,
                     (uint32_t)seed, (uint32_t)(seed >> 32), shared, r2, every, invK, invKK, per_couple,
                     rows);
}

template <class Head>
int couple_scores_launch(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                         const float* head_params, uint64_t seed, int K, int B, float reach,
                         int32_t* per_couple, float* per_frame_f, int32_t* per_frame_i, float* sums,
                         int32_t* hist, int64_t* tot, int32_t* rows, hipStream_t st) {
  const CoupleGeom g = couple_geom(*d, K);
  const int64_t units = (int64_t)d->S * d->F * g.W;
  if (units > 0x7fffffff)
    return set_err(G2K_EINVAL, "%scouple_scores: %lld workgroups", Head::kPrefix, (long long)units);
  const float r2 = reach * reach;
  const int every = reach > 3.402823466e38f ? 1 : 0;
  if (units > 0) {
    if (g.TR == 16)
      couple_scores_start<Head, 16>(units, st, pred, targets, n_active, n_frames, ped_mask, head_params,
                                    d, g.W, K, B, seed, r2, every, per_couple, rows);
    else
      couple_scores_start<Head, 8>(units, st, pred, targets, n_active, n_frames, ped_mask, head_params,
                                   d, g.W, K, B, seed, r2, every, per_couple, rows);
    const int rc = check_launch("couple_scores_kernel");
    if (rc) return rc;
  }
  const int64_t ids = (int64_t)d->S * (kCpRowHead + 2 * B);
  hipLaunchKernelGGL(couple_rows_kernel, dim3((unsigned)((ids + 255) / 256)), dim3(256), 0, st, rows,
                     d->S, d->F, g.W, B, per_frame_f, per_frame_i, sums, hist,
                     reinterpret_cast<long long*>(tot));
  return check_launch("couple_rows_kernel");
}

inline bool couples_k_ok(int32_t K) { return K >= G2K_COUPLES_KMIN && K <= G2K_COUPLES_KMAX; }
inline bool couples_bins_ok(int32_t B) { return B >= 1 && B <= G2K_COUPLES_BMAX; }

int check_couples_k(int32_t K) {
  if (!couples_k_ok(K))
    return set_err(G2K_EINVAL, "K=%d (%d..%d)", K, G2K_COUPLES_KMIN, G2K_COUPLES_KMAX);
  return G2K_OK;
}

// one row [12 + 2 B] of int32 per workgroup
int64_t couples_ws_bytes(const g2k_dims* d, int32_t K, int32_t B) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * couple_geom(*d, K).W * (kCpRowHead + 2 * B) * 4;
}

int check_align4(const void* p, const char* what) {
  if (((uintptr_t)p) & 3) return set_err(G2K_EINVAL, "%s must be 4-byte aligned", what);
  return G2K_OK;
}

// the argument checks, before any HIP call; G2K_OK with S > 0: launch
int couples_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                     const void* n_active, const void* head, int32_t K, int32_t B, float reach,
                     const void* per_couple, const void* per_frame_f, const void* per_frame_i,
                     const void* sums, const void* hist, const void* tot, const void* workspace,
                     int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "%s: flags %d (0 or G2K_STEP_TARGETS_SHARED)", name, d->flags);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_couples_k(K)) return rc;
  if (!couples_bins_ok(B) || (K + 1) % B)
    return set_err(G2K_EINVAL, "B=%d (1..%d, a divisor of K + 1 = %d)", B, G2K_COUPLES_BMAX, K + 1);
  if (!(reach > 0.f)) return set_err(G2K_EINVAL, "reach=%g (> 0, or +inf: every couple)", (double)reach);
  if (const int rc = check_required({pred, targets, n_active, head, sums, hist, tot})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (const int rc = check_align4(per_couple, "per_couple")) return rc;
  if (const int rc = check_align4(per_frame_f, "per_frame_f")) return rc;
  if (const int rc = check_align4(per_frame_i, "per_frame_i")) return rc;
  if (const int rc = check_align4(sums, "sums")) return rc;
  if (const int rc = check_align4(hist, "hist")) return rc;
  if (((uintptr_t)tot) & 7) return set_err(G2K_EINVAL, "tot must be 8-byte aligned");
  return check_workspace(d, workspace, workspace_bytes, couples_ws_bytes(d, K, B), 4);   // rows of int32
}

template <class Head>
int couple_scores(const char* name, const g2k_dims* d, const float* pred, const float* targets,
                  const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                  const float* head, uint64_t seed, int32_t K, int32_t B, float reach,
                  int32_t* per_couple, float* per_frame_f, int32_t* per_frame_i, float* sums,
                  int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = couples_validate(name, d, pred, targets, n_active, head, K, B, reach, per_couple,
                                  per_frame_f, per_frame_i, sums, hist, tot, workspace, workspace_bytes);
  if (rc || d->S == 0) return rc;
  return couple_scores_launch<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K, B,
                                    reach, per_couple, per_frame_f, per_frame_i, sums, hist, tot,
                                    static_cast<int32_t*>(workspace), (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

// the heads share the geometry, so the workspace too
int64_t g2k_couple_scores_workspace_bytes(const g2k_dims* d, int32_t K, int32_t B) {
  if (!d || !pair_sizes_ok(d) || !couples_k_ok(K) || !couples_bins_ok(B)) return -1;
  return couples_ws_bytes(d, K, B);
}

// the launch geometry (couple_geom: host arithmetic, no HIP call), as the
// launcher works it out
int g2k_couple_scores_geometry(const g2k_dims* d, int32_t K, int32_t* out) {
  if (const int rc = check_dims(d)) return rc;
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_couples_k(K)) return rc;
  if (!out) return set_err(G2K_EINVAL, "out is NULL");
  const CoupleGeom g = couple_geom(*d, K);
  out[G2K_COUPLES_GEOM_TR] = g.TR;
  out[G2K_COUPLES_GEOM_TC] = kCpTC;
  out[G2K_COUPLES_GEOM_CP] = g.CP;
  out[G2K_COUPLES_GEOM_DR] = kCpDR;
  out[G2K_COUPLES_GEOM_TILES] = g.tiles;
  out[G2K_COUPLES_GEOM_W] = g.W;
  out[G2K_COUPLES_GEOM_PASSES] = g.passes;
  out[G2K_COUPLES_GEOM_LDS_BYTES] = cp_lds_bytes(g.TR);
  return G2K_OK;
}

int g2k_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                          const float* head, uint64_t seed, int32_t K, int32_t B, float reach,
                          int32_t* per_couple, float* per_frame_f, int32_t* per_frame_i, float* sums,
                          int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  return couple_scores<PerStepHead>("couple_scores", d, pred, targets, n_active, n_frames, ped_mask,
                                    head, seed, K, B, reach, per_couple, per_frame_f, per_frame_i, sums,
                                    hist, tot, workspace, workspace_bytes, stream);
}

int g2k_fullcov_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                                  const int32_t* n_active, const int32_t* n_frames,
                                  const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                                  int32_t B, float reach, int32_t* per_couple, float* per_frame_f,
                                  int32_t* per_frame_i, float* sums, int32_t* hist, int64_t* tot,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return couple_scores<FullCovHead>("fullcov_couple_scores", d, pred, targets, n_active, n_frames,
                                    ped_mask, chol, seed, K, B, reach, per_couple, per_frame_f,
                                    per_frame_i, sums, hist, tot, workspace, workspace_bytes, stream);
}

int g2k_mix_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                              const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                              const float* mix, uint64_t seed, int32_t K, int32_t B, float reach,
                              int32_t* per_couple, float* per_frame_f, int32_t* per_frame_i, float* sums,
                              int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  return couple_scores<MixHead>("mix_couple_scores", d, pred, targets, n_active, n_frames, ped_mask, mix,
                                seed, K, B, reach, per_couple, per_frame_f, per_frame_i, sums, hist, tot,
                                workspace, workspace_bytes, stream);
}

int g2k_coupled_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                                  const int32_t* n_active, const int32_t* n_frames,
                                  const uint8_t* ped_mask, const float* cpl, uint64_t seed, int32_t K,
                                  int32_t B, float reach, int32_t* per_couple, float* per_frame_f,
                                  int32_t* per_frame_i, float* sums, int32_t* hist, int64_t* tot,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return couple_scores<CoupledHead>("coupled_couple_scores", d, pred, targets, n_active, n_frames,
                                    ped_mask, cpl, seed, K, B, reach, per_couple, per_frame_f,
                                    per_frame_i, sums, hist, tot, workspace, workspace_bytes, stream);
}

}  // extern "C"
