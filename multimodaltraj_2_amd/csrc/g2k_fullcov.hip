// g2k_fullcov.hip — the full-covariance trajectory head: ONE Gaussian over a
// pair's whole 24-vector of residuals (the per-step head of g2k_nll.hip is its
// block-diagonal special case).  Its closed-form fit, joint NLL and
// calibration (g2k_fullcov_stats_f32) and its sampler (g2k_fullcov_sample_f32);
// the fused evaluations over its draws (g2k_fullcov_best_of_k_f32,
// g2k_fullcov_joint_eval_f32) are the shared kernels of g2k_bestk.hip and
// g2k_joint.hip with this head's policy (FullCovHead, g2k_head_draw.h).  The
// build's: the reference has no probabilistic head, so PARITY UNPINNED;
// tests/fullcov_ref.py restates the definition in float64 NumPy.
//
// Definition.  Pairs, pred, targets, n_active, n_frames, ped_mask as
// g2k_best_of_k_f32.  Coordinate i = 2 t + c (step t, c = 0 for x, 1 for y):
// time-major, so a lower-triangular factor is causal in time.
//   r[i] = targets[..][t][c] - pred[c 12 + t]                     (double)
//   chol [24][24] f32 row-major = L, the lower Cholesky factor of the residual
//     covariance; diagonal > 0 (the caller's contract); entries j > i are
//     never read
//   z[2t], z[2t+1] = the element's normals (gauss_normals, g2k_common.h) for
//     e = ((s F + f) 12 + t) Nmax + n and seed (seed + k) mod 2^64
//   draw: x[i] = mu[i] + sum_{j <= i} L[i][j] z[j], accumulated as acc = mu[i];
//     for j = 0..i: acc = fmaf(L[i][j], z[j], acc)  (fullcov_advance,
//     g2k_head_draw.h: one function for the sampler and the fused evaluations,
//     so they agree bit for bit); written in band layout, out[c 12 + t] =
//     x[2t + c]
//   NLL: z = L^-1 r (double), q_t = z[2t]^2 + z[2t+1]^2 (step t's innovation:
//     chi^2(2) under a calibrated head), q = sum_t q_t (chi^2(24)),
//     nll_t = log 2 pi + log L[2t][2t] + log L[2t+1][2t+1] + q_t / 2
//   fit: M = sum_pairs r r^T (uncentred), C = M / n, C_ii <- C_ii (1 + 1e-6) +
//     1e-12, fit = chol(C) in double, written as f32, zeros above the
//     diagonal; the identity when n = 0
//
// The draw.  Row i of the product takes column j's term in ascending j, so a
// sweep over the columns in order gives every row the defined order: after
// step t's two normals have been added into the rows >= 2t, x[2t] and x[2t+1]
// are final (a fused evaluation takes the step's error at once).  A lane holds
// 24 means and 24 running sums; the factor (300 wave-uniform floats) sits
// transposed in LDS (a column's entries contiguous: wide broadcast reads),
// read again for every draw — each step starts with a compiler barrier so that
// the reads are not hoisted out of the draw loop into 300 registers.  The step
// loop is unrolled, no per-thread array is indexed at run time: no scratch.
//
// Stats.  A slot is (s, f, n), n < Nmax; the S F Nmax slots are dealt in W
// contiguous ranges to W workgroups of 256 threads (fullcov_geom: at least
// 512 slots each, at most 256 workgroups).  A round is 256 slots, a thread
// per slot: the thread forms its pair's 24 residuals in double (non-pairs
// load nothing and stand as zeros), whitens them in registers with W = L^-1
// (formed once per workgroup in double from an LDS copy of L, a column per
// thread in registers; broadcast reads from LDS, no division in the loop), adds q_t to its 12 sums and takes part
// in the level counts (ballot + popcount, lane l keeps level l as in
// g2k_calib.hip).  The residuals are staged in LDS as 28 rows x 256 slots
// (24 coordinates, a row of ones for the pairs — so the Gram's row 24 is
// sum r and its corner the pair count — and three rows of zeros), and the Gram
// sum r r^T is taken by 252 threads: thread (g, b) owns the 4 x 4 block b of
// the lower triangle's 28 blocks over the slots g, g + 9, ...: 8 LDS reads per
// 16 double FMAs.  Plain double FMAs: the 16x16x4 f64 MFMA would want four
// pairs spread over a wave's lanes, a second staging layout, for arithmetic
// that is a fifth of the kernel's LDS time; not built.  Reduction: the nine
// slot subsets in order, the four waves' q sums (w0 + w1) + (w2 + w3), the
// counts likewise; W == 1 finishes in the same kernel, otherwise the rows
// [460 + 13 NL] (8-byte words) go to the workspace and g2k_fullcov_rows_kernel
// (one workgroup) adds them in row order and finishes: moments, stats, inside
// and the 24 x 24 Cholesky (one wave, serial over the columns, a row per lane
// in registers, a column's entries by lane shuffles).  No
// atomics: repeated calls are bit-identical, and the moments' bits do not
// depend on chol or the levels.
#include <float.h>

#include "g2k_common.h"
#include "g2k_head_draw.h"

namespace g2k {
namespace {

// ---------------------------------------------------------------------------
// the sampler
// ---------------------------------------------------------------------------
// fullcov_load_lt / fullcov_advance: g2k_head_draw.h (shared with the fused
// evaluations)

// one thread per (s, f, n): 24 coalesced loads along n, the 12 steps, 24 stores
__global__ void __launch_bounds__(256) g2k_fullcov_sample_kernel(
    const float* __restrict__ pred, const float* __restrict__ chol, int64_t slots, int Nmax,
    uint32_t seed_lo, uint32_t seed_hi, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float Lt[kL2 * kL2];
  fullcov_load_lt(chol, Lt, threadIdx.x, 256);
  __syncthreads();
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= slots) return;
  const int64_t sf = id / Nmax;
  const int n = (int)(id - sf * Nmax);
  const size_t pb = (size_t)sf * kL2 * Nmax + n;
  const int64_t e0 = sf * kL * Nmax + n;                   // element of step 0
  float a[kL2];
#pragma unroll
  for (int t = 0; t < kL; ++t) {
    a[2 * t] = pred[pb + (size_t)t * Nmax];
    a[2 * t + 1] = pred[pb + (size_t)(kL + t) * Nmax];
  }
  const uint32_t ehi0 = (uint32_t)(e0 >> 32);
  const uint32_t stream0 = gauss_stream(seed_lo, seed_hi, ehi0);
#pragma unroll
  for (int t = 0; t < kL; ++t) {
    const int64_t e = e0 + (int64_t)t * Nmax;
    const uint32_t ehi = (uint32_t)(e >> 32);
    uint32_t stream = stream0;
    if (ehi != ehi0) stream = gauss_stream(seed_lo, seed_hi, ehi);
    float z0, z1;
    gauss_normals(stream, (uint32_t)e, z0, z1);
    fullcov_advance(Lt, t, z0, z1, a);
    out[pb + (size_t)t * Nmax] = a[2 * t];
    out[pb + (size_t)(kL + t) * Nmax] = a[2 * t + 1];
  }
}

// ---------------------------------------------------------------------------
// stats and fit
// ---------------------------------------------------------------------------
constexpr int kFsThreads = 256;
constexpr int kFsDim = 28;                     // 24 coordinates, the ones row, 3 rows of zeros
constexpr int kFsBlocks = 28;                  // 4 x 4 blocks of the 7 x 7 lower triangle
constexpr int kFsSub = 9;                      // slot subsets: 9 * 28 = 252 threads
constexpr int kFsGram = kFsBlocks * 16;        // 448
constexpr int kFsPitch = kFsThreads + 1;       // odd: a round's rows start one 8-byte bank apart
constexpr int kFsVals = kFsGram + kL;          // 460: the Gram, then sum q_t
constexpr int kFsCnt = kL + 1;                 // 13 count rows: the steps, then the joint q
constexpr int kFsMaxLevels = 32;
constexpr int kFsRowMax = kFsVals + kFsCnt * kFsMaxLevels;   // 876
constexpr int kFsSlots = 512;                  // slots per workgroup, at least
constexpr int kFsMaxWgs = 256;
constexpr int kFsRowsThreads = 1024;
constexpr double kFsLog2Pi = 1.8378770664093454835606594728112;
// LDS of the stats kernel, in doubles: the staged round, then W (later the
// Cholesky's matrix); after the last round the staging area holds the
// reduction's parts
constexpr int kFsStage = kFsDim * kFsPitch;    // 7196
constexpr int kFsOffQ = kFsSub * kFsGram;      // 4032: the waves' q sums [4][12]
constexpr int kFsOffCnt = kFsOffQ + 4 * kL;    // 4080: the waves' counts [4][13][32]
constexpr int kFsOffFin = kFsOffCnt + 4 * kFsCnt * kFsMaxLevels;   // 5744: the totals [876]
static_assert(kFsOffFin + kFsRowMax <= kFsStage, "the reduction's parts fit the staging area");
static_assert(kFsSub * kFsBlocks <= kFsThreads, "a thread per (subset, block)");

struct FullcovGeom { int W; int64_t U; };

FullcovGeom fullcov_geom(const g2k_dims& d) {
  const int64_t slots = (int64_t)d.S * d.F * d.Nmax;
  int64_t w = (slots + kFsSlots - 1) / kFsSlots;
  if (w > kFsMaxWgs) w = kFsMaxWgs;
  if (w < 1) w = 1;
  FullcovGeom g;
  g.W = (int)w;
  g.U = (slots + w - 1) / w;
  return g;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Gram entry (i, j), i >= j, of the totals
__device__ __forceinline__ double gram_at(const long long* fin, int i, int j) {
  const int I = i >> 2, J = j >> 2;
  return __longlong_as_double(fin[(I * (I + 1) / 2 + J) * 16 + (i & 3) * 4 + (j & 3)]);
}

// fin [460 + 13 NL] (LDS, the launch's totals) -> moments, stats, inside, fit;
// A [576] doubles of LDS for the Cholesky.  Every thread of the workgroup
// calls it (a barrier inside).
__device__ __forceinline__ void fullcov_finish(const long long* fin, double* A, int NL,
                                               const float* __restrict__ chol, int tid, int nthreads,
                                               double* __restrict__ moments,
                                               double* __restrict__ stats,
                                               long long* __restrict__ inside,
                                               float* __restrict__ fit) {
  const double n = gram_at(fin, kL2, kL2);
  for (int idx = tid; idx < (kL2 + 1) * kL2; idx += nthreads) {
    const int i = idx / kL2, j = idx - i * kL2;
    moments[idx] = i >= j ? gram_at(fin, i, j) : gram_at(fin, j, i);
  }
  if (tid < kL) {
    double nl = 0.0, q = 0.0;
    if (chol) {
      q = __longlong_as_double(fin[kFsGram + tid]);
      const double base = kFsLog2Pi + log((double)chol[(2 * tid) * kL2 + 2 * tid]) +
                          log((double)chol[(2 * tid + 1) * kL2 + 2 * tid + 1]);
      nl = n * base + 0.5 * q;
    }
    stats[tid * 4] = n;
    stats[tid * 4 + 1] = nl;
    stats[tid * 4 + 2] = q;
    stats[tid * 4 + 3] = 0.0;
  }
  if (inside)
    for (int i = tid; i < kFsCnt * NL; i += nthreads) inside[i] = fin[kFsVals + i];
  if (!fit) return;                                        // uniform
  for (int idx = tid; idx < kL2 * kL2; idx += nthreads) {
    const int i = idx / kL2, j = idx - i * kL2;
    double v = 0.0;
    if (n > 0.0) {
      if (j <= i) v = gram_at(fin, i, j) / n;
      if (j == i) v = v * (1.0 + 1e-6) + 1e-12;
    } else if (j == i) {
      v = 1.0;
    }
    A[idx] = v;
  }
  __syncthreads();
  // right-looking in wave 0, lane i keeps row i in registers (the column loop
  // is unrolled: every index is a constant); column j's entries travel by
  // lane shuffles, no barrier.  What a lane gathers above its diagonal is
  // never used.  The ridge keeps every pivot positive.
  if (tid < 64) {
    const int row = tid < kL2 ? tid : kL2 - 1;
    double a[kL2];
#pragma unroll
    for (int k = 0; k < kL2; ++k) a[k] = A[row * kL2 + k];
#pragma unroll
    for (int j = 0; j < kL2; ++j) {
      const double dj = sqrt(fmax(__shfl(a[j], j), DBL_MIN));
      const double l = tid == j ? dj : a[j] / dj;          // L[row][j] (unused for row < j)
      a[j] = l;
#pragma unroll
      for (int k = j + 1; k < kL2; ++k) a[k] -= l * __shfl(l, k);   // ... times L[k][j]
    }
    if (tid < kL2) {
#pragma unroll
      for (int k = 0; k < kL2; ++k) fit[tid * kL2 + k] = k <= tid ? (float)a[k] : 0.f;
    }
  }
}

__global__ void __launch_bounds__(kFsThreads) g2k_fullcov_stats_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ chol,
    const double* __restrict__ r2, int NL, int S, int F, int Nmax, int64_t total, int64_t U,
    int shared_targets, long long* __restrict__ rows, double* __restrict__ moments,
    double* __restrict__ stats, long long* __restrict__ inside, float* __restrict__ fit) {
  __shared__ double sm[kFsStage + kL2 * kL2];
  double* rsT = sm;                                        // [28][257]: row i, slot p
  double* Wm = sm + kFsStage;                              // [24][24] = L^-1
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const bool has = chol != nullptr;

  for (int idx = tid; idx < (kFsDim - kL2 - 1) * kFsPitch; idx += kFsThreads)
    rsT[(kL2 + 1) * kFsPitch + idx] = 0.0;                 // the rows of zeros, once
  if (has) {                                               // uniform
    // L in double in the (still unused) rows 0..2 of the staging area, then
    // column tid of W = L^-1 by forward substitution, L w = e_tid, in
    // registers: the loops are unrolled, the reads of L broadcast
    double* Ls = rsT;
    for (int idx = tid; idx < kL2 * kL2; idx += kFsThreads) {
      const int i = idx / kL2, j = idx - i * kL2;
      double v = 0.0;
      if (j <= i) v = (double)chol[idx];
      Ls[idx] = v;
    }
    __syncthreads();
    if (tid < kL2) {
      double wc[kL2];
#pragma unroll
      for (int i = 0; i < kL2; ++i) {
        double acc = i == tid ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) acc = fma(-Ls[i * kL2 + k], wc[k], acc);
        wc[i] = acc / Ls[i * kL2 + i];
      }
#pragma unroll
      for (int i = 0; i < kL2; ++i) Wm[i * kL2 + tid] = wc[i];
    }
  }
  // lane l keeps level l: its two radii and its counts
  const double r2s = lane < NL ? r2[lane] : 0.0;           // the steps' (chi^2(2))
  const double r2j = lane < NL ? r2[NL + lane] : 0.0;      // the joint's (chi^2(24))
  const int r2slo = __double2loint(r2s), r2shi = __double2hiint(r2s);
  const int r2jlo = __double2loint(r2j), r2jhi = __double2hiint(r2j);
  int cl[kFsCnt];
#pragma unroll
  for (int t = 0; t < kFsCnt; ++t) cl[t] = 0;
  double qa[kL];
#pragma unroll
  for (int t = 0; t < kL; ++t) qa[t] = 0.0;

  // the Gram block of this thread: b = I (I + 1) / 2 + J, I >= J
  const int gsub = tid / kFsBlocks, gb = tid - gsub * kFsBlocks;
  int gI = 0;
  while ((gI + 1) * (gI + 2) / 2 <= gb) ++gI;
  const int gJ = gb - gI * (gI + 1) / 2;
  double g[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) g[a][c] = 0.0;

  const int64_t i0 = (int64_t)blockIdx.x * U;
  const int64_t left = total - i0;
  const int cnt = (int)(left < 0 ? 0 : (left < U ? left : U));
  const int64_t sf0 = i0 / Nmax;
  const int n0 = (int)(i0 - sf0 * Nmax);
  const int Fd = F > 0 ? F : 1;                            // F == 0: no slot, nothing divided
  __syncthreads();

  for (int base = 0; base < cnt; base += kFsThreads) {     // uniform trip count
    const int jslot = base + tid;
    const bool valid = jslot < cnt;
    const int jj = n0 + (valid ? jslot : 0);
    const int sfl = jj / Nmax;
    const int n = jj - sfl * Nmax;
    const int sf = (int)sf0 + sfl;                         // < S F <= INT32_MAX
    const int s = sf / Fd;
    const int f = sf - s * F;
    const int sl = min(s, S - 1);                          // a lane past the range: in bounds, off
    const int na = n_active[sl];
    const int nf = n_frames ? n_frames[sl] : F;
    const int mk = ped_mask ? ped_mask[(size_t)sl * Nmax + n] : 1;
    const bool on = valid & (n < clampi(na, 0, Nmax)) & (f < clampi(nf, 0, F)) & (mk != 0);
    double r[kL2];
    if (on) {
      const size_t pb = (size_t)sf * kL2 * Nmax + n;
      const size_t tf = shared_targets ? (size_t)s : (size_t)sf;
      const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf * Nmax + n) * kL;
      float px[kL], py[kL];
      float2 tg[kL];
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        px[t] = pred[pb + (size_t)t * Nmax];
        py[t] = pred[pb + (size_t)(kL + t) * Nmax];
        tg[t] = t2[t];
      }
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        r[2 * t] = (double)tg[t].x - (double)px[t];
        r[2 * t + 1] = (double)tg[t].y - (double)py[t];
      }
    } else {
#pragma unroll
      for (int i = 0; i < kL2; ++i) r[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < kL2; ++i) rsT[i * kFsPitch + tid] = r[i];
    rsT[kL2 * kFsPitch + tid] = on ? 1.0 : 0.0;
    if (has) {                                             // uniform
      double qsum = 0.0;
#pragma unroll
      for (int t = 0; t < kL; ++t) {
        double z0 = 0.0, z1 = 0.0;
#pragma unroll
        for (int k = 0; k <= 2 * t; ++k) z0 = fma(Wm[(2 * t) * kL2 + k], r[k], z0);
#pragma unroll
        for (int k = 0; k <= 2 * t + 1; ++k) z1 = fma(Wm[(2 * t + 1) * kL2 + k], r[k], z1);
        const double qt = z0 * z0 + z1 * z1;               // 0 for a non-pair
        qa[t] += qt;
        qsum += qt;
        for (int l = 0; l < NL; ++l) {                     // uniform; every lane takes part
          const double rr = __hiloint2double(__builtin_amdgcn_readlane(r2shi, l),
                                             __builtin_amdgcn_readlane(r2slo, l));
          const int c = __popcll(__ballot(on && qt <= rr));
          cl[t] += lane == l ? c : 0;
        }
      }
      for (int l = 0; l < NL; ++l) {
        const double rr = __hiloint2double(__builtin_amdgcn_readlane(r2jhi, l),
                                           __builtin_amdgcn_readlane(r2jlo, l));
        const int c = __popcll(__ballot(on && qsum <= rr));
        cl[kL] += lane == l ? c : 0;
      }
    }
    __syncthreads();
    if (tid < kFsSub * kFsBlocks) {
      for (int p = gsub; p < kFsThreads; p += kFsSub) {
        double x[4], y[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          x[a] = rsT[(4 * gI + a) * kFsPitch + p];
          y[a] = rsT[(4 * gJ + a) * kFsPitch + p];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) g[a][c] = fma(x[a], y[c], g[a][c]);
      }
    }
    __syncthreads();
  }

  // the workgroup's row: the subsets in order, the waves (w0 + w1) + (w2 + w3)
  double* part = sm;
  double* qpart = sm + kFsOffQ;
  long long* cpart = reinterpret_cast<long long*>(sm + kFsOffCnt);
  long long* fin = reinterpret_cast<long long*>(sm + kFsOffFin);
  if (tid < kFsSub * kFsBlocks) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) part[gsub * kFsGram + gb * 16 + a * 4 + c] = g[a][c];
  }
#pragma unroll
  for (int t = 0; t < kL; ++t) {
    const double v = wave_sum_d(qa[t]);
    if (lane == 0) qpart[w * kL + t] = v;
  }
#pragma unroll
  for (int t = 0; t < kFsCnt; ++t)
    if (lane < NL) cpart[(w * kFsCnt + t) * kFsMaxLevels + lane] = (long long)cl[t];
  __syncthreads();
  const int nv = kFsVals + kFsCnt * NL;
  for (int i = tid; i < nv; i += kFsThreads) {
    long long v;
    if (i < kFsGram) {
      double sacc = part[i];
#pragma unroll
      for (int k = 1; k < kFsSub; ++k) sacc += part[k * kFsGram + i];
      v = __double_as_longlong(sacc);
    } else if (i < kFsVals) {
      const int t = i - kFsGram;
      v = __double_as_longlong((qpart[t] + qpart[kL + t]) + (qpart[2 * kL + t] + qpart[3 * kL + t]));
    } else {
      const int k = i - kFsVals;
      const int t = k / NL, l = k - t * NL;
      const long long* c0 = cpart + t * kFsMaxLevels + l;
      const int ws = kFsCnt * kFsMaxLevels;
      v = (c0[0] + c0[ws]) + (c0[2 * ws] + c0[3 * ws]);
    }
    if (rows) rows[(size_t)blockIdx.x * nv + i] = v;
    else fin[i] = v;
  }
  if (!rows) {
    __syncthreads();
    fullcov_finish(fin, Wm, NL, chol, tid, kFsThreads, moments, stats, inside, fit);
  }
}

// the W rows added in row order (16 loads in flight), then the outputs
__global__ void __launch_bounds__(kFsRowsThreads) g2k_fullcov_rows_kernel(
    const long long* __restrict__ rows, int W, int NL, const float* __restrict__ chol,
    double* __restrict__ moments, double* __restrict__ stats, long long* __restrict__ inside,
    float* __restrict__ fit) {
  __shared__ long long fin[kFsRowMax];
  __shared__ double A[kL2 * kL2];
  const int tid = threadIdx.x;
  const int nv = kFsVals + kFsCnt * NL;
  if (tid < nv) {
    const bool fp = tid < kFsVals;                         // doubles, then int64 counts
    long long v = 0;                                       // +0.0 and 0 alike
    for (int r0 = 0; r0 < W; r0 += 16) {
      long long x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) x[u] = rows[(size_t)min(r0 + u, W - 1) * nv + tid];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        if (r0 + u >= W) x[u] = 0;
        v = fp ? __double_as_longlong(__longlong_as_double(v) + __longlong_as_double(x[u])) : v + x[u];
      }
    }
    fin[tid] = v;
  }
  __syncthreads();
  fullcov_finish(fin, A, NL, chol, tid, kFsRowsThreads, moments, stats, inside, fit);
}

}  // namespace

// one row [460 + 13 NL] of 8-byte words per workgroup; none when one
// workgroup covers the launch
int64_t fullcov_stats_ws_bytes(const g2k_dims* d, int n_levels) {
  const FullcovGeom g = fullcov_geom(*d);
  return g.W > 1 ? (int64_t)g.W * (kFsVals + kFsCnt * n_levels) * 8 : 0;
}

int fullcov_stats_launch(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                         const float* chol, const double* r2, int n_levels, double* moments,
                         double* stats, int64_t* inside, float* fit, void* workspace, hipStream_t st) {
  const FullcovGeom g = fullcov_geom(*d);
  const int64_t total = (int64_t)d->S * d->F * d->Nmax;
  const int NL = inside ? n_levels : 0;                    // no counts asked for: none made
  long long* rows = g.W > 1 ? static_cast<long long*>(workspace) : nullptr;
  hipLaunchKernelGGL(g2k_fullcov_stats_kernel, dim3((unsigned)g.W), dim3(kFsThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, chol, r2, NL, d->S, d->F, d->Nmax, total,
                     g.U, (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0, rows, moments, stats,
                     reinterpret_cast<long long*>(inside), fit);
  int rc = check_launch("g2k_fullcov_stats_kernel");
  if (rc || g.W == 1) return rc;
  hipLaunchKernelGGL(g2k_fullcov_rows_kernel, dim3(1), dim3(kFsRowsThreads), 0, st, rows, g.W, NL, chol,
                     moments, stats, reinterpret_cast<long long*>(inside), fit);
  return check_launch("g2k_fullcov_rows_kernel");
}

int fullcov_sample_launch(const g2k_dims* d, const float* pred, const float* chol, uint64_t seed,
                          float* out, hipStream_t st) {
  const int64_t slots = (int64_t)d->S * d->F * d->Nmax;
  const int64_t wgs = (slots + 255) / 256;
  if (wgs > 0x7fffffff) return set_err(G2K_EINVAL, "fullcov_sample: %lld workgroups", (long long)wgs);
  hipLaunchKernelGGL(g2k_fullcov_sample_kernel, dim3((unsigned)wgs), dim3(256), 0, st, pred, chol, slots,
                     d->Nmax, (uint32_t)seed, (uint32_t)(seed >> 32), out);
  return check_launch("g2k_fullcov_sample_kernel");
}

}  // namespace g2k
