// g2k_coupled.hip — the scene-coupled trajectory head (include/g2k_coupled.h
// states the definition): r_gi = c_g + e_gi, c_g ~ N(0, B) one per scene-frame,
// e_gi ~ N(0, W) one per member.  Its sums for the closed-form fit and its
// exact likelihood (g2k_coupled_stats_f32) and its sampler
// (g2k_coupled_sample_f32); the fused evaluations over its joint draws
// (g2k_coupled_joint_eval_f32, g2k_coupled_couple_scores_f32) are the shared
// kernels of g2k_joint.hip and g2k_couples.hip with this head's policy
// (CoupledHead, g2k_head_draw.h), which the sampler below calls too: a draw
// made inside a fused evaluation is, bit for bit, the sampler's.  The build's:
// the reference has no probabilistic head, so PARITY UNPINNED; pinned against
// tests/coupled_ref.py.
//
// Stats.  A group is a scene-frame, so a workgroup of 256 threads takes WHOLE
// scene-frames, a contiguous range of them (coupled_geom: at least 256 columns'
// worth each, at most 256 workgroups), one at a time, thread n looking at
// column n.  Per scene-frame: the members' residuals in double, their mean
// (lanes by butterfly, the four waves in order), the centred residuals staged
// in LDS as 24 rows x 256 columns, and SSW's lower triangle taken from there as
// fullcov_stats_kernel takes its Gram: thread (g, b) owns the 4 x 4 block b of
// the triangle's 21 over the columns g, g + 12, ... < Nmax.  SSB's 576 entries
// are dealt to the threads, P rbar rbar^T added per scene-frame.  With whiten,
// thread d < 24 forms ybar_d = (A rbar)_d and the group's two terms; a member's
// thread forms A (r - rbar), 576 double FMAs on broadcast LDS reads, and from
// it and ybar both quadratic forms.  Reduction: the twelve column subsets in
// order, the waves (w0 + w1) + (w2 + w3).  One workgroup finishes in the same
// kernel; otherwise the rows [920] (8-byte words) go to the workspace and
// coupled_rows_kernel (one workgroup) adds them in row order and finishes.  No
// atomics.  Several scene-frames per round when Nmax is small would fill the
// Gram's threads better; not built.
#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_coupled.h"
#include "g2k_head_draw.h"

namespace g2k {
namespace {

static_assert((((uint64_t)kCoupledSaltHi << 32) | kCoupledSaltLo) == G2K_COUPLED_SALT,
              "g2k_head_draw.h's salt is the header's");
static_assert(G2K_COUPLED_DIM == kL2, "24 coordinates");

// ---------------------------------------------------------------------------
// the sampler: one thread per (s, f, n), the policy's draw
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) coupled_sample_kernel(
    const float* __restrict__ pred, const float* __restrict__ cpl, int64_t slots, int Nmax,
    uint32_t seed_lo, uint32_t seed_hi, float* __restrict__ out) {
  __shared__ CoupledHead::Lds hlds;
  CoupledHead::stage<256>(cpl, hlds, threadIdx.x);
  __syncthreads();
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= slots) return;
  CoupledHead head;
  head.bind(hlds);
  const int64_t sf = id / Nmax;
  const int n = (int)(id - sf * Nmax);
  const size_t pb = (size_t)sf * kL2 * Nmax + n;
  const int64_t e0 = sf * kL * Nmax + n;                   // element of step 0
  float mu[kL2];
#pragma unroll
  for (int t = 0; t < kL; ++t) {
    mu[2 * t] = pred[pb + (size_t)t * Nmax];
    mu[2 * t + 1] = pred[pb + (size_t)(kL + t) * Nmax];
  }
  head.draw(seed_lo, seed_hi, e0, n, Nmax, mu, [&](int t, float x, float y) {
    out[pb + (size_t)t * Nmax] = x;
    out[pb + (size_t)(kL + t) * Nmax] = y;
  });
}

// ---------------------------------------------------------------------------
// stats
// ---------------------------------------------------------------------------
constexpr int kCsThreads = 256;
constexpr int kCsPitch = kCsThreads + 1;       // odd: a scene-frame's rows start one 8-byte bank apart
constexpr int kCsBlocks = 21;                  // 4 x 4 blocks of the 6 x 6 lower triangle
constexpr int kCsSub = 12;                     // column subsets: 12 * 21 = 252 threads
constexpr int kCsGram = kCsBlocks * 16;        // 336
constexpr int kCsSq = kL2 * kL2;               // 576
constexpr int kCsOffB = kCsGram;               // a row: SSW's blocks, SSB, 4 sums, 4 counts
constexpr int kCsOffQ = kCsOffB + kCsSq;       // 912: q_within, the independent head's, q_between, logs
constexpr int kCsOffN = kCsOffQ + 4;           // 916: the counts (int64)
constexpr int kCsRow = kCsOffN + G2K_COUPLED_COUNTS;   // 920
constexpr int kCsCols = 256;                   // columns per workgroup, at least
constexpr int kCsMaxWgs = 256;
constexpr int kCsRowsThreads = 1024;
// LDS of the stats kernel, in doubles: the staged scene-frame; after the last
// one the staging area holds the reduction's parts and the totals
constexpr int kCsStage = kL2 * kCsPitch;       // 6168
constexpr int kCsOffPart = kCsSub * kCsGram;   // 4032: the waves' sums [4][2]
constexpr int kCsOffFin = kCsOffPart + 8;      // 4040: the totals [920]
static_assert(kCsOffFin + kCsRow <= kCsStage, "the reduction's parts fit the staging area");
static_assert(kCsSub * kCsBlocks <= kCsThreads, "a thread per (subset, block)");
static_assert(kCsRow <= kCsRowsThreads, "a thread per column of the rows");

struct CoupledGeom { int W; int64_t U; };      // workgroups, scene-frames each

CoupledGeom coupled_geom(const g2k_dims& d) {
  const int64_t sf = (int64_t)d.S * d.F;
  const int64_t per = (kCsCols + d.Nmax - 1) / d.Nmax;     // scene-frames per workgroup, at least
  int64_t w = (sf + per - 1) / per;
  if (w > kCsMaxWgs) w = kCsMaxWgs;
  if (w < 1) w = 1;
  CoupledGeom g;
  g.W = (int)w;
  g.U = (sf + w - 1) / w;
  return g;
}

__device__ __forceinline__ double cs_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// SSW entry (i, j), i >= j, of the totals
__device__ __forceinline__ double cs_gram_at(const long long* fin, int i, int j) {
  const int I = i >> 2, J = j >> 2;
  return __longlong_as_double(fin[(I * (I + 1) / 2 + J) * 16 + (i & 3) * 4 + (j & 3)]);
}

// fin [920] (LDS, the launch's totals) -> within, between, counts, stats
__device__ __forceinline__ void coupled_finish(const long long* fin, const double* __restrict__ whiten,
                                               int tid, int nthreads, double* __restrict__ within,
                                               double* __restrict__ between,
                                               long long* __restrict__ counts,
                                               double* __restrict__ stats) {
  for (int idx = tid; idx < kCsSq; idx += nthreads) {
    const int i = idx / kL2, j = idx - i * kL2;
    const int hi = i >= j ? i : j, lo = i >= j ? j : i;
    within[idx] = cs_gram_at(fin, hi, lo);
    between[idx] = __longlong_as_double(fin[kCsOffB + hi * kL2 + lo]);
  }
  if (tid < G2K_COUPLED_COUNTS) counts[tid] = fin[kCsOffN + tid];
  if (tid == 0) {
    double o[G2K_COUPLED_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (whiten) {
      const double qw = __longlong_as_double(fin[kCsOffQ]), qi = __longlong_as_double(fin[kCsOffQ + 1]);
      const double qb = __longlong_as_double(fin[kCsOffQ + 2]), lg = __longlong_as_double(fin[kCsOffQ + 3]);
      double l1 = 0.0;
      for (int dd = 0; dd < kL2; ++dd) l1 += log1p(whiten[kCsSq + dd]);
      o[0] = 0.5 * ((qw + qb) + lg);
      o[1] = 0.5 * (qi + (double)fin[kCsOffN] * l1);
      o[2] = qw; o[3] = qb; o[4] = lg;
    }
#pragma unroll
    for (int i = 0; i < G2K_COUPLED_STATS; ++i) stats[i] = o[i];
  }
}

__global__ void __launch_bounds__(kCsThreads) coupled_stats_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const double* __restrict__ whiten, int F, int Nmax,
    int64_t total, int64_t U, int shared_targets, long long* __restrict__ rows,
    double* __restrict__ within, double* __restrict__ between, long long* __restrict__ counts,
    double* __restrict__ stats) {
  __shared__ double sm[kCsStage];                          // eT [24][257]: row i, column n
  __shared__ double Am[kCsSq];                             // A
  __shared__ double lam[kL2], inv1[kL2];                   // lambda, 1 / (1 + lambda)
  __shared__ double mpart[4][kL2];
  __shared__ double rbar[kL2], ybar[kL2];
  __shared__ int wcnt[4];
  double* eT = sm;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const bool has = whiten != nullptr;
  if (has) {                                               // uniform
    for (int idx = tid; idx < kCsSq; idx += kCsThreads) Am[idx] = whiten[idx];
    if (tid < kL2) {
      const double l = whiten[kCsSq + tid];
      lam[tid] = l;
      inv1[tid] = 1.0 / (1.0 + l);
    }
  }
  // the SSW block of this thread: b = I (I + 1) / 2 + J, I >= J
  const int gsub = tid / kCsBlocks, gb = tid - gsub * kCsBlocks;
  int gI = 0;
  while ((gI + 1) * (gI + 2) / 2 <= gb) ++gI;
  const int gJ = gb - gI * (gI + 1) / 2;
  double g[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) g[a][c] = 0.0;
  double sb[3] = {0.0, 0.0, 0.0};                          // SSB entries tid, tid + 256, tid + 512
  double qw = 0.0, qi = 0.0;                               // this column's members
  double qb = 0.0, lg = 0.0;                               // coordinate tid < 24 of the groups
  long long cN = 0, cG = 0, cG2 = 0, cPP = 0;              // uniform

  const int64_t sf0 = (int64_t)blockIdx.x * U;
  const int64_t sf1 = sf0 + U < total ? sf0 + U : total;
  __syncthreads();
#pragma nounroll
  for (int64_t sf = sf0; sf < sf1; ++sf) {                 // uniform
    const int s = (int)(sf / F), f = (int)(sf - (int64_t)s * F);
    const int nact = clampi(n_active[s], 0, Nmax);
    const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
    bool on = f < nf && tid < nact;
    if (on && ped_mask) on = ped_mask[(size_t)s * Nmax + tid] != 0;
    const unsigned long long bal = __ballot(on);
    if (lane == 0) wcnt[w] = __popcll(bal);
    double r[kL2];
    if (on) {
      const size_t pb = (size_t)sf * kL2 * Nmax + tid;
      const size_t tf = shared_targets ? (size_t)s : (size_t)sf;
      const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf * Nmax + tid) * kL;
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
    for (int i = 0; i < kL2; ++i) {
      const double v = cs_wave_sum(r[i]);
      if (lane == 0) mpart[w][i] = v;
    }
    __syncthreads();
    const int P = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    if (P == 0) {                                          // uniform: nothing of this scene-frame
      __syncthreads();                                     // wcnt, mpart: read before the next one's
      continue;
    }
    if (tid < kL2)
      rbar[tid] = ((mpart[0][tid] + mpart[1][tid]) + (mpart[2][tid] + mpart[3][tid])) / (double)P;
    __syncthreads();
    cN += P; cG += 1; cG2 += P >= 2 ? 1 : 0; cPP += (long long)P * P;
#pragma unroll
    for (int i = 0; i < kL2; ++i) {
      r[i] = on ? r[i] - rbar[i] : 0.0;                    // centred
      eT[i * kCsPitch + tid] = r[i];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int idx = q * kCsThreads + tid;
      if (idx < kCsSq) {
        const int i = idx / kL2, j = idx - i * kL2;
        sb[q] = fma((double)P * rbar[i], rbar[j], sb[q]);
      }
    }
    if (has && tid < kL2) {                                // the group's terms of coordinate tid
      double yb = 0.0;
#pragma unroll
      for (int k = 0; k < kL2; ++k) yb = fma(Am[tid * kL2 + k], rbar[k], yb);
      ybar[tid] = yb;
      const double pl = (double)P * lam[tid];
      qb += (double)P * yb * yb / (1.0 + pl);
      lg += log1p(pl);
    }
    __syncthreads();
    if (tid < kCsSub * kCsBlocks) {
      for (int p = gsub; p < Nmax; p += kCsSub) {
        double x[4], y[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          x[a] = eT[(4 * gI + a) * kCsPitch + p];
          y[a] = eT[(4 * gJ + a) * kCsPitch + p];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) g[a][c] = fma(x[a], y[c], g[a][c]);
      }
    }
    if (has && on) {
#pragma unroll 2
      for (int dd = 0; dd < kL2; ++dd) {
        double yc = 0.0;
#pragma unroll
        for (int k = 0; k < kL2; ++k) yc = fma(Am[dd * kL2 + k], r[k], yc);
        const double y = yc + ybar[dd];
        qw = fma(yc, yc, qw);
        qi = fma(y * y, inv1[dd], qi);
      }
    }
    __syncthreads();                                       // eT, ybar, wcnt, mpart: read
  }

  // the workgroup's row: the subsets in order, the waves (w0 + w1) + (w2 + w3)
  double* part = sm;
  double* qpart = sm + kCsOffPart;
  long long* fin = reinterpret_cast<long long*>(sm + kCsOffFin);
  long long* dst = rows ? rows + (size_t)blockIdx.x * kCsRow : fin;
  if (tid < kCsSub * kCsBlocks) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) part[gsub * kCsGram + gb * 16 + a * 4 + c] = g[a][c];
  }
  {
    const double a = cs_wave_sum(qw), b = cs_wave_sum(qi);
    if (lane == 0) { qpart[w * 2] = a; qpart[w * 2 + 1] = b; }
  }
  // wave 0 holds the groups' terms in its lanes < 24 (zeros elsewhere)
  const double qbs = cs_wave_sum(qb), lgs = cs_wave_sum(lg);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int idx = q * kCsThreads + tid;
    if (idx < kCsSq) dst[kCsOffB + idx] = __double_as_longlong(sb[q]);
  }
  __syncthreads();
  for (int i = tid; i < kCsGram; i += kCsThreads) {
    double sacc = part[i];
#pragma unroll
    for (int k = 1; k < kCsSub; ++k) sacc += part[k * kCsGram + i];
    // fin lies past the parts: no thread's part is overwritten
    dst[i] = __double_as_longlong(sacc);
  }
  if (tid == 0) {
    dst[kCsOffQ] = __double_as_longlong((qpart[0] + qpart[2]) + (qpart[4] + qpart[6]));
    dst[kCsOffQ + 1] = __double_as_longlong((qpart[1] + qpart[3]) + (qpart[5] + qpart[7]));
    dst[kCsOffQ + 2] = __double_as_longlong(qbs);
    dst[kCsOffQ + 3] = __double_as_longlong(lgs);
    dst[kCsOffN] = cN; dst[kCsOffN + 1] = cG; dst[kCsOffN + 2] = cG2; dst[kCsOffN + 3] = cPP;
  }
  if (!rows) {
    __syncthreads();
    coupled_finish(fin, whiten, tid, kCsThreads, within, between, counts, stats);
  }
}

// the W rows added in row order (16 loads in flight), then the outputs
__global__ void __launch_bounds__(kCsRowsThreads) coupled_rows_kernel(
    const long long* __restrict__ rows, int W, const double* __restrict__ whiten,
    double* __restrict__ within, double* __restrict__ between, long long* __restrict__ counts,
    double* __restrict__ stats) {
  __shared__ long long fin[kCsRow];
  const int tid = threadIdx.x;
  if (tid < kCsRow) {
    const bool fp = tid < kCsOffN;                         // doubles, then int64 counts
    long long v = 0;                                       // +0.0 and 0 alike
    for (int r0 = 0; r0 < W; r0 += 16) {
      long long x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) x[u] = rows[(size_t)min(r0 + u, W - 1) * kCsRow + tid];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        if (r0 + u >= W) x[u] = 0;
        v = fp ? __double_as_longlong(__longlong_as_double(v) + __longlong_as_double(x[u])) : v + x[u];
      }
    }
    fin[tid] = v;
  }
  __syncthreads();
  coupled_finish(fin, whiten, tid, kCsRowsThreads, within, between, counts, stats);
}

inline bool coupled_stats_sizes_ok(const g2k_dims* d) {
  return pair_sizes_ok(d) && (int64_t)d->S * d->F <= 0x7fffffff;
}

// one row [920] of 8-byte words per workgroup; none when one workgroup covers
// the launch
int64_t coupled_stats_ws_bytes(const g2k_dims* d) {
  const CoupledGeom g = coupled_geom(*d);
  return g.W > 1 ? (int64_t)g.W * kCsRow * 8 : 0;
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

int64_t g2k_coupled_stats_workspace_bytes(const g2k_dims* d) {
  if (!d || !coupled_stats_sizes_ok(d)) return -1;
  return coupled_stats_ws_bytes(d);
}

int g2k_coupled_stats_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                          const double* whiten, double* within, double* between, int64_t* counts,
                          double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & ~G2K_STEP_TARGETS_SHARED)
    return set_err(G2K_EUNSUPPORTED, "coupled_stats: flags %d (0 or G2K_STEP_TARGETS_SHARED)", d->flags);
  if (!coupled_stats_sizes_ok(d))
    return set_err(G2K_EINVAL, "S=%d F=%d Nmax=%d (Nmax 1..256, S F < 2^31)", d->S, d->F, d->Nmax);
  if (const int rc = check_required({pred, targets, n_active, within, between, counts, stats})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if ((((uintptr_t)whiten) | ((uintptr_t)within) | ((uintptr_t)between) | ((uintptr_t)counts) |
       ((uintptr_t)stats)) & 7)
    return set_err(G2K_EINVAL, "whiten, within, between, counts and stats must be 8-byte aligned");
  // rows of doubles and int64 counts: a workspace that is named is held to it,
  // whether or not this launch needs one
  if (workspace && (((uintptr_t)workspace) & 7))
    return set_err(G2K_EINVAL, "workspace must be 8-byte aligned");
  const int64_t need = coupled_stats_ws_bytes(d);
  if (d->S > 0 && need > 0 && (!workspace || workspace_bytes < need))
    return set_err(G2K_EINVAL, "workspace of %lld bytes needed (got %lld), 8-byte aligned",
                   (long long)need, (long long)workspace_bytes);
  if (d->S == 0) return G2K_OK;
  const CoupledGeom g = coupled_geom(*d);
  hipStream_t st = (hipStream_t)stream;
  long long* rows = g.W > 1 ? static_cast<long long*>(workspace) : nullptr;
  hipLaunchKernelGGL(coupled_stats_kernel, dim3((unsigned)g.W), dim3(kCsThreads), 0, st, pred, targets,
                     n_active, n_frames, ped_mask, whiten, d->F, d->Nmax, (int64_t)d->S * d->F, g.U,
                     (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0, rows, within, between,
                     reinterpret_cast<long long*>(counts), stats);
  const int rc = check_launch("coupled_stats_kernel");
  if (rc || g.W == 1) return rc;
  hipLaunchKernelGGL(coupled_rows_kernel, dim3(1), dim3(kCsRowsThreads), 0, st, rows, g.W, whiten, within,
                     between, reinterpret_cast<long long*>(counts), stats);
  return check_launch("coupled_rows_kernel");
}

int g2k_coupled_sample_f32(const g2k_dims* d, const float* pred, const float* cpl, uint64_t seed,
                           float* out, void* stream) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & G2K_STEP_PRED_PED_MAJOR)
    return set_err(G2K_EUNSUPPORTED, "coupled_sample reads pred_path_band [S, F, 2L, Nmax]");
  if (const int rc = check_pair_sizes(d)) return rc;
  if (const int rc = check_required({pred, cpl, out})) return rc;
  const int64_t slots = (int64_t)d->S * d->F * d->Nmax;
  if (slots == 0) return G2K_OK;
  const int64_t wgs = (slots + 255) / 256;
  if (wgs > 0x7fffffff) return set_err(G2K_EINVAL, "coupled_sample: %lld workgroups", (long long)wgs);
  hipLaunchKernelGGL(coupled_sample_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, pred,
                     cpl, slots, d->Nmax, (uint32_t)seed, (uint32_t)(seed >> 32), out);
  return check_launch("coupled_sample_kernel");
}

}  // extern "C"
