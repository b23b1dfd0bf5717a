// g2k_calib.hip — calibration of the bivariate-Gaussian head (g2k_nll.hip):
// the per-step residual moments, their closed-form maximum-likelihood head,
// and the coverage / NLL of a given head, in one pass over pred and targets.
// The build's: the reference has no probabilistic head, so PARITY UNPINNED;
// tests/calib_ref.py restates the definition in float64 NumPy.
//
// Definition.  Inputs as g2k_best_of_k_f32: pred [S, F, 2L, Nmax] (band
// layout), targets [S, F, Nmax, L, 2] ([S, 1, Nmax, L, 2] with
// G2K_STEP_TARGETS_SHARED), n_active [S], n_frames [S] or NULL, ped_mask
// [S, Nmax] or NULL, head [3, 12] or NULL, r2 [NL] doubles (NL in 0..32).  A
// pair is (s, f, n) with f < n_frames[s], n < n_active[s], ped_mask[s][n] != 0.
// For pair and step t, all in double (the f32 inputs' differences are exact):
//   dx = target_x - pred_x, dy = target_y - pred_y
//   a = dx / sigma_x, b = dy / sigma_y, c = 1 - rho^2   (head: log sigma_x,
//     log sigma_y, atanh rho)
//   q   = (a^2 + b^2 - 2 rho a b) / c        squared Mahalanobis distance
//   nll = log 2 pi + log sigma_x + log sigma_y + 1/2 log c + q / 2
// Outputs (every element written):
//   stats [12][8] double = {pairs, S dx, S dy, S dx^2, S dy^2, S dx dy,
//     S nll_t, S q_t} over the pairs; columns 6, 7 exactly 0 without a head
//   inside [12][NL] int64 (or NULL): pairs with q_t <= r2[l]
//   fit [3][12] f32 (or NULL): the head that minimises the NLL (no bias term:
//     the uncentred second moments):
//     log sigma_x = 1/2 ln max(S dx^2 / n, 1e-12), log sigma_y likewise,
//     atanh rho with rho = S dx dy / sqrt(S dx^2 S dy^2) clamped to
//     +-(1 - 1e-6), 0 when either sum is 0; zeros for a step with n = 0
//
// Geometry.  A slot is (s, f, n), n < Nmax; the S F Nmax slots are dealt in
// W contiguous ranges to W workgroups of 1024 threads (calib_geom: at least
// 512 slots each, at most 256 workgroups: one per CU, 4 waves per SIMD).  The
// 16 waves are 4 groups of 4: wave w of group g owns the steps w, w + 4, w + 8
// and walks the range's slots g 64 .. g 64 + 63, then 256 further on, lane
// along n: a pred row is read coalesced along n, a target by one 8-byte load
// (rows of 96 bytes: the four waves of a group use up every line between
// them).  Non-pairs load nothing; a round's three index loads (n_active,
// n_frames, the mask byte) are independent and unconditional: one round trip.  Per lane 3 x 7 double sums; the
// level counts by ballot: for level l the wave's count is a popcount, kept
// by lane l (lane l also holds r2[l]: no per-thread array, no scratch).  The
// per-step constants are formed in double by threads 0..11, once per
// workgroup; the loop has no transcendental and no division.
// Reduction: lanes by butterfly; within a group a step belongs to one wave;
// the four groups' rows [96 + 12 NL] (8-byte words: doubles, then int64
// counts) are added in LDS, (g0 + g1) + (g2 + g3).  W == 1 writes the outputs
// directly; otherwise the rows go to the caller's workspace and
// g2k_head_stats_rows_kernel (one workgroup of 1024 threads) adds them in an
// order fixed by W: 32 interleaved slices per value (all of a thread's loads
// of two rounds in flight together), then the slices in order.  No atomics:
// repeated calls are bit-identical, and the moments' bits do not depend on the
// head or the levels.
#include "g2k_common.h"

namespace g2k {
namespace {

constexpr int kCbThreads = 1024;
constexpr int kCbGroups = kCbThreads / 256;   // 4 groups of 4 waves
constexpr int kCbSlots = 512;         // slots per workgroup, at least
constexpr int kCbMaxWgs = 256;
constexpr int kCbMaxLevels = 32;
constexpr int kCbStats = kL * 8;      // 96
constexpr int kCbRowMax = kCbStats + kL * kCbMaxLevels;   // 480
constexpr int kCbRowsThreads = 1024;
constexpr double kCbLog2Pi = 1.8378770664093454835606594728112;

struct CalibGeom { int W; int64_t U; };

CalibGeom calib_geom(const g2k_dims& d) {
  const int64_t slots = (int64_t)d.S * d.F * d.Nmax;
  int64_t w = (slots + kCbSlots - 1) / kCbSlots;
  if (w > kCbMaxWgs) w = kCbMaxWgs;
  if (w < 1) w = 1;
  CalibGeom g;
  g.W = (int)w;
  g.U = (slots + w - 1) / w;
  return g;
}

struct CalibStep { double isx, isy, rho, ic, base; };

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// fin [96 + 12 NL] (LDS, the launch's totals) -> stats, inside, fit
__device__ __forceinline__ void calib_finish(const long long* fin, int NL, int tid, int nthreads,
                                             double* __restrict__ stats,
                                             long long* __restrict__ inside,
                                             float* __restrict__ fit) {
  for (int i = tid; i < kCbStats; i += nthreads) stats[i] = __longlong_as_double(fin[i]);
  if (inside)
    for (int i = tid; i < kL * NL; i += nthreads) inside[i] = fin[kCbStats + i];
  if (fit && tid < kL) {
    const double n = __longlong_as_double(fin[tid * 8]);
    const double sxx = __longlong_as_double(fin[tid * 8 + 3]);
    const double syy = __longlong_as_double(fin[tid * 8 + 4]);
    const double sxy = __longlong_as_double(fin[tid * 8 + 5]);
    float lx = 0.f, ly = 0.f, r = 0.f;
    if (n > 0.0) {
      lx = (float)(0.5 * log(fmax(sxx / n, 1e-12)));
      ly = (float)(0.5 * log(fmax(syy / n, 1e-12)));
      double rho = 0.0;
      if (sxx != 0.0 && syy != 0.0) rho = sxy / sqrt(sxx * syy);
      rho = fmin(fmax(rho, -(1.0 - 1e-6)), 1.0 - 1e-6);
      r = (float)atanh(rho);
    }
    fit[tid] = lx;
    fit[kL + tid] = ly;
    fit[2 * kL + tid] = r;
  }
}

__global__ void __launch_bounds__(kCbThreads) g2k_head_stats_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head,
    const double* __restrict__ r2, int NL, int S, int F, int Nmax, int64_t total, int64_t U,
    int shared_targets, long long* __restrict__ rows, double* __restrict__ stats,
    long long* __restrict__ inside, float* __restrict__ fit) {
  __shared__ CalibStep hs[kL];
  __shared__ long long fin[kCbGroups][kCbRowMax];
  const int tid = threadIdx.x, lane = tid & 63;
  const int grp = wave_id() >> 2, w = wave_id() & 3;
  const bool has_head = head != nullptr;
  if (tid < kL && has_head) {
    const double lsx = (double)head[tid], lsy = (double)head[kL + tid];
    const double rho = tanh((double)head[2 * kL + tid]);
    const double c = 1.0 - rho * rho;
    CalibStep h;
    h.isx = exp(-lsx);
    h.isy = exp(-lsy);
    h.rho = rho;
    h.ic = 1.0 / c;
    h.base = kCbLog2Pi + lsx + lsy + 0.5 * log(c);
    hs[tid] = h;
  }
  __syncthreads();
  CalibStep cs[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (has_head) cs[k] = hs[w + 4 * k];
    else cs[k] = CalibStep{0.0, 0.0, 0.0, 0.0, 0.0};
  }
  // lane l keeps level l: its radius and its counts
  const double r2l = lane < NL ? r2[lane] : 0.0;
  const int r2lo = __double2loint(r2l), r2hi = __double2hiint(r2l);
  int cl[3] = {0, 0, 0};

  const int64_t i0 = (int64_t)blockIdx.x * U;
  const int64_t left = total - i0;
  const int cnt = (int)(left < 0 ? 0 : (left < U ? left : U));
  const int64_t sf0 = i0 / Nmax;
  const int n0 = (int)(i0 - sf0 * Nmax);

  double acc[3][7];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < 7; ++i) acc[k][i] = 0.0;
  int npairs = 0;                                          // wave-uniform

  // a lane's slot of the round that starts at `base`: is it a pair, and where
  // (the three index loads are independent of each other: one round trip)
  struct Slot { bool on; int sf, s, n; };
  const int Fd = F > 0 ? F : 1;                            // F == 0: no slot, nothing divided
  auto slot_at = [&](int base) {
    const int j = base + lane;
    const bool valid = j < cnt;
    const int jj = n0 + (valid ? j : 0);
    const int sfl = jj / Nmax;
    Slot q;
    q.n = jj - sfl * Nmax;
    q.sf = (int)sf0 + sfl;                                 // < S F <= INT32_MAX
    q.s = q.sf / Fd;
    // no branch around the loads (they can go out behind the data loads): a
    // lane past the range reads scene min(s, S - 1), in bounds, and is off
    const int sl = min(q.s, S - 1);
    const int f = q.sf - q.s * F;
    const int na = n_active[sl];
    const int nf = n_frames ? n_frames[sl] : F;
    const int mk = ped_mask ? ped_mask[(size_t)sl * Nmax + q.n] : 1;
    q.on = valid & (q.n < clampi(na, 0, Nmax)) & (f < clampi(nf, 0, F)) & (mk != 0);
    return q;
  };
  Slot cur = slot_at(grp * 64);
  for (int base = grp * 64; base < cnt; base += 64 * kCbGroups) {   // uniform in the wave
    const bool on = cur.on;
    const int sf = cur.sf, s = cur.s, n = cur.n;
    double dx[3], dy[3];
    float px[3] = {0.f, 0.f, 0.f}, py[3] = {0.f, 0.f, 0.f};
    float2 tg[3] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
    if (on) {
      const size_t pb = (size_t)sf * kL2 * Nmax + n;
      const size_t tf = shared_targets ? (size_t)s : (size_t)sf;
      const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf * Nmax + n) * kL;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int t = w + 4 * k;
        px[k] = pred[pb + (size_t)t * Nmax];
        py[k] = pred[pb + (size_t)(kL + t) * Nmax];
        tg[k] = t2[t];
      }
    }
    // the next round's index loads go out behind this round's data
    cur = slot_at(base + 64 * kCbGroups);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dx[k] = on ? (double)tg[k].x - (double)px[k] : 0.0;
      dy[k] = on ? (double)tg[k].y - (double)py[k] : 0.0;
    }
    npairs += __popcll(__ballot(on));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acc[k][0] += dx[k];
      acc[k][1] += dy[k];
      acc[k][2] += dx[k] * dx[k];
      acc[k][3] += dy[k] * dy[k];
      acc[k][4] += dx[k] * dy[k];
      if (has_head) {                                      // uniform
        const double a = dx[k] * cs[k].isx, b = dy[k] * cs[k].isy;
        const double q = (a * a + b * b - 2.0 * cs[k].rho * a * b) * cs[k].ic;
        if (on) {
          acc[k][5] += cs[k].base + 0.5 * q;
          acc[k][6] += q;
        }
        for (int l = 0; l < NL; ++l) {                     // uniform; every lane takes part
          const double r = __hiloint2double(__builtin_amdgcn_readlane(r2hi, l),
                                            __builtin_amdgcn_readlane(r2lo, l));
          const int c = __popcll(__ballot(on && q <= r));
          cl[k] += lane == l ? c : 0;
        }
      }
    }
  }

  // the group's row: a step's values come from the one wave that owns it
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int t = w + 4 * k;
    double v[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) v[i] = wave_sum_d(acc[k][i]);
    if (lane == 0) {
      fin[grp][t * 8] = __double_as_longlong((double)npairs);
#pragma unroll
      for (int i = 0; i < 7; ++i) fin[grp][t * 8 + 1 + i] = __double_as_longlong(v[i]);
    }
    if (lane < NL) fin[grp][kCbStats + t * NL + lane] = (long long)cl[k];
  }
  __syncthreads();
  // the workgroup's row: the groups in a fixed order (thread i alone touches word i)
  const int nv = kCbStats + kL * NL;
  if (tid < nv) {
    long long v;
    if (tid < kCbStats)
      v = __double_as_longlong(
          (__longlong_as_double(fin[0][tid]) + __longlong_as_double(fin[1][tid])) +
          (__longlong_as_double(fin[2][tid]) + __longlong_as_double(fin[3][tid])));
    else
      v = (fin[0][tid] + fin[1][tid]) + (fin[2][tid] + fin[3][tid]);
    if (rows) rows[(size_t)blockIdx.x * nv + tid] = v;
    else fin[0][tid] = v;
  }
  if (!rows) {
    __syncthreads();
    calib_finish(fin[0], NL, tid, kCbThreads, stats, inside, fit);
  }
}

// the W rows added in a fixed order that depends on W alone (so the moments'
// bits do not depend on the head or the levels): value i by two threads,
// thread (i, j) keeps the 16 slices 16 j + u (slice k = rows k, k + 32, ...),
// two rounds' loads in flight together; then the slices in order, then the
// two threads' sums
__global__ void __launch_bounds__(kCbRowsThreads) g2k_head_stats_rows_kernel(
    const long long* __restrict__ rows, int W, int NL, double* __restrict__ stats,
    long long* __restrict__ inside, float* __restrict__ fit) {
  constexpr int P = kCbRowsThreads / 2;                    // 512 >= kCbRowMax
  __shared__ long long part[kCbRowsThreads];
  __shared__ long long fin[kCbRowMax];
  const int tid = threadIdx.x;
  const int nv = kCbStats + kL * NL;
  const int i = tid & (P - 1), j = tid / P;
  if (i < nv) {
    const bool fp = i < kCbStats;                          // doubles, then int64 counts
    long long v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = 0;                 // +0.0 and 0 alike
    for (int r0 = 16 * j; r0 < W; r0 += 32) {
      long long x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)                         // unconditional: all 16 in flight
        x[u] = rows[(size_t)min(r0 + u, W - 1) * nv + i];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        if (r0 + u >= W) x[u] = 0;
        v[u] = fp ? __double_as_longlong(__longlong_as_double(v[u]) + __longlong_as_double(x[u]))
                  : v[u] + x[u];
      }
    }
    long long t = v[0];
#pragma unroll
    for (int u = 1; u < 16; ++u)
      t = fp ? __double_as_longlong(__longlong_as_double(t) + __longlong_as_double(v[u])) : t + v[u];
    part[tid] = t;
  }
  __syncthreads();
  if (tid < nv) {
    if (tid < kCbStats)
      fin[tid] = __double_as_longlong(__longlong_as_double(part[tid]) +
                                      __longlong_as_double(part[P + tid]));
    else
      fin[tid] = part[tid] + part[P + tid];
  }
  __syncthreads();
  calib_finish(fin, NL, tid, kCbRowsThreads, stats, inside, fit);
}

}  // namespace

// one row [96 + 12 NL] of 8-byte words per workgroup; none when one workgroup
// covers the launch
int64_t head_stats_ws_bytes(const g2k_dims* d, int n_levels) {
  const CalibGeom g = calib_geom(*d);
  return g.W > 1 ? (int64_t)g.W * (kCbStats + kL * n_levels) * 8 : 0;
}

int head_stats_launch(const g2k_dims* d, const float* pred, const float* targets,
                      const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                      const float* head, const double* r2, int n_levels, double* stats,
                      int64_t* inside, float* fit, void* workspace, hipStream_t st) {
  const CalibGeom g = calib_geom(*d);
  const int64_t total = (int64_t)d->S * d->F * d->Nmax;
  const int NL = inside ? n_levels : 0;                    // no counts asked for: none made
  long long* rows = g.W > 1 ? static_cast<long long*>(workspace) : nullptr;
  hipLaunchKernelGGL(g2k_head_stats_kernel, dim3((unsigned)g.W), dim3(kCbThreads), 0, st, pred,
                     targets, n_active, n_frames, ped_mask, head, r2, NL, d->S, d->F, d->Nmax, total, g.U,
                     (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0, rows, stats,
                     reinterpret_cast<long long*>(inside), fit);
  int rc = check_launch("g2k_head_stats_kernel");
  if (rc || g.W == 1) return rc;
  hipLaunchKernelGGL(g2k_head_stats_rows_kernel, dim3(1), dim3(kCbRowsThreads), 0, st, rows, g.W, NL,
                     stats, reinterpret_cast<long long*>(inside), fit);
  return check_launch("g2k_head_stats_rows_kernel");
}

}  // namespace g2k
