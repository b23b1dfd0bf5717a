// g2k_mix.hip — the Gaussian-mixture trajectory head: up to 8 full-covariance
// Gaussians over a pair's 24 residuals (include/g2k_mix.h holds the
// definition; the full-covariance head of g2k_fullcov.hip is its one-slot,
// b = 0 special case).  One EM step or, without mix_out, the evaluation of a
// given mixture (g2k_mix_em_f32) and the sampler (g2k_mix_sample_f32); the
// fused best-of-K over its draws (g2k_mix_best_of_k_f32) is the shared kernel
// of g2k_bestk.hip with this head's policy (MixHead, g2k_head_draw.h).  The
// build's: the reference has no probabilistic head, so PARITY UNPINNED;
// tests/mixture_ref.py restates the definition in float64 NumPy.
//
// EM.  The S F Nmax slots are dealt in W contiguous ranges to W workgroups of
// 256 threads exactly as in g2k_fullcov.hip (at least 512 slots each, at most
// 256 workgroups), a thread per slot and 256 slots per round.  Three launches:
//  1. g2k_mix_resp_kernel (W workgroups): W_m = L_m^-1 of every live component
//     formed once per workgroup in double (a column per thread, as the
//     full-covariance stats) and kept in LDS with b_m and the component's
//     constant log(w_m / sum w) - 12 log 2 pi - sum log L_m[i][i]; a thread
//     forms its pair's residuals in double, whitens r - b_m with each live
//     W_m (broadcast reads), takes the max-shifted logsumexp and writes the
//     pair's gamma_m to the workspace ([8][slots] f64; non-pairs and dead
//     slots are never written and never read).  The workgroup's row is
//     {sum l, pairs, hard counts[8]}: lanes by butterfly / ballot, waves
//     (w0 + w1) + (w2 + w3).
//  2. g2k_mix_gram_kernel (W x 8 workgroups; those of a dead slot write a row
//     of zeros and leave): the 28-row staging and 4 x 4-block Gram of the
//     full-covariance stats with the staged rows sqrt(gamma_m) r and the
//     "ones" row sqrt(gamma_m), so the Gram's row 24 is sum gamma r and its
//     corner sum gamma.  The nine slot subsets are added in order.
//  3. g2k_mix_finish_kernel (8 workgroups, one per slot): the W rows added in
//     row order, moments / resp / total, and the M-step with the one-wave
//     24 x 24 Cholesky of the full-covariance fit.
// No atomics, every sum in a fixed order: repeated calls are bit-identical;
// the first two kernels do not look at mix_out, so the E-step's outputs do
// not depend on it.
#include <float.h>

#include "g2k_common.h"
#include "g2k_head_draw.h"
#include "g2k_mix.h"

namespace g2k {
namespace {

static_assert(kMixSlots == G2K_MIX_SLOTS && kMixPitch == G2K_MIX_PITCH, "the header's block");

constexpr int kMxThreads = 256;
constexpr int kMxDim = 28;                     // 24 coordinates, the sqrt(gamma) row, 3 rows of zeros
constexpr int kMxBlocks = 28;                  // 4 x 4 blocks of the 7 x 7 lower triangle
constexpr int kMxSub = 9;                      // slot subsets: 9 * 28 = 252 threads
constexpr int kMxGram = kMxBlocks * 16;        // 448
constexpr int kMxPitch = kMxThreads + 1;       // odd: a round's rows start one 8-byte bank apart
constexpr int kMxStage = kMxDim * kMxPitch;    // 7196
constexpr int kMxRowA = 2 + kMixSlots;         // {sum l, pairs, hard counts[8]}
constexpr int kMxSlots = 512;                  // slots per workgroup, at least
constexpr int kMxMaxWgs = 256;
constexpr int kMxFinThreads = 512;
constexpr double kMxLog2Pi = 1.8378770664093454835606594728112;
static_assert(kMxSub * kMxGram <= kMxStage, "the subsets' parts fit the staging area");
static_assert(kMxGram + kMxRowA <= kMxFinThreads, "a thread per value of the finish");

struct MixGeom { int W; int64_t U; };

MixGeom mix_geom(const g2k_dims& d) {
  const int64_t slots = (int64_t)d.S * d.F * d.Nmax;
  int64_t w = (slots + kMxSlots - 1) / kMxSlots;
  if (w > kMxMaxWgs) w = kMxMaxWgs;
  if (w < 1) w = 1;
  MixGeom g;
  g.W = (int)w;
  g.U = (slots + w - 1) / w;
  return g;
}

__device__ __forceinline__ double mix_wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Gram entry (i, j), i >= j, of a row [448]
__device__ __forceinline__ double mix_gram_at(const double* fin, int i, int j) {
  const int I = i >> 2, J = j >> 2;
  return fin[(I * (I + 1) / 2 + J) * 16 + (i & 3) * 4 + (j & 3)];
}

// what a thread's slot is, and its pair's residuals in double (zeros for a
// slot that is no pair: nothing of it is loaded)
struct MixSlot { bool on; int64_t gslot; };

__device__ __forceinline__ MixSlot mix_residuals(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, int S, int F, int Nmax, int shared_targets, int64_t i0,
    int64_t sf0, int n0, int jslot, bool valid, double (&r)[kL2]) {
  const int Fd = F > 0 ? F : 1;
  const int jj = n0 + (valid ? jslot : 0);
  const int sfl = jj / Nmax;
  const int n = jj - sfl * Nmax;
  const int sf = (int)sf0 + sfl;                           // < S F <= INT32_MAX
  const int s = sf / Fd;
  const int f = sf - s * F;
  const int sl = min(s, S - 1);                            // a lane past the range: in bounds, off
  const int na = n_active[sl];
  const int nf = n_frames ? n_frames[sl] : F;
  const int mk = ped_mask ? ped_mask[(size_t)sl * Nmax + n] : 1;
  MixSlot o;
  o.on = valid & (n < clampi(na, 0, Nmax)) & (f < clampi(nf, 0, F)) & (mk != 0);
  o.gslot = i0 + (valid ? jslot : 0);
  if (o.on) {
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
  return o;
}

// ---------------------------------------------------------------------------
// 1. responsibilities
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kMxThreads) g2k_mix_resp_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ mix, int S, int F, int Nmax,
    int64_t total, int64_t U, int shared_targets, double* __restrict__ gamma,
    double* __restrict__ rowsA) {
  __shared__ double Ls[kL2 * kL2];                         // one component's L in double
  __shared__ double Wm[kMixSlots * kL2 * kL2];             // L_m^-1
  __shared__ double bd[kMixSlots * kL2];
  __shared__ double lc[kMixSlots];
  __shared__ double lm[kMixSlots * kMxThreads];            // a round's l_m, a column per thread
  __shared__ double lpart[4];
  __shared__ int cpart[4][1 + kMixSlots];
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();

  int live = 0;
  double sumw = 0.0;
#pragma unroll
  for (int m = 0; m < kMixSlots; ++m) {
    const float wm = mix[m * kMixPitch];
    if (wm != 0.f) live |= 1 << m;
    sumw += (double)wm;
  }
  live = __builtin_amdgcn_readfirstlane(live);
#pragma nounroll
  for (int m = 0; m < kMixSlots; ++m) {
    if (!((live >> m) & 1)) continue;                      // uniform
    const float* Lg = mix + m * kMixPitch + kMixOffL;
    for (int idx = tid; idx < kL2 * kL2; idx += kMxThreads) {
      const int i = idx / kL2, j = idx - i * kL2;
      double v = 0.0;
      if (j <= i) v = (double)Lg[idx];
      Ls[idx] = v;
    }
    __syncthreads();
    if (tid < kL2) {
      // column tid of L^-1 by forward substitution, in registers
      double wc[kL2];
#pragma unroll
      for (int i = 0; i < kL2; ++i) {
        double acc = i == tid ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) acc = fma(-Ls[i * kL2 + k], wc[k], acc);
        wc[i] = acc / Ls[i * kL2 + i];
      }
#pragma unroll
      for (int i = 0; i < kL2; ++i) Wm[m * kL2 * kL2 + i * kL2 + tid] = wc[i];
    } else if (tid == 64) {
      double c = log((double)mix[m * kMixPitch] / sumw) - 12.0 * kMxLog2Pi;
      for (int i = 0; i < kL2; ++i) c -= log(Ls[i * kL2 + i]);
      lc[m] = c;
    } else if (tid >= 128 && tid < 128 + kL2) {
      bd[m * kL2 + tid - 128] = (double)mix[m * kMixPitch + kMixOffB + tid - 128];
    }
    __syncthreads();
  }

  double lsum = 0.0;
  int pairs = 0;
  int hc[kMixSlots];
#pragma unroll
  for (int m = 0; m < kMixSlots; ++m) hc[m] = 0;

  const int64_t i0 = (int64_t)blockIdx.x * U;
  const int64_t left = total - i0;
  const int cnt = (int)(left < 0 ? 0 : (left < U ? left : U));
  const int64_t sf0 = i0 / Nmax;
  const int n0 = (int)(i0 - sf0 * Nmax);

  for (int base = 0; base < cnt; base += kMxThreads) {     // uniform trip count
    const int jslot = base + tid;
    const bool valid = jslot < cnt;
    double r[kL2];
    const MixSlot sl = mix_residuals(pred, targets, n_active, n_frames, ped_mask, S, F, Nmax,
                                     shared_targets, i0, sf0, n0, jslot, valid, r);
    double lmax = -DBL_MAX;
#pragma nounroll
    for (int m = 0; m < kMixSlots; ++m) {
      if (!((live >> m) & 1)) continue;                    // uniform
      const double* Wc = Wm + m * kL2 * kL2;
      const double* bc = bd + m * kL2;
      double dv[kL2];
#pragma unroll
      for (int i = 0; i < kL2; ++i) dv[i] = r[i] - bc[i];
      double q = 0.0;
#pragma unroll
      for (int i = 0; i < kL2; ++i) {
        double z = 0.0;
#pragma unroll
        for (int k = 0; k <= i; ++k) z = fma(Wc[i * kL2 + k], dv[k], z);
        q = fma(z, z, q);
      }
      const double l = lc[m] - 0.5 * q;
      lm[m * kMxThreads + tid] = l;                        // this thread's column: no barrier
      lmax = fmax(lmax, l);
    }
    double se = 0.0;
#pragma nounroll
    for (int m = 0; m < kMixSlots; ++m)
      if ((live >> m) & 1) se += exp(lm[m * kMxThreads + tid] - lmax);
    const double l = lmax + log(se);
    double gbest = -1.0;
    int hm = 0;
#pragma nounroll
    for (int m = 0; m < kMixSlots; ++m) {
      if (!((live >> m) & 1)) continue;
      const double g = exp(lm[m * kMxThreads + tid] - l);
      if (g > gbest) { gbest = g; hm = m; }                // strict: the lowest m stays
      if (sl.on) gamma[(size_t)m * total + sl.gslot] = g;
    }
    if (sl.on) { lsum += l; pairs += 1; }
#pragma unroll
    for (int m = 0; m < kMixSlots; ++m) {                  // every lane takes part
      const int c = __popcll(__ballot(sl.on && hm == m));
      hc[m] += lane == 0 ? c : 0;
    }
  }

  const double lw = mix_wave_sum_d(lsum);
  const int pw = wave_sum_i(pairs);
  if (lane == 0) {
    lpart[w] = lw;
    cpart[w][0] = pw;
#pragma unroll
    for (int m = 0; m < kMixSlots; ++m) cpart[w][1 + m] = hc[m];
  }
  __syncthreads();
  if (tid < kMxRowA) {
    double v;
    if (tid == 0) {
      v = (lpart[0] + lpart[1]) + (lpart[2] + lpart[3]);
    } else {
      const int k = tid - 1;
      v = (double)((cpart[0][k] + cpart[1][k]) + (cpart[2][k] + cpart[3][k]));
    }
    rowsA[(size_t)blockIdx.x * kMxRowA + tid] = v;
  }
}

// ---------------------------------------------------------------------------
// 2. the weighted Gram of one (workgroup range, component)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kMxThreads) g2k_mix_gram_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ mix, int S, int F, int Nmax,
    int64_t total, int64_t U, int shared_targets, const double* __restrict__ gamma,
    double* __restrict__ rowsB) {
  __shared__ double rsT[kMxStage];                         // [28][257]: row i, slot p
  const int tid = threadIdx.x;
  const int m = blockIdx.y;
  double* row = rowsB + ((size_t)blockIdx.x * kMixSlots + m) * kMxGram;
  if (mix[m * kMixPitch] == 0.f) {                         // a dead slot (uniform)
    for (int i = tid; i < kMxGram; i += kMxThreads) row[i] = 0.0;
    return;
  }
  for (int idx = tid; idx < (kMxDim - kL2 - 1) * kMxPitch; idx += kMxThreads)
    rsT[(kL2 + 1) * kMxPitch + idx] = 0.0;                 // the rows of zeros, once

  // the Gram block of this thread: b = I (I + 1) / 2 + J, I >= J
  const int gsub = tid / kMxBlocks, gb = tid - gsub * kMxBlocks;
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
  __syncthreads();

  for (int base = 0; base < cnt; base += kMxThreads) {     // uniform trip count
    const int jslot = base + tid;
    const bool valid = jslot < cnt;
    double r[kL2];
    const MixSlot sl = mix_residuals(pred, targets, n_active, n_frames, ped_mask, S, F, Nmax,
                                     shared_targets, i0, sf0, n0, jslot, valid, r);
    double sg = 0.0;
    if (sl.on) sg = sqrt(gamma[(size_t)m * total + sl.gslot]);
#pragma unroll
    for (int i = 0; i < kL2; ++i) rsT[i * kMxPitch + tid] = sg * r[i];
    rsT[kL2 * kMxPitch + tid] = sg;
    __syncthreads();
    if (tid < kMxSub * kMxBlocks) {
      for (int p = gsub; p < kMxThreads; p += kMxSub) {
        double x[4], y[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          x[a] = rsT[(4 * gI + a) * kMxPitch + p];
          y[a] = rsT[(4 * gJ + a) * kMxPitch + p];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) g[a][c] = fma(x[a], y[c], g[a][c]);
      }
    }
    __syncthreads();
  }

  double* part = rsT;                                      // [9][448]
  if (tid < kMxSub * kMxBlocks) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) part[gsub * kMxGram + gb * 16 + a * 4 + c] = g[a][c];
  }
  __syncthreads();
  for (int i = tid; i < kMxGram; i += kMxThreads) {
    double sacc = part[i];
#pragma unroll
    for (int k = 1; k < kMxSub; ++k) sacc += part[k * kMxGram + i];
    row[i] = sacc;
  }
}

// ---------------------------------------------------------------------------
// 3. the rows added in row order, the outputs and the M-step of slot blockIdx.x
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kMxFinThreads) g2k_mix_finish_kernel(
    const double* __restrict__ rowsA, const double* __restrict__ rowsB, int W,
    const float* __restrict__ mix_in, double* __restrict__ moments, double* __restrict__ resp,
    double* __restrict__ total, float* __restrict__ mix_out) {
  __shared__ double fin[kMxGram];
  __shared__ double tot[kMxRowA];
  __shared__ double A[kL2 * kL2];
  __shared__ double bn[kL2];
  const int tid = threadIdx.x;
  const int m = blockIdx.x;
  if (tid < kMxGram) {
    double v = 0.0;
    for (int w = 0; w < W; ++w) v += rowsB[((size_t)w * kMixSlots + m) * kMxGram + tid];
    fin[tid] = v;
  } else if (tid < kMxGram + kMxRowA) {
    const int k = tid - kMxGram;
    double v = 0.0;
    for (int w = 0; w < W; ++w) v += rowsA[(size_t)w * kMxRowA + k];
    tot[k] = v;
  }
  __syncthreads();
  const float* in = mix_in + m * kMixPitch;
  const float w_in = in[0];
  const bool live = w_in != 0.f;                           // uniform
  const double n = tot[1];
  const double N = live ? mix_gram_at(fin, kL2, kL2) : 0.0;
  double* mo = moments + (size_t)m * (kL2 + 1) * kL2;
  for (int idx = tid; idx < (kL2 + 1) * kL2; idx += kMxFinThreads) {
    const int i = idx / kL2, j = idx - i * kL2;
    mo[idx] = live ? (i >= j ? mix_gram_at(fin, i, j) : mix_gram_at(fin, j, i)) : 0.0;
  }
  if (tid == 0) {
    resp[m * 2] = N;
    resp[m * 2 + 1] = tot[2 + m];
  }
  if (m == 0 && tid < 4) total[tid] = tid == 0 ? n : (tid == 1 ? tot[0] : 0.0);
  if (!mix_out) return;                                    // uniform: the E-step only
  float* out = mix_out + m * kMixPitch;
  if (!live) {
    for (int i = tid; i < kMixPitch; i += kMxFinThreads) out[i] = 0.f;
    return;
  }
  const bool update = n > 0.0 && N >= 1.0;                 // uniform
  if (tid < kMixOffB) out[tid] = tid == 0 ? (n > 0.0 ? (float)(N / n) : w_in) : 0.f;
  if (!update) {
    // too little mass (or no pair): the component stays where it is
    for (int i = tid; i < kL2; i += kMxFinThreads) out[kMixOffB + i] = in[kMixOffB + i];
    for (int idx = tid; idx < kL2 * kL2; idx += kMxFinThreads) {
      const int i = idx / kL2, j = idx - i * kL2;
      float v = 0.f;
      if (j <= i) v = in[kMixOffL + idx];
      out[kMixOffL + idx] = v;
    }
    return;
  }
  if (tid < kL2) {
    const double b = mix_gram_at(fin, kL2, tid) / N;
    bn[tid] = b;
    out[kMixOffB + tid] = (float)b;
  }
  __syncthreads();
  for (int idx = tid; idx < kL2 * kL2; idx += kMxFinThreads) {
    const int i = idx / kL2, j = idx - i * kL2;
    double v = 0.0;
    if (j <= i) v = mix_gram_at(fin, i, j) / N - bn[i] * bn[j];
    if (j == i) v = v * (1.0 + 1e-6) + 1e-12;
    A[idx] = v;
  }
  __syncthreads();
  // the one-wave Cholesky of the full-covariance fit: right-looking, lane i
  // keeps row i in registers, column j's entries travel by lane shuffles
  if (tid < 64) {
    const int rowi = tid < kL2 ? tid : kL2 - 1;
    double a[kL2];
#pragma unroll
    for (int k = 0; k < kL2; ++k) a[k] = A[rowi * kL2 + k];
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
      for (int k = 0; k < kL2; ++k) out[kMixOffL + tid * kL2 + k] = k <= tid ? (float)a[k] : 0.f;
    }
  }
}

// ---------------------------------------------------------------------------
// the sampler: one thread per (s, f, n), the draw of MixHead (so that the fused
// best-of-K's draw is, bit for bit, this one)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) g2k_mix_sample_kernel(
    const float* __restrict__ pred, const float* __restrict__ mix, int64_t slots, int Nmax,
    uint32_t seed_lo, uint32_t seed_hi, float* __restrict__ out, int32_t* __restrict__ comp) {
  __shared__ MixHead::Lds hlds;
  MixHead::stage<256>(mix, hlds, threadIdx.x);
  __syncthreads();
  MixHead head;
  head.bind(hlds);
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= slots) return;
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
  if (comp) comp[id] = head.select(seed_lo, seed_hi, e0);
  head.draw(seed_lo, seed_hi, e0, n, Nmax, mu, [&](int t, float x, float y) {
    out[pb + (size_t)t * Nmax] = x;
    out[pb + (size_t)(kL + t) * Nmax] = y;
  });
}

}  // namespace

// gamma [8][slots], then a row [10] and 8 rows [448] per workgroup, 8-byte words
int64_t mix_em_ws_bytes(const g2k_dims* d) {
  const MixGeom g = mix_geom(*d);
  const int64_t slots = (int64_t)d->S * d->F * d->Nmax;
  return 8 * ((int64_t)kMixSlots * slots + (int64_t)g.W * (kMxRowA + kMixSlots * kMxGram));
}

int mix_em_launch(const g2k_dims* d, const float* pred, const float* targets,
                  const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                  const float* mix_in, double* moments, double* resp, double* total, float* mix_out,
                  void* workspace, hipStream_t st) {
  const MixGeom g = mix_geom(*d);
  const int64_t slots = (int64_t)d->S * d->F * d->Nmax;
  double* gamma = static_cast<double*>(workspace);
  double* rowsA = gamma + (size_t)kMixSlots * slots;
  double* rowsB = rowsA + (size_t)g.W * kMxRowA;
  const int shared = (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0;
  hipLaunchKernelGGL(g2k_mix_resp_kernel, dim3((unsigned)g.W), dim3(kMxThreads), 0, st, pred, targets,
                     n_active, n_frames, ped_mask, mix_in, d->S, d->F, d->Nmax, slots, g.U, shared,
                     gamma, rowsA);
  int rc = check_launch("g2k_mix_resp_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(g2k_mix_gram_kernel, dim3((unsigned)g.W, kMixSlots), dim3(kMxThreads), 0, st,
                     pred, targets, n_active, n_frames, ped_mask, mix_in, d->S, d->F, d->Nmax, slots,
                     g.U, shared, gamma, rowsB);
  if ((rc = check_launch("g2k_mix_gram_kernel"))) return rc;
  hipLaunchKernelGGL(g2k_mix_finish_kernel, dim3(kMixSlots), dim3(kMxFinThreads), 0, st, rowsA, rowsB,
                     g.W, mix_in, moments, resp, total, mix_out);
  return check_launch("g2k_mix_finish_kernel");
}

int mix_sample_launch(const g2k_dims* d, const float* pred, const float* mix, uint64_t seed,
                      float* out, int32_t* comp, hipStream_t st) {
  const int64_t slots = (int64_t)d->S * d->F * d->Nmax;
  const int64_t wgs = (slots + 255) / 256;
  if (wgs > 0x7fffffff) return set_err(G2K_EINVAL, "mix_sample: %lld workgroups", (long long)wgs);
  hipLaunchKernelGGL(g2k_mix_sample_kernel, dim3((unsigned)wgs), dim3(256), 0, st, pred, mix, slots,
                     d->Nmax, (uint32_t)seed, (uint32_t)(seed >> 32), out, comp);
  return check_launch("g2k_mix_sample_kernel");
}

}  // namespace g2k
