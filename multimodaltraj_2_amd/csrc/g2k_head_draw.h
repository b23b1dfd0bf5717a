// g2k_head_draw.h — the probabilistic heads as device-side policies: what the
// fused evaluations (best_of_k_kernel, g2k_bestk.hip; joint_kernel and
// joint_wave_kernel, g2k_joint.hip; kde_nll_kernel, g2k_kde.hip) take as their
// template parameter.  A policy owns exactly what differs between the heads:
//   Lds                       what it keeps in LDS for the workgroup
//   stage<NT>(p, lds, tid)    fills it from the head's parameters, NT threads
//                             taking part, a compile-time constant (the
//                             caller's barrier follows)
//   bind(lds)                 what a lane then draws from
//   draw(lo, hi, e0, n, Nmax, mu, step)
//                             one draw of one member for seed (hi, lo), whose
//                             step-0 element is e0, whose column is n (e0 - n
//                             is the scene-frame's column-0 element: only the
//                             coupled head looks at it) and whose means are mu
//                             (time-major, mu[2t + c]); calls step(t, x, y) as
//                             soon as step t's two coordinates are final
//   kPrefix                   the head's prefix in a launcher's messages
//   kJointWaveOccupancy       joint_wave_kernel's amdgpu_waves_per_eu (1: no
//                             hint, the compiler's default)
//   kKdeRunningMean           kde_nll_kernel's moments (g2k_kde.hip): false =
//                             plain sums of d = x - mu (the draws sit around
//                             the means), true = a running mean and centred
//                             sums (the draws sit around mu + b_m, |b_m| far
//                             above the spread)
// Each draw is the code of its head's sampler (gauss_draw, g2k_common.h, and
// g2k_gauss_sample_kernel; fullcov_advance below and g2k_fullcov_sample_kernel),
// so that a draw made inside a fused evaluation is, bit for bit, the sampler's.
#pragma once
#include "g2k_common.h"

namespace g2k {
namespace {

// ---------------------------------------------------------------------------
// the per-step bivariate-Gaussian head (g2k_nll.hip): head [3, 12]
// ---------------------------------------------------------------------------
struct PerStepHead {
  static constexpr const char* kPrefix = "";
  static constexpr int kJointWaveOccupancy = 1;
  static constexpr bool kKdeRunningMean = false;
  struct Lds { float4 hs[kL]; };       // per step {sigma_x, sigma_y, rho, sqrt(1 - rho^2)}
  GaussStep gs[kL];                    // wave-uniform: scalar registers

  template <int NT>
  static __device__ __forceinline__ void stage(const float* __restrict__ head, Lds& lds, int tid) {
    for (int t = tid; t < kL; t += NT) {
      const GaussStep g = gauss_step(head, t);
      lds.hs[t] = make_float4(g.sx, g.sy, g.rho, g.sq);
    }
  }
  __device__ __forceinline__ void bind(const Lds& lds) {
#pragma unroll
    for (int t = 0; t < kL; ++t) {
      const float4 v = lds.hs[t];
      gs[t].sx = sgpr_f(v.x); gs[t].sy = sgpr_f(v.y); gs[t].rho = sgpr_f(v.z); gs[t].sq = sgpr_f(v.w);
    }
  }
  template <class Step>
  __device__ __forceinline__ void draw(uint32_t lo, uint32_t hi, int64_t e0, int /*n*/, int Nmax,
                                       const float (&mu)[kL2], Step&& step) const {
    const uint32_t ehi0 = (uint32_t)(e0 >> 32);
    const uint32_t stream0 = gauss_stream(lo, hi, ehi0);
#pragma unroll
    for (int t = 0; t < kL; ++t) {
      const int64_t e = e0 + (int64_t)t * Nmax;
      const uint32_t ehi = (uint32_t)(e >> 32);
      uint32_t stream = stream0;
      if (ehi != ehi0) stream = gauss_stream(lo, hi, ehi);   // a member that straddles 2^32
      float x, y;
      gauss_draw(stream, (uint32_t)e, gs[t], mu[2 * t], mu[2 * t + 1], x, y);
      step(t, x, y);
    }
  }
};

// ---------------------------------------------------------------------------
// the full-covariance trajectory head (g2k_fullcov.hip holds the definition):
// chol [24][24], the lower Cholesky factor over the coordinates i = 2t + c
// ---------------------------------------------------------------------------
// Lt (LDS) = the factor transposed: Lt[j * 24 + i] = L[i][j], j <= i (entries
// above the diagonal are not read from memory)
__device__ __forceinline__ void fullcov_load_lt(const float* __restrict__ chol, float* Lt, int tid,
                                                int nthreads) {
  for (int idx = tid; idx < kL2 * kL2; idx += nthreads) {
    const int i = idx / kL2, j = idx - i * kL2;
    float v = 0.f;
    if (j <= i) v = chol[idx];
    Lt[j * kL2 + i] = v;
  }
}

// step t of a draw: column 2t's terms into the rows >= 2t, then column 2t+1's
// into the rows >= 2t+1; a[2t], a[2t+1] are final afterwards (t a constant
// after unrolling: every index is one)
__device__ __forceinline__ void fullcov_advance(const float* Lt, int t, float z0, float z1,
                                                float (&a)[kL2]) {
  // a step's columns are read when the step is reached: the compiler may not
  // gather the 300 reads of a draw ahead of the draw loop
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < kL2; ++i)
    if (i >= 2 * t) a[i] = fmaf(Lt[(2 * t) * kL2 + i], z0, a[i]);
#pragma unroll
  for (int i = 0; i < kL2; ++i)
    if (i >= 2 * t + 1) a[i] = fmaf(Lt[(2 * t + 1) * kL2 + i], z1, a[i]);
}

// The draw: row i of the product takes column j's term in ascending j, so a
// sweep over the columns in order gives every row the defined order; the 24
// running sums start as the means, and after step t's two normals have been
// added into the rows >= 2t, a[2t] and a[2t+1] are final.  The factor (300
// wave-uniform floats) is read from LDS again for every draw by broadcast
// reads.  The step loop is unrolled, no per-thread array is indexed at run
// time: no scratch.
struct FullCovHead {
  static constexpr const char* kPrefix = "fullcov_";
  static constexpr int kJointWaveOccupancy = 2;
  static constexpr bool kKdeRunningMean = false;
  struct alignas(16) Lds { float Lt[kL2 * kL2]; };
  const float* Lt;

  template <int NT>
  static __device__ __forceinline__ void stage(const float* __restrict__ chol, Lds& lds, int tid) {
    fullcov_load_lt(chol, lds.Lt, tid, NT);
  }
  __device__ __forceinline__ void bind(const Lds& lds) { Lt = lds.Lt; }
  template <class Step>
  __device__ __forceinline__ void draw(uint32_t lo, uint32_t hi, int64_t e0, int /*n*/, int Nmax,
                                       const float (&mu)[kL2], Step&& step) const {
    const uint32_t ehi0 = (uint32_t)(e0 >> 32);
    const uint32_t stream0 = gauss_stream(lo, hi, ehi0);
    float a[kL2];
#pragma unroll
    for (int r = 0; r < kL2; ++r) a[r] = mu[r];
    // step 0's element index, opaque to the compiler: the 12 indices (and the
    // 12 straddle tests) that it otherwise forms ahead of the draw loop and
    // keeps across it cost registers (the indices are 32-bit here: t Nmax <
    // 2^32, so the high word moves at most once, by a carry)
    uint32_t elo0 = (uint32_t)e0;
    asm volatile("" : "+v"(elo0));
#pragma unroll
    for (int t = 0; t < kL; ++t) {
      const uint32_t elo = elo0 + (uint32_t)(t * Nmax);
      uint32_t stream = stream0;
      if (elo < elo0) stream = gauss_stream(lo, hi, ehi0 + 1u);   // a member that straddles 2^32
      float z0, z1;
      gauss_normals(stream, elo, z0, z1);
      fullcov_advance(Lt, t, z0, z1, a);
      // the step's sums are formed in the step: without this the compiler sinks
      // the later rows' FMAs past the following steps' (branching) sin / cos to
      // where the rows are used, and keeps the 300 values read from Lt (which
      // cannot move) in registers until then — 256 VGPRs + 219 AGPRs in the
      // joint kernels
#pragma unroll
      for (int i = 2 * t + 2; i < kL2; ++i) asm volatile("" : "+v"(a[i]));
      step(t, a[2 * t], a[2 * t + 1]);
    }
  }
};

// ---------------------------------------------------------------------------
// the Gaussian-mixture trajectory head (include/g2k_mix.h holds the
// definition): mix [8][608] = per slot {w, 7 unused, b[24], L[24][24]}; a slot
// with w == 0 is dead (nothing but its w is read)
// ---------------------------------------------------------------------------
constexpr int kMixSlots = 8;
constexpr int kMixPitch = 608;                 // floats per slot of the parameter block
constexpr int kMixOffB = 8, kMixOffL = 32;
// A component's transposed factor in LDS.  The lanes of a wave hold different
// components, so a column read is no longer one broadcast: with a pitch of 576
// floats (0 mod the 64 banks) every component's column would start on the same
// bank and the read would conflict as many ways as there are components in the
// wave; 580 moves each component by one ds_read_b128 (4 banks), so the eight
// components' columns start on banks 0, 4, ..., 28.
constexpr int kMixLtPitch = kL2 * kL2 + 4;     // 580
constexpr uint32_t kMixSelSalt = 0x9E3779B9u;

// The draw is FullCovHead's with a per-lane factor: the component is selected
// once per trajectory from step 0's key (hashed twice: 2 key + 1 and 2 key + 2
// between them cover every 32-bit value, so one hash of any function of the
// key would be some other element's Box-Muller input), the running sums start
// as mu + b_m, and the steps are fullcov_advance on L_m.
struct MixHead {
  static constexpr const char* kPrefix = "mix_";
  static constexpr int kJointWaveOccupancy = 2;
  static constexpr bool kKdeRunningMean = true;
  struct alignas(16) Lds {
    float Lt[kMixSlots * kMixLtPitch];
    float b[kMixSlots * kL2];
    float cw[kMixSlots];
    int live;                                  // bit m: slot m is live
    int last;                                  // the last live slot
  };
  const Lds* lds;

  template <int NT>
  static __device__ __forceinline__ void stage(const float* __restrict__ mix, Lds& l, int tid) {
    // a thread takes at most kTrips entries of a factor, in registers: NT is a
    // constant so that the trips past a factor's end fold away
    static_assert(NT >= 64 && NT % 64 == 0, "MixHead::stage: whole waves, at least one");
    // every thread forms the live mask (uniform); thread 0 the cumulative weights
    float w[kMixSlots];
    int live = 0, last = 0;
#pragma unroll
    for (int m = 0; m < kMixSlots; ++m) {
      w[m] = mix[m * kMixPitch];
      if (w[m] != 0.f) { live |= 1 << m; last = m; }
    }
    if (tid == 0) {
      double sum = 0.0;
#pragma unroll
      for (int m = 0; m < kMixSlots; ++m) sum += (double)w[m];
      double c = 0.0;
#pragma unroll
      for (int m = 0; m < kMixSlots; ++m) {
        c += (double)w[m] / sum;
        l.cw[m] = m == last ? 1.f : (float)c;
      }
      l.live = live;
      l.last = last;
    }
    // The live slots' factors, a slot's 576 entries strided over the threads
    // (NT >= 64: at most kTrips each).  Every load of every live slot
    // is issued before the first store (the slot test is uniform), so a
    // one-wave workgroup pays one round trip to memory and not one per trip:
    // joint_wave_kernel's units are short, their staging is a large part of
    // them.
    constexpr int kTrips = (kL2 * kL2 + 63) / 64;          // 9
    float v[kMixSlots][kTrips];
#pragma unroll
    for (int m = 0; m < kMixSlots; ++m) {
      if (!((live >> m) & 1)) continue;
#pragma unroll
      for (int q = 0; q < kTrips; ++q) {
        const int r = q * NT + tid;
        const int i = r / kL2, j = r - i * kL2;
        v[m][q] = 0.f;
        if (r < kL2 * kL2 && j <= i) v[m][q] = mix[m * kMixPitch + kMixOffL + r];
      }
    }
#pragma unroll
    for (int m = 0; m < kMixSlots; ++m) {
      if (!((live >> m) & 1)) continue;
#pragma unroll
      for (int q = 0; q < kTrips; ++q) {
        const int r = q * NT + tid;
        const int i = r / kL2, j = r - i * kL2;
        if (r < kL2 * kL2) l.Lt[m * kMixLtPitch + j * kL2 + i] = v[m][q];
      }
    }
    for (int idx = tid; idx < kMixSlots * kL2; idx += NT) {
      const int m = idx / kL2;
      if ((live >> m) & 1) l.b[idx] = mix[m * kMixPitch + kMixOffB + (idx - m * kL2)];
    }
  }
  __device__ __forceinline__ void bind(const Lds& l) { lds = &l; }
  // the component of the trajectory whose step-0 element is e0
  __device__ __forceinline__ int select(uint32_t lo, uint32_t hi, int64_t e0) const {
    const uint32_t key0 = gauss_stream(lo, hi, (uint32_t)(e0 >> 32)) ^ (uint32_t)e0;
    const uint32_t h = pcg_hash(pcg_hash(key0) + kMixSelSalt);
    const float u = ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const int live = lds->live;
    int m = lds->last;
#pragma unroll
    for (int k = kMixSlots - 1; k >= 0; --k)
      if (((live >> k) & 1) && u < lds->cw[k]) m = k;
    return m;
  }
  template <class Step>
  __device__ __forceinline__ void draw(uint32_t lo, uint32_t hi, int64_t e0, int /*n*/, int Nmax,
                                       const float (&mu)[kL2], Step&& step) const {
    const uint32_t ehi0 = (uint32_t)(e0 >> 32);
    const uint32_t stream0 = gauss_stream(lo, hi, ehi0);
    const int m = select(lo, hi, e0);
    const float* Lt = lds->Lt + m * kMixLtPitch;           // per lane
    const float* bm = lds->b + m * kL2;
    float a[kL2];
#pragma unroll
    for (int r = 0; r < kL2; ++r) a[r] = mu[r] + bm[r];
    // the pins of FullCovHead::draw: step 0's element index opaque, each
    // step's later sums formed in the step
    uint32_t elo0 = (uint32_t)e0;
    asm volatile("" : "+v"(elo0));
#pragma unroll
    for (int t = 0; t < kL; ++t) {
      const uint32_t elo = elo0 + (uint32_t)(t * Nmax);
      uint32_t stream = stream0;
      if (elo < elo0) stream = gauss_stream(lo, hi, ehi0 + 1u);   // a member that straddles 2^32
      float z0, z1;
      gauss_normals(stream, elo, z0, z1);
      fullcov_advance(Lt, t, z0, z1, a);
#pragma unroll
      for (int i = 2 * t + 2; i < kL2; ++i) asm volatile("" : "+v"(a[i]));
      step(t, a[2 * t], a[2 * t + 1]);
    }
  }
};

// ---------------------------------------------------------------------------
// the scene-coupled head (include/g2k_coupled.h holds the definition): cpl
// [2][24][24] = {Lw, Lb}, the lower Cholesky factors of the covariance W of a
// member's own part and B of the part that the members of a scene-frame share
// ---------------------------------------------------------------------------
// G2K_COUPLED_SALT (include/g2k_coupled.h; g2k_coupled.hip asserts the two
// equal): the scene-frame's normals are drawn under seed XOR this
constexpr uint32_t kCoupledSaltLo = 0x7F4A6000u, kCoupledSaltHi = 0x9E3779B9u;

// The draw is FullCovHead's twice over: first the shared part c = Lb zc from
// zeros, zc the normals of the scene-frame's column-0 element under the salted
// seed (every member of the scene-frame forms the same c, bit for bit: 300
// FMAs and 12 Box-Muller pairs a lane repeats, no exchange between lanes and
// no barrier, so the policy fits every kernel that takes one); then the
// running sums start as mu + c (one add) and the member's own steps are
// fullcov_advance on Lw.  The first loop leaves only the 24 sums live, which
// the second then carries: the registers of FullCovHead::draw, not twice them.
struct CoupledHead {
  static constexpr const char* kPrefix = "coupled_";
  static constexpr int kJointWaveOccupancy = 2;
  static constexpr bool kKdeRunningMean = false;
  struct alignas(16) Lds { float Ltw[kL2 * kL2]; float Ltb[kL2 * kL2]; };
  const float* Ltw;
  const float* Ltb;

  template <int NT>
  static __device__ __forceinline__ void stage(const float* __restrict__ cpl, Lds& lds, int tid) {
    fullcov_load_lt(cpl, lds.Ltw, tid, NT);
    fullcov_load_lt(cpl + kL2 * kL2, lds.Ltb, tid, NT);
  }
  __device__ __forceinline__ void bind(const Lds& lds) { Ltw = lds.Ltw; Ltb = lds.Ltb; }
  // 12 steps of fullcov_advance on Lt into a, the normals those of the element
  // e0 + t Nmax under seed (hi, lo); FullCovHead::draw's pins
  template <class Step>
  static __device__ __forceinline__ void sweep(const float* Lt, uint32_t lo, uint32_t hi, int64_t e0,
                                               int Nmax, float (&a)[kL2], Step&& step) {
    const uint32_t ehi0 = (uint32_t)(e0 >> 32);
    const uint32_t stream0 = gauss_stream(lo, hi, ehi0);
    uint32_t elo0 = (uint32_t)e0;
    asm volatile("" : "+v"(elo0));
#pragma unroll
    for (int t = 0; t < kL; ++t) {
      const uint32_t elo = elo0 + (uint32_t)(t * Nmax);
      uint32_t stream = stream0;
      if (elo < elo0) stream = gauss_stream(lo, hi, ehi0 + 1u);   // an element that straddles 2^32
      float z0, z1;
      gauss_normals(stream, elo, z0, z1);
      fullcov_advance(Lt, t, z0, z1, a);
#pragma unroll
      for (int i = 2 * t + 2; i < kL2; ++i) asm volatile("" : "+v"(a[i]));
      step(t, a[2 * t], a[2 * t + 1]);
    }
  }
  template <class Step>
  __device__ __forceinline__ void draw(uint32_t lo, uint32_t hi, int64_t e0, int n, int Nmax,
                                       const float (&mu)[kL2], Step&& step) const {
    float a[kL2];
#pragma unroll
    for (int r = 0; r < kL2; ++r) a[r] = 0.f;
    sweep(Ltb, lo ^ kCoupledSaltLo, hi ^ kCoupledSaltHi, e0 - n, Nmax, a, [](int, float, float) {});
#pragma unroll
    for (int r = 0; r < kL2; ++r) a[r] = mu[r] + a[r];
    sweep(Ltw, lo, hi, e0, Nmax, a, step);
  }
};

// A pair's (a member's) 24 means and 24 target coordinates, both time-major
// ([2t + c]: the indices are constants after unrolling, so the order is one
// of names only); zeros for a lane that is off.
__device__ __forceinline__ void load_mu_tg(bool on, const float* __restrict__ pred,
                                           const float* __restrict__ targets, size_t sf, size_t tf,
                                           int n, int Nmax, float (&mu)[kL2], float (&tg)[kL2]) {
  if (on) {
    const size_t pb = sf * kL2 * Nmax + n;
    const float2* t2 = reinterpret_cast<const float2*>(targets) + (tf * Nmax + n) * kL;
#pragma unroll
    for (int t = 0; t < kL; ++t) {
      mu[2 * t] = pred[pb + (size_t)t * Nmax];
      mu[2 * t + 1] = pred[pb + (size_t)(kL + t) * Nmax];
      const float2 v = t2[t];
      tg[2 * t] = v.x; tg[2 * t + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int r = 0; r < kL2; ++r) { mu[r] = 0.f; tg[r] = 0.f; }
  }
}

}  // namespace
}  // namespace g2k
