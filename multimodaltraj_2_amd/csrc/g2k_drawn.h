// g2k_drawn.h — what the DRAWN-ONCE sampled evaluations have in common
// (sample_scores_kernel, g2k_scores.hip; sample_modes_kernel, g2k_modes.hip;
// sample_ranks_kernel, g2k_ranks.hip; sample_kin_kernel, g2k_kin.hip).  Unlike
// best-of-K and the KDE-NLL (g2k_bestk_geom.h) the K draws of a pair must all
// be live at once, so a draw is made ONCE and parked in LDS:
//   one workgroup of 256 threads per (scene, chunk of FC frames); a pass takes
//   G = min(256 / K, cap) pairs; lane tid owns (pair tid / K, draw tid % K) and
//   LDS slot tid, 24 floats (96 B: ds_read_b128 aligned); FC is sized for 4
//   passes; draw k is the head's sampler at seed (seed + k) mod 2^64
// Here, once each: the constants, the geometry, the device scaffold of a pass
// (the chunk, the lane, the pass's item, the slot store, the zeros of per_ped),
// the two row reductions that add a scene's C chunk rows in chunk order, and
// the launchers' tail.  A kernel keeps its own stages, its own LDS and its own
// validator ("the drawn-once family").
#pragma once
#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_head_draw.h"
#include "g2k_kin.h"
#include "g2k_modes.h"
#include "g2k_ranks.h"
#include "g2k_scores.h"

namespace g2k {
namespace {

constexpr int kDrThreads = 256;
constexpr int kDrMaxG = 32;                   // pairs per pass: the LDS budget, a finishing lane each
constexpr int kDrPasses = 4;                  // passes that a workgroup's frames are sized for
constexpr int kDrPitch = kL2;                 // floats per draw in LDS (96 B: ds_read_b128 aligned)

struct DrawnGeom { int G, FC, C; };

// maxG: a kernel's own cap on the pairs of a pass, at most kDrMaxG
inline DrawnGeom drawn_geom(const g2k_dims& d, int K, int maxG = kDrMaxG) {
  DrawnGeom g;
  g.G = kDrThreads / K;
  if (g.G > maxG) g.G = maxG;
  int fc = (kDrPasses * g.G) / d.Nmax;
  if (fc > d.F) fc = d.F;
  if (fc < 1) fc = 1;
  g.FC = fc;
  g.C = d.F > 0 ? (d.F + fc - 1) / fc : 1;
  return g;
}

// ---------------------------------------------------------------------------
// device scaffold
// ---------------------------------------------------------------------------
// A workgroup's (scene, chunk): its pairs are (fl, n), fl < nfc, n < nact, in
// that order, less the masked ones.
//
// How the scaffold is written is pinned by the kernels' register figures (the
// table in DESIGN.md §6, "the drawn-once family"), which are the ones from
// before the kernels shared this file.  What it took: the records go to the
// helpers BY VALUE and the helpers are free functions (a reference or a member
// function takes the record's address and keeps it in memory until the helpers
// are inlined, after the first round of simplification: the arithmetic then
// lands elsewhere); the pair count, a pair's frame and its element are
// functions called where the kernels formed them and no fields filled ahead
// (sample_kin_kernel's SGPR spills moved by one or two with fields); and the
// NULL test of an optional output stays in the kernel, on its own argument.
struct DrawnChunk {
  int s, f0;                                  // the scene, the chunk's first frame
  int fcn;                                    // frames of this chunk (0 when F == 0)
  int nact;
  int nfc;                                    // ... of them below n_frames
  const uint8_t* mask;                        // the scene's row of ped_mask, or null
  int F, Nmax;
};

// nfc * nact: masked ones counted
__device__ __forceinline__ int drawn_npairs(DrawnChunk ch) { return ch.nfc * ch.nact; }
__device__ __forceinline__ bool drawn_live(DrawnChunk ch, int n) {
  return ch.mask ? ch.mask[n] != 0 : true;
}
__device__ __forceinline__ bool drawn_is_pair(DrawnChunk ch, int fl, int n) {
  return fl < ch.nfc && n < ch.nact && drawn_live(ch, n);
}
// frame fl of the chunk among all S * F, and the element of step 0 of its member n
__device__ __forceinline__ size_t drawn_frame(DrawnChunk ch, int fl) {
  return (size_t)ch.s * ch.F + ch.f0 + fl;
}
__device__ __forceinline__ int64_t drawn_elem0(DrawnChunk ch, size_t sf, int n) {
  return (int64_t)(sf * kL) * ch.Nmax + n;
}

__device__ __forceinline__ DrawnChunk drawn_chunk(const int32_t* n_active, const int32_t* n_frames,
                                                  const uint8_t* ped_mask, int F, int Nmax, int FC,
                                                  int C) {
  DrawnChunk ch;
  ch.s = blockIdx.x / C;
  const int c = blockIdx.x - ch.s * C;
  ch.f0 = c * FC;
  ch.fcn = min(FC, F - ch.f0);
  ch.nact = clampi(n_active[ch.s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[ch.s], 0, F) : F;
  ch.nfc = clampi(nf - ch.f0, 0, ch.fcn);
  ch.mask = ped_mask ? ped_mask + (size_t)ch.s * Nmax : nullptr;
  ch.F = F;
  ch.Nmax = Nmax;
  return ch;
}

// non-pairs: zeros in per_ped's NQ float4 columns (per_ped not NULL)
template <int NQ>
__device__ __forceinline__ void drawn_zero_per_ped(DrawnChunk ch, float* per_ped, int tid) {
  for (int idx = tid; idx < ch.fcn * ch.Nmax; idx += kDrThreads) {
    const int fl = idx / ch.Nmax, n = idx - fl * ch.Nmax;
    if (drawn_is_pair(ch, fl, n)) continue;
    float4* o = reinterpret_cast<float4*>(per_ped) + (drawn_frame(ch, fl) * ch.Nmax + n) * NQ;
#pragma unroll
    for (int q = 0; q < NQ; ++q) o[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// this lane's pair of the pass, its draw and the draw's seed
struct DrawnLane {
  int g, k;
  uint32_t lo, hi;                            // (seed + k) mod 2^64
};

__device__ __forceinline__ DrawnLane drawn_lane(int tid, int K, uint32_t seed_lo, uint32_t seed_hi) {
  DrawnLane ln;
  ln.g = tid / K;
  ln.k = tid - ln.g * K;
  ln.lo = seed_lo + (uint32_t)ln.k;
  ln.hi = seed_hi + (ln.lo < seed_lo ? 1u : 0u);
  return ln;
}

// the partners of draw k among the couples: the next h draws, circularly.
// h = (K - 1) / 2, one more for the lanes k < K / 2 of an even K (the antipodal
// couple once): a circular half range counts every unordered couple once
__device__ __forceinline__ int drawn_partners(int K, int k) {
  return (K - 1) / 2 + ((K & 1) == 0 && k < K / 2 ? 1 : 0);
}

// the lane's item of the pass that starts at pair `base`
struct DrawnItem {
  int gp;                                     // pairs of this pass
  bool valid;                                 // the lane's pair is one of them
  int fl, n;                                  // (0, 0) for a lane that is not valid
  bool on;                                    // ... and not masked: the lane draws
};

__device__ __forceinline__ DrawnItem drawn_item(DrawnChunk ch, int base, int G, int g) {
  DrawnItem it;
  it.gp = min(G, drawn_npairs(ch) - base);
  const int p = base + g;
  it.valid = g < it.gp;
  it.fl = it.valid ? p / ch.nact : 0;
  it.n = it.valid ? p - it.fl * ch.nact : 0;
  it.on = it.valid && drawn_live(ch, it.n);
  return it;
}

// a draw (time-major) into its slot, 6 ds_write_b128
__device__ __forceinline__ void store_draw(float* slot, const float (&x)[kL2]) {
  float4* o = reinterpret_cast<float4*>(slot);
#pragma unroll
  for (int q = 0; q < kL2 / 4; ++q)
    o[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}

// the draw of a lane that is off
__device__ __forceinline__ void zero_draw(float (&x)[kL2]) {
#pragma unroll
  for (int i = 0; i < kL2; ++i) x[i] = 0.f;
}

// ---------------------------------------------------------------------------
// row reductions: a scene's C chunk rows, added in chunk order
// ---------------------------------------------------------------------------
// out[s][i] = the sum of rows[s * C + c][i], i < 8, in T; rounded once to float
template <class T>
__global__ void __launch_bounds__(256) drawn_rows8_kernel(const T* __restrict__ rows, int S, int C,
                                                          float* __restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)S * 8) return;
  const int64_t s = id >> 3;
  const int i = (int)(id & 7);
  T v = 0;
  for (int c = 0; c < C; ++c) v += rows[((size_t)s * C + c) * 8 + i];
  out[id] = (float)v;
}

template <class T>
int drawn_rows8(const T* rows, int S, int C, float* out, hipStream_t st) {
  hipLaunchKernelGGL(drawn_rows8_kernel<T>, dim3((unsigned)(((int64_t)S * 8 + 255) / 256)), dim3(256),
                     0, st, rows, S, C, out);
  return check_launch("drawn_rows8_kernel");
}

// hist[s][HB] int32, tot[s][NT] int64 and, with NS > 0, sums[s][NS] f32
template <int NT, int NS>
__global__ void __launch_bounds__(256) drawn_hist_rows_kernel(
    const int32_t* __restrict__ hist_rows, const int64_t* __restrict__ tot_rows,
    const float* __restrict__ sum_rows, int S, int C, int HB, int32_t* __restrict__ hist,
    int64_t* __restrict__ tot, float* __restrict__ sums) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per = HB + NT + NS;                            // a scene's outputs
  if (id >= (int64_t)S * per) return;
  const int64_t s = id / per;
  const int i = (int)(id - s * per);
  if (i < HB) {
    int32_t v = 0;
    for (int c = 0; c < C; ++c) v += hist_rows[((size_t)s * C + c) * HB + i];
    hist[s * HB + i] = v;
  } else if (NS == 0 || i < HB + NT) {
    int64_t v = 0;
    for (int c = 0; c < C; ++c) v += tot_rows[((size_t)s * C + c) * NT + (i - HB)];
    tot[s * NT + (i - HB)] = v;
  } else {
    const int j = i - HB - NT;
    float v = 0.f;
    for (int c = 0; c < C; ++c) v += sum_rows[((size_t)s * C + c) * NS + j];
    sums[s * NS + j] = v;
  }
}

template <int NT, int NS>
int drawn_hist_rows(const int32_t* hist_rows, const int64_t* tot_rows, const float* sum_rows, int S,
                    int C, int HB, int32_t* hist, int64_t* tot, float* sums, hipStream_t st) {
  const int64_t ids = (int64_t)S * (HB + NT + NS);
  hipLaunchKernelGGL((drawn_hist_rows_kernel<NT, NS>), dim3((unsigned)((ids + 255) / 256)), dim3(256),
                     0, st, hist_rows, tot_rows, sum_rows, S, C, HB, hist, tot, sums);
  return check_launch("drawn_hist_rows_kernel");
}

// ---------------------------------------------------------------------------
// host tail
// ---------------------------------------------------------------------------
// what a launcher hands its kernel besides its own arguments
struct DrawnLaunch {
  DrawnGeom g;
  int64_t wgs;                                // S * C workgroups
  uint32_t seed_lo, seed_hi;
  int shared_targets;
  bool direct;                                // C == 1: the kernel writes the outputs, no rows
};

// `what` = the family ("sample_scores"), `prefix` = Head::kPrefix
inline int drawn_launch(const g2k_dims* d, const DrawnGeom& g, uint64_t seed, const char* prefix,
                        const char* what, DrawnLaunch& L) {
  L.g = g;
  L.wgs = (int64_t)d->S * g.C;
  if (L.wgs > 0x7fffffff)
    return set_err(G2K_EINVAL, "%s%s: %lld workgroups", prefix, what, (long long)L.wgs);
  L.seed_lo = (uint32_t)seed;
  L.seed_hi = (uint32_t)(seed >> 32);
  L.shared_targets = (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0;
  L.direct = g.C == 1;
  return G2K_OK;
}

// the four geometry entry points fill the same five fields
#define G2K_DRAWN_SAME(f)                                                                   \
  static_assert(G2K_SCORES_GEOM_##f == G2K_MODES_GEOM_##f &&                                \
                G2K_SCORES_GEOM_##f == G2K_RANKS_GEOM_##f &&                                \
                G2K_SCORES_GEOM_##f == G2K_KIN_GEOM_##f, "the families' GEOM_" #f " differ")
G2K_DRAWN_SAME(G); G2K_DRAWN_SAME(LANES); G2K_DRAWN_SAME(FC); G2K_DRAWN_SAME(C);
G2K_DRAWN_SAME(LDS_BYTES); G2K_DRAWN_SAME(FIELDS);
#undef G2K_DRAWN_SAME

// after the entry point's own checks of d and K
inline int drawn_write_geom(const DrawnGeom& g, int K, int lds_bytes, int32_t* out) {
  if (!out) return set_err(G2K_EINVAL, "out is NULL");
  out[G2K_SCORES_GEOM_G] = g.G;
  out[G2K_SCORES_GEOM_LANES] = K;
  out[G2K_SCORES_GEOM_FC] = g.FC;
  out[G2K_SCORES_GEOM_C] = g.C;
  out[G2K_SCORES_GEOM_LDS_BYTES] = lds_bytes;
  return G2K_OK;
}

}  // namespace
}  // namespace g2k
