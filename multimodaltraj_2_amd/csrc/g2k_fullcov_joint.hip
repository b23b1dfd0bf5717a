// g2k_fullcov_joint.hip — fused JOINT best-of-K evaluation of the
// full-covariance trajectory head: JADE_K / JFDE_K and the collision counts of
// its correlated draws.  The build's: the reference has no probabilistic head,
// so PARITY UNPINNED; tests/fullcov_joint_ref.py restates the definition over
// tests/fullcov_ref.py, tests/bestk_ref.py and tests/joint_ref.py.
//
// Definition.  That of g2k_joint.hip, word for word, with one change: joint
// sample k of scene-frame (s, f) is, for every member, the draw that
// g2k_fullcov_sample_f32 writes for seed (seed + k) mod 2^64 and factor chol
// (g2k_fullcov.hip: gauss_normals for e = ((s F + f) 12 + t) Nmax + n, acc =
// mu[i]; for j = 0..i: acc = fmaf(L[i][j], z[j], acc), a member whose element
// counter straddles 2^32 re-keyed as there).  Members, P, PP, JADE_k / JFDE_k,
// the independent minima with the lowest k, col(X) with fmaf(dx, dx, dy * dy) <
// radius * radius, col_pred, col_gt, sum_k col_k, col_best, the zeros and the
// outputs are those of g2k_joint_eval_f32.  Entries of chol above the diagonal
// are never read.
//
// Geometry.  That of g2k_joint.hip (g2k_joint.h: the same KD, the same rows,
// the same pair pass; g2k_joint_rows_kernel merges the rows): units of
// (scene-frame, slice of the draws), four waves per unit for Nmax > 64 with
// the 64 x 32 tile deal and the parity double-buffering, one wave with lane
// groups of 16 / 32 / 64 for Nmax <= 64.
//
// The draw.  A lane holds its member's 24 means and 24 target coordinates,
// both time-major ([2t + c]; the indices are constants after unrolling, so the
// order is one of names only).  The 24 sample registers that g2k_joint.hip
// fills per step are here the running sums of fullcov_advance
// (g2k_fullcov_draw.h), initialised to the means; the factor sits transposed
// in LDS (fullcov_load_lt, once per workgroup, shared by all lane groups) and
// is read per step by broadcast reads; step t's ADE / FDE term is taken as soon
// as a[2t], a[2t+1] are final.  The sample then goes to LDS as xy[i][24] (12 x,
// 12 y) and is paired from there: no draw reaches global memory.
#include "g2k_common.h"
#include "g2k_fullcov_draw.h"
#include "g2k_joint.h"

namespace g2k {
namespace {

// One member's 24 coordinates of a pass, time-major (c[2t] = x, c[2t+1] = y):
// kind 1 the targets, kind 2 the mean, kind 3 draw k with its ADE / FDE
// against the targets.
__device__ __forceinline__ void fcj_coords(int kind, int k, const float (&mu)[kL2],
                                           const float (&tg)[kL2], const float* Lt, int64_t e0,
                                           int Nmax, uint32_t seed_lo, uint32_t seed_hi,
                                           float (&c)[kL2], float& ade, float& fde) {
  if (kind != 3) {
#pragma unroll
    for (int r = 0; r < kL2; ++r) c[r] = kind == 1 ? tg[r] : mu[r];
    return;
  }
  const uint32_t ehi0 = (uint32_t)(e0 >> 32);
  const uint32_t lo = seed_lo + (uint32_t)k;               // (seed + k) mod 2^64
  const uint32_t hi = seed_hi + (lo < seed_lo ? 1u : 0u);
  const uint32_t stream0 = gauss_stream(lo, hi, ehi0);
#pragma unroll
  for (int r = 0; r < kL2; ++r) c[r] = mu[r];
  // step 0's element index, opaque to the compiler: the 12 indices (and the
  // 12 straddle tests) that it otherwise forms ahead of the pass loop and
  // keeps across it cost registers; 32-bit as in g2k_fullcov_best_of_k_kernel
  // (t Nmax < 2^32, so the high word moves at most once, by a carry)
  uint32_t elo0 = (uint32_t)e0;
  asm volatile("" : "+v"(elo0));
#pragma unroll
  for (int t = 0; t < kL; ++t) {
    const uint32_t elo = elo0 + (uint32_t)(t * Nmax);
    uint32_t stream = stream0;
    if (elo < elo0) stream = gauss_stream(lo, hi, ehi0 + 1u);   // a member that straddles 2^32
    float z0, z1;
    gauss_normals(stream, elo, z0, z1);
    fullcov_advance(Lt, t, z0, z1, c);
    // the step's sums are formed in the step: without this the compiler sinks
    // the later rows' FMAs past the following steps' (branching) sin / cos to
    // where the rows are used, and keeps the 300 values read from Lt (which
    // cannot move) in registers until then — 256 VGPRs + 219 AGPRs
#pragma unroll
    for (int i = 2 * t + 2; i < kL2; ++i) asm volatile("" : "+v"(c[i]));
    const float dx = c[2 * t] - tg[2 * t], dy = c[2 * t + 1] - tg[2 * t + 1];
    fde = sqrtf(fmaf(dx, dx, dy * dy));
    ade += fde;
  }
  ade *= 1.0f / 12.0f;
}

// time-major c -> xy[i][24] = 12 x, then 12 y
__device__ __forceinline__ void fcj_store(float4* dst, const float (&c)[kL2]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    dst[r] = make_float4(c[8 * r], c[8 * r + 2], c[8 * r + 4], c[8 * r + 6]);
    dst[3 + r] = make_float4(c[8 * r + 1], c[8 * r + 3], c[8 * r + 5], c[8 * r + 7]);
  }
}

// the members' means and targets, time-major
__device__ __forceinline__ void fcj_load(bool on, const float* __restrict__ pred,
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

__global__ void __launch_bounds__(kJtWaves * 64) g2k_fullcov_joint_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ chol, int F, int Nmax, int KD,
    int K, uint32_t seed_lo, uint32_t seed_hi, int shared_targets, float r2,
    int32_t* __restrict__ rows) {
  constexpr int WAVES = kJtWaves, NBUF = 2;
  constexpr int CAP = WAVES * 64;                          // members a unit holds (>= Nmax)
  __shared__ __attribute__((aligned(16))) float Lt[kL2 * kL2];
  __shared__ float4 xy[NBUF][CAP * 6];
  __shared__ float jpart[NBUF][WAVES][2];
  __shared__ int cpart[NBUF][WAVES];
  __shared__ int wcnt[WAVES];
  __shared__ int midx[CAP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sfi = blockIdx.x / KD, sl = blockIdx.x - sfi * KD;
  const int s = sfi / F, f = sfi - s * F;
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  int32_t* row = rows + (size_t)blockIdx.x * kJtRow;

  fullcov_load_lt(chol, Lt, tid, CAP);
  // compact the members: thread i owns member i = column midx[i]
  bool mem = f < nf && tid < nact;
  if (mem && ped_mask) mem = ped_mask[(size_t)s * Nmax + tid] != 0;
  const unsigned long long bal = __ballot(mem);
  const int pre = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wcnt[w] = __popcll(bal);
  __syncthreads();
  int base = 0, P = 0;
#pragma unroll
  for (int v = 0; v < WAVES; ++v) {
    const int c = wcnt[v];
    if (v < w) base += c;
    P += c;
  }
  if (mem) midx[base + pre] = tid;
  __syncthreads();
  if (P == 0) {                                            // uniform over the workgroup
    if (tid < kJtRow) row[tid] = 0;
    return;
  }

  const bool on = tid < P;
  const int n = on ? midx[tid] : 0;
  const size_t sf = (size_t)sfi;
  const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;        // element of step 0
  float mu[kL2], tg[kL2];
  fcj_load(on, pred, targets, sf, shared_targets ? (size_t)s : sf, n, Nmax, mu, tg);

  // passes: slice 0 first counts the targets (kind 1) and the mean (kind 2);
  // then the slice's draws k = sl, sl + KD, ... (kind 3; 4 once it is the
  // unit's best JADE so far)
  const int npre = sl == 0 ? 2 : 0;
  const int total = npre + (K - sl + KD - 1) / KD;
  const float invP = 1.0f / (float)P;
  float bJA = __builtin_inff(), bJF = __builtin_inff();
  int kJA = 0, kJF = 0, sumcol = 0, colbest = 0, colpred = 0, colgt = 0;
  int prev = 0;
  auto consume = [&](int par) {                            // the previous pass's collisions
    if (!prev) return;
    int c = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) c += cpart[par][v];
    colgt = prev == 1 ? c : colgt;                         // selects: no indexed private array
    colpred = prev == 2 ? c : colpred;
    sumcol += prev >= 3 ? c : 0;
    colbest = prev == 4 ? c : colbest;
  };
#pragma nounroll
  for (int q = 0; q < total; ++q) {
    const int par = q & (NBUF - 1);
    const int kind = q < npre ? q + 1 : 3;
    const int k = sl + (q - npre) * KD;
    float ade = 0.f, fde = 0.f;
    if (on) {
      float c[kL2];
      fcj_coords(kind, k, mu, tg, Lt, e0, Nmax, seed_lo, seed_hi, c, ade, fde);
      fcj_store(&xy[par][(size_t)tid * 6], c);
    }
    if (kind == 3) {                                       // every lane takes part in the butterfly
      const float sa = wave_sum(ade), sfd = wave_sum(fde);
      if (lane == 0) { jpart[par][w][0] = sa; jpart[par][w][1] = sfd; }
    }
    __syncthreads();
    consume((q - 1) & (NBUF - 1));
    int cur = kind;
    if (kind == 3) {
      float ja = 0.f, jf = 0.f;
#pragma unroll
      for (int v = 0; v < WAVES; ++v) { ja += jpart[par][v][0]; jf += jpart[par][v][1]; }
      ja *= invP; jf *= invP;
      if (ja < bJA) { bJA = ja; kJA = k; cur = 4; }        // ascending k, strict: the lowest k stays
      if (jf < bJF) { bJF = jf; kJF = k; }
    }
    prev = cur;
    const int ct = wave_sum_i(pair_pass(xy[par], P, w, lane, r2));
    if (lane == 0) cpart[par][w] = ct;
  }
  __syncthreads();
  consume((total - 1) & (NBUF - 1));
  if (tid == 0) {
    row[0] = (int32_t)__float_as_uint(bJA); row[1] = kJA;
    row[2] = (int32_t)__float_as_uint(bJF); row[3] = kJF;
    row[4] = sumcol; row[5] = colbest;
    row[6] = P; row[7] = colpred; row[8] = colgt; row[9] = 0;
  }
}

// Nmax <= 64: a unit on ONE wave, cut into 64 / GL groups of GL = 16, 32 or 64
// lanes (the smallest that holds P); every group takes another item of the
// unit's list in the same pass (g2k_joint_wave_kernel, g2k_joint.hip).  The
// groups draw different k from the same factor: their reads of Lt are the same
// address in every lane.  Without the occupancy hint the allocator settles at
// 256 VGPRs + 1 AGPR, one register over two waves per SIMD; with it 256 + 0,
// scratch 0, nothing spilled.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
g2k_fullcov_joint_wave_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ chol, int F, int Nmax, int KD,
    int K, uint32_t seed_lo, uint32_t seed_hi, int shared_targets, float r2,
    int32_t* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) float Lt[kL2 * kL2];
  __shared__ float4 xy[64 * 6 + 4];
  __shared__ int midx[64];
  const int lane = threadIdx.x;
  const int sfi = blockIdx.x / KD, sl = blockIdx.x - sfi * KD;
  const int s = sfi / F, f = sfi - s * F;
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  int32_t* row = rows + (size_t)blockIdx.x * kJtRow;

  fullcov_load_lt(chol, Lt, lane, 64);
  bool mem = f < nf && lane < nact;                        // Nmax <= 64: lane n looks at column n
  if (mem && ped_mask) mem = ped_mask[(size_t)s * Nmax + lane] != 0;
  const unsigned long long bal = __ballot(mem);
  const int P = __popcll(bal);
  if (mem) midx[__popcll(bal & ((1ull << lane) - 1ull))] = lane;
  __syncthreads();
  if (P == 0) {                                            // uniform
    if (lane < kJtRow) row[lane] = 0;
    return;
  }

  const int gl2 = P <= 16 ? 4 : (P <= 32 ? 5 : 6);         // log2 of the lanes per group
  const int GL = 1 << gl2, G = 64 >> gl2;
  const int g = lane >> gl2, i = lane & (GL - 1);          // group, member
  const bool on = i < P;
  const int n = on ? midx[i] : 0;
  const size_t sf = (size_t)sfi;
  const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;        // element of step 0
  float mu[kL2], tg[kL2];
  fcj_load(on, pred, targets, sf, shared_targets ? (size_t)s : sf, n, Nmax, mu, tg);
  float4* mine = xy + g * (GL * 6 + 1);                    // the group's sample: at most 386 + 1 < 388

  // items: slice 0 begins with the targets (kind 1) and the mean (kind 2),
  // then the slice's draws k = sl, sl + KD, ... (kind 3); pass q gives item
  // q G + g to group g (kind 0: none left)
  const int npre = sl == 0 ? 2 : 0;
  const int nitems = npre + (K - sl + KD - 1) / KD;
  const float invP = 1.0f / (float)P;
  float bJA = __builtin_inff(), bJF = __builtin_inff();
  int kJA = 0, kJF = 0, sumcol = 0, colbest = 0, colpred = 0, colgt = 0;
#pragma nounroll
  for (int q = 0; q * G < nitems; ++q) {
    const int item = q * G + g;
    const int kind = item < nitems ? (item < npre ? item + 1 : 3) : 0;
    const int k = sl + (item - npre) * KD;
    float c[kL2];
    float ade = 0.f, fde = 0.f;
    if (on && kind) {
      fcj_coords(kind, k, mu, tg, Lt, e0, Nmax, seed_lo, seed_hi, c, ade, fde);
      fcj_store(mine + i * 6, c);
    } else {
#pragma unroll
      for (int r = 0; r < kL2; ++r) c[r] = 0.f;
    }
    for (int off = 1; off < GL; off <<= 1) {               // every lane takes part
      ade += __shfl_xor(ade, off);
      fde += __shfl_xor(fde, off);
    }
    __syncthreads();                                       // one wave: the sample is in LDS
    int cnt = 0;
    for (int j = 1; j < P; ++j) {                          // a group's lanes read member j
      const float4* pj = mine + j * 6;
      float m = __builtin_inff();
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const float4 a = pj[u], bq = pj[3 + u];
        const float xj[4] = {a.x, a.y, a.z, a.w}, yj[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float dx = c[2 * (4 * u + v)] - xj[v], dy = c[2 * (4 * u + v) + 1] - yj[v];
          m = fminf(m, fmaf(dx, dx, dy * dy));
        }
      }
      cnt += (i < j && m < r2) ? 1 : 0;                    // lanes >= P: i < j never holds
    }
    for (int off = 1; off < GL; off <<= 1) cnt += __shfl_xor(cnt, off);
    __syncthreads();                                       // read before the next pass overwrites it
    if (kind == 3) {
      const float ja = ade * invP, jf = fde * invP;
      const bool better = ja < bJA;                        // ascending k, strict: the lowest k stays
      bJA = better ? ja : bJA; kJA = better ? k : kJA; colbest = better ? cnt : colbest;
      if (jf < bJF) { bJF = jf; kJF = k; }
      sumcol += cnt;
    }
    colgt = kind == 1 ? cnt : colgt;
    colpred = kind == 2 ? cnt : colpred;
  }
  for (int off = GL; off < 64; off <<= 1) {                // the groups' results
    const float oA = __shfl_xor(bJA, off), oF = __shfl_xor(bJF, off);
    const int okA = __shfl_xor(kJA, off), okF = __shfl_xor(kJF, off), ocb = __shfl_xor(colbest, off);
    if (oA < bJA || (oA == bJA && okA < kJA)) { bJA = oA; kJA = okA; colbest = ocb; }
    if (oF < bJF || (oF == bJF && okF < kJF)) { bJF = oF; kJF = okF; }
    sumcol += __shfl_xor(sumcol, off);
    colgt += __shfl_xor(colgt, off);
    colpred += __shfl_xor(colpred, off);
  }
  if (lane == 0) {
    row[0] = (int32_t)__float_as_uint(bJA); row[1] = kJA;
    row[2] = (int32_t)__float_as_uint(bJF); row[3] = kJF;
    row[4] = sumcol; row[5] = colbest;
    row[6] = P; row[7] = colpred; row[8] = colgt; row[9] = 0;
  }
}

}  // namespace

// the rows of g2k_joint_eval_f32: one [10] per unit, joint_kd_max units per
// scene-frame at most
int64_t fullcov_joint_eval_ws_bytes(const g2k_dims* d) {
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * joint_kd_max(*d) * kJtRow * 4;
}

int fullcov_joint_eval_launch(const g2k_dims* d, const float* pred, const float* targets,
                              const int32_t* n_active, const int32_t* n_frames,
                              const uint8_t* ped_mask, const float* chol, uint64_t seed, int K,
                              float radius, float* per_frame_f, int32_t* per_frame_i, float* sums_f,
                              int64_t* sums_i, int32_t* rows, hipStream_t st) {
  const JointGeom g = joint_geom(*d, K);
  const int64_t units = (int64_t)d->S * d->F * g.KD;
  if (units > 0x7fffffff)
    return set_err(G2K_EINVAL, "fullcov_joint_eval: %lld workgroups", (long long)units);
  const float r2 = radius * radius;
  const int shared = (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0;
  if (units > 0) {
    if (g.waves == 1)
      hipLaunchKernelGGL(g2k_fullcov_joint_wave_kernel, dim3((unsigned)units), dim3(64), 0, st, pred,
                         targets, n_active, n_frames, ped_mask, chol, d->F, d->Nmax, g.KD, K,
                         (uint32_t)seed, (uint32_t)(seed >> 32), shared, r2, rows);
    else
      hipLaunchKernelGGL(g2k_fullcov_joint_kernel, dim3((unsigned)units), dim3(kJtWaves * 64), 0, st,
                         pred, targets, n_active, n_frames, ped_mask, chol, d->F, d->Nmax, g.KD, K,
                         (uint32_t)seed, (uint32_t)(seed >> 32), shared, r2, rows);
    const int rc = check_launch("g2k_fullcov_joint_kernel");
    if (rc) return rc;
  }
  return joint_rows_launch(d, rows, g.KD, K, per_frame_f, per_frame_i, sums_f, sums_i, st);
}

}  // namespace g2k
