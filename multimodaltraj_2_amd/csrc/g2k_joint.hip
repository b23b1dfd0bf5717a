// g2k_joint.hip — fused JOINT best-of-K evaluation of a probabilistic head:
// JADE_K / JFDE_K (one draw index for the whole scene-frame) and the collision
// counts of the draws, of the mean prediction and of the targets.  ONE pair of
// kernels, joint_kernel<Head> and joint_wave_kernel<Head>, instantiated for
// the per-step bivariate-Gaussian head (g2k_joint_eval_f32), for the
// full-covariance trajectory head (g2k_fullcov_joint_eval_f32), for the
// Gaussian-mixture head (g2k_mix_joint_eval_f32, include/g2k_mix.h) and for the
// scene-coupled head (g2k_coupled_joint_eval_f32, include/g2k_coupled.h); the
// heads are the policies of g2k_head_draw.h.  The C entry points and their validator
// are at the end of this file.  The build's: the reference has no
// probabilistic head, so PARITY UNPINNED; tests/joint_ref.py restates the
// definition over oracle/g2k_ref.py gauss_sample and tests/bestk_ref.py,
// tests/fullcov_joint_ref.py over tests/fullcov_ref.py, tests/mix_eval_ref.py
// over tests/mixture_ref.py.
//
// Definition.  Inputs as g2k_best_of_k_f32 (g2k_bestk.hip) plus radius
// (finite, >= 0).  The MEMBERS of scene-frame (s, f), f < n_frames[s], are the
// n with n < n_active[s] and ped_mask[s][n] != 0 (the pairs of g2k_bestk.hip);
// P their number, PP = P (P - 1) / 2 the unordered member couples.
//   joint sample k (k < K) = for every member what the head's sampler
//     (g2k_gauss_sample_f32, g2k_fullcov_sample_f32) writes for seed
//     (seed + k) mod 2^64: the sampler's bits, the draws the head's marginal
//     best-of-K sees (a member whose element counter straddles 2^32 re-keyed
//     as there; entries of chol above the diagonal are never read)
//   JADE_k = mean over members of ADE_k, JFDE_k = mean over members of FDE_k
//     (ADE_k / FDE_k as in g2k_bestk.hip); minJADE / minJFDE taken
//     independently, kJA / kJF the lowest k attaining each
//   col(X) = number of member couples i < j with
//     min_t fmaf(dx, dx, dy * dy) < radius * radius   (f32, no sqrt; radius 0
//     counts nothing), d = X_i(t) - X_j(t) over the 12 predicted steps
//   col_k = col(draw k), col_pred = col(mean), col_gt = col(targets),
//   col_best = col_kJA
// Outputs (every element written; zeros where P = 0 or f >= n_frames[s]):
//   per_frame_f [S, F, 4] = {minJADE, minJFDE, kJA, kJF} or NULL
//   per_frame_i [S, F, 6] = {P, PP, col_pred, col_gt, sum_k col_k, col_best}
//     or NULL
//   sums_f [S, 4] = {sum_f P minJADE, sum_f P minJFDE, K, 0}
//   sums_i [S, 6] (int64) = sum_f of the per_frame_i columns
//
// Geometry.  A UNIT is (scene-frame, slice of the K draws): the draws are
// dealt round-robin to KD units (k = slice, slice + KD, ...).  KD comes from
// the shapes alone (joint_geom): enough units to fill the device (2048 waves /
// 512 workgroups), at most 8, and at least two draws per unit so that a unit's
// set-up (compaction, 24 means and 24 target coordinates per member into
// registers, both time-major, [2t + c]) is shared.  The unit first compacts
// its members (ballot + prefix count): non-members never reach the hash or the
// pair loop.  Its ITEMS are, for slice 0, the targets and the mean prediction
// (col_gt, col_pred), then for every slice its draws.  An item's sample is
// written to LDS as xy[i][24] (12 x, 12 y: six 16-byte reads fetch a whole
// member) — no draw reaches global memory — and paired all-against-all from
// there: a lane keeps member i's 24 coordinates in registers, all lanes that
// share a sample read the same member j (one LDS address: a broadcast), and
// count i < j only.
//   Nmax > 64 (joint_kernel; dense_crowd, P up to 256): four waves per
// unit, thread i owns member i, one item per pass.  The draw's ADE / FDE sums
// go lanes-by-butterfly, waves-in-order.  The pair pass walks 64-row x
// 32-column tiles of the upper triangle, dealt round-robin to the waves.  The
// coordinates and the partial sums are double-buffered on the pass's parity,
// one barrier per pass: waves that finish their tiles early draw the next
// sample while the others still count.  A pass's collision total is read one
// barrier later (the same parity argument).
//   Nmax <= 64 (joint_wave_kernel; real-data evaluation: F 1, hundreds of
// scenes, P 2..32): one wave per unit, cut into 64 / GL groups of GL = 16, 32
// or 64 lanes (the smallest that holds P); every group takes another item in
// the same pass, so a small scene-frame still fills the wave.
//   Each unit leaves one row [10] in the caller's workspace; g2k_joint_rows_
// kernel (one wave per scene) combines a scene-frame's KD rows — minima
// lexicographically on (value, k), so the lowest k wins whatever the dealing,
// counts as integers — and adds the frames in a fixed order (lane-strided,
// then the butterfly).  No atomics: results are bit-identical from run to run
// and, JADE_k being computed the same way in whichever unit draws k, do not
// depend on KD.
#include "g2k_checks.h"
#include "g2k_common.h"
#include "g2k_coupled.h"
#include "g2k_head_draw.h"
#include "g2k_mix.h"

namespace g2k {
namespace {

constexpr int kJtMaxDeal = 8;        // units per scene-frame at most
constexpr int kJtRow = 10;           // int32 words per unit row
constexpr int kJtTileJ = 32;         // columns (j) per pair-pass tile
constexpr int kJtWaves = 4;          // waves of a unit when Nmax > 64

struct JointGeom { int waves, KD; };

int joint_kd_max(const g2k_dims& d) {
  const int64_t sf = (int64_t)d.S * d.F;
  const int64_t fill = d.Nmax <= 64 ? 2048 : 512;      // waves / workgroups that fill 256 CUs
  int64_t kd = sf > 0 ? (fill + sf - 1) / sf : 1;
  if (kd > kJtMaxDeal) kd = kJtMaxDeal;
  return (int)kd;
}

JointGeom joint_geom(const g2k_dims& d, int K) {
  JointGeom g;
  g.waves = d.Nmax <= 64 ? 1 : kJtWaves;
  g.KD = joint_kd_max(d);
  const int two = (K + 1) / 2;                          // >= 2 draws per unit (K = 1: one unit)
  if (g.KD > two) g.KD = two;
  return g;
}

// Collisions of the LDS sample `buf` (xy[i][24], P members) among this wave's
// tiles: tile (b, c) = rows 64 b .. 64 b + 63 x columns 32 c .. 32 c + 31,
// c >= 2 b (the upper triangle), tile number % kJtWaves == w.
__device__ __forceinline__ int pair_pass(const float4* __restrict__ buf, int P, int w, int lane,
                                         float r2) {
  const int NB = (P + 63) >> 6, NC = (P + kJtTileJ - 1) / kJtTileJ;
  int cnt = 0, tix = 0;
  for (int b = 0; b < NB; ++b) {
    bool loaded = false;
    float xi[kL], yi[kL];
    const int i = (b << 6) + lane;
    for (int c = 2 * b; c < NC; ++c, ++tix) {
      if ((tix & (kJtWaves - 1)) != w) continue;
      if (!loaded) {                                      // this row block's coordinates
        const float4* pi = buf + (size_t)min(i, P - 1) * 6;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 a = pi[q], bq = pi[3 + q];
          xi[4 * q] = a.x; xi[4 * q + 1] = a.y; xi[4 * q + 2] = a.z; xi[4 * q + 3] = a.w;
          yi[4 * q] = bq.x; yi[4 * q + 1] = bq.y; yi[4 * q + 2] = bq.z; yi[4 * q + 3] = bq.w;
        }
        loaded = true;
      }
      const int j0 = max(c * kJtTileJ, (b << 6) + 1), j1 = min((c + 1) * kJtTileJ, P);
      for (int j = j0; j < j1; ++j) {                     // uniform: every lane reads member j
        const float4* pj = buf + (size_t)j * 6;
        float m = __builtin_inff();
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 a = pj[q], bq = pj[3 + q];
          const float xj[4] = {a.x, a.y, a.z, a.w}, yj[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float dx = xi[4 * q + u] - xj[u], dy = yi[4 * q + u] - yj[u];
            m = fminf(m, fmaf(dx, dx, dy * dy));
          }
        }
        cnt += (i < j && m < r2) ? 1 : 0;                 // rows >= P: i < j never holds
      }
    }
  }
  return cnt;
}

// One member's 24 coordinates of a pass, time-major (c[2t] = x, c[2t+1] = y):
// kind 1 the targets, kind 2 the mean, kind 3 draw k with its ADE / FDE
// against the targets (step t's term is taken as soon as the step is final).
template <class Head>
__device__ __forceinline__ void joint_coords(const Head& head, int kind, int k, const float (&mu)[kL2],
                                             const float (&tg)[kL2], int64_t e0, int n, int Nmax,
                                             uint32_t seed_lo, uint32_t seed_hi, float (&c)[kL2],
                                             float& ade, float& fde) {
  if (kind != 3) {
#pragma unroll
    for (int r = 0; r < kL2; ++r) c[r] = kind == 1 ? tg[r] : mu[r];
    return;
  }
  const uint32_t lo = seed_lo + (uint32_t)k;               // (seed + k) mod 2^64
  const uint32_t hi = seed_hi + (lo < seed_lo ? 1u : 0u);
  head.draw(lo, hi, e0, n, Nmax, mu, [&](int t, float x, float y) {
    c[2 * t] = x; c[2 * t + 1] = y;
    const float dx = x - tg[2 * t], dy = y - tg[2 * t + 1];
    fde = sqrtf(fmaf(dx, dx, dy * dy));
    ade += fde;
  });
  ade *= 1.0f / 12.0f;
}

// time-major c -> xy[i][24] = 12 x, then 12 y
__device__ __forceinline__ void joint_store(float4* dst, const float (&c)[kL2]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    dst[r] = make_float4(c[8 * r], c[8 * r + 2], c[8 * r + 4], c[8 * r + 6]);
    dst[3 + r] = make_float4(c[8 * r + 1], c[8 * r + 3], c[8 * r + 5], c[8 * r + 7]);
  }
}

template <class Head>
__global__ void __launch_bounds__(kJtWaves * 64) joint_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int KD, int K, uint32_t seed_lo, uint32_t seed_hi, int shared_targets, float r2,
    int32_t* __restrict__ rows) {
  constexpr int WAVES = kJtWaves, NBUF = 2;
  constexpr int CAP = WAVES * 64;                          // members a unit holds (>= Nmax)
  __shared__ typename Head::Lds hlds;
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

  Head::template stage<CAP>(head_params, hlds, tid);
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
  Head head;
  head.bind(hlds);

  const bool on = tid < P;
  const int n = on ? midx[tid] : 0;
  const size_t sf = (size_t)sfi;
  const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;        // element of step 0
  float mu[kL2], tg[kL2];
  load_mu_tg(on, pred, targets, sf, shared_targets ? (size_t)s : sf, n, Nmax, mu, tg);

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
      joint_coords(head, kind, k, mu, tg, e0, n, Nmax, seed_lo, seed_hi, c, ade, fde);
      joint_store(&xy[par][(size_t)tid * 6], c);
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

// Nmax <= 64: a unit on ONE wave.  Its members fill P of the 64 lanes, so the
// wave is cut into G = 64 / GL groups of GL = 16, 32 or 64 lanes (the smallest
// that holds P) and every group takes another item of the unit's list (targets,
// mean, draws) in the same pass: each group has its own sample in LDS, the lanes
// of a group read the same column j (one address per group; the groups' samples
// start 16 bytes off a multiple of the bank cycle, so their reads do not
// collide), sums run over the group's lanes by an xor butterfly.  The groups'
// results are merged like the units' (lexicographic minima, integer sums).  The
// groups draw different k from the same head: what the per-step and the
// full-covariance head read of it in LDS is the same address in every lane
// (the mixture head's lanes read their own component's factor, whatever the
// group: MixHead, g2k_head_draw.h).  The occupancy hint is the head's
// (kJointWaveOccupancy): without it the allocator settles the full-covariance
// instantiation at 256 VGPRs + 1 AGPR, one register over two waves per SIMD;
// with it 256 + 0, scratch 0, nothing spilled.  The per-step instantiation
// runs without one (205 VGPRs): with the hint it came out at 191 VGPRs and
// 1.8 us slower at the real-data evaluation's shape (51.8 -> 53.6 us).
template <class Head>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(Head::kJointWaveOccupancy))) joint_wave_kernel(
    const float* __restrict__ pred, const float* __restrict__ targets,
    const int32_t* __restrict__ n_active, const int32_t* __restrict__ n_frames,
    const uint8_t* __restrict__ ped_mask, const float* __restrict__ head_params, int F, int Nmax,
    int KD, int K, uint32_t seed_lo, uint32_t seed_hi, int shared_targets, float r2,
    int32_t* __restrict__ rows) {
  __shared__ typename Head::Lds hlds;
  __shared__ float4 xy[64 * 6 + 4];
  __shared__ int midx[64];
  const int lane = threadIdx.x;
  const int sfi = blockIdx.x / KD, sl = blockIdx.x - sfi * KD;
  const int s = sfi / F, f = sfi - s * F;
  const int nact = clampi(n_active[s], 0, Nmax);
  const int nf = n_frames ? clampi(n_frames[s], 0, F) : F;
  int32_t* row = rows + (size_t)blockIdx.x * kJtRow;

  Head::template stage<64>(head_params, hlds, lane);
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
  Head head;
  head.bind(hlds);

  const int gl2 = P <= 16 ? 4 : (P <= 32 ? 5 : 6);         // log2 of the lanes per group
  const int GL = 1 << gl2, G = 64 >> gl2;
  const int g = lane >> gl2, i = lane & (GL - 1);          // group, member
  const bool on = i < P;
  const int n = on ? midx[i] : 0;
  const size_t sf = (size_t)sfi;
  const int64_t e0 = (int64_t)(sf * kL) * Nmax + n;        // element of step 0
  float mu[kL2], tg[kL2];
  load_mu_tg(on, pred, targets, sf, shared_targets ? (size_t)s : sf, n, Nmax, mu, tg);
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
      joint_coords(head, kind, k, mu, tg, e0, n, Nmax, seed_lo, seed_hi, c, ade, fde);
      joint_store(mine + i * 6, c);
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

// One wave per scene: a scene-frame's KD rows -> per_frame_f / per_frame_i,
// then the scene's sums over its frames (lane-strided, then the butterfly).
__global__ void __launch_bounds__(64) g2k_joint_rows_kernel(
    const int32_t* __restrict__ rows, int F, int KD, int K, float* __restrict__ per_frame_f,
    int32_t* __restrict__ per_frame_i, float* __restrict__ sums_f, long long* __restrict__ sums_i) {
  const int s = blockIdx.x, lane = threadIdx.x;
  float fa = 0.f, ff = 0.f;
  long long acc[6] = {0, 0, 0, 0, 0, 0};
  for (int f = lane; f < F; f += 64) {
    const size_t sf = (size_t)s * F + f;
    const int32_t* r = rows + sf * KD * kJtRow;
    const int P = r[6];
    float bA = 0.f, bF = 0.f;
    int kA = 0, kF = 0, col[6] = {0, 0, 0, 0, 0, 0};
    if (P > 0) {
      bA = __uint_as_float((uint32_t)r[0]); kA = r[1];
      bF = __uint_as_float((uint32_t)r[2]); kF = r[3];
      col[0] = P; col[1] = P * (P - 1) / 2; col[2] = r[7]; col[3] = r[8]; col[4] = r[4]; col[5] = r[5];
      for (int d = 1; d < KD; ++d) {
        const int32_t* o = r + (size_t)d * kJtRow;
        const float oA = __uint_as_float((uint32_t)o[0]), oF = __uint_as_float((uint32_t)o[2]);
        if (oA < bA || (oA == bA && o[1] < kA)) { bA = oA; kA = o[1]; col[5] = o[5]; }
        if (oF < bF || (oF == bF && o[3] < kF)) { bF = oF; kF = o[3]; }
        col[4] += o[4];
      }
    }
    if (per_frame_f) {
      float* o = per_frame_f + sf * 4;
      o[0] = bA; o[1] = bF; o[2] = (float)kA; o[3] = (float)kF;
    }
    if (per_frame_i) {
#pragma unroll
      for (int i = 0; i < 6; ++i) per_frame_i[sf * 6 + i] = col[i];
    }
    fa += (float)P * bA;
    ff += (float)P * bF;
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] += col[i];
  }
  fa = wave_sum(fa);
  ff = wave_sum(ff);
#pragma unroll
  for (int i = 0; i < 6; ++i)
    for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_xor(acc[i], off);
  if (lane == 0) {
    sums_f[(size_t)s * 4 + 0] = fa; sums_f[(size_t)s * 4 + 1] = ff;
    sums_f[(size_t)s * 4 + 2] = (float)K; sums_f[(size_t)s * 4 + 3] = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) sums_i[(size_t)s * 6 + i] = acc[i];
  }
}

template <class Head>
int joint_eval_launch_as(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                         const float* head_params, uint64_t seed, int K, float radius,
                         float* per_frame_f, int32_t* per_frame_i, float* sums_f, int64_t* sums_i,
                         int32_t* rows, hipStream_t st) {
  const JointGeom g = joint_geom(*d, K);
  const int64_t units = (int64_t)d->S * d->F * g.KD;
  if (units > 0x7fffffff)
    return set_err(G2K_EINVAL, "%sjoint_eval: %lld workgroups", Head::kPrefix, (long long)units);
  const float r2 = radius * radius;
  const int shared = (d->flags & G2K_STEP_TARGETS_SHARED) ? 1 : 0;
  if (units > 0) {
    if (g.waves == 1)
      hipLaunchKernelGGL(joint_wave_kernel<Head>, dim3((unsigned)units), dim3(64), 0, st, pred, targets,
                         n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.KD, K,
                         (uint32_t)seed, (uint32_t)(seed >> 32), shared, r2, rows);
    else
      hipLaunchKernelGGL(joint_kernel<Head>, dim3((unsigned)units), dim3(kJtWaves * 64), 0, st, pred,
                         targets, n_active, n_frames, ped_mask, head_params, d->F, d->Nmax, g.KD, K,
                         (uint32_t)seed, (uint32_t)(seed >> 32), shared, r2, rows);
    const int rc = check_launch("joint_kernel");
    if (rc) return rc;
  }
  // the merge of the units' rows (KD per scene-frame): the same for every head
  hipLaunchKernelGGL(g2k_joint_rows_kernel, dim3((unsigned)d->S), dim3(64), 0, st, rows, d->F, g.KD, K,
                     per_frame_f, per_frame_i, sums_f, reinterpret_cast<long long*>(sums_i));
  return check_launch("g2k_joint_rows_kernel");
}

// one row [10] per unit; at most joint_kd_max units per scene-frame
int64_t joint_eval_ws_bytes(const g2k_dims* d) {
  if (!d || d->S < 0 || d->F < 0) return -1;
  return (int64_t)d->S * (d->F > 1 ? d->F : 1) * joint_kd_max(*d) * kJtRow * 4;
}

// the argument checks, before any HIP call; `name` is the entry point's in the
// message; G2K_OK with S > 0: launch
int joint_eval_validate(const char* name, const g2k_dims* d, const void* pred, const void* targets,
                        const void* n_active, const void* head, int32_t K, float radius,
                        const void* sums_f, const void* sums_i, const void* workspace,
                        int64_t workspace_bytes) {
  if (const int rc = check_dims(d)) return rc;
  if (d->flags & G2K_STEP_PRED_PED_MAJOR)
    return set_err(G2K_EUNSUPPORTED, "%s reads pred_path_band [S, F, 2L, Nmax]", name);
  if (const int rc = check_pair_sizes(d)) return rc;
  if (K < 1 || K > 4096) return set_err(G2K_EINVAL, "K=%d (1..4096)", K);
  if (!(radius >= 0.f) || radius > 3.402823466e38f)
    return set_err(G2K_EINVAL, "radius=%g (finite, >= 0)", (double)radius);
  if (const int rc = check_required({pred, targets, n_active, head, sums_f, sums_i})) return rc;
  if (const int rc = check_targets(targets)) return rc;
  if (((uintptr_t)sums_i) & 7) return set_err(G2K_EINVAL, "sums_i must be 8-byte aligned");
  // rows of int32
  return check_workspace(d, workspace, workspace_bytes, joint_eval_ws_bytes(d), 4, ", 4-byte aligned");
}

template <class Head>
int joint_eval(const char* name, const g2k_dims* d, const float* pred, const float* targets,
               const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
               const float* head, uint64_t seed, int32_t K, float radius, float* per_frame_f,
               int32_t* per_frame_i, float* sums_f, int64_t* sums_i, void* workspace,
               int64_t workspace_bytes, void* stream) {
  const int rc = joint_eval_validate(name, d, pred, targets, n_active, head, K, radius, sums_f, sums_i,
                                     workspace, workspace_bytes);
  if (rc || d->S == 0) return rc;
  return joint_eval_launch_as<Head>(d, pred, targets, n_active, n_frames, ped_mask, head, seed, K,
                                    radius, per_frame_f, per_frame_i, sums_f, sums_i,
                                    static_cast<int32_t*>(workspace), (hipStream_t)stream);
}

}  // namespace
}  // namespace g2k

using namespace g2k;

extern "C" {

// the heads share the geometry, so the workspace too
int64_t g2k_joint_eval_workspace_bytes(const g2k_dims* d) { return joint_eval_ws_bytes(d); }
int64_t g2k_fullcov_joint_eval_workspace_bytes(const g2k_dims* d) { return joint_eval_ws_bytes(d); }
int64_t g2k_mix_joint_eval_workspace_bytes(const g2k_dims* d) { return joint_eval_ws_bytes(d); }
int64_t g2k_coupled_joint_eval_workspace_bytes(const g2k_dims* d) { return joint_eval_ws_bytes(d); }

// the full-covariance head's first: see g2k_bestk.hip
int g2k_fullcov_joint_eval_f32(const g2k_dims* d, const float* pred, const float* targets,
                               const int32_t* n_active, const int32_t* n_frames,
                               const uint8_t* ped_mask, const float* chol, uint64_t seed,
                               int32_t K, float radius, float* per_frame_f, int32_t* per_frame_i,
                               float* sums_f, int64_t* sums_i, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  return joint_eval<FullCovHead>("fullcov_joint_eval", d, pred, targets, n_active, n_frames, ped_mask,
                                 chol, seed, K, radius, per_frame_f, per_frame_i, sums_f, sums_i,
                                 workspace, workspace_bytes, stream);
}

int g2k_joint_eval_f32(const g2k_dims* d, const float* pred, const float* targets,
                       const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                       const float* head, uint64_t seed, int32_t K, float radius, float* per_frame_f,
                       int32_t* per_frame_i, float* sums_f, int64_t* sums_i, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return joint_eval<PerStepHead>("joint_eval", d, pred, targets, n_active, n_frames, ped_mask, head,
                                 seed, K, radius, per_frame_f, per_frame_i, sums_f, sums_i, workspace,
                                 workspace_bytes, stream);
}

// mix [8][608] (include/g2k_mix.h).  Every member selects its own component,
// so one joint sample mixes components across the members of a scene-frame.
// joint_kernel<MixHead> holds 69.7 KB of static LDS (the double-buffered
// sample, 48 KB, beside the eight staged factors): above 64 KB, inside
// gfx950's 160 KB per workgroup, two workgroups per CU.
int g2k_mix_joint_eval_f32(const g2k_dims* d, const float* pred, const float* targets,
                           const int32_t* n_active, const int32_t* n_frames,
                           const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                           float radius, float* per_frame_f, int32_t* per_frame_i, float* sums_f,
                           int64_t* sums_i, void* workspace, int64_t workspace_bytes, void* stream) {
  return joint_eval<MixHead>("mix_joint_eval", d, pred, targets, n_active, n_frames, ped_mask, mix,
                             seed, K, radius, per_frame_f, per_frame_i, sums_f, sums_i, workspace,
                             workspace_bytes, stream);
}

// cpl [2][24][24] (include/g2k_coupled.h).  Every member of a scene-frame forms
// the shared part itself from the scene-frame's own normals, so one joint
// sample moves the members together.
int g2k_coupled_joint_eval_f32(const g2k_dims* d, const float* pred, const float* targets,
                               const int32_t* n_active, const int32_t* n_frames,
                               const uint8_t* ped_mask, const float* cpl, uint64_t seed, int32_t K,
                               float radius, float* per_frame_f, int32_t* per_frame_i, float* sums_f,
                               int64_t* sums_i, void* workspace, int64_t workspace_bytes, void* stream) {
  return joint_eval<CoupledHead>("coupled_joint_eval", d, pred, targets, n_active, n_frames, ped_mask,
                                 cpl, seed, K, radius, per_frame_f, per_frame_i, sums_f, sums_i,
                                 workspace, workspace_bytes, stream);
}

}  // extern "C"
