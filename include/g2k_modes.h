/*
 * g2k_modes.h — k-means reduction of a probabilistic head's samples to M modes
 * (added after ABI 11; detect by symbol: g2k_abi_version() stays 11).  A header
 * of its own, as include/g2k_scores.h: what a binding looks up by name
 * (multimodaltraj_2_amd/modes.py).  The kernel is csrc/g2k_modes.hip.
 *
 * K draws of a pair are clustered to M representative trajectories with
 * probabilities (Lloyd's algorithm over the 24-D trajectories), and the M
 * centres are scored: minADE_M / minFDE_M, their Brier variants and the miss
 * rate, for the per-step head, the full-covariance head and the mixture head
 * alike.  The build's: the reference has no probabilistic head, so PARITY
 * UNPINNED; tests/modes_ref.py restates the definition in float64 NumPy.
 *
 * Inputs, pairs and draws are those of g2k_best_of_k_f32 (include/g2k_hip.h).
 * Draw k, k < K, of a pair (s, f, n) is bit for bit what the head's sampler
 * (g2k_gauss_sample_f32, g2k_fullcov_sample_f32, g2k_mix_sample_f32) writes for
 * seed (seed + k) mod 2^64: X_k, 24 f32 coordinates, index j = 2t + c.
 * Parameters: M modes in 1..32, K draws in M..256, iters in 0..64, miss_radius
 * finite and >= 0.
 *
 * EVERYTHING AFTER THE DRAW IS DOUBLE PRECISION.  Lloyd's assignment is an
 * argmin; in f32 a near-tie flips it and the flip changes every later
 * iteration, so an f32 loop cannot be reproduced by a float64 checker, a
 * double one can.
 *   start     c_m = X_m, m < M
 *   iters x   assign: d2(k, m) = sum_j (X_k[j] - c_m[j])^2, j ascending;
 *                     a(k) = the lowest m that attains the minimum
 *             update: n_m = #{k : a(k) = m}; c_m = (sum of X_k over a(k) = m,
 *                     k ascending) / n_m; a cluster with n_m = 0 keeps its
 *                     centre
 *   final     one more assignment against the final centres: n_m, w_m = n_m /
 *             K, inertia = 1/K sum_k d2(k, a(k)), live = #{m : n_m > 0}
 *   scoring   against the target Y: A_m = 1/12 sum_t ||c_m(t) - Y(t)||_2, F_m =
 *             ||c_m(11) - Y(11)||_2; cA = min_m A_m, mA the lowest m attaining
 *             it; cF, mF likewise from F_m.  All M centres are candidates, the
 *             empty clusters' too.
 *
 * per_ped [S, F, Nmax, 8] f32 or NULL: {cA, cF, mA, mF, w_mA, w_mF, inertia,
 *   live} per pair.
 * centres [S, F, M, 2L, Nmax] f32 or NULL: each [:, :, m] slice laid out as
 *   pred (rows 0..11 x, 12..23 y), so it can be fed to the other entry points.
 * weights [S, F, M, Nmax] f32 or NULL: w_m.
 * All three are exactly zero for non-pairs, and every element is written.
 * out [S, 8] f32, required, over the scene's pairs: sum cA, sum cF, sum (1 -
 *   w_mA)^2, sum (1 - w_mF)^2, the number of pairs with cF > miss_radius, sum
 *   inertia, sum live, the pair count.  Accumulated in double in a fixed order
 *   and rounded once; no atomics: repeated calls are bit-identical, and out's
 *   bits do not depend on which optional outputs are NULL.
 * Columns >= n_active, frames >= n_frames and masked columns of pred and
 * targets are never read.
 *
 * What the host forms from the sums (means over the pairs): min_ade, min_fde,
 * brier_ade = mean of cA + (1 - w_mA)^2, brier_fde, miss_rate, inertia, live.
 *
 * g2k_sample_modes_f32 (head [3][12]), g2k_fullcov_sample_modes_f32 (chol
 * [24][24]), g2k_mix_sample_modes_f32 (mix [8][608], include/g2k_mix.h): one
 * launch (two when a scene has several workgroups) on the stream, no
 * allocation, capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED, anything
 * else is G2K_EUNSUPPORTED; Nmax in 1..256; workspace >=
 * g2k_sample_modes_workspace_bytes(d) (one size for the three heads; -1 for
 * dims out of range).  Every argument check comes before any HIP call.  S = 0
 * is a no-op; F = 0 writes out = 0.
 * g2k_sample_modes_geometry: host arithmetic, no HIP call; what the launcher
 * itself computes, out[G2K_MODES_GEOM_FIELDS]: the pairs of one pass of a
 * workgroup (G), the lanes of a pair (K: one per draw), the frames of a
 * workgroup (FC), the workgroups of a scene (C) and the LDS bytes of the
 * workgroup without the head's own (the per-step head adds 192, the
 * full-covariance head 2304, the mixture head 19376).
 *
 * Alignment (bytes) of g2k_sample_modes_f32, g2k_fullcov_sample_modes_f32
 * and g2k_mix_sample_modes_f32: targets 8, per_ped 16, workspace 8.
 */
#ifndef G2K_MODES_H_
#define G2K_MODES_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_MODES_MMAX 32
#define G2K_MODES_KMAX 256
#define G2K_MODES_ITERS_MAX 64

#define G2K_MODES_GEOM_G 0
#define G2K_MODES_GEOM_LANES 1
#define G2K_MODES_GEOM_FC 2
#define G2K_MODES_GEOM_C 3
#define G2K_MODES_GEOM_LDS_BYTES 4
#define G2K_MODES_GEOM_FIELDS 5

int64_t g2k_sample_modes_workspace_bytes(const g2k_dims* d);
int g2k_sample_modes_geometry(const g2k_dims* d, int32_t K, int32_t M, int32_t* out);
int g2k_sample_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames,
                         const uint8_t* ped_mask, const float* head, uint64_t seed, int32_t K,
                         int32_t M, int32_t iters, float miss_radius, float* per_ped,
                         float* centres, float* weights, float* out, void* workspace,
                         int64_t workspace_bytes, void* stream);
int g2k_fullcov_sample_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                                 const int32_t* n_active, const int32_t* n_frames,
                                 const uint8_t* ped_mask, const float* chol, uint64_t seed,
                                 int32_t K, int32_t M, int32_t iters, float miss_radius,
                                 float* per_ped, float* centres, float* weights, float* out,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int g2k_mix_sample_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                             const int32_t* n_active, const int32_t* n_frames,
                             const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                             int32_t M, int32_t iters, float miss_radius, float* per_ped,
                             float* centres, float* weights, float* out, void* workspace,
                             int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_MODES_H_ */
