/*
 * g2k_scores.h — trajectory-level scores of a probabilistic head's samples
 * (added after ABI 11; detect by symbol: g2k_abi_version() stays 11).  A header
 * of its own, as include/g2k_mix.h: what a binding looks up by name
 * (multimodaltraj_2_amd/scores.py).  The kernel is csrc/g2k_scores.hip.
 *
 * The energy score, the variogram score, the expected ADE / FDE of a draw and
 * the average pairwise displacement (APD) of the K draws, for the per-step
 * head, the full-covariance head and the mixture head alike.  The build's: the
 * reference has no probabilistic head, so PARITY UNPINNED; tests/scores_ref.py
 * restates the definition in float64 NumPy.
 *
 * Inputs, pairs and draws are those of g2k_best_of_k_f32 (include/g2k_hip.h),
 * K in 2..256.  Draw k of a pair (s, f, n) is bit for bit what the head's
 * sampler (g2k_gauss_sample_f32, g2k_fullcov_sample_f32, g2k_mix_sample_f32)
 * writes for seed (seed + k) mod 2^64.
 *
 * X_k(t) = draw k's 2-D position at step t, Y(t) = the target.  For two
 * trajectories A and B:
 *   a(A, B) = 1/12 sum_t ||A(t) - B(t)||_2      (the ADE of g2k_best_of_k_f32)
 *   f(A, B) = ||A(11) - B(11)||_2
 *   r(A, B) = ||A - B||_2 over all 24 coordinates
 *
 * per_ped [S, F, Nmax, 8] f32 or NULL, per pair:
 *   0  mA = 1/K sum_k a(X_k, Y)                 the expected ADE of a draw
 *   1  mF = 1/K sum_k f(X_k, Y)
 *   2  mR = 1/K sum_k r(X_k, Y)
 *   3  pA = 2/(K (K - 1)) sum_{k<l} a(X_k, X_l) the APD
 *   4  pF = the same with f
 *   5  pR = the same with r
 *   6  vs = sum_{t<u} (||Y(t) - Y(u)||_2^(1/2) - 1/K sum_k ||X_k(t) - X_k(u)||_2^(1/2))^2
 *           the variogram score of order 1/2 over the 66 step pairs
 *   7  0
 * Non-pairs are exactly zero; every element is written.  Columns >= n_active
 * of pred and targets are never read.
 * out [S, 8] f32: the sums of columns 0..6 over the scene's pairs, the pair
 * count in column 7.  Fixed summation order, no atomics: repeated calls are
 * bit-identical, and out's bits do not depend on whether per_ped is NULL.
 *
 * What the host forms from the sums (per pair, then the mean over the pairs;
 * all linear in the sums):
 *   es_traj = mR - pR / 2   the fair (unbiased) energy score of the 24-D law,
 *                           strictly proper for the joint
 *   es_ade  = mA - pA / 2   the mean of the 12 per-step energy scores: sees
 *                           the marginals only
 *   es_fde  = mF - pF / 2
 *   mean_ade = mA, mean_fde = mF, apd = pA, vs
 * pR <= 2 mR by the triangle inequality, so every es_* >= 0 in real arithmetic.
 *
 * g2k_sample_scores_f32 (head [3][12]), g2k_fullcov_sample_scores_f32 (chol
 * [24][24]), g2k_mix_sample_scores_f32 (mix [8][608], include/g2k_mix.h): one
 * launch (two when a scene has several workgroups) on the stream, no
 * allocation, capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED, anything
 * else is G2K_EUNSUPPORTED; Nmax in 1..256; workspace >=
 * g2k_sample_scores_workspace_bytes(d) (one size for the three heads; -1 for
 * dims out of range).  S = 0 is a no-op; F = 0 writes out = 0.
 * g2k_sample_scores_geometry: host arithmetic, no HIP call; what the launcher
 * itself computes, out[G2K_SCORES_GEOM_FIELDS]: the pairs of one pass of a
 * workgroup (G), the lanes of a pair (K: one per draw), the frames of a
 * workgroup (FC), the workgroups of a scene (C) and the LDS bytes of the
 * workgroup without the head's own (the per-step head adds 192, the
 * full-covariance head 2304, the mixture head 19376).
 *
 * Alignment (bytes) of g2k_sample_scores_f32, g2k_fullcov_sample_scores_f32
 * and g2k_mix_sample_scores_f32: targets 8, per_ped 16, workspace 4.
 */
#ifndef G2K_SCORES_H_
#define G2K_SCORES_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_SCORES_KMIN 2
#define G2K_SCORES_KMAX 256

#define G2K_SCORES_GEOM_G 0
#define G2K_SCORES_GEOM_LANES 1
#define G2K_SCORES_GEOM_FC 2
#define G2K_SCORES_GEOM_C 3
#define G2K_SCORES_GEOM_LDS_BYTES 4
#define G2K_SCORES_GEOM_FIELDS 5

int64_t g2k_sample_scores_workspace_bytes(const g2k_dims* d);
int g2k_sample_scores_geometry(const g2k_dims* d, int32_t K, int32_t* out);
int g2k_sample_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames,
                          const uint8_t* ped_mask, const float* head, uint64_t seed, int32_t K,
                          float* per_ped, float* out, void* workspace, int64_t workspace_bytes,
                          void* stream);
int g2k_fullcov_sample_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                                  const int32_t* n_active, const int32_t* n_frames,
                                  const uint8_t* ped_mask, const float* chol, uint64_t seed,
                                  int32_t K, float* per_ped, float* out, void* workspace,
                                  int64_t workspace_bytes, void* stream);
int g2k_mix_sample_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                              const int32_t* n_active, const int32_t* n_frames,
                              const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                              float* per_ped, float* out, void* workspace, int64_t workspace_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_SCORES_H_ */
