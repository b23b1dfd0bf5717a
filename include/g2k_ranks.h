/*
 * g2k_ranks.h — rank-histogram calibration of a probabilistic head's samples
 * (added after ABI 11; detect by symbol: g2k_abi_version() stays 11).  A header
 * of its own, as include/g2k_scores.h: what a binding looks up by name
 * (multimodaltraj_2_amd/ranks.py).  The kernel is csrc/g2k_ranks.hip.
 *
 * The multivariate rank histogram (Gneiting et al. 2008): the target pooled
 * with the K draws, a scalar pre-rank per point that says how typical the point
 * is among the other K, and the target's rank among the K + 1 pre-ranks.  When
 * the target comes from the law of the draws the K + 1 points are exchangeable
 * and the rank is uniform on 0..K, whatever the law: one definition for the
 * per-step head, the full-covariance head and the mixture head alike.  The
 * build's: the reference has no probabilistic head, so PARITY UNPINNED;
 * tests/ranks_ref.py restates the definition in float64 NumPy.
 *
 * Inputs, pairs and draws are those of g2k_best_of_k_f32 (include/g2k_hip.h),
 * K in 4..255, B bins in 1..64 with (K + 1) % B == 0.  Draw k, k < K, of a pair
 * (s, f, n) is bit for bit what the head's sampler (g2k_gauss_sample_f32,
 * g2k_fullcov_sample_f32, g2k_mix_sample_f32) writes for seed (seed + k) mod
 * 2^64.
 *
 * For a pair the pooled set is Z = {Y, X_0, ..., X_{K-1}}: the target and the
 * K draws, K + 1 trajectories of 12 2-D positions.
 *
 * Per step t, the density pre-rank:
 *   c_t      = sample covariance of the K + 1 positions Z(t), divisor K
 *   H_t      = (K + 1)^(-1/3) c_t     (Scott's rule as g2k_kde_nll_f32's, on the
 *                                      pooled set: the points stay exchangeable)
 *   rho_t(z) = sum over the OTHER K points z' of exp(-1/2 (z - z')^T H_t^-1 (z - z'))
 *   r_t      = #{k : rho_t(X_k) > rho_t(Y)}  in 0..K; 0: the target is the most
 *              typical point, K: the most outlying
 * A step whose det H_t is not a positive finite number is DEGENERATE: r_t = -1,
 * it enters no histogram and is counted.  The quadratic forms, their exp and the
 * sums rho in fp32; the moments, the bandwidth and the inverse of its Cholesky
 * factor in double (the inverse's three entries rounded to fp32).  Unlike
 * g2k_kde_nll_f32 the moments are summed in double: a rank compares two sums,
 * and fp32 moments leave them 1e-4 apart from the definition where the pooled
 * points are nearly collinear.  The moments are centred as the head's KDE-NLL
 * centres them (sums of z - mu for the per-step and the full-covariance head, a
 * running mean for the mixture head, whose draws sit far from mu).
 *
 * Per trajectory, the energy pre-rank:
 *   rho_traj(z) = sum over the other K points of ||z - z'||_2 over the 24 coordinates
 *   r_traj      = #{k : rho_traj(X_k) < rho_traj(Y)}
 * No bandwidth: never degenerate.
 *
 * per_ped [S, F, Nmax, 16] f32 or NULL, per pair: r_0 .. r_11, r_traj, the
 *   pair's degenerate steps, 0, 0.
 * hist [S, 13, B] int32, required: row t < 12 counts the scene's pairs'
 *   non-degenerate r_t in bin floor(r B / (K + 1)), row 12 the same with r_traj.
 * tot [S, 4] int64, required: pairs, degenerate steps, sum of r_t over the
 *   non-degenerate steps, sum of r_traj.
 * Every element is written; non-pairs are exactly zero.  No float is
 * accumulated across pairs: repeated calls are bit-identical, and hist / tot do
 * not depend on whether per_ped is NULL.  Columns >= n_active, frames >=
 * n_frames and masked columns of pred and targets are never read.
 *
 * g2k_sample_ranks_f32 (head [3][12]), g2k_fullcov_sample_ranks_f32 (chol
 * [24][24]), g2k_mix_sample_ranks_f32 (mix [8][608], include/g2k_mix.h): one
 * launch (two when a scene has several workgroups) on the stream, no
 * allocation, capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED, anything
 * else is G2K_EUNSUPPORTED; Nmax in 1..256; workspace >=
 * g2k_sample_ranks_workspace_bytes(d, B) (one size for the three heads; -1 for
 * dims or B out of range).  S = 0 is a no-op; F = 0 writes hist = 0, tot = 0.
 * g2k_sample_ranks_geometry: host arithmetic, no HIP call; what the launcher
 * itself computes, out[G2K_RANKS_GEOM_FIELDS]: the pairs of one pass of a
 * workgroup (G), the lanes of a pair (K: one per draw), the frames of a
 * workgroup (FC), the workgroups of a scene (C) and the LDS bytes of the
 * workgroup without the head's own (the per-step head adds 192, the
 * full-covariance head 2304, the mixture head 19376).
 *
 * Alignment (bytes) of g2k_sample_ranks_f32, g2k_fullcov_sample_ranks_f32
 * and g2k_mix_sample_ranks_f32: targets 8, per_ped 16, hist 4, tot 8,
 * workspace 8.
 */
#ifndef G2K_RANKS_H_
#define G2K_RANKS_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_RANKS_KMIN 4
#define G2K_RANKS_KMAX 255
#define G2K_RANKS_BMAX 64
#define G2K_RANKS_ROWS 13      /* the rows of hist: 12 steps and the trajectory */

#define G2K_RANKS_GEOM_G 0
#define G2K_RANKS_GEOM_LANES 1
#define G2K_RANKS_GEOM_FC 2
#define G2K_RANKS_GEOM_C 3
#define G2K_RANKS_GEOM_LDS_BYTES 4
#define G2K_RANKS_GEOM_FIELDS 5

int64_t g2k_sample_ranks_workspace_bytes(const g2k_dims* d, int32_t B);
int g2k_sample_ranks_geometry(const g2k_dims* d, int32_t K, int32_t* out);
int g2k_sample_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                         const int32_t* n_active, const int32_t* n_frames,
                         const uint8_t* ped_mask, const float* head, uint64_t seed, int32_t K,
                         int32_t B, float* per_ped, int32_t* hist, int64_t* tot, void* workspace,
                         int64_t workspace_bytes, void* stream);
int g2k_fullcov_sample_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                                 const int32_t* n_active, const int32_t* n_frames,
                                 const uint8_t* ped_mask, const float* chol, uint64_t seed,
                                 int32_t K, int32_t B, float* per_ped, int32_t* hist, int64_t* tot,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int g2k_mix_sample_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                             const int32_t* n_active, const int32_t* n_frames,
                             const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                             int32_t B, float* per_ped, int32_t* hist, int64_t* tot, void* workspace,
                             int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_RANKS_H_ */
