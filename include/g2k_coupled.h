/*
 * g2k_coupled.h — the scene-coupled trajectory head (added after ABI 11; detect
 * by symbol: g2k_abi_version() stays 11).  A header of its own, as
 * include/g2k_couples.h: what a binding looks up by name
 * (multimodaltraj_2_amd/coupled.py).  The stats and the sampler are
 * csrc/g2k_coupled.hip; the two fused evaluations are the kernels of
 * csrc/g2k_joint.hip and csrc/g2k_couples.hip with this head's draw policy
 * (CoupledHead, csrc/g2k_head_draw.h).
 *
 * The other heads draw every pedestrian of a scene-frame independently.  This
 * one is the Gaussian whose joint draws share a part: over the 24-vector
 * residuals r (time-major, i = 2 t + c, as the full-covariance head's)
 *   r_gi = c_g + e_gi,   c_g ~ N(0, B) one per GROUP,   e_gi ~ N(0, W) one per
 *   member
 * a group being a scene-frame (s, f), f < n_frames[s], its members those of
 * g2k_joint_eval_f32 (include/g2k_hip.h: the columns n < n_active[s] with
 * ped_mask[s][n] != 0), P their number.  A member's marginal is N(0, W + B), a
 * full-covariance head; B = 0 is that head itself.  The build's: the reference
 * has no probabilistic head, so PARITY UNPINNED; tests/coupled_ref.py restates
 * the definition in float64 NumPy.
 *
 * cpl [2][24][24] f32 row-major = {Lw, Lb}, the lower Cholesky factors of W and
 * B; entries above the diagonal are never read; Lw's diagonal > 0 (the
 * caller's contract), Lb may be all zero.
 *
 * The draw.  z[2t], z[2t+1] are the member's normals, those of
 * g2k_fullcov_sample_f32 for element e = ((s F + f) 12 + t) Nmax + n and seed
 * (seed + k) mod 2^64.  zc[2t], zc[2t+1] are the scene-frame's: the pair the
 * same generator forms for column 0's element ((s F + f) 12 + t) Nmax under
 * seed ((seed + k) mod 2^64) XOR G2K_COUPLED_SALT.  The salt's top bit is set
 * and its low 13 bits are clear: x XOR salt differs from x by a non-zero
 * multiple of 2^13 modulo 2^64, so no salted seed is one of the K <= 4096
 * member seeds seed .. seed + K - 1, whatever seed is.
 *   c[i] = sum_{j <= i} Lb[i][j] zc[j]   acc = 0; acc = fmaf(Lb[i][j], zc[j], acc), ascending j
 *   x[i] = (mu[i] + c[i]) + sum_{j <= i} Lw[i][j] z[j]
 *                                        acc = mu[i] + c[i] (one fp32 add);
 *                                        acc = fmaf(Lw[i][j], z[j], acc), ascending j
 * With Lb = 0 the bits are g2k_fullcov_sample_f32's with chol = Lw.
 *
 * g2k_coupled_sample_f32: out [S, F, 24, Nmax] in band layout (out[c 12 + t] =
 * x[2t + c]) holds one draw per (s, f, n), every element written.  The checks
 * run in this order, before any HIP call: d, flags (G2K_STEP_PRED_PED_MAJOR is
 * G2K_EUNSUPPORTED), sizes (Nmax in 1..256), the required pointers (pred, cpl,
 * out).  S F = 0 is a no-op.
 *
 * g2k_coupled_stats_f32: one pass over pred and targets, r = targets - pred in
 * double (exact: both are f32), every sum in double.  N is the number of
 * members over all groups, G the number of groups with P >= 1, rbar_g a
 * group's mean.
 *   within [24][24]  = SSW = sum_g sum_i (r_gi - rbar_g)(r_gi - rbar_g)^T,
 *     summed from the centred residuals
 *   between [24][24] = SSB = sum_g P_g rbar_g rbar_g^T
 *   counts [4] int64 = {N, G, groups with P >= 2, sum_g P_g^2}
 *   stats [6]: with whiten [25][24] doubles (rows 0..23 = A with A W A^T = I
 *     and A B A^T = diag(lambda), row 24 = lambda >= 0), y = A r,
 *       q_within  = sum_g sum_i sum_d (y_id - ybar_d)^2
 *       q_between = sum_g sum_d P ybar_d^2 / (1 + P lambda_d)
 *       logs      = sum_g sum_d log(1 + P lambda_d)
 *     stats = {(q_within + q_between + logs) / 2: the groups' joint NLL without
 *     its constant N (12 log 2 pi + log det Lw);  1/2 sum_g sum_i sum_d [y_id^2
 *     / (1 + lambda_d) + log(1 + lambda_d)]: the NLL of the independent head
 *     with the same marginals, without the same constant;  q_within;
 *     q_between;  logs;  0}.  Without whiten (NULL) stats is exact zeros.
 * Both matrices are written in full (symmetric).  Every element of the four
 * outputs is written on every call with S >= 1 (F = 0: zeros).  Non-members,
 * columns >= n_active and frames >= n_frames of pred and targets are never
 * read.  A workgroup takes a contiguous range of whole scene-frames and leaves
 * one row in the workspace; a second kernel adds the rows in row order (one
 * workgroup covers a small launch and writes the outputs itself: no workspace,
 * one kernel).  No atomics, a fixed summation order: repeated calls are
 * bit-identical, and the bits of within, between and counts do not depend on
 * whiten.  No allocation, capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED,
 * anything else is G2K_EUNSUPPORTED; Nmax in 1..256, S F < 2^31; workspace >=
 * g2k_coupled_stats_workspace_bytes(d) (-1 for dims out of range).  S = 0 is a
 * no-op.  The checks run in this order, before any HIP call: d, flags, sizes,
 * the required pointers (pred, targets, n_active, within, between, counts,
 * stats), the alignments, the workspace.
 *
 * g2k_coupled_joint_eval_f32 and g2k_coupled_couple_scores_f32: the arguments,
 * outputs, checks and workspace queries of g2k_fullcov_joint_eval_f32
 * (include/g2k_hip.h) and g2k_fullcov_couple_scores_f32
 * (include/g2k_couples.h) with cpl in place of chol; joint sample k gives every
 * member the bits g2k_coupled_sample_f32 writes for seed (seed + k) mod 2^64.
 * The workspaces are those of the twins
 * (g2k_coupled_joint_eval_workspace_bytes equals
 * g2k_fullcov_joint_eval_workspace_bytes; g2k_couple_scores_workspace_bytes is
 * one size for every head).  The per-pedestrian evaluations have no
 * coupled twin: one member's law is N(mu, W + B), so those figures are a
 * full-covariance head's with chol(W + B).
 *
 * g2k_coupled_scene_ranks_f32: the arguments, outputs, checks and workspace
 * query of g2k_fullcov_scene_ranks_f32 (include/g2k_scene_ranks.h;
 * g2k_scene_ranks_workspace_bytes is one size for every head) with cpl in
 * place of chol, over the same joint samples: the scene-level rank calibration
 * is the figure that says whether the coupling is too weak or too strong.
 *
 * g2k_coupled_scene_modes_f32: the arguments, outputs, checks and workspace
 * query of g2k_fullcov_scene_modes_f32 (include/g2k_scene_modes.h;
 * g2k_scene_modes_workspace_bytes is one size for every head) with cpl in
 * place of chol, over the same joint samples: the k-medoid reduction of the K
 * joint draws to M scene modes, where a shared part lets a few draws cover a
 * scene whose pedestrians move together.
 *
 * Alignment (bytes).  g2k_coupled_stats_f32: targets 8, whiten 8, within 8,
 * between 8, counts 8, stats 8, workspace 8.  g2k_coupled_sample_f32: pred 4,
 * cpl 4, out 4.  g2k_coupled_joint_eval_f32: targets 8, sums_i 8, workspace 4.
 * g2k_coupled_couple_scores_f32: targets 8, per_couple 4, per_frame_f 4,
 * per_frame_i 4, sums 4, hist 4, tot 8, workspace 4.
 * g2k_coupled_scene_ranks_f32: targets 8, per_frame_i 4, per_frame_d 8, sums 8,
 * hist 4, tot 8, workspace 8.  g2k_coupled_scene_modes_f32: targets 8,
 * per_frame_i 4, per_frame_d 8, medoids 4, counts 4, sums 8, tot 8, workspace 8.
 */
#ifndef G2K_COUPLED_H_
#define G2K_COUPLED_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_COUPLED_SALT 0x9E3779B97F4A6000ull
#define G2K_COUPLED_DIM 24
#define G2K_COUPLED_COUNTS 4       /* N, G, groups with P >= 2, sum P^2 */
#define G2K_COUPLED_STATS 6

int64_t g2k_coupled_stats_workspace_bytes(const g2k_dims* d);
int g2k_coupled_stats_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                          const double* whiten, double* within, double* between, int64_t* counts,
                          double* stats, void* workspace, int64_t workspace_bytes, void* stream);
int g2k_coupled_sample_f32(const g2k_dims* d, const float* pred, const float* cpl, uint64_t seed,
                           float* out, void* stream);
int64_t g2k_coupled_joint_eval_workspace_bytes(const g2k_dims* d);
int g2k_coupled_joint_eval_f32(const g2k_dims* d, const float* pred, const float* targets,
                               const int32_t* n_active, const int32_t* n_frames,
                               const uint8_t* ped_mask, const float* cpl, uint64_t seed, int32_t K,
                               float radius, float* per_frame_f, int32_t* per_frame_i, float* sums_f,
                               int64_t* sums_i, void* workspace, int64_t workspace_bytes, void* stream);
int g2k_coupled_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                                  const int32_t* n_active, const int32_t* n_frames,
                                  const uint8_t* ped_mask, const float* cpl, uint64_t seed, int32_t K,
                                  int32_t B, float reach, int32_t* per_couple, float* per_frame_f,
                                  int32_t* per_frame_i, float* sums, int32_t* hist, int64_t* tot,
                                  void* workspace, int64_t workspace_bytes, void* stream);
int g2k_coupled_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                                const int32_t* n_active, const int32_t* n_frames,
                                const uint8_t* ped_mask, const float* cpl, uint64_t seed, int32_t K,
                                int32_t B, int32_t* per_frame_i, double* per_frame_d, double* sums,
                                int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                                void* stream);
int g2k_coupled_scene_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                                const int32_t* n_active, const int32_t* n_frames,
                                const uint8_t* ped_mask, const float* cpl, uint64_t seed, int32_t K,
                                int32_t M, int32_t iters, float miss_radius, int32_t* per_frame_i,
                                double* per_frame_d, int32_t* medoids, int32_t* counts, double* sums,
                                int64_t* tot, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_COUPLED_H_ */
