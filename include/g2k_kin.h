/*
 * g2k_kin.h — kinematic scores of a probabilistic head's samples (added after
 * ABI 11; detect by symbol: g2k_abi_version() stays 11).  A header of its own,
 * as include/g2k_ranks.h: what a binding looks up by name
 * (multimodaltraj_2_amd/kin.py).  The kernel is csrc/g2k_kin.hip.
 *
 * The evaluations so far compare positions.  What the heads differ in is how a
 * drawn pedestrian MOVES: how fast it walks, how hard it accelerates from one
 * 0.4 s step to the next, how straight its path is.  This one scores 32 scalar
 * features of a trajectory, in the dataset's units per step: the fair CRPS (the
 * 1-D energy score, strictly proper) and the target's probability-integral-
 * transform (PIT) rank among the K draws, which is uniform on 0..K when the
 * target follows the head's law — no bandwidth, no degenerate case.  The
 * build's: the reference has no probabilistic head, so PARITY UNPINNED;
 * tests/kin_ref.py restates the definition in float32 NumPy.
 *
 * Inputs, pairs and draws are those of g2k_best_of_k_f32 (include/g2k_hip.h),
 * K in 2..255, B bins in 1..64 with (K + 1) % B == 0.  Draw k, k < K, of a pair
 * (s, f, n) is bit for bit what the head's sampler (g2k_gauss_sample_f32,
 * g2k_fullcov_sample_f32, g2k_mix_sample_f32) writes for seed (seed + k) mod
 * 2^64.
 *
 * The features of a trajectory Z (a draw X_k or the target Y) of 12 fp32
 * positions.  Every operation is ONE IEEE fp32 operation, rounded to nearest,
 * in this order, none contracted into an fma:
 *   v_t = (Zx(t+1) - Zx(t), Zy(t+1) - Zy(t))                       t = 0..10
 *   s_t = sqrt(vx vx + vy vy)    speed: two products, one add,     t = 0..10
 *                                one correctly rounded square root  rows 0..10
 *   a_t = sqrt(wx wx + wy wy), w = v_(t+1) - v_t   acceleration     t = 0..9
 *                                                                   rows 11..20
 *   l_t = s_(t+1) - s_t          longitudinal acceleration          t = 0..9
 *                                                                   rows 21..30
 *   st  = net / len              straightness                       row 31
 *         len = ((s_0 + s_1) + s_2) + ... + s_10
 *         net = the speed recipe applied to Z(11) - Z(0)
 *         the division correctly rounded; st = 1 when len == 0
 * The four groups g: speed (n_g = 11 rows), acc (10), lacc (10), straight (1).
 *
 * Per pair, x_kj draw k's feature j and y_j the target's:
 *   r_j = #{k : x_kj < y_j}  in 0..K, a comparison of fp32 values
 *   m_g = 1/(K n_g) sum_k sum_{j in g} |x_kj - y_j|
 *   p_g = 2/(K (K - 1) n_g) sum_{k<l} sum_{j in g} |x_kj - x_lj|
 *   d_g = 1/(K n_g) sum_k sum_{j in g} x_kj        the draws' mean feature
 *   y_g = 1/n_g sum_{j in g} y_j                   the target's
 * The sums m, p, d, y in fp32, in no stated order (fma allowed).  The host
 * forms crps_g = m_g - p_g / 2, the fair CRPS averaged over the group's rows.
 *
 * per_ped [S, F, Nmax, 48] f32 or NULL, per pair: columns 0..31 the ranks r_j
 *   as floats, 32..35 m_g, 36..39 p_g, 40..43 d_g, 44..47 y_g.
 * sums [S, 16] f32, required: the sums of columns 32..47 over the scene's pairs.
 *   Fixed summation order, no atomics.
 * hist [S, 32, B] int32, required: row j counts the scene's pairs' r_j in bin
 *   floor(r B / (K + 1)).
 * tot [S, 8] int64, required: pairs, the sum of r_j over the rows of speed,
 *   acc, lacc, straight, then 0, 0, 0.
 * Every element is written; non-pairs are exactly zero.  Repeated calls are
 * bit-identical, and sums / hist / tot do not depend on whether per_ped is
 * NULL.  Columns >= n_active, frames >= n_frames and masked columns of pred and
 * targets are never read.
 *
 * g2k_sample_kin_f32 (head [3][12]), g2k_fullcov_sample_kin_f32 (chol
 * [24][24]), g2k_mix_sample_kin_f32 (mix [8][608], include/g2k_mix.h): one
 * launch (two when a scene has several workgroups) on the stream, no
 * allocation, capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED, anything
 * else is G2K_EUNSUPPORTED; Nmax in 1..256; workspace >=
 * g2k_sample_kin_workspace_bytes(d, B) (one size for the three heads; -1 for
 * dims or B out of range).  S = 0 is a no-op; F = 0 writes sums = 0, hist = 0,
 * tot = 0.  g2k_sample_kin_geometry: host arithmetic, no HIP call; what the
 * launcher itself computes, out[G2K_KIN_GEOM_FIELDS], the five fields of
 * include/g2k_scores.h: the pairs of one pass of a workgroup (G), the lanes of
 * a pair (K: one per draw), the frames of a workgroup (FC), the workgroups of a
 * scene (C) and the LDS bytes of the workgroup without the head's own (the
 * per-step head adds 192, the full-covariance head 2304, the mixture head
 * 19376).
 *
 * Alignment (bytes) of g2k_sample_kin_f32, g2k_fullcov_sample_kin_f32 and
 * g2k_mix_sample_kin_f32: targets 8, per_ped 16, sums 4, hist 4, tot 8,
 * workspace 8.
 */
#ifndef G2K_KIN_H_
#define G2K_KIN_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_KIN_KMIN 2
#define G2K_KIN_KMAX 255
#define G2K_KIN_BMAX 64
#define G2K_KIN_ROWS 32        /* the features: 11 speeds, 10 acc, 10 lacc, straightness */
#define G2K_KIN_GROUPS 4
#define G2K_KIN_COLS 48        /* per_ped: the ranks, then m, p, d, y per group */

#define G2K_KIN_GEOM_G 0
#define G2K_KIN_GEOM_LANES 1
#define G2K_KIN_GEOM_FC 2
#define G2K_KIN_GEOM_C 3
#define G2K_KIN_GEOM_LDS_BYTES 4
#define G2K_KIN_GEOM_FIELDS 5

int64_t g2k_sample_kin_workspace_bytes(const g2k_dims* d, int32_t B);
int g2k_sample_kin_geometry(const g2k_dims* d, int32_t K, int32_t* out);
int g2k_sample_kin_f32(const g2k_dims* d, const float* pred, const float* targets,
                       const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                       const float* head, uint64_t seed, int32_t K, int32_t B, float* per_ped,
                       float* sums, int32_t* hist, int64_t* tot, void* workspace,
                       int64_t workspace_bytes, void* stream);
int g2k_fullcov_sample_kin_f32(const g2k_dims* d, const float* pred, const float* targets,
                               const int32_t* n_active, const int32_t* n_frames,
                               const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                               int32_t B, float* per_ped, float* sums, int32_t* hist, int64_t* tot,
                               void* workspace, int64_t workspace_bytes, void* stream);
int g2k_mix_sample_kin_f32(const g2k_dims* d, const float* pred, const float* targets,
                           const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                           const float* mix, uint64_t seed, int32_t K, int32_t B, float* per_ped,
                           float* sums, int32_t* hist, int64_t* tot, void* workspace,
                           int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_KIN_H_ */
