/*
 * g2k_scene_ranks.h — scene-level rank calibration of a probabilistic head's
 * JOINT samples (added after ABI 11; detect by symbol: g2k_abi_version() stays
 * 11).  A header of its own, as include/g2k_couples.h: what a binding looks up
 * by name (multimodaltraj_2_amd/sceneranks.py).  The kernel is
 * csrc/g2k_scene_ranks.hip.
 *
 * g2k_sample_ranks_f32 (include/g2k_ranks.h) ranks ONE pedestrian's target
 * among that pedestrian's K draws, so it cannot see dependence between
 * pedestrians; g2k_couple_scores_f32 sees two members at a time, and only
 * their distance.  This one is the multivariate rank histogram (Gneiting et
 * al. 2008) of a whole scene-frame: the targets' configuration is pooled with
 * the K joint draws and ranked among them by three pre-rank functions (Allen,
 * Ziegel and Ginsbourger 2023) chosen so that the histogram's shape says what
 * is wrong — typicality, common mode, within-scene spread — and the same
 * distance matrix gives the two terms of the fair energy score of the scene's
 * joint law.  One definition for every head.  The build's: the reference has
 * no probabilistic head, so PARITY UNPINNED; tests/scene_ranks_ref.py restates
 * the definition in float64 NumPy.
 *
 * Inputs, members and joint samples are those of g2k_couple_scores_f32
 * (include/g2k_couples.h): the MEMBERS of scene-frame (s, f), f < n_frames[s],
 * are the columns n < n_active[s] with ped_mask[s][n] != 0, P their number;
 * joint sample k, k < K, gives every member the bits that the head's sampler
 * (g2k_gauss_sample_f32, g2k_fullcov_sample_f32, g2k_mix_sample_f32) writes for
 * seed (seed + k) mod 2^64.  K in 2..64, B bins in 1..64 with (K + 1) % B == 0.
 * A scene-frame is SCORED when P >= 2.
 *
 * The pooled ITEMS of a scored scene-frame are Z_0..Z_{K-1} = the K draws and
 * Z_K = Y, the targets; each is P x 24 fp32 values (member i's coordinate c =
 * 2 t + x/y, time-major).  Every operation below is one IEEE double operation
 * on the fp32 values converted to double (fma(a, b, c) = a b + c rounded
 * once), in this order: members in ascending column, a member's coordinates
 * ascending, items ascending.
 *   D2(j, l)  acc = 0; per member, per coordinate: d = Z_j - Z_l,
 *             acc = fma(d, d, acc)                               j < l <= K
 *   D(j, l)   = D(l, j) = sqrt(D2(j, l))
 *   t_j       typicality: acc = 0; acc = acc + D(j, l), l = 0..K, l != j
 *   r         = Z - pred, the residual (one subtraction)
 *   s_j[c]    acc = 0; per member: acc = acc + r[c]              c = 0..23
 *   q_j       acc = 0; per member, per coordinate: acc = fma(r, r, acc)
 *   loc_j     common mode: acc = 0; acc = fma(s_j[c], s_j[c], acc), c = 0..23;
 *             loc_j = acc / P
 *   spr_j     within-scene spread: q_j - loc_j (the within-scene sum of
 *             squares; the formula as written is the definition)
 *   r_g       = #{k < K : g_k < g_K}  for g = typ (t), loc, spr: in 0..K, a
 *             strict comparison of doubles; exact ties arise only for a
 *             degenerate head and are not special-cased
 *   m         = t_K / K           (= 1/K sum_k D(k, K))
 *   p         = 2 u / (K (K - 1)), u: acc = 0; acc = acc + u_l, l = 1..K-1,
 *             u_l: acc = 0; acc = acc + D(k, l), k = 0..l-1
 *             (= 2/(K (K - 1)) sum_{k<l<K} D(k, l))
 *   mean_k g_k: acc = 0; acc = acc + g_k, k = 0..K-1; acc / K
 * The host forms the fair energy score m - p / 2.  Distances are taken as
 * differences, not through a Gram identity.
 *
 * per_frame_i [S, F, 4] int32 or NULL: {P if scored else 0, r_typ, r_loc,
 *   r_spr}.
 * per_frame_d [S, F, 6] f64 or NULL: {m, p, mean_k loc_k, loc_K, mean_k spr_k,
 *   spr_K}.
 * sums [S, 6] f64, required: the sum over f of per_frame_d, in frame order.
 * hist [S, 3, B] int32, required: row g counts the scene's scored
 *   scene-frames' r_g in bin floor(r B / (K + 1)).
 * tot [S, 4] int64, required: {scored scene-frames, sum r_typ, sum r_loc, sum
 *   r_spr}.
 * Every element is written; scene-frames with P < 2 or f >= n_frames[s]
 * contribute exact zeros.  Repeated calls are bit-identical (fixed summation
 * order, no float atomics), and sums / hist / tot do not depend on which
 * optional outputs are NULL.  Columns >= n_active, frames >= n_frames and
 * masked columns of pred and targets are never read.
 *
 * g2k_scene_ranks_f32 (head [3][12]), g2k_fullcov_scene_ranks_f32 (chol
 * [24][24]), g2k_mix_scene_ranks_f32 (mix [8][608], include/g2k_mix.h); the
 * scene-coupled head's twin is declared in include/g2k_coupled.h (bound by
 * multimodaltraj_2_amd/coupled.py).  Two launches on the stream (a workgroup per
 * scene-frame leaves one row in the workspace, a second kernel adds a scene's
 * rows in frame order; no workgroup waits for another), no allocation,
 * capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED, anything else is
 * G2K_EUNSUPPORTED; Nmax in 1..256; workspace >=
 * g2k_scene_ranks_workspace_bytes(d, K, B) (one size for every head; -1 for
 * dims, K or B out of range).  S = 0 is a no-op; F = 0 writes sums = 0, hist =
 * 0, tot = 0.  The checks run in this order, before any HIP call: d, flags,
 * sizes, K, B, the required pointers, the alignments, the workspace.
 *
 * g2k_scene_ranks_geometry: host arithmetic, no HIP call; what the launcher
 * itself computes, out[G2K_SCENE_RANKS_GEOM_FIELDS].  ONE workgroup of 256
 * lanes owns a whole scene-frame, whatever P (W = 1: a rank needs every
 * member).  It walks the compacted members in TILES of TM (16 for K <= 31, 8
 * above; TILES = ceil(Nmax / TM) when every column is a member) and makes a
 * tile's K + 1 items once into LDS, DR = 256 / TM items to a round; PAIRS =
 * K (K + 1) / 2 item pairs, dealt APT = ceil(PAIRS / 256) at most to a lane,
 * each a double accumulator kept over the tiles, as are the 25 (K + 1) sums s
 * and q, AFT = ceil(25 (K + 1) / 256) at most to a lane; LDS_BYTES the
 * workgroup's without the head's own (the per-step head adds 192, the
 * full-covariance head 2304, the mixture head 19376, the scene-coupled head
 * 4608).
 *
 * Alignment (bytes) of g2k_scene_ranks_f32, g2k_fullcov_scene_ranks_f32 and
 * g2k_mix_scene_ranks_f32: targets 8, per_frame_i 4, per_frame_d 8, sums 8,
 * hist 4, tot 8, workspace 8.
 */
#ifndef G2K_SCENE_RANKS_H_
#define G2K_SCENE_RANKS_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_SCENE_RANKS_KMIN 2
#define G2K_SCENE_RANKS_KMAX 64
#define G2K_SCENE_RANKS_BMAX 64
#define G2K_SCENE_RANKS_FEATURES 3   /* typ: typicality; loc: common mode; spr: within-scene spread */
#define G2K_SCENE_RANKS_SUMS 6       /* m, p, mean_k loc_k, loc_K, mean_k spr_k, spr_K */
#define G2K_SCENE_RANKS_TOT 4        /* scored scene-frames, sum r_typ, sum r_loc, sum r_spr */

#define G2K_SCENE_RANKS_GEOM_TM 0
#define G2K_SCENE_RANKS_GEOM_DR 1
#define G2K_SCENE_RANKS_GEOM_TILES 2
#define G2K_SCENE_RANKS_GEOM_W 3
#define G2K_SCENE_RANKS_GEOM_PAIRS 4
#define G2K_SCENE_RANKS_GEOM_APT 5
#define G2K_SCENE_RANKS_GEOM_AFT 6
#define G2K_SCENE_RANKS_GEOM_LDS_BYTES 7
#define G2K_SCENE_RANKS_GEOM_FIELDS 8

int64_t g2k_scene_ranks_workspace_bytes(const g2k_dims* d, int32_t K, int32_t B);
int g2k_scene_ranks_geometry(const g2k_dims* d, int32_t K, int32_t* out);
int g2k_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* head, uint64_t seed, int32_t K, int32_t B, int32_t* per_frame_i,
                        double* per_frame_d, double* sums, int32_t* hist, int64_t* tot, void* workspace,
                        int64_t workspace_bytes, void* stream);
int g2k_fullcov_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                                const int32_t* n_active, const int32_t* n_frames,
                                const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                                int32_t B, int32_t* per_frame_i, double* per_frame_d, double* sums,
                                int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                                void* stream);
int g2k_mix_scene_ranks_f32(const g2k_dims* d, const float* pred, const float* targets,
                            const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                            const float* mix, uint64_t seed, int32_t K, int32_t B, int32_t* per_frame_i,
                            double* per_frame_d, double* sums, int32_t* hist, int64_t* tot,
                            void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_SCENE_RANKS_H_ */
