/*
 * g2k_scene_modes.h — k-medoid reduction of a probabilistic head's JOINT
 * samples to M scene modes (added after ABI 11; detect by symbol:
 * g2k_abi_version() stays 11).  A header of its own, as
 * include/g2k_scene_ranks.h: what a binding looks up by name
 * (multimodaltraj_2_amd/scenemodes.py).  The kernel is
 * csrc/g2k_scene_modes.hip.
 *
 * g2k_sample_modes_f32 (include/g2k_modes.h) reduces the K draws of ONE
 * pedestrian to M centres; a mean of joint draws is no coherent scene (a centre
 * between two modes can put two pedestrians on top of each other), so the joint
 * reduction is k-medoids: every mode is one of the K joint draws, named by its
 * draw index — the seed regenerates it, nothing is stored.  The M modes with
 * their probabilities are scored by minJADE_M / minJFDE_M, their Brier
 * variants and a scene-level miss rate.  One definition for every head.  The
 * build's: the reference has no probabilistic head, so PARITY UNPINNED;
 * tests/scene_modes_ref.py restates the definition in float64 NumPy.
 *
 * Inputs, members and joint samples are those of g2k_scene_ranks_f32
 * (include/g2k_scene_ranks.h) and g2k_joint_eval_f32: the MEMBERS of
 * scene-frame (s, f), f < n_frames[s], are the columns n < n_active[s] with
 * ped_mask[s][n] != 0, P their number; joint sample k, k < K, gives every
 * member the bits that the head's sampler writes for seed (seed + k) mod 2^64.
 * M in 1..32, K in max(M, 2)..64, iters in 0..32, miss_radius finite and >= 0.
 * A scene-frame is SCORED when P >= 1 (as g2k_joint_eval_f32: the pair counts
 * agree).
 *
 * The ITEMS of a scored scene-frame are Z_0..Z_{K-1} = the K draws and Z_K = Y,
 * the targets.  Every operation below is one IEEE double operation on the fp32
 * values converted to double (fma(a, b, c) = a b + c rounded once), in this
 * order: members in ascending column, steps ascending, items ascending.
 *   e         per member and step, dx and dy the differences of two items:
 *             e = sqrt(fma(dy, dy, dx dx))
 *   A(j, l)   = A(l, j): acc = 0; per member, per step: acc = acc + e
 *             j < l <= K;  A(j, j) = 0
 *   Fn(k)     acc = 0; per member: acc = acc + (the final step's e between
 *             draw k and Y)
 *   Mx(k)     the maximum over the members of that e
 * Per pair A takes a root per member and step (g2k_scene_ranks_f32 takes one
 * at the end): JADE is a mean of norms.
 *
 * The clustering runs on A restricted to the draws.  Every argmin or argmax
 * takes the lowest index on an exact tie; every sum runs in ascending index
 * from acc = 0 (the term A(j, j) = 0 included).
 *   start (PAM BUILD)   m_0 = argmin_j sum_k A(j, k).  dmin(k) = A(k, m_0).
 *             For i = 1..M-1: m_i = the unchosen j that maximises sum_k max(0,
 *             dmin(k) - A(j, k)); then dmin(k) = min(dmin(k), A(k, m_i)).
 *   rounds    up to iters.  A round assigns every draw k to a(k) = the mode m
 *             with the lowest A(k, med_m) (lowest m on a tie); then the medoid
 *             of each non-empty cluster becomes its member j with the lowest
 *             sum over the cluster's members k of A(j, k).  After the first
 *             round that changes no medoid the rounds stop; `rounds` counts
 *             the rounds run, that one included.
 *   final assignment    a(k) once more; n_m = #{k : a(k) = m}, w_m = n_m / K,
 *             cost = (sum_k A(k, med_a(k))) / (12 K P).
 * Scoring:
 *   J_A(m) = A(med_m, K) / (12 P),  J_F(m) = Fn(med_m) / P
 *   cA = min_m J_A(m), mA the lowest m attaining it; cF, mF from J_F
 *   mx = min_m Mx(med_m); the scene-frame is MISSED when mx > miss_radius: no
 *        mode keeps every member within the radius at the final step
 *   raw = min_{k < M} A(k, K) / (12 P): what M draws give without a reduction
 *   all = min_{k < K} A(k, K) / (12 P): JADE_K, the floor
 * 12 K P, 12 P and P are exact integers converted to double; each quotient is
 * one division.
 *
 * per_frame_i [S, F, 4] int32 or NULL: {P if scored else 0, mA, mF, rounds}.
 * per_frame_d [S, F, 8] f64 or NULL: {cA, cF, w_mA, w_mF, cost, raw, all, mx}.
 * medoids [S, F, M] int32 or NULL: the draw index of each mode.
 * counts [S, F, M] int32 or NULL: n_m.
 * sums [S, 8] f64, required, over the scene's scored frames in frame order
 *   (acc = 0; acc = acc + term): {P cA, P cF, (1 - w_mA)^2, (1 - w_mF)^2,
 *   P cost, P raw, P all, 0}; (1 - w)^2 is t = 1 - w, t t.
 * tot [S, 4] int64, required: {scored frames, sum P, missed frames, sum rounds}.
 * Every element is written; scene-frames with P = 0 or f >= n_frames[s]
 * contribute exact zeros (their rows of medoids and counts are zeros too).
 * Repeated calls are bit-identical (fixed summation order, no float atomics),
 * and sums / tot do not depend on which optional outputs are NULL.  Columns >=
 * n_active, frames >= n_frames and masked columns of pred and targets are never
 * read.
 *
 * g2k_scene_modes_f32 (head [3][12]), g2k_fullcov_scene_modes_f32 (chol
 * [24][24]), g2k_mix_scene_modes_f32 (mix [8][608], include/g2k_mix.h); the
 * scene-coupled head's twin is declared in its own header (bound by
 * multimodaltraj_2_amd/coupled.py).  Two launches on the stream (a workgroup per
 * scene-frame leaves one row in the workspace, a second kernel adds a scene's
 * rows in frame order; no workgroup waits for another), no allocation,
 * capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED, anything else is
 * G2K_EUNSUPPORTED; Nmax in 1..256; workspace >=
 * g2k_scene_modes_workspace_bytes(d, K, M) (one size for every head; -1 for
 * dims, K or M out of range).  S = 0 is a no-op; F = 0 writes sums = 0, tot =
 * 0.  The checks run in this order, before any HIP call: d, flags, sizes, M, K,
 * iters, miss_radius, the required pointers, the alignments, the workspace.
 *
 * g2k_scene_modes_geometry: host arithmetic, no HIP call; what the launcher
 * itself computes, out[G2K_SCENE_MODES_GEOM_FIELDS].  ONE workgroup of 256
 * lanes owns a whole scene-frame, whatever P (W = 1).  It walks the compacted
 * members in TILES of TM (16 for K <= 31, 8 above; TILES = ceil(Nmax / TM) when
 * every column is a member) and makes a tile's K + 1 items once into LDS, DR =
 * 256 / TM items to a round; PAIRS = K (K + 1) / 2 item pairs, dealt APT =
 * ceil(PAIRS / 256) at most to a lane, each a double accumulator kept over the
 * tiles, as are Fn and Mx of draw k in lane k; ROW_BYTES = 88 + 8 M the
 * scene-frame's row in the workspace; LDS_BYTES the workgroup's without the
 * head's own (the per-step head adds 192, the full-covariance head 2304, the
 * mixture head 19376, the scene-coupled head 4608).
 *
 * Alignment (bytes) of g2k_scene_modes_f32, g2k_fullcov_scene_modes_f32 and
 * g2k_mix_scene_modes_f32: targets 8, per_frame_i 4, per_frame_d 8, medoids 4,
 * counts 4, sums 8, tot 8, workspace 8.
 */
#ifndef G2K_SCENE_MODES_H_
#define G2K_SCENE_MODES_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_SCENE_MODES_MMAX 32
#define G2K_SCENE_MODES_KMIN 2
#define G2K_SCENE_MODES_KMAX 64
#define G2K_SCENE_MODES_ITERS_MAX 32
#define G2K_SCENE_MODES_SUMS 8       /* P cA, P cF, (1 - w_mA)^2, (1 - w_mF)^2, P cost, P raw, P all, 0 */
#define G2K_SCENE_MODES_TOT 4        /* scored frames, sum P, missed frames, sum rounds */

#define G2K_SCENE_MODES_GEOM_TM 0
#define G2K_SCENE_MODES_GEOM_DR 1
#define G2K_SCENE_MODES_GEOM_TILES 2
#define G2K_SCENE_MODES_GEOM_W 3
#define G2K_SCENE_MODES_GEOM_PAIRS 4
#define G2K_SCENE_MODES_GEOM_APT 5
#define G2K_SCENE_MODES_GEOM_ROW_BYTES 6
#define G2K_SCENE_MODES_GEOM_LDS_BYTES 7
#define G2K_SCENE_MODES_GEOM_FIELDS 8

int64_t g2k_scene_modes_workspace_bytes(const g2k_dims* d, int32_t K, int32_t M);
int g2k_scene_modes_geometry(const g2k_dims* d, int32_t K, int32_t M, int32_t* out);
int g2k_scene_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* head, uint64_t seed, int32_t K, int32_t M, int32_t iters,
                        float miss_radius, int32_t* per_frame_i, double* per_frame_d, int32_t* medoids,
                        int32_t* counts, double* sums, int64_t* tot, void* workspace,
                        int64_t workspace_bytes, void* stream);
int g2k_fullcov_scene_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                                const int32_t* n_active, const int32_t* n_frames,
                                const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                                int32_t M, int32_t iters, float miss_radius, int32_t* per_frame_i,
                                double* per_frame_d, int32_t* medoids, int32_t* counts, double* sums,
                                int64_t* tot, void* workspace, int64_t workspace_bytes, void* stream);
int g2k_mix_scene_modes_f32(const g2k_dims* d, const float* pred, const float* targets,
                            const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                            const float* mix, uint64_t seed, int32_t K, int32_t M, int32_t iters,
                            float miss_radius, int32_t* per_frame_i, double* per_frame_d,
                            int32_t* medoids, int32_t* counts, double* sums, int64_t* tot,
                            void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_SCENE_MODES_H_ */
