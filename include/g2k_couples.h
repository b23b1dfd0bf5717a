/*
 * g2k_couples.h — couple-distance scores of a probabilistic head's JOINT
 * samples (added after ABI 11; detect by symbol: g2k_abi_version() stays 11).
 * A header of its own, as include/g2k_kin.h: what a binding looks up by name
 * (multimodaltraj_2_amd/couples.py).  The kernel is csrc/g2k_couples.hip.
 *
 * Every other proper score here is a score of ONE pedestrian's K draws; the
 * joint evaluation's collision count is one threshold of the distribution that
 * matters between pedestrians: the distance between two of them under the
 * head's joint law.  This one scores that distribution without a threshold:
 * per couple of members the fair CRPS and the target's probability-integral-
 * transform (PIT) rank of two features, the closest approach over the 12
 * predicted steps and the final separation, among the K joint draws.  The
 * build's: the reference has no probabilistic head, so PARITY UNPINNED;
 * tests/couples_ref.py restates the definition in float32 NumPy.
 *
 * Inputs, members and joint samples are those of g2k_joint_eval_f32
 * (include/g2k_hip.h): the MEMBERS of scene-frame (s, f), f < n_frames[s], are
 * the columns n < n_active[s] with ped_mask[s][n] != 0, P their number, PP =
 * P (P - 1) / 2 the member couples; joint sample k, k < K, gives every member
 * the bits that the head's sampler (g2k_gauss_sample_f32,
 * g2k_fullcov_sample_f32, g2k_mix_sample_f32) writes for seed (seed + k) mod
 * 2^64.  K in 2..64, B bins in 1..64 with (K + 1) % B == 0.
 *
 * A COUPLE is two members at columns a < b.  For a set of trajectories Z (a
 * joint draw X_k, the targets Y or the mean prediction M = pred), every
 * operation is ONE IEEE fp32 operation, rounded to nearest, in this order, none
 * contracted into an fma:
 *   q_t  = (dx dx) + (dy dy),  dx = Za_x(t) - Zb_x(t), dy likewise    t = 0..11
 *   qmin = min_t q_t           qfin = q_11
 *   smin = sqrt(qmin)          sfin = sqrt(qfin)      correctly rounded
 * This is not g2k_joint_eval_f32's fmaf(dx, dx, dy * dy): a count of qmin <
 * r * r over the draws may differ from its col() in the last bit of q.
 *
 * A couple is SCORED when qmin(M) < reach * reach (one fp32 product); reach is
 * > 0 or +inf, and +inf scores every couple whatever qmin(M) is.  The
 * selection looks at the prediction alone, so the scores stay proper.
 *
 * Per scored couple, for the two features g = min (0), fin (1):
 *   r_g = #{k : q_g(X_k) < q_g(Y)}   in 0..K, an fp32 comparison of the SQUARED
 *                                    values
 *   m_g = 1/K sum_k |s_g(X_k) - s_g(Y)|
 *   p_g = 2/(K (K - 1)) sum_{k<l} |s_g(X_k) - s_g(X_l)|
 *   d_g = 1/K sum_k s_g(X_k)         y_g = s_g(Y)
 * The sums m, p, d in fp32, in no stated order.  The host forms the fair CRPS
 * m_g - p_g / 2.
 *
 * per_couple [S, F, Nmax, Nmax] int32 or NULL: element (a, b) of a scored
 *   couple a < b is 1 + r_min + 256 r_fin; every other element is 0.
 * per_frame_f [S, F, 8] f32 or NULL: the scored couples' sums of m_min, m_fin,
 *   p_min, p_fin, d_min, d_fin, y_min, y_fin.
 * per_frame_i [S, F, 4] int32 or NULL: {scored couples, sum r_min, sum r_fin,
 *   PP}.
 * sums [S, 8] f32, required: the sum over f of per_frame_f, in frame order.
 * hist [S, 2, B] int32, required: row g counts the scene's scored couples' r_g
 *   in bin floor(r B / (K + 1)).
 * tot [S, 4] int64, required: the sum over f of per_frame_i.
 * Every element is written; scene-frames with P < 2 or f >= n_frames[s] and
 * unscored couples contribute exact zeros.  Repeated calls are bit-identical
 * (fixed summation order, no float atomics), and sums / hist / tot do not
 * depend on which optional outputs are NULL.  Columns >= n_active, frames >=
 * n_frames and masked columns of pred and targets are never read.
 *
 * g2k_couple_scores_f32 (head [3][12]), g2k_fullcov_couple_scores_f32 (chol
 * [24][24]), g2k_mix_couple_scores_f32 (mix [8][608], include/g2k_mix.h): two
 * launches on the stream (the workgroups leave rows in the workspace, a second
 * kernel adds them in a fixed order; no workgroup waits for another), no
 * allocation, capturable.  d->flags: 0 or G2K_STEP_TARGETS_SHARED, anything
 * else is G2K_EUNSUPPORTED; Nmax in 1..256; workspace >=
 * g2k_couple_scores_workspace_bytes(d, K, B) (one size for the three heads; -1
 * for dims, K or B out of range).  S = 0 is a no-op; F = 0 writes sums = 0,
 * hist = 0, tot = 0.  The checks run in this order, before any HIP call: d,
 * flags, sizes, K, B, reach, the required pointers, the alignments, the
 * workspace.
 *
 * g2k_couple_scores_geometry: host arithmetic, no HIP call; what the launcher
 * itself computes, out[G2K_COUPLES_GEOM_FIELDS].  A PASS of a workgroup is one
 * tile of TR row members x TC column members of the scene-frame's compacted
 * members (TR = 16 for K <= 22, 8 above; TC = 16), CP = TR TC couples, whose
 * K + 2 items (the draws, the targets, the mean) are made DR = 8 to a round;
 * TILES is the number of tiles that hold a couple when P = Nmax, dealt
 * round-robin to the W workgroups of a scene-frame, PASSES = ceil(TILES / W)
 * the most one of them takes; LDS_BYTES the workgroup's without the head's own
 * (the per-step head adds 192, the full-covariance head 2304, the mixture head
 * 19376, the scene-coupled head of include/g2k_coupled.h 4608: its two
 * transposed factors).
 *
 * Alignment (bytes) of g2k_couple_scores_f32, g2k_fullcov_couple_scores_f32 and
 * g2k_mix_couple_scores_f32: targets 8, per_couple 4, per_frame_f 4,
 * per_frame_i 4, sums 4, hist 4, tot 8, workspace 4.
 */
#ifndef G2K_COUPLES_H_
#define G2K_COUPLES_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_COUPLES_KMIN 2
#define G2K_COUPLES_KMAX 64
#define G2K_COUPLES_BMAX 64
#define G2K_COUPLES_FEATURES 2     /* min: the closest approach; fin: the final separation */
#define G2K_COUPLES_SUMS 8         /* m, p, d, y per feature */
#define G2K_COUPLES_TOT 4          /* scored couples, sum r_min, sum r_fin, PP */

#define G2K_COUPLES_GEOM_TR 0
#define G2K_COUPLES_GEOM_TC 1
#define G2K_COUPLES_GEOM_CP 2
#define G2K_COUPLES_GEOM_DR 3
#define G2K_COUPLES_GEOM_TILES 4
#define G2K_COUPLES_GEOM_W 5
#define G2K_COUPLES_GEOM_PASSES 6
#define G2K_COUPLES_GEOM_LDS_BYTES 7
#define G2K_COUPLES_GEOM_FIELDS 8

int64_t g2k_couple_scores_workspace_bytes(const g2k_dims* d, int32_t K, int32_t B);
int g2k_couple_scores_geometry(const g2k_dims* d, int32_t K, int32_t* out);
int g2k_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                          const float* head, uint64_t seed, int32_t K, int32_t B, float reach,
                          int32_t* per_couple, float* per_frame_f, int32_t* per_frame_i, float* sums,
                          int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                          void* stream);
int g2k_fullcov_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                                  const int32_t* n_active, const int32_t* n_frames,
                                  const uint8_t* ped_mask, const float* chol, uint64_t seed, int32_t K,
                                  int32_t B, float reach, int32_t* per_couple, float* per_frame_f,
                                  int32_t* per_frame_i, float* sums, int32_t* hist, int64_t* tot,
                                  void* workspace, int64_t workspace_bytes, void* stream);
int g2k_mix_couple_scores_f32(const g2k_dims* d, const float* pred, const float* targets,
                              const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                              const float* mix, uint64_t seed, int32_t K, int32_t B, float reach,
                              int32_t* per_couple, float* per_frame_f, int32_t* per_frame_i, float* sums,
                              int32_t* hist, int64_t* tot, void* workspace, int64_t workspace_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_COUPLES_H_ */
