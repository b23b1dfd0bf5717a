/*
 * g2k_mix.h — the Gaussian-mixture trajectory head of libg2k_hip.so (added
 * after ABI 11; detect by symbol: g2k_abi_version() stays 11).  A header of
 * its own: include/g2k_hip.h declares the versioned ABI, this one what a
 * binding looks up by name (multimodaltraj_2_amd/mixture.py).
 *
 * A mixture of up to 8 full-covariance Gaussians over a pair's 24 residuals.
 * The build's: the reference has no probabilistic head, so PARITY UNPINNED;
 * tests/mixture_ref.py restates the definition in float64 NumPy.
 *
 * Pairs, pred, targets, n_active, n_frames, ped_mask and
 * G2K_STEP_TARGETS_SHARED as g2k_fullcov_stats_f32; coordinate i = 2 t + c;
 * r = target - pred in double.
 *
 * Parameter block: mix [8][608] f32, always 8 slots.  Per slot:
 *   float 0        w
 *   floats 1..7    unused (written as 0, never read)
 *   floats 8..31   b[24], the component's mean offset
 *   floats 32..607 L[24][24] row-major, the component's lower Cholesky
 *                  factor; entries j > i are never read; diagonal > 0 (the
 *                  caller's contract)
 * A slot with w == 0 is dead: never staged, never drawn from, never updated
 * (nothing but its w is read); at least one slot is live and every w >= 0
 * (the caller's contract).
 *
 * Mixture log density of a pair, in double from the f32 parameters, dead
 * slots skipped, max-shifted:
 *   l_m = log(w_m / sum w) - 12 log 2 pi - sum_i log L_m[i][i] - q_m / 2,
 *   q_m = ||L_m^-1 (r - b_m)||^2,   l = logsumexp_m l_m,
 *   gamma_m = exp(l_m - l); the hard assignment is the lowest m that attains
 *   max gamma.
 *
 * One EM step over the n pairs:
 *   N_m = sum gamma_m, s_m = sum gamma_m r, G_m = sum gamma_m r r^T
 *   new w_m = N_m / n, new b_m = s_m / N_m,
 *   C_m = G_m / N_m - b_m b_m^T, C_ii <- C_ii (1 + 1e-6) + 1e-12,
 *   new L_m = chol(C_m) in double, written as f32, zeros above the diagonal
 *   a live slot with N_m < 1 keeps its b and L (lower triangle) and gets
 *   w = N_m / n; n = 0: every live slot keeps w, b and L
 *   a dead slot of mix_in is 608 zeros in mix_out
 *
 * g2k_mix_em_f32: one E-step (and, with mix_out, the M-step).
 *   moments [8][25][24] f64: rows 0..23 = G_m (both triangles written,
 *     equal), row 24 = s_m; zeros for dead slots
 *   resp [8][2] f64 = {N_m, hard count}
 *   total [4] f64 = {pairs, sum l, 0, 0}
 *   mix_out [8][608] f32 or NULL: the new block (floats 1..7 and the entries
 *     above the diagonals are zeros); NULL = the E-step only, the evaluation
 *     of a given mixture: the other outputs' bits do not depend on it
 *   Every element of every output is written on every call with S >= 1;
 *   non-pairs of pred / targets are never read.  mix_out must not overlap
 *   mix_in.  Nmax in 1..256, S F Nmax < 2^31; workspace >=
 *   g2k_mix_em_workspace_bytes(d) (the responsibilities [8][S F Nmax] f64
 *   and the workgroups' rows).  Three launches on the stream, no allocation,
 *   no atomics, fixed summation order: repeated calls are bit-identical.
 * g2k_mix_sample_f32: out [S, F, 2L, Nmax] = one draw per (s, f, n), every
 *   element written; comp [S][F][Nmax] int32 or NULL: the drawn component of
 *   every element.  Stream and element index are g2k_fullcov_sample_f32's.
 *   The selector is drawn once per trajectory from step 0's key:
 *     key0 = stream(e0 >> 32) ^ (uint32)e0,
 *     h = pcg_hash(pcg_hash(key0) + 0x9E3779B9u),
 *     u = ((float)(h >> 8) + 0.5f) / 2^24 (f32),
 *     cw[m] = (float) of the double running sum of (double)w_m / sum w, the
 *     last live slot's cw forced to 1; the component is the first live m with
 *     u < cw[m] (the last live slot when there is none: u rounds to 1 for the
 *     largest h).
 *   The draw: a[i] = mu[i] + b_m[i] (one f32 add), then the steps of
 *   g2k_fullcov_sample_f32 with L_m on the element's normals.  pred may be out
 *   (in place) but must not otherwise overlap it; d->flags must be 0, T = 8,
 *   L = 12.
 * g2k_mix_best_of_k_f32: g2k_fullcov_best_of_k_f32 with mix in place of chol
 *   and these draws: the same per_ped, best (draw kA, bit-identical to
 *   g2k_mix_sample_f32 at seed + kA, for pairs; pred elsewhere) and out, K in
 *   1..4096, no draw in memory, ties to the lowest k.
 * g2k_mix_joint_eval_f32: g2k_fullcov_joint_eval_f32 (include/g2k_hip.h) with
 *   mix in place of chol: the same outputs (per_frame_f [S, F, 4], per_frame_i
 *   [S, F, 6] or NULL, sums_f [S, 4], sums_i [S, 6] int64; zeros where P = 0 or
 *   f >= n_frames[s]; every element written), K in 1..4096, radius finite and
 *   >= 0, workspace >= g2k_mix_joint_eval_workspace_bytes(d).  Draw k of a
 *   member is bit for bit what g2k_mix_sample_f32 writes for seed (seed + k)
 *   mod 2^64.  In joint sample k EVERY MEMBER SELECTS ITS OWN COMPONENT from
 *   its own step-0 key: one joint sample mixes components across the
 *   pedestrians of the scene-frame (the mixture is over a pair's residuals,
 *   not over the scene's).
 * g2k_mix_kde_nll_f32: g2k_fullcov_kde_nll_f32 with mix in place of chol and
 *   these draws: the same per_ped [S, F, Nmax, 4] or NULL and out [S, 8], K in
 *   4..4096, log_floor finite, workspace >= g2k_mix_kde_nll_workspace_bytes(d);
 *   S = 0 or F = 0 launches nothing.  The definition is the same; the fp32
 *   moments of the K draws are taken as a running mean and centred sums (the
 *   draws sit around mu + b_m, not around mu), so a one-slot, b = 0 mixture
 *   agrees with g2k_fullcov_kde_nll_f32 to rounding, not bit for bit.
 * Both: flags, validation, workspace sizes and the S = 0 / F = 0 no-ops are
 *   the full-covariance entry points'; no atomics, repeated calls are
 *   bit-identical; dead slots, floats 1..7 and the entries above the diagonals
 *   are never read.
 * All five: S = 0 is a no-op; asynchronous, no allocation, capturable.
 * Alignment (bytes) of g2k_mix_em_f32: targets 8, moments 8, resp 8, total 8,
 * workspace 8.
 * Alignment (bytes) of g2k_mix_best_of_k_f32: targets 8, per_ped 16,
 * workspace 4.
 * Alignment (bytes) of g2k_mix_joint_eval_f32: targets 8, sums_i 8,
 * workspace 4.
 * Alignment (bytes) of g2k_mix_kde_nll_f32: targets 8, per_ped 16,
 * workspace 4.
 */
#ifndef G2K_MIX_H_
#define G2K_MIX_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_MIX_SLOTS 8
#define G2K_MIX_PITCH 608

int64_t g2k_mix_em_workspace_bytes(const g2k_dims* d);
int g2k_mix_em_f32(const g2k_dims* d, const float* pred, const float* targets,
                   const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                   const float* mix_in, double* moments, double* resp, double* total,
                   float* mix_out, void* workspace, int64_t workspace_bytes, void* stream);
int g2k_mix_sample_f32(const g2k_dims* d, const float* pred, const float* mix, uint64_t seed,
                       float* out, int32_t* comp, void* stream);
int64_t g2k_mix_best_of_k_workspace_bytes(const g2k_dims* d);
int g2k_mix_best_of_k_f32(const g2k_dims* d, const float* pred, const float* targets,
                          const int32_t* n_active, const int32_t* n_frames,
                          const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                          float* per_ped, float* best, float* out, void* workspace,
                          int64_t workspace_bytes, void* stream);
int64_t g2k_mix_joint_eval_workspace_bytes(const g2k_dims* d);
int g2k_mix_joint_eval_f32(const g2k_dims* d, const float* pred, const float* targets,
                           const int32_t* n_active, const int32_t* n_frames,
                           const uint8_t* ped_mask, const float* mix, uint64_t seed, int32_t K,
                           float radius, float* per_frame_f, int32_t* per_frame_i, float* sums_f,
                           int64_t* sums_i, void* workspace, int64_t workspace_bytes, void* stream);
int64_t g2k_mix_kde_nll_workspace_bytes(const g2k_dims* d);
int g2k_mix_kde_nll_f32(const g2k_dims* d, const float* pred, const float* targets,
                        const int32_t* n_active, const int32_t* n_frames, const uint8_t* ped_mask,
                        const float* mix, uint64_t seed, int32_t K, float log_floor, float* per_ped,
                        float* out, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_MIX_H_ */
