/*
 * g2k_step_fixed.h — which build of the fused step a launch takes, and how
 * many of its workgroups a CU holds (added after ABI 11; detect by symbol:
 * g2k_abi_version() stays 11).  A header of its own, as include/g2k_kin.h: what
 * a binding looks up by name (multimodaltraj_2_amd/frame_step.py
 * step_fixed_geometry).  The kernel is csrc/g2k_scene.hip.
 *
 * The forward step has a build with the frame count as a compile-time
 * constant: F = 20 (obs_len 8 + pred_len 12, the model's own scene length) in
 * one chunk, stride 1.  A launch takes it exactly when
 *   - it is the forward step (not train mode),
 *   - under G2K_STEP_CORESIDENT with the 8-wave geometry in force (H < 512 and
 *     the scene's LDS fits a CU twice: G2K_GEOM_NP = 4),
 *   - d->stride = 1 and d->F = 20,
 *   - one workgroup per scene (G2K_GEOM_SPLIT = 1) and the general variant.
 * Every other launch takes the builds it took before.  The fixed build
 * computes bit for bit what the general build computes; g2k_step_geometry
 * reports the same fields for it (variant "general"), except that its LDS is
 * smaller: its position window shares the space of the attention ring, which
 * g2k_step_lds_bytes and G2K_GEOM_LDS_BYTES report.
 *
 * g2k_step_fixed_geometry: host arithmetic only, no HIP call — the same answer
 * with or without a GPU.  Arguments as g2k_step_geometry (an automatic split is
 * resolved for `cus` compute units).  out[G2K_STEP_FIXED_FIELDS]:
 *   FRAMES      the frame count the build is fixed to (20), or 0: a build with
 *               runtime frames
 *   WGS_PER_CU  workgroups of the launch a CU holds at once: for the fixed
 *               build the times its LDS fits in 160 KiB, at most 3 (24 waves at
 *               <= 80 VGPRs; at most 2 at H = 256, whose build needs 90 VGPRs);
 *               2 for the other 8-wave forward builds; else 1
 *   LDS_BYTES   the workgroup's LDS (= g2k_step_lds_bytes for a forward launch)
 * Returns G2K_OK or what g2k_step_geometry returns for the same arguments.
 */
#ifndef G2K_STEP_FIXED_H_
#define G2K_STEP_FIXED_H_

#include "g2k_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2K_STEP_FIXED_FRAMES 0
#define G2K_STEP_FIXED_WGS_PER_CU 1
#define G2K_STEP_FIXED_LDS_BYTES 2
#define G2K_STEP_FIXED_FIELDS 3

int g2k_step_fixed_geometry(const g2k_dims* d, int32_t train, int32_t has_h_in, int32_t cus,
                            int32_t* out);

#ifdef __cplusplus
}
#endif

#endif  /* G2K_STEP_FIXED_H_ */
