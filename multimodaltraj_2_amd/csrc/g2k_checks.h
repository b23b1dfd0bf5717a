// g2k_checks.h — the argument checks that the validators of the sampled
// evaluations have word for word in common (g2k_bestk.hip, g2k_joint.hip,
// g2k_kde.hip, g2k_scores.hip, g2k_modes.hip), one inline function each.  Host
// only, before any HIP call.  Each returns G2K_OK or what set_err returns, so
// a validator is a sequence of
//   if (const int rc = check_...(...)) return rc;
// between its own checks, in the order its entry point reports faults.
#pragma once
#include <initializer_list>

#include "g2k_common.h"

namespace g2k {
namespace {

inline int check_dims(const g2k_dims* d) {
  if (!d) return set_err(G2K_EINVAL, "dims is NULL");
  return G2K_OK;
}

// the sizes of an evaluation over the pairs; T and L are not looked at
inline bool pair_sizes_ok(const g2k_dims* d) {
  return d->S >= 0 && d->F >= 0 && d->Nmax >= 1 && d->Nmax <= kMaxN;
}

inline int check_pair_sizes(const g2k_dims* d) {
  if (!pair_sizes_ok(d)) return set_err(G2K_EINVAL, "S=%d F=%d Nmax=%d", d->S, d->F, d->Nmax);
  return G2K_OK;
}

inline int check_required(std::initializer_list<const void*> buffers) {
  for (const void* p : buffers)
    if (!p) return set_err(G2K_EINVAL, "a required buffer pointer is NULL");
  return G2K_OK;
}

// float2 reads
inline int check_targets(const void* targets) {
  if (((uintptr_t)targets) & 7) return set_err(G2K_EINVAL, "targets must be 8-byte aligned");
  return G2K_OK;
}

// float4 stores; the optional output may be NULL
inline int check_per_ped(const void* per_ped) {
  if (((uintptr_t)per_ped) & 15) return set_err(G2K_EINVAL, "per_ped must be 16-byte aligned");
  return G2K_OK;
}

// The workgroups' rows (`align` = the bytes of their element): a workspace
// that is named is held to it, an empty batch's too; with S > 0 it must be
// there and hold `need` bytes.
inline int check_workspace(const g2k_dims* d, const void* workspace, int64_t workspace_bytes,
                           int64_t need, int align, const char* suffix = "") {
  if (workspace && (((uintptr_t)workspace) & (uintptr_t)(align - 1)))
    return set_err(G2K_EINVAL, "workspace must be %d-byte aligned", align);
  if (d->S > 0 && (!workspace || workspace_bytes < need))
    return set_err(G2K_EINVAL, "workspace of %lld bytes needed (got %lld)%s", (long long)need,
                   (long long)workspace_bytes, suffix);
  return G2K_OK;
}

}  // namespace
}  // namespace g2k
