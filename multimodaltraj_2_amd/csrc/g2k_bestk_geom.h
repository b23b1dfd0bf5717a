// g2k_bestk_geom.h — the launch geometry that the per-pair sampled evaluations
// share (best_of_k_kernel, g2k_bestk.hip; kde_nll_kernel, g2k_kde.hip): one
// workgroup of 256 threads per (scene, chunk of FC frames), the K draws of a
// pair dealt round-robin to KS = 2^ks_log2 adjacent lanes.  KS and FC come from
// the shapes alone: KS grows until the launch has ~2 * 256 CUs * 1024 items or
// K is used up (KS <= K: every slice has a draw), FC fills the 256 threads.
#pragma once
#include "g2k_common.h"

namespace g2k {
namespace {

constexpr int kBkThreads = 256;
constexpr int64_t kBkFill = 2 * 256 * 1024;   // items that fill 256 CUs twice over
constexpr int kBkMaxSlices = 64;              // one wave: the combine is lane shuffles

struct BestkGeom { int ks_log2, FC, C; };

inline BestkGeom bestk_geom(const g2k_dims& d, int K) {
  const int64_t slots = (int64_t)d.S * d.F * d.Nmax;
  int j = 0;
  while ((2 << j) <= K && (2 << j) <= kBkMaxSlices && (slots << j) < kBkFill) ++j;
  int fc = kBkThreads / (d.Nmax << j);
  if (fc > d.F) fc = d.F;
  if (fc < 1) fc = 1;
  BestkGeom g;
  g.ks_log2 = j;
  g.FC = fc;
  g.C = d.F > 0 ? (d.F + fc - 1) / fc : 1;
  return g;
}

}  // namespace
}  // namespace g2k
