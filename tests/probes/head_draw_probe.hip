// head_draw_probe.hip — TEST INFRASTRUCTURE ONLY (tests/draw_probe.py compiles
// it, tests/test_draw_probe_gpu.py runs it): the heads' device-side draw
// (csrc/g2k_head_draw.h) at an arbitrary (seed, element), so that the branches
// a member takes when its elements straddle 2^32 can run without the 34 GB of
// pred that an entry point would need to get there.  Not part of the library.
//
// One workgroup of 64 threads stages the head's parameters as the fused
// evaluations do (Head::stage<64>, a barrier, bind); lane i < P then makes one
// draw of the member whose column is cols[i] in the scene-frame whose
// column-0, step-0 element is e_scene, around the means mu[i] (time-major,
// mu[i][2t + c]), and stores step t's coordinates to out[i][2t], out[i][2t + 1].
// For the mixture head comp[i] (when given) is the component selected.
#include <type_traits>

#include "g2k_head_draw.h"

namespace g2k {
namespace {

constexpr int kProbeLanes = 64;

template <class Head>
__global__ __launch_bounds__(kProbeLanes) void probe_kernel(
    const float* __restrict__ params, const float* __restrict__ mu_in, uint32_t lo, uint32_t hi,
    int64_t e_scene, const int* __restrict__ cols, int Nmax, int P, float* __restrict__ out,
    int* __restrict__ comp) {
  __shared__ typename Head::Lds lds;
  const int i = threadIdx.x;
  Head::template stage<kProbeLanes>(params, lds, i);
  __syncthreads();
  if (i >= P) return;
  Head head;
  head.bind(lds);
  const int n = cols[i];
  const int64_t e0 = e_scene + n;
  float mu[kL2];
#pragma unroll
  for (int r = 0; r < kL2; ++r) mu[r] = mu_in[i * kL2 + r];
  float* o = out + i * kL2;
  head.draw(lo, hi, e0, n, Nmax, mu, [o](int t, float x, float y) {
    o[2 * t] = x;
    o[2 * t + 1] = y;
  });
  if constexpr (std::is_same<Head, MixHead>::value) {
    if (comp) comp[i] = head.select(lo, hi, e0);
  }
}

template <class Head>
int launch(const float* params, const float* mu, uint64_t seed, int64_t e_scene, const int* cols,
           int Nmax, int P, float* out, int* comp, hipStream_t stream) {
  hipLaunchKernelGGL(probe_kernel<Head>, dim3(1), dim3(kProbeLanes), 0, stream, params, mu,
                     (uint32_t)seed, (uint32_t)(seed >> 32), e_scene, cols, Nmax, P, out, comp);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace g2k

// which: 0 per-step (params = head [3][12]), 1 full covariance (chol [24][24]),
// 2 mixture (mix [8][608]), 3 scene-coupled (cpl [2][24][24]).  0 on success,
// -1 for arguments outside the probe's domain, else the launch's hipError_t.
extern "C" int head_draw_probe(int which, const float* params, const float* mu, uint64_t seed,
                               int64_t e_scene, const int* cols, int Nmax, int P, float* out,
                               int* comp, void* stream) {
  using namespace g2k;
  if (!params || !mu || !cols || !out || P < 0 || P > kProbeLanes || Nmax < 1 || Nmax > kMaxN ||
      e_scene < 0)
    return -1;
  if (P == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  switch (which) {
    case 0: return launch<PerStepHead>(params, mu, seed, e_scene, cols, Nmax, P, out, nullptr, s);
    case 1: return launch<FullCovHead>(params, mu, seed, e_scene, cols, Nmax, P, out, nullptr, s);
    case 2: return launch<MixHead>(params, mu, seed, e_scene, cols, Nmax, P, out, comp, s);
    case 3: return launch<CoupledHead>(params, mu, seed, e_scene, cols, Nmax, P, out, nullptr, s);
  }
  return -1;
}
