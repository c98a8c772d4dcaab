// The finishing launch of the posterior samplers' statistics (posterior.hip, inpaint_posterior.hip, enhance_post.hip): the
// sample tiles' partial sums (sum y, sum y^2), fp64, folded in tile order -> mean and unbiased standard deviation, rounded to
// fp32 once.
#pragma once
#include "common.h"

namespace {

// part [tiles][n], out [n]
__global__ __launch_bounds__(256) void post_finish_kernel(const double2* __restrict__ part, size_t n, int tiles, int S,
                                                          float* __restrict__ mean, float* __restrict__ sd) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    double s1 = 0.0, s2 = 0.0;
    for (int t = 0; t < tiles; ++t) {
      const double2 v = part[(size_t)t * n + e];
      s1 += v.x;
      s2 += v.y;
    }
    const double var = (s2 - s1 * s1 / S) / (S - 1);
    mean[e] = (float)(s1 / S);
    sd[e] = (float)sqrt(var > 0.0 ? var : 0.0);
  }
}

inline void post_finish(const double2* part, size_t n, int tiles, int S, float* mean, float* sd, hipStream_t st) {
  const size_t g = (n + 255) / 256;
  hipLaunchKernelGGL(post_finish_kernel, dim3((unsigned)(g > 2048 ? 2048 : g)), dim3(256), 0, st, part, n, tiles, S, mean, sd);
}

}  // namespace
