// Masked spectral MSE of the inpainting restorer trainer (restoration_trainer.py:189-191) for gfx950:
//   loss = sum_{b,f,t} (out - clean)^2 (1 - m[b,t]) / (F sum_{b,t} (1 - m[b,t]) + 1e-6)
// out, clean [B][F][T] fp32 (the [B,1,F,T] maps), m [B][T] fp32 (1 = known frame), broadcast over F.
// Deterministic without float atomics: a fixed grid of MSE_BLOCKS workgroups writes fp64 partials (grid-stride over the
// elements, so the assignment does not depend on the device), one workgroup folds them in a fixed tree order.
// The backward reads the incoming gradient from device memory: dout = 2 g (out - clean) (1 - m) / den.
#include "common.h"
#include "nppc_hip.h"

namespace {

constexpr int MSE_BLOCKS = 256;
constexpr int MSE_WORK = 2 * MSE_BLOCKS + 2;     // partials (num, den), then den (+1e-6) and num of the finished sum

__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[256]) {
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  a = red[0][0];
  b = red[1][0];
}

__global__ __launch_bounds__(256) void masked_mse_part_kernel(const float* __restrict__ out, const float* __restrict__ clean,
                                                              const float* __restrict__ m, long N, int FT, int T,
                                                              double* __restrict__ work) {
  __shared__ double red[2][256];
  double num = 0.0, den = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < N; e += (long)MSE_BLOCKS * 256) {
    const long b = e / FT;
    const int t = (int)(e % T);
    const double om = 1.0 - (double)m[b * T + t];
    const double d = (double)out[e] - (double)clean[e];
    num += d * d * om;
    den += om;
  }
  block_sum2(num, den, red);
  if (threadIdx.x == 0) {
    work[blockIdx.x] = num;
    work[MSE_BLOCKS + blockIdx.x] = den;
  }
}

__global__ __launch_bounds__(256) void masked_mse_finish_kernel(double* __restrict__ work, float* __restrict__ loss) {
  __shared__ double red[2][256];
  double num = work[threadIdx.x], den = work[MSE_BLOCKS + threadIdx.x];     // MSE_BLOCKS == 256: one partial per thread
  block_sum2(num, den, red);
  if (threadIdx.x == 0) {
    den += 1e-6;
    work[2 * MSE_BLOCKS] = den;
    work[2 * MSE_BLOCKS + 1] = num;
    *loss = (float)(num / den);
  }
}

__global__ __launch_bounds__(256) void masked_mse_bwd_kernel(const float* __restrict__ out, const float* __restrict__ clean,
                                                             const float* __restrict__ m, const float* __restrict__ g,
                                                             const double* __restrict__ work, float* __restrict__ dout, long N,
                                                             int FT, int T) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  const float coef = (float)(2.0 * (double)*g / work[2 * MSE_BLOCKS]);
  const long b = e / FT;
  const int t = (int)(e % T);
  dout[e] = coef * (out[e] - clean[e]) * (1.f - m[b * T + t]);
}

}  // namespace

extern "C" {

int nppc_masked_mse_work_elems(long* elems) {
  if (!elems) return NPPC_EBADARG;
  *elems = MSE_WORK;
  return NPPC_OK;
}

int nppc_masked_mse(const float* out, const float* clean, const float* mask, int B, int F, int T, double* work, float* loss,
                    void* stream) {
  if (!out || !clean || !mask || !work || !loss || B <= 0 || F <= 0 || T <= 0) return NPPC_EBADARG;
  if ((long)F * T >= (1L << 31)) return NPPC_EUNSUPPORTED;
  const long N = (long)B * F * T;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(masked_mse_part_kernel, dim3(MSE_BLOCKS), dim3(256), 0, s, out, clean, mask, N, F * T, T, work);
  hipLaunchKernelGGL(masked_mse_finish_kernel, dim3(1), dim3(256), 0, s, work, loss);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_masked_mse_bwd(const float* out, const float* clean, const float* mask, const float* g, const double* work,
                        float* dout, int B, int F, int T, void* stream) {
  if (!out || !clean || !mask || !g || !work || !dout || B <= 0 || F <= 0 || T <= 0) return NPPC_EBADARG;
  if ((long)F * T >= (1L << 31)) return NPPC_EUNSUPPORTED;
  const long N = (long)B * F * T;
  if ((N + 255) / 256 >= (1L << 31)) return NPPC_EUNSUPPORTED;
  hipLaunchKernelGGL(masked_mse_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, clean,
                     mask, g, work, dout, N, F * T, T);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
