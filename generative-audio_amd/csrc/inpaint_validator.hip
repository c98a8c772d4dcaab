// Validation side of the inpainting sibling ("Inpainting validator"):
//   nppc_istft_any           torch.istft(center=True, periodic hann, win_length = n_fft) for ANY n_fft <= 512
//   nppc_pc_variation_waves  save_pc_audio_variations (inpainting/validator/validator_nppc_model.py:553-619): the K x A
//                            waveforms prediction + alpha * PC_k and the clean waveform, spectra formed in LDS only
//   nppc_metrics_batch       the (2n + 3) x (2n + 3) Gram matrix behind compute_metrics (:742-828) of every item, one launch
// The inverse transform is the mirror image of stft_dft_kernel (frontend.hip): direct DFT out of LDS, twiddles
// exp(+2 pi i j / N) tabulated in fp64 and indexed by (k n) mod N in integers, fp64 accumulation.  One workgroup owns
// IS_S consecutive output samples of one item; a thread owns one sample and GATHERS the <= ceil(N / hop) frames that cover
// it in ascending frame order: no atomics, the same thread does the same sums whatever the batch.
#include "common.h"
#include "istft_any_core.h"
#include "nppc_hip.h"
#include "stft_core.h"

#include <math.h>

namespace {

using namespace nppc_isany;   // IS_S, IstftGeom, frame_range, gather_sample, istft_geom (istft_any_core.h)

__global__ __launch_bounds__(IS_S) void istft_any_kernel(const float* __restrict__ re, const float* __restrict__ im, long sb,
                                                         float* __restrict__ out, long ld, IstftGeom g) {
  extern __shared__ double2 is_lds[];
  double2* tw = is_lds;
  float2* spec = reinterpret_cast<float2*>(is_lds + g.N);
  const int tid = threadIdx.x, b = blockIdx.y;
  const int o0 = blockIdx.x * IS_S;                           // first output sample of this workgroup
  const int p0 = o0 + g.N / 2;
  const int pend = (o0 + IS_S < g.Lk ? o0 + IS_S : g.Lk) + g.N / 2;
  float* orow = out + (size_t)b * ld;
  if (pend <= p0) {                                           // wholly past the overlap-add: the zero-filled tail
    if (o0 + tid < g.L) orow[o0 + tid] = 0.f;
    return;
  }
  int t_lo, t_hi;
  frame_range(g, p0, pend, &t_lo, &t_hi);
  dft_twiddles(tw, g.N, IS_S);
  const int nt = t_hi - t_lo + 1;
  const float* rb = re + (size_t)b * sb;
  const float* ib = im + (size_t)b * sb;
  for (int e = tid; e < nt * g.F; e += IS_S) {
    const int k = e / nt, j = e % nt;
    const size_t o = (size_t)k * g.T + t_lo + j;
    spec[j * g.F + k] = make_float2(rb[o], ib[o]);
  }
  __syncthreads();
  const int o = o0 + tid;
  if (o >= g.L) return;
  orow[o] = o < g.Lk ? gather_sample(g, tw, spec, t_lo, t_hi, o + g.N / 2) : 0.f;
}

// blockIdx.y = variation: v < K * A -> direction v / A, alpha v % A; v == K * A -> the clean waveform
__global__ __launch_bounds__(IS_S) void pc_variation_kernel(const float* __restrict__ pred, const float* __restrict__ pc,
                                                            const float* __restrict__ clean_norm,
                                                            const float* __restrict__ clean_spec,
                                                            const float* __restrict__ mean_p, const float* __restrict__ std_p,
                                                            const float* __restrict__ alphas, float* __restrict__ out,
                                                            float* __restrict__ clean_wave, int K, int A, IstftGeom g) {
  extern __shared__ double2 is_lds[];
  double2* tw = is_lds;
  float2* spec = reinterpret_cast<float2*>(is_lds + g.N);
  const int tid = threadIdx.x, v = blockIdx.y, b = blockIdx.z;
  const int o0 = blockIdx.x * IS_S;
  const int p0 = o0 + g.N / 2;
  const int pend = (o0 + IS_S < g.Lk ? o0 + IS_S : g.Lk) + g.N / 2;
  const bool is_clean = v == K * A;
  float* orow = is_clean ? clean_wave + (size_t)b * g.L : out + ((size_t)b * K * A + v) * g.L;
  if (pend <= p0) {
    if (o0 + tid < g.L) orow[o0 + tid] = 0.f;
    return;
  }
  int t_lo, t_hi;
  frame_range(g, p0, pend, &t_lo, &t_hi);
  dft_twiddles(tw, g.N, IS_S);
  const int nt = t_hi - t_lo + 1;
  const size_t FT = (size_t)g.F * g.T;
  const double mean = (double)*mean_p, sd = (double)*std_p;
  const float* base = is_clean ? clean_norm + b * FT : pred + b * FT;
  const float* dir = is_clean ? nullptr : pc + ((size_t)b * K + v / A) * FT;
  const double alpha = is_clean ? 0.0 : (double)alphas[v % A];
  const float* cr = clean_spec + (size_t)b * 2 * FT;
  const float* ci = cr + FT;
  for (int e = tid; e < nt * g.F; e += IS_S) {
    const int k = e / nt, j = e % nt;
    const size_t o = (size_t)k * g.T + t_lo + j;
    const double xr = (double)cr[o], xi = (double)ci[o];
    const double h = sqrt(xr * xr + xi * xi);
    // angle(0 + 0i) = 0; atan2 of signed zeros: a real part of -0 gives +-pi, i.e. (-1, 0)
    const double ur = h > 0.0 ? xr / h : (signbit(xr) ? -1.0 : 1.0), ui = h > 0.0 ? xi / h : 0.0;
    double mag;
    if (is_clean)
      mag = exp((double)base[o] * sd + mean) - 1e-6;          // :557-558
    else
      mag = exp(((double)base[o] + alpha * (double)dir[o]) * sd + mean);   // :608-610: no 1e-6 here
    spec[j * g.F + k] = make_float2((float)(mag * ur), (float)(mag * ui));
  }
  __syncthreads();
  const int o = o0 + tid;
  if (o >= g.L) return;
  orow[o] = o < g.Lk ? gather_sample(g, tw, spec, t_lo, t_hi, o + g.N / 2) : 0.f;
}

// ------------------------------------------------------------------------------------------------ batched metrics
// Row r of item b: r < n NPPC direction, r < 2n MC-dropout direction, then the three error rows of nppc_metric_rows
// (formed in fp32 exactly as that kernel stores them).  Workgroup (i, b) owns row i of G_b: every thread strides over N
// with R running sums, folded across the wave by the xor butterfly and across the four waves in a fixed order.
template <int NDIR>
__global__ __launch_bounds__(256) void metrics_gram_kernel(const float* __restrict__ nppc, const float* __restrict__ mc,
                                                           const float* __restrict__ pred, const float* __restrict__ clean,
                                                           const float* __restrict__ mean, const float* __restrict__ mask,
                                                           double* __restrict__ G, long N) {
  constexpr int R = 2 * NDIR + 3;
  __shared__ double red[4][R];
  const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* wn = nppc + (size_t)b * NDIR * N;
  const float* wm = mc + (size_t)b * NDIR * N;
  const float* pr = pred + (size_t)b * N;
  const float* cl = clean + (size_t)b * N;
  const float* mn = mean + (size_t)b * N;
  const float* mk = mask + (size_t)b * N;
  double acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.0;
  for (long k = tid; k < N; k += 256) {
    float v[R];
#pragma unroll
    for (int j = 0; j < NDIR; ++j) {
      v[j] = wn[(size_t)j * N + k];
      v[NDIR + j] = wm[(size_t)j * N + k];
    }
    const float hole = mk[k] == 0.f ? 1.f : 0.f;
    const float e = pr[k] - cl[k];
    v[2 * NDIR] = e;
    v[2 * NDIR + 1] = e * hole;
    v[2 * NDIR + 2] = (mn[k] - cl[k]) * hole;
    float vi = 0.f;
#pragma unroll
    for (int j = 0; j < R; ++j) vi = j == i ? v[j] : vi;      // select, not an indexed register array
    const double di = (double)vi;
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] += di * (double)v[j];
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const double s = wave_sum(acc[j]);
    if ((tid & 63) == 0) red[tid >> 6][j] = s;
  }
  __syncthreads();
  if (tid < R) G[((size_t)b * R + i) * R + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

}  // namespace

extern "C" {

int nppc_istft_any(const float* re, const float* im, long sb, float* out, long ld, int B, int T, int nfft, int hop, int L,
                   void* stream) {
  if (!re || !im || !out || B <= 0 || B > 65535 || ld < L) return NPPC_EBADARG;
  IstftGeom g;
  size_t lds;
  const int rc = istft_geom(T, nfft, hop, L, &g, &lds);
  if (rc != NPPC_OK) return rc;
  if (sb < (long)g.F * T) return NPPC_EBADARG;
  hipLaunchKernelGGL(istft_any_kernel, dim3(ceil_div(L, IS_S), B), dim3(IS_S), lds, (hipStream_t)stream, re, im, sb, out, ld, g);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_pc_variation_waves(const float* pred, const float* pc, const float* clean_norm, const float* clean_spec,
                            const float* mean, const float* stdev, const float* alphas, float* out, float* clean_wave, int B,
                            int K, int A, int T, int nfft, int hop, int L, void* stream) {
  if (!pred || !pc || !clean_norm || !clean_spec || !mean || !stdev || !alphas || !out || !clean_wave || B <= 0 || B > 65535 ||
      K <= 0 || A <= 0 || (long)K * A + 1 > 65535)
    return NPPC_EBADARG;
  IstftGeom g;
  size_t lds;
  const int rc = istft_geom(T, nfft, hop, L, &g, &lds);
  if (rc != NPPC_OK) return rc;
  hipLaunchKernelGGL(pc_variation_kernel, dim3(ceil_div(L, IS_S), K * A + 1, B), dim3(IS_S), lds, (hipStream_t)stream, pred, pc,
                     clean_norm, clean_spec, mean, stdev, alphas, out, clean_wave, K, A, g);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_metrics_batch(const float* nppc, const float* mc, const float* pred, const float* clean, const float* mean,
                       const float* mask, double* G, int B, int n, long N, void* stream) {
  if (!nppc || !mc || !pred || !clean || !mean || !mask || !G || B <= 0 || B > 65535 || n <= 0 || N <= 0) return NPPC_EBADARG;
  if (n > 8) return NPPC_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
#define NPPC_MG(ND)                                                                                                   \
  case ND:                                                                                                            \
    hipLaunchKernelGGL(metrics_gram_kernel<ND>, dim3(2 * ND + 3, B), dim3(256), 0, s, nppc, mc, pred, clean, mean, mask, G, N); \
    break;
  switch (n) {
    NPPC_MG(1) NPPC_MG(2) NPPC_MG(3) NPPC_MG(4) NPPC_MG(5) NPPC_MG(6) NPPC_MG(7) NPPC_MG(8)
  }
#undef NPPC_MG
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
