// Ragged (variable-length) inference of the FullSubNet+ restorer (n_maps = 1): a padded batch [B][Lmax] whose item b
// is L_b samples / T_b = 1 + L_b / hop frames long.  Each kernel here is the per-item form of a uniform kernel
// (tcn.hip, subband.hip, frontend.hip's cIRM MSE) whose work decomposition differs from its twin's: it reads an item's
// own length from a device int[B] and computes exactly what the uniform kernel computes for that item run alone.  (The
// ragged STFT / iSTFT and the ragged TSSE front are the RAGGED instantiations of frontend.hip's and spec.hip's own
// kernels.)  Padding past an item's end is never read, and
// what these kernels write past it is zero.  No float atomics: every sum has one writer and a fixed order.
// The uniform GEMMs, the staging and the LSTM run at the batch's longest length.
#include "common.h"
#include "nppc_hip.h"

namespace {

// ---------------------------------------------------------------- TCN depthwise stage (tcn.hip: dwconv_kernel)
// The depthwise conv is CENTRED (padding = dilation): frame t reads t + dil, so the frames of a longer item would leak
// into a shorter one's last frames.  Per item: z = GN1(y1) on frames t < Tv_b = T_b + la, 0 outside; out rows
// t >= Tv_b are 0.  No statistics here: nppc_tcn_gn_stats_ragged computes them from the stored output.
constexpr int RDW_FRAMES = 32;

template <typename TT>
__global__ __launch_bounds__(256) void dwconv_ragged_kernel(const TT* __restrict__ in, TT* __restrict__ out,
                                                            const double* __restrict__ st1, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ wd,
                                                            const float* __restrict__ bd, const float* __restrict__ slope2,
                                                            const int* __restrict__ frames, int la, int Cc, int ld, int Tp,
                                                            int Tv, int dil, float eps, long strideAct, long strideSt,
                                                            long strideP) {
  const int z = blockIdx.z, b = blockIdx.y;
  in += (size_t)z * strideAct;
  out += (size_t)z * strideAct;
  st1 += (size_t)z * strideSt;
  gamma += (size_t)z * strideP; beta += (size_t)z * strideP; bd += (size_t)z * strideP; wd += (size_t)z * strideP;
  const float a2 = slope2[(size_t)z * strideP];
  const int Tvb = clampi(frames[b] + la, 1, Tv);
  const double cnt = (double)Cc * Tv;                  // the sums were rescaled to Tv frames (gn_stats_ragged_kernel)
  const double m = st1[b * 2] / cnt;
  const double var = st1[b * 2 + 1] / cnt - m * m;
  const float mean = (float)m, rstd = (float)(1.0 / sqrt((var > 0 ? var : 0) + (double)eps));
  const int cpr = Cc / 8;
  const int rpi = 256 / cpr;
  const int tl = threadIdx.x / cpr, c8 = (threadIdx.x % cpr) * 8;
  if (tl >= rpi) return;
  float g8[8], be8[8], b8[8], w8[3][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    g8[i] = gamma[c8 + i] * rstd;
    be8[i] = beta[c8 + i] - mean * g8[i];
    b8[i] = bd[c8 + i];
#pragma unroll
    for (int k = 0; k < 3; ++k) w8[k][i] = wd[(c8 + i) * 3 + k];
  }
  const int t1 = min((int)(blockIdx.x + 1) * RDW_FRAMES, Tp);
  for (int t = blockIdx.x * RDW_FRAMES + tl; t < t1; t += rpi) {
    float o[8];
    if (t < Tvb) {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = b8[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int ts = t + (k - 1) * dil;
        if (ts >= 0 && ts < Tvb) {
          float v[8];
          load8<TT>(in + ((size_t)b * Tp + ts) * ld + c8, v);
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] += w8[k][i] * (v[i] * g8[i] + be8[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = o[i] > 0.f ? o[i] : a2 * o[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = 0.f;
    }
    store8<TT>(out + ((size_t)b * Tp + t) * ld + c8, o);
  }
}

// GroupNorm(1, C) statistics of item b from the STORED activation act[z][b][t][c] (the rounded values the uniform kernels
// sum), over its own rows t < Tv_b, rescaled by Tv / Tv_b so the consumers' m = s1 / (C Tv) is the item's own mean.
// One workgroup per (item, branch), fp64 accumulation in a fixed order; the entry replaces whatever the uniform launch added.
template <typename TT>
__global__ __launch_bounds__(1024) void gn_stats_ragged_kernel(const TT* __restrict__ act, double* __restrict__ st,
                                                               const int* __restrict__ frames, int la, int Cc, int ld, int Tp,
                                                               int Tv, long strideAct, long strideSt) {
  __shared__ double red[2][16];
  const int z = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  act += (size_t)z * strideAct + (size_t)b * Tp * ld;
  st += (size_t)z * strideSt + (size_t)b * 2;
  const int Tvb = clampi(frames[b] + la, 1, Tv);
  const int cpr = Cc / 8;
  double s1 = 0.0, s2 = 0.0;
  for (long e = tid; e < (long)Tvb * cpr; e += 1024) {
    const int t = (int)(e / cpr), c8 = (int)(e % cpr) * 8;
    float v[8];
    load8<TT>(act + (size_t)t * ld + c8, v);
    float p1 = 0.f, p2 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { p1 += v[i]; p2 += v[i] * v[i]; }
    s1 += (double)p1;
    s2 += (double)p2;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, q = 0.0;
    for (int w = 0; w < 16; ++w) { a += red[0][w]; q += red[1][w]; }
    const double r = (double)Tv / Tvb;
    st[0] = a * r;
    st[1] = q * r;
  }
}

// ---------------------------------------------------------------- sub-band norm (subband.hip: subband_mean_kernel)
// scale[b] = 1 / (mean over (F, nfeat, Tv_b) of the concatenated sub-band input + 1e-5), one workgroup per item
template <typename TT>
__global__ __launch_bounds__(1024) void subband_mean_ragged_kernel(const TT* __restrict__ src, int ldS, const TT* __restrict__ fb,
                                                                   int ldF, long strideFb, const float* __restrict__ mult,
                                                                   float* __restrict__ scale, const int* __restrict__ frames,
                                                                   int la, int F, int Tp, int Tv, int nfeat) {
  __shared__ double red[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tvb = clampi(frames[b] + la, 1, Tv);
  double s = 0.0;
  for (long e = tid; e < (long)Tvb * F; e += 1024) {
    const int t = (int)(e / F), f = (int)(e % F);
    const size_t row = (size_t)b * Tp + t;
    float v = mult[f] * to_f32<TT>(src[row * ldS + f]);
    v += to_f32<TT>(fb[row * ldF + f]) + to_f32<TT>(fb[strideFb + row * ldF + f]) + to_f32<TT>(fb[2 * strideFb + row * ldF + f]);
    s += (double)v;
  }
  const double tot = block_sum_waves<16>(s, red);
  if (tid == 0) {
    const float mu = (float)(tot / ((double)F * nfeat * Tvb));
    scale[b] = 1.0f / (mu + 1e-5f);
  }
}

// ---------------------------------------------------------------- output crop: x[b][r][t] = 0 for t >= T_b
__global__ __launch_bounds__(256) void crop_frames_kernel(float* __restrict__ x, long rows, int T, const int* __restrict__ frames,
                                                          int B) {
  const size_t total = (size_t)B * rows * T;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int t = (int)(e % T);
    const int b = (int)(e / ((size_t)rows * T));
    if (t >= frames[b]) x[e] = 0.f;
  }
}

// ---------------------------------------------------------------- per-item cIRM MSE (frontend.hip: crm_mse, G = 1)
// loss[b] = mean over [2][F][T_b] of (gt - crm)^2, gt = compress(cIRM(noisy, clean)) with crm_mse's formula; one workgroup
// per item, fixed-order fp64 reduction
__global__ __launch_bounds__(1024) void crm_mse_ragged_kernel(const float* __restrict__ nr, const float* __restrict__ ni,
                                                              const float* __restrict__ cr, const float* __restrict__ ci,
                                                              const float* __restrict__ crm, const int* __restrict__ frames,
                                                              int F, int T, float eps, double* __restrict__ loss) {
  __shared__ double red[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = clampi(frames[b], 1, T);
  const size_t FT = (size_t)F * T;
  double s = 0.0;
  for (long e = tid; e < (long)F * Tb; e += 1024) {
    const int f = (int)(e / Tb), t = (int)(e % Tb);
    const size_t i = ((size_t)b * F + f) * T + t;
    const float a = nr[i], bb = ni[i], c = cr[i], d = ci[i];
    const float den = a * a + bb * bb + eps;
    const float gr = compress_cirm((a * c + bb * d) / den);
    const float gi = compress_cirm((a * d - bb * c) / den);
    const size_t o = (size_t)b * 2 * FT + (size_t)f * T + t;
    const double dr = (double)gr - (double)crm[o], di = (double)gi - (double)crm[o + FT];
    s += dr * dr + di * di;
  }
  const double tot = block_sum_waves<16>(s, red);
  if (tid == 0) {
    loss[b] = tot / (2.0 * F * Tb);
  }
}

}  // namespace

extern "C" {

int nppc_tcn_dwconv_ragged(int prec, const void* in, void* out, const double* st1, const float* gamma, const float* beta,
                           const float* wd, const float* bd, const float* slope2, const int* frames, int la, int B, int Cc, int ld,
                           int Tp, int Tv, int dil, float eps, long sAct, long sSt, long sP, int batch, void* stream) {
  if (!in || !out || !st1 || !frames || B <= 0 || batch <= 0 || Cc % 8 || Cc / 8 > 256 || ld % 8 || Tv > Tp) return NPPC_EBADARG;
  dim3 grid(ceil_div(Tp, RDW_FRAMES), B, batch);
  hipStream_t s = (hipStream_t)stream;
  if (prec == NPPC_PREC_BF16)
    hipLaunchKernelGGL(dwconv_ragged_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)in, (bf16_t*)out, st1, gamma, beta, wd,
                       bd, slope2, frames, la, Cc, ld, Tp, Tv, dil, eps, sAct, sSt, sP);
  else if (prec == NPPC_PREC_F32)
    hipLaunchKernelGGL(dwconv_ragged_kernel<float>, grid, dim3(256), 0, s, (const float*)in, (float*)out, st1, gamma, beta, wd,
                       bd, slope2, frames, la, Cc, ld, Tp, Tv, dil, eps, sAct, sSt, sP);
  else
    return NPPC_EBADARG;
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_tcn_gn_stats_ragged(int prec, const void* act, double* stats, const int* frames, int la, int B, int Cc, int ld, int Tp,
                             int Tv, long sAct, long sSt, int batch, void* stream) {
  if (!act || !stats || !frames || B <= 0 || batch <= 0 || Cc % 8 || ld % 8 || Cc > ld || Tv > Tp) return NPPC_EBADARG;
  hipStream_t s = (hipStream_t)stream;
  if (prec == NPPC_PREC_BF16)
    hipLaunchKernelGGL(gn_stats_ragged_kernel<bf16_t>, dim3(B, batch), dim3(1024), 0, s, (const bf16_t*)act, stats, frames, la, Cc,
                       ld, Tp, Tv, sAct, sSt);
  else if (prec == NPPC_PREC_F32)
    hipLaunchKernelGGL(gn_stats_ragged_kernel<float>, dim3(B, batch), dim3(1024), 0, s, (const float*)act, stats, frames, la, Cc,
                       ld, Tp, Tv, sAct, sSt);
  else
    return NPPC_EBADARG;
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_subband_mean_ragged(int prec, const void* src, int ldS, const void* fb, int ldF, long strideFb, const float* mult,
                             float* scale, const int* frames, int la, int B, int F, int Tp, int Tv, int nfeat, void* stream) {
  if (!src || !fb || !mult || !scale || !frames || B <= 0 || F <= 0 || Tv > Tp || F > ldS || F > ldF) return NPPC_EBADARG;
  hipStream_t s = (hipStream_t)stream;
  if (prec == NPPC_PREC_BF16)
    hipLaunchKernelGGL(subband_mean_ragged_kernel<bf16_t>, dim3(B), dim3(1024), 0, s, (const bf16_t*)src, ldS, (const bf16_t*)fb,
                       ldF, strideFb, mult, scale, frames, la, F, Tp, Tv, nfeat);
  else if (prec == NPPC_PREC_F32)
    hipLaunchKernelGGL(subband_mean_ragged_kernel<float>, dim3(B), dim3(1024), 0, s, (const float*)src, ldS, (const float*)fb, ldF,
                       strideFb, mult, scale, frames, la, F, Tp, Tv, nfeat);
  else
    return NPPC_EBADARG;
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_crop_frames_ragged(float* x, long rows, int T, const int* frames, int B, void* stream) {
  if (!x || !frames || rows <= 0 || T <= 0 || B <= 0) return NPPC_EBADARG;
  const size_t total = (size_t)B * rows * T;
  const int grid = (int)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096);
  hipLaunchKernelGGL(crop_frames_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, rows, T, frames, B);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_crm_mse_ragged(const float* nr, const float* ni, const float* cr, const float* ci, const float* crm, const int* frames,
                        int B, int F, int T, float eps, double* loss, void* stream) {
  if (!nr || !ni || !cr || !ci || !crm || !frames || !loss || B <= 0 || F <= 0 || T <= 0) return NPPC_EBADARG;
  hipLaunchKernelGGL(crm_mse_ragged_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, nr, ni, cr, ci, crm, frames, F, T, eps,
                     loss);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
