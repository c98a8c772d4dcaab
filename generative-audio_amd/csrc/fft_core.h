// Radix-2 transform in LDS, the overlap-add of the centred inverse STFT and the cIRM decompression, shared by the front end
// (frontend.hip: stft_kernel, istft_kernel, decompress_apply_kernel) and the posterior samplers (posterior.hip,
// enhance_post.hip).  The sampler at z = 0 has to equal decompress + iSTFT bit for bit; it does because both call these, so
// the order of the operations below is a contract.  (stft_core.h holds the any-N helpers.)
#pragma once
#include "common.h"

// tw[i] = exp(sign 2 pi i / N) and the periodic hann window, generated in fp64 -> fp32 once per workgroup
template <int LOGN>
__device__ __forceinline__ void fft_tables(float2* tw, float* win, double sign) {
  constexpr int N = 1 << LOGN;
  for (int i = threadIdx.x; i < N / 2; i += 256) {
    double s, c;
    sincospi(sign * 2.0 * i / N, &s, &c);
    tw[i] = make_float2((float)c, (float)s);
  }
  for (int i = threadIdx.x; i < N; i += 256) win[i] = (float)(0.5 - 0.5 * cospi(2.0 * i / N));
}

// DIT butterfly stages over nfr rows loaded in bit-reversed order; ends on a barrier
template <int LOGN>
__device__ __forceinline__ void fft_stages(float2 (*buf)[(1 << LOGN) + 1], const float2* tw, int nfr) {
  constexpr int N = 1 << LOGN;
#pragma unroll 1
  for (int s = 0; s < LOGN; ++s) {
    const int half = 1 << s;
    for (int e = threadIdx.x; e < nfr * (N / 2); e += 256) {
      const int j = e / (N / 2), k = e % (N / 2);
      const int grp = k >> s, pos = k & (half - 1);
      const int i0 = (grp << (s + 1)) + pos, i1 = i0 + half;
      const float2 w = tw[pos << (LOGN - 1 - s)];
      const float2 a = buf[j][i0], c = buf[j][i1];
      const float xr = c.x * w.x - c.y * w.y, xi = c.x * w.y + c.y * w.x;
      buf[j][i0] = make_float2(a.x + xr, a.y + xi);
      buf[j][i1] = make_float2(a.x - xr, a.y - xi);
    }
    __syncthreads();
  }
}

// workgroup = ISTFT_FR * hop consecutive output samples of one clip
constexpr int ISTFT_FR = 4;
constexpr int ISTFT_MAXFR = ISTFT_FR + 7;        // frames a workgroup inverts at most: supports hop >= N/8

// padded-coordinate sample p of the inverse STFT from the nfr transformed frames tfirst .. in buf (frames outside
// 0 .. Tb - 1 do not count): sum_t w x_t / N over sum_t w^2, 0 where the envelope is below 1e-11
template <int LOGN>
__device__ __forceinline__ float istft_ola(const float2 (*buf)[(1 << LOGN) + 1], const float* win, int p, int tfirst, int nfr,
                                           int Tb, int hop) {
  constexpr int N = 1 << LOGN;
  float num = 0.f, den = 0.f;
  for (int j = 0; j < nfr; ++j) {
    const int t = tfirst + j;
    const int off = p - t * hop;
    if (t >= 0 && t < Tb && off >= 0 && off < N) {
      const float w = win[off];
      num += w * buf[j][off].x * (1.0f / N);
      den += w * w;
    }
  }
  return den > 1e-11f ? num / den : 0.f;
}

// decompress_cIRM of mask.py:57-60
__device__ __forceinline__ float decompress_cirm(float m) {
  m = fminf(fmaxf(m, -9.9f), 9.9f);
  return -10.f * logf((10.f - m) / (10.f + m));
}
