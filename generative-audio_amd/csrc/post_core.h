// The per-bin rule of the posterior samplers and the host arithmetic of their sample tiles, shared by the sampler of cut
// clips (posterior.hip) and the sampler of whole recordings (enhance_post.hip): both build a sampled mask with post_mask and
// apply it with cirm_apply_true, so a recording of one chunk and the clip it is give the same bits.
#pragma once
#include "common.h"
#include "fft_core.h"
#include "nppc_hip.h"

namespace {

// mask * noisy, the true complex product, and the magnitude of the result, with the fused multiply-adds that
// decompress_apply_kernel (frontend.hip, conj_mask = 0) compiles to spelled out: left to the compiler, the contraction of
// these sums depends on the code around them, and the sampler at z = 0 has to give that kernel's bits (the tests hold the
// two together).
__device__ __forceinline__ void cirm_apply_true(float mr, float mi, float a, float c, float* xr, float* xi) {
  *xr = __builtin_fmaf(mr, a, -(mi * c));
  *xi = __builtin_fmaf(mr, c, mi * a);
}
__device__ __forceinline__ float spec_mag(float xr, float xi) { return sqrtf(__builtin_fmaf(xr, xr, xi * xi)); }

// the sampled mask of one bin.  pr / pi: the restoration's compressed mask; wr / wi: direction k at wr[k * wstride];
// z: this sample's K (real, imaginary) pairs.
__device__ __forceinline__ void post_mask(float pr, float pi, const float* __restrict__ wr, const float* __restrict__ wi,
                                          size_t wstride, const float* __restrict__ z, int K, int domain, float* Mr,
                                          float* Mi) {
#pragma clang fp contract(off)
  float mr, mi;
  if (domain == NPPC_POST_COMPRESSED) {
    mr = pr;
    mi = pi;
    for (int k = 0; k < K; ++k) {
      const float zr = z[2 * k], zi = z[2 * k + 1];
      const float a = wr[k * wstride], c = wi[k * wstride];
      const float t0 = zr * a, t1 = zi * c, t2 = zr * c, t3 = zi * a;
      const float dr = t0 - t1, di = t2 + t3;
      mr = mr + dr;
      mi = mi + di;
    }
    mr = decompress_cirm(mr);
    mi = decompress_cirm(mi);
  } else {
    mr = decompress_cirm(pr);
    mi = decompress_cirm(pi);
    for (int k = 0; k < K; ++k) {
      const float zr = z[2 * k], zi = z[2 * k + 1];
      const float a = decompress_cirm(wr[k * wstride]), c = decompress_cirm(wi[k * wstride]);
      const float t0 = zr * a, t1 = zi * c, t2 = zr * c, t3 = zi * a;
      const float dr = t0 - t1, di = t2 + t3;
      mr = mr + dr;
      mi = mi + di;
    }
  }
  *Mr = mr;
  *Mi = mi;
}

inline bool post_config_ok(int nfft, int hop) {
  return (nfft == 64 || nfft == 128 || nfft == 256 || nfft == 512) && hop > 0 && nfft % hop == 0 && nfft / hop <= 8;
}

// S samples over sample tiles of a grid whose other dimensions hold `groups` workgroups: NPPC_POST_TILE samples a tile, but
// with statistics (partial sums cost memory per tile) only as many tiles as fill the chip.  -> tiles, *per samples in each
inline long post_tiles(int S, long groups, int stats, int* per) {
  long nt = ceil_div(S, NPPC_POST_TILE);
  if (stats) {
    long fill = ceil_div(NPPC_POST_FILL, groups);
    fill = fill < 1 ? 1 : (fill > NPPC_POST_MAX_STAT_TILES ? NPPC_POST_MAX_STAT_TILES : fill);
    nt = nt < fill ? nt : fill;
  }
  *per = ceil_div(S, nt);
  return ceil_div(S, *per);
}

}  // namespace
