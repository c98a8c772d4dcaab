// Ragged-gap variant of the MC-dropout + PCA baseline for gfx950: the items of a batch may have
// different numbers of gap (mask == 0) elements, as the batches of the reference's AudioInpaintingDataset do.  This file
// holds what moves the gap elements in and out of the dense [B][Nmax] rows the PCA works on:
//   * gap_scan_kernel      counts [B] and the row-major positions idx [B][Nmax] of the gap elements (-1 past counts[b]):
//                          one workgroup per item, ballot + block scan, no atomics;
//   * gap_gather_kernel    U-Net output [B][N] -> one slice [B][Nmax] of the MC stack through idx (0 at padded positions);
//   * gap_scatter_kernel   [B][R][Nmax] -> zero-initialised [B][R][N] through idx.
// The ragged PCA itself (nppc_pca_ragged, nppc_pca_ragged_work_elems) is in mc_pca.hip beside the uniform one, whose mean
// and components kernels it shares.
#include "common.h"
#include "nppc_hip.h"

namespace {

// counts (nullable) [B]; idx (nullable) [B][Nmax].  Tiles of 256 elements in row-major order: the position of a gap
// element is (gap elements of earlier tiles) + (of earlier waves of its tile) + (of lower lanes of its wave).
__global__ __launch_bounds__(256) void gap_scan_kernel(const float* __restrict__ mask, int* __restrict__ counts,
                                                       int* __restrict__ idx, long N, int Nmax) {
  __shared__ int wtot[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* mk = mask + (size_t)b * N;
  int* out = idx ? idx + (size_t)b * Nmax : nullptr;
  int base = 0;
  for (long t0 = 0; t0 < N; t0 += 256) {
    const long i = t0 + tid;
    const bool hole = i < N && mk[i] == 0.f;
    const unsigned long long bal = __ballot(hole);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    if (hole && out) {
      const int p = off + __popcll(bal & ((1ull << lane) - 1ull));
      if (p < Nmax) out[p] = (int)i;
    }
    base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (counts && tid == 0) counts[b] = base;
  if (out)
    for (int p = base + tid; p < Nmax; p += 256) out[p] = -1;
}

// out [B][Nmax] = src [B][N] through idx; consecutive threads write consecutive elements
__global__ __launch_bounds__(256) void gap_gather_kernel(const float* __restrict__ src, const int* __restrict__ idx,
                                                         float* __restrict__ out, long N, int Nmax) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= Nmax) return;
  const int i = idx[(size_t)b * Nmax + j];
  out[(size_t)b * Nmax + j] = (i >= 0 && i < N) ? src[(size_t)b * N + i] : 0.f;
}

// out [B][R][N] (zeroed by the caller) <- vals [B][R][Nmax] through idx
__global__ __launch_bounds__(256) void gap_scatter_kernel(const float* __restrict__ vals, const int* __restrict__ idx,
                                                          float* __restrict__ out, int R, long N, int Nmax) {
  const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  if (j >= Nmax) return;
  const int i = idx[(size_t)b * Nmax + j];
  if (i >= 0 && i < N) out[((size_t)b * R + r) * N + i] = vals[((size_t)b * R + r) * Nmax + j];
}

inline bool gap_dims_ok(int B, long N, int Nmax) { return B > 0 && B <= 65535 && N > 0 && N <= 0x7fffffffL && Nmax > 0 && Nmax <= N; }

}  // namespace

extern "C" {

int nppc_gap_count(const float* mask, int* counts, int B, long N, void* stream) {
  if (!mask || !counts || B <= 0 || N <= 0 || N > 0x7fffffffL) return NPPC_EBADARG;
  hipLaunchKernelGGL(gap_scan_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mask, counts, (int*)nullptr, N, 0);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_gap_index(const float* mask, int* idx, int B, long N, int Nmax, void* stream) {
  if (!mask || !idx || !gap_dims_ok(B, N, Nmax)) return NPPC_EBADARG;
  hipLaunchKernelGGL(gap_scan_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mask, (int*)nullptr, idx, N, Nmax);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_gap_gather(const float* src, const int* idx, float* out, int B, long N, int Nmax, void* stream) {
  if (!src || !idx || !out || !gap_dims_ok(B, N, Nmax)) return NPPC_EBADARG;
  hipLaunchKernelGGL(gap_gather_kernel, dim3(ceil_div(Nmax, 256), B), dim3(256), 0, (hipStream_t)stream, src, idx, out, N, Nmax);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_gap_scatter(const float* vals, const int* idx, float* out, int B, int R, long N, int Nmax, void* stream) {
  if (!vals || !idx || !out || !gap_dims_ok(B, N, Nmax) || R <= 0 || R > 65535) return NPPC_EBADARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * R * N, s) != hipSuccess) return NPPC_ELAUNCH;
  hipLaunchKernelGGL(gap_scatter_kernel, dim3(ceil_div(Nmax, 256), R, B), dim3(256), 0, s, vals, idx, out, R, N, Nmax);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
