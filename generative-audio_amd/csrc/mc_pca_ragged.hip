// Ragged-gap variant of the MC-dropout + PCA baseline for gfx950: the items of a batch may have
// different numbers of gap (mask == 0) elements, as the batches of the reference's AudioInpaintingDataset do.
//   * gap_scan_kernel      counts [B] and the row-major positions idx [B][Nmax] of the gap elements (-1 past counts[b]):
//                          one workgroup per item, ballot + block scan, no atomics;
//   * gap_gather_kernel    U-Net output [B][N] -> one slice [B][Nmax] of the MC stack through idx (0 at padded positions);
//   * ragged PCA           mean -> per-chunk partial Grams (each workgroup STORES its chunk's upper triangle) -> sum of an
//                          item's partials in ascending chunk order -> Jacobi (pca_eigh.h) -> components over counts[b]
//                          elements, zeros at padded positions;
//   * gap_scatter_kernel   [B][R][Nmax] -> zero-initialised [B][R][N] through idx.
// Chunks start at element 0 of the item and hold PCR_CH elements, so what is summed for item b, and in which order, is
// a function of that item alone: item b of a batch equals, bit for bit, the same call on that item alone, and two runs
// agree bit for bit.  HBM-bound like mc_pca.hip: every MC sample is read three times (mean, Gram, components).
#include "common.h"
#include "nppc_hip.h"
#include "pca_eigh.h"

namespace {

constexpr int PCR_CH = 64;                               // elements per Gram chunk (the uniform path's PCA_CH)

__device__ __forceinline__ int item_count(const int* __restrict__ counts, int b, int Nmax) {
  const int c = counts[b];
  return c < 0 ? 0 : (c > Nmax ? Nmax : c);              // a count the caller sized no room for is never followed
}

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

// X [K][B][Nmax]; mean [B][Nmax], 0 past counts[b]
__global__ __launch_bounds__(256) void pcr_mean_kernel(const float* __restrict__ X, const int* __restrict__ counts,
                                                       float* __restrict__ mean, int K, int B, int Nmax) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= Nmax) return;
  float m = 0.f;
  if (j < item_count(counts, b, Nmax)) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += (double)X[((size_t)k * B + b) * Nmax + j];
    m = (float)(s / K);
  }
  mean[(size_t)b * Nmax + j] = m;
}

// upper-triangle entry e of a K x K matrix, row-major over (i, j >= i)
__device__ __forceinline__ void tri_entry(int e, int K, int* i, int* j) {
  int r = 0;
  while (e >= K - r) { e -= K - r; ++r; }
  *i = r;
  *j = r + e;
}

// part[b][chunk][e] = sum_{d in chunk} xc[i][d] * xc[j][d] for the K (K + 1) / 2 entries e = (i, j >= i);
// xc = float(X - mean) as scikit-learn centres in the input dtype, 0 past counts[b].  Chunks past the item's end return.
__global__ __launch_bounds__(256) void pcr_gram_partial_kernel(const float* __restrict__ X, const float* __restrict__ mean,
                                                               const int* __restrict__ counts, double* __restrict__ part,
                                                               int K, int B, int Nmax, int nch) {
  __shared__ float xc[PCA_KMAX][PCR_CH + 1];
  const int b = blockIdx.y, chunk = blockIdx.x, d0 = chunk * PCR_CH, tid = threadIdx.x;
  const int D = item_count(counts, b, Nmax);
  if (d0 >= D) return;
  for (int e = tid; e < K * PCR_CH; e += 256) {
    const int k = e / PCR_CH, j = e % PCR_CH, d = d0 + j;
    xc[k][j] = d < D ? X[((size_t)k * B + b) * Nmax + d] - mean[(size_t)b * Nmax + d] : 0.f;
  }
  __syncthreads();
  const int tri = K * (K + 1) / 2;
  double* pr = part + ((size_t)b * nch + chunk) * tri;
  for (int e = tid; e < tri; e += 256) {
    int i, j;
    tri_entry(e, K, &i, &j);
    double s = 0.0;
#pragma unroll 8
    for (int d = 0; d < PCR_CH; ++d) s += (double)xc[i][d] * (double)xc[j][d];
    pr[e] = s;
  }
}

// G[b] = sum of the item's partials in ascending chunk order (both triangles written)
__global__ __launch_bounds__(256) void pcr_gram_reduce_kernel(const double* __restrict__ part, const int* __restrict__ counts,
                                                              double* __restrict__ G, int K, int Nmax, int nch) {
  const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, tri = K * (K + 1) / 2;
  if (e >= tri) return;
  const int used = (item_count(counts, b, Nmax) + PCR_CH - 1) / PCR_CH;
  const double* pr = part + (size_t)b * nch * tri + e;
  double s = 0.0;
  for (int c = 0; c < used; ++c) s += pr[(size_t)c * tri];
  int i, j;
  tri_entry(e, K, &i, &j);
  G[((size_t)b * K + i) * K + j] = s;
  G[((size_t)b * K + j) * K + i] = s;
}

// pca_components_kernel (mc_pca.hip) over the item's own counts[b] elements of rows of Nmax: the same sums and the same
// sign rule (largest-magnitude entry positive, lowest index among equals); zeros past counts[b].
__global__ __launch_bounds__(256) void pcr_components_kernel(const float* __restrict__ X, const float* __restrict__ mean,
                                                             const int* __restrict__ counts, const double* __restrict__ eval,
                                                             const double* __restrict__ evec, float* __restrict__ comps,
                                                             float* __restrict__ scaled, float* __restrict__ svals,
                                                             float* __restrict__ weights, int K, int B, int Nmax, int n) {
  __shared__ double u[PCA_KMAX];
  __shared__ float bestv[4];
  __shared__ int besti[4];
  __shared__ float sgn;
  const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = item_count(counts, b, Nmax);
  const double lam = eval[(size_t)b * n + i];
  const double s = lam > 0.0 ? sqrt(lam) : 0.0;
  for (int k = tid; k < K; k += 256) u[k] = evec[((size_t)b * n + i) * K + k];
  __syncthreads();
  const double inv = s > 0.0 ? 1.0 / s : 0.0;
  float* cv = comps + ((size_t)b * n + i) * Nmax;
  float bv = -1.f;
  int bi = 0x7fffffff;
  for (int d = tid; d < D; d += 256) {
    double a = 0.0;
    const float m = mean[(size_t)b * Nmax + d];
    for (int k = 0; k < K; ++k) a += u[k] * (double)(X[((size_t)k * B + b) * Nmax + d] - m);
    const float v = (float)(a * inv);
    cv[d] = v;
    if (fabsf(v) > bv) { bv = fabsf(v); bi = d; }              // ascending d per thread: first index kept on ties
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { bestv[wave] = bv; besti[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (bestv[w] > bv || (bestv[w] == bv && besti[w] < bi)) { bv = bestv[w]; bi = besti[w]; }
    sgn = (bi < D && cv[bi] < 0.f) ? -1.f : 1.f;
    double tot = 0.0;
    for (int j = 0; j < n; ++j) { const double l = eval[(size_t)b * n + j]; tot += l > 0.0 ? sqrt(l) : 0.0; }
    svals[(size_t)b * n + i] = (float)s;
    weights[(size_t)b * n + i] = (float)(s / tot);
  }
  __syncthreads();
  const float sg = sgn, sf = (float)s;
  float* sc = scaled + ((size_t)b * n + i) * Nmax;
  for (int d = tid; d < Nmax; d += 256) {
    const float v = d < D ? cv[d] * sg : 0.f;
    cv[d] = v;
    sc[d] = v * sf;
  }
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

int nppc_pca_ragged_work_elems(int K, int B, int Nmax, int n, long* elems) {
  if (!elems || K <= 0 || B <= 0 || Nmax <= 0 || n <= 0) return NPPC_EBADARG;
  const long tri = (long)K * (K + 1) / 2;
  *elems = (long)B * ((long)K * K + n + (long)n * K + (long)ceil_div(Nmax, PCR_CH) * tri);
  return NPPC_OK;
}

int nppc_pca_ragged(const float* X, const int* counts, int K, int B, int Nmax, int n, float* mean, float* comps, float* scaled,
                    float* svals, float* weights, double* work, void* stream) {
  if (!X || !counts || !mean || !comps || !scaled || !svals || !weights || !work || B <= 0 || B > 65535 || Nmax <= 0 || n <= 0)
    return NPPC_EBADARG;
  if (K < 2 || K > PCA_KMAX || n > K || n > 8) return NPPC_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int nch = ceil_div(Nmax, PCR_CH), tri = K * (K + 1) / 2;
  double* G = work;
  double* eval = G + (size_t)B * K * K;
  double* evec = eval + (size_t)B * n;
  double* part = evec + (size_t)B * n * K;
  hipLaunchKernelGGL(pcr_mean_kernel, dim3(ceil_div(Nmax, 256), B), dim3(256), 0, s, X, counts, mean, K, B, Nmax);
  hipLaunchKernelGGL(pcr_gram_partial_kernel, dim3(nch, B), dim3(256), 0, s, X, mean, counts, part, K, B, Nmax, nch);
  hipLaunchKernelGGL(pcr_gram_reduce_kernel, dim3(ceil_div(tri, 256), B), dim3(256), 0, s, part, counts, G, K, Nmax, nch);
  hipLaunchKernelGGL(pca_eigh_kernel, dim3(B), dim3(256), 0, s, G, eval, evec, K, n);
  hipLaunchKernelGGL(pcr_components_kernel, dim3(n, B), dim3(256), 0, s, X, mean, counts, eval, evec, comps, scaled, svals,
                     weights, K, B, Nmax, n);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
